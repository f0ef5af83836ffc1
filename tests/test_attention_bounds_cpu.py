"""The per-element attention bounds of tests/attention_bounds.py, proved on the CPU before any kernel is held to them: the clean rounding
model (the kernels' arithmetic in float64 with their 16-bit roundings) stays within the derived K for every input family, both 16-bit types,
every head dim and length used on the GPU side; every injected defect is rejected; and three of those defects pass the whole-tensor bars of
tests/test_gpu_attention.py::check, which is the gap the elementwise tests close."""
import math

import pytest
import torch

import attention_bounds as ab
from oracle import denoiser as od

B, H = 2, 3
DTYPES = [torch.bfloat16, torch.float16]
NAMES = ("out", "dv", "dq", "dk")


def model(c, defect=None, **where):
    q, k, v = ab.split(c["qkv"])
    out, lse, dq, dk, dv = ab.rounding_model(q, k, v, ab.bhnd(c["dout"]), c["scale"], c["dtype"], defect, **where)
    return {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


def worst_units(c, res):
    u = ab.U[c["dtype"]]
    w = {name: ab.worst(res[name], c["ref"][name], c["c"][name], u)[0] for name in NAMES}
    w["lse"] = float((res["lse"] - c["ref"]["lse"]).abs().max()) / ab.LSE_BAR          # in units of its bar
    return w


@pytest.mark.parametrize("n", [129, 200, 385, 641])
@pytest.mark.parametrize("d", [32, 64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("family", ab.FAMILIES)
def test_clean_model_is_within_the_derived_bounds_and_every_defect_is_not(family, dtype, d, n):
    c = ab.case(family, B, H, n, d, dtype, 1000 * d + n)
    u = ab.U[dtype]
    res = model(c)
    for name in NAMES:
        ab.assert_within(res[name], c["ref"][name], c["c"][name], ab.K[name], u, f"model {family} {dtype} d={d} n={n} {name}", quiet=True)
    assert float((res["lse"] - c["ref"]["lse"]).abs().max()) <= ab.LSE_MODEL_WORST, "LSE_MODEL_WORST is the model's worst error: update it"
    # which checked quantities a defect must push past their bound (the others may or may not move).  The denominator defect is held to
    # the lse bar: its error on `out` is the lost share of the row sum times |out|, which for a flat softmax (the unscaled rows of `spike` at
    # d = 128: the largest 16-key group holds 6 % of a row) stays under K u scale in bf16 -- 2.0 units -- while lse moves by 6e-2.
    bound = dict(ab.K, lse=1.0)
    hit = {"fwd_tile": ("out",), "fwd_bwd_tile": ("out", "dq"), "last_key": ("out", "dq"), "denominator": ("lse",), "swap_rows": ("out",),
           "dq_tile": ("dq",), "dkdv_last_row": ("dv",), "dv_element": ("dv",)}
    for defect in ab.DEFECTS:
        w = worst_units(c, model(c, defect))
        for name in hit[defect]:
            assert w[name] > bound[name], f"{family} {dtype} d={d} n={n}: defect {defect} passes the bound on {name} ({w[name]:.2f} units)"


def test_three_defects_pass_the_whole_tensor_bars_and_fail_the_elementwise_bound():
    """bf16, n = 385, d = 64, the `rand` family: the denominator defect, the last query row missing from one key tile of dK / dV, and the
    single dV element pass every bar of tests/test_gpu_attention.py::check; the elementwise bound rejects all three.  The defects sit at a
    typical position here (not the most visible one that the defaults of rounding_model pick): the 16-key group / 64-key tile whose share of
    the row's softmax is closest to the uniform share."""
    n, d, dtype = 385, 64, torch.bfloat16
    c = ab.case("rand", B, H, n, d, dtype, 1000 * d + n)
    assert ab.old_criteria_pass(model(c), c["ref"])
    q, k, _ = ab.split(c["qkv"])
    p = torch.softmax(c["scale"] * (q[B - 1, H - 1].double() @ k[B - 1, H - 1].double().T), -1)

    def typical(row, width):
        pad = (-n) % width
        share = torch.cat([p[row], p.new_zeros(pad)]).view(-1, width).sum(-1)[:n // width]      # whole groups only
        return int((share - width / n).abs().argmin())

    for defect, where, name in (("denominator", {"row": n // 2, "key0": 16 * typical(n // 2, 16)}, "out"),
                                ("dkdv_last_row", {"tile": typical(n - 1, 64)}, "dv"),
                                ("dv_element", {}, "dv")):
        res = model(c, defect, **where)
        w = worst_units(c, res)
        print(f"[attention-bounds] gap: {defect} {where}: units {w}")
        assert ab.old_criteria_pass(res, c["ref"]), f"{defect} no longer passes the whole-tensor bars"
        assert w[name] > ab.K[name], f"{defect} passes the elementwise bound on {name}: {w[name]:.2f} units"


@pytest.mark.parametrize("d,n", [(64, 130), (32, 17)])
def test_reference_matches_the_oracle_and_its_autograd(d, n):
    """attention_bounds.reference against oracle.denoiser.attention_qkvpacked and autograd, float64, scale 1 / sqrt(d): 1e-12 relative."""
    gen = torch.Generator().manual_seed(n)
    qkv = torch.randn(B, n, H, 3 * d, generator=gen, dtype=torch.float64)
    dout = torch.randn(B, n, H, d, generator=gen, dtype=torch.float64)
    x = qkv.reshape(B, n, 3 * H * d).clone().requires_grad_(True)
    o = od.attention_qkvpacked(x, H)
    (o * dout.reshape(B, n, H * d)).sum().backward()
    q, k, v = ab.split(qkv)
    out, lse, dq, dk, dv = ab.reference(q, k, v, ab.bhnd(dout), 1.0 / math.sqrt(d))
    g = x.grad.view(B, n, H, 3 * d)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    assert rel(ab.bhnd(out), o.detach().view(B, n, H, d)) < 1e-12
    for j, got in enumerate((dq, dk, dv)):
        assert rel(ab.bhnd(got), g[..., j * d:(j + 1) * d]) < 1e-12
    s = torch.einsum("bhnd,bhmd->bhnm", q, k) / math.sqrt(d)
    assert rel(lse, torch.logsumexp(s, -1)) < 1e-12
