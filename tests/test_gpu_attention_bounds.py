"""The 16-bit attention kernels held to per-element bounds at every tile-count regime (tests/attention_bounds.py has the bound, its
derivation from the kernels' code and the float64 reference; tests/test_attention_bounds_cpu.py proves on the CPU that the bound holds
for the kernels' arithmetic and rejects localised defects that the whole-tensor bars of tests/test_gpu_attention.py let through).

Every case prints one line per checked tensor with the worst error in units of u * scale: docs/experiments.md ("Attention: per-element
bounds") records them.  B = 2, H = 3 throughout, so that a wrong batch / head decomposition shows.
"""
import math

import pytest
import torch

import attention_bounds as ab

pytestmark = pytest.mark.gpu

B, H = 2, 3
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "f16"]
# d = 64, one regime each at the smallest n that reaches it (seeded: (n & 63) == 1, n > 64; edge: (n & 127) == 1, n > 128, nb = 4 (n >> 7)
# partial records per edge row; row split of the 64-row forward: (n - 1) % 256 == 0, n > 256)
LENGTHS = [1, 2, 33, 64,            # single tile, unseeded
           65,                      # smallest seeded length
           128, 200, 256,           # plain
           129,                     # smallest edge length, one partial chunk
           193, 321, 449,           # seeded but not edge: 3, 5, 7 key tiles
           257,                     # edge and smallest row split
           385,                     # edge, three workgroups, nb = 12
           641,                     # edge, nb = 20: the first 16-chunk + 4-chunk sum
           769,                     # edge, nb = 24; row split with three 256-row tiles
           897,                     # edge, nb = 28
           1025,                    # the automatic switch to the 64-row form
           1153]                    # edge, not row split, 64-row form by default; nb = 36
FAMILY_N = (129, 385, 641)          # where `wide`, `spike` and `edge_dominant` run as well


def family_cases(lengths):
    return [("rand", n) for n in lengths] + [(f, n) for f in ab.FAMILIES[1:] for n in lengths if n in FAMILY_N]


def edge_mode(n):
    return (n & 127) == 1 and n > 128


def rowx_mode(n):
    return n > 256 and (n - 1) % 256 == 0


def on_gpu(c):
    """the case's inputs on the GPU: q, k, v [B, n, H, d] views of the packed buffer, dout [B, n, H, d]"""
    qkv = c["qkv"].cuda()
    d = qkv.shape[-1] // 3
    return qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], c["dout"].cuda()


def check_fwd(c, out, lse, tag):
    u = ab.U[c["dtype"]]
    ab.assert_within(ab.bhnd(out), c["ref"]["out"], c["c"]["out"], ab.K["out"], u, f"{tag} out")
    ab.assert_lse(lse, c["ref"]["lse"], tag)


def check_bwd(c, dq, dk, dv, tag):
    u = ab.U[c["dtype"]]
    n = c["dout"].shape[1]
    got = {"dq": ab.bhnd(dq), "dk": ab.bhnd(dk), "dv": ab.bhnd(dv)}
    if edge_mode(n):         # the edge token's three rows (attn_bwd_edge_kernel) as a line of their own
        print(f"[attention-bounds] {tag}: edge token rows: " + ", ".join(
            f"{name} {ab.row_units(got[name], c['ref'][name], c['c'][name], u, n - 1):.2f}" for name in got))
    for name in got:
        ab.assert_within(got[name], c["ref"][name], c["c"][name], ab.K[name], u, f"{tag} {name}")


def packed_grad(q):
    B_, n, H_, d = q.shape
    g = torch.zeros((B_, n, H_, 3 * d), dtype=q.dtype, device=q.device)
    return g, (g[..., :d], g[..., d:2 * d], g[..., 2 * d:])


@pytest.fixture(params=["auto", "32", "64"])
def fwd_form(request, monkeypatch):
    if request.param == "auto":
        monkeypatch.delenv("NPCD_ATTN_FWD", raising=False)
    else:
        monkeypatch.setenv("NPCD_ATTN_FWD", request.param)
    return request.param


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family,n", family_cases(LENGTHS))
def test_forward(family, n, dtype, fwd_form):
    from npcd.hip import attention as A
    c = ab.case(family, B, H, n, 64, dtype, 64000 + n)
    q, k, v, _ = on_gpu(c)
    out, lse = A._fwd(q, k, v, c["scale"])
    check_fwd(c, out, lse, f"fwd[{fwd_form}] {IDS[DTYPES.index(dtype)]} {family} n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [257, 769, 1025])
def test_forward_row_split_lengths_without_the_scratch(n, dtype, monkeypatch):
    """NPCD_ATTN_FWD_WS=0: the 64-row form runs a row-split length with a workgroup for the last query row instead of the scratch and the
    merge kernel.  The same bound; and _fwd then asks for no scratch at all (with the switch on it asks for the library's size)."""
    from npcd.hip import arena
    from npcd.hip import attention as A
    monkeypatch.setenv("NPCD_ATTN_FWD", "64")
    c = ab.case("rand", B, H, n, 64, dtype, 64000 + n)
    q, k, v, _ = on_gpu(c)
    want = A.lib().npcd_attn_fwd_workspace_floats(B, n, H)
    assert want == B * H * ((n - 1) // 64) * 68
    for ws_on in (True, False):
        monkeypatch.setattr(A, "FWD_WS", ws_on)
        rec = arena.StepArena()
        with rec.active():
            out, lse = A._fwd(q, k, v, c["scale"])
        asked = [t.numel() for t in rec.slots[2:]]            # behind out and lse
        assert asked == ([want] if ws_on else []), asked
        check_fwd(c, out, lse, f"fwd[64, scratch {'on' if ws_on else 'off'}] {IDS[DTYPES.index(dtype)]} rand n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family,n", family_cases(LENGTHS))
def test_two_pass_backward(family, n, dtype, monkeypatch):
    """dq, dk, dv of the default backward from the kernels' own forward (out, lse); with and without the column-sum by-product the gradients
    are bit-equal."""
    from npcd.hip import attention as A
    monkeypatch.delenv("NPCD_ATTN_FWD", raising=False)
    monkeypatch.setattr(A, "BWD_MODE", "twopass")
    c = ab.case(family, B, H, n, 64, dtype, 64000 + n)
    q, k, v, dout = on_gpu(c)
    out, lse = A._fwd(q, k, v, c["scale"])
    g0, (dq, dk, dv) = packed_grad(q)
    A._bwd(q, k, v, out, dout, lse, dq, dk, dv, c["scale"])
    g1, (dq1, dk1, dv1) = packed_grad(q)
    part, rows = A.colsum_part_for(dq1)
    A._bwd(q, k, v, out, dout, lse, dq1, dk1, dv1, c["scale"], colsum_part=part)
    assert torch.equal(g0, g1), "the column-sum by-product changes the gradients' bits"
    check_bwd(c, dq, dk, dv, f"bwd {IDS[DTYPES.index(dtype)]} {family} n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family,n", family_cases([64, 129, 256, 257, 385, 641, 769]))
def test_single_pass_backward(family, n, dtype, monkeypatch):
    """NPCD_ATTN_BWD=fused (attn_bwd_fused_kernel): both sides of its 256-key pass and an odd number of passes; the K of the two-pass kernels
    (the same rounding points: tests/attention_bounds.py)."""
    from npcd.hip import attention as A
    monkeypatch.delenv("NPCD_ATTN_FWD", raising=False)
    monkeypatch.setattr(A, "BWD_MODE", "fused")
    c = ab.case(family, B, H, n, 64, dtype, 64000 + n)
    q, k, v, dout = on_gpu(c)
    out, lse = A._fwd(q, k, v, c["scale"])
    _, (dq, dk, dv) = packed_grad(q)
    A._bwd(q, k, v, out, dout, lse, dq, dk, dv, c["scale"])
    check_bwd(c, dq, dk, dv, f"bwd-fused {IDS[DTYPES.index(dtype)]} {family} n={n}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family,n", family_cases([1, 33, 65, 129, 200, 385, 641]))
@pytest.mark.parametrize("d,forced", [(32, False), (128, False), (64, True)], ids=["d32", "d128", "d64gen"])
def test_generic_family(d, forced, family, n, dtype, monkeypatch):
    """csrc/attention_gen.hip: head dims 32 and 128, and 64 under NPCD_ATTN_GEN=1; forward and backward."""
    from npcd.hip import attention as A
    monkeypatch.delenv("NPCD_ATTN_FWD", raising=False)
    monkeypatch.setattr(A, "BWD_MODE", "twopass")
    if forced:
        monkeypatch.setenv("NPCD_ATTN_GEN", "1")
    else:
        monkeypatch.delenv("NPCD_ATTN_GEN", raising=False)
    c = ab.case(family, B, H, n, d, dtype, 1000 * d + n)
    q, k, v, dout = on_gpu(c)
    out, lse = A._fwd(q, k, v, c["scale"])
    tag = f"gen d={d} {IDS[DTYPES.index(dtype)]} {family} n={n}"
    check_fwd(c, out, lse, tag)
    _, (dq, dk, dv) = packed_grad(q)
    A._bwd(q, k, v, out, dout, lse, dq, dk, dv, c["scale"])
    check_bwd(c, dq, dk, dv, tag)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [129, 385])
@pytest.mark.parametrize("s", [0.05, 0.3])
def test_free_softmax_scale(s, n, dtype, monkeypatch):
    """flash_attn_func(q, k, v, softmax_scale=s) with s other than 1 / sqrt(d): forward and backward against reference(..., scale=s)."""
    from flash_attn import flash_attn_func
    monkeypatch.delenv("NPCD_ATTN_FWD", raising=False)
    c = ab.case("rand", B, H, n, 64, dtype, 64000 + n, s)
    assert c["scale"] == s
    x = c["qkv"].cuda().requires_grad_(True)
    q, k, v = torch.split(x, 64, dim=-1)
    out = flash_attn_func(q, k, v, softmax_scale=s)
    out.backward(c["dout"].cuda())
    tag = f"scale={s} {IDS[DTYPES.index(dtype)]} rand n={n}"
    u = ab.U[dtype]
    ab.assert_within(ab.bhnd(out.detach()), c["ref"]["out"], c["c"]["out"], ab.K["out"], u, f"{tag} out")
    g = x.grad
    check_bwd(c, g[..., :64], g[..., 64:128], g[..., 128:], tag)


# ------------------------------------------------------------------------------------------------------ layouts and guard bands
SENTINEL = -12288.0          # exact in bf16, f16 and fp32; no attention output comes near it
GUARD = 256                  # elements in front of and behind every carved buffer (keeps 16-byte alignment)


class Carved:
    """`numel` elements inside a larger sentinel-filled buffer"""

    def __init__(self, numel, dtype):
        self.buf = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + numel]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.t.numel():] == SENTINEL).all())


def padded_rows(n, d, pad, dtype):
    """[B, n, H, d] whose rows are d + pad elements apart, carved; -> (Carved, the [B, n, H, d + pad] view with the padding columns)"""
    cv = Carved(B * n * H * (d + pad), dtype)
    return cv, cv.t.view(B, n, H, d + pad)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("pad", [8, 24])
@pytest.mark.parametrize("n", [1, 65, 129, 257, 641])
def test_layouts_and_guard_bands(n, pad, dtype, monkeypatch):
    """Through the library entry points with the argument block built by hand: out / dout rows padded by `pad` elements; dq, dk, dv as three
    separate contiguous tensors (g_sh = d); out, lse, the gradients, delta (exactly npcd_attn_bwd_workspace_floats), the row-split scratch
    (exactly npcd_attn_fwd_workspace_floats) and, in a second backward on the packed layout, the gradient and the column-sum partials
    (npcd_attn_bwd_colsum_rows + the scratch rows) all carved out of sentinel-filled buffers.  Afterwards every sentinel outside the documented
    extents is intact -- the padding columns too --, none is left inside out, lse or the gradients, and the values meet the bounds.  Both forms
    of the forward.  Everything read here is memory the test owns."""
    from npcd.hip import attention as A
    from npcd.hip import check, lib, stream_ptr
    d = 64
    c = ab.case("rand", B, H, n, d, dtype, 64000 + n)
    q, k, v, dout_c = on_gpu(c)
    u = ab.U[dtype]
    name = IDS[DTYPES.index(dtype)]
    for form in ("32", "64"):
        monkeypatch.setenv("NPCD_ATTN_FWD", form)
        tag = f"layout pad={pad} fwd[{form}] {name} n={n}"
        out_cv, out_p = padded_rows(n, d, pad, dtype)
        out = out_p[..., :d]
        lse_cv = Carved(B * H * n, torch.float32)
        lse = lse_cv.t.view(B, H, n)
        nws = lib().npcd_attn_fwd_workspace_floats(B, n, H)
        assert (nws > 0) == (form == "64" and rowx_mode(n))
        ws_cv = Carved(nws, torch.float32) if nws > 0 else None
        a = A._args(q, k, v, out, lse, c["scale"], workspace=ws_cv.t if ws_cv else None)
        check(lib().npcd_attn_fwd(a, stream_ptr()), "npcd_attn_fwd")
        torch.cuda.synchronize()
        assert out_cv.guards_intact() and lse_cv.guards_intact() and (ws_cv is None or ws_cv.guards_intact()), f"{tag}: a forward guard band was written"
        assert bool((out_p[..., d:] == SENTINEL).all()), f"{tag}: the padding columns of out were written"
        assert not bool((out == SENTINEL).any()) and not bool((lse == SENTINEL).any()), f"{tag}: out or lse has unwritten elements"
        check_fwd(c, out, lse, tag)

        # backward: padded dout (its padding columns hold the sentinel as well), three separate gradient tensors
        dout_cv, dout_p = padded_rows(n, d, pad, dtype)
        dout = dout_p[..., :d]
        dout.copy_(dout_c)
        assert dout.stride() == out.stride()
        g_cv = [Carved(B * n * H * d, dtype) for _ in range(3)]
        dq, dk, dv = (g.t.view(B, n, H, d) for g in g_cv)
        delta_cv = Carved(lib().npcd_attn_bwd_workspace_floats(B, n, H), torch.float32)
        a = A._args(q, k, v, out, lse, c["scale"], dout, dq, dk, dv, delta_cv.t)
        check(lib().npcd_attn_bwd(a, 3, stream_ptr()), "npcd_attn_bwd")
        torch.cuda.synchronize()
        assert all(g.guards_intact() for g in g_cv) and delta_cv.guards_intact(), f"{tag}: a backward guard band was written"
        assert out_cv.guards_intact() and dout_cv.guards_intact() and bool((out_p[..., d:] == SENTINEL).all())
        assert not any(bool((g.t == SENTINEL).any()) for g in g_cv), f"{tag}: a gradient has unwritten elements"
        check_bwd(c, dq, dk, dv, tag)

        # the packed layout with the column-sum partials: the same bits as the three separate tensors
        gp_cv = Carved(B * n * H * 3 * d, dtype)
        gp = gp_cv.t.view(B, n, H, 3 * d)
        rows = lib().npcd_attn_bwd_colsum_rows(B, n, H)
        width = 3 * H * d
        part_cv = Carved((rows + lib().npcd_colsum_scratch_rows()) * width, torch.float32)
        delta2_cv = Carved(delta_cv.t.numel(), torch.float32)
        a = A._args(q, k, v, out, lse, c["scale"], dout, gp[..., :d], gp[..., d:2 * d], gp[..., 2 * d:], delta2_cv.t, part_cv.t)
        check(lib().npcd_attn_bwd(a, 3, stream_ptr()), "npcd_attn_bwd(colsum)")
        torch.cuda.synchronize()
        assert gp_cv.guards_intact() and part_cv.guards_intact() and delta2_cv.guards_intact(), f"{tag}: a guard band of the packed backward was written"
        assert not bool((part_cv.t[:rows * width] == SENTINEL).any()), f"{tag}: a column-sum partial row was not written"
        assert torch.equal(gp[..., :d], dq) and torch.equal(gp[..., d:2 * d], dk) and torch.equal(gp[..., 2 * d:], dv)
        assert torch.equal(delta2_cv.t, delta_cv.t)
