"""The ray march of csrc/geometry.hip, restated: the cases, the float64 references and the bars that tests/test_gpu_ray_march.py holds
the kernels to -- and the proof, on the CPU, that those bars can fail.

Cases (march_case): dense inputs of a march of Nr rays with M slots each.  Ray 0 is empty and ray 1 full; ray 2 has one valid slot,
the last (a point without weight); a march of a single ray consists of that last-slot-only ray, so that it reads a point at all.
About 40 % of the other slots are valid.  Every third ray looks along (0, 0, 1) exactly and every fifth along normalize((0, 0.3, 1)):
components that are 0 make (p - o) / d = 0 / 0, the branch of the depth's nanmean that skips a component.  The slot positions of the
last five rays are shuffled along the ray, so that the running maximum of the depth has work to do.  Positions of valid slots are
o + t d in fp32; positions of invalid slots are NaN, since nothing may read them.  compact_view() is the same case in the layout of
the compact entry points.

References: the slot depths come from oracle.renderer.depths_from_points in fp32 -- the kernels' own, separately rounded operations --
and are then cast to float64; the march on them is oracle.renderer.ray_march in float64, its backward float64 autograd through the same
formulas (terms()).  The depth term of the backward's scalar selects the rows with weight BEFORE it divides: a `where` after the
division lets 0 * inf into the gradients.  The same code in fp32 (dtype=torch.float32) is the yardstick: a bar is
max(16 x the fp32 restatement's error on that case, 4 fp32 ulps of the output's scale) and may not exceed its ceiling (CEILINGS).
The wave kernels add and multiply in scan and tree order and the device's expf may differ from the host's by an ulp or two, hence 16;
a wrong index, mask bit or prefix shows at 1e-3 or more (the mutants below: each leaves a ceiling by a factor of 10 at least).

Measured, fp32 restatement against float64, the maximum over all the cases: mask 1.3e-7, channels 1.8e-7, depth at mask >= 0.05
4.8e-7, depth error x mask 1.7e-7, dsigma 2.3e-7 (gated g_depth, against gradients of 1.8), drgb 1.3e-7: every bar is below 8e-6.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import renderer as orr

FORWARD_SHAPES = [(1, 1), (5, 2), (3, 63), (4, 64), (5, 64), (257, 64), (1003, 48), (130, 65), (130, 100)]
BACKWARD_SHAPES = [(1, 1), (5, 2), (63, 50), (64, 64), (65, 64), (300, 50)]
OPAQUE = (257, 64, 2000.0)              # (Nr, M, sigma_max)
ALL_EMPTY = (70, 33)
MASK_GATE = 0.05                        # depth is judged, and g_depth non-zero, on rays with at least this much weight
CEILINGS = {"mask": 5e-6, "chan": 5e-6, "drgb": 5e-6, "depth": 2e-5, "depth_w": 5e-6}
CEILINGS_FORWARD = {k: CEILINGS[k] for k in ("mask", "chan", "depth", "depth_w")}
DSIGMA_CEILING = 1e-4                   # times max(1, max |dsigma_ref|)
FORWARD_MUTANTS = ("inclusive_transmittance", "no_running_maximum", "leading_empty_at_zero", "last_slot_closed", "background_when_black",
                   "point_base_off_by_one")
BACKWARD_MUTANTS = ("suffix_inclusive", "depth_gradient_when_clamped")
STANDARD_FORWARD = [(257, 64), (1003, 48), (130, 100)]
STANDARD_BACKWARD = [(64, 64), (300, 50)]


# ------------------------------------------------------------------ cases ---------------------
@functools.lru_cache(maxsize=None)
def march_case(Nr, M, seed=None, sigma_max=5.0, empty_rays=(), all_empty=False):
    """-> dict of CPU tensors: valid [Nr,M] bool, o, d [Nr,3], slot_loc [Nr,M,3], t1 [Nr], sigma [P], rgb [P,3], point_base [Nr] int32,
    g_mask, g_depth [Nr], g_chan [Nr,3].  Cached: treat as read-only."""
    g = torch.Generator().manual_seed(1000 * Nr + M if seed is None else seed)
    valid = torch.rand(Nr, M, generator=g) < 0.4
    if Nr == 1:
        valid[0] = False
        valid[0, M - 1] = True
    else:
        valid[0] = False
        valid[1] = True
        if Nr > 2:
            valid[2] = False
            valid[2, M - 1] = True
    for r in empty_rays:
        valid[r] = False
    if all_empty:
        valid[:] = False
    o = torch.randn(Nr, 3, generator=g) * 0.1 + torch.tensor([0.0, 0.0, -2.0])
    d = torch.nn.functional.normalize(torch.randn(Nr, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 1.0]), dim=1)
    d[4::5] = torch.nn.functional.normalize(torch.tensor([0.0, 0.3, 1.0]), dim=0)
    d[0::3] = torch.tensor([0.0, 0.0, 1.0])
    t = torch.sort(torch.rand(Nr, M, generator=g) * 1.5 + 0.5, dim=1).values
    for r in range(max(Nr - 5, 3), Nr):
        t[r] = t[r, torch.randperm(M, generator=g)]
    loc = o[:, None, :] + t[..., None] * d[:, None, :]               # fp32, each operation rounded
    loc = torch.where(valid[..., None], loc, torch.full_like(loc, math.nan))
    t1 = 2.05 + 0.4 * torch.rand(Nr, generator=g)
    per_ray = valid.sum(1).int()
    P = int(per_ray.sum())
    return {"Nr": Nr, "M": M, "valid": valid, "o": o, "d": d, "slot_loc": loc, "t1": t1,
            "sigma": torch.rand(P, generator=g) * sigma_max, "rgb": torch.rand(P, 3, generator=g),
            "point_base": (torch.cumsum(per_ray, 0) - per_ray).int(),
            "g_mask": torch.randn(Nr, generator=g), "g_depth": torch.randn(Nr, generator=g), "g_chan": torch.randn(Nr, 3, generator=g)}


def compact_view(case):
    """-> ray_bits [Nr] int64 (bit j = slot j valid; built as uint64), pts [P,3], ray_base [Nr] int32"""
    assert case["M"] <= 64
    bits = np.zeros(case["Nr"], dtype=np.uint64)
    v = case["valid"].numpy()
    for j in range(case["M"]):
        bits |= v[:, j].astype(np.uint64) << np.uint64(j)
    return torch.from_numpy(bits.view(np.int64)), case["slot_loc"][case["valid"]].contiguous(), case["point_base"]


def changed(case, **kw):
    out = dict(case)
    out.update(kw)
    return out


# ------------------------------------------------------------------ references ----------------
def slot_depths(case, defect=None):
    """-> [Nr,M] fp32, renderer.py:96-110"""
    end = case["t1"][:, None]
    if defect is None:
        return orr.depths_from_points(case["slot_loc"], case["valid"], case["o"], case["d"], end)
    raw = torch.nanmean((case["slot_loc"] - case["o"][:, None, :]) / case["d"][:, None, :], dim=-1)
    if defect == "no_running_maximum":
        return torch.where(case["valid"], raw, end.expand_as(raw))
    assert defect == "leading_empty_at_zero"
    run = torch.cummax(torch.where(case["valid"], raw, torch.full_like(raw, -math.inf)), dim=1).values
    return torch.where(run == -math.inf, torch.zeros_like(run), run)


def dense(valid, base, sigma, rgb):
    """compact [P], [P,3] -> dense [Nr,M], [Nr,M,3] with zeros at invalid slots (differentiable)"""
    idx = base[:, None].long() + (valid.cumsum(1) - valid.long())
    if sigma.shape[0] == 0:
        return torch.zeros(valid.shape, dtype=sigma.dtype), torch.zeros(valid.shape + (3,), dtype=sigma.dtype)
    idx = idx.clamp(0, sigma.shape[0] - 1)
    return torch.where(valid, sigma[idx], torch.zeros((), dtype=sigma.dtype)), \
        torch.where(valid[..., None], rgb[idx], torch.zeros((), dtype=sigma.dtype))


def terms(sigma, depths, rgb, valid, white_back, ray_end=None, defect=None):
    """volume_renderer.py:23-39 -> alpha, trans, w [Nr,M], total, wd [Nr], chan [Nr,3]; the operations of oracle.renderer.ray_march"""
    last = torch.zeros_like(depths[:, :1]) if defect != "last_slot_closed" else ray_end[:, None].to(depths.dtype) - depths[:, -1:]
    delta = torch.cat((depths[:, 1:] - depths[:, :-1], last), dim=1)
    alpha = 1.0 - torch.exp(-(sigma * delta))
    prod = torch.cumprod(torch.cat((torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-10), dim=1), dim=1)
    trans = prod[:, 1:] if defect == "inclusive_transmittance" else prod[:, :-1]
    w = alpha * trans
    total = w.sum(dim=1, keepdim=True)
    wd = (w * depths).sum(dim=1, keepdim=True)
    chan = ((w * valid)[..., None] * rgb).sum(dim=1)
    if white_back or defect == "background_when_black":
        chan = chan + 1.0 - total
    return {"delta": delta, "alpha": alpha, "trans": trans, "w": w, "total": total[:, 0], "wd": wd[:, 0], "chan": chan}


def march_reference(case, white_back, dtype=torch.float64, defect=None):
    """-> mask [Nr], depth [Nr], chan [Nr,3] in `dtype`, lo, hi: the fp32 limits of the slot depths"""
    dep32 = slot_depths(case, defect if defect in ("no_running_maximum", "leading_empty_at_zero") else None)
    lo, hi = dep32.min(), dep32.max()
    base = case["point_base"]
    if defect == "point_base_off_by_one":
        base = base.clone()
        base[1 if case["Nr"] > 1 else 0] += 1
    sd, rd = dense(case["valid"], base, case["sigma"].to(dtype), case["rgb"].to(dtype))
    dep = dep32.to(dtype)
    if defect is None:
        total, depth, chan = orr.ray_march(sd, dep, rd, case["valid"], white_back)
        return {"mask": total[:, 0], "depth": depth[:, 0], "chan": chan, "lo": lo, "hi": hi}
    t = terms(sd, dep, rd, case["valid"], white_back, case["t1"], defect)
    depth = torch.nan_to_num(t["wd"] / t["total"], float("inf")).clamp(dep.min(), dep.max())
    return {"mask": t["total"], "depth": depth, "chan": t["chan"], "lo": lo, "hi": hi}


def gated_g_depth(case, white_back):
    """the case's g_depth, zero where the reference mask is below MASK_GATE (there fp32's g_depth / mask would set the bar)"""
    return torch.where(march_reference(case, white_back)["mask"] >= MASK_GATE, case["g_depth"], torch.zeros_like(case["g_depth"]))


def backward_reference(case, white_back, g_depth, dtype=torch.float64):
    """autograd through terms() -> dsigma [P], drgb [P,3] in `dtype`"""
    sigma = case["sigma"].to(dtype).clone().requires_grad_(True)
    rgb = case["rgb"].to(dtype).clone().requires_grad_(True)
    dep = slot_depths(case).to(dtype)
    sd, rd = dense(case["valid"], case["point_base"], sigma, rgb)
    t = terms(sd, dep, rd, case["valid"], white_back)
    rows = t["total"] > 0                                   # select, then divide
    raw = t["wd"][rows] / t["total"][rows]
    inside = ((raw >= dep.min()) & (raw <= dep.max())).to(dtype)
    scalar = (t["total"] * case["g_mask"].to(dtype)).sum() + (t["chan"] * case["g_chan"].to(dtype)).sum() \
        + (raw * inside * g_depth.to(dtype)[rows]).sum()
    if sigma.shape[0] == 0:
        return {"dsigma": torch.zeros(0, dtype=dtype), "drgb": torch.zeros(0, 3, dtype=dtype)}
    scalar.backward()
    return {"dsigma": sigma.grad, "drgb": rgb.grad}


def backward_formula(case, white_back, g_depth, defect=None):
    """The backward as csrc/geometry.hip states it above ray_march_bwd_kernel, in float64: with G_i = dL/dw_i and the suffix sum
    S_i = sum_{j>i} G_j w_j,  dL/dalpha_i = G_i T_i - S_i / (1 - alpha_i + 1e-10),  dsigma_i = dL/dalpha_i delta_i exp(-sigma_i delta_i),
    drgb_i = g_chan w_i.  Equal to autograd (tested below); it is what the backward's mutants are applied to."""
    f8 = torch.float64
    dep = slot_depths(case).to(f8)
    valid = case["valid"]
    sd, rd = dense(valid, case["point_base"], case["sigma"].to(f8), case["rgb"].to(f8))
    t = terms(sd, dep, rd, valid, white_back)
    gm, gd, gc = case["g_mask"].to(f8), g_depth.to(f8), case["g_chan"].to(f8)
    raw = t["wd"] / t["total"]                                                      # NaN on a ray without weight
    live = (t["total"] > 0) & (raw >= dep.min()) & (raw <= dep.max())
    G = (gm - (gc.sum(1) if white_back else 0.0))[:, None] + (rd * gc[:, None, :]).sum(-1) * valid
    depth_term = (gd / t["total"])[:, None] * (dep - raw[:, None])
    G = G + (depth_term if defect == "depth_gradient_when_clamped" else torch.where(live[:, None], depth_term, torch.zeros_like(G)))
    Gw = G * t["w"]
    S = torch.flip(torch.cumsum(torch.flip(Gw, [1]), 1), [1])
    if defect != "suffix_inclusive":
        S = S - Gw
    dalpha = G * t["trans"] - S / (1.0 - t["alpha"] + 1e-10)
    dsig = dalpha * t["delta"] * torch.exp(-(sd * t["delta"]))
    return {"dsigma": dsig[valid], "drgb": (gc[:, None, :] * t["w"][..., None])[valid]}


# ------------------------------------------------------------------ errors and bars -----------
def ulp(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def worst(x):
    """max |x|, NaN counting as infinite; 0 for no element"""
    return float(torch.nan_to_num(x.double().abs(), nan=math.inf).max()) if x.numel() else 0.0


def forward_errors(got, ref):
    """got, ref: dicts of mask / depth / chan (CPU tensors) -> the four figures a forward result is judged by"""
    heavy = ref["mask"] >= MASK_GATE
    derr = got["depth"].double() - ref["depth"].double()
    return {"mask": worst(got["mask"].double() - ref["mask"].double()), "chan": worst(got["chan"].double() - ref["chan"].double()),
            "depth": worst(derr[heavy]), "depth_w": worst(derr * ref["mask"].double())}


def backward_errors(got, ref):
    return {"dsigma": worst(got["dsigma"].double() - ref["dsigma"].double()), "drgb": worst(got["drgb"].double() - ref["drgb"].double())}


def bar(e32, scale, ceiling):
    b = max(16.0 * e32, 4.0 * ulp(scale))
    assert b <= ceiling, f"bar {b:.3g} above its ceiling {ceiling:.3g}: change the case"
    return b


def forward_bars(case, white_back, ref=None):
    """-> (float64 reference, bars, fp32 restatement's errors)"""
    ref = march_reference(case, white_back) if ref is None else ref
    e32 = forward_errors(march_reference(case, white_back, torch.float32), ref)
    scale = {"mask": 1.0, "chan": 1.0, "depth": float(ref["hi"]), "depth_w": float(ref["hi"])}
    return ref, {k: bar(e32[k], scale[k], CEILINGS[k]) for k in e32}, e32


def backward_ceilings(ref):
    return {"dsigma": DSIGMA_CEILING * max(1.0, worst(ref["dsigma"])), "drgb": CEILINGS["drgb"]}


def backward_bars(case, white_back, g_depth):
    ref = backward_reference(case, white_back, g_depth)
    assert not torch.isnan(ref["dsigma"]).any() and not torch.isnan(ref["drgb"]).any()
    e32 = backward_errors(backward_reference(case, white_back, g_depth, torch.float32), ref)
    ceil = backward_ceilings(ref)
    scale = {"dsigma": max(1.0, worst(ref["dsigma"])), "drgb": max(1.0, worst(ref["drgb"]))}
    return ref, {k: bar(e32[k], scale[k], ceil[k]) for k in e32}, e32


def g_depth_runs(case, white_back):
    """the two gradient runs of a shape: without a depth term, and with the gated one"""
    return {"g_depth = 0": torch.zeros_like(case["g_depth"]), "gated g_depth": gated_g_depth(case, white_back)}


def fkey(x):
    """the monotone key csrc/geometry.hip orders floats by (unsigned compare): negative floats flipped, others with the top bit set"""
    u = int(np.array(x, dtype=np.float32).view(np.uint32))
    return (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)


def cameras(res, zoom=1.0, V=3):
    """-> extr [V,4,4], intr [V,3,3]: cameras on the data set's sphere; zoom < 1 widens the view until the corner rays miss the cube"""
    extr = torch.stack([orr.look_at_pose(30 + 97 * i, 20 - 13 * i) for i in range(V)])
    K = orr.srn_intrinsics().clone()
    K[0, 0] = K[1, 1] = 131.25 * res / 128 * zoom
    K[0, 2] = K[1, 2] = res / 2
    return extr, K[None].expand(V, 3, 3).contiguous()


def raw_box_limits(o, d, box=1.0):
    """math_utils.py:46-97 in fp32 -> tmin, tmax [...] with -1 / -2 for a ray that misses: oracle.renderer.ray_box_limits before it gives
    the missing rays the limits of the others"""
    inv = 1.0 / d
    neg = inv < 0
    t0 = (torch.where(neg, box, -box) - o) * inv
    t1 = (torch.where(neg, -box, box) - o) * inv
    tmin, tmax = t0[..., 0], t1[..., 0]
    ok = ~((tmin > t1[..., 1]) | (t0[..., 1] > tmax))
    tmin, tmax = torch.max(tmin, t0[..., 1]), torch.min(tmax, t1[..., 1])
    ok &= ~((tmin > t1[..., 2]) | (t0[..., 2] > tmax))
    tmin, tmax = torch.max(tmin, t0[..., 2]), torch.min(tmax, t1[..., 2])
    return torch.where(ok, tmin, torch.full_like(tmin, -1.0)), torch.where(ok, tmax, torch.full_like(tmax, -2.0))


# ------------------------------------------------------------------ tests ---------------------
ALL_CASES = sorted(set(FORWARD_SHAPES) | set(BACKWARD_SHAPES))


@pytest.mark.parametrize("Nr,M", ALL_CASES)
def test_the_cases_hold_what_they_promise(Nr, M):
    c = march_case(Nr, M)
    v, d = c["valid"], c["d"]
    assert c["sigma"].shape == (int(v.sum()),) and c["rgb"].shape == (int(v.sum()), 3)
    if Nr == 1:
        assert v[0].sum() == 1 and v[0, M - 1]
    else:
        assert not v[0].any() and v[1].all()
    if Nr > 2:
        assert v[2].sum() == 1 and v[2, M - 1]
    assert (d[0::3] == torch.tensor([0.0, 0.0, 1.0])).all()
    if Nr > 4:
        tilted = d[[r for r in range(4, Nr, 5) if r % 3]]
        assert (tilted[:, 0] == 0).all() and (tilted[:, 1] > 0.28).all() and (tilted[:, 2] < 1).all()
    if Nr > 100:
        assert 0.35 < float(v[3:].float().mean()) < 0.45
    # positions: o + t d where valid (a zero direction component gives the origin's component back exactly), NaN elsewhere
    assert torch.isnan(c["slot_loc"][~v]).all() and torch.isfinite(c["slot_loc"][v]).all()
    zero = (d == 0)[:, None, :].expand(-1, M, -1) & v[..., None]
    assert torch.equal(c["slot_loc"][zero], c["o"][:, None, :].expand(-1, M, -1)[zero])
    # the depths: the oracle's nanmean is ((q0 + q1) + q2) / count over the components that are numbers, as the kernels add them
    q = (c["slot_loc"] - c["o"][:, None, :]) / c["d"][:, None, :]
    acc, cnt = torch.zeros(Nr, M), torch.zeros(Nr, M)
    for a in range(3):
        ok = ~torch.isnan(q[..., a])
        acc = torch.where(ok, acc + q[..., a], acc)
        cnt = cnt + ok
    run = torch.cummax(torch.where(v, acc / cnt, torch.full_like(acc, -math.inf)), dim=1).values
    mine = torch.where(run == -math.inf, c["t1"][:, None].expand_as(run), run)
    dep = slot_depths(c)
    assert torch.equal(mine.view(torch.int32), dep.view(torch.int32))
    assert torch.isfinite(dep).all() and float(dep.min()) >= 0.49 and float(dep.max()) <= 2.46
    if Nr >= 8 and M >= 8:                                   # the shuffled rays are out of order, the running maximum is not
        raw = torch.where(v, acc / cnt, torch.full_like(acc, math.nan))[Nr - 5:]
        out_of_order = sum(int((r[~torch.isnan(r)].diff() < 0).any()) for r in raw)
        assert out_of_order >= 3
    assert (dep.diff(dim=1)[v[:, :-1]] >= 0).all()
    if M <= 64:
        bits, pts, base = compact_view(c)
        assert pts.shape == (int(v.sum()), 3)
        for r in (0, Nr // 2, Nr - 1):
            word = int(bits[r]) & 0xFFFFFFFFFFFFFFFF
            assert [bool(word >> j & 1) for j in range(M)] == v[r].tolist() and word >> M == 0
        if M == 64 and Nr > 1:
            assert int(bits[1]) == -1                         # the full ray: all 64 bits, the top one included


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("Nr,M", FORWARD_SHAPES)
def test_forward_reference_and_bars(Nr, M, white_back):
    c = march_case(Nr, M)
    ref, bars, e32 = forward_bars(c, white_back)
    print(f"fp32 restatement ({Nr},{M}) white_back={white_back}: " + " ".join(f"{k} {e32[k]:.2e} (bar {bars[k]:.2e})" for k in bars))
    for k in ("mask", "depth", "chan"):
        assert torch.isfinite(ref[k]).all()
    # terms() is oracle.renderer.ray_march operation for operation
    dep = slot_depths(c).double()
    sd, rd = dense(c["valid"], c["point_base"], c["sigma"].double(), c["rgb"].double())
    t = terms(sd, dep, rd, c["valid"], white_back)
    assert torch.equal(t["total"], ref["mask"]) and torch.equal(t["chan"], ref["chan"])
    weightless = ref["mask"] == 0
    assert weightless[0] and (Nr < 3 or weightless[2])
    assert (ref["depth"][weightless] == float(ref["hi"])).all()
    assert (ref["chan"][weightless] == (1.0 if white_back else 0.0)).all()
    assert float(ref["lo"]) == float(dep.min()) and float(ref["hi"]) == float(dep.max())
    if Nr > 100:
        assert float(ref["mask"].max()) > 0.95 and int((ref["mask"] >= MASK_GATE).sum()) > Nr // 2


def test_opaque_and_empty_cases():
    Nr, M, smax = OPAQUE
    c = march_case(Nr, M, sigma_max=smax)
    for wb in (True, False):
        ref, bars, e32 = forward_bars(c, wb)
        print(f"fp32 restatement opaque white_back={wb}: " + " ".join(f"{k} {e32[k]:.2e} (bar {bars[k]:.2e})" for k in bars))
        assert all(torch.isfinite(ref[k]).all() for k in ("mask", "depth", "chan"))
        assert float(ref["mask"].max()) == 1.0 or float(ref["mask"].max()) > 1 - 1e-9
    e = march_case(*ALL_EMPTY, all_empty=True)
    ref, _, _ = forward_bars(e, True)
    assert e["sigma"].numel() == 0 and (ref["mask"] == 0).all() and (ref["chan"] == 1).all()
    assert float(ref["lo"]) == float(e["t1"].min()) and float(ref["hi"]) == float(e["t1"].max())
    assert (ref["depth"] == float(ref["hi"])).all()


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("Nr,M", BACKWARD_SHAPES)
def test_backward_reference_and_bars(Nr, M, white_back):
    c = march_case(Nr, M)
    mask = march_reference(c, white_back)["mask"]
    for name, g_depth in g_depth_runs(c, white_back).items():
        assert (g_depth[mask < MASK_GATE] == 0).all()                       # the condition on the inputs
        ref, bars, e32 = backward_bars(c, white_back, g_depth)
        print(f"fp32 restatement ({Nr},{M}) white_back={white_back} {name}: "
              + " ".join(f"{k} {e32[k]:.2e} (bar {bars[k]:.2e}, max |ref| {worst(ref[k]):.2e})" for k in bars))
        formula = backward_formula(c, white_back, g_depth)
        for k in ("dsigma", "drgb"):
            assert ref[k].shape == formula[k].shape
            assert worst(formula[k] - ref[k]) <= 1e-12 * max(1.0, worst(ref[k])), k
        if Nr > 2 or Nr == 1:                                               # the point of the last-slot-only ray
            p = int(c["point_base"][2 if Nr > 2 else 0])
            assert float(ref["dsigma"][p]) == 0.0 and (ref["drgb"][p] == 0).all()
    if Nr >= 63:
        assert int((gated_g_depth(c, white_back) != 0).sum()) > Nr // 2


def leaves_the_ceilings(errors, ceilings):
    return max(errors[k] / ceilings[k] for k in errors)


@pytest.mark.parametrize("defect", FORWARD_MUTANTS)
def test_forward_mutants_leave_the_ceilings(defect):
    for Nr, M in STANDARD_FORWARD:
        c = march_case(Nr, M)
        wb = defect != "background_when_black"
        ref = march_reference(c, wb)
        got = march_reference(c, wb, defect=defect)
        factor = leaves_the_ceilings(forward_errors(got, ref), CEILINGS_FORWARD)
        if defect == "leading_empty_at_zero":
            # a slot before the first point has no density: where it lies changes no weight, only the depth limits (and with them
            # the depth of the rays without weight), which have no tolerance: the kernels' two limit words and those depths equal
            # the reference bit for bit
            assert factor == 0.0 and float(got["lo"]) == 0.0 and float(ref["lo"]) > 0.49 and float(got["hi"]) < float(ref["hi"])
            factor = math.inf
        print(f"{defect} ({Nr},{M}): {factor:.3g} x ceiling")
        assert factor >= 10.0, (defect, Nr, M, factor)



@pytest.mark.parametrize("defect", BACKWARD_MUTANTS)
def test_backward_mutants_leave_the_ceilings(defect):
    for Nr, M in STANDARD_BACKWARD:
        c = march_case(Nr, M)
        for wb in (True, False):
            g_depth = gated_g_depth(c, wb)
            ref = backward_reference(c, wb, g_depth)
            factor = leaves_the_ceilings(backward_errors(backward_formula(c, wb, g_depth, defect), ref), backward_ceilings(ref))
            print(f"{defect} ({Nr},{M}) white_back={wb}: {factor:.3g} x ceiling")
            assert factor >= 10.0, (defect, Nr, M, wb, factor)


def test_a_where_after_the_division_poisons_the_gradients():
    """why backward_reference selects the rows first"""
    c = march_case(64, 64)
    sigma = c["sigma"].double().clone().requires_grad_(True)
    dep = slot_depths(c).double()
    sd, rd = dense(c["valid"], c["point_base"], sigma, c["rgb"].double())
    t = terms(sd, dep, rd, c["valid"], True)
    torch.where(t["total"] > 0, t["wd"] / t["total"], torch.zeros_like(t["wd"])).sum().backward()
    assert torch.isnan(sigma.grad).any()


def test_key_and_box_limits_helpers():
    xs = [-math.inf, -2.0, -1.0, -0.0, 0.0, 1e-30, 1.0, 3.5, math.inf]
    keys = [fkey(x) for x in xs]
    assert all(a < b for a, b in zip(keys, keys[1:])) and 0 < keys[0] and keys[-1] < 0xFFFFFFFF
    o, d = orr.camera_rays(*cameras(24, 0.45), 24)
    lo, hi = raw_box_limits(o, d)
    hit = hi > lo
    assert 0 < int(hit.sum()) < hit.numel() and (lo[~hit] == -1).all() and (hi[~hit] == -2).all()
    s, e = orr.ray_box_limits(o, d)
    assert torch.equal(s[..., 0][hit], lo[hit]) and torch.equal(e[..., 0][hit], hi[hit])
    assert (s[..., 0][~hit] == lo[hit].min()).all() and (e[..., 0][~hit] == hi[hit].max()).all()
