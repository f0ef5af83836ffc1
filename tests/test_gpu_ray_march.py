"""Every form of the ray march of csrc/geometry.hip -- ray_march_kernel<COMPACT>, ray_march_wave_kernel<COMPACT, FUSED>,
ray_march_bwd_kernel, depth_clamp_kernel -- against the float64 references of tests/test_ray_march_cpu.py, and npcd_ray_gen_subset
against the full ray generation.

The cases, the references and the bars are those of tests/test_ray_march_cpu.py, where the mutants prove that the bars can fail: a
bar is max(16 x the error of the fp32 restatement on that case, 4 fp32 ulps of the output's scale) and is asserted to lie below its
ceiling.  Shapes: lane 63 and the top bit of ray_bits (M = 63, 64), the four-ray and the 256-thread workgroup (Nr = 3, 4, 5, 257), the
64-thread workgroup of the backward (Nr = 63, 64, 65), M = 1 and 2, M > 64 (slot loop only).  Every test prints what it measured
before it asserts.

Measured on an MI355X: the largest error over the shapes and both backgrounds, the bar of the case where it fell, the ceiling.
  form (dense = compact, bit for bit)   mask               channels           depth, mask >= 0.05   depth error x mask
  wave                                  1.8e-7 / 1.9e-6    3.2e-7 / 2.6e-6    5.5e-7 / 6.9e-6       1.9e-7 / 1.9e-6
  thread per ray                        4.4e-7 / 1.6e-6    4.2e-7 / 3.0e-6    5.5e-7 / 6.9e-6       2.4e-7 / 2.8e-6
  wave, opaque                          2.3e-8 / 9.8e-7    7.8e-8 / 2.1e-6    1.2e-7 / 1.8e-6       1.2e-7 / 1.8e-6
  thread per ray, opaque                6.1e-8 / 9.8e-7    1.1e-7 / 2.1e-6    1.4e-7 / 1.8e-6       1.4e-7 / 1.8e-6
  fused wave                            1.4e-7 / 2.0e-6    1.1e-7 / 2.5e-6    3.7e-7 / 5.3e-6       2.1e-7 / 2.4e-6
  overflow, wave                        1.3e-7 / 1.8e-6    1.2e-7 / 2.6e-6    3.5e-7 / 6.9e-6       1.9e-7 / 1.9e-6
  overflow, thread per ray              2.1e-7 / 1.8e-6    1.9e-7 / 2.6e-6    3.4e-7 / 6.9e-6       1.9e-7 / 1.9e-6
  ceiling                               5e-6               5e-6               2e-5                  5e-6
  backward                              dsigma                                 drgb
  g_depth = 0                           1.9e-7 / 1.2e-6  (max |ref| 1.0)       1.9e-7 / 2.0e-6
  gated g_depth                         3.0e-7 / 2.8e-6  (max |ref| 1.1)       1.9e-7 / 2.0e-6
  ceiling                               1e-4 max(1, max |ref|)                 5e-6
The limit words, the rays without weight, the two runs of a form and the two layouts of a form agreed to the bit everywhere.
"""
import numpy as np
import pytest
import torch

from test_ray_march_cpu import (ALL_EMPTY, BACKWARD_SHAPES, FORWARD_SHAPES, OPAQUE, backward_bars, backward_errors, cameras, changed,
                                compact_view, fkey, forward_bars, forward_errors, g_depth_runs, march_case, raw_box_limits)

pytestmark = pytest.mark.gpu

ENV = "NPCD_MARCH_PER_THREAD"
ERR_ARG, ERR_UNSUPPORTED = -1, -2
POISON = -7.25
GUARD = 64
f32 = torch.float32


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def on_gpu(case):
    """the case's tensors as the entry points take them; a case without points gets one row that nothing reads"""
    c = {k: v.cuda() for k, v in case.items() if torch.is_tensor(v)}
    c["valid"] = c["valid"].to(torch.uint8).contiguous()
    if case["M"] <= 64:
        c["ray_bits"], c["pts"], _ = (x.cuda() for x in compact_view(case))
    if c["sigma"].numel() == 0:
        c["sigma"], c["rgb"], c["pts"] = torch.zeros(1, device="cuda"), torch.zeros(1, 3, device="cuda"), torch.zeros(1, 3, device="cuda")
    return c


def outputs(Nr):
    from npcd import hip
    n_ws = hip.lib().npcd_ray_march_ws_floats(Nr)
    return [torch.full(shape, POISON, dtype=f32, device="cuda") for shape in ((Nr,), (Nr,), (Nr, 3), (n_ws,))]


def march(c, Nr, M, white_back, layout, out=None, capacity=None, fused=None):
    """one direct call -> (return code, mask, depth, chan, ws); layout: "dense" or "compact"; fused = (t0, lim_part)"""
    from npcd import hip
    L, P = hip.lib(), hip.ptr
    mask, depth, chan, ws = outputs(Nr) if out is None else out
    if layout == "dense":
        rc = L.npcd_ray_march(P(c["sigma"]), P(c["rgb"]), P(c["valid"]), P(c["slot_loc"]), P(c["point_base"]), P(c["o"]), P(c["d"]), P(c["t1"]),
                              Nr, M, int(white_back), P(mask), P(depth), P(chan), P(ws), hip.stream_ptr())
    else:
        cap = c["sigma"].shape[0] if capacity is None else capacity
        head = (P(c["sigma"]), P(c["rgb"]), P(c["ray_bits"]), P(c["pts"]), P(c["point_base"]), P(c["o"]), P(c["d"]))
        tail = (Nr, M, cap, int(white_back), P(mask), P(depth), P(chan), P(ws), hip.stream_ptr())
        if fused is None:
            rc = L.npcd_ray_march_compact(*head, P(c["t1"]), *tail)
        else:
            t0, lim = fused
            rc = L.npcd_ray_march_compact_fused(*head, P(t0), P(c["t1"]), P(lim), lim.numel() // 2, *tail)
    torch.cuda.synchronize()
    return rc, mask, depth, chan, ws


def as_result(mask, depth, chan, ws):
    return {"mask": mask.cpu(), "depth": depth.cpu(), "chan": chan.cpu(), "limits": ws[:2].cpu().view(torch.int32).numpy().view(np.uint32)}


def judge(tag, got, ref, bars):
    """print every figure, then hold the result to the bars, the limits and the rays without weight to the reference's bits"""
    err = forward_errors(got, ref)
    for k in err:
        print(f"FIGURE {tag} | {k} | error {err[k]:.3e} | bar {bars[k]:.3e}")
    for k in err:
        assert err[k] <= bars[k], (tag, k, err[k], bars[k])
    want = np.array([fkey(float(ref["lo"])), fkey(float(ref["hi"]))], dtype=np.uint32)
    assert (got["limits"] == want).all(), (tag, got["limits"], want)
    empty = ref["mask"] == 0
    assert (got["mask"][empty] == 0).all(), tag
    assert (got["chan"][empty] == ref["chan"][empty].float()).all(), tag
    assert same_bits(got["depth"][empty], ref["hi"].expand(int(empty.sum())).contiguous()), tag


def hold_every_form(name, case, white_back, monkeypatch, ref=None):
    Nr, M = case["Nr"], case["M"]
    ref, bars, _ = forward_bars(case, white_back, ref)
    c = on_gpu(case)
    got = {}
    for form in ("wave", "thread"):
        if form == "thread":
            monkeypatch.setenv(ENV, "1")
        else:
            monkeypatch.delenv(ENV, raising=False)
        for layout in ("dense", "compact"):
            if M > 64 and layout == "compact":
                rc, *out = march(changed(c, ray_bits=torch.zeros(Nr, dtype=torch.int64, device="cuda"), pts=c["sigma"]), Nr, M, white_back, layout)
                assert rc in (ERR_ARG, ERR_UNSUPPORTED) and all((t == POISON).all() for t in out), (name, form, "M > 64 must be refused")
                continue
            rc, *out = march(c, Nr, M, white_back, layout)
            assert rc == 0, (name, form, layout, rc)
            got[form, layout] = as_result(*out)
            if form == "wave":
                rc, *again = march(c, Nr, M, white_back, layout)
                assert rc == 0 and all(same_bits(a, b) for a, b in zip(out[:3], again[:3])), (name, layout, "two runs differ")
                assert same_bits(out[3], again[3])
    monkeypatch.delenv(ENV, raising=False)
    for (form, layout), g in got.items():
        judge(f"{name} white_back={white_back} {layout} {form}", g, ref, bars)
    for form in ("wave", "thread"):
        if M <= 64:                                       # one template body: the layouts agree to the bit
            for k in ("mask", "depth", "chan"):
                assert same_bits(got[form, "dense"][k], got[form, "compact"][k]), (name, form, k)
    if M > 64:                                            # the slot loop is the only form there, with the switch or without
        for k in ("mask", "depth", "chan"):
            assert same_bits(got["wave", "dense"][k], got["thread", "dense"][k]), (name, k)
    return got


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("Nr,M", FORWARD_SHAPES)
def test_every_form_against_the_float64_reference(Nr, M, white_back, monkeypatch):
    hold_every_form(f"({Nr},{M})", march_case(Nr, M), white_back, monkeypatch)


@pytest.mark.parametrize("white_back", [True, False])
def test_opaque_rays(white_back, monkeypatch):
    Nr, M, sigma_max = OPAQUE
    hold_every_form("opaque", march_case(Nr, M, sigma_max=sigma_max), white_back, monkeypatch)


def test_every_ray_empty(monkeypatch):
    case = march_case(*ALL_EMPTY, all_empty=True)
    got = hold_every_form("all empty", case, True, monkeypatch)
    want = np.array([fkey(float(case["t1"].min())), fkey(float(case["t1"].max()))], dtype=np.uint32)
    for g in got.values():
        assert (g["limits"] == want).all() and (g["mask"] == 0).all() and (g["chan"] == 1).all()


@pytest.mark.parametrize("form", ["wave", "thread"])
def test_overflowed_lists_march_the_cut_rays_as_empty(form, monkeypatch):
    """the compact lists end inside the last rays' rows: those rays come out as the same case with their slots cleared, every other ray
    keeps its bits, and nothing past the capacity is read -- the arrays end there"""
    Nr, M = 257, 64
    case = march_case(Nr, M)
    count = case["valid"].sum(1)
    capacity = case["sigma"].shape[0] - 40
    cut = (case["point_base"] + count) > capacity
    assert 2 <= int(cut.sum()) < 6 and bool((case["point_base"][cut] < capacity).any())          # one ray straddles the end
    cleared = changed(case, valid=case["valid"] & ~cut[:, None])
    ref, bars, _ = forward_bars(cleared, True)
    c = on_gpu(case)
    if form == "thread":
        monkeypatch.setenv(ENV, "1")
    else:
        monkeypatch.delenv(ENV, raising=False)
    rc, *whole = march(c, Nr, M, True, "compact")
    assert rc == 0
    short = changed(c, sigma=c["sigma"][:capacity].clone(), rgb=c["rgb"][:capacity].clone(), pts=c["pts"][:capacity].clone())
    rc, *out = march(short, Nr, M, True, "compact", capacity=capacity)
    assert rc == 0
    judge(f"overflow compact {form}", as_result(*out), ref, bars)
    keep = (~cut).cuda()
    for a, b in zip(out[:3], whole[:3]):
        assert same_bits(a[keep], b[keep])
    assert (out[0][cut.cuda()] == 0).all()


def limit_pairs(t0, t1):
    """the (min start, max end) keys the query of a fused render leaves per 64 rays; 0xffffffff / 0 where no ray of the group hits"""
    words = []
    for first in range(0, len(t0), 64):
        hit = [(a, b) for a, b in zip(t0[first:first + 64].tolist(), t1[first:first + 64].tolist()) if b > a]
        words += [min((fkey(a) for a, _ in hit), default=0xFFFFFFFF), max((fkey(b) for _, b in hit), default=0)]
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32)).cuda()


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("Nr,M,miss", [(5, 64, (0, 3)), (257, 64, (0, 7, 8, 64, 256))])
def test_fused_march_ends_missed_rays_at_the_global_end(Nr, M, miss, white_back, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    case = march_case(Nr, M, empty_rays=miss)
    t0, t1 = torch.full((Nr,), 0.25), case["t1"].clone()
    t0[list(miss)], t1[list(miss)] = -1.0, -2.0
    raw = changed(case, t1=t1)
    hits = t1 > t0
    fixed = changed(case, t1=torch.where(hits, t1, t1[hits].max()))
    c = on_gpu(raw)
    for name, expect, lim in (("fused", fixed, limit_pairs(t0, t1)), ("fused, no ray hit", raw, limit_pairs(t1, t1))):
        if name == "fused":
            assert bool((lim[1::2] != 0).any()) and (Nr < 257 or int(lim[-1]) == 0)            # (the last group holds one ray, which misses)
        else:
            assert (lim[0::2] == -1).all() and (lim[1::2] == 0).all()
        ref, bars, _ = forward_bars(expect, white_back)
        rc, *out = march(c, Nr, M, white_back, "compact", fused=(t0.cuda(), lim))
        assert rc == 0
        judge(f"{name} ({Nr},{M}) white_back={white_back}", as_result(*out), ref, bars)
        rc, *plain = march(on_gpu(expect), Nr, M, white_back, "compact")                   # the same march with the limits fixed beforehand
        assert rc == 0 and all(same_bits(a, b) for a, b in zip(out[:3], plain[:3]))
    monkeypatch.setenv(ENV, "1")                                                           # no thread-per-ray form of the fused march
    rc, *out = march(c, Nr, M, white_back, "compact", fused=(t0.cuda(), limit_pairs(t0, t1)))
    assert rc == ERR_UNSUPPORTED and all((t == POISON).all() for t in out)


def backward_direct(c, Nr, M, white_back, ws, g_depth, out=None):
    from npcd import hip
    L, P = hip.lib(), hip.ptr
    dsigma, drgb = (torch.full_like(c["sigma"], POISON), torch.full_like(c["rgb"], POISON)) if out is None else out
    rc = L.npcd_ray_march_bwd(P(c["sigma"]), P(c["rgb"]), P(c["valid"]), P(c["slot_loc"]), P(c["point_base"]), P(c["o"]), P(c["d"]), P(c["t1"]),
                              Nr, M, int(white_back), P(ws), P(c["g_mask"]), P(g_depth), P(c["g_chan"]), P(dsigma), P(drgb), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, dsigma, drgb


@pytest.mark.parametrize("white_back", [True, False])
@pytest.mark.parametrize("Nr,M", BACKWARD_SHAPES)
def test_backward_against_float64_autograd(Nr, M, white_back, monkeypatch):
    from npcd.hip import render as hr
    monkeypatch.delenv(ENV, raising=False)
    case = march_case(Nr, M)
    c = on_gpu(case)
    last_only = int(case["point_base"][2 if Nr > 2 else 0]) if Nr != 2 else None
    for name, g_depth in g_depth_runs(case, white_back).items():
        ref, bars, _ = backward_bars(case, white_back, g_depth)
        sigma, rgb = c["sigma"].clone().requires_grad_(True), c["rgb"].clone().requires_grad_(True)
        m, dpt, ch = hr.ray_march_train(sigma, rgb, c["valid"], c["slot_loc"], c["point_base"], c["o"], c["d"], c["t1"], white_back)
        torch.autograd.backward([m, dpt, ch], [c["g_mask"], g_depth.cuda(), c["g_chan"]])
        got = {"dsigma": sigma.grad.cpu(), "drgb": rgb.grad.cpu()}
        err = backward_errors(got, ref)
        for k in err:
            print(f"FIGURE backward ({Nr},{M}) white_back={white_back} {name} | {k} | error {err[k]:.3e} | bar {bars[k]:.3e} "
                  f"| max |ref| {float(ref[k].abs().max()):.3e}")
        for k in err:
            assert err[k] <= bars[k], (name, k, err[k], bars[k])
        if last_only is not None:
            assert float(got["dsigma"][last_only]) == 0.0 and (got["drgb"][last_only] == 0).all()
        # by direct call, twice: the same bits as through autograd
        rc, _, _, _, ws = march(c, Nr, M, white_back, "dense")
        assert rc == 0
        for _ in range(2):
            rc, dsigma, drgb = backward_direct(c, Nr, M, white_back, ws, g_depth.cuda())
            assert rc == 0 and same_bits(dsigma, sigma.grad) and same_bits(drgb, rgb.grad), name


def test_backward_refuses_more_than_64_slots():
    Nr, M = 130, 65
    c = on_gpu(march_case(Nr, M))
    rc, _, _, _, ws = march(c, Nr, M, True, "dense")
    assert rc == 0
    rc, dsigma, drgb = backward_direct(c, Nr, M, True, ws, c["g_depth"])
    assert rc == ERR_UNSUPPORTED and (dsigma == POISON).all() and (drgb == POISON).all()


def arena(counts):
    """-> (buffer, views): `counts` float regions in one poisoned buffer, GUARD floats before, between and after them"""
    total = GUARD + sum(n + GUARD for n in counts)
    buf = torch.full((total,), POISON, dtype=f32, device="cuda")
    views, at = [], GUARD
    for n in counts:
        views.append(buf[at:at + n])
        at += n + GUARD
    return buf, views


def bands_intact(buf, counts):
    band = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
    at = GUARD
    for n in counts:
        band[at:at + n] = False
        at += n + GUARD
    return bool((buf[band] == POISON).all())


@pytest.mark.parametrize("Nr,M", [(5, 64), (257, 64)])
def test_the_entry_points_write_their_outputs_and_nothing_else(Nr, M, monkeypatch):
    """Direct C calls on another stream; the outputs and the scratch (npcd_ray_march_ws_floats(Nr) floats exactly) lie in one poisoned
    arena between guard bands: an element that is not written shows, and so does a write outside."""
    from npcd import hip
    monkeypatch.delenv(ENV, raising=False)
    miss = (0, Nr - 2)
    case = march_case(Nr, M, empty_rays=miss)
    t0, t1 = torch.full((Nr,), 0.25), case["t1"].clone()
    t0[list(miss)], t1[list(miss)] = -1.0, -2.0
    c, cf = on_gpu(case), on_gpu(changed(case, t1=t1))
    lim, t0 = limit_pairs(t0, t1), t0.cuda()
    g_depth = g_depth_runs(case, True)["gated g_depth"].cuda()
    n_ws = hip.lib().npcd_ray_march_ws_floats(Nr)
    assert n_ws == 2 + 2 * ((Nr + 3) // 4)
    P = c["sigma"].shape[0]
    expect = {name: march(cc, Nr, M, True, layout, fused=fu) for name, cc, layout, fu in
              (("dense", c, "dense", None), ("compact", c, "compact", None), ("fused", cf, "compact", (t0, lim)))}
    _, want_dsigma, want_drgb = backward_direct(c, Nr, M, True, expect["dense"][4], g_depth)
    side = torch.cuda.Stream()
    for name, cc, layout, fu in (("dense", c, "dense", None), ("compact", c, "compact", None), ("fused", cf, "compact", (t0, lim))):
        counts = [Nr, Nr, 3 * Nr, n_ws] + ([P, 3 * P] if name == "dense" else [])
        buf, views = arena(counts)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            rc, *out = march(cc, Nr, M, True, layout, out=(views[0], views[1], views[2].view(Nr, 3), views[3]), fused=fu)
            assert rc == 0
            if name == "dense":
                rc, dsigma, drgb = backward_direct(c, Nr, M, True, views[3], g_depth, out=(views[4], views[5].view(P, 3)))
                assert rc == 0
        side.synchronize()
        assert bands_intact(buf, counts), name
        for v in views:
            assert (v != POISON).all(), (name, "an element was not written")
        for a, b in zip(out, expect[name][1:]):
            assert same_bits(a, b), name
        if name == "dense":
            assert same_bits(dsigma, want_dsigma) and same_bits(drgb, want_drgb)


# ------------------------------------------------------------------ npcd_ray_gen_subset -------
RES = 24


def pixel_sets():
    g = torch.Generator().manual_seed(11)
    hundred = torch.randperm(RES * RES, generator=g)[:100]
    hundred[57] = hundred[3]                                                   # a duplicate
    return {"1": torch.tensor([137]), "100 with a duplicate": hundred, "257": torch.randperm(RES * RES, generator=g)[:257]}


@pytest.mark.parametrize("zoom", [1.0, 0.45])
def test_ray_gen_subset_is_the_full_generation_at_the_chosen_pixels(zoom):
    from npcd.hip import render as hr
    extr, intr = (x.cuda() for x in cameras(RES, zoom))
    o, d, t0, t1 = (x.cpu() for x in hr.ray_gen(extr, intr, RES))
    lo, hi = raw_box_limits(o, d)
    hit = hi > lo
    # the classification is the kernel's: hitting rays carry their own limits, the others the limits of those that hit
    assert float((t0 - lo)[hit].abs().max()) < 1e-6 and float((t1 - hi)[hit].abs().max()) < 1e-6
    assert bool(hit.all()) == (zoom == 1.0) and int(hit.sum()) > 0
    assert (t0[~hit] == t0[hit].min()).all() and (t1[~hit] == t1[hit].max()).all()
    sets = pixel_sets()
    if zoom != 1.0:
        assert any(0 < int(hit[:, ids].sum()) < hit[:, ids].numel() for ids in sets.values())
        # a subset that only misses keeps the sentinels (no pixel misses in all three views: one view, the pixels that miss in it)
        v = int((~hit).sum(1).argmax())
        ids = torch.nonzero(~hit[v])[:, 0]
        assert 2 <= len(ids) < RES * RES
        so, sd, s0, s1 = (x.cpu() for x in hr.ray_gen(extr[v:v + 1], intr[v:v + 1], RES, pixel_ids=ids.cuda()))
        assert same_bits(so, o[v:v + 1, ids]) and same_bits(sd, d[v:v + 1, ids]) and (s0 == -1).all() and (s1 == -2).all()
    for name, ids in sets.items():
        so, sd, s0, s1 = (x.cpu() for x in hr.ray_gen(extr, intr, RES, pixel_ids=ids.cuda()))
        assert so.shape == (3, len(ids), 3) and s0.shape == (3, len(ids))
        assert same_bits(so, o[:, ids]) and same_bits(sd, d[:, ids]), name
        h = hit[:, ids]
        assert h.any(), name
        assert same_bits(s0[h], t0[:, ids][h]) and same_bits(s1[h], t1[:, ids][h]), name
        assert (s0[~h] == t0[:, ids][h].min()).all() and (s1[~h] == t1[:, ids][h].max()).all(), name
