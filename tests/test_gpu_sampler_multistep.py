"""Second-order few-step sampling on the GPU: the one-launch multistep step kernel (npcd_sampler_step_multistep, DPM-Solver++ 2M in data
prediction) against float64 and against its first-order parents, the loop around it step by step and under graph replay, the
convergence conditions of tests/test_sampler_multistep_cpu.py on the fused loop, and DiffusionModel.generate(solver=).

Conventions of tests/test_gpu_sampler_steps.py: float64 references computed on the device from the kernel's own inputs, outputs (and
here the history, which the kernel updates in place) between sentinel guard bands, t = (0, one mid-chain level) so that one sample has
w = 0 and the other w > 0, bars from first-order rounding counts with U = 2^-24, a count of n roundings held to (n + 1) U as there.
Read off the kernel (csrc/sampler.hip, sampler_x0 / sampler_element: every rounding is a written-out subtraction, multiply or fused
multiply-add):
    x0  = fma(r, x, -(m eps))                   2 roundings  ->  x0bar = 3 U (|r x| + |m eps|); the clamp is 1-Lipschitz
    D   = fma(w, x0 - hist, x0)                 2 roundings  ->  Dbar  = (1 + |w|) x0bar + 3 U (|x0| + |w (x0 - hist)|); hist is an input
          w = 0: D = x0, nothing is added       0 roundings  ->  Dbar  = x0bar
    out = fma(c1, D, c2 x)                      2 roundings  ->  |c1| Dbar + 3 U (|c1 D| + |c2 x|)
    hold and kept points = fma(h1, k, h2 z)     2 roundings  ->  3 U (|h1 k| + |h2 z|)                      (ref_hold of that file)
"""
import ctypes
import math

import pytest
import torch

from test_gpu_sampler_steps import BF16, F32, SIZE_IDS, SIZES, U, Guarded, _tiny_model, close, gen, randn, ref_hold, ref_reverse
from test_sampler_multistep_cpu import Gaussian, check_convergence

pytestmark = pytest.mark.gpu

CLIPS = ((-1.5, 1.5), (-0.75, 1.0))
NAN = math.nan


def _ew():
    from npcd.hip import elementwise as ew
    return ew


@pytest.fixture(scope="module")
def process():
    from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion().cuda()


@pytest.fixture(scope="module")
def sched50(process):
    """50 logsnr levels with the multistep weights, the DDIM (eta = 0) schedule of the same levels, t = (0, a mid-chain level)"""
    sched = process.sampling_schedule(steps=50, solver="dpmpp2m")
    ddim = process.sampling_schedule(steps=50, eta=0.0, spacing="logsnr")
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")
    assert sched.timesteps[0] == 0 and float(sched.multistep_table[0, 7]) == 0.0 and float(sched.multistep_table[t[1], 7]) > 0.25
    assert ddim.deterministic and torch.equal(ddim.table[t, :7], sched.multistep_table[t, :7])
    return sched, ddim, t


def ref_multistep(table, t, x, eps, hist, clip):
    """float64 single multistep step of a reverse-mode tensor -> (x0, x0 bar, out, out bar).  The history of a sample with w = 0 is
    not part of the expression (it may be NaN)."""
    x0, x0bar, _, _ = ref_reverse(table, t, x, eps, None, clip)
    row = table[t].double()
    c1, c2, w = (row[:, j].reshape((-1,) + (1,) * (x.dim() - 1)) for j in (2, 3, 7))
    first = (w == 0).expand_as(x0)
    ext = torch.where(first, torch.zeros_like(x0), w * (x0 - torch.where(first, torch.zeros_like(x0), hist.double())))
    d = x0 + ext
    dbar = torch.where(first, x0bar, (1 + w.abs()) * x0bar + 3 * U * (x0.abs() + ext.abs()))
    xd = x.double()
    return x0, x0bar, c1 * d + c2 * xd, c1.abs() * dbar + 3 * U * ((c1 * d).abs() + (c2 * xd).abs()) + 1e-300


def _history(g, shape):
    """(the history the kernel gets, guarded; its starting values): random, and NaN for sample 0, whose level has w = 0"""
    start = randn(g, *shape)
    start[0] = NAN
    h = Guarded(shape)
    h.t.copy_(start)
    return h, start


def _same(a, b):
    return torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0))


# =====================================================================================================================================
# 1. the kernel against float64 and against the first-order step
# =====================================================================================================================================
@pytest.mark.parametrize("sizes", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("modes", [("reverse", "reverse"), ("hold", "reverse"), ("reverse", "hold")], ids=["rev_rev", "hold_rev", "rev_hold"])
@pytest.mark.parametrize("with_clip", [True, False], ids=["clip", "no_clip"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_multistep_kernel_against_float64(sched50, dtype, with_clip, modes, sizes):
    ew = _ew()
    sched, ddim, t = sched50
    table = sched.multistep_table
    g = gen(sizes[0] + 7 * len(modes[0]) + 3 * with_clip)
    B = 2
    specs, plain, refs = [], [], []
    for z, (mode, per) in enumerate(zip(modes, sizes)):
        x, eps, known, noise = randn(g, B, per), randn(g, B, per).to(dtype), randn(g, B, per), randn(g, B, per)
        clip = CLIPS[z] if with_clip else None
        out, x0 = Guarded((B, per)), Guarded((B, per))
        hist, start = _history(g, (B, per))
        if mode == "hold":
            specs.append(dict(mode="hold", known=known, noise=noise, out=out.t))
            plain.append(dict(mode="hold", known=known, noise=noise))
        else:
            specs.append(dict(mode="reverse", x_t=x, eps=eps, clip=clip, out=out.t, x0_out=x0.t, hist=hist.t))
            plain.append(dict(mode="reverse", x_t=x, eps=eps, noise=None, clip=clip, want_x0=True))
        refs.append((mode, per, x, eps, known, noise, clip, out, x0, hist, start))
    # the first-order step on the same operands and the same levels
    first_order = [(o.clone(), None if x0 is None else x0.clone()) for o, x0 in ew.sampler_step(plain[0], plain[1], t, ddim.table, True)]
    (oc, x0c), (of, x0f) = ew.sampler_step_multistep(specs[0], specs[1], t, table)
    kept = []
    for name, (mode, per, x, eps, known, noise, clip, out, x0, hist, start), got, got0, (o1, x01) in zip(
            ("coords", "feats"), refs, (oc, of), (x0c, x0f), first_order):
        assert got is out.t
        out.check(f"{name} out")
        if mode == "hold":
            ref, bar = ref_hold(table, t, known, noise)
            close(f"hold {name}[{per}]", out.t, ref, bar)
            assert got0 is None and torch.equal(out.t, o1) and torch.equal(out.t[0], known[0])
            x0.check(f"{name} x0 (hold mode writes none)", written=False)
        else:
            assert got0 is x0.t
            x0.check(f"{name} x0")
            hist.check(f"{name} hist")
            x0r, x0bar, ref, bar = ref_multistep(table, t, x, eps, start, clip)
            close(f"x0 {name}[{per}]", x0.t, x0r, x0bar)
            close(f"out {name}[{per}]", out.t, ref, bar)
            assert torch.equal(x0.t, x01), f"{name}: x0 differs from npcd_sampler_step's"
            assert torch.equal(hist.t, x0.t), f"{name}: the history after the call is not x0"
            # w = 0 (sample 0, whose history is NaN): the bits of the first-order step; w > 0: the step did extrapolate
            assert torch.equal(out.t[0], o1[0]), f"{name}: a row with w = 0 differs from NPCD_SAMPLER_REVERSE with `deterministic`"
            assert not torch.equal(out.t[1], o1[1])
            if clip is not None:
                assert float(hist.t.min()) >= clip[0] and float(hist.t.max()) <= clip[1]
        kept.append((out.t.clone(), x0.t.clone(), hist.t.clone()))
        if mode != "hold":
            hist.t.copy_(start)                                               # restored: the same bits twice
    ew.sampler_step_multistep(specs[0], specs[1], t, table)
    for (o1, z1, h1), (mode, _, _, _, _, _, _, out, x0, hist, _) in zip(kept, refs):
        assert torch.equal(out.t, o1) and _same(x0.t, z1) and _same(hist.t, h1)
        out.check("second call out")
        if mode != "hold":
            hist.check("second call hist")


# =====================================================================================================================================
# 2. masks
# =====================================================================================================================================
# (channels, n_points) of coords and of feats: the smallest 16-byte case; one element per lane (mask rows not 4-byte addressable); the
# protocol's shape; feats past the grid cap of the 16-byte loop (32 x 32800 = 1,049,600 > 1,048,576), coords one element per lane
MASK_SHAPES = [((3, 4), (32, 4)), ((3, 509), (32, 509)), ((3, 512), (32, 512)), ((3, 100001), (32, 32800))]


def _mask(g, B, N):
    m = torch.rand(B, N, device="cuda", generator=g) < 0.5
    m[:, 0], m[:, 1] = True, False
    return m


@pytest.mark.parametrize("shapes", MASK_SHAPES, ids=["vec_min", "scalar_509", "protocol_512", "past_cap"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_masked_multistep_is_a_select_of_hold_and_the_unmasked_step(sched50, dtype, shapes):
    """Kept points: the bits of the hold mode on `known`; free points: the bits of the unmasked multistep call; x0_out and the
    history: `known` at kept points.  The masked call gets NaN wherever it must not read: `known` at free points, x_t / eps / hist at
    kept points (and the whole history of sample 0, w = 0)."""
    ew = _ew()
    sched, ddim, t = sched50
    table = sched.multistep_table
    B = 2
    g = gen(shapes[0][1] + 11)
    one_n = shapes[0][1] == shapes[1][1]
    masks = [_mask(g, B, shapes[0][1])]
    masks.append(masks[0] if one_n else _mask(g, B, shapes[1][1]))
    byte_masks = [m.to(torch.uint8) * 173 if dtype == BF16 else m for m in masks]       # a byte mask: any non-zero value keeps
    clean, dirty = [], []
    for (C, N), mask in zip(shapes, masks):
        m3 = mask[:, None, :]
        x, eps, known, noise, hist = randn(g, B, C, N), randn(g, B, C, N).to(dtype), randn(g, B, C, N), randn(g, B, C, N), randn(g, B, C, N)
        nan = torch.full_like(x, NAN)
        clean.append((x, eps, known, noise, hist))
        dh = torch.where(m3, nan, hist)
        dh[0] = NAN
        dirty.append((torch.where(m3, nan, x), torch.where(m3, nan.to(dtype), eps), torch.where(m3, known, nan), noise, dh))
    hold = [o.clone() for o, _ in ew.sampler_step(*[dict(mode="hold", known=c[2], noise=c[3]) for c in clean], t, ddim.table, True)]
    free_hist = [c[4].clone() for c in clean]
    free = [(o.clone(), x0.clone()) for o, x0 in ew.sampler_step_multistep(
        *[dict(x_t=c[0], eps=c[1], clip=cl, want_x0=True, hist=h) for c, cl, h in zip(clean, CLIPS, free_hist)], t, table)]
    # a launch has one n_points: where the two tensors differ in it, each is masked in a launch of its own, beside the other without a mask
    for plan in [(True, True)] if one_n else [(True, False), (False, True)]:
        outs = [(Guarded((B,) + s), Guarded((B,) + s), Guarded((B,) + s)) for s in shapes]
        for masked, (_, _, h), c, d in zip(plan, outs, clean, dirty):
            h.t.copy_(d[4] if masked else c[4])
        specs = [dict(mode="keep", x_t=d[0], eps=d[1], known=d[2], noise=d[3], keep=bm, clip=cl, out=o.t, x0_out=x0.t, hist=h.t) if masked else
                 dict(x_t=c[0], eps=c[1], clip=cl, out=o.t, x0_out=x0.t, hist=h.t)
                 for masked, c, d, bm, cl, (o, x0, h) in zip(plan, clean, dirty, byte_masks, CLIPS, outs)]
        ew.sampler_step_multistep(specs[0], specs[1], t, table)
        for name, masked, mask, (x, eps, known, noise, hist), cl, (o, x0, h), oh, (om, x0m), fh in zip(
                ("coords", "feats"), plan, masks, clean, CLIPS, outs, hold, free, free_hist):
            m3 = mask[:, None, :]
            for buf, what in ((o, "out"), (x0, "x0"), (h, "hist")):
                buf.check(f"{name} {what}")
            if not masked:
                assert torch.equal(o.t, om) and torch.equal(x0.t, x0m) and torch.equal(h.t, x0m), f"{name}: without a mask, not the unmasked call"
                continue
            assert 0 < int(m3.sum()) < m3.numel()
            assert torch.equal(o.t, torch.where(m3, oh, om)), f"{name}: out is not where(mask, hold, multistep)"
            assert torch.equal(x0.t, torch.where(m3, known, x0m)), f"{name}: x0 is not where(mask, known, x0)"
            assert torch.equal(h.t, x0.t) and torch.equal(fh, x0m), f"{name}: the history after the call is not x0"
            href, hbar = ref_hold(table, t, known, noise)
            _, _, rref, rbar = ref_multistep(table, t, x, eps, hist, cl)
            close(f"masked {name}{tuple(x.shape[1:])}", o.t, torch.where(m3, href, rref), torch.where(m3, hbar, rbar))
            k0 = m3[0].expand_as(o.t[0])
            assert torch.equal(o.t[0][k0], known[0][k0])                      # the step to the data: the known values themselves


def test_one_masked_tensor_beside_a_held_and_a_plain_one(sched50):
    """coords masked with the mask at an odd address (n_points a multiple of 4, yet one element per lane), feats in hold mode and
    then in reverse mode without a mask: each tensor has the bits of its own call."""
    ew = _ew()
    sched, ddim, t = sched50
    table = sched.multistep_table
    B, N, g = 2, 512, gen(79)
    mask = _mask(g, B, N)
    m3 = mask[:, None, :]
    odd = torch.zeros(B * N + 1, dtype=torch.bool, device="cuda")[1:].view(B, N).copy_(mask)
    assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    xc, ec, kc, zc, hc = (randn(g, B, 3, N) for _ in range(5))
    xf, ef, kf, zf, hf = (randn(g, B, 32, N) for _ in range(5))
    both = ew.sampler_step_multistep(dict(mode="keep", x_t=xc, eps=ec, known=kc, noise=zc, keep=mask, clip=CLIPS[0], hist=hc.clone()),
                                     dict(x_t=xf, eps=ef, clip=CLIPS[1], hist=hf.clone()), t, table)
    want_c, want_f = both[0][0].clone(), both[1][0].clone()
    held = ew.sampler_step(dict(mode="hold", known=kc, noise=zc), dict(mode="hold", known=kf, noise=zf), t, ddim.table, True)[1][0].clone()
    for other in ("hold", "reverse"):
        oc, of, h1, h2 = Guarded((B, 3, N)), Guarded((B, 32, N)), hc.clone(), hf.clone()
        fspec = dict(mode="hold", known=kf, noise=zf, out=of.t) if other == "hold" else dict(x_t=xf, eps=ef, clip=CLIPS[1], out=of.t, hist=h2)
        ew.sampler_step_multistep(dict(mode="keep", x_t=xc, eps=ec, known=kc, noise=zc, keep=odd, clip=CLIPS[0], out=oc.t, hist=h1), fspec, t, table)
        oc.check("coords")
        of.check("feats")
        assert torch.equal(oc.t, want_c) and torch.equal(of.t, held if other == "hold" else want_f)
        assert torch.equal(h1[m3.expand_as(kc)], kc[m3.expand_as(kc)])
        assert torch.equal(h2, hf) == (other == "hold")                       # a held tensor has no history: nothing wrote it


# =====================================================================================================================================
# 3. refusals
# =====================================================================================================================================
def test_multistep_step_refuses_before_any_launch(sched50):
    """A missing history, a missing operand of a held or a masked tensor, an eps type the kernel does not take, an n_points that does
    not divide per_sample: the documented code, and nothing is launched (the guarded outputs and histories stay NaN)."""
    from npcd import hip
    ew = _ew()
    sched, _, t = sched50
    table = sched.multistep_table
    g = gen(5)
    B, N = 2, 512
    mask = _mask(g, B, N)
    xc, ec, zc, kc = (randn(g, B, 3, N) for _ in range(4))
    xf, ef, zf, kf = (randn(g, B, 32, N) for _ in range(4))
    oc, of, hc, hf = Guarded((B, 3, N)), Guarded((B, 32, N)), Guarded((B, 3, N)), Guarded((B, 32, N))
    plain_c, plain_f = dict(x_t=xc, eps=ec, out=oc.t, hist=hc.t), dict(x_t=xf, eps=ef, out=of.t, hist=hf.t)
    full_c = dict(mode="keep", x_t=xc, eps=ec, noise=zc, known=kc, keep=mask, out=oc.t, hist=hc.t)
    full_f = dict(mode="keep", x_t=xf, eps=ef, noise=zf, known=kf, keep=mask, out=of.t, hist=hf.t)

    def untouched():
        torch.cuda.synchronize()
        for buf, name in ((oc, "coords out"), (of, "feats out"), (hc, "coords hist"), (hf, "feats hist")):
            buf.check(name, written=False)

    cases = [(dict(plain_c, hist=None), plain_f), (plain_c, dict(plain_f, hist=None)),
             (dict(full_c, hist=None), full_f), (full_c, dict(full_f, hist=None)),
             (dict(plain_c, eps=None), plain_f), (plain_c, dict(plain_f, x_t=None, eps=ef)),
             (dict(mode="hold", known=None, noise=zc, out=oc.t), plain_f), (plain_c, dict(mode="hold", known=kf, noise=None, out=of.t))]
    cases += [(dict(full_c, **{missing: None}), plain_f) for missing in ("eps", "noise", "known")]
    cases += [(plain_c, dict(full_f, **{missing: None})) for missing in ("eps", "noise", "known")]
    for c, f in cases:
        with pytest.raises(RuntimeError, match=r"npcd_sampler_step_multistep failed.*code -1"):
            ew.sampler_step_multistep(c, f, t, table)
        untouched()
    for c, f in ((dict(plain_c, eps=ec.half()), plain_f), (full_c, dict(full_f, eps=ef.half()))):
        with pytest.raises(RuntimeError, match=r"npcd_sampler_step_multistep failed.*code -2"):
            ew.sampler_step_multistep(c, f, t, table)
        untouched()
    with pytest.raises(RuntimeError, match="hist"):                            # the wrapper: a history of another size or type
        ew.sampler_step_multistep(dict(plain_c, hist=hf.t), plain_f, t, table)
    with pytest.raises(RuntimeError, match="hist"):
        ew.sampler_step_multistep(plain_c, dict(plain_f, hist=hf.t.double()), t, table)
    untouched()
    # the C entry itself: n_points the wrapper would derive from the mask
    rc, _, _, mc, keep_c = ew._sampler_tensor(full_c, B)
    rf, _, _, mf, keep_f = ew._sampler_tensor(full_f, B)
    L = hip.lib()

    def call(n, h_c=hc.t):
        return L.npcd_sampler_step_multistep(ctypes.byref(rc), ctypes.byref(rf), hip.ptr(h_c), hip.ptr(hf.t), hip.ptr(mc), hip.ptr(mf), n,
                                             hip.ptr(t), hip.ptr(table), table.shape[0], B, hip.stream_ptr())

    assert call(0) == -1 and call(-4) == -1
    assert call(5) == -1                                                       # 3 * 512 and 32 * 512 are no multiples of 5
    assert call(1024) == -1                                                    # divides 32 * 512, not 3 * 512
    assert call(N, h_c=None) == -1
    untouched()
    hc.t.zero_()                                                               # sample 1 has w > 0 and reads its history
    hf.t.zero_()
    assert call(N) == 0                                                        # the same records, complete, run
    torch.cuda.synchronize()
    for buf, name in ((oc, "coords out"), (of, "feats out"), (hc, "coords hist"), (hf, "feats hist")):
        buf.check(name)
    del keep_c, keep_f


# =====================================================================================================================================
# 4. the loop
# =====================================================================================================================================
def _loop_case():
    m = _tiny_model()
    g = gen(31)
    c0, f0, kc = randn(g, 2, 3, 48), randn(g, 2, 32, 48), randn(g, 2, 3, 48) * 0.8
    mask = _mask(g, 2, 48)
    return m, c0, f0, kc, mask


@pytest.mark.parametrize("masked", [False, True], ids=["free", "keep_coords"])
def test_loop_is_one_multistep_launch_per_step_eager_and_replayed(monkeypatch, masked):
    """The tiny model at K = 6 logsnr levels: p_sample_loop(solver="dpmpp2m") is a loop of ew.sampler_step_multistep calls composed
    here by hand, bit for bit; graph replay gives the bits of the eager loop; one multistep launch per step and no npcd_sampler_step
    launch."""
    ew = _ew()
    K = 6
    clip_c, clip_f = (-3.0, 3.0), (-1.0, 1.0)
    m, c0, f0, kc, mask = _loop_case()
    process = m.diffusion_process
    sched = process.sampling_schedule(steps=K, solver="dpmpp2m", device=c0.device)
    assert sched.spacing == "logsnr" and int((sched.multistep_table[:, 7] > 0).sum()) == K - 2
    keep = {"coords": (kc, mask)} if masked else None
    count = {"multistep": 0, "step": 0}
    real_m, real_s = ew.sampler_step_multistep, ew.sampler_step
    monkeypatch.setattr(ew, "sampler_step_multistep", lambda *a, **kw: (count.__setitem__("multistep", count["multistep"] + 1), real_m(*a, **kw))[1])
    monkeypatch.setattr(ew, "sampler_step", lambda *a, **kw: (count.__setitem__("step", count["step"] + 1), real_s(*a, **kw))[1])
    torch.manual_seed(123)
    with torch.no_grad():
        c_end, f_end = process.p_sample_loop(m.denoiser, c0, f0, clip_c, clip_f, steps=K, solver="dpmpp2m", keep=keep)
    assert count == {"multistep": K, "step": 0}
    # by hand, replaying the generator: a tensor with a mask draws once per step, a reverse-mode tensor never
    torch.manual_seed(123)
    t = torch.full((2,), int(sched.timesteps[-1]), device="cuda", dtype=torch.long)
    c, f = c0, f0
    if masked:
        c = torch.where(mask[:, None, :], process.q_sample(kc, t, c0), c0)
    hc, hf = torch.full_like(c0, NAN), torch.full_like(f0, NAN)                # the first step reads no history
    with torch.no_grad():
        for lv in [int(i) for i in sched.timesteps[::-1]]:
            t.fill_(lv)
            ec, ef = m.denoiser(c, f, t)
            if masked:
                spec_c = dict(mode="keep", x_t=c, eps=ec, noise=torch.randn_like(c), known=kc, keep=mask, clip=clip_c, hist=hc)
            else:
                spec_c = dict(x_t=c, eps=ec, clip=clip_c, hist=hc)
            (c, _), (f, _) = real_m(spec_c, dict(x_t=f, eps=ef, clip=clip_f, hist=hf), t, sched.multistep_table)
    assert torch.equal(c_end, c) and torch.equal(f_end, f)
    assert bool(torch.isfinite(c_end).all()) and bool(torch.isfinite(f_end).all())
    if masked:
        m3 = mask[:, None, :].expand_as(kc)
        assert torch.equal(c_end[m3], kc[m3])
    # graph replay: the same bits as eager, one captured launch
    count.update(multistep=0, step=0)
    torch.manual_seed(123)
    with torch.no_grad():
        c_g, f_g = process.p_sample_loop(m.denoiser, c0, f0, clip_c, clip_f, steps=K, solver="dpmpp2m", keep=keep, use_graph=True)
    assert torch.equal(c_g, c_end) and torch.equal(f_g, f_end)
    assert count == {"multistep": 3, "step": 0}                                # two warm-up steps and the captured one


def test_loop_holds_a_tensor_beside_the_multistep_one():
    m, c0, f0, kc, _ = _loop_case()
    out = []
    for use_graph in (False, True):
        torch.manual_seed(9)
        with torch.no_grad():
            out.append(m.diffusion_process.p_sample_loop(m.denoiser, c0, f0, (-3.0, 3.0), (-1.0, 1.0), steps=6, solver="dpmpp2m",
                                                         hold=("coords", kc), use_graph=use_graph))
        assert torch.equal(out[-1][0], kc) and bool(torch.isfinite(out[-1][1]).all())
    assert torch.equal(out[0][1], out[1][1])


def test_second_order_convergence_on_the_device(process, monkeypatch):
    """The analytic Gaussian denoiser of tests/test_sampler_multistep_cpu.py as an fp32 torch callable on the device, the fused
    loop (one npcd_sampler_step_multistep launch per step), the same data and the same two conditions.  fp32 round-off is about
    1e-6, against solver errors of 1e-3 and more."""
    ew = _ew()
    launches = []
    real = ew.sampler_step_multistep
    monkeypatch.setattr(ew, "sampler_step_multistep", lambda *a, **kw: (launches.append(1), real(*a, **kw))[1])
    check_convergence(process, Gaussian(process, dtype=F32, device="cuda"))
    assert len(launches) == 10 + 20 + 40


# =====================================================================================================================================
# 5. the model
# =====================================================================================================================================
def test_generate_with_the_multistep_solver_eager_and_replayed():
    m = _tiny_model()
    out = []
    for use_graph in (False, True):
        torch.manual_seed(4)
        coords, feats = m.generate(8, batch_size=4, progress=False, sampling_steps=5, solver="dpmpp2m", use_graph=use_graph)
        assert len(coords) == 8 and len(feats) == 8 and coords[0].shape == (3, 48) and feats[0].shape == (32, 48)
        assert all(bool(torch.isfinite(x).all()) for x in coords + feats)
        assert float(torch.stack(coords).abs().max()) <= 3.0 + 1e-5 and float(torch.stack(feats).abs().max()) <= 1.0 + 1e-5
        out.append((torch.stack(coords), torch.stack(feats)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    torch.manual_seed(4)
    ddim = m.generate(8, batch_size=4, progress=False, sampling_steps=5, eta=0.0, spacing="logsnr")
    assert not torch.equal(torch.stack(ddim[0]), out[0][0])
    torch.manual_seed(4)
    bf = m.generate(8, batch_size=4, progress=False, sampling_steps=5, solver="dpmpp2m", dtype=torch.bfloat16, use_graph=True)
    assert all(bool(torch.isfinite(x).all()) for x in bf[0] + bf[1]) and float(torch.stack(bf[0]).abs().max()) <= 3.0 + 1e-5
    with pytest.raises(ValueError):
        m.generate(8, batch_size=4, progress=False, sampling_steps=5, solver="dpmpp2m", eta=1.0)
    with pytest.raises(ValueError):
        m.generate(8, batch_size=4, progress=False, sampling_steps=5, solver="dpmpp2m", resample=2)


def test_sample_and_render_passes_the_solver_through():
    from npcd.eval import load_test_poses, sample_and_render
    from npcd.models import NPCD
    poses, intr = load_test_poses("srncars")
    torch.manual_seed(0)
    net = NPCD(n_obj=1, coords_dim=3, feats_dim=32, num_points=512, use_view_dir=False, width=128, layers=2, heads=2).cuda().eval()
    with torch.no_grad():
        net.diffusion.coords_normalization.min.fill_(-2.5); net.diffusion.coords_normalization.max.fill_(2.5)
        net.diffusion.coords_normalization.scale.fill_(0.25)
        net.diffusion.feats_normalization.min.fill_(-1.0); net.diffusion.feats_normalization.max.fill_(1.0)
    seen = []
    real = net.diffusion.diffusion_process.p_sample_loop
    net.diffusion.diffusion_process.p_sample_loop = lambda *a, **kw: (seen.append((kw.get("steps"), kw.get("eta"), kw.get("spacing"),
                                                                                   kw.get("solver"))), real(*a, **kw))[1]
    res = sample_and_render(net, poses[:2], intr[:2], num_samples=2, generate_batch_size=2, render_batch_size=2, resolution=16,
                            sampling_steps=3, solver="dpmpp2m", spacing="logsnr")
    assert seen == [(3, None, "logsnr", "dpmpp2m")]
    assert res["clouds"] == 2 and res["poses_per_cloud"] == 2 and res["image_batch_shape"] == (2, 3, 16, 16)
