"""Per-point conditioning of the scheduled sampler on the GPU: the masked step kernel (npcd_sampler_step_keep) against its two parents
(the hold and the reverse mode of npcd_sampler_step on the same operands) and against float64, the loop with masks and resampling
against the same loop composed by hand, the completion toy of tests/test_sampler_keep_cpu.py on the device, and
DiffusionModel.generate with masks.

Conventions and bars of tests/test_gpu_sampler_steps.py: guarded outputs that start as NaN, t = (0, one mid-chain level), the rounding
counts of sampler_x0 / sampler_element (csrc/sampler.hip).  The masked kernel evaluates the two parents' expressions and selects, so the bar
of an element is its parent's.
"""
import ctypes
import math

import pytest
import torch

from test_gpu_sampler_steps import BF16, F32, Guarded, _tiny_model, close, gen, randn, ref_hold, ref_reverse
from test_sampler_keep_cpu import _stub, pair_slope

pytestmark = pytest.mark.gpu

# (channels, n_points) of coords and of feats: the smallest vector case; the scalar path, where the mask rows are not 4-byte addressable;
# the protocol's shape; past the 1024-workgroup cap on the scalar (coords) and the vector (feats) path
SHAPES = [((3, 4), (32, 4)), ((3, 509), (32, 509)), ((3, 512), (32, 512)), ((3, 100001), (32, 32800))]
IDS = ["vec_min", "scalar_509", "protocol_512", "past_cap"]
CLIPS = ((-1.5, 1.5), (-0.75, 1.0))


def _ew():
    from npcd.hip import elementwise as ew
    return ew


@pytest.fixture(scope="module")
def process():
    from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion().cuda()


def _operands(g, B, shape, dtype, mask):
    """clean operands of one tensor and the poisoned ones the masked kernel gets: NaN in `known` at free points, in x_t / eps at kept"""
    C, N = shape
    x, eps, known, noise = randn(g, B, C, N), randn(g, B, C, N).to(dtype), randn(g, B, C, N), randn(g, B, C, N)
    m3 = mask.bool()[:, None, :]
    nan = torch.full_like(x, math.nan)
    return (x, eps, known, noise), (torch.where(m3, nan, x), torch.where(m3, nan.to(dtype), eps), torch.where(m3, known, nan), noise)


def _parents(ew, sched, t, ops, clips, with_noise):
    """out_hold, out_reverse, x0_reverse of both tensors from npcd_sampler_step on the clean operands"""
    res = []
    hold = ew.sampler_step(*[dict(mode="hold", known=o[2], noise=o[3]) for o in ops], t, sched.table, sched.deterministic)
    rev = ew.sampler_step(*[dict(mode="reverse", x_t=o[0], eps=o[1], noise=o[3] if with_noise else None, clip=cl, want_x0=True)
                            for o, cl in zip(ops, clips)], t, sched.table, sched.deterministic)
    for (oh, _), (orv, x0) in zip(hold, rev):
        res.append((oh.clone(), orv.clone(), x0.clone()))
    return res


# =====================================================================================================================================
# 1. the kernel
# =====================================================================================================================================
@pytest.mark.parametrize("shapes", SHAPES, ids=IDS)
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "no_noise"])
@pytest.mark.parametrize("with_clip", [True, False], ids=["clip", "no_clip"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_masked_step_is_a_select_of_its_two_parents(process, dtype, with_clip, with_noise, shapes):
    ew = _ew()
    sched = process.sampling_schedule(steps=50, eta=0.5 if with_noise else 0.0)
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")
    assert sched.deterministic == (not with_noise)
    B = 2
    g = gen(shapes[0][1] + 3 * with_clip + 5 * with_noise)
    masks = [torch.rand(B, shape[1], device="cuda", generator=g) < 0.5 for shape in shapes]
    if dtype == BF16:                                                          # a byte mask: any non-zero value keeps
        masks = [m.to(torch.uint8) * 173 for m in masks]
    clips = CLIPS if with_clip else (None, None)
    both = [_operands(g, B, shape, dtype, m) for shape, m in zip(shapes, masks)]
    clean, dirty = [b[0] for b in both], [b[1] for b in both]
    parents = _parents(ew, sched, t, clean, clips, with_noise)
    # a launch has one n_points: where the two tensors differ in it, each is masked in a launch of its own, beside the other in reverse mode
    plans = [(True, True)] if shapes[0][1] == shapes[1][1] else [(True, False), (False, True)]
    for plan in plans:
        outs = [(Guarded((B,) + shape), Guarded((B,) + shape)) for shape in shapes]
        specs = [dict(mode="keep", x_t=d[0], eps=d[1], known=d[2], noise=d[3], keep=m, clip=cl, out=o.t, x0_out=x0.t) if masked else
                 dict(mode="reverse", x_t=c[0], eps=c[1], noise=c[3] if with_noise else None, clip=cl, out=o.t, x0_out=x0.t)
                 for masked, c, d, m, cl, (o, x0) in zip(plan, clean, dirty, masks, clips, outs)]
        got = ew.sampler_step(specs[0], specs[1], t, sched.table, sched.deterministic)
        first = []
        for name, masked, (x, eps, known, noise), m, cl, (o, x0), (oh, orv, x0r), (go, gx0) in zip(("coords", "feats"), plan, clean, masks, clips,
                                                                                                    outs, parents, got):
            assert go is o.t and gx0 is x0.t
            o.check(f"{name} out")
            x0.check(f"{name} x0")
            first.append((o.t.clone(), x0.t.clone()))
            if not masked:
                assert torch.equal(o.t, orv) and torch.equal(x0.t, x0r), f"{name}: without a mask, not the bits of npcd_sampler_step"
                continue
            m3 = m.bool()[:, None, :]
            assert 0 < int(m3.sum()) < m3.numel()
            assert torch.equal(o.t, torch.where(m3, oh, orv)), f"{name}: out is not where(mask, hold, reverse)"
            assert torch.equal(x0.t, torch.where(m3, known, x0r)), f"{name}: x0 is not where(mask, known, x0 of reverse)"
            # against float64, each element under its parent's bar
            href, hbar = ref_hold(sched.table, t, known, noise)
            _, _, rref, rbar = ref_reverse(sched.table, t, x, eps, noise if with_noise else None, cl)
            close(f"masked {name}{tuple(x.shape[1:])}", o.t, torch.where(m3, href, rref), torch.where(m3, hbar, rbar))
            kept0 = m3[0].expand_as(o.t[0])
            assert torch.equal(o.t[0][kept0], known[0][kept0])                # last step: the known values themselves
        ew.sampler_step(specs[0], specs[1], t, sched.table, sched.deterministic)   # the same bits twice
        for (o1, z1), (o, x0) in zip(first, outs):
            assert torch.equal(o.t, o1) and torch.equal(x0.t, z1)
            o.check("second call out")
            x0.check("second call x0")


@pytest.mark.parametrize("other", ["reverse", "hold"])
def test_a_tensor_without_a_mask_follows_its_mode(process, other):
    """coords masked, feats by its mode, and the other way round: the unmasked tensor has the bits of npcd_sampler_step.  The feats
    mask lies at an odd address: n_points is a multiple of 4, yet the four mask bytes cannot be read at once (one element per lane)."""
    ew = _ew()
    sched = process.sampling_schedule(steps=50, eta=0.5)
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")
    B, shapes, g = 2, SHAPES[2], gen(77)
    mask = torch.rand(B, 512, device="cuda", generator=g) < 0.5
    both = [_operands(g, B, shape, F32, mask) for shape in shapes]
    clean, dirty = [b[0] for b in both], [b[1] for b in both]
    parents = _parents(ew, sched, t, clean, CLIPS, True)
    odd = torch.zeros(B * 512 + 1, dtype=torch.bool, device="cuda")[1:].view(B, 512).copy_(mask)
    assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    for masked in (0, 1):
        outs = [(Guarded((B,) + shape), Guarded((B,) + shape)) for shape in shapes]
        specs = []
        for z, (c, d, cl, (o, x0)) in enumerate(zip(clean, dirty, CLIPS, outs)):
            if z == masked:
                specs.append(dict(mode="keep", x_t=d[0], eps=d[1], known=d[2], noise=d[3], keep=odd if z else mask, clip=cl, out=o.t,
                                  x0_out=x0.t))
            elif other == "hold":
                specs.append(dict(mode="hold", known=c[2], noise=c[3], out=o.t))
            else:
                specs.append(dict(mode="reverse", x_t=c[0], eps=c[1], noise=c[3], clip=cl, out=o.t, x0_out=x0.t))
        ew.sampler_step(specs[0], specs[1], t, sched.table, sched.deterministic)
        m3 = mask[:, None, :]
        for z, ((o, x0), (oh, orv, x0r), c) in enumerate(zip(outs, parents, clean)):
            o.check(f"tensor {z} out")
            if z == masked:
                assert torch.equal(o.t, torch.where(m3, oh, orv)) and torch.equal(x0.t, torch.where(m3, c[2], x0r))
            elif other == "hold":
                assert torch.equal(o.t, oh)
                x0.check(f"tensor {z} x0 (hold mode writes none)", written=False)
            else:
                assert torch.equal(o.t, orv) and torch.equal(x0.t, x0r)


def test_masked_step_refuses_before_any_launch(process):
    """A missing operand of a masked tensor, n_points = 0 and a per_sample that n_points does not divide: NPCD_ERR_ARG, and nothing is
    launched (the guarded outputs stay NaN)."""
    from npcd import hip
    ew = _ew()
    g = gen(5)
    B, N = 2, 512
    sched = process.sampling_schedule(steps=50, eta=0.5)
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")
    mask = torch.rand(B, N, device="cuda", generator=g) < 0.5
    xc, ec, zc, kc = (randn(g, B, 3, N) for _ in range(4))
    xf, ef, zf, kf = (randn(g, B, 32, N) for _ in range(4))
    oc, of = Guarded((B, 3, N)), Guarded((B, 32, N))
    full_c = dict(mode="keep", x_t=xc, eps=ec, noise=zc, known=kc, keep=mask, out=oc.t)
    full_f = dict(mode="keep", x_t=xf, eps=ef, noise=zf, known=kf, keep=mask, out=of.t)
    plain_f = dict(x_t=xf, eps=ef, noise=zf, out=of.t)

    def untouched():
        torch.cuda.synchronize()
        oc.check("coords", written=False)
        of.check("feats", written=False)

    for missing in ("eps", "noise", "known"):
        for c, f in ((dict(full_c, **{missing: None}), full_f), (full_c, dict(full_f, **{missing: None})), (dict(full_c, **{missing: None}), plain_f)):
            with pytest.raises(RuntimeError, match=r"npcd_sampler_step_keep failed.*code -1"):
                ew.sampler_step(c, f, t, sched.table, sched.deterministic)
            untouched()
    with pytest.raises(RuntimeError, match=r"npcd_sampler_step_keep failed.*code -1"):   # the unmasked tensor's own rules still hold
        ew.sampler_step(full_c, dict(plain_f, noise=None), t, sched.table, sched.deterministic)
    untouched()
    with pytest.raises(RuntimeError, match=r"code -2"):                        # an eps type the kernel does not take
        ew.sampler_step(dict(full_c, eps=ec.half()), full_f, t, sched.table, sched.deterministic)
    untouched()
    # the C entry itself: x_t missing, n_points = 0, n_points that does not divide per_sample (the wrapper derives both from the mask)
    rc, _, _, mc, keep_c = ew._sampler_tensor(full_c, B)
    rf, _, _, mf, keep_f = ew._sampler_tensor(full_f, B)
    L = hip.lib()

    def call(rc_, rf_, mc_, mf_, n):
        return L.npcd_sampler_step_keep(ctypes.byref(rc_), ctypes.byref(rf_), hip.ptr(mc_), hip.ptr(mf_), n, hip.ptr(t), hip.ptr(sched.table),
                                        sched.table.shape[0], B, 0, hip.stream_ptr())

    assert call(rc, rf, mc, mf, 0) == -1
    assert call(rc, rf, mc, None, 0) == -1
    assert call(rc, rf, mc, mf, -4) == -1
    assert call(rc, rf, mc, mf, 5) == -1                                       # 3 * 512 and 32 * 512 are no multiples of 5
    assert call(rc, rf, mc, mf, 1024) == -1                                    # divides 32 * 512, not 3 * 512
    saved, rc.x_t = rc.x_t, 0
    assert call(rc, rf, mc, mf, N) == -1
    rc.x_t = saved
    untouched()
    assert call(rc, rf, mc, mf, N) == 0                                        # the same records, complete, run
    torch.cuda.synchronize()
    oc.check("coords")
    of.check("feats")
    del keep_c, keep_f


# =====================================================================================================================================
# 2. the loop
# =====================================================================================================================================
def _loop_case():
    B, N = 2, 512
    g = gen(31)
    c0, f0, kc, kf = randn(g, B, 3, N), randn(g, B, 32, N), randn(g, B, 3, N) * 0.8, randn(g, B, 32, N) * 0.5
    mc, mf = torch.rand(B, N, device="cuda", generator=g) < 0.5, torch.rand(B, N, device="cuda", generator=g) < 0.3
    return c0, f0, kc, kf, mc, mf


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_loop_with_masks_and_resampling_is_the_loop_composed_by_hand(process, eta):
    ew = _ew()
    K, r = 4, 2
    clip_c, clip_f = (-3.0, 3.0), (-1.0, 1.0)
    c0, f0, kc, kf, mc, mf = _loop_case()
    sched = process.sampling_schedule(steps=K, eta=eta)
    keep = {"coords": (kc, mc), "feats": (kf, mf)}
    torch.manual_seed(123)
    with torch.no_grad():
        c_end, f_end = process.p_sample_loop(_stub, c0, f0, clip_c, clip_f, steps=K, eta=eta, keep=keep, resample=r)
    # by hand, replaying the generator: per performance coords noise, feats noise (masked tensors always draw); per re-noise both
    torch.manual_seed(123)
    t = torch.full((2,), int(sched.timesteps[-1]), device="cuda", dtype=torch.long)
    c = torch.where(mc[:, None, :], process.q_sample(kc, t, c0), c0)
    f = torch.where(mf[:, None, :], process.q_sample(kf, t, f0), f0)
    for lv in [int(i) for i in sched.timesteps[::-1]]:
        t.fill_(lv)
        for j in range(r):
            ec, ef = _stub(c, f, t)
            zc, zf = torch.randn_like(c), torch.randn_like(f)
            (c, _), (f, _) = ew.sampler_step(dict(mode="keep", x_t=c, eps=ec, noise=zc, known=kc, keep=mc, clip=clip_c),
                                             dict(mode="keep", x_t=f, eps=ef, noise=zf, known=kf, keep=mf, clip=clip_f), t, sched.table,
                                             sched.deterministic)
            if j + 1 < r:
                zc, zf = torch.randn_like(c), torch.randn_like(f)
                (c, _), (f, _) = ew.sampler_step(dict(mode="hold", known=c, noise=zc), dict(mode="hold", known=f, noise=zf), t,
                                                 sched.renoise_table, False)
    assert torch.equal(c_end, c) and torch.equal(f_end, f)
    m3c, m3f = mc[:, None, :].expand_as(kc), mf[:, None, :].expand_as(kf)
    assert torch.equal(c_end[m3c], kc[m3c]) and torch.equal(f_end[m3f], kf[m3f])
    assert bool(torch.isfinite(c_end).all()) and bool(torch.isfinite(f_end).all())
    # graph replay: the same bits as eager
    torch.manual_seed(123)
    with torch.no_grad():
        c_g, f_g = process.p_sample_loop(_stub, c0, f0, clip_c, clip_f, steps=K, eta=eta, keep=keep, resample=r, use_graph=True)
    assert torch.equal(c_g, c_end) and torch.equal(f_g, f_end)


def test_completion_on_the_device_follows_the_kept_points_only_with_resampling(process):
    """The toy of tests/test_sampler_keep_cpu.py with the fp32 analytic denoiser and the fused step: B = 8, coords 3 x 512, feats
    4 x 512 = 14,336 pairs, even points kept.  The slope's sampling error is about 0.004; the conditions are those of the CPU test."""
    one = pair_slope(process, 1, dtype=F32, device="cuda", B=8, cc=3, fc=4, N=512)
    ten = pair_slope(process, 10, dtype=F32, device="cuda", B=8, cc=3, fc=4, N=512)
    print(f"slope with resample=1: {one:.4f}, with resample=10: {ten:.4f}")
    assert one <= 0.75
    assert ten >= 0.88


# =====================================================================================================================================
# 3. the model
# =====================================================================================================================================
def test_generate_keeps_points_under_bf16_graph_replay_and_resampling():
    m = _tiny_model()
    g = gen(8)
    coords, feats = randn(g, 3, 3, 48) * 5.0, randn(g, 3, 32, 48) * 4.0        # beyond the clip ranges: kept values are never clipped
    mc, mf = torch.rand(3, 48, device="cuda", generator=g) < 0.5, torch.rand(3, 48, device="cuda", generator=g) < 0.3
    torch.manual_seed(6)
    c, f = m.generate(3, batch_size=2, progress=False, sampling_steps=4, eta=1.0, dtype=torch.bfloat16, use_graph=True, resample=2,
                      coords=coords, feats=feats, keep_coords=mc, keep_feats=mf)
    for out, given, mask, hi in ((torch.stack(c), coords, mc, 3.0), (torch.stack(f), feats, mf, 1.0)):
        m3 = mask[:, None, :].expand_as(given)
        assert torch.equal(out[m3], given[m3])
        assert bool(torch.isfinite(out).all()) and float(out[~m3].abs().max()) <= hi + 1e-5
        assert not bool((out[~m3] == given[~m3]).any())


def test_generate_resamples_without_masks():
    m = _tiny_model()
    kw = dict(batch_size=2, progress=False, sampling_steps=4, eta=1.0)
    torch.manual_seed(7)
    a = m.generate(2, resample=1, **kw)
    torch.manual_seed(7)
    b = m.generate(2, resample=3, **kw)
    assert all(bool(torch.isfinite(x).all()) for x in b[0] + b[1]) and b[0][0].shape == (3, 48) and b[1][0].shape == (32, 48)
    assert not torch.equal(torch.stack(a[0]), torch.stack(b[0])) and not torch.equal(torch.stack(a[1]), torch.stack(b[1]))
