"""The scheduled sampler on the GPU: the one-launch step kernel (npcd_sampler_step) against float64, the loop around it step by step,
and DiffusionModel.generate / npcd.eval.sample_and_render with the new arguments.

Conventions of tests/test_gpu_streaming_kernels.py: float64 references computed on the device from the kernel's own inputs, outputs
between sentinel guard bands that start as NaN, bars from first-order rounding counts with U = 2^-24.  The counts are upper bounds read
off the kernel (csrc/sampler.hip, sampler_x0 / sampler_element: every rounding is written out as a multiply or a fused
multiply-add):
    x0     = fma(r, x, -(m eps))                2 roundings  ->  x0bar = 3 U (|r x| + |m eps|); the clamp is 1-Lipschitz, no element exempt
    x_prev = fma(s, z, fma(c1, x0, c2 x))       3 roundings  ->  |c1| x0bar + 4 U (|c1 x0| + |c2 x|) + 3 U |s z|
    hold   = fma(h1, k, h2 z)                   2 roundings  ->  3 U (|h1 k| + |h2 z|)
For the expression shared with the DDPM kernel (x0, the posterior mean) these are the counts of test_ddpm_reverse_step_past_the_grid_cap;
the noise term has 3 where that test has 6 (no exp).
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16, F32 = torch.bfloat16, torch.float32
SENT = 1536.0
# (coords, feats) elements per sample; the second pair lies past the grid cap with one element per lane (odd sizes), the third takes
# feats past the cap of the 16-byte loop: 4 (1024 x 256) + 4 x 257 elements, a stride of 1024 workgroups x 256 lanes x 4 elements
SIZES = [(255, 2720), (300001, 1024 * 256 * 2 + 4465), (300001, 1_049_604)]
SIZE_IDS = ["small", "past_cap", "past_cap_vec"]


def _ew():
    from npcd.hip import elementwise as ew
    return ew


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


class Guarded:
    """A tensor of `shape` that starts as NaN, between two guard bands of at least one row."""

    def __init__(self, shape, dtype=F32):
        shape = tuple(shape)
        n = int(np.prod(shape))
        self.pad = (max(64, shape[-1]) + 63) // 64 * 64          # keeps the 16-byte alignment of the body
        self.buf = torch.full((n + 2 * self.pad,), SENT, dtype=dtype, device="cuda")
        self.t = self.buf[self.pad:self.pad + n].view(shape)
        self.t.fill_(math.nan)

    def check(self, name, written=True):
        g = torch.cat([self.buf[:self.pad], self.buf[-self.pad:]])
        assert bool((g == SENT).all()), f"{name}: a guard band was written"
        if written:
            assert not bool(torch.isnan(self.t).any()), f"{name}: elements of the range were not written"
        else:
            assert bool(torch.isnan(self.t).all()), f"{name}: written although the call was refused"


def close(name, got, ref, bar):
    """|got - ref| <= bar for EVERY element (float64); prints the worst ratio first."""
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    worst = float(ratio.max())
    print(f"[bar] {name}: max |err| / bar = {worst:.3f}")
    assert worst <= 1.0, f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements outside the bar, worst {worst:.3g} x at flat index {int(ratio.argmax())}"


def _coef(table, t, ndim):
    """The seven float64 coefficient columns of the rows table[t], shaped to broadcast over [B, ...]."""
    row = table[t].double()
    return [row[:, j].reshape((-1,) + (1,) * (ndim - 1)) for j in range(7)]


def ref_reverse(table, t, x, eps, z, clip):
    """float64 single step of a reverse-mode tensor -> (x0, x0 bar, x_prev, x_prev bar); z None: no noise term"""
    r, m, c1, c2, s, _, _ = _coef(table, t, x.dim())
    xd, ed = x.double(), eps.double()
    x0 = r * xd - m * ed
    if clip is not None:
        x0 = x0.clamp(clip[0], clip[1])
    x0bar = 3 * U * ((r * xd).abs() + (m * ed).abs())
    sz = s * z.double() if z is not None else torch.zeros_like(xd)
    ref = c1 * x0 + c2 * xd + sz
    bar = c1.abs() * x0bar + 4 * U * ((c1 * x0).abs() + (c2 * xd).abs()) + 3 * U * sz.abs()
    return x0, x0bar + 1e-300, ref, bar + 1e-300


def ref_hold(table, t, known, z):
    h1, h2 = _coef(table, t, known.dim())[5:7]
    a, b = h1 * known.double(), h2 * z.double()
    return a + b, 3 * U * (a.abs() + b.abs()) + 1e-300


@pytest.fixture(scope="module")
def process():
    from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion().cuda()


# =====================================================================================================================================
# 1. the kernel against float64
# =====================================================================================================================================
@pytest.mark.parametrize("sizes", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("modes", [("reverse", "reverse"), ("hold", "reverse"), ("reverse", "hold")], ids=["rev_rev", "hold_rev", "rev_hold"])
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "no_noise"])
@pytest.mark.parametrize("with_clip", [True, False], ids=["clip", "no_clip"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_step_kernel_against_float64(process, dtype, with_clip, with_noise, modes, sizes):
    ew = _ew()
    sched = process.sampling_schedule(steps=50, eta=0.5 if with_noise else 0.0)
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")            # the last step (arrives at the data) and one mid-chain
    assert sched.timesteps[0] == 0 and (with_noise == bool(sched.table[t[1], 4] > 0))
    g = gen(sizes[0] + 7 * len(modes[0]) + 3 * with_clip)
    B, clips = 2, ((-1.5, 1.5), (-0.75, 1.0))
    specs, refs = [], []
    for z, (mode, per) in enumerate(zip(modes, sizes)):
        x, eps, known = randn(g, B, per), randn(g, B, per).to(dtype), randn(g, B, per)
        noise = randn(g, B, per) if (with_noise or mode == "hold") else None
        clip = clips[z] if with_clip else None
        out, x0 = Guarded((B, per)), Guarded((B, per))
        if mode == "hold":
            specs.append(dict(mode="hold", known=known, noise=noise, out=out.t))
        else:
            specs.append(dict(mode="reverse", x_t=x, eps=eps, noise=noise, clip=clip, out=out.t, x0_out=x0.t))
        refs.append((mode, per, x, eps, known, noise, clip, out, x0))
    (oc, x0c), (of, x0f) = ew.sampler_step(specs[0], specs[1], t, sched.table, sched.deterministic)
    first = []
    for name, (mode, per, x, eps, known, noise, clip, out, x0), got, got0 in zip(("coords", "feats"), refs, (oc, of), (x0c, x0f)):
        assert got is out.t
        out.check(f"{name} out")
        if mode == "hold":
            ref, bar = ref_hold(sched.table, t, known, noise)
            close(f"hold {name}[{per}]", out.t, ref, bar)
            assert got0 is None
            assert torch.equal(out.t[0], known[0])                            # h1 = 1, h2 = 0 on the last step: the known tensor itself
            x0.check(f"{name} x0 (hold mode writes none)", written=False)
        else:
            x0.check(f"{name} x0")
            x0r, x0bar, ref, bar = ref_reverse(sched.table, t, x, eps, noise, clip)
            close(f"x0 {name}[{per}]", x0.t, x0r, x0bar)
            close(f"x_prev {name}[{per}]", out.t, ref, bar)
            # the same bits as the DDPM kernel's x0 on the same x, eps, t, clip (r, m are that kernel's table entries)
            _, ddpm_x0 = ew.ddpm_reverse_step(x, eps, torch.zeros_like(x), t, process._device_tables(x.device), clip, want_x0=True)
            assert torch.equal(x0.t, ddpm_x0), f"{name}: x0 differs from npcd_ddpm_reverse_step's"
        first.append((out.t.clone(), x0.t.clone()))
    ew.sampler_step(specs[0], specs[1], t, sched.table, sched.deterministic)   # the same bits twice
    for (o1, z1), (_, _, _, _, _, _, _, out, x0) in zip(first, refs):
        assert torch.equal(out.t, o1) and torch.equal(x0.t.nan_to_num(7.0), z1.nan_to_num(7.0))
        out.check("second call")


# (entry, modes of (coords, feats), eta): every form of the three entries.  coords [2, 3, 8] and feats [2, 32, 36] have different point
# counts, so a launch carries a mask on one tensor at a time.
ACCESS_FORMS = {"step_noise": ("step", ("reverse", "reverse"), 0.5), "step_no_noise": ("step", ("reverse", "reverse"), 0.0),
                "step_hold": ("step", ("hold", "reverse"), 0.5),
                "keep_coords": ("step", ("keep", "reverse"), 0.5), "keep_feats": ("step", ("reverse", "keep"), 0.5),
                "keep_coords_det": ("step", ("keep", "reverse"), 0.0), "keep_feats_det": ("step", ("reverse", "keep"), 0.0),
                "multistep": ("multistep", ("reverse", "reverse"), 0.0),
                "multistep_keep_coords": ("multistep", ("keep", "reverse"), 0.0), "multistep_keep_feats": ("multistep", ("reverse", "keep"), 0.0)}


def _operands_read(entry, mode, eta):
    """the operands that a tensor of this mode reads or writes in this form"""
    if mode == "hold":
        return ["known", "noise", "out"]
    used = ["x_t", "eps", "out", "x0_out"] + (["hist"] if entry == "multistep" else [])
    if mode == "keep":
        return used + ["noise", "known", "keep"]
    return used + (["noise"] if eta > 0 and entry == "step" else [])


def _four_bytes_off(v):
    """The same values, contiguous, 4 bytes (a mask: 1 byte) past a 16-byte boundary: a [k:] slice of a flat buffer."""
    k = 1 if v.dtype in (torch.bool, torch.uint8) else 4 // v.element_size()
    off = torch.empty(v.numel() + k, dtype=v.dtype, device=v.device)[k:].view(v.shape).copy_(v)
    assert off.is_contiguous() and off.data_ptr() % 16 == k * v.element_size()
    return off


@pytest.mark.parametrize("form", list(ACCESS_FORMS))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_both_access_paths_give_the_same_bits(process, dtype, form):
    """Each form once with every operand 16-byte aligned (16 bytes per lane: per_sample and n_points are multiples of 4), then once
    per operand with that one operand 4 bytes off (one element per lane): out, x0 and the history are the same bits.  Every access is
    dword-aligned (eps and mask: element-aligned) either way."""
    ew = _ew()
    entry, modes, eta = ACCESS_FORMS[form]
    multistep = entry == "multistep"
    sched = process.sampling_schedule(steps=50, solver="dpmpp2m") if multistep else process.sampling_schedule(steps=50, eta=eta)
    table = sched.multistep_table if multistep else sched.table
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")
    B, g = 2, gen(41)
    base = []
    for C, N in ((3, 8), (32, 36)):
        b = {k: randn(g, B, C, N) for k in ("x_t", "eps", "noise", "known", "hist")}
        b["eps"] = b["eps"].to(dtype)
        b["keep"] = torch.rand(B, N, device="cuda", generator=g) < 0.5
        base.append(b)

    def run(off_tensor=None, off_operand=None):
        specs, outs = [], []
        for z, (mode, b) in enumerate(zip(modes, base)):
            o = dict(b, out=torch.full_like(b["x_t"], SENT), x0_out=torch.full_like(b["x_t"], SENT), hist=b["hist"].clone())
            assert all(v.data_ptr() % 16 == 0 for v in o.values())
            if z == off_tensor:
                o[off_operand] = _four_bytes_off(o[off_operand])
            if mode == "hold":
                spec = dict(mode="hold", known=o["known"], noise=o["noise"], out=o["out"])
            else:
                spec = dict(mode=mode, x_t=o["x_t"], eps=o["eps"], clip=(-1.5, 1.5), out=o["out"], x0_out=o["x0_out"])
                spec.update({k: o[k] for k in _operands_read(entry, mode, eta) if k not in spec})
            specs.append(spec)
            outs.append((o["out"], o["x0_out"], o["hist"]))
        if multistep:
            ew.sampler_step_multistep(specs[0], specs[1], t, table)
        else:
            ew.sampler_step(specs[0], specs[1], t, table, sched.deterministic)
        return outs

    aligned = run()
    for z, mode in enumerate(modes):
        assert bool((aligned[z][0] != SENT).all())
        for operand in _operands_read(entry, mode, eta):
            for (a, a0, ah), (o, o0, oh) in zip(aligned, run(z, operand)):
                assert torch.equal(o, a) and torch.equal(o0, a0) and torch.equal(oh, ah), (form, ("coords", "feats")[z], operand)


def test_step_kernel_refuses_missing_operands_before_any_launch(process):
    """A null noise on a reverse tensor while the table has non-zero s rows (eta > 0, `deterministic` false), and a hold mode
    without its known tensor: NPCD_ERR_ARG, and nothing is launched (both outputs stay NaN)."""
    ew = _ew()
    g = gen(5)
    B, pc, pf = 2, 255, 2720
    sched = process.sampling_schedule(steps=50, eta=0.5)
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")
    assert float(sched.table[t[1], 4]) > 0 and not sched.deterministic
    xc, ec, zc, xf, ef, zf = (randn(g, B, p) for p in (pc, pc, pc, pf, pf, pf))
    oc, of = Guarded((B, pc)), Guarded((B, pf))
    cases = [(dict(x_t=xc, eps=ec, noise=None, out=oc.t), dict(x_t=xf, eps=ef, noise=zf, out=of.t)),
             (dict(x_t=xc, eps=ec, noise=zc, out=oc.t), dict(x_t=xf, eps=ef, noise=None, out=of.t)),
             (dict(mode="hold", known=None, noise=zc, out=oc.t), dict(x_t=xf, eps=ef, noise=zf, out=of.t)),
             (dict(x_t=xc, eps=ec, noise=zc, out=oc.t), dict(mode="hold", known=None, noise=zf, out=of.t)),
             (dict(x_t=xc, eps=ec, noise=zc, out=oc.t), dict(mode="hold", known=xf, noise=None, out=of.t))]
    for c, f in cases:
        with pytest.raises(RuntimeError, match=r"npcd_sampler_step failed.*code -1"):
            ew.sampler_step(c, f, t, sched.table, sched.deterministic)
        torch.cuda.synchronize()
        oc.check("coords", written=False)
        of.check("feats", written=False)
    with pytest.raises(RuntimeError, match=r"code -2"):                        # an eps type the kernel does not take
        ew.sampler_step(dict(x_t=xc, eps=ec.half(), noise=zc, out=oc.t), dict(x_t=xf, eps=ef, noise=zf, out=of.t), t, sched.table, False)
    oc.check("coords", written=False)
    # the same records with the noise given run
    ew.sampler_step(cases[1][0], dict(x_t=xf, eps=ef, noise=zf, out=of.t), t, sched.table, sched.deterministic)
    oc.check("coords")
    of.check("feats")


# =====================================================================================================================================
# 2. the loop: the schedule is walked, every step is the single-step formula on the state the step received (no error accumulates in
#    the comparison), the documented RNG order
# =====================================================================================================================================
class Recorder:
    """eps = tanh(0.3 x + 1e-3 t), an analytic denoiser that records what it is given and what it returns"""

    def __init__(self):
        self.calls = []

    def __call__(self, c, f, t):
        tt = (1e-3 * t.float())[:, None, None]
        ec, ef = torch.tanh(0.3 * c + tt), torch.tanh(0.3 * f + tt)
        self.calls.append((c.clone(), f.clone(), t.clone(), ec.clone(), ef.clone()))
        return ec, ef


@pytest.mark.parametrize("held", [False, True], ids=["free", "hold_coords"])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_loop_walks_the_schedule_one_launch_per_step(process, monkeypatch, eta, held):
    ew = _ew()
    B, N, F_, K = 2, 64, 32, 6
    g = gen(11)
    c0, f0, k = randn(g, B, 3, N), randn(g, B, F_, N), randn(g, B, 3, N) * 0.8
    clip_c, clip_f = (-3.0, 3.0), (-1.0, 1.0)
    sched = process.sampling_schedule(steps=K, eta=eta)
    launches = []
    real = ew.sampler_step
    monkeypatch.setattr(ew, "sampler_step", lambda *a, **kw: (launches.append(1), real(*a, **kw))[1])
    fn = Recorder()
    torch.manual_seed(123)
    with torch.no_grad():
        c_end, f_end = process.p_sample_loop(fn, c0, f0, clip_c, clip_f, steps=K, eta=eta, hold=("coords", k) if held else None)
    assert len(launches) == K and len(fn.calls) == K                           # the fused path: one launch per step
    levels = [int(i) for i in sched.timesteps[::-1]]
    for (_, _, t, _, _), lv in zip(fn.calls, levels):
        assert t.dtype == torch.int64 and t.shape == (B,) and t.tolist() == [lv] * B
    # the documented draw order, replayed: per step coords noise, then feats noise; reverse tensors only if eta > 0, the held one always
    torch.manual_seed(123)
    noise = []
    for _ in range(K):
        zc = torch.randn_like(c0) if (eta > 0 or held) else None
        zf = torch.randn_like(f0) if eta > 0 else None
        noise.append((zc, zf))
    if held:                                                                   # starts as the known tensor noised to the first level
        assert torch.equal(fn.calls[0][0], process.q_sample(k, fn.calls[0][2], c0)) and torch.equal(fn.calls[0][1], f0)
    else:
        assert torch.equal(fn.calls[0][0], c0) and torch.equal(fn.calls[0][1], f0)
    states = [(c, f) for c, f, _, _, _ in fn.calls[1:]] + [(c_end, f_end)]
    for i, ((c, f, t, ec, ef), (zc, zf), (c_next, f_next)) in enumerate(zip(fn.calls, noise, states)):
        if held:
            ref, bar = ref_hold(sched.table, t, k, zc)
        else:
            _, _, ref, bar = ref_reverse(sched.table, t, c, ec, zc, clip_c)
        close(f"step {i} coords", c_next, ref, bar)
        _, _, ref, bar = ref_reverse(sched.table, t, f, ef, zf, clip_f)
        close(f"step {i} feats", f_next, ref, bar)
    if held:
        assert torch.equal(c_end, k)


# =====================================================================================================================================
# 3. the model
# =====================================================================================================================================
def _tiny_model():
    from npcd.models.diffusion import DiffusionModel
    torch.manual_seed(0)
    m = DiffusionModel(3, 32, 48, 128, 2, 2, True).cuda().eval()
    with torch.no_grad():
        m.coords_normalization.min.fill_(-3.0); m.coords_normalization.max.fill_(3.0)
        m.feats_normalization.min.fill_(-1.0); m.feats_normalization.max.fill_(1.0)
    return m


def test_generate_eager_and_graph_replay_give_the_same_bits():
    """eta = 0: no RNG in the loop and deterministic kernels, so the captured step replayed is the eager step"""
    m = _tiny_model()
    torch.manual_seed(4)
    ac, af = m.generate(2, batch_size=2, progress=False, sampling_steps=5, eta=0.0)
    torch.manual_seed(4)
    bc, bf = m.generate(2, batch_size=2, progress=False, sampling_steps=5, eta=0.0, use_graph=True)
    assert len(ac) == 2 and ac[0].shape == (3, 48) and af[0].shape == (32, 48)
    assert all(bool(torch.isfinite(x).all()) for x in ac + af)
    assert torch.equal(torch.stack(ac), torch.stack(bc)) and torch.equal(torch.stack(af), torch.stack(bf))


def test_generate_bf16_graph_with_noise_stays_finite_and_clipped():
    m = _tiny_model()
    torch.manual_seed(5)
    coords, feats = m.generate(2, batch_size=2, progress=False, sampling_steps=5, eta=1.0, dtype=torch.bfloat16, use_graph=True)
    assert len(coords) == 2 and all(bool(torch.isfinite(x).all()) for x in coords + feats)
    assert float(torch.stack(coords).abs().max()) <= 3.0 + 1e-5               # x0 clipping was applied on the last step


def test_generate_returns_the_given_feats_bit_for_bit():
    m = _tiny_model()
    with torch.no_grad():
        m.feats_normalization.shift.copy_(torch.linspace(-0.3, 0.3, 32)); m.feats_normalization.scale.fill_(0.37)
    given = randn(gen(6), 3, 32, 48) * 4.0                                      # beyond the clip range: the held tensor is never clipped
    torch.manual_seed(6)
    coords, feats = m.generate(3, batch_size=2, progress=False, sampling_steps=5, eta=0.0, feats=given)
    assert torch.equal(torch.stack(feats), given)
    assert len(coords) == 3 and all(bool(torch.isfinite(x).all()) for x in coords)
    with pytest.raises(ValueError):
        m.generate(3, batch_size=2, progress=False, coords=torch.zeros(3, 3, 48, device="cuda"), feats=given)


def test_sample_and_render_passes_the_schedule_through():
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
    net.diffusion.diffusion_process.p_sample_loop = lambda *a, **kw: (seen.append((kw.get("steps"), kw.get("eta"))), real(*a, **kw))[1]
    res = sample_and_render(net, poses[:2], intr[:2], num_samples=2, generate_batch_size=2, render_batch_size=2, resolution=16,
                            sampling_steps=3, eta=0.0)
    assert seen == [(3, 0.0)]
    assert res["clouds"] == 2 and res["poses_per_cloud"] == 2 and res["image_batch_shape"] == (2, 3, 16, 16)
    assert res["generate_seconds"] > 0 and res["views_per_s"] > 0
