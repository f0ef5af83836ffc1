"""Second-order few-step sampling on the host: the log-SNR level spacing of GaussianDiffusion.sampling_schedule(spacing="logsnr"), the
weights and the table of the multistep solver (solver="dpmpp2m", DPM-Solver++ 2M in data prediction, Lu et al. 2022), the torch
formulation of the loop on an analytic denoiser whose probability-flow solution is known, the host-side refusals of
npcd_sampler_step_multistep, and DiffusionModel.generate(solver=) on the CPU.

With lambda(t) = log(acp[t] / (1 - acp[t])) / 2 and the levels tau_0 < ... < tau_{K-1}, performed in the order i = K-1 ... 0:
    h_i = lambda(tau_{i-1}) - lambda(tau_i),   w_i = h_i / (2 h_{i+1}) for 1 <= i <= K-2,   w_{K-1} = w_0 = 0
    x_prev = c1 D + c2 x_t,   D = x0 + w_i (x0 - x0 of the step before)          (c1, c2: the eta = 0 DDIM coefficients of the level)

The analytic denoiser.  Every element's data is N(mu, s^2); then eps(x_t, t) = sqrt(1 - a) (x_t - sqrt(a) mu) / (a s^2 + 1 - a) with
a = acp[t] exactly, and the probability-flow ODE from x_T has the closed solution
    x_0 = mu + s (x_T - sqrt(a_T) mu) / sqrt(a_T s^2 + 1 - a_T).
"""
import ctypes

import numpy as np
import pytest
import torch

from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion
from test_sampler_schedule_cpu import _tiny_model

U = 2.0 ** -24


def _lam(gd):
    acp = np.cumprod(1.0 - gd.np_betas[:gd.num_timesteps].astype(np.float64))
    return 0.5 * np.log(acp / (1.0 - acp))


# =====================================================================================================================================
# 1. the schedule
# =====================================================================================================================================
@pytest.mark.parametrize("T,K", [(1000, 1), (1000, 2), (1000, 7), (1000, 50), (1000, 999), (1000, 1000), (12, 2), (12, 5), (12, 12)])
def test_logsnr_levels_are_k_distinct_levels_that_span_the_chain(T, K):
    gd = GaussianDiffusion()
    gd.num_timesteps = T
    sch = gd.sampling_schedule(steps=K, eta=0.0, spacing="logsnr")
    ts = np.asarray(sch.timesteps)
    assert ts.dtype == np.int64 and ts.shape == (K,)
    assert ts[-1] == T - 1
    if K == 1:
        assert ts.tolist() == [T - 1]
    else:
        assert ts[0] == 0 and bool((np.diff(ts) > 0).all())
    if K == T:
        assert np.array_equal(ts, np.arange(T))
    assert tuple(sch.table.shape) == (T, 8) and int((~torch.isnan(sch.table[:, 0])).sum()) == K
    # the construction, restated: nearest level of K targets uniform in lambda, made distinct upwards, then downwards from T - 1
    if K > 1:
        lam = _lam(gd)
        want = [int(np.abs(lam - x).argmin()) for x in np.linspace(lam[0], lam[-1], K)]
        for i in range(1, K):
            want[i] = max(want[i], want[i - 1] + 1)
        want[-1] = T - 1
        for i in range(K - 2, -1, -1):
            want[i] = min(want[i], want[i + 1] - 1)
        assert ts.tolist() == want


def test_logsnr_levels_are_near_uniform_in_lambda_where_the_chain_allows():
    """K = 10 of 1,000: no two targets share a level, so every level is the nearest one of its target and the lambda steps differ
    from the uniform step by at most the lambda distance of two neighbouring levels at either end of the step."""
    gd = GaussianDiffusion()
    lam = _lam(gd)
    ts = np.asarray(gd.sampling_schedule(steps=10, eta=0.0, spacing="logsnr").timesteps)
    step = (lam[0] - lam[-1]) / 9
    gaps = lam[ts[:-1]] - lam[ts[1:]]
    slack = np.abs(np.diff(lam)).max()
    print(f"levels {ts.tolist()}, lambda steps / uniform step: {np.round(gaps / step, 3).tolist()}")
    assert bool((np.abs(gaps - step) <= slack).all())
    uniform = np.asarray(gd.sampling_schedule(steps=10, eta=0.0).timesteps)
    assert not np.array_equal(ts, uniform)


@pytest.mark.parametrize("K", [10, 50])
def test_weights_are_the_formula_and_zero_at_both_ends(K):
    gd = GaussianDiffusion()
    sch = gd.sampling_schedule(steps=K, solver="dpmpp2m")
    assert sch.spacing == "logsnr" and sch.deterministic and sch.eta == 0.0
    ts, lam = np.asarray(sch.timesteps), _lam(gd)
    w = np.zeros(K)
    for i in range(1, K - 1):
        h_i = lam[ts[i - 1]] - lam[ts[i]]
        h_before = lam[ts[i]] - lam[ts[i + 1]]                                # the transition performed just before: it left tau_{i+1}
        w[i] = h_i / (2.0 * h_before)
    got = sch.coef64["w"]
    assert got.dtype == np.float64 and got.shape == (K,)
    assert got[0] == 0.0 and got[-1] == 0.0
    assert np.allclose(got, w, rtol=1e-13, atol=0.0)
    assert bool((got[1:-1] > 0).all())
    print(f"K = {K}: largest weight {got.max():.3f}")
    assert got.max() < 1.0                                                    # near-uniform lambda steps: w is near 1/2


@pytest.mark.parametrize("K,spacing", [(10, None), (50, "logsnr"), (10, "uniform"), (2, None), (1, None)])
def test_multistep_table_is_the_eta_zero_table_with_w_in_column_seven(K, spacing):
    gd = GaussianDiffusion()
    T = gd.num_timesteps
    sch = gd.sampling_schedule(steps=K, solver="dpmpp2m", spacing=spacing)
    ddim = gd.sampling_schedule(steps=K, eta=0.0, spacing=sch.spacing)
    assert ddim is not sch and np.array_equal(ddim.timesteps, sch.timesteps)
    assert not hasattr(ddim, "multistep_table") and "w" not in ddim.coef64    # built only for the solver
    tab = sch.multistep_table
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (T, 8) and tab.is_contiguous()
    idx = torch.from_numpy(np.asarray(sch.timesteps))
    assert torch.equal(tab[idx, :7].view(torch.int32), ddim.table[idx, :7].view(torch.int32))
    assert torch.equal(sch.table.view(torch.int32), ddim.table.view(torch.int32))        # the step table itself: column 7 stays 0
    assert bool((tab[idx, 4] == 0).all())
    assert torch.equal(tab[idx, 7], torch.from_numpy(sch.coef64["w"]).float())           # rounded once
    err = np.abs(tab[idx, 7].double().numpy() - sch.coef64["w"])
    assert bool((err <= U * np.abs(sch.coef64["w"])).all())
    assert float(tab[idx[0], 7]) == 0.0 and float(tab[idx[-1], 7]) == 0.0
    off = np.setdiff1d(np.arange(T), np.asarray(sch.timesteps))
    assert bool(torch.isnan(tab[torch.from_numpy(off)]).all())


def test_old_schedules_are_the_cached_uniform_objects_with_their_tables():
    gd = GaussianDiffusion()
    a = gd.sampling_schedule(steps=10, eta=0.0)
    assert gd.sampling_schedule(steps=10, eta=0.0) is a
    assert gd.sampling_schedule(steps=10, eta=0.0, spacing="uniform") is a and gd.sampling_schedule(10, 0.0, None, "uniform", None) is a
    assert a.spacing == "uniform" and a.solver is None
    assert gd.sampling_schedule(steps=10, eta=0.0, spacing="logsnr") is not a
    assert gd.sampling_schedule(steps=10, solver="dpmpp2m") is not a
    assert gd.sampling_schedule(steps=10, solver="dpmpp2m") is gd.sampling_schedule(steps=10, eta=0, spacing="logsnr", solver="dpmpp2m")
    assert gd.sampling_schedule(steps=10) is gd.sampling_schedule(steps=10, eta=1.0)     # eta None: 1 without a solver
    ts = np.asarray(a.timesteps)
    assert np.array_equal(ts, np.round(np.linspace(0, 999, 10)).astype(np.int64))
    idx = torch.from_numpy(ts)
    assert bool((a.table[idx, 7] == 0).all()) and bool((a.renoise_table[idx, 7] == 0).all())
    assert set(a.coef64) == {"c1", "c2", "s", "h1", "h2"}
    assert torch.equal(a.table[idx, 0], gd.sqrt_recip_alphas_cumprod[idx])
    # logsnr levels feed every coefficient as the uniform ones do
    b = gd.sampling_schedule(steps=10, eta=0.5, spacing="logsnr")
    acp = np.cumprod(1.0 - gd.np_betas.astype(np.float64))
    tb = np.asarray(b.timesteps)
    p = np.concatenate(([1.0], acp[tb][:-1]))
    assert np.allclose(b.coef64["h1"], np.sqrt(p), rtol=1e-13) and np.allclose(b.renoise64["g1"], np.sqrt(acp[tb] / p), rtol=1e-13)
    assert bool((b.table[torch.from_numpy(tb)[1:], 4] > 0).all())


def _stub(c, f, t):
    tt = (1e-3 * t.float())[:, None, None]
    return torch.tanh(0.3 * c + tt), torch.tanh(0.3 * f + tt)


def _starts(seed=1, B=2, N=16):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, N, generator=g), torch.randn(B, 5, N, generator=g), torch.randn(B, 3, N, generator=g) * 0.8


def test_argument_errors():
    gd = GaussianDiffusion()
    with pytest.raises(ValueError, match="deterministic"):
        gd.sampling_schedule(steps=10, eta=0.5, solver="dpmpp2m")
    with pytest.raises(ValueError, match="deterministic"):
        gd.sampling_schedule(steps=10, eta=1.0, solver="dpmpp2m")
    with pytest.raises(ValueError, match="solver"):
        gd.sampling_schedule(steps=10, solver="dpm3")
    with pytest.raises(ValueError, match="spacing"):
        gd.sampling_schedule(steps=10, spacing="cosine")
    c0, f0, _ = _starts()
    for bad in (dict(solver="dpmpp2m", resample=2), dict(solver="dpmpp2m", eta=0.3), dict(solver="heun"), dict(spacing="karras")):
        with pytest.raises(ValueError):
            gd.p_sample_loop(_stub, c0, f0, steps=5, **bad)
    gd.p_sample_loop(_stub, c0, f0, steps=5, solver="dpmpp2m", resample=1)    # one performance per transition is no resampling


# =====================================================================================================================================
# 2. the loop in torch
# =====================================================================================================================================
class Gaussian:
    """The analytic denoiser of the module docstring and the exact solution, in `dtype` on `device`: 4,096 elements, seed 0, mu uniform
    in [-0.5, 0.5], s uniform in [0.2, 0.8], split into a coords tensor [1, 3, 128] and a feats tensor [1, 29, 128]."""

    def __init__(self, gd, dtype=torch.float64, device="cpu"):
        g = torch.Generator().manual_seed(0)
        n, self.nc = 4096, 3 * 128
        mu = torch.rand(n, generator=g, dtype=torch.float64) - 0.5
        s = 0.2 + 0.6 * torch.rand(n, generator=g, dtype=torch.float64)
        x_T = torch.randn(n, generator=g, dtype=torch.float64)
        acp = torch.from_numpy(np.cumprod(1.0 - gd.np_betas.astype(np.float64)))
        a_T = acp[-1]
        self.exact = mu + s * (x_T - a_T.sqrt() * mu) / torch.sqrt(a_T * s * s + (1.0 - a_T))         # float64, on the host
        self.acp = acp.to(device=device, dtype=dtype)
        self.mu = [v.to(device=device, dtype=dtype) for v in self.split(mu)]
        self.s2 = [(v * v).to(device=device, dtype=dtype) for v in self.split(s)]
        self.start = [v.to(device=device, dtype=dtype) for v in self.split(x_T)]

    def split(self, v):
        return v[:self.nc].reshape(1, 3, 128), v[self.nc:].reshape(1, -1, 128)

    def __call__(self, c, f, t):
        a = self.acp[t].reshape(-1, 1, 1)
        return [torch.sqrt(1.0 - a) * (x - a.sqrt() * m) / (a * s2 + (1.0 - a)) for x, m, s2 in zip((c, f), self.mu, self.s2)]

    def rms_error(self, gd, K, **kw):
        with torch.no_grad():
            c, f = gd.p_sample_loop(self, self.start[0].clone(), self.start[1].clone(), steps=K, **kw)
        got = torch.cat([c.reshape(-1), f.reshape(-1)]).double().cpu()
        return float(((got - self.exact) ** 2).mean().sqrt())


def check_convergence(gd, toy, **kw):
    """The two conditions of the feature: the multistep solver on logsnr levels is at least 5 times as accurate as the DDIM step on the
    same levels at K = 10, 20, 40 (the float64 reference gives 7.1, 8.2, 16.7), and halving its step from K = 20 to 40 cuts its error
    at least 3 times (4.0: second order)."""
    ddim = {K: toy.rms_error(gd, K, eta=0.0, spacing="logsnr", **kw) for K in (10, 20, 40)}
    two = {K: toy.rms_error(gd, K, solver="dpmpp2m", **kw) for K in (10, 20, 40)}
    for K in (10, 20, 40):
        print(f"K = {K}: DDIM rms error {ddim[K]:.3e}, 2M rms error {two[K]:.3e}, ratio {ddim[K] / two[K]:.2f}")
    print(f"2M, K = 20 -> 40: error ratio {two[20] / two[40]:.2f}")
    for K in (10, 20, 40):
        assert two[K] <= ddim[K] / 5.0, (K, ddim[K], two[K])
    assert two[40] <= two[20] / 3.0, (two[20], two[40])


def test_second_order_convergence_on_the_analytic_denoiser():
    """float64 states through the torch formulation (its coefficients are the fp32 tables: 6e-8 relative, against solver errors of
    1e-3 and more)"""
    gd = GaussianDiffusion()
    check_convergence(gd, Gaussian(gd))


def test_the_solver_on_uniform_levels_is_no_better_than_ddim_at_few_steps():
    """Why the solver's default spacing is logsnr: uniform in t, the last transitions before the data span lambda intervals several
    times their predecessors', the weights exceed 2 and the extrapolation overshoots.  Recorded, and the weights asserted."""
    gd = GaussianDiffusion()
    toy = Gaussian(gd)
    for K in (10, 20):
        sch = gd.sampling_schedule(steps=K, solver="dpmpp2m", spacing="uniform")
        ddim, two = toy.rms_error(gd, K, eta=0.0), toy.rms_error(gd, K, solver="dpmpp2m", spacing="uniform")
        print(f"K = {K} uniform in t: DDIM {ddim:.3e}, 2M {two:.3e}, largest weight {sch.coef64['w'].max():.2f}")
        assert sch.coef64["w"].max() > 2.0 and two > ddim


@pytest.mark.parametrize("K", [1, 2])
def test_one_and_two_levels_are_the_ddim_loop_bit_for_bit(K):
    """K <= 2: every transition is a first or a last one, w = 0 throughout"""
    gd = GaussianDiffusion()
    c0, f0, _ = _starts()
    with torch.no_grad():
        want = gd.p_sample_loop(_stub, c0, f0, (-3.0, 3.0), (-1.0, 1.0), steps=K, eta=0.0, spacing="logsnr")
        got = gd.p_sample_loop(_stub, c0, f0, (-3.0, 3.0), (-1.0, 1.0), steps=K, solver="dpmpp2m")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_the_loop_is_the_formula_step_by_step_and_composes_with_hold_and_keep():
    """K = 5 with clip: every state the denoiser receives is the multistep formula, restated here in float64, on what the previous
    call received and returned and on the previous clipped x0.  Bar as in tests/test_sampler_keep_cpu.py: fewer than ten roundings
    of terms below 8 (w < 1, |x0| <= 3), 10 * 8 * 2^-24 < 1e-5."""
    gd = GaussianDiffusion()
    K = 5
    c0, f0, kc = _starts()
    sch = gd.sampling_schedule(steps=K, solver="dpmpp2m")
    clips = ((-3.0, 3.0), (-1.0, 1.0))
    calls = []

    def fn(c, f, t):
        ec, ef = _stub(c, f, t)
        calls.append((c.clone(), f.clone(), t.clone(), ec, ef))
        return ec, ef

    with torch.no_grad():
        end = gd.p_sample_loop(fn, c0, f0, *clips, steps=K, solver="dpmpp2m")
    assert [int(t[0]) for _, _, t, _, _ in calls] == [int(i) for i in sch.timesteps[::-1]]
    nexts = [(c, f) for c, f, _, _, _ in calls[1:]] + [end]
    prev = [None, None]
    for (c, f, t, ec, ef), nxt in zip(calls, nexts):
        k = [sch.multistep_table[t].double()[:, j].reshape(-1, 1, 1) for j in range(8)]
        for z, (x, e, clip) in enumerate(((c, ec, clips[0]), (f, ef, clips[1]))):
            x0 = (k[0] * x - k[1] * e).clamp(*clip)
            d = x0 if prev[z] is None else x0 + k[7] * (x0 - prev[z])
            assert float((nxt[z].double() - (k[2] * d + k[3] * x)).abs().max()) <= 1e-5
            prev[z] = x0
    assert float(sch.multistep_table[int(sch.timesteps[2]), 7]) > 0           # the middle steps did extrapolate
    # hold: the held tensor ends as the known one; keep: kept points end as the known values, and NaN in `known` at free points is not read
    torch.manual_seed(3)
    with torch.no_grad():
        hc, hf = gd.p_sample_loop(_stub, c0, f0, *clips, steps=K, solver="dpmpp2m", hold=("coords", kc))
    assert torch.equal(hc, kc) and bool(torch.isfinite(hf).all())
    mask = torch.rand(2, 16, generator=torch.Generator().manual_seed(5)) < 0.5
    m3 = mask[:, None, :].expand_as(kc)
    torch.manual_seed(3)
    with torch.no_grad():
        a = gd.p_sample_loop(_stub, c0, f0, *clips, steps=K, solver="dpmpp2m", keep={"coords": (kc, mask)})
        torch.manual_seed(3)
        b = gd.p_sample_loop(_stub, c0, f0, *clips, steps=K, solver="dpmpp2m",
                             keep={"coords": (torch.where(m3, kc, torch.full_like(kc, float("nan"))), mask)})
    assert torch.equal(a[0][m3], kc[m3]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())
    # an all-False mask is the unmasked loop
    with torch.no_grad():
        none = gd.p_sample_loop(_stub, c0, f0, *clips, steps=K, solver="dpmpp2m",
                                keep={"coords": (torch.full_like(kc, float("nan")), torch.zeros(2, 16, dtype=torch.bool))})
    assert torch.equal(none[0], end[0]) and torch.equal(none[1], end[1])


# =====================================================================================================================================
# 3. the C entry point on the host, the model
# =====================================================================================================================================
def test_entry_point_refuses_on_the_host():
    """Refused before any pointer is followed and before any launch: made-up addresses, no GPU.  -1: NPCD_ERR_ARG, -2:
    NPCD_ERR_UNSUPPORTED."""
    from npcd import hip
    from npcd.hip.elementwise import SAMPLER_HOLD, SAMPLER_REVERSE, SamplerTensor
    L = hip.lib()
    assert L.npcd_abi_version() == 10 and "npcd_sampler_step_multistep" not in L.npcd_missing
    A = 0x10000                                                               # 16-byte aligned, never followed

    def rec(**kw):
        r = SamplerTensor()
        r.x_t, r.eps, r.noise, r.known, r.out, r.x0_out = A, A, A, A, A, 0
        r.per_sample, r.mode, r.eps_dtype = 3 * 512, SAMPLER_REVERSE, hip.NPCD_F32
        for name, v in kw.items():
            setattr(r, name, v)
        return r

    def call(c, f, hc=A, hf=A, kc=0, kf=0, n=0, t=A, table=A, T=1000, B=2):
        P = ctypes.c_void_p
        return L.npcd_sampler_step_multistep(None if c is None else ctypes.byref(c), None if f is None else ctypes.byref(f), P(hc), P(hf),
                                             P(kc), P(kf), n, P(t), P(table), T, B, P(0))

    ok = rec()
    assert call(None, ok) == -1 and call(ok, None) == -1                      # null operands
    assert call(ok, ok, t=0) == -1 and call(ok, ok, table=0) == -1
    assert call(ok, ok, T=0) == -1 and call(ok, ok, B=0) == -1
    for missing in ("x_t", "eps", "out"):
        assert call(rec(**{missing: 0}), ok) == -1 and call(ok, rec(**{missing: 0})) == -1
    assert call(ok, rec(per_sample=0)) == -1
    assert call(ok, ok, hc=0) == -1 and call(ok, ok, hf=0) == -1              # a missing history
    assert call(ok, ok, hc=0, kc=A, n=512) == -1                              # ... of a masked tensor too
    assert call(rec(mode=2), ok) == -1 and call(ok, rec(mode=-1)) == -1       # a bad mode
    assert call(rec(mode=SAMPLER_HOLD, known=0), ok, hc=0) == -1              # hold mode: known and noise, as in npcd_sampler_step
    assert call(ok, rec(mode=SAMPLER_HOLD, noise=0), hf=0) == -1
    assert call(ok, ok, kc=A, n=0) == -1 and call(ok, ok, kf=A, n=-4) == -1   # a mask needs n_points
    assert call(ok, ok, kc=A, n=5) == -1                                      # 3 * 512 is no multiple of 5
    assert call(ok, rec(per_sample=32 * 512), kc=A, kf=A, n=1024) == -1       # divides 32 * 512, not 3 * 512
    assert call(rec(noise=0), ok, kc=A, n=512) == -1 and call(rec(known=0), ok, kc=A, n=512) == -1
    assert call(rec(eps_dtype=hip.NPCD_F16), ok) == -2 and call(ok, rec(eps_dtype=hip.NPCD_F16), kf=A, n=512) == -2
    assert call(ok, ok, B=65536) == -2 and call(ok, ok, table=A + 4) == -2


def test_wrapper_refuses_cpu_tensors():
    from npcd.hip import elementwise as ew
    x = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ew.sampler_step_multistep(dict(x_t=x, eps=x, hist=x.clone()), dict(x_t=x, eps=x, hist=x.clone()), torch.zeros(2, dtype=torch.int64),
                                  torch.zeros(10, 8))


def test_generate_on_the_cpu_with_four_multistep_levels(monkeypatch):
    m = _tiny_model(monkeypatch)
    seen = []
    real = m.diffusion_process.p_sample_loop
    monkeypatch.setattr(m.diffusion_process, "p_sample_loop", lambda *a, **kw: (seen.append(kw), real(*a, **kw))[1])
    torch.manual_seed(3)
    coords, feats = m.generate(3, batch_size=2, progress=False, sampling_steps=4, solver="dpmpp2m")
    assert len(coords) == 3 and len(feats) == 3 and coords[0].shape == (3, 48) and feats[0].shape == (32, 48)
    assert all(bool(torch.isfinite(x).all()) for x in coords + feats)
    assert float(torch.stack(coords).abs().max()) <= 3.0 * 0.7 + 0.3 + 1e-5 and float(torch.stack(feats).abs().max()) <= 1.0 + 1e-5
    assert all(kw["steps"] == 4 and kw["solver"] == "dpmpp2m" and kw["eta"] is None and "spacing" not in kw for kw in seen)
    torch.manual_seed(3)
    again = m.generate(3, batch_size=2, progress=False, sampling_steps=4, solver="dpmpp2m")
    assert torch.equal(torch.stack(coords), torch.stack(again[0])) and torch.equal(torch.stack(feats), torch.stack(again[1]))
    torch.manual_seed(3)
    ddim = m.generate(3, batch_size=2, progress=False, sampling_steps=4, eta=0.0, spacing="logsnr")
    assert not torch.equal(torch.stack(coords), torch.stack(ddim[0]))          # the two middle steps extrapolate
    given = torch.randn(3, 3, 48, generator=torch.Generator().manual_seed(9)) * 5.0
    torch.manual_seed(3)
    held, _ = m.generate(3, batch_size=2, progress=False, sampling_steps=4, solver="dpmpp2m", spacing="uniform", coords=given)
    assert torch.equal(torch.stack(held), given) and seen[-1]["spacing"] == "uniform"
    for bad in (dict(solver="dpmpp2m", eta=0.5), dict(solver="dpmpp2m", resample=2), dict(solver="euler"), dict(spacing="linear")):
        with pytest.raises(ValueError):
            m.generate(2, batch_size=2, progress=False, sampling_steps=4, **bad)
