"""The scheduled sampler on the host: GaussianDiffusion.sampling_schedule (strided DDIM levels, eta, the [T, 8] device table) against
a float64 restatement, and DiffusionModel.generate(sampling_steps=, eta=, coords=) on the CPU formulation of the step.

The restatement (Song et al. 2021, eq. 12 / 16, in the variables of the DDPM posterior): with a = acp[tau_i], p = acp[tau_{i-1}] (1 for
the last step), sigma = eta sqrt((1 - p) / (1 - a)) sqrt(1 - a / p), d = sqrt(1 - p - sigma^2):
    c1 = sqrt(p) - d / sqrt(1 / a - 1),  c2 = d sqrt(1 / a) / sqrt(1 / a - 1),  s = sigma,  h1 = sqrt(p),  h2 = sqrt(1 - p).
"""
import numpy as np
import pytest
import torch

from npcd.models.diffusion import DiffusionModel
from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion

U = 2.0 ** -24
COLS = ("r", "m", "c1", "c2", "s", "h1", "h2")


def _coef64(gd, ts, eta):
    acp = np.cumprod(1.0 - gd.np_betas[:gd.num_timesteps].astype(np.float64))
    a = acp[ts]
    p = np.concatenate(([1.0], a[:-1]))
    sigma = eta * np.sqrt((1 - p) / (1 - a)) * np.sqrt(1 - a / p)
    d = np.sqrt(1 - p - sigma ** 2)
    return {"c1": np.sqrt(p) - d / np.sqrt(1 / a - 1), "c2": d * np.sqrt(1 / a) / np.sqrt(1 / a - 1), "s": sigma, "h1": np.sqrt(p),
            "h2": np.sqrt(1 - p)}


@pytest.mark.parametrize("K", [1, 2, 7, 50, 999, 1000])
def test_timesteps_are_strictly_increasing_and_span_the_chain(K):
    gd = GaussianDiffusion()
    T = gd.num_timesteps
    ts = np.asarray(gd.sampling_schedule(steps=K, eta=0.0).timesteps)
    assert ts.dtype == np.int64 and ts.shape == (K,)
    assert ts[-1] == T - 1
    if K == 1:
        assert ts.tolist() == [T - 1]
    else:
        assert ts[0] == 0 and bool((np.diff(ts) > 0).all())
        assert np.array_equal(ts, np.round(np.linspace(0, T - 1, K)).astype(np.int64))
    if K == T:
        assert np.array_equal(ts, np.arange(T))
        assert np.array_equal(gd.sampling_schedule().timesteps, ts)          # steps=None means every level


def test_arguments_outside_their_range_raise_and_the_schedule_is_cached():
    gd = GaussianDiffusion()
    for bad in (0, gd.num_timesteps + 1):
        with pytest.raises(ValueError):
            gd.sampling_schedule(steps=bad)
    with pytest.raises(ValueError):
        gd.sampling_schedule(steps=10, eta=1.5)
    with pytest.raises(ValueError):
        gd.sampling_schedule(steps=10, eta=-0.1)
    a = gd.sampling_schedule(steps=10, eta=0.5)
    assert gd.sampling_schedule(steps=10, eta=0.5) is a and gd.sampling_schedule(steps=10, eta=0.0) is not a
    gd.num_timesteps = 12                                                    # read at call time: a shortened chain is another schedule
    short = gd.sampling_schedule(steps=10, eta=0.5)
    assert short is not a and short.timesteps[-1] == 11 and tuple(short.table.shape) == (12, 8)
    with pytest.raises(ValueError):
        gd.sampling_schedule(steps=13)


def test_every_level_with_eta_one_is_the_ddpm_posterior():
    """K = T, eta = 1: c1, c2, s^2 are the posterior mean coefficients and variance of the reference's DDPM, beta sqrt(p) / (1 - a),
    (1 - p) sqrt(alpha) / (1 - a), beta (1 - p) / (1 - a).  The identity is exact; evaluated in float64 it holds to 7.5e-13 relative,
    the bar of 1e-9 leaves three orders of magnitude for the cumulative product."""
    gd = GaussianDiffusion()
    sch = gd.sampling_schedule(steps=None, eta=1.0)
    beta = gd.np_betas.astype(np.float64)
    acp = np.cumprod(1.0 - beta)
    prev = np.concatenate(([1.0], acp[:-1]))
    want = {"c1": beta * np.sqrt(prev) / (1 - acp), "c2": (1 - prev) * np.sqrt(1 - beta) / (1 - acp)}
    for name, ref in want.items():
        rel = np.abs(sch.coef64[name] - ref) / np.maximum(np.abs(ref), 1e-300)
        rel[ref == 0] = np.abs(sch.coef64[name])[ref == 0]
        print(f"{name}: max relative difference {rel.max():.3g}")
        assert rel.max() <= 1e-9, (name, rel.max())
    var = beta * (1 - prev) / (1 - acp)
    s2 = sch.coef64["s"] ** 2
    rel = np.abs(s2 - var) / np.where(var == 0, 1.0, var)
    print(f"s^2: max relative difference {rel.max():.3g}")
    assert rel.max() <= 1e-9 and s2[0] == 0.0 and var[0] == 0.0


@pytest.mark.parametrize("K,eta", [(1000, 1.0), (50, 0.0), (50, 0.5), (7, 1.0), (2, 0.0), (1, 1.0)])
def test_table_is_the_float64_schedule_rounded_once(K, eta):
    gd = GaussianDiffusion()
    T = gd.num_timesteps
    sch = gd.sampling_schedule(steps=K, eta=eta)
    ts = np.asarray(sch.timesteps)
    tab = sch.table
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (T, 8) and tab.is_contiguous()
    ref = _coef64(gd, ts, eta)
    rows = tab[torch.from_numpy(ts)].double().numpy()
    for j, name in enumerate(COLS[2:], start=2):
        assert np.allclose(sch.coef64[name], ref[name], rtol=1e-13, atol=0.0), name
        err = np.abs(rows[:, j] - ref[name])
        assert bool((err <= U * np.abs(ref[name])).all()), (name, float((err / np.maximum(np.abs(ref[name]), 1e-300)).max()))
    idx = torch.from_numpy(ts)
    assert torch.equal(tab[idx, 0], gd.sqrt_recip_alphas_cumprod[idx]) and torch.equal(tab[idx, 1], gd.sqrt_recipm1_alphas_cumprod[idx])
    assert bool((tab[idx, 7] == 0).all())
    off = np.setdiff1d(np.arange(T), ts)
    assert bool(torch.isnan(tab[torch.from_numpy(off)]).all())
    last = tab[int(ts[0])]                                                   # the step that arrives at the data
    assert float(last[3]) == 0.0 and float(last[4]) == 0.0 and float(last[5]) == 1.0 and float(last[6]) == 0.0
    assert abs(float(last[2]) - 1.0) <= U
    if eta == 0.0:
        assert sch.deterministic and bool((tab[idx, 4] == 0).all())
    else:
        assert not sch.deterministic and (K == 1 or bool((tab[idx[1:], 4] > 0).all()))


def _torch_attention(qkv, heads):
    """softmax(q k^T / sqrt(d)) v on the packed layout of npcd.hip.attention.attention_qkvpacked, in torch"""
    B, n, w3 = qkv.shape
    d = w3 // heads // 3
    q, k, v = (x.transpose(1, 2) for x in qkv.view(B, n, heads, 3, d).unbind(3))
    return torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, n, heads * d)


def _tiny_model(monkeypatch):
    """The tiny denoiser on the CPU.  Its attention is a HIP kernel with no CPU form (by design), so these tests, which are about
    the sampling loop around the denoiser, put the torch restatement above in its place."""
    from npcd.models.diffusion import transformer
    monkeypatch.setattr(transformer, "attention_qkvpacked", _torch_attention)
    torch.manual_seed(0)
    m = DiffusionModel(3, 32, 48, 128, 2, 2, True).eval()
    with torch.no_grad():
        m.coords_normalization.min.fill_(-3.0); m.coords_normalization.max.fill_(3.0)
        m.coords_normalization.shift.copy_(torch.tensor([0.1, -0.2, 0.3])); m.coords_normalization.scale.fill_(0.7)
        m.feats_normalization.min.fill_(-1.0); m.feats_normalization.max.fill_(1.0)
    return m


def test_generate_on_the_cpu_with_four_deterministic_steps(monkeypatch):
    m = _tiny_model(monkeypatch)
    torch.manual_seed(3)
    coords, feats = m.generate(3, batch_size=2, progress=False, sampling_steps=4, eta=0.0)
    assert len(coords) == 3 and len(feats) == 3 and coords[0].shape == (3, 48) and feats[0].shape == (32, 48)
    assert all(bool(torch.isfinite(x).all()) for x in coords + feats)
    torch.manual_seed(3)
    coords2, feats2 = m.generate(3, batch_size=2, progress=False, sampling_steps=4, eta=0.0)
    assert torch.equal(torch.stack(coords), torch.stack(coords2)) and torch.equal(torch.stack(feats), torch.stack(feats2))


def test_generate_on_the_cpu_holds_the_given_coords(monkeypatch):
    m = _tiny_model(monkeypatch)
    given = torch.randn(3, 3, 48, generator=torch.Generator().manual_seed(9)) * 5.0          # beyond the clip range: never clipped
    out = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        coords, feats = m.generate(3, batch_size=2, progress=False, sampling_steps=4, eta=0.0, coords=given)
        assert torch.equal(torch.stack(coords), given)
        assert all(bool(torch.isfinite(x).all()) for x in feats)
        out.append(torch.stack(feats))
    assert not torch.equal(out[0], out[1])
    with pytest.raises(ValueError):
        m.generate(3, batch_size=2, progress=False, coords=given, feats=torch.zeros(3, 32, 48))
