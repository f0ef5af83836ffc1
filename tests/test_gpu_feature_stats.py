"""The feature-statistics kernels (csrc/feature_stats.hip) and their surfaces npcd.hip.feature_stats and
npcd.utils.fidkid.DeviceFIDKID on the GPU, at the smallest shapes at which they can go wrong: one row, one feature, ragged edges of
the 16-wide instruction and of the workgroup's tile, more than one tile, more than one flush.

Features are non-negative, like Inception pool features, so the sum of the absolute terms of every reduction is the reduction itself.

Bounds of the real-valued tests.  A D-term float64 product sum plus divide, add and cube perturbs a kernel entry by at most
3 (D + 4) u relative, a reduction of chain length L adds L u, u = 2^-53: below 8e-13 for D <= 2048, m <= 1000, and 4096 u = 4.5e-13 for
the rows of the moments.  The bars (1e-12 of the largest sum of absolute terms for cov, 1e-13 max|x| for the mean, 1e-10 of the sum for
the KID sums) keep two orders of margin above that; a host run with another summation order lands at 1-2e-15 of that scale."""
import functools
import pickle

import numpy as np
import pytest
import torch

from test_feature_stats_cpu import feats

pytestmark = pytest.mark.gpu


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


# ---- 1. exact integers, moments ------------------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 1), (3, 17), (5, 16), (70, 65), (259, "tile+1"), (1027, 130)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("shifted", [False, True], ids=["unshifted", "integer_shift"])
@pytest.mark.parametrize("rows,D", MOMENT_SHAPES)
def test_moments_of_small_integers_are_exact(rows, D, shifted, dtype):
    """X in {0 .. 7}, a column slice of a wider and taller tensor (row stride D + 5, rows [2, 2 + rows)): sum and the upper tiles of
    gram equal the int64 result exactly on top of what the accumulators held, entries of tiles below the diagonal keep their bits,
    and the finished cov is symmetric bit for bit."""
    from npcd.hip import feature_stats as fs
    T = fs.tile()
    D = T + 1 if D == "tile+1" else D
    g = np.random.RandomState(rows * 131 + D)
    wide = g.randint(0, 8, size=(rows + 3, D + 5))
    shift = g.randint(0, 4, size=D) if shifted else None
    z = wide[2:2 + rows, 2:2 + D].astype(np.int64) - (0 if shift is None else shift)
    want_sum, want_gram = z.sum(0), z.T @ z
    x = torch.from_numpy(wide.astype(_np_dtype(dtype))).cuda()[:, 2:2 + D]
    assert x.stride() == (D + 5, 1)
    dev_shift = None if shift is None else torch.from_numpy(shift.astype(np.float64)).cuda()
    total = torch.full((D,), 5.0, dtype=torch.float64, device="cuda")
    gram = torch.full((D, D), 3.0, dtype=torch.float64, device="cuda")
    fs.moments_update(x, 2, 2 + rows, dev_shift, total, gram)
    total, gram = total.cpu().numpy(), gram.cpu().numpy()
    np.testing.assert_array_equal(total, 5.0 + want_sum)
    blocks = np.arange(D) // T
    upper = blocks[None, :] >= blocks[:, None]
    np.testing.assert_array_equal(gram[upper], 3.0 + want_gram[upper])
    np.testing.assert_array_equal(gram[~upper], 3.0)
    if rows >= 2:
        acc = fs.FeatureMoments(D, "cuda", shift=shift, block_rows=256)
        acc.add(x[2:2 + rows])
        mean, cov = acc.finalize()
        assert acc.rows == acc.n == rows and torch.equal(acc.features(), x[2:2 + rows])
        assert torch.equal(cov, cov.T)
        _, _, ref_mean, ref_cov = fs.moments_reference(wide[2:2 + rows, 2:2 + D], shift)
        scale = float((np.abs(z).T @ np.abs(z)).max()) / (rows - 1)
        assert np.abs(mean.cpu().numpy() - ref_mean).max() <= 1e-13 * 7
        assert np.abs(cov.cpu().numpy() - ref_cov).max() <= 1e-12 * max(scale, 1.0)


# ---- 2. exact integers, KID sums -----------------------------------------------------------------------------------------------------------------
def _subsets(S, m, Nf, Nr, seed):
    g = np.random.RandomState(seed)
    return (np.stack([g.choice(Nf, m, replace=False) for _ in range(S)]), np.stack([g.choice(Nr, m, replace=False) for _ in range(S)]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("S,m,Nf,Nr", [(1, 2, 2, 2), (3, 70, 150, 120), (2, 64, 64, 90), (2, 129, 200, 129), (1, "2*tile+1", 0, 0)])
def test_kid_sums_of_small_integers_are_exact(S, m, Nf, Nr, dtype):
    """Features in {0 .. 3}, D = 16: every k is a multiple of 1 / 4096 below 1,000 and every sum is exact."""
    from npcd.hip import feature_stats as fs
    if m == "2*tile+1":
        m = 2 * fs.kid_tile() + 1
        Nf, Nr = m + 4, m
    D = 16
    g = np.random.RandomState(S * 1000 + m)
    fake, real = g.randint(0, 4, size=(Nf, D + 3)), g.randint(0, 4, size=(Nr, D))
    idx_f, idx_r = _subsets(S, m, Nf, Nr, seed=m)
    want = np.empty((S, 3))
    for s in range(S):
        x, y = fake[idx_f[s], 1:1 + D].astype(np.int64), real[idx_r[s]].astype(np.int64)
        off = ~np.eye(m, dtype=bool)
        for w, (a, b, mask) in enumerate(((x, x, off), (y, y, off), (x, y, np.ones((m, m), dtype=bool)))):
            t = (a @ b.T).astype(np.float64) / D + 1.0
            k = t * t * t
            assert (k * 4096 == np.round(k * 4096)).all() and k.max() < 1000
            want[s, w] = k[mask].sum()
    dev_fake = torch.from_numpy(fake.astype(_np_dtype(dtype))).cuda()[:, 1:1 + D]          # row stride D + 3
    dev_real = torch.from_numpy(real.astype(_np_dtype(dtype))).cuda()
    got = fs.kid_subsets(dev_fake, dev_real, idx_f, idx_r)
    assert got.shape == (S, 3) and got.dtype == torch.float64 and got.is_cuda
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(want, fs.kid_sums_reference(fake[:, 1:1 + D], real, idx_f, idx_r))


# ---- 3. real-valued parity -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _moment_case(n, D, dtype):
    """(features, np.mean, np.cov, the largest sum of absolute terms of a cov entry), computed once; the features are never changed."""
    if D <= 256:
        x = feats(n, D, 7, shift=0.5)
    else:          # the same kind of features without the D x D mixing product: a common factor correlates the columns
        g = np.random.RandomState(8)
        x = np.abs(g.randn(n, D) + 0.7 * g.randn(n, 1) + 0.5)
    x = x.astype(_np_dtype(dtype))
    x64 = x.astype(np.float64)
    x.setflags(write=False)
    return x, x64.mean(0), np.cov(x64, rowvar=False), float((x64 * x64).sum(0).max()) / (n - 1)


MOMENT_CASES = [(600, 24, torch.float64), (600, 24, torch.float32), (1100, 136, torch.float64), (1100, 136, torch.float32),
                (4096, 2048, torch.float32)]


def _check_moments(mean, cov, n, D, dtype, what=""):
    x, ref_mean, ref_cov, scale = _moment_case(n, D, dtype)
    mean_err, cov_err = np.abs(mean.cpu().numpy() - ref_mean).max(), np.abs(cov.cpu().numpy() - ref_cov).max()
    print(f"{what}({n}, {D}) {dtype}: |mean - ref| {mean_err:.3g} (bar {1e-13 * np.abs(x).max():.3g}), |cov - ref| {cov_err:.3g} "
          f"(bar {1e-12 * scale:.3g})")
    assert mean_err <= 1e-13 * float(np.abs(x).max())
    assert cov_err <= 1e-12 * scale


@pytest.mark.parametrize("shifted", [False, True], ids=["unshifted", "shifted"])
@pytest.mark.parametrize("n,D,dtype", MOMENT_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_moments_agree_with_numpy(n, D, dtype, shifted):
    from npcd.hip import feature_stats as fs
    x = _moment_case(n, D, dtype)[0]
    shift = x[:100].astype(np.float64).mean(0) if shifted else None
    acc = fs.FeatureMoments(D, "cuda", shift=shift, max_rows=n)
    acc.add(torch.tensor(x).cuda())          # a copy: the shared features are read-only
    mean, cov = acc.finalize()
    assert mean.dtype == cov.dtype == torch.float64 and cov.shape == (D, D) and torch.equal(cov, cov.T)
    _check_moments(mean, cov, n, D, dtype)


@pytest.mark.parametrize("S,m,D,dtype", [(3, 70, 36, torch.float64), (3, 70, 36, torch.float32), (2, 129, 2048, torch.float32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_kid_sums_agree_with_the_host_restatement(S, m, D, dtype):
    from npcd.hip import feature_stats as fs
    g = np.random.RandomState(D)
    fake = np.abs(g.randn(m + 30, D) + 0.3).astype(_np_dtype(dtype))
    real = np.abs(g.randn(m + 11, D) * 1.2).astype(_np_dtype(dtype))
    idx_f, idx_r = _subsets(S, m, m + 30, m + 11, seed=5)
    want = fs.kid_sums_reference(fake, real, idx_f, idx_r)
    got = fs.kid_subsets(torch.from_numpy(fake).cuda(), torch.from_numpy(real).cuda(), idx_f, idx_r).cpu().numpy()
    rel = np.abs(got - want) / want
    print(f"KID sums ({S}, {m}, D = {D}) {dtype}: relative differences up to {rel.max():.3g}")
    assert (want > 0).all() and (rel <= 1e-10).all()


# ---- 4. reproducibility and cut-invariance -------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_how_the_stream_is_cut():
    """(1100, 136) as one call, in 32s and in 251s (the protocol's two chunk sizes) with block_rows = 256: mean, cov and the store are
    the same bits; two accumulators over the two halves, merged, agree with one within the bar of the parity test."""
    from npcd.hip import feature_stats as fs
    n, D, dtype = 1100, 136, torch.float32
    x = torch.tensor(_moment_case(n, D, dtype)[0]).cuda()
    shift = x[:50].double().mean(0).cpu().numpy()
    results = []
    for chunk in (n, 32, 251):
        acc = fs.FeatureMoments(D, "cuda", shift=shift, max_rows=n, block_rows=256)
        for i in range(0, n, chunk):
            acc.add(x[i:i + chunk])
        mean, cov = acc.finalize()
        again = acc.finalize()
        assert torch.equal(again[0], mean) and torch.equal(again[1], cov) and acc.rows == n
        results.append((mean, cov, acc.features().clone()))
    for mean, cov, store in results[1:]:
        assert torch.equal(mean, results[0][0]) and torch.equal(cov, results[0][1]) and torch.equal(store, results[0][2])
    assert torch.equal(results[0][2], x)
    _check_moments(results[0][0], results[0][1], n, D, dtype, "block_rows 256 ")
    halves = [fs.FeatureMoments(D, "cuda", shift=shift, block_rows=256) for _ in range(2)]
    halves[0].add(x[:n // 2]), halves[1].add(x[n // 2:])
    merged = halves[0].merge_(halves[1])
    assert merged.n == n and merged.rows == n // 2
    _check_moments(*merged.finalize(), n, D, dtype, "merged ")
    loose = fs.FeatureMoments(D, "cuda", shift=shift, keep_features=False)
    for i in range(0, n, 251):
        loose.add(x[i:i + 251])
    _check_moments(*loose.finalize(), n, D, dtype, "keep_features=False ")


def test_kid_subsets_is_reproducible():
    from npcd.hip import feature_stats as fs
    g = np.random.RandomState(3)
    fake, real = (torch.from_numpy(np.abs(g.randn(k, 40)).astype(np.float32)).cuda() for k in (150, 140))
    idx_f, idx_r = _subsets(4, 131, 150, 140, seed=9)
    first = fs.kid_subsets(fake, real, idx_f, idx_r)
    assert torch.equal(first, fs.kid_subsets(fake, real, idx_f, idx_r))
    # a subset's sums do not depend on the other subsets of the call
    assert torch.equal(first[2:3], fs.kid_subsets(fake, real, idx_f[2:3], idx_r[2:3]))


# ---- 5. DeviceFIDKID against FIDKID --------------------------------------------------------------------------------------------------------------
def _projection_pair(d_in, D, seed=0):
    """The same fixed random projection with an abs as a float64 extractor on the host and on the device."""
    P = torch.from_numpy(np.random.RandomState(seed).randn(d_in, D) / d_in ** 0.5)
    P_dev = P.cuda()
    return (lambda im: (im.double().flatten(1) @ P).abs()), (lambda im: (im.double().flatten(1) @ P_dev).abs())


@pytest.mark.parametrize("with_pickle", [True, False], ids=["pickle", "reals_fed"])
def test_device_fidkid_follows_fidkid(tmp_path, with_pickle):
    from npcd.utils.fidkid import FIDKID, DeviceFIDKID
    N, D = 640, 24
    g = torch.Generator().manual_seed(1)
    reals = torch.rand(N + 20, 3, 8, 8, generator=g, dtype=torch.float64)
    fakes = torch.rand(N + 20, 3, 8, 8, generator=g, dtype=torch.float64) * 0.8 + 0.3 * torch.rand(N + 20, 1, 1, 1, generator=g, dtype=torch.float64)
    host_extractor, dev_extractor = _projection_pair(3 * 8 * 8, D)
    kwargs = dict(num_images=N, num_subsets=10, max_subset_size=200)
    if with_pickle:
        rf = host_extractor(reals[:N]).numpy()
        path = tmp_path / "ref.pkl"
        with open(path, "wb") as f:
            pickle.dump({"mean": rf.mean(0), "cov": np.cov(rf, rowvar=False), "feats_np": rf}, f)
        kwargs["inception_pkl"] = str(path)
    host, dev = FIDKID(feature_extractor=host_extractor, **kwargs), DeviceFIDKID(feature_extractor=dev_extractor, device="cuda", **kwargs)
    host.prepare(), dev.prepare()
    for mode, images in (("reals", reals), ("fakes", fakes)):
        for i in range(0, N + 20, 32):          # the last chunk is overfull: 20 of its 32 images are beyond the cap
            batch = images[i:i + 32]
            assert host.feed(batch, mode) == dev.feed(batch.cuda(), mode), (mode, i)
        assert host.feed(images[:4], mode) == dev.feed(images[:4].cuda(), mode) == 0
    assert dev.num_fake_feeded == host.num_fake_feeded == N and dev.num_real_feeded == host.num_real_feeded == N
    np.random.seed(3)
    want = host.summary()
    np.random.seed(3)
    got = dev.summary()
    print(f"FIDKID {want}\nDeviceFIDKID {got}")
    assert set(dev._result_dict) == set(host._result_dict) == {"fid", "fid_mean", "fid_cov", "kid"}
    for key in ("fid", "fid_mean", "fid_cov"):
        assert dev._result_dict[key] == pytest.approx(host._result_dict[key], rel=1e-8), key
    assert dev._result_dict["kid"] == pytest.approx(host._result_dict["kid"], rel=1e-8, abs=1e-9)
    assert got == tuple(dev._result_dict[k] for k in ("fid", "fid_mean", "fid_cov", "kid")) and dev._result_str.count("(") == 1
    assert want[0] > 1e-3 and abs(want[3]) > 1e-3          # the two sides differ: nothing above compares zeros
    with pytest.raises(RuntimeError, match="feature_extractor"):
        DeviceFIDKID(num_images=4, device="cuda").feed(torch.zeros(2, 3, 8, 8, device="cuda"), "fakes")


# ---- 6. no host wait in feed ---------------------------------------------------------------------------------------------------------------------
def test_feed_does_not_wait_for_the_device():
    from npcd.utils.fidkid import DeviceFIDKID
    _, dev_extractor = _projection_pair(3 * 8 * 8, 24)
    m = DeviceFIDKID(num_images=700, feature_extractor=dev_extractor, device="cuda", block_rows=64)
    images = torch.rand(8, 32, 3, 8, 8, device="cuda")
    features = torch.rand(3, 32, 24, device="cuda", dtype=torch.float64)
    m.feed(images[0], "fakes"), m.feed(images[0], "reals")          # the first feeds allocate and load the code objects
    torch.cuda.synchronize()
    mask = torch.rand(64, device="cuda") > 0.5
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tripped = False
        try:
            torch.nonzero(mask)
        except RuntimeError:
            tripped = True
        if tripped:
            for batch in images[1:]:          # 224 more rows: three flushes of 64 on each side
                assert m.feed(batch, "fakes") == 32 and m.feed(batch * 0.5, "reals") == 32
            for batch in features:
                assert m.feed(batch, "fakes") == 32
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not tripped:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not trip on torch.nonzero on this torch build")
    assert m.num_fake_feeded == 8 * 32 + 3 * 32 and m.num_real_feeded == 8 * 32


# ---- 7. the feed= hook of sample_and_render --------------------------------------------------------------------------------------------------------
def test_the_feed_hook_takes_a_chunk_of_rendered_views():
    from npcd.utils.fidkid import DeviceFIDKID
    _, dev_extractor = _projection_pair(3 * 16 * 16, 24)
    m = DeviceFIDKID(num_images=300, feature_extractor=dev_extractor, device="cuda")
    feed = lambda im: m.feed(im * 2 - 1, "fakes")          # noqa: E731  (the hook as npcd.eval.sample_and_render takes it)
    views = torch.rand(251, 3, 16, 16, device="cuda")
    assert feed(views) == 251 and m.num_fake_feeded == 251
    assert feed(views) == 49 and m.num_fake_feeded == 300 and feed(views) == 0
    stored = m._moments["fakes"].features()
    assert stored.shape == (300, 24) and torch.equal(stored[:251], dev_extractor(views * 2 - 1))
    assert torch.allclose(stored[251:], stored[:49], rtol=1e-12, atol=0)          # the 49 went through the extractor as a batch of their own
