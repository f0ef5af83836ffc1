"""The feature k-NN kernels (csrc/feature_manifold.hip) and their surfaces npcd.hip.feature_manifold and
npcd.utils.fidkid.DeviceFIDKID(prdc=True) on the GPU, at the smallest shapes at which they can go wrong: one feature, fewer rows
than a tile, ragged edges of the 16-wide instruction and of the 64-row tile, more than one row block, more than one tile of columns,
more than one split of the columns, m - 1 == k and m == k.

Bound of the real-valued tests.  The kernel forms d2 = max((nx + ny) - 2 g, +0) in float64, u = 2^-53.  To first order a D-term sum
of products carries at most D u of the sum of its absolute terms: |g| <= (nx + ny) / 2, so 2 g carries D u (nx + ny); the two norms
carry D u nx and D u ny; the two additions round values of at most 2 (nx + ny), 2 u (nx + ny) each: together (2 D + 4) u (nx + ny).
The bar is four times that, 4 (D + 2) 2^-52 (nx_i + ny_j) for the pair (i, j) -- the same pair on both sides, because the order of a row's distances is the
reference's (gaps between them are many bars wide).  The reference (the sum over the features of the squared differences, added in
float64) is itself within (D + 2) u d2 <= 2 (D + 2) u (nx + ny), a quarter of the bar.  Clamping at 0 moves a value towards the
exact one.

Counts compare a distance with a radius and must equal the reference's exactly; each real-valued count test first asserts on the
reference that no compared pair has |d2 - rho| within 100 bars, so that no rounding of either side can flip a comparison.  The
exact-integer tests (features in {-2 .. 2}: every product, norm and distance is a small integer, exact in float64) are full of equal
distances and of distances equal to a radius: they pin the multiset semantics and the strict comparison."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 64
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])


def _np_dtype(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def sliced(values, dtype):
    """values [n, D] on the GPU as a row and column slice of a taller, wider tensor: row stride D + 5."""
    n, D = values.shape
    wide = np.full((n + 3, D + 5), 77.0)
    wide[2:2 + n, 3:3 + D] = values
    t = torch.from_numpy(wide.astype(_np_dtype(dtype))).cuda()[2:2 + n, 3:3 + D]
    assert t.stride() == (D + 5, 1) and not t.is_contiguous()
    return t


@functools.lru_cache(maxsize=None)
def integer_case(n, m, D, k):
    """-> (x, y or None, the reference's lists): features in {-2 .. 2}.  Computed once, never written to."""
    from npcd.hip.feature_manifold import knn_reference
    g = np.random.RandomState(n * 1009 + (m or 0) * 31 + D)
    x = g.randint(-2, 3, size=(n, D)).astype(np.float64)
    y = None if m is None else g.randint(-2, 3, size=(m, D)).astype(np.float64)
    return x, y, knn_reference(x, y, k)


# ---- 1. exact integers, k-NN ---------------------------------------------------------------------------------------------------------------------
KNN_CASES = [(2, None, 1, 1), (9, None, 17, 8), (5, 3, 16, 3), (70, 65, 33, 5), (130, None, 70, 8), (2 * TILE + 1, None, 16, 3),
             (3, 4 * TILE + 3, 5, 2)]


@DTYPES
@pytest.mark.parametrize("n,m,D,k", KNN_CASES)
def test_knn_of_small_integers_is_exact(n, m, D, k, dtype):
    from npcd.hip.feature_manifold import knn_sq_distances
    x, y, want = integer_case(n, m, D, k)
    got = knn_sq_distances(sliced(x, dtype), None if y is None else sliced(y, dtype), k=k)
    assert got.shape == (n, k) and got.dtype == torch.float64 and got.is_cuda
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    assert not np.signbit(got).any()          # a zero distance is +0
    assert (np.diff(got, axis=1) >= 0).all()
    if n >= 9:
        assert (np.diff(want, axis=1) == 0).any()          # equal distances are there to be kept


# ---- 2. exact integers, counts -------------------------------------------------------------------------------------------------------------------
COUNT_CASES = [(9, None, 17, 8), (70, 65, 33, 5), (130, None, 70, 8), (2 * TILE + 1, None, 16, 3), (3, 4 * TILE + 3, 5, 2), (150, 131, 70, 3)]


@DTYPES
@pytest.mark.parametrize("n,m,D,k", COUNT_CASES)
def test_ball_counts_of_small_integers_are_exact(n, m, D, k, dtype):
    """rho_y: the k-th radius of y among its own rows, from the reference.  cnt and near equal the reference; a distance equal to the
    radius is outside."""
    from npcd.hip.feature_manifold import _sq_distances, ball_counts, ball_counts_reference, knn_reference
    x, y, _ = integer_case(n, m, D, k)
    y = x if y is None else y
    rho = knn_reference(y, None, k)[:, k - 1]
    want_cnt, want_near = ball_counts_reference(x, y, rho)
    if (n, m, D, k) == (150, 131, 70, 3):
        ties = int((_sq_distances(x, y) == rho[None, :]).sum())
        print(f"{ties} pairs with d2 == rho")
        assert ties >= 1          # strict < is exercised
    cnt, near = ball_counts(sliced(x, dtype), sliced(y, dtype), torch.from_numpy(rho).cuda())
    assert cnt.shape == near.shape == (n,) and cnt.dtype == torch.int32 and near.dtype == torch.float64
    np.testing.assert_array_equal(cnt.cpu().numpy(), want_cnt)
    np.testing.assert_array_equal(near.cpu().numpy(), want_near)
    assert want_cnt.max() > 0


# ---- 3. duplicates -------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_repeated_row_keeps_its_zero_and_only_the_index_is_left_out(dtype):
    from npcd.hip.feature_manifold import knn_reference, knn_sq_distances
    g = np.random.RandomState(5)
    x = g.randint(-2, 3, size=(TILE + 6, 9)).astype(np.float64)
    x[40] = x[3]                    # a pair
    x[TILE + 2] = x[20] = x[11]     # a triple, across the edge of the row block
    got = knn_sq_distances(sliced(x, dtype), None, k=4).cpu().numpy()
    np.testing.assert_array_equal(got, knn_reference(x, None, 4))
    for i in (3, 40):
        assert got[i, 0] == 0.0 and got[i, 1] > 0.0
    for i in (11, 20, TILE + 2):
        assert got[i, 0] == 0.0 and got[i, 1] == 0.0 and got[i, 2] > 0.0
    assert got[0, 0] > 0.0          # its own zero is left out by the index
    assert not np.signbit(got).any()


# ---- 4. real-valued ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def real_case(n, m, D, fp32, k=3):
    """randn features (rounded to the dtype first) with the reference's distance matrix and what follows from it."""
    from npcd.hip.feature_manifold import _sq_distances, knn_reference
    g = np.random.RandomState(D)
    x, y = (g.randn(r, D).astype(np.float32 if fp32 else np.float64).astype(np.float64) for r in (n, m))
    d2 = _sq_distances(x, y)
    rho = knn_reference(y, None, k)[:, k - 1]
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    bar = 4 * (D + 2) * 2.0 ** -52 * (nx[:, None] + ny[None, :])          # per pair
    return x, y, d2, rho, bar


@pytest.mark.parametrize("n,m,D,dtype", [(150, 131, 70, torch.float32), (150, 131, 70, torch.float64), (130, 130, 2048, torch.float32)],
                         ids=["150x131x70-fp32", "150x131x70-fp64", "130x130x2048-fp32"])
def test_real_valued_lists_minima_and_counts(n, m, D, dtype):
    from npcd.hip.feature_manifold import ball_counts, knn_sq_distances
    k = 3
    x, y, d2, rho, bar = real_case(n, m, D, dtype == torch.float32)
    dx, dy = sliced(x, dtype), sliced(y, dtype)
    order = np.argsort(d2, axis=1)[:, :k]
    rows = np.arange(n)[:, None]
    want, want_bar = d2[rows, order], bar[rows, order]
    assert (np.diff(np.sort(d2, axis=1)[:, :k + 1], axis=1) > 100 * bar.max()).all()          # the order is not in question
    got = knn_sq_distances(dx, dy, k=k).cpu().numpy()
    excess = np.abs(got - want) / want_bar
    print(f"lists: max |got - ref| = {np.abs(got - want).max():.3e}, {excess.max():.3e} of the bar (bar about {want_bar.mean():.3e})")
    assert (excess <= 1).all()
    # no compared pair within 100 bars of its radius: the counts must be the reference's
    margin = (np.abs(d2 - rho[None, :]) / bar).min()
    print(f"smallest |d2 - rho| = {np.abs(d2 - rho[None, :]).min():.3e}, {margin:.3e} bars")
    assert margin > 100
    cnt, near = ball_counts(dx, dy, torch.from_numpy(rho).cuda())
    np.testing.assert_array_equal(cnt.cpu().numpy(), (d2 < rho[None, :]).sum(1))
    near = near.cpu().numpy()
    assert near.shape == (n,)
    near_excess = np.abs(near - d2.min(1)) / bar[np.arange(n), d2.argmin(1)]
    print(f"near: {near_excess.max():.3e} of the bar")
    assert (near_excess <= 1).all()
    np.testing.assert_array_equal(near, got[:, 0])          # the same pair through both entry points: the same bits


@DTYPES
def test_real_valued_self_lists(dtype):
    """The set against itself: the index is left out, every other entry is within the bar."""
    from npcd.hip.feature_manifold import knn_sq_distances
    from npcd.hip.feature_manifold import _sq_distances
    k, D = 3, 70
    x = real_case(150, 131, D, dtype == torch.float32)[0]
    d2 = _sq_distances(x, x)
    d2[np.arange(len(x)), np.arange(len(x))] = np.inf
    nx = (x * x).sum(1)
    bar = 4 * (D + 2) * 2.0 ** -52 * (nx[:, None] + nx[None, :])
    order = np.argsort(d2, axis=1)[:, :k]
    rows = np.arange(len(x))[:, None]
    got = knn_sq_distances(sliced(x, dtype), None, k=k).cpu().numpy()
    assert (np.abs(got - d2[rows, order]) <= bar[rows, order]).all() and (got > 0).all()


# ---- 5. partition and repetition -------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_the_same_bits_for_every_split_and_on_every_run(dtype):
    from npcd.hip.feature_manifold import ball_counts, knn_sq_distances
    n, m, D, k = 70, 5 * TILE + 3, 40, 5
    g = torch.Generator().manual_seed(7)
    x, y = torch.randn(n, D, generator=g, dtype=dtype).cuda(), torch.randn(m, D, generator=g, dtype=dtype).cuda()
    rho = knn_sq_distances(y, None, k=k, splits=1)[:, k - 1].contiguous()
    lists, selfs, balls = [], [], []
    for splits in (1, 2, 3, 0, 1, 3):
        lists.append(knn_sq_distances(x, y, k=k, splits=splits))
        selfs.append(knn_sq_distances(y, None, k=k, splits=splits))
        balls.append(ball_counts(x, y, rho, splits=splits))
    for other in lists[1:]:
        assert torch.equal(other, lists[0])
    for other in selfs[1:]:
        assert torch.equal(other, selfs[0])
    for cnt, near in balls[1:]:
        assert torch.equal(cnt, balls[0][0]) and torch.equal(near, balls[0][1])
    assert torch.equal(selfs[0][:, k - 1], rho) and int(balls[0][0].sum()) > 0 and bool(torch.isfinite(lists[0]).all())


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------------------------
PRDC = ("precision", "recall", "density", "coverage")


def fed(metric, reals, fakes):
    """Reals in chunks of 251, fakes in chunks of 32."""
    for mode, feats, chunk in (("reals", reals, 251), ("fakes", fakes, 32)):
        for i in range(0, feats.shape[0], chunk):
            metric.feed(feats[i:i + chunk], mode)
    return metric


@functools.lru_cache(maxsize=None)
def end_to_end_features():
    g = torch.Generator().manual_seed(3)
    return torch.randn(640, 24, generator=g), torch.randn(640, 24, generator=g) * 1.1 + 0.15


@pytest.mark.parametrize("nearest_k,prdc_rows", [(3, None), (5, None), (5, 200)])
def test_device_fidkid_with_prdc_agrees_with_the_host(nearest_k, prdc_rows, monkeypatch):
    from npcd.utils.fidkid import FIDKID, DeviceFIDKID
    reals, fakes = end_to_end_features()
    host = fed(FIDKID(num_images=640, num_subsets=3, max_subset_size=100, prdc=True, nearest_k=nearest_k, prdc_rows=prdc_rows), reals, fakes)
    host.summary()
    kwargs = dict(num_images=640, num_subsets=3, max_subset_size=100, device="cuda")
    plain = fed(DeviceFIDKID(rng=np.random.RandomState(1), **kwargs), reals.cuda(), fakes.cuda())
    plain_out = plain.summary()
    dev = fed(DeviceFIDKID(rng=np.random.RandomState(1), prdc=True, nearest_k=nearest_k, prdc_rows=prdc_rows, **kwargs), reals.cuda(), fakes.cuda())
    calls, cpu = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **kw: (calls.append(1), cpu(self, *a, **kw))[1])
    out = dev.summary()
    monkeypatch.undo()
    assert len(calls) == 1          # the four numbers ride in the one read-back
    assert len(out) == 4 and out == plain_out          # fid and kid are untouched, bit for bit
    assert set(plain._result_dict) == {"fid", "fid_mean", "fid_cov", "kid"}
    assert set(dev._result_dict) == set(plain._result_dict) | set(PRDC)
    assert all(dev._result_dict[key] == plain._result_dict[key] for key in plain._result_dict)
    got, want = {key: dev._result_dict[key] for key in PRDC}, {key: host._result_dict[key] for key in PRDC}
    print(got)
    assert got == want          # ratios of equal integers
    assert 0 < got["precision"] < 1 and 0 < got["recall"] < 1 and 0 < got["coverage"] < 1 and got["density"] > 0
    assert dev._result_str == plain._result_str + host._result_str[len(host._result_str.split(", P/R")[0]):]


def test_device_prdc_known_answers():
    from npcd.utils.fidkid import DeviceFIDKID
    reals = end_to_end_features()[0][:200].cuda()
    for fakes, want in ((reals.clone(), 1.0), (reals + 1000.0, 0.0)):
        m = DeviceFIDKID(num_images=200, num_subsets=2, max_subset_size=50, device="cuda", prdc=True, nearest_k=5)
        fed(m, reals, fakes).summary()
        got = m._result_dict
        assert got["precision"] == got["recall"] == got["coverage"] == want, got
        if want == 0.0:
            assert got["density"] == 0.0
        else:
            assert got["density"] > 0.5
