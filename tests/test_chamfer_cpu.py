"""The Chamfer kernel and the shape metrics, everything that needs no GPU: the oracle and the float64 metric implementation that the GPU
tests share, the wrapper's refusals, the host-side query and refusals of the C entry point, metrics_from_chamfer and normalize_clouds
on CPU tensors, the kernels' resources as the compiler reports them."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_kernel_resources import _compile

U = 2.0 ** -24          # unit roundoff of fp32


# ---- oracle, from the spec of DESIGN.md 5.7 ------------------------------------------------------------------------------------------
def chamfer_oracle(x, y, x_len=None, y_len=None):
    """Directed Chamfer matrix [M, N] in float64: the per-point minima in numpy fp32, the squared distance evaluated exactly as
    written, ((dx dx + dy dy) + dz dz) (numpy never contracts); then a float64 sum over the valid points and a float64 division."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    (M, P, _), (N, Q, _) = x.shape, y.shape
    out = np.empty((M, N), dtype=np.float64)
    beyond = None if y_len is None else np.arange(Q)[None, None, :] >= np.asarray(y_len).reshape(N, 1, 1)
    for i in range(M):
        Lx = P if x_len is None else int(x_len[i])
        total = np.zeros(N, dtype=np.float64)
        for p0 in range(0, Lx, 512):
            a = x[i, p0:min(Lx, p0 + 512)]
            dx = a[None, :, None, 0] - y[:, None, :, 0]
            dy = a[None, :, None, 1] - y[:, None, :, 1]
            dz = a[None, :, None, 2] - y[:, None, :, 2]
            d = (dx * dx + dy * dy) + dz * dz
            assert d.dtype == np.float32
            if beyond is not None:
                d = np.where(beyond, np.float32(np.inf), d)
            total += d.min(axis=2).astype(np.float64).sum(axis=1)
        out[i] = total / Lx
    return out


def chamfer_matrix_oracle(x, y=None, x_len=None, y_len=None):
    """The symmetric distance of the metrics: directed(x, y) + directed(y, x).T, float64."""
    if y is None:
        d = chamfer_oracle(x, x, x_len, x_len)
        return d + d.T
    return chamfer_oracle(x, y, x_len, y_len) + chamfer_oracle(y, x, y_len, x_len).T


def chamfer_float64(x, y):
    """Pure float64, no fp32 anywhere: what the oracle's form is measured against."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.stack([((xi[None, :, None, :] - y[:, None, :, :]) ** 2).sum(-1).min(axis=2).mean(axis=1) for xi in x])


# ---- the three definitions in float64 numpy ------------------------------------------------------------------------------------------
def metrics_float64(cd, M):
    """cd [T, T] float64, rows / columns [:M] generated, [M:] reference.  np.argmin returns the first (lowest) index among equals."""
    cd = np.asarray(cd, dtype=np.float64)
    T = cd.shape[0]
    N = T - M
    gen_ref = cd[:M, M:]
    others = cd.copy()
    np.fill_diagonal(others, np.inf)
    nearest = others.argmin(axis=1)
    side = np.arange(T) < M
    return {"mmd_cd": float(gen_ref.min(axis=0).mean()), "cov_matched": len(set(gen_ref.argmin(axis=1).tolist())),
            "nna_correct": int((side[nearest] == side).sum()), "num_generated": M, "num_reference": N}


def smallest_argmin_gap(cd, M):
    """The smallest relative gap between the best and the second-best candidate over every arg-min the metrics take: each generated
    cloud's nearest reference (COV) and each cloud's nearest other cloud (1-NNA)."""
    cd = np.asarray(cd, dtype=np.float64)
    others = cd.copy()
    np.fill_diagonal(others, np.inf)
    gaps = []
    for rows in (cd[:M, M:], others):
        two = np.sort(rows, axis=1)[:, :2]
        gaps.append(((two[:, 1] - two[:, 0]) / two[:, 1]).min())
    return float(min(gaps))


def check_metrics(got, want, bar):
    """Counts equal, MMD within the relative bar; the derived ratios follow from the counts."""
    assert got["cov_matched"] == want["cov_matched"] and got["nna_correct"] == want["nna_correct"], (got, want)
    M, N = want["num_generated"], want["num_reference"]
    assert (got["num_generated"], got["num_reference"]) == (M, N)
    assert got["cov_cd"] == want["cov_matched"] / N and got["nna_cd"] == want["nna_correct"] / (M + N)
    err = abs(got["mmd_cd"] - want["mmd_cd"]) / want["mmd_cd"]
    print(f"mmd_cd {got['mmd_cd']:.8g} against {want['mmd_cd']:.8g}: error / bar = {err / bar:.3f}")
    assert err <= bar, (got["mmd_cd"], want["mmd_cd"], err, bar)


@functools.lru_cache(maxsize=None)
def metric_sets():
    """The sets of the metric tests: 20 generated and 24 reference clouds of 64 points, anisotropically scaled; and the twins of the
    reference set, 1e-3 away."""
    def clouds(seed, n):
        rng = np.random.default_rng(seed)
        c = rng.standard_normal((n, 64, 3)).astype(np.float32)
        c *= rng.uniform(0.5, 1.5, (n, 1, 3)).astype(np.float32)
        return c
    gen, ref = clouds(1, 20), clouds(2, 24)
    twins = ref + np.float32(1e-3) * np.random.default_rng(3).standard_normal(ref.shape).astype(np.float32)
    assert twins.dtype == np.float32
    return gen, ref, twins


@functools.lru_cache(maxsize=None)
def metric_matrices():
    """The oracle's float64 union matrices of (generated, reference) and (twins, reference), computed once."""
    gen, ref, twins = metric_sets()
    return chamfer_matrix_oracle(np.concatenate([gen, ref])), chamfer_matrix_oracle(np.concatenate([twins, ref]))


BAR_64 = (64 + 3) * U          # chamfer_matrix at 64 points: (max(Lx, Ly) + 3) u


def test_the_metric_sets_meet_their_precondition():
    """Asserted, not skipped: every arg-min is decided by more than 4 x the bar, so fp32 rounding cannot change a count."""
    plain, twin = metric_matrices()
    gap = smallest_argmin_gap(plain, 20)
    want = metrics_float64(plain, 20)
    print(f"smallest gap {gap:.3g} against bar {BAR_64:.3g}; COV {want['cov_matched']}/24, 1-NNA {want['nna_correct']}/44, "
          f"MMD {want['mmd_cd']:.5f}")
    assert gap > 4 * BAR_64
    assert (want["cov_matched"], want["nna_correct"]) == (7, 21) and abs(want["mmd_cd"] - 0.80776) < 5e-6
    assert smallest_argmin_gap(twin, 24) > 4 * BAR_64
    want = metrics_float64(twin, 24)
    assert (want["cov_matched"], want["nna_correct"]) == (24, 0) and 5e-6 < want["mmd_cd"] < 7e-6


def test_the_oracle_agrees_with_float64_on_the_metric_sets():
    gen, ref, _ = metric_sets()
    a, b = chamfer_oracle(gen[:4], ref[:5]), chamfer_float64(gen[:4], ref[:5])
    assert np.abs(a - b).max() <= 1e-6 * b.max()


def test_metrics_from_chamfer_on_the_metric_sets():
    from npcd.eval import metrics_from_chamfer
    plain, twin = metric_matrices()
    for cd, M in ((plain, 20), (twin, 24)):
        for t in (torch.from_numpy(cd), torch.from_numpy(cd.astype(np.float32))):          # float64 as it is, and rounded to fp32
            got = metrics_from_chamfer(t, M)
            check_metrics(got, metrics_float64(cd, M), 1e-15 if t.dtype == torch.float64 else U)
            assert isinstance(got["cov_matched"], int) and isinstance(got["nna_correct"], int) and isinstance(got["mmd_cd"], float)


def test_ties_go_to_the_lowest_index():
    """2 generated (0, 1) and 3 reference clouds (2, 3, 4).  Generated 0 is equally near references 2 and 3 -> 2; generated 1 is
    nearest 2 as well, so COV matches one reference, where the highest index of the tie would match two.  Cloud 4 is equally near 1
    and 3 -> 1, the other side, where 3 would count as correct."""
    from npcd.eval import metrics_from_chamfer
    cd = np.array([[0, 9, 2, 2, 8],
                   [9, 0, 1, 5, 3],
                   [2, 1, 0, 7, 6],
                   [2, 5, 7, 0, 3],
                   [8, 3, 6, 3, 0]], dtype=np.float32)
    assert (cd == cd.T).all()
    got = metrics_from_chamfer(torch.from_numpy(cd), 2)
    # nearest others: 0 -> 2 (tie 2 / 3), 1 -> 2, 2 -> 1, 3 -> 0, 4 -> 1 (tie 1 / 3): none on the same side
    assert got["cov_matched"] == 1 and got["nna_correct"] == 0, got
    assert got["mmd_cd"] == (1 + 2 + 3) / 3 and got["cov_cd"] == 1 / 3 and got["nna_cd"] == 0.0
    assert (got["num_generated"], got["num_reference"]) == (2, 3)
    check_metrics(got, metrics_float64(cd, 2), 1e-15)
    with pytest.raises(ValueError, match="square"):
        metrics_from_chamfer(torch.zeros(3, 4), 1)
    with pytest.raises(ValueError, match="reference"):
        metrics_from_chamfer(torch.zeros(3, 3), 3)


def normalize_bbox_numpy(c):
    c = np.asarray(c, dtype=np.float64)
    lo, hi = c.min(axis=1, keepdims=True), c.max(axis=1, keepdims=True)
    return (c - (lo + hi) / 2) / ((hi - lo).max(axis=2, keepdims=True) / 2)


def test_normalize_clouds_against_numpy():
    from npcd.eval import normalize_clouds
    gen, _, _ = metric_sets()
    c = gen[:6] * np.float32(3) + np.float32(5)
    got = normalize_clouds(torch.from_numpy(c), "bbox")
    assert got.dtype == torch.float32 and got.shape == c.shape
    np.testing.assert_allclose(got.numpy(), normalize_bbox_numpy(c), rtol=0, atol=4e-6)          # coordinates near 5 in fp32: 5 u each
    lo, hi = got.min(dim=1).values, got.max(dim=1).values
    assert float((hi - lo).max(dim=1).values.sub(2).abs().max()) < 1e-5 and float((hi + lo).abs().max()) < 1e-5
    assert normalize_clouds(torch.from_numpy(c), None) is not None and torch.equal(normalize_clouds(torch.from_numpy(c), None), torch.from_numpy(c))
    with pytest.raises(ValueError, match="mode"):
        normalize_clouds(torch.from_numpy(c), "sphere")


def test_eval_exports_the_four_names_without_a_gpu():
    import npcd.eval
    from npcd.eval import shapes
    for name in ("metrics_from_chamfer", "normalize_clouds", "shape_metrics", "evaluate_shapes"):
        assert getattr(npcd.eval, name) is getattr(shapes, name)


# ---- the wrapper and the C entry point -----------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from npcd.hip.chamfer import chamfer_directed, chamfer_matrix
    from npcd.eval import shape_metrics
    with pytest.raises(RuntimeError, match="GPU"):
        chamfer_directed(torch.zeros(2, 10, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        chamfer_matrix(torch.zeros(2, 10, 3), torch.zeros(3, 7, 3), x_lengths=[10, 3], y_lengths=torch.tensor([7, 1, 2]))
    with pytest.raises(RuntimeError, match="GPU"):
        shape_metrics(torch.zeros(2, 10, 3), torch.zeros(3, 10, 3))


def test_bad_arguments_are_refused_on_the_host():
    from npcd.hip.chamfer import chamfer_directed, chamfer_matrix
    x, y = torch.zeros(2, 10, 3), torch.zeros(3, 7, 3)
    for fn in (chamfer_directed, chamfer_matrix):
        with pytest.raises(RuntimeError, match="supports fp32"):
            fn(x.double())
        with pytest.raises(RuntimeError, match="supports fp32"):
            fn(x, y.half())
        with pytest.raises(ValueError, match=r"\[n, P, 3\]"):
            fn(torch.zeros(2, 10, 2))
        with pytest.raises(ValueError, match=r"\[n, P, 3\]"):
            fn(x, torch.zeros(7, 3))
        with pytest.raises(ValueError, match=r"\[n, P, 3\]"):
            fn(torch.zeros(0, 10, 3))
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=[10, 11])
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=[0, 10])
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=torch.tensor([10, -1]))
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=[10])
        with pytest.raises(ValueError, match="y_lengths"):
            fn(x, y, y_lengths=[7, 7, 8])
        with pytest.raises(ValueError, match="y_lengths"):
            fn(x, y, y_lengths=[7, 7])
        with pytest.raises(ValueError, match="y_lengths"):
            fn(x, y_lengths=[10, 10])


def test_host_side_query_and_refusals():
    from npcd import hip
    from npcd.hip import chamfer
    L = hip.lib()
    largest = L.npcd_chamfer_max_points()
    assert largest >= 4096 and chamfer.max_points() == largest
    null = ctypes.c_void_p(0)
    unsupported = -2
    # refused before any pointer is looked at and before any launch: null pointers, no GPU.  16,384 clouds a side is the launch limit
    for M, P, N, Q in ((0, 8, 1, 8), (1, 0, 1, 8), (1, 8, 0, 8), (1, 8, 1, 0), (-1, 8, 1, 8), (1, -8, 1, 8), (1, 8, -1, 8), (1, 8, 1, -8),
                       (1, largest + 1, 1, 8), (1, 8, 1, largest + 1), (1 << 30, 8, 1, 8), (1, 8, 1 << 30, 8), (16385, 8, 1, 8), (1, 8, 16385, 8)):
        assert L.npcd_chamfer_directed(null, null, null, null, null, M, P, N, Q, null) == unsupported, (M, P, N, Q)
    assert L.npcd_chamfer_directed(null, null, null, null, null, 16384, largest, 16384, largest, null) == -1          # supported, but no buffers


# ---- the kernels' resources ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chamfer_kernels(tmp_path_factory):
    return _compile("chamfer.hip", str(tmp_path_factory.mktemp("chamfer_resources") / "chamfer.s"))


def test_no_kernel_of_chamfer_uses_scratch(chamfer_kernels):
    """Five instantiations <owned points per X cloud, X clouds per workgroup>; minima and coordinates live in registers."""
    assert len(chamfer_kernels) == 5, sorted(chamfer_kernels)
    assert all("chamfer_kernel" in k for k in chamfer_kernels), sorted(chamfer_kernels)
    spilling = {k: v["scratch"] for k, v in chamfer_kernels.items() if v["scratch"] != 0}
    assert not spilling, spilling


def test_chamfer_kernels_fit_a_256_thread_workgroup(chamfer_kernels):
    """One wave per SIMD needs no more than the 512 registers of a lane; the kernels are meant to run 4 and more waves per SIMD (128
    registers).  LDS: two tiles of 512 rows x 12 bytes and two sets of per-wave partial sums (4 waves x X clouds per workgroup)."""
    clouds_per_workgroup = {"Li1ELi8E": 8, "Li2ELi4E": 4, "Li4ELi2E": 2, "Li8ELi1E": 1, "Li16ELi1E": 1}
    seen = set()
    for k, v in chamfer_kernels.items():
        tag = [t for t in clouds_per_workgroup if f"chamfer_kernelI{t}E" in k]
        assert len(tag) == 1, k
        seen.add(tag[0])
        assert v["vgpr"] <= 128, (k, v)
        assert v["lds"] == 2 * 512 * 12 + 2 * clouds_per_workgroup[tag[0]] * 4 * 4, (k, v)
    assert seen == set(clouds_per_workgroup)


def test_chamfer_source_is_compiled_without_contraction():
    from test_kernel_resources import _build_py
    assert "-ffp-contract=off" in _build_py().SOURCES["chamfer.hip"]
