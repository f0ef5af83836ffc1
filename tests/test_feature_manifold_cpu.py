"""The feature k-NN kernels (csrc/feature_manifold.hip, DESIGN.md 5.12: the radii and ball counts behind precision / recall and
density / coverage), everything that needs no GPU: the host restatements of the spec (`knn_reference`, `ball_counts_reference`)
against plain Python loops, so that tests/test_gpu_feature_manifold.py leans on something checked; the metric on the host against a
worked example; the wrappers' refusals; the host-side queries and refusals of the C entry points; header, exports and SIGNATURES; the
kernels' resources as the compiler reports them.

The worked example: reals {0, 1, 2, 3}, fakes {0.4, 10}, k = 1.  Every real's nearest other real is at squared distance 1, the two
fakes are 92.16 apart.  The fake 0.4 lies in the balls of the reals 0 (0.16 < 1) and 1 (0.36 < 1), the fake 10 in none: precision
1/2, density (2 + 0) / (1 x 2) = 1.  Every real is within 92.16 of the fake 0.4: recall 1.  The reals 0 and 1 have a fake inside
their own ball, 2 and 3 (2.56, 6.76) have not: coverage 1/2."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_kernel_resources import _build_py, _compile

NEW_SYMBOLS = ("npcd_feature_knn_max_k", "npcd_feature_rows_workspace_bytes", "npcd_feature_knn", "npcd_feature_ball_counts")
UNSUPPORTED, BAD_ARG = -2, -1
REALS, FAKES = np.array([[0.0], [1.0], [2.0], [3.0]]), np.array([[0.4], [10.0]])
WORKED = dict(precision=0.5, recall=1.0, density=1.0, coverage=0.5)


# ---- the host restatements against plain loops -------------------------------------------------------------------------------------------------
def loops_d2(a, b):
    return sum((float(p) - float(q)) ** 2 for p, q in zip(a, b))


def test_the_references_agree_with_plain_loops():
    from npcd.hip.feature_manifold import ball_counts_reference, knn_reference
    g = np.random.RandomState(0)
    x, y = g.randint(-2, 3, (7, 3)).astype(np.float64), g.randint(-2, 3, (5, 3)).astype(np.float64)
    x[4] = x[1]                                                    # a duplicate row: its 0 stays in the list of the other
    for k in (1, 3, 4):
        want_cross = [sorted(loops_d2(a, b) for b in y)[:k] for a in x]
        want_self = [sorted(loops_d2(a, b) for l, b in enumerate(x) if l != i)[:k] for i, a in enumerate(x)]
        np.testing.assert_array_equal(knn_reference(x, y, k), np.array(want_cross))
        np.testing.assert_array_equal(knn_reference(x, None, k), np.array(want_self))
    assert knn_reference(x, None, 2)[1, 0] == 0.0 and knn_reference(x, None, 2)[4, 0] == 0.0
    assert knn_reference(x, None, 1)[0, 0] > 0.0                   # the index is left out, not the value 0
    rho = knn_reference(y, None, 2)[:, 1]
    cnt, near = ball_counts_reference(x, y, rho)
    assert cnt.dtype == np.int32 and near.dtype == np.float64
    np.testing.assert_array_equal(cnt, [sum(loops_d2(a, b) < rho[j] for j, b in enumerate(y)) for a in x])
    np.testing.assert_array_equal(near, [min(loops_d2(a, b) for b in y) for a in x])
    # strict: a distance equal to the radius is outside
    cnt, near = ball_counts_reference(np.array([[1.0]]), np.array([[0.0], [3.0]]), np.array([1.0, 4.0 + 1e-9]))
    assert cnt.tolist() == [1] and near.tolist() == [1.0]


# ---- the metric on the host ---------------------------------------------------------------------------------------------------------------------
def test_the_worked_example_on_the_host():
    from npcd.utils.fidkid import precision_recall_density_coverage
    assert precision_recall_density_coverage(REALS, FAKES, nearest_k=1) == WORKED
    assert precision_recall_density_coverage(REALS, FAKES, nearest_k=1, block_rows=3) == WORKED          # row blocks change nothing
    same = precision_recall_density_coverage(REALS, REALS, nearest_k=2)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0
    far = precision_recall_density_coverage(REALS, REALS + 100.0, nearest_k=2)
    assert far == dict(precision=0.0, recall=0.0, density=0.0, coverage=0.0)
    for k in (0, 2, True, 1.0):          # 2: the two fakes have one neighbour each
        with pytest.raises(ValueError, match="nearest_k"):
            precision_recall_density_coverage(REALS, FAKES, nearest_k=k)


def worked_metric(tmp_path, **kwargs):
    """FIDKID over the worked example with a zero second feature (distances unchanged; the Frechet distance wants D >= 2): the four
    reals come from a statistics pickle, the two fakes are fed."""
    from npcd.utils.fidkid import FIDKID
    reals, fakes = np.concatenate([REALS, 0 * REALS], 1), np.concatenate([FAKES, 0 * FAKES], 1)
    path = str(tmp_path / "reals.pkl")
    with open(path, "wb") as f:
        pickle.dump(dict(mean=reals.mean(0), cov=np.cov(reals, rowvar=False), feats_np=reals), f)
    m = FIDKID(num_images=2, num_subsets=2, inception_pkl=path, **kwargs)
    m.prepare()
    assert m.feed(torch.from_numpy(fakes), "fakes") == 2
    return m


def test_fidkid_reports_the_worked_example_with_prdc(tmp_path):
    m = worked_metric(tmp_path, prdc=True, nearest_k=1)
    out = m.summary()
    assert len(out) == 4
    assert set(m._result_dict) == {"fid", "fid_mean", "fid_cov", "kid", "precision", "recall", "density", "coverage"}
    assert {k: m._result_dict[k] for k in WORKED} == WORKED
    assert (m._result_dict["fid"], m._result_dict["kid"]) == (out[0], out[3])
    plain = worked_metric(tmp_path)
    plain.summary()
    assert m._result_str.startswith(plain._result_str.rsplit(",", 1)[0]) and m._result_str.endswith(", P/R 0.5000/1.0000, D/C 1.0000/0.5000")
    # two evenly strided rows a side, the reals {0, 2} (rows int(i 4 / 2)): rho_R = 4; the fake 0.4 is in both balls (0.16, 2.56), the
    # fake 10 in none, every real is within 92.16 of 0.4 and has it inside its own ball
    m = worked_metric(tmp_path, prdc=True, nearest_k=1, prdc_rows=2)
    m.summary()
    assert {k: m._result_dict[k] for k in WORKED} == dict(precision=0.5, recall=1.0, density=1.0, coverage=1.0)
    with pytest.raises(ValueError, match="prdc_rows"):
        worked_metric(tmp_path, prdc=True, nearest_k=1, prdc_rows=3).summary()          # more than the two fakes


def test_without_prdc_the_result_is_todays(tmp_path):
    m = worked_metric(tmp_path)
    m.summary()
    assert set(m._result_dict) == {"fid", "fid_mean", "fid_cov", "kid"}
    assert re.fullmatch(r"-?[\d.]+ \(-?[\d.]+/-?[\d.]+\), -?[\d.]+", m._result_str), m._result_str


def test_the_new_keywords_come_after_the_pinned_ones():
    import inspect
    from npcd.utils.fidkid import FIDKID, DeviceFIDKID
    for cls in (FIDKID, DeviceFIDKID):
        p = inspect.signature(cls.__init__).parameters
        assert [p[k].default for k in ("prdc", "nearest_k", "prdc_rows")] == [False, 5, None]
    names = list(inspect.signature(DeviceFIDKID.__init__).parameters)
    assert names.index("prdc") > names.index("rng") and names[9:12] == ["prdc", "nearest_k", "prdc_rows"]


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse():
    from npcd.hip.feature_manifold import ball_counts, knn_sq_distances, max_k
    assert max_k() >= 8
    x, y = torch.rand(9, 6), torch.rand(4, 6)
    for k in (0, -1, max_k() + 1, 2.0, True):
        with pytest.raises(ValueError, match="knn_sq_distances.*k must be"):
            knn_sq_distances(x, y, k=k)
    with pytest.raises(ValueError, match="knn_sq_distances.*at least 5 rows of the set itself"):
        knn_sq_distances(y, None, k=4)                 # m - 1 < k
    with pytest.raises(ValueError, match="knn_sq_distances.*at least 5 rows of y"):
        knn_sq_distances(x, y, k=5)
    with pytest.raises(RuntimeError, match="fp32 and fp64"):
        knn_sq_distances(x.half(), None, k=3)
    with pytest.raises(RuntimeError, match="fp32 and fp64"):
        ball_counts(x, y.bfloat16(), torch.rand(4).double())
    with pytest.raises(RuntimeError, match="float64"):
        knn_sq_distances(x, y.double(), k=3)
    with pytest.raises(RuntimeError, match="GPU"):
        knn_sq_distances(x, None, k=5)
    with pytest.raises(RuntimeError, match="GPU"):
        knn_sq_distances(x.double(), y.double(), k=4)  # m == k is supported
    with pytest.raises(RuntimeError, match="GPU"):
        ball_counts(x, y, torch.rand(4).double())
    with pytest.raises(ValueError, match="knn_sq_distances.*expected D = 6"):
        knn_sq_distances(x, y[:, :5], k=1)
    with pytest.raises(ValueError, match=r"knn_sq_distances.*\[n, D\]"):
        knn_sq_distances(x[0], None, k=1)
    with pytest.raises(ValueError, match="knn_sq_distances.*splits"):
        knn_sq_distances(x, y, k=1, splits=-1)
    with pytest.raises(ValueError, match="ball_counts.*splits"):
        ball_counts(x, y, torch.rand(4).double(), splits=1.5)
    with pytest.raises(ValueError, match=r"ball_counts.*rho_y must be \[4\]"):
        ball_counts(x, y, torch.rand(9).double())
    with pytest.raises(ValueError, match="knn_sq_distances.*D = 5000"):
        knn_sq_distances(torch.rand(3, 5000), None, k=1)


def test_device_fidkid_refuses_without_a_gpu_before_any_launch():
    from npcd.utils.fidkid import DeviceFIDKID
    m = DeviceFIDKID(num_images=4, device="cuda", prdc=True, nearest_k=2, prdc_rows=3)
    assert (m.prdc, m.nearest_k, m.prdc_rows) == (True, 2, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        m.feed(torch.zeros(2, 8), "fakes")
    with pytest.raises(RuntimeError, match="GPU"):
        m._prdc_on_device(torch.rand(6, 4), torch.rand(6, 4))
    with pytest.raises(ValueError, match="nearest_k"):
        m._prdc_on_device(torch.rand(2, 4), torch.rand(6, 4))


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------
def test_host_side_queries_and_refusals():
    from npcd import hip
    L = hip.lib()
    null = ctypes.c_void_p(0)
    top = L.npcd_feature_knn_max_k()
    assert top >= 8

    def knn(n=9, m=9, D=16, k=3, exclude=0, splits=0, dtype=hip.NPCD_F32):
        return L.npcd_feature_knn(null, null, dtype, n, m, D, max(D, 1), max(D, 1), exclude, k, splits, null, null, null)

    def counts(n=9, m=9, D=16, splits=0, dtype=hip.NPCD_F32):
        return L.npcd_feature_ball_counts(null, null, dtype, n, m, D, max(D, 1), max(D, 1), null, splits, null, null, null, null)

    # refused before any pointer is looked at and before any launch: null pointers, no GPU
    for D in (0, -1, 4097, 1 << 30):
        assert knn(D=D) == UNSUPPORTED and counts(D=D) == UNSUPPORTED, D
    for dtype in (hip.NPCD_BF16, hip.NPCD_F16, 4, -1):
        assert knn(dtype=dtype) == UNSUPPORTED and counts(dtype=dtype) == UNSUPPORTED, dtype
    for k in (0, -1, top + 1, 1 << 20):
        assert knn(m=1 << 21, k=k) == UNSUPPORTED, k
    for k in (-1, top + 1):
        assert L.npcd_feature_rows_workspace_bytes(9, 9, k, 0) == UNSUPPORTED, k
    assert knn(m=3, k=4) == UNSUPPORTED and knn(n=4, m=4, k=4, exclude=1) == UNSUPPORTED and knn(n=1, m=1, k=1, exclude=1) == UNSUPPORTED
    assert knn(exclude=2) == UNSUPPORTED and knn(exclude=-1) == UNSUPPORTED
    for n, m in ((0, 9), (9, 0), (-3, 9), (9, -3), ((1 << 24) + 1, 9), (9, (1 << 24) + 1)):
        assert knn(n=n, m=m) == UNSUPPORTED and counts(n=n, m=m) == UNSUPPORTED, (n, m)
        assert L.npcd_feature_rows_workspace_bytes(n, m, 3, 0) == UNSUPPORTED and L.npcd_feature_rows_workspace_bytes(n, m, 0, 0) == UNSUPPORTED
    assert knn(splits=-1) == UNSUPPORTED and counts(splits=-1) == UNSUPPORTED and L.npcd_feature_rows_workspace_bytes(9, 9, 3, -1) == UNSUPPORTED
    # supported, no buffers
    for D in (1, 17, 2048, 4096):
        for dtype in (hip.NPCD_F32, hip.NPCD_F64):
            assert knn(D=D, dtype=dtype) == BAD_ARG and counts(D=D, dtype=dtype) == BAD_ARG, (D, dtype)
    for n, m, k, exclude in ((2, 2, 1, 1), (9, 9, 8, 1), (5, 3, 3, 0), (1, 1, 1, 0), (3, 259, 2, 0), (1 << 24, 1 << 24, top, 1)):
        assert knn(n=n, m=m, k=k, exclude=exclude) == BAD_ARG and counts(n=n, m=m) == BAD_ARG, (n, m, k)
    for splits in (1, 2, 300):
        assert knn(splits=splits) == BAD_ARG and counts(splits=splits) == BAD_ARG


def test_workspace_bytes_match_their_formula():
    """8 (n + m) for the norms; with S > 1 splits in effect 8 S n k for the partial lists, 16 S n for the partial counts and minima.
    S = min(splits, tiles of y, 256); splits = 0 asks for ceil(8192 / row blocks)."""
    from npcd import hip
    L = hip.lib()
    tile = 64
    for n, m in ((2, 2), (70, 65), (3, 4 * tile + 3), (70, 5 * tile + 3), (16064, 16064), (50000, 50000), (100, 1 << 20), (1 << 20, 100)):
        tiles, blocks = -(-m // tile), -(-n // tile)
        for splits in (0, 1, 2, 3, 7, 1000):
            S = min(splits if splits else -(-8192 // blocks), tiles, 256)
            for k in (0, 1, 5, 8):
                want = 8 * (n + m + (S * n * (k if k else 2) if S > 1 else 0))
                assert L.npcd_feature_rows_workspace_bytes(n, m, k, splits) == want, (n, m, k, splits)


def test_header_exports_and_signatures_agree_for_the_new_names():
    from npcd import hip
    header = open(os.path.join(ROOT, "include", "npcd_hip.h")).read()
    declared = set(re.findall(r"\b(npcd_feature_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NEW_SYMBOLS)
    L = hip.lib()
    for name in NEW_SYMBOLS:
        assert name in hip.SIGNATURES and hasattr(L, name), name
        assert not name.startswith(("npcd_moments_", "npcd_kid_"))
    assert {n for n in hip.SIGNATURES if n.startswith("npcd_feature_")} == set(NEW_SYMBOLS)
    assert hip.SIGNATURES["npcd_feature_rows_workspace_bytes"][0] is ctypes.c_int64
    assert len(hip.SIGNATURES["npcd_feature_knn"][1]) == 14 and len(hip.SIGNATURES["npcd_feature_ball_counts"][1]) == 14
    assert L.npcd_missing == ()
    assert L.npcd_abi_version() == 10


# ---- the kernels' resources ----------------------------------------------------------------------------------------------------------------------
def test_feature_manifold_kernels_use_no_scratch(tmp_path):
    """The tiles kernel in its four forms (two dtypes x lists / counts), the norms in two, the two finish kernels; no scratch; static
    LDS of at most 64 KB; the matrix instruction is the float64 one."""
    out = str(tmp_path / "feature_manifold.s")
    kernels = _compile("feature_manifold.hip", out)
    for name, forms in (("feature_rows_kernel", 4), ("feature_norms_kernel", 2), ("knn_finish_kernel", 1), ("ball_finish_kernel", 1)):
        assert sum(name in k for k in kernels) == forms, (name, sorted(kernels))
    assert len(kernels) == 8
    for k, v in kernels.items():
        print(f"{k}: {v['vgpr']} VGPRs, {v['lds']} bytes of LDS, {v['scratch']} bytes of scratch")
        assert v["scratch"] == 0 and v["lds"] <= 65536, (k, v)
    text = open(out).read()
    assert text.count("v_mfma_f64_16x16x4_f64") >= 4 * 4 and "v_mfma_f32" not in text


def test_feature_manifold_source_is_compiled_without_contraction():
    assert "-ffp-contract=off" in _build_py().SOURCES["feature_manifold.hip"]
