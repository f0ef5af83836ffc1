"""The feature-statistics kernels (csrc/feature_stats.hip, DESIGN.md 5.11: the moments behind FID and the subset sums behind KID),
everything that needs no GPU: the host restatements of the spec (`moments_reference`, `kid_sums_reference`) against np.cov and
oracle.fidkid.calc_kid, so that tests/test_gpu_feature_stats.py leans on something pinned to the oracle; the wrappers' refusals; the
host-side queries and refusals of the C entry points; header, exports and SIGNATURES; the kernels' resources as the compiler reports
them."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import fidkid as ofk
from test_kernel_resources import _compile

NEW_SYMBOLS = ("npcd_moments_tile", "npcd_moments_max_features", "npcd_moments_update", "npcd_moments_finish", "npcd_kid_tile",
               "npcd_kid_workspace_bytes", "npcd_kid_subsets")
UNSUPPORTED, BAD_ARG = -2, -1


def feats(n, d, seed, shift=0.0, scale=1.0):
    """Non-negative features, like Inception pool features: the absolute value of tests/test_fidkid_cpu.py's."""
    g = np.random.RandomState(seed)
    a = g.randn(d, d) / d ** 0.5
    return np.abs((g.randn(n, d) @ a) * scale + shift)


class ReplayedChoice:
    """Records what rng.choice returns, to hand the subsets of a calc_kid run to kid_sums_reference."""

    def __init__(self, seed):
        self.rng, self.drawn = np.random.RandomState(seed), []

    def choice(self, *args, **kwargs):
        self.drawn.append(self.rng.choice(*args, **kwargs))
        return self.drawn[-1]


# ---- the host restatements against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(2, 1), (70, 17), (600, 24)])
def test_moments_reference_agrees_with_numpy(n, d):
    from npcd.hip.feature_stats import moments_reference
    x = feats(n, d, 1, shift=0.4)
    want_mean, want_cov = x.mean(0), np.cov(x, rowvar=False).reshape(d, d)
    scale = np.abs(x).T @ np.abs(x) / (n - 1)
    for shift in (None, x[: max(n // 2, 1)].mean(0)):
        total, gram, mean, cov = moments_reference(x, shift)
        assert total.shape == (d,) and gram.shape == cov.shape == (d, d)
        assert np.abs(mean - want_mean).max() <= 1e-13 * np.abs(x).max()
        assert np.abs(cov - want_cov).max() <= 1e-12 * scale.max()
        np.testing.assert_array_equal(cov, cov.T)
    with np.errstate(all="ignore"):
        assert np.isnan(moments_reference(x[:1])[3]).all()


def test_kid_sums_reference_agrees_with_the_oracle():
    from npcd.hip.feature_stats import kid_from_sums, kid_sums_reference
    real, fake = feats(150, 16, 4), feats(120, 16, 5, shift=0.2)
    S, cap = 7, 50
    replay = ReplayedChoice(11)
    want = ofk.calc_kid(real, fake, S, cap, rng=replay)
    idx_f, idx_r = np.stack(replay.drawn[0::2]), np.stack(replay.drawn[1::2])          # per subset: the fakes first, then the reals
    assert idx_f.shape == idx_r.shape == (S, cap) and idx_f.max() < 120 <= idx_r.max()
    sums = kid_sums_reference(fake, real, idx_f, idx_r)
    assert sums.shape == (S, 3) and (sums > 0).all()
    assert kid_from_sums(sums, cap) == pytest.approx(want, rel=1e-10)
    # each sum on its own, against the reference's own expression for one subset
    x, y = fake[idx_f[0]], real[idx_r[0]]
    kxx, kyy, kxy = (x @ x.T / 16 + 1) ** 3, (y @ y.T / 16 + 1) ** 3, (x @ y.T / 16 + 1) ** 3
    for got, ref in zip(sums[0], (kxx.sum() - np.diag(kxx).sum(), kyy.sum() - np.diag(kyy).sum(), kxy.sum())):
        assert got == pytest.approx(ref, rel=1e-12)


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_refuse():
    from npcd.hip.feature_stats import FeatureMoments, kid_subsets, max_features
    x = torch.rand(8, 6)
    idx = np.arange(8)[None, :4]
    with pytest.raises(RuntimeError, match="GPU"):
        FeatureMoments(6, "cpu").add(x)
    with pytest.raises(RuntimeError, match="GPU"):
        FeatureMoments(6, "cuda").add(x)
    with pytest.raises(RuntimeError, match="GPU"):
        FeatureMoments(6, "cuda", keep_features=False).add(x.double())
    with pytest.raises(RuntimeError, match="GPU"):
        kid_subsets(x, x, idx, idx)
    with pytest.raises(RuntimeError, match="fp32 and fp64"):
        FeatureMoments(6, "cuda").add(x.half())
    with pytest.raises(RuntimeError, match="fp32 and fp64"):
        kid_subsets(x.half(), x.half(), idx, idx)
    with pytest.raises(RuntimeError, match="float64"):
        kid_subsets(x, x.double(), idx, idx)
    with pytest.raises(ValueError, match="FeatureMoments.*D = 6"):
        FeatureMoments(6, "cuda").add(x[:, :5])
    with pytest.raises(ValueError, match=r"FeatureMoments.*\[n, D\]"):
        FeatureMoments(6, "cuda").add(x[0])
    with pytest.raises(ValueError, match="FeatureMoments.*at least 2 rows"):
        FeatureMoments(6, "cuda").finalize()
    for D in (0, -1, 2.0, max_features() + 1):
        with pytest.raises(ValueError, match="FeatureMoments.*D"):
            FeatureMoments(D, "cuda")
    with pytest.raises(ValueError, match="FeatureMoments.*block_rows"):
        FeatureMoments(6, "cuda", block_rows=0)
    with pytest.raises(ValueError, match="FeatureMoments.*shift"):
        FeatureMoments(6, "cuda", shift=np.zeros(5))
    with pytest.raises(ValueError, match="FeatureMoments.*merge_"):
        FeatureMoments(6, "cuda").merge_(FeatureMoments(5, "cuda"))
    with pytest.raises(ValueError, match="FeatureMoments.*same shift"):
        FeatureMoments(6, "cuda", shift=np.zeros(6)).merge_(FeatureMoments(6, "cuda", shift=np.ones(6)))
    with pytest.raises(ValueError, match="kid_subsets.*m >= 2"):
        kid_subsets(x, x, idx[:, :1], idx[:, :1])
    with pytest.raises(ValueError, match="kid_subsets.*S >= 1"):
        kid_subsets(x, x, idx[:0], idx[:0])
    with pytest.raises(ValueError, match="kid_subsets.*idx_r is out of range"):
        kid_subsets(x, x[:3], idx, idx)
    with pytest.raises(ValueError, match="kid_subsets.*idx_f is out of range"):
        kid_subsets(x, x, idx - 1, idx)
    with pytest.raises(ValueError, match="kid_subsets.*one shape"):
        kid_subsets(x, x, idx, idx[:, :3])
    with pytest.raises(ValueError, match="kid_subsets.*integer"):
        kid_subsets(x, x, idx.astype(np.float64), idx)
    with pytest.raises(ValueError, match="kid_subsets.*expected D = 6"):
        kid_subsets(x, x[:, :5], idx, idx)


def test_device_fidkid_has_the_surface_of_fidkid_without_a_gpu():
    import inspect
    from npcd.utils.fidkid import FIDKID, DeviceFIDKID
    assert list(inspect.signature(DeviceFIDKID.__init__).parameters)[1:9] == ["num_images", "num_subsets", "max_subset_size", "inception_pkl",
                                                                              "feature_extractor", "device", "block_rows", "rng"]
    for name in ("prepare", "feed", "summary", "name"):
        assert hasattr(DeviceFIDKID, name) and hasattr(FIDKID, name)
    m = DeviceFIDKID(num_images=4, device="cuda")
    m.prepare()
    assert m._result_dict is None and m._result_str is None and m.num_fake_feeded == 0
    with pytest.raises(RuntimeError, match="feature_extractor"):
        m.feed(torch.zeros(2, 3, 8, 8), "fakes")
    with pytest.raises(ValueError):
        m.feed(torch.zeros(2, 8), "fake")
    with pytest.raises(RuntimeError, match="GPU"):
        m.feed(torch.zeros(2, 8), "fakes")


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------
def test_host_side_queries_and_refusals():
    from npcd import hip
    L = hip.lib()
    null = ctypes.c_void_p(0)
    tile, kid_tile = ctypes.c_int(0), ctypes.c_int(0)
    assert L.npcd_moments_tile(ctypes.byref(tile)) == 0 and tile.value >= 64 and tile.value % 16 == 0
    assert L.npcd_kid_tile(ctypes.byref(kid_tile)) == 0 and kid_tile.value >= 16 and kid_tile.value % 16 == 0
    assert L.npcd_moments_tile(None) == BAD_ARG and L.npcd_kid_tile(None) == BAD_ARG
    limit = L.npcd_moments_max_features()
    assert limit >= 2048

    def update(D, dtype=hip.NPCD_F32, r0=0, r1=8):
        return L.npcd_moments_update(null, dtype, max(D, 1), r0, r1, D, null, null, null, null)

    def finish(D, n=8):
        return L.npcd_moments_finish(null, null, null, D, n, null, null, null)

    def subsets(S, m, D=16, dtype=hip.NPCD_F32):
        return L.npcd_kid_subsets(null, null, dtype, 8, 8, D, max(D, 1), max(D, 1), null, null, S, m, null, null, null)

    # refused before any pointer is looked at and before any launch: null pointers, no GPU
    for D in (0, -1, limit + 1, 1 << 30):
        assert update(D) == UNSUPPORTED and finish(D) == UNSUPPORTED and subsets(2, 4, D) == UNSUPPORTED, D
    for dtype in (hip.NPCD_BF16, hip.NPCD_F16, 4, -1):
        assert update(16, dtype) == UNSUPPORTED and subsets(2, 4, 16, dtype) == UNSUPPORTED, dtype
    for n in (1, 0, -5):
        assert finish(16, n) == UNSUPPORTED
    for S, m in ((0, 4), (-1, 4), (2, 1), (2, 0), (2, -3), (1 << 23, 1000), (1, (1 << 20) + 1)):
        assert subsets(S, m) == UNSUPPORTED and L.npcd_kid_workspace_bytes(S, m) == UNSUPPORTED, (S, m)
    # supported, no buffers
    for D in (1, 17, 2048, limit):
        for dtype in (hip.NPCD_F32, hip.NPCD_F64):
            assert update(D, dtype) == BAD_ARG and subsets(2, 4, D, dtype) == BAD_ARG, (D, dtype)
        assert finish(D) == BAD_ARG and finish(D, 2) == BAD_ARG
    t = kid_tile.value
    for S, m in ((1, 2), (3, 70), (2, t), (2, t + 1), (2, 2 * t + 1), (100, 1000)):
        assert subsets(S, m) == BAD_ARG
        tiles = -(-m // t)
        assert L.npcd_kid_workspace_bytes(S, m) == 8 * S * (tiles * (tiles + 1) + tiles * tiles), (S, m)


def test_header_exports_and_signatures_agree_for_the_new_names():
    from npcd import hip
    header = open(os.path.join(ROOT, "include", "npcd_hip.h")).read()
    declared = set(re.findall(r"\b(npcd_(?:moments|kid)_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NEW_SYMBOLS)
    L = hip.lib()
    for name in NEW_SYMBOLS:
        assert name in hip.SIGNATURES and hasattr(L, name), name
    assert hip.SIGNATURES["npcd_kid_workspace_bytes"][0] is ctypes.c_int64
    assert len(hip.SIGNATURES["npcd_moments_update"][1]) == 10 and len(hip.SIGNATURES["npcd_moments_finish"][1]) == 8
    assert len(hip.SIGNATURES["npcd_kid_subsets"][1]) == 15
    assert re.search(r"#define NPCD_F64 3\b", header) and hip.NPCD_F64 == 3
    assert L.npcd_abi_version() == 10


# ---- the kernels' resources ----------------------------------------------------------------------------------------------------------------------
def test_feature_stats_kernels_use_no_scratch(tmp_path):
    """Four kernels, the two with a feature dtype in both forms; no scratch; static LDS of at most 64 KB; the matrix instruction is
    the float64 one."""
    out = str(tmp_path / "feature_stats.s")
    kernels = _compile("feature_stats.hip", out)
    for name, forms in (("moments_update_kernel", 2), ("moments_finish_kernel", 1), ("kid_tiles_kernel", 2), ("kid_finish_kernel", 1)):
        assert sum(name in k for k in kernels) == forms, (name, sorted(kernels))
    assert len(kernels) == 6
    for k, v in kernels.items():
        print(f"{k}: {v['vgpr']} VGPRs, {v['lds']} bytes of LDS, {v['scratch']} bytes of scratch")
        assert v["scratch"] == 0 and v["lds"] <= 65536, (k, v)
    text = open(out).read()
    assert text.count("v_mfma_f64_16x16x4_f64") >= 4 * 2 + 4 * 2 and "v_mfma_f32" not in text


def test_feature_stats_source_is_compiled_without_contraction():
    from test_kernel_resources import _build_py
    assert "-ffp-contract=off" in _build_py().SOURCES["feature_stats.hip"]
