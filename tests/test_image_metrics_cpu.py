"""The image-metrics kernel (SSIM and the mean squared error of rendered views), everything that needs no GPU: the float64 oracle written
from the definition of DESIGN.md 5.10, cross-checked against a second formulation on scipy's filters; the render-like images that
tests/test_gpu_image_metrics.py uses, with their preconditions asserted; the window helper; the wrapper's refusals; the host-side
queries and refusals of the C entry points; header, exports and SIGNATURES; the kernels' resources as the compiler reports them.

The oracle takes the five window means as explicit sliding-window sums with weights t[i] t[j] over the valid positions, in float64 on
the fp32 pixels, and evaluates S exactly as the definition writes it."""
import ctypes
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

from conftest import ROOT
from test_kernel_resources import _compile

NEW_SYMBOLS = ("npcd_image_metrics", "npcd_image_metrics_workspace_bytes", "npcd_image_metrics_tile")
WINDOWS = ("uniform", "gaussian")
SIGMAS = (0.0, 0.01, 0.1)          # noise on the object, one prediction each


# ---- oracle, from the definition of DESIGN.md 5.10 -------------------------------------------------------------------------------------
def window_oracle(window, win_size=7, sigma=1.5):
    """-> (taps float64 summing to 1, n)."""
    if window == "uniform":
        w = win_size
        return np.full(w, 1.0 / w, dtype=np.float64), w * w / (w * w - 1.0)
    r = int(3.5 * sigma + 0.5)
    t = np.exp(-((np.arange(2 * r + 1, dtype=np.float64) - r) ** 2) / (2.0 * sigma * sigma))
    return t / t.sum(), 1.0


def moments_oracle(x, y, taps):
    """x, y [H, W] float64 -> ux, uy, uxx, uyy, uxy at the valid positions [H - w + 1, W - w + 1]."""
    w = len(taps)
    weights = np.outer(taps, taps)

    def mean(a):
        return (sliding_window_view(a, (w, w)) * weights).sum(axis=(-2, -1))
    return mean(x), mean(y), mean(x * x), mean(y * y), mean(x * y)


def s_of(ux, uy, uxx, uyy, uxy, n, data_range=1.0):
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
    return ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2)), vx + vy


def image_metrics_oracle(pred, target, window="uniform", win_size=7, sigma=1.5, data_range=1.0):
    """pred, target [V, C, H, W] fp32 -> map [V, C, H - w + 1, W - w + 1], channels [V, C], ssim [V], mse [V], and `spread`, vx + vy
    at every valid position; all float64."""
    assert pred.dtype == target.dtype == np.float32 and pred.shape == target.shape and pred.ndim == 4
    taps, n = window_oracle(window, win_size, sigma)
    x, y = pred.astype(np.float64), target.astype(np.float64)
    V, C, H, W = x.shape
    w = len(taps)
    smap, spread = (np.empty((V, C, H - w + 1, W - w + 1)) for _ in range(2))
    for v in range(V):
        for c in range(C):
            smap[v, c], spread[v, c] = s_of(*moments_oracle(x[v, c], y[v, c], taps), n, data_range)
    channels = smap.mean(axis=(2, 3))
    return SimpleNamespace(map=smap, channels=channels, ssim=channels.mean(axis=1), mse=((x - y) ** 2).mean(axis=(1, 2, 3)), spread=spread)


def filtered_s(x, y, window, data_range=1.0):
    """The second formulation: the same S from scipy's filters over the whole image, cropped by (w - 1) / 2."""
    from scipy import ndimage
    if window == "uniform":
        blur, w, n = functools.partial(ndimage.uniform_filter, size=7), 7, 49.0 / 48.0
    else:
        blur, w, n = functools.partial(ndimage.gaussian_filter, sigma=1.5, truncate=3.5), 11, 1.0
    p = (w - 1) // 2
    return s_of(*(blur(a)[p:-p, p:-p] for a in (x, y, x * x, y * y, x * y)), n, data_range)[0]


# ---- the images of the GPU tests ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def render_like(V, C, H, W, seed=0):
    """-> (target [V, C, H, W] fp32, {sigma: prediction}).  A white background (exactly 1), an elliptical object that carries a smooth
    pattern plus noise clipped to [0, 1] -- wide bands of it saturate at exactly 0 and at exactly 1 -- and predictions equal to the
    target plus noise of `sigma` on the object only (not clipped)."""
    rng = np.random.default_rng(1000 * H + 10 * W + V + seed)
    i, j = np.mgrid[0:H, 0:W].astype(np.float64)
    target = np.ones((V, C, H, W), dtype=np.float64)
    inside = np.zeros((V, H, W), dtype=bool)
    for v in range(V):
        ci, cj = H / 2 + 0.02 * H * np.sin(1.3 * v), W / 2 + 0.02 * W * np.cos(2.1 * v)
        inside[v] = ((i - ci) / (0.37 * H)) ** 2 + ((j - cj) / (0.41 * W)) ** 2 <= 1.0
        for c in range(C):
            # the phase puts the middle of channel 0's zero band on the object's centre; the period is 40 pixels across
            phase = 2.0 * np.pi * ((j - cj) / 40.0 + (i - ci) / 160.0) + 1.5 * np.pi + 2.0 * np.pi * c / 3.0
            pattern = np.clip(0.5 + 1.2 * np.sin(phase) + rng.normal(0.0, 0.02, (H, W)), 0.0, 1.0)
            target[v, c][inside[v]] = pattern[inside[v]]
    target = target.astype(np.float32)
    preds = {}
    for sigma in SIGMAS:
        noise = rng.normal(0.0, sigma, target.shape) * inside[:, None] if sigma else 0.0
        preds[sigma] = (target.astype(np.float64) + noise).astype(np.float32)
    return target, preds


SHAPES = [(2, 3, 37, 45), (5, 3, 128, 128)]          # the small set, and the workload's own view size


@functools.lru_cache(maxsize=None)
def oracle_case(shape, sigma, window):
    """The oracle on render_like(*shape) at one noise level, computed once for both test files."""
    target, preds = render_like(*shape)
    return image_metrics_oracle(preds[sigma], target, window)


# ---- the oracle against the second formulation, and the preconditions of the GPU tests -----------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
def test_the_oracle_agrees_with_the_filter_formulation(window):
    shape = SHAPES[0]
    target, preds = render_like(*shape)
    worst = 0.0
    for sigma in SIGMAS:
        want = oracle_case(shape, sigma, window)
        for v in range(shape[0]):
            for c in range(shape[1]):
                other = filtered_s(preds[sigma][v, c].astype(np.float64), target[v, c].astype(np.float64), window)
                assert other.shape == want.map[v, c].shape
                worst = max(worst, float(np.abs(other - want.map[v, c]).max()))
    print(f"{window}: the two formulations differ by at most {worst:.3g} per pixel")
    assert worst <= 1e-10


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_the_images_meet_their_preconditions(shape, window):
    """What the GPU tests rely on: some window without any variance (vx + vy == 0, so C2 alone is the denominator's second factor),
    some S below 0.6, and the pair without noise at exactly 1 with mse == 0."""
    target, preds = render_like(*shape)
    assert target.dtype == np.float32 and (target == 1.0).any() and target.min() == 0.0 and target.max() == 1.0
    cases = [oracle_case(shape, sigma, window) for sigma in SIGMAS]
    clean = cases[0]
    assert (clean.map == 1.0).all() and (clean.channels == 1.0).all() and (clean.ssim == 1.0).all() and (clean.mse == 0.0).all()
    assert any((c.spread == 0.0).any() for c in cases)
    assert min(float(c.map.min()) for c in cases) < 0.6
    for sigma, c in zip(SIGMAS, cases):
        print(f"{shape} {window} sigma {sigma}: ssim {c.ssim.min():.4f} .. {c.ssim.max():.4f}, least S {c.map.min():.3f}, "
              f"{int((c.spread == 0.0).sum())} windows without variance, mse {c.mse.max():.3g}")
    assert (cases[2].ssim < cases[1].ssim).all() and (cases[1].ssim < 1.0).all() and (cases[2].mse > cases[1].mse).all()


# ---- the window helper ------------------------------------------------------------------------------------------------------------------------
def test_ssim_window_equals_the_oracle():
    from npcd.hip.image_metrics import ssim_window
    for args in (("uniform",), ("uniform", 3), ("uniform", 15), ("gaussian",), ("gaussian", 7, 0.8), ("gaussian", 7, 2.0)):
        taps, n = ssim_window(*args)
        want, want_n = window_oracle(*args)
        assert taps.dtype == np.float64 and n == want_n
        np.testing.assert_array_equal(taps, want)
        assert abs(taps.sum() - 1.0) <= 4e-16
    assert ssim_window()[1] == 49.0 / 48.0 and len(ssim_window()[0]) == 7
    taps, n = ssim_window("gaussian")
    assert n == 1.0 and len(taps) == 11 and taps.argmax() == 5
    np.testing.assert_array_equal(taps, taps[::-1])
    for bad in (("box",), ("uniform", 8), ("uniform", 1), ("uniform", 17), ("uniform", 7.0), ("gaussian", 7, 0.0), ("gaussian", 7, 0.1),
                ("gaussian", 7, 2.5), ("gaussian", 7, float("nan"))):
        with pytest.raises(ValueError):
            ssim_window(*bad)


# ---- the wrapper -----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses():
    import npcd.eval
    from npcd.hip.image_metrics import image_metrics
    x = torch.zeros(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="GPU"):
        image_metrics(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        image_metrics(x.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1), window="gaussian", layout="hwc", return_map=True)
    with pytest.raises(RuntimeError, match="GPU"):
        npcd.eval.ssim(x, x)
    with pytest.raises(RuntimeError, match="fp32"):
        image_metrics(x.double(), x.double())
    with pytest.raises(RuntimeError, match="fp32"):
        image_metrics(x, x.half())
    with pytest.raises(ValueError, match="one shape"):
        image_metrics(x, x[:, :, :15])
    with pytest.raises(ValueError, match="must be"):
        image_metrics(x[0, 0], x[0, 0])
    with pytest.raises(ValueError, match="empty"):
        image_metrics(x[:0], x[:0])
    with pytest.raises(ValueError, match="smaller than the window"):
        image_metrics(x[..., :6], x[..., :6])
    with pytest.raises(ValueError, match="smaller than the window"):
        image_metrics(x[:, :, :10], x[:, :, :10], window="gaussian")
    with pytest.raises(ValueError, match="smaller than the window"):
        image_metrics(x, x, layout="hwc")          # read as 3 x 16 pixels of 16 channels
    with pytest.raises(ValueError, match="window"):
        image_metrics(x, x, window="box")
    with pytest.raises(ValueError, match="window"):
        image_metrics(x, x, win_size=8)
    with pytest.raises(ValueError, match="layout"):
        image_metrics(x, x, layout="cwh")
    for data_range in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            image_metrics(x, x, data_range=data_range)


def test_strided_images_are_viewed_and_never_copied():
    from npcd.hip.image_metrics import as_views
    channels = torch.arange(4 * 5 * 36 * 3, dtype=torch.float32).view(4, 5, 36, 3)[1:3, 2]          # [2, 36, 3] inside a larger tensor
    hwc = channels.unflatten(1, (6, 6))
    got = as_views(hwc, "hwc")
    assert got.shape == (2, 3, 6, 6) and got.data_ptr() == channels.data_ptr() and got.stride() == (5 * 36 * 3, 1, 18, 3)
    assert torch.equal(got, hwc.permute(0, 3, 1, 2))
    chw = torch.zeros(2, 4, 3, 8, 8)
    assert as_views(chw, "chw").shape == (8, 3, 8, 8) and as_views(chw, "chw").data_ptr() == chw.data_ptr()
    assert as_views(chw[0, 0], "chw").shape == (1, 3, 8, 8) and as_views(chw[:, 1], "chw").data_ptr() == chw[:, 1].data_ptr()
    assert as_views(chw[:, 1], "chw").stride(0) == 4 * 3 * 64


def test_eval_exports_the_new_names_without_a_gpu():
    import inspect
    import npcd.eval
    from npcd.hip import image_metrics as module
    assert npcd.eval.image_metrics is module.image_metrics and callable(npcd.eval.ssim)
    parameters = inspect.signature(npcd.eval.evaluate_pointnerf).parameters
    assert parameters["ssim"].default is False and parameters["ssim_window"].default == "uniform"
    assert list(inspect.signature(module.image_metrics).parameters) == ["pred", "target", "window", "win_size", "sigma", "data_range", "layout",
                                                                        "return_map"]


# ---- the C entry points ------------------------------------------------------------------------------------------------------------------------
def _launch(L, V, C, H, W, w, n=1.0, data_range=1.0):
    null = ctypes.c_void_p(0)
    return L.npcd_image_metrics(null, null, V, C, H, W, C * H * W, H * W, W, 1, C * H * W, H * W, W, 1, null, w, n, data_range, null, null, null,
                                null, null)


def test_host_side_queries_and_refusals():
    from npcd import hip
    L = hip.lib()
    rows, cols = ctypes.c_int(0), ctypes.c_int(0)
    assert L.npcd_image_metrics_tile(ctypes.byref(rows), ctypes.byref(cols)) == 0 and rows.value > 0 and cols.value > 0
    assert L.npcd_image_metrics_tile(None, ctypes.byref(cols)) == -1
    unsupported = -2
    # refused before any pointer is looked at and before any launch: null pointers, no GPU
    for V, C, H, W, w in ((0, 3, 16, 16, 7), (2, 0, 16, 16, 7), (2, 3, 0, 16, 7), (2, 3, 16, 0, 7), (-1, 3, 16, 16, 7), (2, -3, 16, 16, 7),
                          (2, 3, -16, 16, 7), (2, 3, 16, -16, 7), (2, 3, 6, 16, 7), (2, 3, 16, 6, 7), (2, 3, 10, 16, 11), (2, 3, 16, 16, 8),
                          (2, 3, 16, 16, 6), (2, 3, 16, 16, 1), (2, 3, 32, 32, 17), (2, 3, 16, 16, 0), (2, 3, 16, 16, -7),
                          (1 << 11, 4, 1 << 9, 1 << 9, 7), (1 << 16, 1 << 16, 1 << 16, 1 << 16, 7), (3, 1, 1 << 15, 1 << 15, 7)):
        assert _launch(L, V, C, H, W, w) == unsupported, (V, C, H, W, w)
        assert L.npcd_image_metrics_workspace_bytes(V, C, H, W, w) == unsupported, (V, C, H, W, w)
    for V, C, H, W, w in ((1, 1, 3, 3, 3), (1, 1, 15, 15, 15), (251, 3, 128, 128, 7), (251, 3, 128, 128, 11), ((1 << 11) - 1, 4, 1 << 9, 1 << 9, 7)):
        assert _launch(L, V, C, H, W, w) == -1, (V, C, H, W, w)          # supported, no buffers
        tiles = V * C * -(-(H - w + 1) // rows.value) * -(-(W - w + 1) // cols.value)
        assert L.npcd_image_metrics_workspace_bytes(V, C, H, W, w) == 16 * tiles


def test_header_exports_and_signatures_agree_for_the_new_names():
    from npcd import hip
    header = open(os.path.join(ROOT, "include", "npcd_hip.h")).read()
    declared = set(re.findall(r"\b(npcd_image_[a-z0-9_]+)\s*\(", header))
    assert declared == set(NEW_SYMBOLS)
    L = hip.lib()
    for name in NEW_SYMBOLS:
        assert name in hip.SIGNATURES and hasattr(L, name), name
    assert hip.SIGNATURES["npcd_image_metrics_workspace_bytes"][0] is ctypes.c_int64
    assert len(hip.SIGNATURES["npcd_image_metrics"][1]) == 23


# ---- the kernels' resources ----------------------------------------------------------------------------------------------------------------------
def test_image_metrics_kernels_use_no_scratch_and_fit_two_to_a_compute_unit(tmp_path):
    """Two kernels, the tiles and the fixed-order sum; no scratch; static LDS of at most 64 KB."""
    kernels = _compile("ssim.hip", str(tmp_path / "ssim.s"))
    assert len(kernels) == 2 and any("image_metrics_tile_kernel" in k for k in kernels) and any("image_metrics_finish_kernel" in k for k in kernels)
    for k, v in kernels.items():
        print(f"{k}: {v['vgpr']} VGPRs, {v['lds']} bytes of LDS, {v['scratch']} bytes of scratch")
        assert v["scratch"] == 0 and v["lds"] <= 65536, (k, v)


def test_image_metrics_source_is_compiled_without_contraction():
    from test_kernel_resources import _build_py
    assert "-ffp-contract=off" in _build_py().SOURCES["ssim.hip"]
