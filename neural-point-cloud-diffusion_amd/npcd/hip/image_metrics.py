"""Image metrics of rendered views on their own kernel (csrc/ssim.hip): the structural similarity index (SSIM) of
every view and channel and the mean squared error of every view, in one fused pass.  The operator under npcd.eval.ssim and the ssim=
switch of npcd.eval.evaluate_pointnerf.

Float64 arithmetic on fp32 pixels, no float atomics: the same bits on every run, and a view's numbers do not depend on the other views
of the call.  Images are read through their strides, so [V, C, H, W] and the renderer's [V, H, W, C] need no copy.  This module imports
without a GPU (`ssim_window` is a host helper); only the launch needs one.  There is no CPU fallback: a non-GPU tensor or a dtype
other than fp32 raises RuntimeError.
"""
import ctypes
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import check, lib, ptr, require_gpu, stream_ptr

_OP = "image_metrics"
MIN_WINDOW, MAX_WINDOW = 3, 15


class ImageMetrics(NamedTuple):
    """float64 tensors on the GPU: mse [V], ssim [V] (mean over channels), ssim_channels [V, C], map [V, C, H - w + 1, W - w + 1] or None."""
    mse: torch.Tensor
    ssim: torch.Tensor
    ssim_channels: torch.Tensor
    map: Optional[torch.Tensor]


def tile() -> Tuple[int, int]:
    """(rows, columns) of valid positions that one workgroup covers."""
    rows, cols = ctypes.c_int(0), ctypes.c_int(0)
    check(lib().npcd_image_metrics_tile(ctypes.byref(rows), ctypes.byref(cols)), "npcd_image_metrics_tile")
    return rows.value, cols.value


def ssim_window(window: str = "uniform", win_size: int = 7, sigma: float = 1.5) -> Tuple[np.ndarray, float]:
    """-> (taps, n): the separable window as float64 taps that sum to 1, and the factor n on the variances and the covariance.

    "uniform": taps 1 / win_size and n = w^2 / (w^2 - 1), the sample covariance -- skimage.metrics.structural_similarity at its
    defaults (win_size 7).  "gaussian": taps proportional to exp(-(i - r)^2 / (2 sigma^2)) over r = int(3.5 sigma + 0.5) pixels
    either side, normalised in float64, and n = 1 -- the setting of Wang et al. (sigma 1.5: 11 taps); `win_size` is not used.  The
    window must be odd and lie in [3, 15]."""
    if window == "uniform":
        if isinstance(win_size, bool) or not isinstance(win_size, int):
            raise ValueError(f"{_OP}: win_size must be an integer; got {win_size!r}")
        w = win_size
        taps, n = np.full(max(w, 0), 1.0 / max(w, 1), dtype=np.float64), None
    elif window == "gaussian":
        sigma = float(sigma)
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"{_OP}: sigma must be positive and finite; got {sigma!r}")
        r = int(3.5 * sigma + 0.5)
        w = 2 * r + 1
        taps = np.exp(-((np.arange(w, dtype=np.float64) - r) ** 2) / (2.0 * sigma * sigma))
        taps, n = taps / taps.sum(), 1.0
    else:
        raise ValueError(f"{_OP}: window must be 'uniform' or 'gaussian'; got {window!r}")
    if w % 2 == 0 or not MIN_WINDOW <= w <= MAX_WINDOW:
        raise ValueError(f"{_OP}: the window must be odd and lie in [{MIN_WINDOW}, {MAX_WINDOW}]; got {w} taps")
    return taps, (w * w / (w * w - 1.0) if n is None else n)


_tables = {}


def _device_window(window, win_size, sigma, dev):
    """(taps on the device, w, n), uploaded once per window and device."""
    key = (window, win_size if window == "uniform" else None, float(sigma) if window == "gaussian" else None, str(dev))
    if key not in _tables:
        taps, n = ssim_window(window, win_size, sigma)
        _tables[key] = (torch.from_numpy(taps).to(dev), len(taps), n)
    return _tables[key]


def as_views(t: torch.Tensor, layout: str = "chw") -> torch.Tensor:
    """The images as a [V, C, H, W] view: leading dimensions flattened to V, "hwc" permuted.  No copy wherever the leading dimensions
    can be addressed by one stride (any single one; contiguous ones); only then a reshape copies."""
    lead = t.shape[:-3]
    if len(lead) != 1:
        try:
            t = t.view(-1, *t.shape[-3:])
        except RuntimeError:
            t = t.reshape(-1, *t.shape[-3:])
    return t.permute(0, 3, 1, 2) if layout == "hwc" else t


def _images(pred, target, layout):
    if layout not in ("chw", "hwc"):
        raise ValueError(f"{_OP}: layout must be 'chw' or 'hwc'; got {layout!r}")
    for name, t in (("pred", pred), ("target", target)):
        if not isinstance(t, torch.Tensor) or t.dim() < 3:
            shape = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)
            raise ValueError(f"{_OP}: {name} must be [..., {'C, H, W' if layout == 'chw' else 'H, W, C'}]; got {shape}")
    if pred.shape != target.shape:
        raise ValueError(f"{_OP}: pred and target must have one shape; got {tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.numel() == 0:
        raise ValueError(f"{_OP}: empty images {tuple(pred.shape)}")
    for name, t in (("pred", pred), ("target", target)):
        if t.dtype != torch.float32:
            raise RuntimeError(f"HIP image metrics support fp32 images; got {t.dtype} for {name}")
    return as_views(pred.detach(), layout), as_views(target.detach(), layout)


def image_metrics(pred: torch.Tensor, target: torch.Tensor, window: str = "uniform", win_size: int = 7, sigma: float = 1.5,
                  data_range: float = 1.0, layout: str = "chw", return_map: bool = False) -> ImageMetrics:
    """pred, target: fp32 images [..., C, H, W] (layout "chw") or [..., H, W, C] ("hwc") on the GPU, the same shape -> ImageMetrics.

    ssim_channels[v, c]: the mean over the (H - w + 1)(W - w + 1) valid window positions of
    S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2, with the
    window means, variances and covariance of `ssim_window(window, win_size, sigma)`; ssim[v]: its mean over the
    channels; mse[v]: the mean squared error over all pixels and channels, so psnr = 10 log10(data_range^2 / mse); map (with
    return_map): S itself.  Nothing is read back and strided inputs are not copied.  A non-finite pixel makes its view's mse and
    ssim NaN and leaves the other views as they are."""
    x, y = _images(pred, target, layout)
    data_range = float(data_range)
    if not (math.isfinite(data_range) and data_range > 0):
        raise ValueError(f"{_OP}: data_range must be positive and finite; got {data_range!r}")
    taps_host, _ = ssim_window(window, win_size, sigma)
    V, C, H, W = x.shape
    w = len(taps_host)
    if H < w or W < w:
        raise ValueError(f"{_OP}: images of {H} x {W} pixels are smaller than the window of {w}")
    if V * C * H * W >= 1 << 31:
        raise ValueError(f"{_OP}: {V} x {C} x {H} x {W} is 2^31 pixels or more; measure the views in batches")
    require_gpu(x, y)
    dev = x.device
    if y.device != dev:
        raise RuntimeError(f"{_OP}: pred is on {dev}, target on {y.device}")
    taps, w, n = _device_window(window, win_size, sigma, dev)
    L = lib()
    f64 = dict(dtype=torch.float64, device=dev)
    workspace = torch.empty(L.npcd_image_metrics_workspace_bytes(V, C, H, W, w) // 8, **f64)
    mse, channels = torch.empty(V, **f64), torch.empty((V, C), **f64)
    smap = torch.empty((V, C, H - w + 1, W - w + 1), **f64) if return_map else None
    with torch.cuda.device(dev):
        check(L.npcd_image_metrics(ptr(x), ptr(y), V, C, H, W, *x.stride(), *y.stride(), ptr(taps), w, n, data_range, ptr(workspace),
                                   ptr(mse), ptr(channels), ptr(smap), stream_ptr()), "npcd_image_metrics")
    return ImageMetrics(mse, channels.sum(dim=1) / C, channels, smap)          # a true division: three ones give 1 exactly
