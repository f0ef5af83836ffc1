"""Feature k-NN of the diffusion evaluation on its own kernels (csrc/feature_manifold.hip): the k smallest squared
distances of every row of one feature set to another, and the ball counts and nearest distances behind improved precision / recall
(Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020).  The operators under
npcd.utils.fidkid.DeviceFIDKID(prdc=True).

Float64 arithmetic on the float64 matrix instruction, on fp32 or fp64 features; the distance matrix is streamed in tiles and never
stored; no atomics: the same bits on every run and for every `splits`.  Nothing is read back.  This module imports without a GPU
(`knn_reference` and `ball_counts_reference` are host restatements of the spec in numpy); only the launches need one.  There is no
CPU fallback: a non-GPU tensor or a dtype other than fp32 / fp64 raises RuntimeError.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from . import check, lib, ptr, require_gpu, stream_ptr
from .feature_stats import _DTYPES, _check_D, _unit_columns


def max_k() -> int:
    """The largest k of `knn_sq_distances`."""
    return lib().npcd_feature_knn_max_k()


# ---- the spec, restated on the host ---------------------------------------------------------------------------------------------------------
def _sq_distances(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """d2 [n, m] as the sum over the features of the squared differences, float64, added in the order of the features: exact on small
    integers."""
    d2 = np.zeros((x.shape[0], y.shape[0]))
    for c in range(x.shape[1]):
        diff = x[:, c, None] - y[None, :, c]
        d2 += diff * diff
    return d2


def knn_reference(x: np.ndarray, y: Optional[np.ndarray] = None, k: int = 5) -> np.ndarray:
    """-> float64 [n, k]: per row of x the k smallest squared distances to the rows of y, ascending, equal values kept.  y=None: to
    the other rows of x, row i itself left out by its index (a duplicate of it elsewhere contributes its 0)."""
    x = np.asarray(x, dtype=np.float64)
    d2 = _sq_distances(x, x if y is None else np.asarray(y, dtype=np.float64))
    if y is None:
        d2[np.arange(len(x)), np.arange(len(x))] = np.inf
    return np.sort(d2, axis=1)[:, :k]


def ball_counts_reference(x: np.ndarray, y: np.ndarray, rho_y: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """-> (cnt int32 [n], near float64 [n]): cnt[i] = #{j : d2(x_i, y_j) < rho_y[j]} (strict), near[i] = min_j d2(x_i, y_j)."""
    d2 = _sq_distances(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    return (d2 < np.asarray(rho_y, dtype=np.float64)[None, :]).sum(1).astype(np.int32), d2.min(1)


# ---- the launches --------------------------------------------------------------------------------------------------------------------------
def _features(op, name, t, D=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{op}: {name} must be features [n, D]; got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if D is not None and t.shape[1] != D:
        raise ValueError(f"{op}: {name} has {t.shape[1]} features, expected D = {D}")
    if t.dtype not in _DTYPES:
        raise RuntimeError(f"HIP feature k-NN supports fp32 and fp64 features; got {t.dtype} for {name}")
    if t.shape[0] < 1:
        raise ValueError(f"{op}: {name} has no rows")
    return t.detach()


def _check_splits(op, splits):
    if isinstance(splits, bool) or not isinstance(splits, int) or splits < 0:
        raise ValueError(f"{op}: splits must be a non-negative integer (0: chosen from n and m); got {splits!r}")


def _pair(op, x, y):
    """Validated (x, y) on one device in one dtype, rows addressed by one stride."""
    if x.dtype != y.dtype:
        raise RuntimeError(f"{op}: x is {x.dtype}, y {y.dtype}")
    require_gpu(x, y)
    if y.device != x.device:
        raise RuntimeError(f"{op}: x is on {x.device}, y on {y.device}")
    return _unit_columns(x), _unit_columns(y)


def _workspace(op, n, m, k, splits, dev):
    size = lib().npcd_feature_rows_workspace_bytes(n, m, k, splits)
    if size < 0:
        raise ValueError(f"{op}: n = {n} rows against m = {m} are more than one launch takes")
    return torch.empty(size // 8, dtype=torch.float64, device=dev)


def knn_sq_distances(x: torch.Tensor, y: Optional[torch.Tensor] = None, k: int = 5, splits: int = 0) -> torch.Tensor:
    """x [n, D], y [m, D]: features on the GPU, one dtype -> float64 [n, k] on the device: per row of x the k smallest squared
    distances to the rows of y, ascending, equal values kept (`knn_reference`).  y=None: the set against itself, with row i itself
    left out by its index.  `splits`: workgroups per 64 rows of x (0: chosen from n and m); the result does not depend on it."""
    op = "knn_sq_distances"
    x = _features(op, "x", x)
    other = x if y is None else _features(op, "y", y, x.shape[1])
    _check_D(op, x.shape[1])
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > max_k():
        raise ValueError(f"{op}: k must be an integer in [1, {max_k()}]; got {k!r}")
    _check_splits(op, splits)
    n, m, exclude = x.shape[0], other.shape[0], int(y is None)
    if m - exclude < k:
        raise ValueError(f"{op}: k = {k} neighbours need at least {k + exclude} rows{' of the set itself' if exclude else ' of y'}; got {m}")
    x, other = _pair(op, x, other)
    D, dev = x.shape[1], x.device
    workspace = _workspace(op, n, m, k, splits, dev)
    out = torch.empty((n, k), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().npcd_feature_knn(ptr(x), ptr(other), _DTYPES[x.dtype], n, m, D, max(x.stride(0), D), max(other.stride(0), D), exclude, k,
                                     splits, ptr(workspace), ptr(out), stream_ptr()), "npcd_feature_knn")
    return out


def ball_counts(x: torch.Tensor, y: torch.Tensor, rho_y: torch.Tensor, splits: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [n, D], y [m, D]: features on the GPU, one dtype; rho_y [m]: squared radii of the rows of y -> (cnt int32 [n], near float64
    [n]) on the device: cnt[i] = #{j : d2(x_i, y_j) < rho_y[j]} (strict), near[i] = min_j d2(x_i, y_j) (`ball_counts_reference`)."""
    op = "ball_counts"
    x = _features(op, "x", x)
    y = _features(op, "y", y, x.shape[1])
    _check_D(op, x.shape[1])
    _check_splits(op, splits)
    n, m = x.shape[0], y.shape[0]
    if not isinstance(rho_y, torch.Tensor) or rho_y.shape != (m,):
        raise ValueError(f"{op}: rho_y must be [{m}], one squared radius per row of y; got "
                         f"{tuple(rho_y.shape) if isinstance(rho_y, torch.Tensor) else type(rho_y)}")
    x, y = _pair(op, x, y)
    require_gpu(rho_y)
    D, dev = x.shape[1], x.device
    rho_y = rho_y.detach().to(device=dev, dtype=torch.float64).contiguous()
    workspace = _workspace(op, n, m, 0, splits, dev)
    cnt, near = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib().npcd_feature_ball_counts(ptr(x), ptr(y), _DTYPES[x.dtype], n, m, D, max(x.stride(0), D), max(y.stride(0), D), ptr(rho_y),
                                             splits, ptr(workspace), ptr(cnt), ptr(near), stream_ptr()), "npcd_feature_ball_counts")
    return cnt, near
