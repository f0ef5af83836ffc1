"""Occupancy grid of point clouds on its own kernel (csrc/occupancy.hip): every point goes to the nearest valid cell of
an R^3 lattice, and two integer histograms are taken -- points per cell and clouds per cell.  The operator under the Jensen-Shannon
divergence and the occupancy entropy of npcd/eval/shapes.py, beside npcd/hip/chamfer.py and npcd/hip/emd.py.

One launch per call, integer atomics only: the same bits on every run.  This module imports without a GPU (`grid_lattice` and
`grid_mask` are host helpers); only the launch needs one.  There is no CPU fallback: a non-GPU tensor or a dtype other than fp32
raises RuntimeError.
"""
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import check, lib, ptr, require_gpu, stream_ptr
from ._clouds import IntList, clouds, device_i32, lengths as _lengths

_OP, _TITLE = "occupancy_grid", "occupancy grid"


def max_resolution() -> int:
    """Largest lattice resolution supported."""
    return lib().npcd_occupancy_max_resolution()


def clouds_per_workgroup(n: int, P: int, resolution: int = 28) -> int:
    """How many consecutive clouds the launch gives one workgroup (a cloud is never split)."""
    got = lib().npcd_occupancy_clouds_per_workgroup(n, P, resolution)
    check(min(got, 0), "npcd_occupancy_clouds_per_workgroup")
    return got


def _grid_arguments(resolution, extent, largest: Optional[int] = None) -> Tuple[int, float]:
    if isinstance(resolution, bool) or not isinstance(resolution, int) or resolution < 2 or (largest is not None and resolution > largest):
        top = "" if largest is None else f", {largest}"
        raise ValueError(f"{_OP}: resolution must be an integer in [2{top}]; got {resolution!r}")
    extent = float(extent)
    if not (math.isfinite(extent) and extent > 0):
        raise ValueError(f"{_OP}: extent must be positive and finite; got {extent!r}")
    return resolution, extent


def _lattice(resolution: int, extent: float) -> np.ndarray:
    # float64 on the host, rounded once to fp32
    return (np.arange(resolution, dtype=np.float64) * (2.0 * extent / (resolution - 1)) - extent).astype(np.float32)


def _mask(lattice: np.ndarray, extent: float, in_sphere: bool) -> np.ndarray:
    R = len(lattice)
    if not in_sphere:
        return np.ones((R, R, R), dtype=bool)
    sq = lattice.astype(np.float64) ** 2
    return sq[:, None, None] + sq[None, :, None] + sq[None, None, :] <= extent * extent


def grid_lattice(resolution: int = 28, extent: float = 0.5) -> torch.Tensor:
    """-> fp32 [R] on the CPU: g[a] = fp32(a (2 extent / (R - 1)) - extent), the cell centres along every axis."""
    resolution, extent = _grid_arguments(resolution, extent)
    return torch.from_numpy(_lattice(resolution, extent))


def grid_mask(resolution: int = 28, extent: float = 0.5, in_sphere: bool = True) -> torch.Tensor:
    """-> bool [R, R, R] on the CPU: the valid cells.  in_sphere: those with g[i]^2 + g[j]^2 + g[k]^2 <= extent^2, decided in
    float64 on the fp32 lattice values; otherwise all."""
    resolution, extent = _grid_arguments(resolution, extent)
    return torch.from_numpy(_mask(_lattice(resolution, extent), extent, bool(in_sphere)))


def _columns(mask: np.ndarray):
    """The mask as the kernel takes it: per column (i, j) the inclusive range [k_lo, k_hi] of valid k, k_lo > k_hi when empty."""
    R = mask.shape[0]
    some = mask.any(axis=2)
    lo = np.where(some, mask.argmax(axis=2), 1).astype(np.uint8)
    hi = np.where(some, R - 1 - mask[:, :, ::-1].argmax(axis=2), 0).astype(np.uint8)
    k = np.arange(R)
    if not np.array_equal(mask, (k >= lo[:, :, None]) & (k <= hi[:, :, None])):
        raise ValueError(f"{_OP}: the valid cells of a column must be one interval")
    return lo.reshape(-1), hi.reshape(-1)


_tables = {}


def _host_tables(resolution: int, extent: float, in_sphere: bool):
    """(lattice, k_lo, k_hi) as numpy arrays, made once per grid; an empty mask is refused here."""
    key = (resolution, extent, in_sphere)
    if key not in _tables:
        lattice = _lattice(resolution, extent)
        mask = _mask(lattice, extent, in_sphere)
        if not mask.any():
            raise ValueError(f"{_OP}: no cell of the {resolution}^3 lattice is valid (extent {extent}, in_sphere {in_sphere})")
        _tables[key] = (lattice, *_columns(mask))
    return _tables[key]


def _device_tables(resolution: int, extent: float, in_sphere: bool, dev):
    """The same on the device, uploaded once per grid and device."""
    key = (resolution, extent, in_sphere, str(dev))
    if key not in _tables:
        _tables[key] = tuple(torch.from_numpy(a).to(dev) for a in _host_tables(resolution, extent, in_sphere))
    return _tables[key]


def occupancy_grid(points: torch.Tensor, lengths: Optional[IntList] = None, resolution: int = 28, extent: float = 0.5,
                   in_sphere: bool = True, return_cells: bool = False, out=None):
    """points [n, P, 3] fp32 on the GPU -> (counts [R, R, R], clouds [R, R, R][, cells [n, P]]), all int32 on the GPU.

    Every point goes to the valid cell of the lattice `grid_lattice(resolution, extent)` whose centre is nearest; the valid cells
    are `grid_mask(resolution, extent, in_sphere)`.  counts: points per cell; clouds: clouds with at least one point in the cell;
    cells (with return_cells): each point's flat cell index (i R + j) R + k, -1 where the point was not counted.  Not counted are
    the rows at or after a cloud's length and points with a non-finite coordinate.  `lengths`: valid points per cloud as for
    npcd.hip.chamfer -- host values are checked here, a GPU tensor is never read back and is clamped to [1, P] by the kernel.
    out = (counts, clouds): int32 GPU tensors of R^3 elements that are accumulated into (a set fed in batches) and returned;
    otherwise fresh zeros.  n P < 2^31."""
    points = clouds(points, "points", _OP, _TITLE)
    n, P = points.shape[0], points.shape[1]
    lens = _lengths(lengths, n, P, "lengths", _OP)
    resolution, extent = _grid_arguments(resolution, extent, max_resolution())
    _host_tables(resolution, extent, bool(in_sphere))
    if n * P >= 1 << 31:
        raise ValueError(f"{_OP}: {n} clouds of {P} points are 2^31 points or more; feed the set in batches through out=")
    require_gpu(points, lens if isinstance(lens, torch.Tensor) else None)
    dev = points.device
    lattice, lo, hi = _device_tables(resolution, extent, bool(in_sphere), dev)
    if out is None:
        counts, per_cloud = (torch.zeros((resolution,) * 3, dtype=torch.int32, device=dev) for _ in range(2))
    else:
        counts, per_cloud = out
        for name, t in (("counts", counts), ("clouds", per_cloud)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() != resolution ** 3 or not t.is_contiguous():
                raise ValueError(f"{_OP}: out {name} must be a contiguous int32 tensor of {resolution}^3 elements")
            if t.device != dev:
                raise RuntimeError(f"{_OP}: points are on {dev}, out {name} on {t.device}")
    points = points.detach().contiguous()
    cells = torch.empty((n, P), dtype=torch.int32, device=dev) if return_cells else None
    with torch.cuda.device(dev):
        check(lib().npcd_occupancy_grid(ptr(points), ptr(device_i32(lens, dev)), ptr(lattice), ptr(lo), ptr(hi), ptr(counts),
                                        ptr(per_cloud), ptr(cells), n, P, resolution, stream_ptr()), "npcd_occupancy_grid")
    return (counts, per_cloud, cells) if return_cells else (counts, per_cloud)
