"""From raw surface clouds to the fixed geometry of stage 1: every object's cloud is cut down to num_points points by farthest point
sampling on the GPU (npcd.hip.fps), a whole batch of clouds of differing sizes per launch.  The on-disk convention is the reference's
(npcd/data/srn.py:170-193): `<object>/pointcloud3.npz` holds the raw `points` and `normals`, and the subsampled cloud is cached beside
it as `pointcloud3_{num_points}.npz` with the same two keys.
"""
import os
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

RAW_NAME = "pointcloud3.npz"


def cached_name(num_points: int) -> str:
    return f"pointcloud3_{num_points}.npz"


def write_raw_pointcloud(directory: str, points, normals) -> str:
    """Write `<directory>/pointcloud3.npz` with the raw surface cloud of one object: `points` [P, 3] and `normals` [P, 3] as float32,
    the two keys load_pointclouds reads -- e.g. what npcd.hip.surface.sample_surface draws from an extracted mesh.  -> the path."""
    arrays = []
    for name, a in (("points", points), ("normals", normals)):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"write_raw_pointcloud: {name} must be [P, 3]; got {a.shape}")
        arrays.append(np.ascontiguousarray(a, dtype=np.float32))
    if len(arrays[0]) != len(arrays[1]):
        raise ValueError(f"write_raw_pointcloud: {len(arrays[0])} points and {len(arrays[1])} normals")
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, RAW_NAME)
    np.savez(path, points=arrays[0], normals=arrays[1])
    return path


def _default_sampler():
    from npcd.hip.fps import sample_farthest_points
    return sample_farthest_points


def pad_clouds(clouds: Sequence, device=None):
    """Clouds [P_i, 3] of differing sizes -> (points [n, Pmax, 3] fp32 zero-padded, lengths: list of the P_i)."""
    tensors = [torch.as_tensor(np.asarray(c) if not isinstance(c, torch.Tensor) else c).to(torch.float32) for c in clouds]
    for t in tensors:
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"a cloud must be [P, 3]; got {tuple(t.shape)}")
    lengths = [int(t.shape[0]) for t in tensors]
    points = torch.zeros((len(tensors), max(lengths), 3), dtype=torch.float32)
    for i, t in enumerate(tensors):
        points[i, :lengths[i]] = t
    return points.to(device) if device is not None else points, lengths


def subsample_clouds(clouds: Sequence, num_points: int, normals: Optional[Sequence] = None, batch: int = 64,
                     sampler: Optional[Callable] = None, device=None):
    """-> (coords [n, num_points, 3] fp32, normals [n, num_points, 3] or None, idx [n, num_points] int64), on the CPU.

    clouds: n arrays or tensors [P_i, 3] with P_i >= num_points; normals: n arrays [P_i, 3] gathered at the picked indices.
    `batch` clouds at a time are padded to the largest of them and go through ONE launch with their lengths; every cloud starts at its
    point 0 like the reference's call.  coords is what PointNeRF.set_all_coords takes.  `sampler` stands in for
    npcd.hip.fps.sample_farthest_points (tests of the host logic); `device` defaults to the current GPU."""
    n = len(clouds)
    if n == 0:
        raise ValueError("subsample_clouds: no clouds")
    if normals is not None and len(normals) != n:
        raise ValueError(f"subsample_clouds: {len(normals)} normal arrays for {n} clouds")
    if batch < 1 or num_points < 1:
        raise ValueError(f"subsample_clouds: batch {batch}, num_points {num_points}")
    sampler = sampler or _default_sampler()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    coords, idx = [], []
    for first in range(0, n, batch):
        points, lengths = pad_clouds(clouds[first:first + batch], device)
        short = [first + i for i, m in enumerate(lengths) if m < num_points]
        if short:
            raise ValueError(f"subsample_clouds: clouds {short} have fewer than {num_points} points")
        sel, ix = sampler(points, lengths=lengths, K=num_points)
        coords.append(sel.cpu())
        idx.append(ix.cpu())
    coords, idx = torch.cat(coords), torch.cat(idx)
    picked = None
    if normals is not None:
        picked = torch.stack([torch.as_tensor(np.asarray(m)).to(torch.float32)[ix] for m, ix in zip(normals, idx)])
    return coords, picked, idx


def load_pointclouds(paths: Sequence[str], num_points: int, batch: int = 64, sampler: Optional[Callable] = None, device=None) -> List[dict]:
    """One {"points": [num_points, 3], "normals": [num_points, 3]} per object directory.  Objects without a cached
    `pointcloud3_{num_points}.npz` are subsampled from their `pointcloud3.npz`, `batch` of them per launch, and the cache is written;
    every object is then read from its cache, so a first and a later call return the same bits."""
    todo = [p for p in paths if not os.path.isfile(os.path.join(p, cached_name(num_points)))]
    for first in range(0, len(todo), batch):
        group = todo[first:first + batch]
        raw = []
        for p in group:
            with np.load(os.path.join(p, RAW_NAME)) as z:
                raw.append((z["points"].astype(np.float32), z["normals"].astype(np.float32)))
        coords, normals, _ = subsample_clouds([r[0] for r in raw], num_points, [r[1] for r in raw], batch, sampler, device)
        for p, c, m in zip(group, coords, normals):
            np.savez(os.path.join(p, cached_name(num_points)), points=c.numpy(), normals=m.numpy())
    out = []
    for p in paths:
        with np.load(os.path.join(p, cached_name(num_points))) as z:
            out.append({"points": torch.from_numpy(z["points"]).float(), "normals": torch.from_numpy(z["normals"]).float()})
    return out


def load_pointcloud(path: str, num_points: int, sampler: Optional[Callable] = None, device=None) -> dict:
    """The reference's Dataset.load_pointcloud for one object directory."""
    return load_pointclouds([path], num_points, 1, sampler, device)[0]
