#!/usr/bin/env python3
"""Occupancy grid of point clouds: the HIP kernel (csrc/occupancy.hip) against what a user could do without it on the
same GPU in the same process -- the same spec written as torch operators: `cdist` of the points against the valid cell centres in
chunks of `--chunk` points, `argmin`, `bincount`, and the clouds-per-cell histogram from a `unique` of (cloud, cell) pairs.  HIP
events, one warm-up call per leg, median with min-max; one JSON line per case.

    python tools/probes/gpu_dev_occupancy.py [--cases a,b] [--reps 3] [--chunk 65536]

  (a) 2,000 clouds of 512 points      (b) 1,000 clouds of 2,048 points
both Gaussian clouds normalised to their bounding boxes, on the 28^3 lattice of half-width 1 clipped to the sphere, so that the
search for the nearest valid cell carries its real share (printed as `searched_share`).

The estimate printed beside the times counts wave instructions as the kernel's source has them: about 60 for a point on the fast
path (load, three axis indices, two LDS atomics, the store of its cell) and, for a point that is searched, ceil(R^2 / 64) = 13
column steps of about 20 instructions (one LDS word, four field extractions, a clamp, three LDS reads, eight for the distance, three
for the key and the minimum) plus about 40 for the wave minimum, issued once for the whole wave; a compute unit issues 2 wave
instructions per cycle at 2.4 GHz.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))

from npcd.eval import normalize_clouds  # noqa: E402
from npcd.hip.occupancy import clouds_per_workgroup, grid_lattice, grid_mask, occupancy_grid  # noqa: E402

WAVE_INSTRUCTIONS_PER_SECOND = 2.4e9 * 256 * 2
R, EXTENT = 28, 1.0


def torch_grid(points, centres, cell_of_centre, chunk):
    """The spec on torch operators -> (counts [R^3], clouds [R^3], cells [n, P])."""
    n, P, _ = points.shape
    flat = points.reshape(-1, 3)
    cells = torch.empty(n * P, dtype=torch.int64, device=points.device)
    for p0 in range(0, n * P, chunk):
        cells[p0:p0 + chunk] = cell_of_centre[torch.cdist(flat[p0:p0 + chunk], centres).argmin(dim=1)]
    counts = torch.bincount(cells, minlength=R ** 3)
    pairs = torch.unique(cells + R ** 3 * torch.arange(n, device=points.device).repeat_interleave(P))
    clouds = torch.bincount(pairs % R ** 3, minlength=R ** 3)
    return counts, clouds, cells.view(n, P)


def timed(fn, warmup, reps):
    """-> (median ms, min, max, last output)"""
    out = None
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2], min(times), max(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=65536)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_occupancy needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    lattice, mask = grid_lattice(R, EXTENT), grid_mask(R, EXTENT, True)
    i, j, k = mask.nonzero(as_tuple=True)
    centres = torch.stack([lattice[i], lattice[j], lattice[k]], dim=1).to(dev)
    cell_of_centre = ((i * R + j) * R + k).to(dev)
    shapes = {"a": (2000, 512), "b": (1000, 2048)}
    for case in args.cases.split(","):
        n, P = shapes[case]
        g = torch.Generator().manual_seed(n + P)
        points = normalize_clouds(torch.randn(n, P, 3, generator=g).to(dev), "bbox").contiguous()
        hip = timed(lambda: occupancy_grid(points, None, R, EXTENT, True), 1, args.reps)
        with_cells = timed(lambda: occupancy_grid(points, None, R, EXTENT, True, return_cells=True), 1, args.reps)
        tor = timed(lambda: torch_grid(points, centres, cell_of_centre, args.chunk), 1, args.reps)
        counts, clouds, cells = with_cells[3]
        t_counts, t_clouds, t_cells = tor[3]
        # the unconstrained nearest cell, per axis, in float64: the share of points whose own cell is outside the sphere
        own = ((points.double() + EXTENT) / (2 * EXTENT / (R - 1))).round().clamp(0, R - 1).long()
        searched = float((~mask.to(dev)[own[..., 0], own[..., 1], own[..., 2]]).double().mean())
        fast, search = 60 * n * P / 64, searched * n * P * (13 * 20 + 40)
        rnd = lambda t: [round(t[0], 3), round(t[1], 3), round(t[2], 3)]
        print(json.dumps({
            "case": case, "gpu": name, "clouds": n, "points_per_cloud": P, "resolution": R, "extent": EXTENT, "valid_cells": int(mask.sum()),
            "clouds_per_workgroup": clouds_per_workgroup(n, P, R), "workgroups": -(-n // clouds_per_workgroup(n, P, R)),
            "searched_share": round(searched, 4), "occupied_cells": int((counts > 0).sum()),
            "hip_ms_median_min_max": rnd(hip), "hip_with_cells_ms_median_min_max": rnd(with_cells),
            "torch_ms_median_min_max": rnd(tor), "torch_chunk_points": args.chunk,
            "torch_over_hip": round(tor[0] / hip[0], 1),
            "estimate_ms_vector_issue": round(1e3 * (fast + search) / WAVE_INSTRUCTIONS_PER_SECOND, 4),
            "estimate_wave_instructions_fast_and_search": [int(fast), int(search)],
            "global_integer_atomics_at_most": int(2 * min(n * P, -(-n // clouds_per_workgroup(n, P, R)) * int(mask.sum()))),
            "cells_differing_from_torch": int((cells != t_cells).sum()),
            "counts_differing_from_torch": int((counts.reshape(-1) != t_counts).sum()),
            "clouds_differing_from_torch": int((clouds.reshape(-1) != t_clouds).sum()),
        }), flush=True)


if __name__ == "__main__":
    main()
