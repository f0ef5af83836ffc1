#!/usr/bin/env python3
"""Mesh export of a generated object: PointNeRF.density_grid and the isosurface kernels (csrc/isosurface.hip) at
128^3 and 256^3 on the bench scene's cloud (oracle.renderer.synthetic_cloud(512, 32, 1, seed=0), init_field_params(32, seed=0)).
HIP events, `--warmup` calls first, median with min-max over `--reps`; one JSON line per resolution.

    python tools/probes/gpu_dev_isosurface.py [--resolutions 128,256] [--reps 5] [--warmup 2]

Timed legs: density_grid (neighbour query + shading of the nodes that have a neighbour + scatter, `chunk` nodes at a time);
isosurface() as the caller sees it (workspace, both passes, the host read between them, the outputs); and the two entry points
alone on buffers made beforehand -- count (two launches) and emit (one) -- beside the bytes each must move at least:
count reads the volume and writes one word per node (8 bytes a node), emit reads the words (4 bytes a node; it reads the volume only at
crossed edges) and writes 12 bytes per vertex and per triangle.  The same two on white noise of the same size, where nearly every
edge is crossed: the densest case for the scans and the writes.  The level is the median of the non-zero densities (the weights
are untrained; the default level of extract_mesh is printed beside it with what it would give)."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))
sys.path.insert(0, ROOT)

from npcd import hip  # noqa: E402
from npcd.eval.mesh import default_level  # noqa: E402
from npcd.hip.isosurface import isosurface, workspace_bytes  # noqa: E402
from npcd.models.pointnerf import PointNeRF  # noqa: E402
from oracle import renderer as orr  # noqa: E402


def timed(fn, warmup, reps):
    """-> ([median ms, min, max], last output)"""
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
    return [round(sorted(times)[len(times) // 2], 4), round(min(times), 4), round(max(times), 4)], out


def passes(vol, level, origin, spacing, warmup, reps):
    """The two entry points alone -> (count ms, emit ms, vertices, faces)."""
    L = hip.lib()
    B, gz, gy, gx = vol.shape
    ws = torch.empty(workspace_bytes(B, gz, gy, gx), dtype=torch.uint8, device=vol.device)
    counts = torch.empty((B, 2), dtype=torch.int64, device=vol.device)
    org, step = (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(*spacing)

    def count():
        hip.check(L.npcd_isosurface_count(hip.ptr(vol), B, gz, gy, gx, level, hip.ptr(ws), hip.ptr(counts), hip.stream_ptr()), "count")
    t_count, _ = timed(count, warmup, reps)
    n_vert, n_face = (int(v) for v in counts.sum(dim=0).cpu())
    offsets = (torch.cumsum(counts, 0) - counts).t().contiguous()
    vertices = torch.empty((max(n_vert, 1), 3), dtype=torch.float32, device=vol.device)
    faces = torch.empty((max(n_face, 1), 3), dtype=torch.int32, device=vol.device)

    def emit():
        hip.check(L.npcd_isosurface_emit(hip.ptr(vol), B, gz, gy, gx, level, org, step, hip.ptr(ws), hip.ptr(offsets[0]), hip.ptr(offsets[1]),
                                         hip.ptr(vertices), hip.ptr(faces), hip.stream_ptr()), "emit")
    t_emit, _ = timed(emit, warmup, reps)
    return t_count, t_emit, n_vert, n_face


def gb_per_s(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e9, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", default="128,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_isosurface needs a GPU: a time taken anywhere else says nothing")
    name = torch.cuda.get_device_name(0)
    m = PointNeRF(1, 32, 512, False)
    m.field.load_state_dict(orr.init_field_params(32, seed=0))
    m = m.cuda().eval()
    coords, feats = (t.cuda() for t in orr.synthetic_cloud(512, 32, 1, seed=0))
    for G in (int(g) for g in args.resolutions.split(",")):
        t_grid, (sigma, origin, spacing) = timed(lambda: m.density_grid(coords, feats, resolution=G), args.warmup, args.reps)
        origin, spacing = origin.tolist(), spacing.tolist()
        shaded = int((sigma > 0).sum())
        level = float(sigma[sigma > 0].median())
        t_whole, meshes = timed(lambda: isosurface(sigma, level, origin, spacing), args.warmup, args.reps)
        t_count, t_emit, n_vert, n_face = passes(sigma, level, origin, spacing, args.warmup, args.reps)
        at_default = isosurface(sigma, default_level(m), origin, spacing)[0]
        noise = torch.randn(sigma.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(G))
        w_count, w_emit, w_vert, w_face = passes(noise, 0.0, origin, spacing, args.warmup, args.reps)
        n = G ** 3
        print(json.dumps({
            "gpu": name, "resolution": G, "nodes": n, "volume_bytes": 4 * n, "nodes_with_a_neighbour": shaded,
            "level_median_of_nonzero": round(level, 5), "vertices": n_vert, "faces": n_face,
            "default_level": round(default_level(m), 3), "at_default_level_vertices_faces": [len(at_default[0]), len(at_default[1])],
            "density_grid_ms_median_min_max": t_grid,
            "isosurface_call_ms_median_min_max": t_whole,
            "count_ms_median_min_max": t_count, "count_bytes": 8 * n, "count_GB_per_s": gb_per_s(8 * n, t_count[0]),
            "emit_ms_median_min_max": t_emit, "emit_bytes": 4 * n + 12 * (n_vert + n_face),
            "emit_GB_per_s": gb_per_s(4 * n + 12 * (n_vert + n_face), t_emit[0]),
            "volume_bytes_over_both_passes_GB_per_s": gb_per_s(4 * n, t_count[0] + t_emit[0]),
            "noise_vertices_faces": [w_vert, w_face], "noise_count_ms_median_min_max": w_count, "noise_emit_ms_median_min_max": w_emit,
            "noise_emit_bytes": 4 * n + 12 * (w_vert + w_face), "noise_emit_GB_per_s": gb_per_s(4 * n + 12 * (w_vert + w_face), w_emit[0]),
            "same_mesh_from_the_call_and_the_passes": [len(meshes[0][0]), len(meshes[0][1])] == [n_vert, n_face],
        }), flush=True)


if __name__ == "__main__":
    main()
