#!/usr/bin/env python3
"""Vertex clustering of a mesh (csrc/simplify.hip) beside a torch composition of the same job and beside the
isosurface call that made the mesh: the isosurface of a sphere volume on a `--resolution`^3 lattice (npcd.hip.isosurface), clustered
at k lattice spacings for every k of `--k`, with three attribute channels.  HIP events, `--warmup` rounds first, then `--reps` rounds
in which the legs alternate, the whole repeated `--runs` times so that the spread between runs shows beside the spread inside one;
median with min-max; one JSON line per k and run.

    python tools/probes/gpu_dev_simplify.py [--resolution 256] [--k 2 4] [--reps 7] [--warmup 2] [--runs 3]

Legs: the four entry points alone on buffers made beforehand -- cluster (a memset and the mark, rank, totals and accumulate launches),
faces (one launch), unique (a memset and the unique, flags and totals launches) and emit (finish and compact) --, the stable torch.sort
of the face keys between them, simplify_mesh() as the caller sees it (allocations, the host read of (V', F')), the torch composition
(floor, unique(return_inverse), float64 index_add_, sort of the faces' rows, a stable sort of packed keys), and the isosurface call.
The composition sums in float64 by atomics, in an order nothing fixes; whether its positions agree with the kernels' and with its own
second run is reported, not assumed."""
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
from npcd.hip.isosurface import isosurface  # noqa: E402
from npcd.hip.simplify import simplify_mesh, workspace_bytes  # noqa: E402


def sphere_volume(G):
    axis = torch.linspace(-1, 1, G, device="cuda")
    z, y, x = torch.meshgrid(axis, axis, axis, indexing="ij")
    return (0.75 - torch.sqrt((x - 0.013) ** 2 + (y + 0.021) ** 2 + (z - 0.034) ** 2)).contiguous()


def torch_composition(v, f, origin, cell, dims):
    """The same job from torch operators -> (vertices', faces', attributes' is left out: one more index_add_)."""
    u = (v.double() - origin) / cell
    c = torch.minimum(torch.clamp(u.floor(), min=0), torch.tensor([d - 1.0 for d in dims], dtype=torch.float64, device=v.device)).long()
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    occupied, cluster = torch.unique(key, return_inverse=True)
    n = occupied.shape[0]
    sums = torch.zeros((n, 3), dtype=torch.float64, device=v.device).index_add_(0, cluster, v.double())
    count = torch.zeros(n, dtype=torch.float64, device=v.device).index_add_(0, cluster, torch.ones_like(key, dtype=torch.float64))
    position = (sums / count[:, None]).float()
    m = cluster[f.long()]
    valid = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    s = torch.sort(m, dim=1)[0]
    packed = torch.where(valid, (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2], torch.iinfo(torch.int64).max)
    ordered, order = torch.sort(packed, stable=True)
    first = torch.ones_like(valid)
    first[1:] = ordered[1:] != ordered[:-1]
    keep = torch.zeros_like(valid)
    keep[order] = first & (ordered != torch.iinfo(torch.int64).max)
    return position, m[keep].int(), cluster


def measure(vol, step, k, warmup, reps, run):
    L, P = hip.lib(), hip.ptr
    G = vol.shape[0]
    origin3, spacing3 = (-1.0, -1.0, -1.0), (step, step, step)
    (v, f) = isosurface(vol, 0.0, origin3, spacing3)[0]
    attrs = (0.5 + 0.5 * torch.sin(7.0 * v)).contiguous()
    V, F, C = v.shape[0], f.shape[0], 3
    dims = [int((G - 1) // k) + 1] * 3
    cell = [k * step] * 3
    org, size, width = (ctypes.c_double * 3)(*origin3), (ctypes.c_int * 3)(*dims), (ctypes.c_double * 3)(*cell)
    ws = torch.empty(workspace_bytes(V, F, C, dims) // 8 + 1, dtype=torch.int64, device="cuda")
    cluster = torch.empty(V, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    key_lo = torch.empty(F, dtype=torch.int64, device="cuda")
    whole = simplify_mesh(v, f, cell, origin=origin3, dims=dims, attributes=attrs)
    Vp, Fp = whole["vertices"].shape[0], whole["faces"].shape[0]
    out_v, out_a = torch.empty((Vp, 3), device="cuda"), torch.empty((Vp, C), device="cuda")
    out_f, out_s = torch.empty((Fp, 3), dtype=torch.int32, device="cuda"), torch.empty(Fp, dtype=torch.int32, device="cuda")
    state = {}
    t_origin, t_cell = torch.tensor(origin3, dtype=torch.float64, device="cuda"), torch.tensor(cell, dtype=torch.float64, device="cuda")

    def leg_cluster():
        hip.check(L.npcd_simplify_cluster(P(v), V, F, P(attrs), C, org, width, size, P(ws), P(cluster), P(counts), hip.stream_ptr()), "cluster")

    def leg_faces():
        hip.check(L.npcd_simplify_faces(P(f), V, F, C, size, P(cluster), P(ws), None, P(key_lo), hip.stream_ptr()), "faces")

    def leg_sort():
        state["order"] = torch.sort(key_lo, stable=True)[1]

    def leg_unique():
        hip.check(L.npcd_simplify_unique(P(state["order"]), V, F, C, size, P(ws), P(counts), hip.stream_ptr()), "unique")

    def leg_emit():
        hip.check(L.npcd_simplify_emit(V, F, C, org, width, size, P(ws), Vp, Fp, P(out_v), P(out_a), P(out_f), P(out_s), hip.stream_ptr()), "emit")
    legs = {"cluster": leg_cluster, "faces": leg_faces, "torch_sort": leg_sort, "unique": leg_unique, "emit": leg_emit,
            "simplify_mesh_call": lambda: simplify_mesh(v, f, cell, origin=origin3, dims=dims, attributes=attrs),
            "torch_composition": lambda: torch_composition(v, f, t_origin, t_cell, dims),
            "isosurface_call": lambda: isosurface(vol, 0.0, origin3, spacing3)}
    times = {name: [] for name in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():          # the legs alternate inside every round; the entry points run in their order
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    stats = {f"{name}_ms_median_min_max": [round(sorted(t)[len(t) // 2], 4), round(min(t), 4), round(max(t), 4)] for name, t in times.items()}
    assert counts.tolist() == [Vp, Fp] and torch.equal(out_v, whole["vertices"]) and torch.equal(out_f, whole["faces"])
    assert torch.equal(out_a, whole["attributes"]) and torch.equal(out_s, whole["face_source"])
    ref_v, ref_f, ref_cluster = torch_composition(v, f, t_origin, t_cell, dims)
    again_v = torch_composition(v, f, t_origin, t_cell, dims)[0]
    launches = sum(stats[f"{name}_ms_median_min_max"][0] for name in ("cluster", "faces", "torch_sort", "unique", "emit"))
    stats.update({
        "gpu": torch.cuda.get_device_name(0), "run": run, "resolution": G, "k": k, "vertices": [V, Vp], "faces": [F, Fp], "channels": C,
        "cells": dims[0] * dims[1] * dims[2], "entry_points_and_sort_ms": round(launches, 4),
        "composition_over_simplify_mesh_call": round(stats["torch_composition_ms_median_min_max"][0] / stats["simplify_mesh_call_ms_median_min_max"][0], 2),
        "simplify_mesh_call_over_isosurface_call": round(stats["simplify_mesh_call_ms_median_min_max"][0] / stats["isosurface_call_ms_median_min_max"][0], 2),
        "same_clusters_and_faces_as_the_composition": bool(torch.equal(ref_cluster.int(), whole["vertex_cluster"]) and torch.equal(ref_f, whole["faces"])),
        "max_position_difference_to_the_composition": float((ref_v - whole["vertices"]).abs().max()),
        "composition_positions_equal_on_two_runs": bool(torch.equal(ref_v, again_v)),
        "kernel_positions_equal_on_two_runs": bool(torch.equal(simplify_mesh(v, f, cell, origin=origin3, dims=dims, attributes=attrs)["vertices"], whole["vertices"])),
    })
    print(json.dumps(stats), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--k", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_simplify needs a GPU: a time taken anywhere else says nothing")
    vol = sphere_volume(args.resolution)
    step = 2.0 / (args.resolution - 1)
    for run in range(args.runs):
        for k in args.k:
            measure(vol, step, k, args.warmup, args.reps, run)


if __name__ == "__main__":
    main()
