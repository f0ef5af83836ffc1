#!/usr/bin/env python3
"""Mesh edges and Taubin smoothing (csrc/smooth.hip) beside a torch composition of the same work: the isosurface of a
sphere volume on a `--resolution`^3 lattice (npcd.hip.isosurface) and its simplification at k = 2 (npcd.hip.simplify).  HIP events,
`--warmup` rounds first, then `--reps` rounds in which the legs alternate, the whole repeated `--runs` times so that the spread between
runs shows beside the spread inside one; median with min-max; one JSON line per mesh and run.

    python tools/probes/gpu_dev_smooth.py [--resolution 256] [--iterations 10] [--reps 7] [--warmup 2] [--runs 3]

Legs: the three entry points of the edges alone on buffers made beforehand -- keys (one launch), unique (a memset and the marks and
totals launches) and emit (a memset and the emit and counts launches) --, the torch.sort of the 6F keys between them, mesh_edges() as the caller sees it
(allocations, the host read of the counts), smooth_mesh() at `--iterations` with the adjacency given and at 0 + 1 iterations for what
a call costs without steps (the per-step time is the difference over the steps), and the torch composition: unique on the edge keys,
then per step a float32 index_add_ of the neighbours' positions.  The composition sums floats by atomics, in an order nothing fixes;
whether its positions agree with its own second run is reported, not assumed."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))
sys.path.insert(0, ROOT)

from npcd import hip  # noqa: E402
from npcd.hip.isosurface import isosurface  # noqa: E402
from npcd.hip.simplify import simplify_mesh  # noqa: E402
from npcd.hip.smooth import mesh_edges, smooth_mesh, workspace_bytes  # noqa: E402


def sphere_volume(G):
    axis = torch.linspace(-1, 1, G, device="cuda")
    z, y, x = torch.meshgrid(axis, axis, axis, indexing="ij")
    return (0.75 - torch.sqrt((x - 0.013) ** 2 + (y + 0.021) ** 2 + (z - 0.034) ** 2)).contiguous()


def composition_edges(V, f):
    """The directed pairs of a mesh of valid faces from torch operators -> (source, target) int64, unique."""
    g = f.long()
    a, b = g.reshape(-1), g[:, [1, 2, 0]].reshape(-1)
    keys = torch.unique(torch.cat([a * 2 ** 31 + b, b * 2 ** 31 + a]))
    return keys >> 31, keys & (2 ** 31 - 1)


def composition_smooth(v, source, target, iterations, lam, mu):
    """Taubin's steps on float32 positions: index_add_ of the neighbours, by float atomics."""
    degree = torch.zeros(v.shape[0], device=v.device).index_add_(0, source, torch.ones(source.shape[0], device=v.device)).clamp_(min=1)[:, None]
    x = v.clone()
    for _ in range(iterations):
        for factor in (lam, mu):
            mean = torch.zeros_like(x).index_add_(0, source, x[target]) / degree
            x = x + factor * (mean - x)
    return x


def measure(label, v, f, iterations, warmup, reps, run):
    L, P = hip.lib(), hip.ptr
    V, F = v.shape[0], f.shape[0]
    lam, mu = 0.5, -0.53
    keys = torch.empty(6 * F, dtype=torch.int64, device="cuda")
    ws = torch.empty(workspace_bytes(V, F) // 8 + 1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(6, dtype=torch.int64, device="cuda")
    whole = mesh_edges(V, f)
    D = whole["neighbours"].shape[0]
    out = {k: torch.empty_like(t) for k, t in whole.items() if k != "counts"}
    state = {}
    source, target = composition_edges(V, f)

    def leg_keys():
        hip.check(L.npcd_mesh_edges_keys(P(f), V, F, P(keys), hip.stream_ptr()), "keys")

    def leg_sort():
        state["sorted"] = torch.sort(keys)[0]

    def leg_unique():
        hip.check(L.npcd_mesh_edges_unique(P(state["sorted"]), V, F, P(ws), P(counts), hip.stream_ptr()), "unique")

    def leg_emit():
        hip.check(L.npcd_mesh_edges_emit(P(state["sorted"]), V, F, P(ws), D, P(out["row_start"]), P(out["neighbours"]), P(out["edges"]),
                                         P(out["edge_faces"]), P(out["edge_forward"]), P(out["boundary_vertex"]), P(counts), hip.stream_ptr()), "emit")
    legs = {"keys": leg_keys, "torch_sort": leg_sort, "unique": leg_unique, "emit": leg_emit,
            "mesh_edges_call": lambda: mesh_edges(V, f),
            "smooth_mesh_call": lambda: smooth_mesh(v, None, iterations, lam, mu, edges=whole),
            "smooth_mesh_one_iteration": lambda: smooth_mesh(v, None, 1, lam, mu, edges=whole),
            "composition_edges": lambda: composition_edges(V, f),
            "composition_smooth": lambda: composition_smooth(v, source, target, iterations, lam, mu)}
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
    median = lambda name: stats[f"{name}_ms_median_min_max"][0]
    assert counts.tolist() == whole["counts"].tolist() and all(torch.equal(out[k], whole[k]) for k in out)
    ours, again = smooth_mesh(v, None, iterations, lam, mu, edges=whole), smooth_mesh(v, None, iterations, lam, mu, edges=whole)
    theirs, theirs_again = (composition_smooth(v, source, target, iterations, lam, mu) for _ in range(2))
    stats.update({
        "gpu": torch.cuda.get_device_name(0), "run": run, "mesh": label, "vertices": V, "faces": F, "distinct_pairs": D,
        "iterations": iterations, "counts": whole["counts"].tolist(), "largest_degree": int((whole["row_start"][1:] - whole["row_start"][:-1]).max()),
        "entry_points_and_sort_ms": round(sum(median(n) for n in ("keys", "torch_sort", "unique", "emit")), 4),
        "per_step_us": round(1000.0 * (median("smooth_mesh_call") - median("smooth_mesh_one_iteration")) / (2 * iterations - 2), 3) if iterations > 1 else None,
        "composition_edges_over_mesh_edges_call": round(median("composition_edges") / median("mesh_edges_call"), 2),
        "composition_smooth_over_smooth_mesh_call": round(median("composition_smooth") / median("smooth_mesh_call"), 2),
        "same_pairs_as_the_composition": bool(torch.equal(target.int(), whole["neighbours"])),
        "max_position_difference_to_the_composition": float((ours - theirs).abs().max()),
        "composition_positions_equal_on_two_runs": bool(torch.equal(theirs, theirs_again)),
        "kernel_positions_equal_on_two_runs": bool(torch.equal(ours, again)),
    })
    print(json.dumps(stats), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_smooth needs a GPU: a time taken anywhere else says nothing")
    G = args.resolution
    step = 2.0 / (G - 1)
    (v, f) = isosurface(sphere_volume(G), 0.0, (-1.0, -1.0, -1.0), (step, step, step))[0]
    small = simplify_mesh(v, f, [2 * step] * 3, origin=(-1.0, -1.0, -1.0), dims=[(G - 1) // 2 + 1] * 3)
    for run in range(args.runs):
        measure("isosurface", v, f, args.iterations, args.warmup, args.reps, run)
        measure("simplified_k2", small["vertices"], small["faces"], args.iterations, args.warmup, args.reps, run)


if __name__ == "__main__":
    main()
