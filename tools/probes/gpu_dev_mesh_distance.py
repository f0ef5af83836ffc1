#!/usr/bin/env python3
"""Point-to-mesh distance (csrc/mesh_distance.hip) beside a torch composition of the same formula: `--samples` surface
samples of the isosurface of a sphere volume on a `--resolution`^3 lattice (npcd.hip.isosurface, npcd.hip.surface) against that mesh
and against its simplification at k = 2 (npcd.hip.simplify).  HIP events, `--warmup` rounds first, then `--reps` rounds in which the
legs alternate, the whole repeated `--runs` times; median with min-max; one JSON line per mesh and run, then one for extract_mesh.

    python tools/probes/gpu_dev_mesh_distance.py [--resolution 256] [--samples 100000] [--reps 5] [--warmup 1] [--runs 2]

Legs: the boxes entry point alone; the query entry point on queries sorted beforehand with cull = 1 and cull = 0, and on the unsorted
queries with cull = 1; closest_on_mesh() as the caller sees it (allocations, the sort of the queries, the scatter back); and the torch
composition of the pair formula on a slice of `--slice-points` x `--slice-faces` that fits memory, scaled to the whole by the number
of pairs.  `evaluated` over waves x tiles says what culling left.  The unculled time gives the lane-operations per second of the pair
loop, `--ops-per-pair` vector operations per pair as counted in the ISA listing, beside the 78.65e12 fp32 ceiling of DESIGN.md 5.7.
The last line is extract_mesh(simplify=2, smooth=10) on a stand-in field of the same sphere with and without deviation=`--samples`."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))
sys.path.insert(0, ROOT)

from npcd import hip  # noqa: E402
from npcd.eval.mesh import extract_mesh  # noqa: E402
from npcd.hip.isosurface import isosurface  # noqa: E402
from npcd.hip.mesh_distance import TILE_FACES, WAVE_POINTS, closest_on_mesh, sort_order  # noqa: E402
from npcd.hip.simplify import simplify_mesh  # noqa: E402
from npcd.hip.surface import sample_surface  # noqa: E402

CEILING = 78.65e12          # fp32 lane-operations per second without FMA


def sphere_volume(G):
    axis = torch.linspace(-1, 1, G, device="cuda")
    z, y, x = torch.meshgrid(axis, axis, axis, indexing="ij")
    return (0.75 - torch.sqrt((x - 0.013) ** 2 + (y + 0.021) ** 2 + (z - 0.034) ** 2)).contiguous()


class Field:
    """Stands in for a PointNeRF: the density of the sphere on the lattice, the colour a function of the position."""

    def __init__(self, G):
        self.G = G

    def density_grid(self, coords, feats, resolution=128, bound=None, mlp_dtype=None):
        step = 2.0 / (self.G - 1)
        return sphere_volume(self.G)[None], torch.tensor([-1.0] * 3, device="cuda"), torch.tensor([step] * 3, device="cuda")

    def query_field(self, coords, feats, x, mlp_dtype=None, view_dir=None):
        return None, 0.5 + 0.5 * torch.sin(5.0 * x)


def composition(p, v, f):
    """The pair formula on every (point, face) of a slice with torch operators -> (sqdist, face): [s, f] temporaries throughout."""
    a, b, c = (v[f[:, k].long()][None] for k in range(3))
    p = p[:, None]
    dot = lambda u, w: (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    d43, d56 = d4 - d3, d5 - d6
    t, den = d43 / (d43 + d56), 1.0 / ((va + vb) + vc)
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
               (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d43 >= 0) & (d56 >= 0)]
    vs = [zero, one, d1 / (d1 - d3), zero, zero, one - t]
    ws = [zero, zero, zero, one, d2 / (d2 - d6), t]
    vv, ww = vb * den, vc * den
    for k in range(5, -1, -1):
        vv, ww = torch.where(regions[k], vs[k], vv), torch.where(regions[k], ws[k], ww)
    e = p - (a + (vv[..., None] * ab + ww[..., None] * ac))
    d = dot(e, e)
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return d.min(dim=1)


def timed(legs, warmup, reps):
    times = {name: [] for name in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():          # the legs alternate inside every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    return {name: [round(sorted(t)[len(t) // 2], 4), round(min(t), 4), round(max(t), 4)] for name, t in times.items()}


def measure(label, points, v, f, args, run):
    L, P = hip.lib(), hip.ptr
    S, V, F = points.shape[0], v.shape[0], f.shape[0]
    ws = torch.empty(L.npcd_mesh_distance_ws_bytes(V, F) // 8 + 2, dtype=torch.int64, device="cuda")
    ordered = points[sort_order(points, v)].contiguous()
    out = (torch.empty(S, device="cuda"), torch.empty(S, dtype=torch.int32, device="cuda"), torch.empty(S, 3, device="cuda"))
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")

    def query(queries, cull, count=None):
        hip.check(L.npcd_mesh_distance_query(P(queries), S, P(v), V, P(f), F, P(ws), cull, P(out[0]), P(out[1]), P(out[2]), P(count),
                                             hip.stream_ptr()), "query")
    sp, sf = points[:args.slice_points], f[:args.slice_faces]
    legs = {"boxes": lambda: hip.check(L.npcd_mesh_distance_boxes(P(v), V, P(f), F, P(ws), hip.stream_ptr()), "boxes"),
            "query_sorted_culled": lambda: query(ordered, 1),
            "query_unsorted_culled": lambda: query(points, 1),
            "query_sorted_unculled": lambda: query(ordered, 0),
            "closest_on_mesh_call": lambda: closest_on_mesh(points, v, f),
            "composition_slice": lambda: composition(sp, v, sf)}
    stats = {f"{name}_ms_median_min_max": t for name, t in timed(legs, args.warmup, args.reps).items()}
    median = lambda name: stats[f"{name}_ms_median_min_max"][0]
    evaluated = {}
    for name, queries in (("sorted", ordered), ("unsorted", points)):
        counter.zero_()
        query(queries, 1, counter)
        evaluated[name] = int(counter)
    waves, tiles = -(-S // WAVE_POINTS), -(-F // TILE_FACES)
    whole, plain = closest_on_mesh(points, v, f), closest_on_mesh(points, v, f, cull=False, sort_points=False)
    theirs = composition(sp, v, sf)
    ours = closest_on_mesh(sp, v, sf, cull=False, sort_points=False)
    pairs = S * F
    scale = pairs / (sp.shape[0] * sf.shape[0])
    stats.update({
        "gpu": torch.cuda.get_device_name(0), "run": run, "mesh": label, "points": S, "vertices": V, "faces": F, "waves_x_tiles": waves * tiles,
        "evaluated_sorted": evaluated["sorted"], "evaluated_unsorted": evaluated["unsorted"],
        "evaluated_share_sorted": round(evaluated["sorted"] / (waves * tiles), 5),
        "evaluated_share_unsorted": round(evaluated["unsorted"] / (waves * tiles), 5),
        "unculled_over_culled_sorted": round(median("query_sorted_unculled") / median("query_sorted_culled"), 2),
        "unculled_lane_ops_per_second": round(pairs * args.ops_per_pair / (median("query_sorted_unculled") * 1e-3), 0),
        "unculled_share_of_fp32_ceiling": round(pairs * args.ops_per_pair / (median("query_sorted_unculled") * 1e-3) / CEILING, 4),
        "composition_scaled_ms": round(median("composition_slice") * scale, 1),
        "composition_scaled_over_unculled": round(median("composition_slice") * scale / median("query_sorted_unculled"), 1),
        "composition_scaled_over_call": round(median("composition_slice") * scale / median("closest_on_mesh_call"), 1),
        "culled_equals_unculled_bits": all(bool(torch.equal(whole[k].view(torch.int32), plain[k].view(torch.int32))) for k in whole),
        "composition_slice_equals_kernel": bool(torch.equal(theirs[0].view(torch.int32), ours["sqdist"].view(torch.int32))),
        "largest_distance": float(whole["sqdist"].max().sqrt()),
    })
    print(json.dumps(stats), flush=True)


def end_to_end(args):
    field = Field(args.resolution)
    coords, feats = torch.zeros(1, 4, 3, device="cuda"), torch.zeros(1, 4, 8, device="cuda")
    common = dict(resolution=args.resolution, level=0.0, simplify=2, smooth=10)
    times = {"without": [], "with_deviation": []}
    for r in range(args.warmup + args.reps):
        for name, extra in (("without", {}), ("with_deviation", {"deviation": args.samples})):
            torch.cuda.synchronize()
            start = time.perf_counter()
            (mesh,) = extract_mesh(field, coords, feats, **common, **extra)
            torch.cuda.synchronize()
            if r >= args.warmup:
                times[name].append(1000.0 * (time.perf_counter() - start))
    stats = {f"extract_mesh_{name}_ms_median_min_max": [round(sorted(t)[len(t) // 2], 2), round(min(t), 2), round(max(t), 2)] for name, t in times.items()}
    stats.update({"faces": int(mesh["faces"].shape[0]), "deviation": mesh["deviation"], "spacing": 2.0 / (args.resolution - 1)})
    print(json.dumps(stats), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--slice-points", type=int, default=2048)
    ap.add_argument("--slice-faces", type=int, default=8192)
    ap.add_argument("--ops-per-pair", type=int, default=129, help="vector operations per (point, face) in the pair loop of the ISA listing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_mesh_distance needs a GPU: a time taken anywhere else says nothing")
    G = args.resolution
    step = 2.0 / (G - 1)
    (v, f) = isosurface(sphere_volume(G), 0.0, (-1.0, -1.0, -1.0), (step, step, step))[0]
    small = simplify_mesh(v, f, [2 * step] * 3, origin=(-1.0, -1.0, -1.0), dims=[(G - 1) // 2 + 1] * 3)
    points = sample_surface((v, f), args.samples, generator=torch.Generator(device="cuda").manual_seed(1))[0]
    for run in range(args.runs):
        measure("isosurface", points, v, f, args, run)
        measure("simplified_k2", points, small["vertices"], small["faces"], args, run)
    end_to_end(args)


if __name__ == "__main__":
    main()
