#!/usr/bin/env python3
"""Crossing counts (csrc/crossings.hip) on a large mesh: the `--nodes`^3 voxelisation of the isosurface of a sphere
volume on a `--resolution`^3 lattice (npcd.hip.isosurface; 256 gives the 1.03 M faces of R35.1 / R37.1).  HIP events, `--warmup`
rounds first, then `--reps` rounds in which the legs alternate, the whole repeated `--runs` times; median with min-max; one JSON line
per run.

    python tools/probes/gpu_dev_crossings.py [--resolution 256] [--nodes 128] [--reps 5] [--warmup 1] [--runs 2]

Legs: the culled query on the lattice's nodes along +x and along (1, 2, 3), each with the nodes in 8 x 8 patches across x
(PATCH_ACROSS) and in 4 x 4 x 4 blocks (PATCH_BLOCK), with `evaluated` over waves x tiles for each; voxelize_mesh() as the caller
sees it (node positions, the order, one mesh_boxes, one count, the scatter); the unculled query on the first `--unculled-rays` nodes
beside cast_rays(cull=False) on the same rays, mesh and workspace, for the time per (ray, face) pair of either; the whole unculled
voxelisation `--unculled-reps` times; and a torch composition of the same rule on a slice of `--slice-rays` x `--slice-faces`, scaled
to the whole by the number of pairs."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))
sys.path.insert(0, ROOT)

from npcd.eval.mesh import PATCH_ACROSS, PATCH_BLOCK, patch_order, voxelize_mesh  # noqa: E402
from npcd.hip.crossings import count_crossings  # noqa: E402
from npcd.hip.isosurface import isosurface  # noqa: E402
from npcd.hip.mesh_distance import TILE_FACES, mesh_boxes  # noqa: E402
from npcd.hip.raycast import WAVE_RAYS, cast_rays  # noqa: E402

DIRECTIONS = {"x": (1.0, 0.0, 0.0), "oblique": (1.0, 2.0, 3.0)}
PATCHES = {"across": PATCH_ACROSS, "block": PATCH_BLOCK}


def sphere_volume(G):
    axis = torch.linspace(-1, 1, G, device="cuda")
    z, y, x = torch.meshgrid(axis, axis, axis, indexing="ij")
    return (0.75 - torch.sqrt((x - 0.013) ** 2 + (y + 0.021) ** 2 + (z - 0.034) ** 2)).contiguous()


def composition(o, d, v, f):
    """The rule of crossings_reference on every (ray, face) of a slice with torch operators, rays that share one direction d (a
    tuple) -> (front, back): [r, f] temporaries throughout."""
    size = [abs(x) for x in d]
    kz = size.index(max(size))
    kx, ky = (kz + 1) % 3, (kz + 2) % 3
    if d[kz] < 0:
        kx, ky = ky, kx
    dz = torch.tensor(d[kz], dtype=torch.float32, device=o.device)
    Sx, Sy, Sz = torch.tensor(d[kx], device=o.device) / dz, torch.tensor(d[ky], device=o.device) / dz, 1.0 / dz
    p = v[f.long()][None] - o[:, None, None, :]          # [r, f, 3 corners, 3]
    pz = p[..., kz]
    x32, y32 = p[..., kx] - Sx * pz, p[..., ky] - Sy * pz
    x, y, z = x32.double(), y32.double(), (Sz * pz).double()
    U = x[..., 2] * y[..., 1] - y[..., 2] * x[..., 1]
    V = x[..., 0] * y[..., 2] - y[..., 0] * x[..., 2]
    W = x[..., 1] * y[..., 0] - y[..., 1] * x[..., 0]
    det = (U + V) + W
    pos = det > 0

    def owns(E, start, end):
        up = torch.where(pos, y[..., end] > y[..., start], y[..., end] < y[..., start])
        left = torch.where(pos, x[..., end] < x[..., start], x[..., end] > x[..., start])
        return torch.where(pos, E > 0, E < 0) | ((E == 0) & (up | ((y[..., end] == y[..., start]) & left)))
    t = (((U * z[..., 0] + V * z[..., 1]) + W * z[..., 2]) / det).float()
    counted = (det != 0) & owns(U, 2, 1) & owns(V, 0, 2) & owns(W, 1, 0) & (t >= 0) & (t < float("inf"))
    return (counted & pos).sum(dim=1, dtype=torch.int32), (counted & ~pos).sum(dim=1, dtype=torch.int32)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--unculled-rays", type=int, default=131072)
    ap.add_argument("--unculled-reps", type=int, default=1)
    ap.add_argument("--slice-rays", type=int, default=2048)
    ap.add_argument("--slice-faces", type=int, default=8192)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_crossings needs a GPU: a time taken anywhere else says nothing")
    G, N = args.resolution, args.nodes
    step = 2.0 / (G - 1)
    (v, f), = isosurface(sphere_volume(G), 0.0, (-1.0, -1.0, -1.0), (step, step, step))
    V, F, R = v.shape[0], f.shape[0], N ** 3
    boxes = mesh_boxes(v, f)
    origin, spacing = (-1.0 + 0.37 / N,) * 3, (2.0 / N,) * 3          # off the volume's own lattice: no node on a vertex
    o32, s32 = torch.tensor(origin, device="cuda"), torch.tensor(spacing, device="cuda")
    nodes = {}
    for name, patch in PATCHES.items():
        order = patch_order((N, N, N), patch, "cuda")
        row = order // N
        nodes[name] = (o32 + s32 * torch.stack([order - row * N, row % N, row // N], dim=1).float()).contiguous()
    rays = {k: torch.tensor(d, device="cuda").expand(R, 3).contiguous() for k, d in DIRECTIONS.items()}
    few = args.unculled_rays
    legs = {f"culled_{dk}_{pk}": (lambda dk=dk, pk=pk: count_crossings(nodes[pk], rays[dk], v, f, boxes=boxes)) for dk in DIRECTIONS for pk in PATCHES}
    legs["voxelize_mesh_call"] = lambda: voxelize_mesh((v, f), origin, spacing, (N, N, N))
    legs["unculled_crossings_part"] = lambda: count_crossings(nodes["across"][:few], rays["x"][:few], v, f, cull=False, boxes=boxes)
    legs["unculled_first_hit_part"] = lambda: cast_rays(nodes["across"][:few], rays["x"][:few], v, f, cull=False, boxes=boxes)
    legs["composition_slice"] = lambda: composition(nodes["across"][:args.slice_rays], DIRECTIONS["x"], v, f[:args.slice_faces])
    waves, tiles = -(-R // WAVE_RAYS), -(-F // TILE_FACES)
    for run in range(args.runs):
        stats = {f"{name}_ms_median_min_max": t for name, t in timed(legs, args.warmup, args.reps).items()}
        median = lambda name: stats[f"{name}_ms_median_min_max"][0]
        whole = timed({"unculled_whole": lambda: count_crossings(nodes["across"], rays["x"], v, f, cull=False, boxes=boxes)}, 0, args.unculled_reps) if args.unculled_reps else {}
        stats.update({f"{name}_ms_median_min_max": t for name, t in whole.items()})
        inside = {}
        for dk in DIRECTIONS:
            for pk in PATCHES:
                got = count_crossings(nodes[pk], rays[dk], v, f, stats=True, boxes=boxes)
                stats[f"evaluated_{dk}_{pk}"] = int(got["evaluated"])
                stats[f"evaluated_share_{dk}_{pk}"] = round(int(got["evaluated"]) / (waves * tiles), 5)
                inside[dk, pk] = ((got["front"] + got["back"]) & 1).bool()
                stats[f"signed_is_parity_{dk}_{pk}"] = bool(torch.equal((got["back"] - got["front"]) == 1, inside[dk, pk])) and int((got["back"] - got["front"]).abs().max()) <= 1
        back = torch.empty(R, dtype=torch.bool, device="cuda")
        back[patch_order((N, N, N), PATCHES["block"], "cuda")] = inside["x", "block"]
        across = torch.empty(R, dtype=torch.bool, device="cuda")
        across[patch_order((N, N, N), PATCHES["across"], "cuda")] = inside["x", "across"]
        plain = count_crossings(nodes["across"][:few], rays["x"][:few], v, f, cull=False, boxes=boxes)
        culled = count_crossings(nodes["across"][:few], rays["x"][:few], v, f, boxes=boxes)
        theirs = composition(nodes["across"][:args.slice_rays], DIRECTIONS["x"], v, f[:args.slice_faces])
        ours = count_crossings(nodes["across"][:args.slice_rays], rays["x"][:args.slice_rays], v, f[:args.slice_faces].contiguous(), cull=False)
        pairs_part, pairs = few * F, R * F
        scale = pairs / (args.slice_rays * args.slice_faces)
        stats.update({
            "gpu": torch.cuda.get_device_name(0), "run": run, "vertices": V, "faces": F, "rays": R, "waves_x_tiles": waves * tiles,
            "inside_nodes": int(across.sum()), "inside_share": round(float(across.float().mean()), 5),
            "sphere_share_analytic": round(4.0 / 3.0 * 3.141592653589793 * 0.75 ** 3 / 8.0, 5),
            "orders_and_directions_agree": all(bool(torch.equal(inside["x", pk].sum(), inside[dk, pk].sum())) for dk in DIRECTIONS for pk in PATCHES) and bool(torch.equal(back, across)),
            "culled_equals_unculled_counts": all(bool(torch.equal(plain[k], culled[k])) for k in ("front", "back")),
            "composition_slice_equals_kernel": bool(torch.equal(theirs[0], ours["front"])) and bool(torch.equal(theirs[1], ours["back"])),
            "unculled_ps_per_pair_crossings": round(median("unculled_crossings_part") * 1e9 / pairs_part, 4),
            "unculled_ps_per_pair_first_hit": round(median("unculled_first_hit_part") * 1e9 / pairs_part, 4),
            "unculled_crossings_over_first_hit": round(median("unculled_crossings_part") / median("unculled_first_hit_part"), 4),
            "composition_scaled_ms": round(median("composition_slice") * scale, 1),
            "composition_scaled_over_culled_x_across": round(median("composition_slice") * scale / median("culled_x_across"), 1),
            "composition_scaled_over_unculled": round(median("composition_slice") * scale / (median("unculled_crossings_part") * R / few), 1),
        })
        print(json.dumps(stats), flush=True)


if __name__ == "__main__":
    main()
