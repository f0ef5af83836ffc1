#!/usr/bin/env python3
"""Rays against meshes (csrc/raycast.hip) beside a torch composition: `--views` views of `--image`^2 pixels, the rays of
npcd.hip.render.ray_gen in 8 x 8 pixel blocks, against the isosurface of a sphere volume on a `--resolution`^3 lattice
(npcd.hip.isosurface) and against its simplification at k = 2 (npcd.hip.simplify): the meshes of R35 and R36.  HIP events, `--warmup`
rounds first, then `--reps` rounds in which the legs alternate, the whole repeated `--runs` times; median with min-max; one JSON line
per mesh and run.

    python tools/probes/gpu_dev_raycast.py [--resolution 256] [--views 8] [--image 128] [--reps 5] [--warmup 1] [--runs 2] [--rates PROGRAM]

Legs: the boxes entry point alone; the query entry point with cull = 1 on the blocked rays and on the rays in row-major order, and with
cull = 0; render_mesh() as the caller sees it; and a torch Moeller-Trumbore (fp32, the first hit by argmin) on a slice of
`--slice-rays` x `--slice-faces` that fits memory, scaled to the whole by the number of pairs.  `evaluated` over waves x tiles says
what culling left.  `--rates` names the program built from tools/probes/valu_rate_probe.hip: its measured fp32 and fp64 issue ceilings
turn the unculled time into a share of either, with `--fp32-ops` and `--fp64-ops` vector operations per pair as counted in the ISA
listing of the pair loop (float64 conversions, comparisons, minima and maxima count as fp64)."""
import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))
sys.path.insert(0, ROOT)

from npcd import hip  # noqa: E402
from npcd.eval.mesh import block_order, render_mesh  # noqa: E402
from npcd.hip.isosurface import isosurface  # noqa: E402
from npcd.hip.mesh_distance import TILE_FACES  # noqa: E402
from npcd.hip.raycast import WAVE_RAYS, cast_rays  # noqa: E402
from npcd.hip.render import ray_gen  # noqa: E402
from npcd.hip.simplify import simplify_mesh  # noqa: E402
from oracle import renderer as orr  # noqa: E402
from tools.probes.gpu_dev_mesh_distance import sphere_volume, timed  # noqa: E402


def composition(o, d, v, f):
    """Moeller and Trumbore on every (ray, face) of a slice with torch operators -> (t, face): [r, f] temporaries throughout."""
    a, b, c = (v[f[:, k].long()][None] for k in range(3))
    o, d = o[:, None], d[:, None]
    dot = lambda u, w: (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]
    e1, e2 = b - a, c - a
    pv = torch.linalg.cross(d.expand(-1, e2.shape[1], -1), e2.expand(d.shape[0], -1, -1))
    det = dot(e1, pv)
    tv = o - a
    u = dot(tv, pv) / det
    qv = torch.linalg.cross(tv, e1.expand(tv.shape[0], -1, -1))
    w = dot(d, qv) / det
    t = dot(e2, qv) / det
    hit = (u >= 0) & (w >= 0) & (u + w <= 1) & (t >= 0)
    return torch.where(hit, t, torch.full_like(t, float("inf"))).min(dim=1)


def cameras(views, image):
    K = orr.srn_intrinsics().clone()
    K[0, 0] = K[1, 1] = 131.25 * image / 128
    K[0, 2] = K[1, 2] = image / 2
    poses = [orr.look_at_pose(360.0 * k / views + 10.0, 25.0 if k % 2 else -15.0) for k in range(views)]
    return torch.stack(poses).cuda(), K[None].repeat(views, 1, 1).cuda()


def measure(label, rays, v, f, args, run, rates):
    L, P = hip.lib(), hip.ptr
    (o, d), (o_rows, d_rows), (extr, intr) = rays["blocked"], rays["rows"], rays["cameras"]
    R, V, F = o.shape[0], v.shape[0], f.shape[0]
    ws = torch.empty(L.npcd_mesh_distance_ws_bytes(V, F) // 8 + 2, dtype=torch.int64, device="cuda")
    out = (torch.empty(R, device="cuda"), torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, 3, device="cuda"),
           torch.empty(R, dtype=torch.int8, device="cuda"))
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")

    def query(origins, directions, cull, count=None):
        hip.check(L.npcd_raycast_query(P(origins), P(directions), R, P(v), V, P(f), F, P(ws), 0.0, float("inf"), cull, P(out[0]), P(out[1]),
                                       P(out[2]), P(out[3]), P(count), hip.stream_ptr()), "query")
    so, sd, sf = o[:args.slice_rays], d[:args.slice_rays], f[:args.slice_faces]
    legs = {"boxes": lambda: hip.check(L.npcd_mesh_distance_boxes(P(v), V, P(f), F, P(ws), hip.stream_ptr()), "boxes"),
            "query_blocked_culled": lambda: query(o, d, 1),
            "query_rows_culled": lambda: query(o_rows, d_rows, 1),
            "query_blocked_unculled": lambda: query(o, d, 0),
            "render_mesh_call": lambda: render_mesh((v, f), extr, intr, args.image, 1.0),
            "composition_slice": lambda: composition(so, sd, v, sf)}
    stats = {f"{name}_ms_median_min_max": t for name, t in timed(legs, args.warmup, args.reps).items()}
    median = lambda name: stats[f"{name}_ms_median_min_max"][0]
    evaluated = {}
    for name, (a, b) in (("blocked", (o, d)), ("rows", (o_rows, d_rows))):
        counter.zero_()
        query(a, b, 1, counter)
        evaluated[name] = int(counter)
    waves, tiles = -(-R // WAVE_RAYS), -(-F // TILE_FACES)
    whole, plain = cast_rays(o, d, v, f), cast_rays(o, d, v, f, cull=False)
    # what the composition finds is compared on the faces that the slice's rays hit, filled up with the first faces
    won = torch.unique(whole["face"][:args.slice_rays].clamp(min=0)).long()[:args.slice_faces]
    seen = torch.cat([f[won], f[:max(0, args.slice_faces - won.shape[0])]])
    theirs = composition(so, sd, v, seen)
    ours = cast_rays(so, sd, v, seen, cull=False)
    pairs = R * F
    scale = pairs / (so.shape[0] * sf.shape[0])
    unculled_s = median("query_blocked_unculled") * 1e-3
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    stats.update({
        "gpu": torch.cuda.get_device_name(0), "run": run, "mesh": label, "rays": R, "vertices": V, "faces": F, "waves_x_tiles": waves * tiles,
        "evaluated_blocked": evaluated["blocked"], "evaluated_rows": evaluated["rows"],
        "evaluated_share_blocked": round(evaluated["blocked"] / (waves * tiles), 5),
        "evaluated_share_rows": round(evaluated["rows"] / (waves * tiles), 5),
        "unculled_over_culled_blocked": round(median("query_blocked_unculled") / median("query_blocked_culled"), 2),
        "unculled_pairs_per_second": round(pairs / unculled_s, 0),
        "composition_scaled_ms": round(median("composition_slice") * scale, 1),
        "composition_scaled_over_culled": round(median("composition_slice") * scale / median("query_blocked_culled"), 1),
        "composition_scaled_over_unculled": round(median("composition_slice") * scale / median("query_blocked_unculled"), 2),
        "composition_scaled_over_render_mesh_call": round(median("composition_slice") * scale / median("render_mesh_call"), 1),
        "culled_equals_unculled_bits": all(bool(torch.equal(bits(whole[k]), bits(plain[k]))) for k in whole),
        "composition_slice_rays_that_hit": int((ours["face"] >= 0).sum()),
        "composition_slice_same_face_share": round(float((theirs[1].int() == ours["face"])[ours["face"] >= 0].float().mean()), 5),
        "rays_that_hit": int((whole["face"] >= 0).sum()),
    })
    if rates:
        stats.update(rates)
        stats["fp64_ops_alone_share_of_unculled_time"] = round(pairs * args.fp64_ops / rates["fp64_lane_ops_per_second"] / unculled_s, 4)
        stats["fp32_ops_alone_share_of_unculled_time"] = round(pairs * args.fp32_ops / rates["fp32_lane_ops_per_second"] / unculled_s, 4)
    print(json.dumps(stats), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--slice-rays", type=int, default=2048)
    ap.add_argument("--slice-faces", type=int, default=8192)
    ap.add_argument("--rates", default=None, help="the program built from tools/probes/valu_rate_probe.hip")
    ap.add_argument("--fp32-ops", type=int, default=40, help="fp32 and select operations per (ray, face) in the pair loop of the ISA listing")
    ap.add_argument("--fp64-ops", type=int, default=26, help="fp64 operations per (ray, face) in the pair loop of the ISA listing")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_raycast needs a GPU: a time taken anywhere else says nothing")
    rates = None
    if args.rates:
        rates = json.loads(subprocess.run([args.rates], capture_output=True, text=True, check=True, timeout=120).stdout.strip().splitlines()[-1])
    G = args.resolution
    step = 2.0 / (G - 1)
    (v, f) = isosurface(sphere_volume(G), 0.0, (-1.0, -1.0, -1.0), (step, step, step))[0]
    small = simplify_mesh(v, f, [2 * step] * 3, origin=(-1.0, -1.0, -1.0), dims=[(G - 1) // 2 + 1] * 3)
    extr, intr = cameras(args.views, args.image)
    o, d, _, _ = ray_gen(extr, intr, args.image, 1.0)
    order = block_order(args.image, o.device)
    rays = {"blocked": (o[:, order].reshape(-1, 3).contiguous(), d[:, order].reshape(-1, 3).contiguous()),
            "rows": (o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()), "cameras": (extr, intr)}
    for run in range(args.runs):
        measure("isosurface", rays, v, f, args, run, rates)
        measure("simplified_k2", rays, small["vertices"], small["faces"], args, run, rates)


if __name__ == "__main__":
    main()
