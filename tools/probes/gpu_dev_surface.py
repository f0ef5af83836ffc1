#!/usr/bin/env python3
"""Surface sampling of meshes (csrc/surface.hip) beside the torch composition it replaces, on isosurfaces of bumpy
spheres made on the GPU (npcd.hip.isosurface): `--batch` meshes of about 2 x 10^5 faces with S = 2,048 samples each, and one mesh of
about 10^6 faces.  HIP events, `--warmup` rounds first, then `--reps` rounds in which the legs alternate; median with min-max; one
JSON line per size.

    python tools/probes/gpu_dev_surface.py [--batch 64] [--resolution 116] [--large 260] [--samples 2048] [--reps 7] [--warmup 2]

Legs: prepare (npcd_surface_prepare on buffers made beforehand: a memset and three launches) and sample (npcd_surface_sample, one
launch) alone, sample_surface() as the caller sees it (packing the batch, the offsets, the workspace, both entry points), and the
torch composition on the same box: the meshes padded to one [B, Fmax] batch, float64 areas of the gathered corners, cumsum,
searchsorted of u0 times the total, the gathers of the chosen faces' corners and the square root -- every step one or a few torch
launches on the whole batch.  The bytes prepare must move at least are 28 a face (12 of indices read, 4 of d written and read again,
8 of prefix sums written) and 12 a vertex, held against the 6.29 TB/s a copy reaches on this chip."""
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
from npcd.hip.surface import _Packed, sample_surface  # noqa: E402

COPY_TB_PER_S = 6.29


def bumpy_sphere(G, seed):
    """A sphere of radius about 0.75 with a few low-frequency bumps on the G^3 lattice over [-1, 1]^3 -> (vertices, faces)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    axis = torch.linspace(-1, 1, G, device="cuda")
    z, y, x = torch.meshgrid(axis, axis, axis, indexing="ij")
    phase = torch.rand(6, generator=g, device="cuda") * 6.28
    bumps = 0.03 * (torch.sin(7 * x + phase[0]) * torch.sin(5 * y + phase[1]) + torch.sin(6 * z + phase[2]) * torch.sin(4 * x + phase[3]))
    vol = 0.75 + bumps - torch.sqrt(x * x + y * y + z * z)
    step = 2.0 / (G - 1)
    return isosurface(vol, 0.0, (-1.0, -1.0, -1.0), (step, step, step))[0]


def torch_composition(vertices, faces, u):
    """vertices [B, Vmax, 3] fp32, faces [B, Fmax, 3] int64 (padding: the face (0, 0, 0), no area), u [B, S, 3] -> points [B, S, 3]."""
    B, F = faces.shape[:2]
    corners = torch.gather(vertices, 1, faces.reshape(B, -1, 1).expand(-1, -1, 3)).reshape(B, F, 3, 3)
    area = torch.linalg.cross(corners[:, :, 1] - corners[:, :, 0], corners[:, :, 2] - corners[:, :, 0]).double().norm(dim=-1)
    sums = torch.cumsum(area, dim=1)
    face = torch.searchsorted(sums, u[:, :, 0].double() * sums[:, -1:], right=True).clamp(max=F - 1)
    picked = torch.gather(corners.reshape(B, F, 9), 1, face[:, :, None].expand(-1, -1, 9)).reshape(B, -1, 3, 3)
    s = torch.sqrt(u[:, :, 1])
    b0, b1, b2 = 1 - s, s * (1 - u[:, :, 2]), s * u[:, :, 2]
    return b0[..., None] * picked[:, :, 0] + b1[..., None] * picked[:, :, 1] + b2[..., None] * picked[:, :, 2], face


def measure(meshes, S, warmup, reps):
    L, P = hip.lib(), hip.ptr
    B = len(meshes)
    packed = _Packed(meshes, "gpu_dev_surface")
    area = packed.prepare()
    u = torch.rand((B, S, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    points = torch.empty((B, S, 3), device="cuda")
    Vmax, Fmax = max(packed.V), max(packed.F)
    padded_v = torch.zeros((B, Vmax, 3), device="cuda")
    padded_f = torch.zeros((B, Fmax, 3), dtype=torch.int64, device="cuda")
    for b, (v, f) in enumerate(meshes):
        padded_v[b, :len(v)], padded_f[b, :len(f)] = v, f

    def prepare():
        hip.check(L.npcd_surface_prepare(P(packed.vertices), P(packed.faces), P(packed.offsets[0]), P(packed.offsets[1]), B, packed.V_total,
                                         packed.F_total, P(packed.ws), P(area), hip.stream_ptr()), "prepare")

    def sample():
        hip.check(L.npcd_surface_sample(P(packed.vertices), P(packed.faces), P(packed.offsets[0]), P(packed.offsets[1]), B, packed.V_total,
                                        packed.F_total, P(packed.ws), P(u), S, P(points), None, 0, None, None, None, 0, None, hip.stream_ptr()), "sample")
    legs = {"prepare": prepare, "sample": sample, "sample_surface_call": lambda: sample_surface(meshes, S, u=u),
            "torch_composition": lambda: torch_composition(padded_v, padded_f, u)}
    times = {k: [] for k in legs}
    for r in range(warmup + reps):
        for name, fn in legs.items():          # the legs alternate inside every round
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(a.elapsed_time(b))
    stats = {f"{k}_ms_median_min_max": [round(sorted(t)[len(t) // 2], 4), round(min(t), 4), round(max(t), 4)] for k, t in times.items()}
    # what the two agree on: the composition picks faces from a float64 scan, the kernels from integer sums -- the same face for nearly
    # every draw, and the same areas to float32 accuracy
    own_points, own_area, own_face = sample_surface(meshes, S, u=u, return_faces=True)
    ref_points, ref_face = torch_composition(padded_v, padded_f, u)
    ours = stats["prepare_ms_median_min_max"][0] + stats["sample_ms_median_min_max"][0]
    nbytes = 28 * packed.F_total + 12 * packed.V_total
    stats.update({
        "gpu": torch.cuda.get_device_name(0), "meshes": B, "samples": S, "faces_total": packed.F_total, "faces_min_max": [min(packed.F), max(packed.F)],
        "vertices_total": packed.V_total, "prepare_plus_sample_ms": round(ours, 4),
        "composition_over_prepare_plus_sample": round(stats["torch_composition_ms_median_min_max"][0] / ours, 2),
        "prepare_min_bytes": nbytes, "prepare_GB_per_s": round(nbytes / (stats["prepare_ms_median_min_max"][0] * 1e-3) / 1e9, 1),
        "prepare_share_of_copy_rate": round(nbytes / (stats["prepare_ms_median_min_max"][0] * 1e-3) / (COPY_TB_PER_S * 1e12), 4),
        "same_face_as_the_composition": round(float((own_face == ref_face).double().mean()), 6),
        "max_point_difference_where_the_face_is_the_same": float(((own_points - ref_points).abs().amax(-1) * (own_face == ref_face)).max()),
        "area_first_mesh": float(own_area[0]),
    })
    print(json.dumps(stats), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--resolution", type=int, default=116)
    ap.add_argument("--large", type=int, default=260)
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_surface needs a GPU: a time taken anywhere else says nothing")
    if args.batch > 0:
        measure([bumpy_sphere(args.resolution, seed) for seed in range(args.batch)], args.samples, args.warmup, args.reps)
    if args.large > 0:
        measure([bumpy_sphere(args.large, 1000)], args.samples, args.warmup, args.reps)


if __name__ == "__main__":
    main()
