#!/usr/bin/env python3
"""All-pairs Chamfer matrix: the HIP kernel (csrc/chamfer.hip) against what a user could do without it on the same GPU in the same
process -- a loop of torch.cdist(..., compute_mode="donot_use_mm_for_euclid_dist") ** 2 -> min -> mean over chunks of cloud pairs
(the exact form, like for like; 2^23 distances per call, the most that mode's launch takes safely) -- and against torch.cdist's
default mode (the norm-expansion form on the matrix library; 1 GiB of distances per call), with its error.  HIP events, two warm-up
calls per leg, the legs alternating, median with min-max; one JSON line per case.

    python tools/probes/chamfer_probe.py [--cases a,b,c] [--reps 7] [--baseline-rows R]

  (a) the self-matrix of 2,000 clouds of 512 points   (the evaluation size: 1,000 generated + 1,000 reference clouds)
  (b) 256 x 256 clouds of 2,048 points
  (c) 64 x 64 clouds of 4,096 points

--baseline-rows R: the torch legs, and a kernel leg beside them, run on the first R X clouds against all Y clouds (0 = all rows).
The torch loops take minutes per pass at these sizes; the comparison is then made on that slice, kernel and torch on the same rows,
and the kernel's time on the whole case is reported next to it.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))

from npcd.hip.chamfer import chamfer_directed  # noqa: E402

# MI355X fp32 vector peak: 157.3 TFLOP/s, counting a fused multiply-add as two.  The kernel's subtractions, multiplications, additions
# and minima are one operation per lane each (the spec forbids contraction), so its ceiling is half of that in lane-operations.
PEAK_LANE_OPS = 157.3e12 / 2
CHUNK_DISTS = (1 << 30) // 4          # distances per torch.cdist call: 1 GiB of fp32
# torch's exact mode launches one 256-thread workgroup per distance and the launch is refused ("invalid configuration argument") once
# the grid passes 2^32 threads: 2^23 distances per call stay below that with room to spare
EXACT_CHUNK_DISTS = 1 << 23


def torch_loop(x, y, mode, max_dists):
    """Directed Chamfer matrix on torch operators: squared cdist of a chunk of cloud pairs (of a slice of x's points where one pair
    alone exceeds `max_dists`), min over y's points, sum over x's points, divided by their number."""
    (M, P, _), (N, Q, _) = x.shape, y.shape
    points = min(P, max(1, max_dists // Q))
    pairs = max(1, max_dists // (points * Q))
    rows, cols = max(1, pairs // N), min(N, pairs)
    out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    for i0 in range(0, M, rows):
        for j0 in range(0, N, cols):
            acc = None
            for p0 in range(0, P, points):
                d = torch.cdist(x[i0:i0 + rows, None, p0:p0 + points], y[None, j0:j0 + cols], compute_mode=mode) ** 2
                part = d.min(dim=3).values.sum(dim=2)          # d: [rows, cols, points, Q]
                acc = part if acc is None else acc + part
                del d
            out[i0:i0 + rows, j0:j0 + cols] = acc / P
    return out


def timed_alternating(legs, warmup, reps):
    """legs: {name: fn}.  -> {name: (median ms, min, max, last output)}; the legs take turns inside every repetition."""
    out, times = {}, {k: [] for k in legs}
    for k, fn in legs.items():
        for _ in range(warmup):
            out[k] = fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out[k] = fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (sorted(t)[len(t) // 2], min(t), max(t), out[k]) for k, t in times.items()}


def rel_diff(a, b):
    a, b = a.double(), b.double()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300))[b != 0].max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-rows", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("chamfer_probe needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    shapes = {"a": (2000, 512, None, None), "b": (256, 2048, 256, 2048), "c": (64, 4096, 64, 4096)}
    for case in args.cases.split(","):
        M, P, N, Q = shapes[case]
        g = torch.Generator().manual_seed(M + P)
        x = torch.randn(M, P, 3, generator=g).to(dev)
        y = x if N is None else torch.randn(N, Q, 3, generator=g).to(dev)
        N, Q = y.shape[0], y.shape[1]
        whole = timed_alternating({"hip": (lambda: chamfer_directed(x) if y is x else chamfer_directed(x, y))}, 2, args.reps)["hip"]
        R = min(M, args.baseline_rows) if args.baseline_rows > 0 else M
        xs = x[:R].contiguous()
        legs = timed_alternating({"hip": lambda: chamfer_directed(xs, y),
                                  "exact": lambda: torch_loop(xs, y, "donot_use_mm_for_euclid_dist", EXACT_CHUNK_DISTS),
                                  "default": lambda: torch_loop(xs, y, "use_mm_for_euclid_dist_if_necessary", CHUNK_DISTS)},
                                 2, args.reps)
        pairs = M * N * P * Q
        rnd = lambda t: [round(t[0], 3), round(t[1], 3), round(t[2], 3)]
        print(json.dumps({
            "case": case, "gpu": name, "x": [M, P], "y": [N, Q], "self_matrix": y is x, "point_pairs": pairs, "lane_ops": 9 * pairs,
            "hip_ms_median_min_max": rnd(whole),
            "hip_lane_ops_per_s": round(9 * pairs / (whole[0] * 1e-3), 0),
            "hip_share_of_fp32_vector_peak_in_lane_ops": round(9 * pairs / (whole[0] * 1e-3) / PEAK_LANE_OPS, 4),
            "peak_meant": "157.3 TFLOP/s fp32 vector (spec), an FMA counted as two: 78.65e12 non-fused lane-operations per second",
            "baseline_rows": R,
            "rows_hip_ms_median_min_max": rnd(legs["hip"]),
            "rows_torch_exact_ms_median_min_max": rnd(legs["exact"]),
            "rows_torch_default_ms_median_min_max": rnd(legs["default"]),
            "torch_exact_over_hip": round(legs["exact"][0] / legs["hip"][0], 2),
            "torch_default_over_hip": round(legs["default"][0] / legs["hip"][0], 2),
            "rows_equal_whole_bitwise": bool(torch.equal(legs["hip"][3], whole[3][:R])),
            "max_rel_diff_hip_vs_torch_exact": rel_diff(legs["hip"][3], legs["exact"][3]),
            "max_rel_diff_torch_default_vs_hip": rel_diff(legs["default"][3], legs["hip"][3]),
        }), flush=True)


if __name__ == "__main__":
    main()
