#!/usr/bin/env python3
"""Farthest point sampling: the HIP kernel (csrc/fps.hip) against the same algorithm written as a loop of torch operators on the same
GPU -- what a user could do without the kernel.  Timed with HIP events after a warm-up; one JSON line per case.

    python tools/probes/fps_probe.py [--reps 5]

  (a) 64 clouds of 30,000 points to K = 512      (a dataset batch: one workgroup per cloud, streamed coordinates)
  (b) one cloud of 100,000 points to K = 512     (the largest form: one workgroup streams 1.2 MB from L2 at every pick)
  (c) 64 clouds of 8,192 points to K = 512       (the resident form: nothing but the winner's row is read after the first pick)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))

from npcd.hip.fps import sample_farthest_points  # noqa: E402


def torch_loop(points, K):
    """The spec of DESIGN.md 5.6 on torch operators, every cloud of the batch at once: seven launches per pick."""
    N, P, _ = points.shape
    rows = torch.arange(N, device=points.device)
    md = torch.full((N, P), float("inf"), device=points.device)
    cur = torch.zeros(N, dtype=torch.int64, device=points.device)
    idx = torch.empty((N, K), dtype=torch.int64, device=points.device)
    for k in range(K):
        idx[:, k] = cur
        diff = points - points[rows, cur][:, None]
        sq = diff * diff
        md = torch.minimum(md, (sq[..., 0] + sq[..., 1]) + sq[..., 2])
        cur = md.argmax(dim=1)
    return idx


def timed(fn, warmup, reps):
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
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fps_probe needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    for case, N, P, K in (("a", 64, 30000, 512), ("b", 1, 100000, 512), ("c", 64, 8192, 512)):
        g = torch.Generator().manual_seed(N)
        points = (torch.randn(N, P, 3, generator=g) * 0.3).to(dev)
        hip_ms, hip_lo, hip_hi, (_, idx) = timed(lambda: sample_farthest_points(points, K=K), 2, args.reps)
        ref_ms, ref_lo, ref_hi, ref_idx = timed(lambda: torch_loop(points, K), 1, max(2, args.reps // 2))
        # the streaming forms read every coordinate of every cloud once per update; the resident form (c) reads them once in all
        streamed = (K - 1) * N * P * 12 if P > 16384 else N * P * 12
        print(json.dumps({
            "case": case, "gpu": name, "clouds": N, "points": P, "K": K,
            "hip_ms": round(hip_ms, 3), "hip_ms_min_max": [round(hip_lo, 3), round(hip_hi, 3)],
            "torch_loop_ms": round(ref_ms, 3), "torch_loop_ms_min_max": [round(ref_lo, 3), round(ref_hi, 3)],
            "torch_over_hip": round(ref_ms / hip_ms, 2),
            "hip_us_per_pick": round(hip_ms * 1e3 / K, 3), "torch_us_per_pick": round(ref_ms * 1e3 / K, 3),
            "hip_coordinate_read_GBps_per_workgroup": round(streamed / N / (hip_ms * 1e-3) / 1e9, 1),
            "indices_equal_torch_loop": bool(torch.equal(idx, ref_idx)),
        }), flush=True)


if __name__ == "__main__":
    main()
