#!/usr/bin/env python3
"""Precision / recall / density / coverage on the feature k-NN kernels (csrc/feature_manifold.hip) against what a
user could do without them on the same GPU in the same process, through torch's library.  HIP events, warm-up calls per leg, the legs
alternating inside every repetition, median with min-max; one JSON line per size.

    python tools/probes/feature_manifold_timing.py [--rows 16064,50000] [--reps 7]

  hip       everything behind DeviceFIDKID.summary(prdc=True): two knn_sq_distances launches for the radii, two ball_counts
            launches with the roles swapped, the device reduction to four doubles
  library   the same four numbers: both sides .double() once, row blocks of 4,096, (nx + ny) - 2 Xb @ Y^T in float64, then
            topk / compare / sum / min on the block

D = 2,048 fp32 features, k = 5.  The float64 matrix rate is what the kernels' own products imply: 2 n m D for each of the four passes,
n and m rounded up to whole tiles, over the time of the whole leg (norms, merges and the reduction included).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools", "probes"))

from npcd.utils import fidkid  # noqa: E402
from feature_stats_timing import timed_alternating  # noqa: E402

BLOCK = 4096


def library_prdc(real, fake, k):
    """-> float64 [4] on the device: precision, recall, density, coverage."""
    rd, fd = real.double(), fake.double()
    nr, nf = (rd * rd).sum(1), (fd * fd).sum(1)

    def blocks(x, nx, y, ny):
        for i0 in range(0, x.shape[0], BLOCK):
            yield i0, ((nx[i0:i0 + BLOCK, None] + ny[None, :]) - 2 * (x[i0:i0 + BLOCK] @ y.T)).clamp_min_(0)

    def radii(x, nx):
        rho = torch.empty_like(nx)
        for i0, d2 in blocks(x, nx, x, nx):
            rows = torch.arange(d2.shape[0], device=d2.device)
            d2[rows, i0 + rows] = float("inf")
            rho[i0:i0 + d2.shape[0]] = torch.topk(d2, k, dim=1, largest=False).values[:, k - 1]
        return rho

    rho_r, rho_f = radii(rd, nr), radii(fd, nf)
    zero = torch.zeros((), dtype=torch.int64, device=real.device)
    in_balls, fake_inside, real_inside, covered = zero, zero, zero, zero
    for _, d2 in blocks(fd, nf, rd, nr):
        c = (d2 < rho_r[None, :]).sum(1)
        in_balls, fake_inside = in_balls + c.sum(), fake_inside + (c > 0).sum()
    for i0, d2 in blocks(rd, nr, fd, nf):
        real_inside = real_inside + ((d2 < rho_f[None, :]).sum(1) > 0).sum()
        covered = covered + (d2.min(1).values < rho_r[i0:i0 + d2.shape[0]]).sum()
    N, M = rd.shape[0], fd.shape[0]
    return torch.stack([fake_inside, real_inside, in_balls, covered]).double() / torch.tensor([M, N, k * M, N], dtype=torch.float64,
                                                                                             device=real.device)


def leg(dev, n, reps, warmup):
    D, k, tile = 2048, 5, 64
    g = torch.Generator(device=dev).manual_seed(n)
    real = torch.randn(n, D, device=dev, generator=g)
    fake = torch.randn(n, D, device=dev, generator=g) * 1.05 + 0.02
    metric = fidkid.DeviceFIDKID(num_images=n, device=dev, prdc=True, nearest_k=k)
    peak = {}
    for name, fn in (("hip", lambda: metric._prdc_on_device(real, fake)), ("library", lambda: library_prdc(real, fake, k))):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)
    t = timed_alternating({"hip": lambda: metric._prdc_on_device(real, fake), "library": lambda: library_prdc(real, fake, k)}, warmup, reps)
    got, want = metric._prdc_on_device(real, fake).cpu().tolist(), library_prdc(real, fake, k).cpu().tolist()
    padded = -(-n // tile) * tile
    flop = 4 * 2.0 * padded * padded * D
    spread = (t["hip"][2] - t["hip"][1]) + (t["library"][2] - t["library"][1])
    return {"rows_per_side": n, "D": D, "dtype": "fp32", "nearest_k": k, "hip_ms_median_min_max": t["hip"],
            "library_ms_median_min_max": t["library"], "library_over_hip": round(t["library"][0] / t["hip"][0], 3),
            "hip_minus_library_ms": round(t["hip"][0] - t["library"][0], 3), "min_max_spread_of_both_ms": round(spread, 3),
            "hip_flop_issued": flop, "hip_fp64_matrix_tflops": round(flop / (t["hip"][0] * 1e-3) / 1e12, 2),
            "library_tflops_on_4x2nmD": round(4 * 2.0 * n * n * D / (t["library"][0] * 1e-3) / 1e12, 2),
            "hip_peak_memory_gib_above_the_features": peak["hip"], "library_peak_memory_gib_above_the_features": peak["library"],
            "hip": got, "library": want}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="16064,50000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feature_manifold_timing needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    for n in (int(r) for r in args.rows.split(",")):
        torch.cuda.empty_cache()
        result = leg(dev, n, args.reps, args.warmup)
        print(json.dumps({"gpu": name, **result}), flush=True)


if __name__ == "__main__":
    main()
