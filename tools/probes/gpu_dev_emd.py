#!/usr/bin/env python3
"""All-pairs approximate earth mover's distance: the HIP kernel (csrc/emd.hip) against what a user could do without it
on the same GPU in the same process -- the same spec written as batched torch operators on [B, P, Q] temporaries, at the largest
batch of cloud pairs that fits `--torch-gib` of temporaries, its time scaled to the case's full pair count.  HIP events, one warm-up
call per leg, median with min-max; one JSON line per case.

    python tools/probes/gpu_dev_emd.py [--cases a,b] [--reps 3] [--torch-gib 8]

  (a) the union matrix of 1,000 + 1,000 clouds of 512 points   (the evaluation size; one launch, 4 x 10^6 directed pairs)
  (b) 64 x 64 clouds of 2,048 points

The arithmetic estimate printed beside the times is the issue's: per point pair and pass 11 lane-operations and one exponential;
2.4 GHz x 256 compute units x 128 lanes = 78.6e12 lane-operations per second; the exponential at quarter rate (4 more slots) and,
as MI355X's measured issue costs have it (8 cycles against 4), at half rate (1 more slot).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))

from npcd.hip.emd import emd_directed  # noqa: E402

PEAK_LANE_OPS = 2.4e9 * 256 * 128
LEVELS = [-(4.0 ** e) for e in range(7, -2, -1)] + [0.0]
PASSES = 3 * len(LEVELS)
TEMPORARIES = 6          # [B, P, Q] fp32 tensors alive at once in torch_emd: d, root, e, and up to three products


def torch_emd(x, y):
    """The spec of DESIGN.md 5.8 on torch operators: x [B, P, 3], y [B, Q, 3] -> [B], pair b is (x[b], y[b]); all rows valid."""
    P, Q = x.shape[1], y.shape[1]
    T = float(max(P, Q))
    dx, dy, dz = (x[:, :, None, c] - y[:, None, :, c] for c in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    del dx, dy, dz
    root = d.sqrt()
    remain_l = torch.full(x.shape[:2], T / P, dtype=torch.float32, device=x.device)
    remain_r = torch.full(y.shape[:2], T / Q, dtype=torch.float32, device=x.device)
    cost = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
    for level in LEVELS:
        e = torch.exp(level * d)
        ratio_l = remain_l / (1e-9 + (e * remain_r[:, None, :]).sum(dim=2))
        sumr = remain_r * (e * ratio_l[:, :, None]).sum(dim=1)
        ratio_r = torch.clamp(remain_r / (sumr + 1e-9), max=1.0) * remain_r
        remain_r = torch.clamp(remain_r - sumr, min=0.0)
        w = e * ratio_l[:, :, None] * ratio_r[:, None, :]
        del e
        cost = cost + (w * root).sum(dim=(1, 2))
        remain_l = torch.clamp(remain_l - w.sum(dim=2), min=0.0)
        del w
    return cost / T


def timed(fn, warmup, reps):
    """-> (median ms, min, max, last output)"""
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
    return sorted(times)[len(times) // 2], min(times), max(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-gib", type=float, default=8.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gpu_dev_emd needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    shapes = {"a": (2000, 512, None, None), "b": (64, 2048, 64, 2048)}
    for case in args.cases.split(","):
        M, P, N, Q = shapes[case]
        g = torch.Generator().manual_seed(M + P)
        x = torch.randn(M, P, 3, generator=g).to(dev)
        y = x if N is None else torch.randn(N, Q, 3, generator=g).to(dev)
        N, Q = y.shape[0], y.shape[1]
        hip = timed((lambda: emd_directed(x)) if y is x else (lambda: emd_directed(x, y)), 1, args.reps)
        # the torch form on the first B pairs of row 0 and onwards, row-major: pair b = (x[b // N], y[b % N])
        B = max(1, min(M * N, int(args.torch_gib * 2 ** 30 / (TEMPORARIES * 4 * P * Q))))
        rows = (B + N - 1) // N
        xb = x[:rows].repeat_interleave(N, dim=0)[:B].contiguous()
        yb = y.repeat(rows, 1, 1)[:B].contiguous()
        tor = timed(lambda: torch_emd(xb, yb), 1, args.reps)
        ref = hip[3].reshape(-1)[:B]
        off = xb.ne(yb).flatten(1).any(dim=1)          # a cloud against itself is ~0 in both: no relative quantity
        rel = float(((tor[3] - ref).abs() / ref.abs().clamp_min(1e-30))[off].max())
        evals = M * N * P * Q * PASSES
        plain = 11 * evals / PEAK_LANE_OPS
        scaled = tor[0] * 1e-3 * (M * N) / B
        rnd = lambda t: [round(t[0], 3), round(t[1], 3), round(t[2], 3)]
        print(json.dumps({
            "case": case, "gpu": name, "x": [M, P], "y": [N, Q], "self_matrix": y is x, "directed_pairs": M * N,
            "distance_and_exp_evaluations": evals,
            "hip_ms_median_min_max": rnd(hip),
            "torch_batch_pairs": B, "torch_batch_ms_median_min_max": rnd(tor),
            "torch_seconds_scaled_to_all_pairs": round(scaled, 2),
            "torch_over_hip": round(scaled / (hip[0] * 1e-3), 1),
            "estimate_seconds_plain_valu_11_ops": round(plain, 3),
            "estimate_seconds_with_exp_at_quarter_rate": round(plain + 4 * evals / PEAK_LANE_OPS, 3),
            "estimate_seconds_with_exp_at_half_rate": round(plain + 1 * evals / PEAK_LANE_OPS, 3),
            "plain_valu_estimate_over_hip": round(plain / (hip[0] * 1e-3), 3),
            "max_rel_diff_torch_vs_hip_on_the_batch": rel,
        }), flush=True)


if __name__ == "__main__":
    main()
