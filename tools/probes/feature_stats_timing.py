#!/usr/bin/env python3
"""Feature statistics (csrc/feature_stats.hip) against what a user could do without them on the same GPU in the same
process, through torch's library.  HIP events, warm-up calls per leg, the legs alternating inside every repetition, median with
min-max; one JSON line per leg.

    python tools/probes/feature_stats_timing.py [--legs flush,kid,summary] [--reps 7]

  flush     one moment update over 1,024 x 2,048 fp32 rows   vs   Xd = X.double(); G += Xd.T @ Xd; s += Xd.sum(0)
  kid       kid_subsets at S = 100, m = 1,000, D = 2,048       vs   the three products as torch.bmm on gathered float64 subsets
            (with the cubic kernel and the sums behind them, and the products alone)
  summary   DeviceFIDKID.summary() of 64 clouds x 251 views, D = 2,048 features of a projection extractor, reals fed
            vs FIDKID.summary() on the host (wall clock, once each; both end in the same host frechet_distance, timed on its own)

The float64 matrix rate is what the kernel's own products imply: the multiply-adds it issues (the upper tiles only), counted as two.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "neural-point-cloud-diffusion_amd"))

from npcd.hip import feature_stats as fs  # noqa: E402
from npcd.utils import fidkid  # noqa: E402


def timed_alternating(legs, warmup, reps):
    """legs: {name: fn}.  -> {name: [median ms, min, max]}; the legs take turns inside every repetition."""
    times = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: [round(sorted(t)[len(t) // 2], 4), round(min(t), 4), round(max(t), 4)] for k, t in times.items()}


def leg_flush(dev, reps):
    n, D, T = 1024, 2048, fs.tile()
    x = torch.rand(n, D, device=dev)
    total, gram = torch.zeros(D, dtype=torch.float64, device=dev), torch.zeros(D, D, dtype=torch.float64, device=dev)
    lib_total, lib_gram = torch.zeros_like(total), torch.zeros_like(gram)

    def library():
        xd = x.double()
        lib_gram.addmm_(xd.T, xd)
        lib_total.add_(xd.sum(0))

    t = timed_alternating({"hip": lambda: fs.moments_update(x, 0, n, None, total, gram), "library": library}, 3, reps)
    blocks = -(-D // T)
    flop = 2.0 * n * (blocks * (blocks + 1) // 2) * T * T
    return {"leg": "flush", "rows": n, "D": D, "hip_ms_median_min_max": t["hip"], "library_ms_median_min_max": t["library"],
            "library_over_hip": round(t["library"][0] / t["hip"][0], 3), "hip_flop_issued": flop,
            "hip_fp64_matrix_tflops": round(flop / (t["hip"][0] * 1e-3) / 1e12, 2),
            "library_full_gram_tflops": round(2.0 * n * D * D / (t["library"][0] * 1e-3) / 1e12, 2)}


def leg_kid(dev, reps):
    S, m, D, N, T = 100, 1000, 2048, 16064, fs.kid_tile()
    fake, real = torch.rand(N, D, device=dev), torch.rand(N, D, device=dev)
    g = np.random.RandomState(0)
    idx_f = np.stack([g.choice(N, m, replace=False) for _ in range(S)])
    idx_r = np.stack([g.choice(N, m, replace=False) for _ in range(S)])
    dev_f, dev_r = torch.from_numpy(idx_f).to(dev), torch.from_numpy(idx_r).to(dev)

    def products():
        x, y = fake[dev_f].double(), real[dev_r].double()
        return torch.bmm(x, x.transpose(1, 2)), torch.bmm(y, y.transpose(1, 2)), torch.bmm(x, y.transpose(1, 2))

    def library():
        xx, yy, xy = (((p / D + 1) ** 3) for p in products())
        return torch.stack([xx.sum((1, 2)) - xx.diagonal(dim1=1, dim2=2).sum(1), yy.sum((1, 2)) - yy.diagonal(dim1=1, dim2=2).sum(1),
                            xy.sum((1, 2))], dim=1)

    t = timed_alternating({"hip": lambda: fs.kid_subsets(fake, real, idx_f, idx_r), "library": library, "library_products": products}, 2, reps)
    rel = float(((fs.kid_subsets(fake, real, idx_f, idx_r) - library()).abs() / library()).max())
    tiles = -(-m // T)
    flop = 2.0 * S * (tiles * (tiles + 1) + tiles * tiles) * T * T * D
    return {"leg": "kid", "S": S, "m": m, "D": D, "hip_ms_median_min_max": t["hip"], "library_ms_median_min_max": t["library"],
            "library_products_only_ms_median_min_max": t["library_products"], "library_over_hip": round(t["library"][0] / t["hip"][0], 3),
            "hip_includes": "index upload, workspace, both launches", "hip_flop_issued": flop,
            "hip_fp64_matrix_tflops": round(flop / (t["hip"][0] * 1e-3) / 1e12, 2),
            "library_products_tflops": round(2.0 * S * 3 * m * m * D / (t["library_products"][0] * 1e-3) / 1e12, 2),
            "max_rel_diff_hip_vs_library": rel}


def leg_summary(dev):
    clouds, views, D = 64, 251, 2048
    n = clouds * views
    P = torch.randn(3 * 16 * 16, D, device=dev) / (3 * 16 * 16) ** 0.5
    device_metric = fidkid.DeviceFIDKID(num_images=n, device=dev)
    host_metric = fidkid.FIDKID(num_images=n)
    g = torch.Generator(device=dev).manual_seed(0)
    feed_ms = []
    for mode, gain in (("reals", 1.0), ("fakes", 0.9)):
        for _ in range(clouds):
            images = torch.rand(views, 3, 16, 16, device=dev, generator=g) * gain
            feats = (images.flatten(1) @ P).abs()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            device_metric.feed(feats, mode)
            torch.cuda.synchronize()
            feed_ms.append((time.perf_counter() - t0) * 1e3)
            host_metric.feed(feats, mode)
    out = {"leg": "summary", "rows_per_side": n, "D": D, "subsets": 100, "subset_size": 1000,
           "device_feed_ms_per_chunk_of_251_median": round(sorted(feed_ms)[len(feed_ms) // 2], 3)}
    np.random.seed(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = device_metric.summary()
    out["device_summary_s"] = round(time.perf_counter() - t0, 3)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    idx = np.stack([np.random.choice(n, 1000, replace=False) for _ in range(100)])
    a.record()
    device_metric._moments["fakes"].finalize(), device_metric._moments["reals"].finalize()
    fs.kid_subsets(device_metric._moments["fakes"].features(), device_metric._moments["reals"].features(), idx, idx)
    b.record()
    torch.cuda.synchronize()
    out["device_statistics_alone_ms"] = round(a.elapsed_time(b), 3)
    t0 = time.perf_counter()
    cov = np.asarray(device_metric.real_cov)
    fidkid.frechet_distance(np.zeros(D), cov, np.ones(D), cov)
    out["host_frechet_distance_alone_s"] = round(time.perf_counter() - t0, 3)
    np.random.seed(3)
    t0 = time.perf_counter()
    want = host_metric.summary()
    out["host_summary_s"] = round(time.perf_counter() - t0, 3)
    out["host_over_device"] = round(out["host_summary_s"] / out["device_summary_s"], 2)
    out["device"], out["host"] = got, want
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="flush,kid,summary")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("feature_stats_timing needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    for leg in args.legs.split(","):
        result = {"flush": lambda: leg_flush(dev, args.reps), "kid": lambda: leg_kid(dev, args.reps), "summary": lambda: leg_summary(dev)}[leg]()
        print(json.dumps({"gpu": name, **result}), flush=True)


if __name__ == "__main__":
    main()
