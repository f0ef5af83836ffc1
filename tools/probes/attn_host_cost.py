"""Dev probe: host cost of one attention forward + backward (with the column-sum by-product) through npcd.hip.attention.

    python tools/probes/attn_host_cost.py [--tree DIR] [--calls N]

bf16, B = 1, n = 64, H = 1: the kernels take a few microseconds, so the wall time of N back-to-back `_fwd` + `_bwd` pairs with one
synchronisation at the end is the Python / ctypes / launch cost of the pair.  --tree names a checkout (its
neural-point-cloud-diffusion_amd/ is imported, with the library built in it), so that two commits can be run alternately, one
process per round.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--calls", type=int, default=4000)
opt = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.abspath(opt.tree), "neural-point-cloud-diffusion_amd"))
import torch
from npcd.hip import attention as A, lib

B, n, H, d = 1, 64, 1, 64
qkv = torch.randn(B, n, H, 3 * d, device="cuda").bfloat16()
dout = torch.randn(B, n, H, d, device="cuda").bfloat16()
g = torch.empty_like(qkv)
q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
dq, dk, dv = g[..., :d], g[..., d:2 * d], g[..., 2 * d:]
part, _ = A.colsum_part_for(dq)


def pairs(count):
    for _ in range(count):
        out, lse = A._fwd(q, k, v, 0.125)
        A._bwd(q, k, v, out, dout, lse, dq, dk, dv, 0.125, colsum_part=part)


pairs(opt.calls // 10)
torch.cuda.synchronize()
t0 = time.perf_counter()
pairs(opt.calls)
host = time.perf_counter() - t0          # the launches are asynchronous: what the host spent issuing them
torch.cuda.synchronize()
total = time.perf_counter() - t0
print(json.dumps({"tree": opt.tree, "abi": lib().npcd_abi_version(), "calls": opt.calls,
                  "issue_us_per_pair": round(host / opt.calls * 1e6, 2), "us_per_pair": round(total / opt.calls * 1e6, 2)}))
