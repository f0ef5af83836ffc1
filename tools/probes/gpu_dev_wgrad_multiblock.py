"""Dev probe (round 18): the weight gradients of FOUR residual blocks as one grouped launch (ew.wgrad_group with 16 products: 768 tiles of
256 x 256 = three rounds of 256 CUs, one workgroup per tile over all token rows) against today's path, fused._wgrad per product (the
library's token-sliced batched GEMM + the slab sum), at the token count of the benchmark step.  bf16, width 1,024.  The operand sets
rotate (>= 3 sets of sixteen (dy, x) pairs, ~4.3 GB each) so that nothing stays in the Infinity Cache from one timing to the next; the
two forms alternate in one process, each bracketed by its own pair of events.  Also timed: one block per launch (4 products, 192 tiles).
usage: python3 tools/probes/gpu_dev_wgrad_multiblock.py [T [sets [reps]]]"""
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "neural-point-cloud-diffusion_amd"))
import torch  # noqa: E402

from npcd.hip import elementwise as ew  # noqa: E402
from npcd.models.diffusion import fused  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 32832
SETS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 6
W, BLOCKS = 1024, 4
SHAPES = (("c_qkv", 3 * W, W), ("attn.c_proj", W, W), ("c_fc", 4 * W, W), ("mlp.c_proj", W, 4 * W))
assert SETS >= 3
assert torch.cuda.is_available(), "this probe measures on the GPU"
print(f"T = {T}, {SETS} operand sets of {BLOCKS} blocks, {REPS} rounds; npcd_wgrad_group_blocks -> "
      f"{ew.wgrad_group_blocks([(n, k) for _, n, k in SHAPES])} blocks per launch on {torch.cuda.get_device_properties(0).multi_processor_count} CUs",
      flush=True)


def make_set(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    trip = []
    for _ in range(BLOCKS):
        for _, N, K in SHAPES:
            dy = torch.randn(T, N, device="cuda", generator=g).bfloat16()
            x = torch.randn(T, K, device="cuda", generator=g).bfloat16()
            trip.append((dy, x, torch.empty(N, K, device="cuda")))
    return trip


sets = [make_set(s) for s in range(SETS)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def grouped(trip):
    assert ew.wgrad_group(trip)


def per_block(trip):
    for b in range(BLOCKS):
        assert ew.wgrad_group(trip[4 * b:4 * b + 4])


def library(trip):
    for dy, x, out in trip:
        fused._wgrad(dy, x, out)


# agreement of the two forms on one set (two fp32 summation orders over the same operands)
grouped(sets[0])
mine = [t[2].clone() for t in sets[0]]
library(sets[0])
torch.cuda.synchronize()
worst = max(float((a - t[2]).abs().max() / t[2].abs().max()) for a, t in zip(mine, sets[0]))
print(f"grouped vs library, worst max-abs difference over 16 products: {worst:.2e} of the largest entry", flush=True)
del mine

forms = (("grouped 16", grouped), ("library", library), ("grouped 4 x 4", per_block))
for name, fn in forms:                          # warm-up: code objects, library solution choice, the slab allocations
    for trip in sets:
        fn(trip)
torch.cuda.synchronize()
times = {name: [] for name, _ in forms}
for r in range(REPS):
    for i in range(SETS):
        for j, (name, fn) in enumerate(forms):
            times[name].append(timed(lambda: fn(sets[(i + j) % SETS])))      # (the set a form just read is never the next one's)
flop = sum(2 * T * N * K for _, N, K in SHAPES)
for name, _ in forms:
    v = sorted(times[name])
    mn, med, mx = v[0] / BLOCKS, statistics.median(v) / BLOCKS, v[-1] / BLOCKS
    print(f"{name:14s} per block: min {mn:7.1f} us  median {med:7.1f} us  max {mx:7.1f} us   ({flop / med / 1e6:5.0f} TF/s at the median, "
          f"{len(v)} timings)", flush=True)
a, b = statistics.median(times["grouped 16"]) / BLOCKS, statistics.median(times["library"]) / BLOCKS
print(f"per block, median: grouped {a:.1f} us, library {b:.1f} us, difference {b - a:+.1f} us ({(b - a) * 24 / 1e3:+.2f} ms per 24-block step)")
