"""Dev probe (round 21): bodies of the 256 x 256 weight-gradient tile (csrc/gemm.hip, wgrad_tile) against each other in the grouped launch
of the training step -- npcd_wgrad_group with the sixteen (dy, x) pairs of FOUR residual blocks at width 1,024: 768 tiles = three rounds
of 256 CUs, one workgroup per tile over all token rows.  The method is that of gpu_dev_wgrad_multiblock.py: bf16, T = 32,832, three
operand sets in rotation (~4.3 GB each, so nothing stays in the Infinity Cache from one timing to the next), the forms alternate in one
process, every timing sits between its own pair of events, 18 timings per form, min / median / max per block.

A form is one shared object that exports npcd_wgrad_group: the library of the package, or a probe-only build of a copy of gemm.hip
(a candidate body, a diagnostic level of the parent's body) linked with a one-line definition of npcd::set_hip_error.  The FIRST form
is the yardstick: every other form whose name does not contain "diag" must give its sixteen outputs bit for bit, and the gate of
docs/experiments.md R21.1 is "median of the form below the MINIMUM of the first form".

    python tools/probes/gpu_dev_wgrad_pipeline.py [--form NAME=PATH ...] [--T 32832] [--sets 3] [--reps 6] [--screen NAME [--launches 200]]

--screen NAME: after the timings, the race screen on that form: `launches` launches on ONE operand set, every output compared bitwise
with the first launch's, once on an otherwise idle chip and once beside a streaming copy on a second stream that perturbs when the
LDS-DMA of the ring lands.  A value check, a few seconds."""
import argparse
import ctypes
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "neural-point-cloud-diffusion_amd"))
import torch  # noqa: E402

from npcd import hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--form", action="append", default=[], metavar="NAME=PATH")
ap.add_argument("--T", type=int, default=32832)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--screen", default=None, metavar="NAME")
ap.add_argument("--launches", type=int, default=200)
args = ap.parse_args()
T, SETS, REPS = args.T, args.sets, args.reps
W, BLOCKS = 1024, 4
SHAPES = (("c_qkv", 3 * W, W), ("attn.c_proj", W, W), ("c_fc", 4 * W, W), ("mlp.c_proj", W, 4 * W))
assert SETS >= 3
assert torch.cuda.is_available(), "this probe measures on the GPU"

forms = [f.split("=", 1) for f in args.form] or [["shipped", hip.LIB_PATH]]
libs = {}
for name, path in forms:
    L = ctypes.CDLL(os.path.abspath(path))
    L.npcd_wgrad_group.restype = ctypes.c_int
    libs[name] = L
print(f"T = {T}, {SETS} operand sets of {BLOCKS} blocks, {REPS} rounds; forms: {', '.join(n for n, _ in forms)}", flush=True)


def make_set(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    trip = []
    for _ in range(BLOCKS):
        for _, N, K in SHAPES:
            dy = torch.randn(T, N, device="cuda", generator=g).bfloat16()
            x = torch.randn(T, K, device="cuda", generator=g).bfloat16()
            trip.append((dy, x, torch.empty(N, K, device="cuda")))
    return trip


def packed(trip):
    n = len(trip)
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    return (n, P(*[t[0].data_ptr() for t in trip]), P(*[t[1].data_ptr() for t in trip]), P(*[t[2].data_ptr() for t in trip]),
            I(*[t[0].shape[1] for t in trip]), I(*[t[1].shape[1] for t in trip]), T, 0)      # 0: NPCD_BF16


sets = [make_set(s) for s in range(SETS)]
packs = [packed(trip) for trip in sets]


def launch(name, i):
    rc = libs[name].npcd_wgrad_group(*packs[i], hip.stream_ptr())
    assert rc == 0, (name, rc)


def timed(name, i):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch(name, i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


# the bits of every form that computes the product, against the first form's, on one set
first = forms[0][0]
launch(first, 0)
torch.cuda.synchronize()
want = [t[2].clone() for t in sets[0]]
for name, _ in forms[1:]:
    for t in sets[0]:
        t[2].fill_(float("nan"))
    launch(name, 0)
    torch.cuda.synchronize()
    if "diag" in name:
        continue
    same = [bool(torch.equal(a, t[2])) for a, t in zip(want, sets[0])]
    print(f"{name}: {sum(same)} of {len(same)} outputs are the bits of {first}", flush=True)
    assert all(same), (name, same)

for name, _ in forms:                           # warm-up: code objects, the LDS attribute
    for i in range(SETS):
        launch(name, i)
torch.cuda.synchronize()
times = {name: [] for name, _ in forms}
for r in range(REPS):
    for i in range(SETS):
        for j, (name, _) in enumerate(forms):
            times[name].append(timed(name, (i + j) % SETS))      # (the set a form just read is never the next one's)
flop = sum(2 * T * N * K for _, N, K in SHAPES)
floor = min(times[first]) / BLOCKS
for name, _ in forms:
    v = sorted(times[name])
    mn, med, mx = v[0] / BLOCKS, statistics.median(v) / BLOCKS, v[-1] / BLOCKS
    gate = "" if name == first or "diag" in name else f"  gate (median < {floor:.1f}): {'PASS' if med < floor else 'no'}"
    print(f"{name:16s} per block: min {mn:7.1f} us  median {med:7.1f} us  max {mx:7.1f} us   ({flop / med / 1e6:5.0f} TF/s at the median, "
          f"{len(v)} timings){gate}", flush=True)

if args.screen:
    name = args.screen
    launch(name, 0)
    torch.cuda.synchronize()
    want = [t[2].clone() for t in sets[0]]
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")          # six copies of 1 GiB last about as long as the launch
    dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    for mode in ("idle chip", "beside a streaming copy"):
        bad = 0
        for it in range(args.launches):
            if mode != "idle chip":
                with torch.cuda.stream(side):
                    for _ in range(6):
                        dst.copy_(src, non_blocking=True)
            launch(name, 0)
            bad += sum(int(not torch.equal(a, t[2])) for a, t in zip(want, sets[0]))
        torch.cuda.synchronize()
        print(f"race screen, {name}, {mode}: {args.launches} launches x 16 outputs, {bad} differ from the first launch's", flush=True)
        assert bad == 0
