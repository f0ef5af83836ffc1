"""Time DiffusionTrainer.step() in fp32 (dtype=None, the module path) and in the fp32 class (dtype="fp32_class", the fused split-operand
node) at the bench configuration (W 1024, L 24, H 16, n 513) and a batch given on the command line; one leg per process, so that the legs
can alternate (and a parent checkout can run the fp32 leg: --pkg points at its package directory).

    python tools/probes/gpu_dev_x2_train_step.py --dtype fp32_class --batch 64 [--steps 10 --warmup 3] [--pkg DIR]
                                                 [--wgrad library|own] [--tag NAME]

--wgrad: the form of the fp32-class weight gradients (NPCD_X2_WGRAD: library GEMMs on strided views of the split buffers, or the own
kernels on the operands stacked along the token dimension); --tag: the leg's name in the output line (default: the dtype).
Prints one line: leg, batch, median / min ms per step, peak memory (GiB)."""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=["none", "fp32_class"], required=True)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--pkg", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "neural-point-cloud-diffusion_amd"))
ap.add_argument("--tag", default="")
ap.add_argument("--wgrad", choices=["library", "own"], default=None)
args = ap.parse_args()
if args.wgrad is not None:
    os.environ["NPCD_X2_WGRAD"] = args.wgrad
sys.path.insert(0, os.path.abspath(args.pkg))

import torch  # noqa: E402
from npcd.models.diffusion import DiffusionModel  # noqa: E402
from npcd.train import DiffusionTrainer  # noqa: E402

W, L, H, F_, N = 1024, 24, 16, 128, 512
torch.manual_seed(0)
model = DiffusionModel(3, F_, N, W, L, H, True).cuda().train()
with torch.no_grad():
    model.denoiser.output_proj.weight.normal_(0, 0.02)        # (zero-initialised in the reference: no gradient would reach the backbone)
tr = DiffusionTrainer(model, dtype=None if args.dtype == "none" else "fp32_class")
g = torch.Generator().manual_seed(1)
B = args.batch
batch = [x.cuda() for x in (torch.randn(B, 3, N, generator=g), torch.randn(B, F_, N, generator=g), torch.randint(0, 1000, (B,), generator=g),
                            torch.randn(B, 3, N, generator=g), torch.randn(B, F_, N, generator=g))]
for _ in range(args.warmup):
    tr.step(*batch)
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
times = []
for _ in range(args.steps):
    t0 = time.perf_counter()
    tr.step(*batch)
    torch.cuda.synchronize()
    times.append((time.perf_counter() - t0) * 1e3)
peak = torch.cuda.max_memory_allocated() / 2 ** 30
print(f"LEG {args.tag or args.dtype} B {B} median_ms {statistics.median(times):.2f} min_ms {min(times):.2f} peak_GiB {peak:.1f}", flush=True)
tr.close()
