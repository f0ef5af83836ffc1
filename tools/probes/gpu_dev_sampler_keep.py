"""Dev probe: what a masked step and a re-noise launch cost beside the unmasked step of the same build.

Three legs on the same operands, HIP events around LAUNCHES back-to-back launches each, rounds alternating, median and min per leg:
  unmasked : npcd_sampler_step, both tensors in reverse mode (3 loads + 1 store per element)
  masked   : npcd_sampler_step_keep, both tensors with a mask of about half the points (4 loads + 1 store per element, one mask byte
             per point and channel row)
  re-noise : npcd_sampler_step, both tensors in hold mode on SamplingSchedule.renoise_table (2 loads + 1 store)
at the benchmark's sampler shape: coords 3 x 512, feats 128 x 512, bf16 eps, batch 16 (and batch 256, where the launch is no longer
all there is).  The backbone forward of that step is 8.4 ms (docs/experiments.md R13.1).

    python tools/probes/gpu_dev_sampler_keep.py [rounds=7] [launches=2000] [out.txt]
"""
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "neural-point-cloud-diffusion_amd"))
import torch  # noqa: E402

from npcd.hip import elementwise as ew  # noqa: E402
from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
OUT = sys.argv[3] if len(sys.argv) > 3 else None
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def legs_for(B, sched):
    g = torch.Generator(device="cuda").manual_seed(B)
    t = torch.full((B,), int(sched.timesteps[31]), device="cuda", dtype=torch.long)
    mask = torch.rand(B, 512, device="cuda", generator=g) < 0.5
    ops = []
    for ch in (3, 128):
        x, eps, z, kn = (torch.randn(B, ch, 512, device="cuda", generator=g) for _ in range(4))
        ops.append(dict(x_t=x, eps=eps.bfloat16(), noise=z, known=kn, out=torch.empty_like(x)))
    clips = ((-3.0, 3.0), (-1.0, 1.0))
    rev = [dict(mode="reverse", x_t=o["x_t"], eps=o["eps"], noise=o["noise"], clip=c, out=o["out"]) for o, c in zip(ops, clips)]
    keep = [dict(mode="keep", keep=mask, clip=c, **o) for o, c in zip(ops, clips)]
    hold = [dict(mode="hold", known=o["x_t"], noise=o["noise"], out=o["out"]) for o in ops]
    return {"unmasked": lambda: ew.sampler_step(rev[0], rev[1], t, sched.table, False),
            "masked": lambda: ew.sampler_step(keep[0], keep[1], t, sched.table, False),
            "re-noise": lambda: ew.sampler_step(hold[0], hold[1], t, sched.renoise_table, False)}


def main():
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    sched = GaussianDiffusion().cuda().sampling_schedule(steps=50, eta=0.5)
    for B in (16, 256):
        legs = legs_for(B, sched)
        us = {k: [] for k in legs}
        for fn in legs.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for name, fn in legs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(LAUNCHES):
                    fn()
                b.record()
                b.synchronize()
                us[name].append(a.elapsed_time(b) / LAUNCHES * 1e3)
        elems = B * (3 + 128) * 512
        for name, v in us.items():
            say(f"B={B:3d} ({elems} elements) {name:9s}: median {statistics.median(v):7.2f} us per launch, min {min(v):7.2f} "
                f"({ROUNDS} rounds x {LAUNCHES} launches, host-paced)")
        base = statistics.median(us["unmasked"])
        for name in ("masked", "re-noise"):
            say(f"B={B:3d} {name:9s} / unmasked = {statistics.median(us[name]) / base:.3f} (medians)")
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
