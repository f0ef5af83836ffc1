"""Dev probe: what the second-order multistep step costs beside the first-order step of the same build, and what a 20-level generate
takes with either solver.

Launch legs on the same operands, HIP events around LAUNCHES back-to-back launches each, rounds alternating, median and min per leg:
  ddim      : npcd_sampler_step, both tensors in reverse mode, deterministic, no noise (2 loads + 1 store per element)
  multistep : npcd_sampler_step_multistep, unmasked, at a level with w > 0 (3 loads + 2 stores: the history is read and rewritten)
at the benchmark's sampler shape: coords 3 x 512, feats 128 x 512, bf16 eps, batch 16 (and batch 256, where the launch is no longer
all there is).
Generate legs: DiffusionModel.generate(16, batch_size=16, sampling_steps=20, use_graph=True, dtype=bf16) of the benchmark denoiser
(width 1024, 24 layers, 16 heads) with eta = 0 on logsnr levels and with solver="dpmpp2m", device-synchronised wall, alternating.

    python tools/probes/gpu_dev_sampler_multistep.py [rounds=7] [launches=2000] [out.txt]
"""
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "neural-point-cloud-diffusion_amd"))
import torch  # noqa: E402

from npcd.hip import elementwise as ew  # noqa: E402
from npcd.models.diffusion import DiffusionModel  # noqa: E402
from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
LAUNCHES = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
OUT = sys.argv[3] if len(sys.argv) > 3 else None
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def legs_for(B, sched, ddim):
    g = torch.Generator(device="cuda").manual_seed(B)
    t = torch.full((B,), int(sched.timesteps[31]), device="cuda", dtype=torch.long)
    assert float(sched.multistep_table[t[0], 7]) > 0
    clips = ((-3.0, 3.0), (-1.0, 1.0))
    one, two = [], []
    for ch, clip in zip((3, 128), clips):
        x, eps, hist = (torch.randn(B, ch, 512, device="cuda", generator=g) for _ in range(3))
        out = torch.empty_like(x)
        one.append(dict(mode="reverse", x_t=x, eps=eps.bfloat16(), noise=None, clip=clip, out=out))
        two.append(dict(mode="reverse", x_t=x, eps=eps.bfloat16(), clip=clip, out=out, hist=hist))
    return {"ddim": lambda: ew.sampler_step(one[0], one[1], t, ddim.table, True),
            "multistep": lambda: ew.sampler_step_multistep(two[0], two[1], t, sched.multistep_table)}


def launches(process):
    sched = process.sampling_schedule(steps=50, solver="dpmpp2m")
    ddim = process.sampling_schedule(steps=50, eta=0.0, spacing="logsnr")
    for B in (16, 256):
        legs = legs_for(B, sched, ddim)
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
        say(f"B={B:3d} multistep / ddim = {statistics.median(us['multistep']) / statistics.median(us['ddim']):.3f} (medians)")


def generates():
    torch.manual_seed(0)
    m = DiffusionModel(3, 128, 512, 1024, 24, 16, True).cuda().eval()
    with torch.no_grad():
        m.coords_normalization.min.fill_(-3.0); m.coords_normalization.max.fill_(3.0)
        m.feats_normalization.min.fill_(-1.0); m.feats_normalization.max.fill_(1.0)
    legs = {"ddim eta=0 logsnr": dict(eta=0.0, spacing="logsnr"), "dpmpp2m": dict(solver="dpmpp2m")}
    kw = dict(batch_size=16, progress=False, sampling_steps=20, use_graph=True, dtype=torch.bfloat16)
    for extra in legs.values():
        m.generate(16, **kw, **extra)
    torch.cuda.synchronize()
    s = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for name, extra in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(16, **kw, **extra)
            torch.cuda.synchronize()
            s[name].append(time.perf_counter() - t0)
    for name, v in s.items():
        say(f"generate(16, sampling_steps=20, graph, bf16) {name:18s}: median {statistics.median(v) * 1e3:8.2f} ms, min {min(v) * 1e3:8.2f} "
            f"({ROUNDS} rounds; 20 replays + 2 warm-up steps + capture)")
    say(f"dpmpp2m / ddim = {statistics.median(s['dpmpp2m']) / statistics.median(s['ddim eta=0 logsnr']):.4f} (medians)")


def main():
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    launches(GaussianDiffusion().cuda())
    generates()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
