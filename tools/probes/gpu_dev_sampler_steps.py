"""Dev probe: the scheduled sampler (DDIM steps / eta / one fused launch per step) beside the 1000-step DDPM loop, on one box, interleaved.

  A. ms per reverse step at the benchmark's model size, batch 16, bf16 autocast + HIP graph: p_sample_loop() as it was (two randn_like and
     two npcd_ddpm_reverse_step per step) against p_sample_loop(steps=None, eta=1.0) (two randn_like and ONE npcd_sampler_step), and
     eta=0.0 (the one launch alone); rounds alternate, median and min per leg.
  B. DiffusionModel.generate seconds (16 clouds) and npcd.eval.sample_and_render clouds/s (4 clouds x 251 poses, 128 x 128) at
     sampling_steps in {1000, 50} and eta in {1, 0}, bf16 autocast + HIP graph.

    python tools/probes/gpu_dev_sampler_steps.py [rounds=5] [steps_per_round=100] [out.txt]
"""
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "neural-point-cloud-diffusion_amd"))
import torch  # noqa: E402

from npcd.eval import load_test_poses, sample_and_render  # noqa: E402
from npcd.models import NPCD  # noqa: E402
from npcd.models.diffusion import DiffusionModel  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
OUT = sys.argv[3] if len(sys.argv) > 3 else None
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def part_a():
    B = 16
    torch.manual_seed(0)
    m = DiffusionModel(3, 128, 512, 1024, 24, 16, True).cuda().eval()
    c, f = torch.randn(B, 3, 512, device="cuda"), torch.randn(B, 128, 512, device="cuda")
    dp = m.diffusion_process
    dp.num_timesteps = STEPS                      # a chain of STEPS levels: every leg walks all of them (capture amortised over them)
    legs = {"ddpm loop (parent)": {}, "scheduled eta=1": dict(steps=None, eta=1.0), "scheduled eta=0": dict(steps=None, eta=0.0)}
    ms = {k: [] for k in legs}

    def run(kw):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return dp.p_sample_loop(m.denoiser, c, f, (-3.0, 3.0), (-1.0, 1.0), use_graph=True, **kw)

    for kw in legs.values():
        run(kw)                                   # warm every leg
    for _ in range(ROUNDS):
        for name, kw in legs.items():
            dt, out = timed(lambda: run(kw))
            assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[1]).all())
            ms[name].append(dt / STEPS * 1e3)
    for name, v in ms.items():
        say(f"A  {name:20s} B={B} bf16+graph: median {statistics.median(v):6.3f} ms per reverse step, min {min(v):6.3f} ({ROUNDS} rounds x {STEPS} steps)")
    base = statistics.median(ms["ddpm loop (parent)"])
    for name in ("scheduled eta=1", "scheduled eta=0"):
        say(f"A  {name:20s} / ddpm loop = {statistics.median(ms[name]) / base:.4f} (medians)")
    del m
    torch.cuda.empty_cache()


def part_b():
    torch.manual_seed(0)
    m = DiffusionModel(3, 128, 512, 1024, 24, 16, True).cuda().eval()
    with torch.no_grad():
        m.coords_normalization.min.fill_(-3.0); m.coords_normalization.max.fill_(3.0)
        m.feats_normalization.min.fill_(-1.0); m.feats_normalization.max.fill_(1.0)
    grid = [(1000, 1.0), (1000, 0.0), (50, 1.0), (50, 0.0)]
    kw = dict(batch_size=16, progress=False, dtype=torch.bfloat16, use_graph=True)
    m.generate(16, sampling_steps=4, eta=1.0, **kw)
    dt0, _ = timed(lambda: m.generate(16, **kw))
    say(f"B  generate(16) as it was (1000-step DDPM loop)      : {dt0:7.3f} s")
    for steps, eta in grid:
        dt, (cs, fs) = timed(lambda: m.generate(16, sampling_steps=steps, eta=eta, **kw))
        ok = all(bool(torch.isfinite(x).all()) for x in cs + fs)
        say(f"B  generate(16, sampling_steps={steps:4d}, eta={eta:.0f})        : {dt:7.3f} s  ({dt0 / dt:5.2f} x the 1000-step DDPM loop; finite={ok})")
    del m
    torch.cuda.empty_cache()
    torch.manual_seed(0)
    net = NPCD(n_obj=1, coords_dim=3, feats_dim=32, num_points=512, use_view_dir=False, width=1024, layers=24, heads=16).cuda().eval()
    with torch.no_grad():
        net.diffusion.coords_normalization.min.fill_(-2.5); net.diffusion.coords_normalization.max.fill_(2.5)
        net.diffusion.coords_normalization.scale.fill_(0.2)
        net.diffusion.feats_normalization.min.fill_(-1.0); net.diffusion.feats_normalization.max.fill_(1.0)
    poses, intr = load_test_poses("srncars")
    skw = dict(num_samples=4, generate_batch_size=4, render_batch_size=8, resolution=128, dtype=torch.bfloat16, use_graph=True)
    sample_and_render(net, poses[:8], intr[:8], sampling_steps=4, eta=1.0, **skw)
    r0 = sample_and_render(net, poses, intr, **skw)
    say(f"B  sample_and_render(4 clouds) as it was             : generate {r0['generate_seconds']:6.3f} s, render {r0['render_seconds']:6.3f} s, "
        f"{r0['clouds_per_s_end_to_end']:6.3f} clouds/s, {r0['views_per_s']:7.1f} views/s")
    for steps, eta in grid:
        r = sample_and_render(net, poses, intr, sampling_steps=steps, eta=eta, **skw)
        say(f"B  sample_and_render(4 clouds, steps={steps:4d}, eta={eta:.0f})  : generate {r['generate_seconds']:6.3f} s, render {r['render_seconds']:6.3f} s, "
            f"{r['clouds_per_s_end_to_end']:6.3f} clouds/s, {r['views_per_s']:7.1f} views/s "
            f"({r['clouds_per_s_end_to_end'] / r0['clouds_per_s_end_to_end']:5.2f} x end to end)")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this probe measures on the GPU"
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}")
    part_a()
    part_b()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as fh:
            fh.write("\n".join(LINES) + "\n")
