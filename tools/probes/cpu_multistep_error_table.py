"""The analytic-denoiser error table of docs/experiments.md R28.1: rms error of the sampler against the exact probability-flow solution
for K = 5 ... 160 levels, both spacings and both solvers, float64 states on the CPU (the torch formulation of the loop).

Every element's data is N(mu, s^2), mu uniform in [-0.5, 0.5], s uniform in [0.2, 0.8], 4,096 elements, seed 0; the denoiser is the
exact one, eps = sqrt(1 - a) (x_t - sqrt(a) mu) / (a s^2 + 1 - a), and x_0 = mu + s (x_T - sqrt(a_T) mu) / sqrt(a_T s^2 + 1 - a_T).

    python tools/probes/cpu_multistep_error_table.py
"""
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(R, "neural-point-cloud-diffusion_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion  # noqa: E402


def main():
    gd = GaussianDiffusion()
    acp = torch.from_numpy(np.cumprod(1.0 - gd.np_betas.astype(np.float64)))
    g = torch.Generator().manual_seed(0)
    n, nc = 4096, 3 * 128
    mu = torch.rand(n, generator=g, dtype=torch.float64) - 0.5
    s = 0.2 + 0.6 * torch.rand(n, generator=g, dtype=torch.float64)
    x_T = torch.randn(n, generator=g, dtype=torch.float64)
    a_T = acp[-1]
    exact = mu + s * (x_T - a_T.sqrt() * mu) / torch.sqrt(a_T * s * s + (1.0 - a_T))

    def split(v):
        return v[:nc].reshape(1, 3, 128), v[nc:].reshape(1, -1, 128)

    mus, s2 = split(mu), split(s * s)

    def denoiser(c, f, t):
        a = acp[t].reshape(-1, 1, 1)
        return [torch.sqrt(1.0 - a) * (x - a.sqrt() * m) / (a * v + (1.0 - a)) for x, m, v in zip((c, f), mus, s2)]

    def rms(K, **kw):
        c0, f0 = split(x_T)
        with torch.no_grad():
            c, f = gd.p_sample_loop(denoiser, c0.clone(), f0.clone(), steps=K, **kw)
        return float(((torch.cat([c.reshape(-1), f.reshape(-1)]) - exact) ** 2).mean().sqrt())

    print("| K | DDIM, uniform in t | 2M, uniform in t | largest w | DDIM, logsnr | 2M, logsnr | largest w | DDIM / 2M on logsnr |")
    print("|---|---|---|---|---|---|---|---|")
    for K in (5, 10, 20, 40, 80, 160):
        du, tu = rms(K, eta=0.0), rms(K, solver="dpmpp2m", spacing="uniform")
        dl, tl = rms(K, eta=0.0, spacing="logsnr"), rms(K, solver="dpmpp2m")
        wu = gd.sampling_schedule(K, solver="dpmpp2m", spacing="uniform").coef64["w"].max()
        wl = gd.sampling_schedule(K, solver="dpmpp2m").coef64["w"].max()
        print(f"| {K} | {du:.3e} | {tu:.3e} | {wu:.2f} | {dl:.3e} | {tl:.3e} | {wl:.2f} | {dl / tl:.1f} |")


if __name__ == "__main__":
    main()
