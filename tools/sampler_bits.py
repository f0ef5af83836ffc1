"""The bits of the scheduled sampler's step kernels (csrc/sampler.hip) on fixed operands: operands are drawn on the CPU from seeded
generators, every case is one launch on the GPU through ew.sampler_step (npcd_sampler_step, or npcd_sampler_step_keep with a mask) or
ew.sampler_step_multistep, and the sha256 of every output (out, x0 and the updated history of either tensor) goes into one JSON object
{case id / tensor / output: digest}.

    python tools/sampler_bits.py <package dir> [out.json]

<package dir> is the directory that holds the `npcd` package whose build is to run (neural-point-cloud-diffusion_amd of a checkout).
tests/golden/sampler_bits_parent.json is this tool's output on the commit BEFORE the three step kernels became one template
(docs/experiments.md R29.1); tests/test_gpu_sampler_bits.py asserts the same digests on the current build.  The kernels are written-out
fp32 operations on tables made on the host, so the digests depend neither on a library nor on the machine."""
import functools
import hashlib
import json
import sys

import torch

# (channels, n_points) of coords and of feats: 16 bytes per lane; one element per lane; feats past the grid cap of the 16-byte loop
# (4 x 1024 x 256 + 4 x 257 elements) beside an odd coords tensor
SHAPES = {"vec": ((3, 64), (32, 64)), "scalar": ((3, 509), (32, 509)), "past_cap_vec": ((1, 300001), (1, 1_049_604))}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
CLIPS = ((-1.5, 1.5), (-0.75, 1.0))
MODES = {"rev_rev": ("reverse", "reverse"), "hold_rev": ("hold", "reverse"), "rev_hold": ("reverse", "hold")}
B = 2


def cases():
    """(case id, entry, size name, dtype name, modes of (coords, feats), clip, noise, seed); a mode is "reverse", "hold" or "keep".
    entry "step": noise = eta > 0, the tables of eta = 0.5 or 0; "multistep": the tables of solver="dpmpp2m"."""
    out = []

    def add(entry, size, dn, modes, clip, noise):
        cid = f"{entry}/{size}/{dn}/{'+'.join(modes)}/{'clip' if clip else 'noclip'}/{'noise' if noise else 'det'}"
        out.append((cid, entry, size, dn, modes, clip, noise, 1000 + len(out)))

    for size in ("vec", "scalar"):
        for dn in DTYPES:
            for modes in MODES.values():
                for on in (True, False):
                    add("step", size, dn, modes, on, on)
        for masks in (("keep", "reverse"), ("keep", "keep")):
            for noise in (True, False):
                add("step", size, "bf16" if (masks[1] == "keep") != noise else "f32", masks, True, noise)
        for modes in (("reverse", "reverse"), ("reverse", "keep"), ("keep", "keep")):
            for dn in DTYPES:
                add("multistep", size, dn, modes, dn == "f32", False)
    add("multistep", "vec", "f32", MODES["hold_rev"], True, False)
    for dn in DTYPES:
        add("step", "past_cap_vec", dn, MODES["rev_rev"], True, True)
    add("step", "past_cap_vec", "bf16", ("reverse", "keep"), True, True)
    add("multistep", "past_cap_vec", "f32", ("reverse", "reverse"), True, False)
    add("multistep", "past_cap_vec", "f32", ("reverse", "keep"), True, False)
    return out


def operands(size, dn, seed):
    """Per tensor (x_t, eps, noise, known, hist, mask) on the CPU: standard normal draws of one seeded generator, eps rounded to its
    type, the mask a fair coin per point."""
    g = torch.Generator().manual_seed(seed)
    ops = []
    for C, N in SHAPES[size]:
        x, eps, noise, known, hist = (torch.randn(B, C, N, generator=g) for _ in range(5))
        ops.append((x, eps.to(DTYPES[dn]), noise, known, hist, torch.rand(B, N, generator=g) < 0.5))
    return ops


@functools.lru_cache(maxsize=None)
def _process():
    from npcd.models.diffusion.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion().cuda()          # (it caches its schedules)


def run(case, ops):
    """One launch of the case on the GPU -> {"coords/out": tensor, "coords/x0": ..., "coords/hist": ..., "feats/...": ...}; outputs
    start as NaN.  A hold-mode tensor has no x0 and no history."""
    from npcd.hip import elementwise as ew
    _, entry, _, _, modes, clip, noise, _ = case
    process = _process()
    multistep = entry == "multistep"
    sched = process.sampling_schedule(steps=50, solver="dpmpp2m") if multistep else process.sampling_schedule(steps=50, eta=0.5 if noise else 0.0)
    t = torch.tensor([0, int(sched.timesteps[31])], device="cuda")
    specs, outs = [], {}
    for name, mode, (x, eps, z, known, hist, mask), cl in zip(("coords", "feats"), modes, ops, CLIPS):
        x, eps, z, known, hist, mask = (v.cuda() for v in (x, eps, z, known, hist, mask))
        outs[f"{name}/out"] = torch.full_like(x, float("nan"))
        if mode == "hold":
            specs.append(dict(mode="hold", known=known, noise=z, out=outs[f"{name}/out"]))
            continue
        outs[f"{name}/x0"] = torch.full_like(x, float("nan"))
        spec = dict(mode=mode, x_t=x, eps=eps, clip=cl if clip else None, out=outs[f"{name}/out"], x0_out=outs[f"{name}/x0"])
        if mode == "keep":
            spec.update(noise=z, known=known, keep=mask)
        elif noise:
            spec.update(noise=z)
        if multistep:
            spec.update(hist=hist)
            outs[f"{name}/hist"] = hist
        specs.append(spec)
    if multistep:
        ew.sampler_step_multistep(specs[0], specs[1], t, sched.multistep_table)
    else:
        ew.sampler_step(specs[0], specs[1], t, sched.table, sched.deterministic)
    torch.cuda.synchronize()
    return outs


def digest(out):
    assert out.dtype == torch.float32 and out.is_contiguous()
    return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def main(argv):
    assert len(argv) > 1, __doc__
    sys.path.insert(0, argv[1])
    assert torch.cuda.is_available(), "the steps run on the GPU"
    bits = {}
    for case in cases():
        for what, out in run(case, operands(case[2], case[3], case[7])).items():
            assert bool(torch.isfinite(out).all()), (case[0], what)
            bits[f"{case[0]}/{what}"] = digest(out)
    text = json.dumps(bits, indent=0, sort_keys=True) + "\n"
    if len(argv) > 2:
        with open(argv[2], "w") as f:
            f.write(text)
    print(f"{len(cases())} cases, {len(bits)} digests" + (f" -> {argv[2]}" if len(argv) > 2 else ""))
    if len(argv) <= 2:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv)
