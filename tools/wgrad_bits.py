"""The bits of the weight-gradient kernels of csrc/gemm.hip on fixed operands: operands are drawn on the CPU from seeded generators,
every product runs on the GPU through ew.wgrad_group (one workgroup per 256 x 256 tile over all token rows) or ew.wgrad (the split-T
form with its slab sum), and the sha256 of every fp32 output goes into one JSON object {case id: digest}.

    python tools/wgrad_bits.py [out.json]

tests/golden/wgrad_bits_parent.json is this tool's output on the commit BEFORE the 64-token pipeline of the tile body (docs/experiments.md
R21.1); tests/test_gpu_wgrad_pipeline.py asserts the same digests on the current build.  A change of the tile body that keeps the
summation order of every accumulator (16-token groups in ascending token order) keeps every digest."""
import hashlib
import json
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (R, os.path.join(R, "neural-point-cloud-diffusion_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

# token counts: around one 32-token stage, around 64 / 128 / 160 tokens (a barrier step and the ring of the body, before and after
# R21.1), past the first wrap of the ring with a ragged last stage, and 513
TOKENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 193, 257, 513)
SLICED = (1026, 2079)                    # ew.wgrad at N = K = 256: npcd_wgrad_slices gives 2 and 4 slices
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
GROUP9 = tuple(((256, 512)[i % 2], (256, 512)[(i // 2 + i // 5) % 2]) for i in range(9))      # every (N, K) of {256, 512}^2 occurs
KINDS = {"one": ((256, 256),), "n512": ((512, 256),), "group9": GROUP9}


def cases():
    """(case id, kind, T, dtype name, ((N, K), ...), seed); kind "sliced" runs through ew.wgrad, the others through ew.wgrad_group"""
    out = []
    for dn in DTYPES:
        for T in TOKENS:
            for ki, (kind, shapes) in enumerate(KINDS.items()):
                out.append((f"{dn}/T{T}/{kind}", kind, T, dn, shapes, 10 * T + ki))
        for T in SLICED:
            out.append((f"{dn}/T{T}/sliced", "sliced", T, dn, ((256, 256),), 10 * T + 7))
    return out


def operands(T, shapes, dtype, seed):
    """[(dy [T, N], x [T, K]), ...] on the CPU: standard normal draws of one seeded generator, rounded to the 16-bit type"""
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(T, N, generator=g).to(dtype), torch.randn(T, K, generator=g).to(dtype)) for N, K in shapes]


def run(kind, ops):
    """the fp32 products of one case on the GPU, filled with NaN before the launch"""
    from npcd.hip import elementwise as ew
    trip = [(dy.cuda(), x.cuda(), torch.full((dy.shape[1], x.shape[1]), float("nan"), device="cuda")) for dy, x in ops]
    if kind == "sliced":
        for dy, x, out in trip:
            assert ew.wgrad(dy, x, out)
    else:
        assert ew.wgrad_group(trip)
    torch.cuda.synchronize()
    return [t[2] for t in trip]


def digest(out):
    assert out.dtype == torch.float32 and out.is_contiguous()
    return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()


def main(argv):
    assert torch.cuda.is_available(), "the products run on the GPU"
    bits = {}
    for cid, kind, T, dn, shapes, seed in cases():
        for i, out in enumerate(run(kind, operands(T, shapes, DTYPES[dn], seed))):
            assert bool(torch.isfinite(out).all()), cid
            bits[f"{cid}/{i}"] = digest(out)
    text = json.dumps(bits, indent=0, sort_keys=True) + "\n"
    if len(argv) > 1:
        with open(argv[1], "w") as f:
            f.write(text)
    print(f"{len(bits)} digests" + (f" -> {argv[1]}" if len(argv) > 1 else ""))
    if len(argv) <= 1:
        sys.stdout.write(text)


if __name__ == "__main__":
    main(sys.argv)
