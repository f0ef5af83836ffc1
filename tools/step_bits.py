"""The bits of a denoiser training step under the switches of the fused backbone node (npcd/models/diffusion/fused.py): for every
case one fresh interpreter with that case's environment (the switches are read at import) builds a seeded DiffusionModel +
DiffusionTrainer, runs one forward + backward on seeded inputs drawn on the CPU and then two step()s, and reports the sha256 of the
flat gradient buffer after the backward, the sha256 of the flat parameter buffer after the steps, and the loss as hex.  All cases
go into one JSON object {case id: {"grad": ..., "params": ..., "loss": ...}}.

    python tools/step_bits.py <package dir> [out.json]

<package dir> is the directory that holds the `npcd` package (with its library built), so the same file runs against a checkout of
another commit: two commits that issue the same kernels in the same order per tensor give byte-identical files on one machine.
(Library GEMM bits are not promised across machines or library builds: compare files of one machine only.)  The children run one
after the other, each under its own time limit; the first one that fails stops the tool."""
import hashlib
import json
import os
import subprocess
import sys

CHILD_TIMEOUT = 240        # seconds per case

SMALL = dict(W=256, H=4, L=6, B=2, N=135)            # T = 272: one 256-row tile + 16 left-over rows
NO_SIDE = {"NPCD_WGRAD_STREAM": "0", "NPCD_WGRAD_MULTIBLOCK": "0"}
SLICED = dict(W=256, H=4, L=2, B=8, N=512)           # T = 4,104: the row-split weight gradients have slices
WIDE = dict(W=1024, H=16, L=1, B=2, N=135)           # attn.c_proj is the 1024 x 1024 product of npcd_linear128_fwd

CASES = [
    ("01_default", SMALL, {}),
    ("02_wgrad_group_off", SMALL, {"NPCD_WGRAD_GROUP": "0"}),
    ("03_join_per_block", SMALL, {"NPCD_WGRAD_JOIN_PER_BLOCK": "1"}),
    ("04_multiblock_force", SMALL, {"NPCD_WGRAD_STREAM": "0", "NPCD_WGRAD_MULTIBLOCK": "force", "NPCD_WGRAD_MULTIBLOCK_MIN_T": "0"}),
    ("05_direct", SMALL, NO_SIDE),
    ("06_direct_own_wgrad", SMALL, {**NO_SIDE, "NPCD_OWN_WGRAD": "1"}),
    ("07_own_dgelu", SMALL, {"NPCD_OWN_DGELU": "1"}),
    ("08_dgrad_t", SMALL, {"NPCD_DGRAD_T_MIN_T": "0"}),
    ("09_dgrad_t_nn", SMALL, {"NPCD_DGRAD_T_MIN_T": "0", "NPCD_DGRAD_NN": "1"}),
    ("10_arena_off", SMALL, {"NPCD_STEP_ARENA": "0"}),
    ("11a_split_min_0", SMALL, {"NPCD_GEMM_SPLIT_MIN": "0"}),
    ("11b_split_min_0_small_first", SMALL, {"NPCD_GEMM_SPLIT_MIN": "0", "NPCD_GEMM_SPLIT_SMALL_FIRST": "1"}),
    ("11c_no_gemm_split", SMALL, {"NPCD_NO_GEMM_SPLIT": "1"}),
    ("12_no_attn_colsum", SMALL, {"NPCD_NO_ATTN_COLSUM": "1"}),
    ("13a_sliced_direct", SLICED, NO_SIDE),
    ("13b_sliced_direct_no_sum_kernel", SLICED, {**NO_SIDE, "NPCD_NO_SUM_KERNEL": "1"}),
    ("14a_wide_default", WIDE, {}),
    ("14b_wide_no_lin128", WIDE, {"NPCD_NO_LIN128": "1"}),
    ("15a_fp32_class_library", {**SMALL, "dtype": "fp32_class"}, {"NPCD_X2_WGRAD": "library"}),
    ("15b_fp32_class_own", {**SMALL, "dtype": "fp32_class"}, {"NPCD_X2_WGRAD": "own"}),
]


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def child(shape):
    """one case, in this interpreter: prints its JSON result as the last line"""
    import torch
    from npcd.models.diffusion import DiffusionModel
    from npcd.train import DiffusionTrainer
    W, H, L, B, N, F_ = shape["W"], shape["H"], shape["L"], shape["B"], shape["N"], 32
    dtype = shape.get("dtype", torch.bfloat16)
    torch.manual_seed(1234)
    model = DiffusionModel(3, F_, N, W, L, H, True)
    g = torch.Generator().manual_seed(99)
    with torch.no_grad():
        for p in model.parameters():               # no parameter is left at an initial zero or one
            p.add_(torch.randn(p.shape, generator=g) * 0.02)
    model = model.cuda().train()
    tr = DiffusionTrainer(model, lr=7e-5, weight_decay=0.01, ema_decay=0.9999, dtype=dtype)
    assert tr.native and model.denoiser.backbone.fused_engine is not None
    coords, feats = torch.randn(B, 3, N, generator=g).cuda(), (torch.rand(B, F_, N, generator=g) * 2 - 1).cuda()
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    cn, fn = torch.randn(B, 3, N, generator=g).cuda(), torch.randn(B, F_, N, generator=g).cuda()
    tr.flat.zero_grad()
    tr.reducer.start_step()
    amp = None if tr.fp32_class else tr.dtype
    with torch.autocast("cuda", dtype=amp, enabled=amp is not None):
        loss, _, _ = tr.model.compute_loss(coords, feats, t=t, coords_noise=cn, feats_noise=fn)
    loss.backward()
    torch.cuda.synchronize()
    out = {"grad": digest(tr.flat.grad), "loss": float(loss).hex()}
    assert bool(torch.isfinite(tr.flat.grad).all())
    for _ in range(2):
        tr.step(coords, feats, t=t, coords_noise=cn, feats_noise=fn)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr.flat.flat).all())
    out["params"] = digest(tr.flat.flat)
    tr.close()
    print(json.dumps(out, sort_keys=True))


def main(argv):
    if len(argv) >= 3 and argv[1] == "--child":
        child(json.loads(argv[2]))
        return 0
    pkg = os.path.abspath(argv[1])
    assert os.path.isdir(os.path.join(pkg, "npcd")), f"{pkg}: no npcd package"
    bits = {}
    for cid, shape, switches in CASES:
        env = {k: v for k, v in os.environ.items() if not k.startswith("NPCD_")}
        env.update(switches)
        env["PYTHONPATH"] = pkg
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(shape)], env=env, cwd=pkg,
                             capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        if run.returncode != 0:
            sys.stderr.write(run.stdout + run.stderr)
            print(f"{cid}: exit status {run.returncode}; stopping", flush=True)
            return 1
        bits[cid] = json.loads(run.stdout.strip().splitlines()[-1])
        print(cid, bits[cid]["grad"][:16], bits[cid]["params"][:16], bits[cid]["loss"], flush=True)
    text = json.dumps(bits, indent=0, sort_keys=True) + "\n"
    if len(argv) > 2:
        with open(argv[2], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
