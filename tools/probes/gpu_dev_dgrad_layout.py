"""docs/experiments.md R10.1: per block at width 1,024 and T token rows (argument, default 32,832) -- the grouped transpose against four
npcd_transpose_16 launches, cycling through ten sets of weights (more than the Infinity Cache holds), and the four data gradients
through fused._dgrad on the weight as stored (nn) and on the transposed copy (tn), tuned file loaded, three rounds; HIP events."""
import os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neural-point-cloud-diffusion_amd")]
import torch
import torch.cuda.tunable as tun
tun.enable(True); tun.tuning_enable(False)
tun.set_filename("/tmp/npcd_probe_unused.csv")
print("tuned file read:", tun.read_file(os.path.join(ROOT, "profiles", "tunableop_gfx950.csv")))
from npcd.hip import linear as hlin
from npcd.models.diffusion import fused

T = int(sys.argv[1]) if len(sys.argv) > 1 else 32832
Wd = 1024
SHAPES = [("c_qkv", 3 * Wd, Wd), ("attn_c_proj", Wd, Wd), ("c_fc", 4 * Wd, Wd), ("mlp_c_proj", Wd, 4 * Wd)]
dev = "cuda"
NB = 10            # sets of block weights cycled through: 10 x 50 MB of sources + destinations, more than the 256 MiB cache
ws = [[(torch.randn(n, k, device=dev) * 0.02).bfloat16() for _, n, k in SHAPES] for _ in range(NB)]
wTs = [[torch.empty(k, n, device=dev, dtype=torch.bfloat16) for _, n, k in SHAPES] for _ in range(NB)]

def timed(fn, iters, warm=3):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3

res = {"T": T}
res["transpose_group_us_per_block"] = timed(lambda i: hlin.transpose16_group(list(zip(ws[i % NB], wTs[i % NB]))), 60)
def old(i):
    for w, o in zip(ws[i % NB], wTs[i % NB]):
        hlin.transpose16(w, out=o)
res["transpose16_x4_us_per_block"] = timed(old, 60)
res["transpose_group_us_per_block_again"] = timed(lambda i: hlin.transpose16_group(list(zip(ws[i % NB], wTs[i % NB]))), 60)
for b in range(NB):
    for w, o in zip(ws[b], wTs[b]):
        assert torch.equal(o, w.t())
dys = {name: torch.randn(T, n, device=dev).bfloat16() for name, n, k in SHAPES}
for rep in range(3):
    for form in ("nn", "tn"):
        tot = 0.0
        for si, (name, n, k) in enumerate(SHAPES):
            dy = dys[name]
            def run(i, si=si, dy=dy):
                b = i % NB
                fused._dgrad(dy, ws[b][si], None if form == "nn" else wTs[b][si])
            us = timed(run, 20)
            res[f"{form}.{name}.rep{rep}"] = us
            tot += us
        res[f"{form}.block_total.rep{rep}"] = tot
print(json.dumps(res, indent=1))
