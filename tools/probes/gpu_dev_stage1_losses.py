"""Dev probe: what the stage-1 regularisers (KL + TV) cost, torch operators against the fused kernel pair (csrc/stage1_losses.hip).
  A. HIP events around the loss forward + backward alone at B 8 / N 512 / F 32 / k 8 (the grid is built once, outside), the two paths
     in alternating blocks; host waits per call counted with torch's sync debug mode in an untimed call.
  B. PointNeRFTrainer.step at the bench_stage1 configuration (8 objects x 50 views x 112 rays, 128 depth samples), fused_losses off / on
     in alternating legs (two of each), for each mlp_dtype; 20 timed steps per leg after 6 burn-in steps, HIP events per step.
usage: python3 tools/probes/gpu_dev_stage1_losses.py [output file]"""
import os
import sys
import warnings

R_ = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R_); sys.path.insert(0, os.path.join(R_, "neural-point-cloud-diffusion_amd"))
import numpy as np
import torch
from npcd.losses import PointNeRFLoss
from npcd.models import NPCD
from npcd.train import PointNeRFTrainer
from npcd.utils import synthetic as orr

dev = torch.device("cuda", 0)
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if out:
        out.write(line + "\n"); out.flush()


def host_waits(fn):
    """synchronising calls of one fn() as torch's sync debug mode reports them"""
    prev = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    return sum("synchroniz" in str(x.message) for x in w)


def make_net(B, N, F_):
    torch.manual_seed(0)
    net = NPCD(n_obj=B, coords_dim=3, feats_dim=F_, num_points=N, use_view_dir=False, width=64, layers=1, heads=1, pointnerf_only=True).to(dev)
    coords, feats = orr.ellipsoid_cloud(N, F_, B, seed=0)
    net.pointnerf.set_all_coords(coords.to(dev))
    return net, coords.to(dev), feats.to(dev)


say("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| hip", torch.version.hip)

# ---- A: the regularisers alone ----------------------------------------------------------------------------------------------------
B, N, F_ = 8, 512, 32
net, coords, feats = make_net(B, N, F_)
net.pointnerf.voxel_grid.set_pointset(coords)
table = torch.cat((feats, torch.full_like(feats, -4.0)), dim=-1).requires_grad_(True)
aux = {"coords": coords, "feats": table[..., :F_], "feats_mean": table[..., :F_], "feats_log_var": table[..., F_:]}
paths = {"torch": PointNeRFLoss(net, 1, 1e-7, 3.5e-7), "fused": PointNeRFLoss(net, 1, 1e-7, 3.5e-7, fused_regularisers=True)}


def regularisers(loss):
    table.grad = None
    kl_l, tv_l = loss.neural_point_cloud_kl_loss, loss.neural_point_cloud_tv_loss
    if kl_l.fused:
        from npcd.hip.losses import stage1_regularisers
        from npcd.losses import self_neighbour_lists
        nb = self_neighbour_lists(net.pointnerf.field.aggregator, coords)
        tv, _, kl, _ = stage1_regularisers(coords, nb, aux["feats"], aux["feats_mean"], aux["feats_log_var"], tv_l.weight, kl_l.weight)
    else:
        kl, tv = kl_l(None, None, aux, 0)[0], tv_l(None, None, aux, 0)[0]
    (kl + tv).backward()
    return kl.detach(), tv.detach()


for name, loss in paths.items():
    for _ in range(5):
        kl, tv = regularisers(loss)
    torch.cuda.synchronize()
    say(f"A {name}: kl {float(kl):.9e} tv {float(tv):.9e} |grad|max {float(table.grad.abs().max()):.6e} host waits per call {host_waits(lambda: regularisers(loss))}")
reps, blocks = 50, 6
ms = {k: [] for k in paths}
for blk in range(blocks):
    for name, loss in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            regularisers(loss)
        e1.record()
        torch.cuda.synchronize()
        ms[name].append(e0.elapsed_time(e1) / reps)
for name, v in ms.items():
    say(f"A {name}: ms per forward + backward, {blocks} alternating blocks of {reps}: " + " ".join(f"{x:.3f}" for x in v) + f" | median {np.median(v):.3f}")

# ---- B: the training step ---------------------------------------------------------------------------------------------------------
B, T, N, F_, res = 8, 50, 512, 32, 128
extr = torch.stack([orr.look_at_pose(7.2 * i, 20 - 0.5 * i) for i in range(T)])[None].expand(B, -1, -1, -1).contiguous().to(dev)
intr = orr.srn_intrinsics()[None, None].expand(B, T, 3, 3).contiguous().to(dev)
sample = {"images": torch.rand(B, T, 3, res, res, device=dev), "intrinsics": intr, "extrinsics": extr, "obj_idx": torch.arange(B, device=dev)}
burn, n = 6, 20
for dt in (None, "fp32_class", torch.bfloat16):
    legs = {False: [], True: []}
    waits = {}
    for leg in range(4):
        fused = bool(leg & 1)
        net, _, _ = make_net(B, N, F_)
        tr = PointNeRFTrainer(net, mlp_dtype=dt, fused_losses=fused)
        torch.cuda.empty_cache()
        torch.manual_seed(1)
        for _ in range(burn):
            tr.step(sample)
        torch.cuda.synchronize()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        marks[0].record()
        for i in range(n):
            loss, _ = tr.step(sample)
            marks[i + 1].record()
        torch.cuda.synchronize()
        per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(n))
        legs[fused].append((per[0], per[n // 2], per[-1], float(np.mean(per))))
        waits[fused] = host_waits(lambda: tr.step(sample))
        del tr, net
    for fused in (False, True):
        say(f"B mlp_dtype={dt} fused_losses={fused}: host waits per step {waits[fused]}; ms per step (min / median / max / mean) per leg: "
            + " | ".join("%.2f / %.2f / %.2f / %.2f" % l for l in legs[fused]))
if out:
    out.close()
