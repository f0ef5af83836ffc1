"""The stage-1 regularisers on their own kernels (csrc/stage1_losses.hip, npcd.hip.losses; `fused=True` on the loss modules,
`fused_losses=True` on PointNeRFTrainer) against float64 evaluations of the reference's formulas and against the torch-operator path.

Bars.  Against the oracle the fused path is held to what the torch path is held to in
test_gpu_train_render.py::test_losses_match_reference_golden_and_oracle: total rtol 1e-4, pointwise rtol 1e-4 / atol 1e-3, gradients
by that file's relative-L2 rule (3e-2), KL against the reference fixture at rtol 1e-5 -- and to its own error against float64 being no
more than twice the torch path's on the same inputs plus 1e-6 of the largest entry (both are fp32 sums of the same terms in other
orders).
Against the torch path on the same lists (the edge cases) the bars follow from the arithmetic.  With eps = 2^-24 per fp32 rounding:
  * a pointwise TV value is a sum of at most k F non-negative terms behind one subtraction, one square root, one division and one
    product each; two orders of that sum differ by at most (k F + 6) eps <= 1030 * 6e-8 = 6.2e-5 of the value -> rtol 1e-4;
  * a total is a mean of B N non-negative values, each within 6.2e-5 of the other side's; any order of adding m non-negative numbers
    is within (m - 1) eps of the exact sum, and both sides add in trees (lanes, waves, clouds here; torch's pairwise reduction
    there) of depth <= 200: 2.4e-5 between them -> rtol 1e-4 with the values' own error;
  * a pointwise KL value sums F SIGNED terms, so its error is relative to sum |term| <= 4 F max(1, m^2, exp(lv)) -> rtol 1e-4 plus
    atol 1e-5 of the largest pointwise value;
  * a feature gradient entry sums n <= 56 terms +-c (this point's k entries and the lists that name it, every c computed by the same
    three roundings on both sides up to the library's square root): two orders differ by at most (n - 1) eps sum |c| <= 55 * 56 * 6e-8 =
    1.9e-4 of the largest |c| -> 2e-4 of the largest gradient entry.  KL gradients are single products: 1e-6 relative.
"""
import types

import numpy as np
import pytest
import torch

from oracle import renderer as orr
from oracle import train_render as otr

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _grad_close(a, b, what, rel_l2=3e-2):
    """the rule of tests/test_gpu_train_render.py::_grad_close"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if float(b.abs().max()) == 0.0:
        assert float(a.abs().max()) == 0.0, what
        return
    l2 = float((a - b).norm() / b.norm())
    assert l2 <= rel_l2, (what, l2)


def _model(F_, N, n_obj=1):
    from npcd.models import NPCD
    net = NPCD(n_obj=n_obj, coords_dim=3, feats_dim=F_, num_points=N, use_view_dir=False, width=64, layers=1, heads=1, pointnerf_only=True)
    net.pointnerf.field.load_state_dict(orr.init_field_params(F_, seed=0))
    return net.cuda()


class _ListAggregator:
    """Aggregator.query_keypoints over GIVEN dense lists [B, N, k] (valid entries first): the torch path then runs on exactly the lists
    the fused kernel reads."""

    def __init__(self, nb):
        self.nb = nb

    def query_keypoints(self, x, kp_pos):
        B, N = self.nb.shape[:2]
        valid = self.nb[..., 0] >= 0
        return self.nb[valid].long(), None, valid.view(B, 1, N, 1, 1)


def _holder(agg):
    return types.SimpleNamespace(pointnerf=types.SimpleNamespace(field=types.SimpleNamespace(aggregator=agg)))


def _torch_path(coords, nb, feats, mean, log_var, w_tv, w_kl, g):
    """The torch-operator losses (npcd/losses) on given lists, forward + backward with the upstream gradients g -> dict."""
    from npcd.losses import NeuralPointCloudKLLoss, NeuralPointCloudTVLoss
    f, m, lv = (t.detach().clone().requires_grad_(True) for t in (feats, mean, log_var))
    tv_tot, _, tv_pw = NeuralPointCloudTVLoss(_holder(_ListAggregator(nb)), w_tv)(None, None, {"feats": f, "coords": coords}, 0)
    kl_tot, _, kl_pw = NeuralPointCloudKLLoss(None, w_kl)(None, None, {"feats_mean": m, "feats_log_var": lv}, 0)
    tv_pw, kl_pw = tv_pw["00_neural_point_cloud_tv"], kl_pw["00_neural_point_cloud_kl"]
    (tv_tot * g["tv_tot"] + (tv_pw * g["tv_pw"]).sum() + kl_tot * g["kl_tot"] + (kl_pw * g["kl_pw"]).sum()).backward()
    return {"tv_tot": tv_tot.detach(), "tv_pw": tv_pw.detach(), "kl_tot": kl_tot.detach(), "kl_pw": kl_pw.detach(),
            "dfeats": f.grad, "dmean": m.grad, "dlog_var": lv.grad}


def _fused(coords, nb, feats, mean, log_var, w_tv, w_kl, g):
    from npcd.hip.losses import stage1_regularisers
    f, m, lv = (t.detach().clone().requires_grad_(True) for t in (feats, mean, log_var))
    tv_tot, tv_pw, kl_tot, kl_pw = stage1_regularisers(coords, nb, f, m, lv, w_tv, w_kl)
    (tv_tot * g["tv_tot"] + (tv_pw * g["tv_pw"]).sum() + kl_tot * g["kl_tot"] + (kl_pw * g["kl_pw"]).sum()).backward()
    return {"tv_tot": tv_tot.detach(), "tv_pw": tv_pw.detach(), "kl_tot": kl_tot.detach(), "kl_pw": kl_pw.detach(),
            "dfeats": f.grad, "dmean": m.grad, "dlog_var": lv.grad}


def _upstream(B, N, gen):
    """non-zero upstream gradients on both totals and both pointwise outputs"""
    return {"tv_tot": 1.7, "kl_tot": -0.6, "tv_pw": (torch.rand(B, N, generator=gen) + 0.5).cuda(),
            "kl_pw": (torch.rand(B, N, generator=gen) - 1.5).cuda()}


def _assert_matches_torch_path(got, ref, what):
    for key in ("tv_tot", "kl_tot"):
        np.testing.assert_allclose(float(got[key]), float(ref[key]), rtol=1e-4, err_msg=f"{what} {key}")
    np.testing.assert_allclose(got["tv_pw"].cpu().numpy(), ref["tv_pw"].cpu().numpy(), rtol=1e-4, atol=0, err_msg=f"{what} tv_pw")
    np.testing.assert_allclose(got["kl_pw"].cpu().numpy(), ref["kl_pw"].cpu().numpy(), rtol=1e-4,
                               atol=1e-5 * float(ref["kl_pw"].abs().max()), err_msg=f"{what} kl_pw")
    for key, rel in (("dfeats", 2e-4), ("dmean", 1e-6), ("dlog_var", 1e-6)):
        err, scale = float((got[key] - ref[key]).abs().max()), float(ref[key].abs().max())
        assert err <= rel * scale, (what, key, err, scale)


def _cpu_lists(coords, k, r, include_self=True):
    """Each point's k nearest points within r (itself among them, like the query's result for a point the grid kept; without itself,
    like for a point dropped from a crowded cell), by (distance, index), as global indices padded with -1 -- computed on the host so
    that the case does not depend on the grid's own limits."""
    B, N = coords.shape[:2]
    d = torch.cdist(coords.double(), coords.double())
    if not include_self:
        d = d + torch.diag(torch.full((N,), float("inf"), dtype=d.dtype))
    d = torch.where(d < r, d, torch.full_like(d, float("inf")))
    kk = min(k, N)
    val, idx = torch.sort(d, dim=-1, stable=True)
    val, idx = val[..., :kk], idx[..., :kk]
    nb = torch.where(torch.isfinite(val), idx + (torch.arange(B) * N)[:, None, None], torch.full_like(idx, -1))
    if kk < k:
        nb = torch.cat((nb, torch.full((B, N, k - kk), -1, dtype=nb.dtype)), dim=-1)
    return nb.int()


def _inputs(B, N, F_, seed):
    gen = torch.Generator().manual_seed(seed)
    coords = torch.rand(B, N, 3, generator=gen) * 1.6 - 0.8
    feats = torch.randn(B, N, F_, generator=gen)
    mean = torch.randn(B, N, F_, generator=gen)
    log_var = torch.randn(B, N, F_, generator=gen) * 0.5 - 1.0
    return coords, feats, mean, log_var, gen


# ---- 1. parity with the oracle (float64) and the torch path ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["grid", "brute"])
def test_fused_losses_match_float64_oracle_no_worse_than_the_torch_path(golden, mode):
    from npcd.losses import NeuralPointCloudKLLoss, NeuralPointCloudTVLoss
    B, N, F_ = 2, 512, 32
    coords, feats = orr.synthetic_cloud(N, F_, B, seed=6)
    net = _model(F_, N)
    pn = net.pointnerf
    agg = pn.field.aggregator
    if mode == "brute":
        agg.voxel_grid = None
    pn.voxel_grid.set_pointset(coords.cuda(), torch.full((B,), N, dtype=torch.int, device="cuda"))
    gen = torch.Generator().manual_seed(1)
    mean, log_var = torch.randn(B, N, F_, generator=gen), torch.randn(B, N, F_, generator=gen) * 0.5 - 1.0
    # float64 yardstick: the oracle's TV loss (its query runs in fp32 like the kernels', everything behind it in float64) + the KL formula
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        fo = feats.double().requires_grad_(True)
        ref, ref_pw = otr.tv_loss(coords.double(), fo, agg.k, agg.r, 0.5, mode=mode)
        ref.backward()
    finally:
        torch.set_default_dtype(prev)
    mo, lo = mean.double().requires_grad_(True), log_var.double().requires_grad_(True)
    kref_pw = -0.5 * torch.sum(1 + lo - mo.pow(2) - lo.exp(), dim=-1) * 0.25
    kref = kref_pw.mean()
    kref.backward()
    out = {}
    for fused in (False, True):
        fd, md, ld = (t.cuda().requires_grad_(True) for t in (feats, mean, log_var))
        tot, _, pw = NeuralPointCloudTVLoss(net, weight=0.5, fused=fused)(None, None, {"feats": fd, "coords": coords.cuda()}, 0)
        ktot, _, kpw = NeuralPointCloudKLLoss(None, weight=0.25, fused=fused)(None, None, {"feats_mean": md, "feats_log_var": ld}, 0)
        (tot + ktot).backward()
        out[fused] = {"tv_tot": tot, "tv_pw": pw["00_neural_point_cloud_tv"], "dfeats": fd.grad, "kl_tot": ktot,
                      "kl_pw": kpw["00_neural_point_cloud_kl"], "dmean": md.grad, "dlog_var": ld.grad}
    want = {"tv_tot": ref, "tv_pw": ref_pw, "dfeats": fo.grad, "kl_tot": kref, "kl_pw": kref_pw, "dmean": mo.grad, "dlog_var": lo.grad}
    assert float(ref.detach()) > 0 and float(fo.grad.abs().max()) > 0
    got = out[True]
    np.testing.assert_allclose(float(got["tv_tot"]), float(ref), rtol=1e-4)
    np.testing.assert_allclose(got["tv_pw"].detach().cpu().numpy(), ref_pw.detach().numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(float(got["kl_tot"]), float(kref), rtol=1e-4)
    np.testing.assert_allclose(got["kl_pw"].detach().cpu().numpy(), kref_pw.detach().numpy(), rtol=1e-4, atol=1e-3)
    for key in ("dfeats", "dmean", "dlog_var"):
        _grad_close(got[key], want[key], f"{mode} {key}")
    for key, w in want.items():
        w = w.detach().double()
        err = {f: float((out[f][key].detach().cpu().double() - w).abs().max()) for f in (False, True)}
        print(f"[{mode}] {key}: |fused - float64| = {err[True]:.3e}, |torch path - float64| = {err[False]:.3e}, largest entry {float(w.abs().max()):.3e}")
        assert err[True] <= 2 * err[False] + 1e-6 * float(w.abs().max()), (mode, key, err)
    if mode == "grid":
        g = golden("losses")
        tot, _, pw = NeuralPointCloudKLLoss(None, weight=float(g["kl_weight"]), fused=True)(
            None, None, {"feats_mean": T(g["kl_mean"]).cuda(), "feats_log_var": T(g["kl_log_var"]).cuda()}, 0)
        np.testing.assert_allclose(float(tot), float(g["kl_total"]), rtol=1e-5)
        np.testing.assert_allclose(pw["00_neural_point_cloud_kl"].cpu().numpy(), g["kl_pointwise"], rtol=1e-5)


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,F_,k,r", [(1, 1, 32, 8, 0.5), (2, 65, 32, 8, 0.5), (1, 4096, 32, 8, 0.12), (2, 65, 1, 8, 0.5), (2, 65, 33, 8, 0.5),
                                        (2, 65, 32, 1, 0.5), (3, 130, 128, 5, 0.4)],
                         ids=["N1", "N65", "N4096", "F1", "F33", "k1", "B3_F128"])
def test_fused_losses_at_edge_shapes_match_the_torch_path(B, N, F_, k, r):
    coords, feats, mean, log_var, gen = _inputs(B, N, F_, seed=100 + N + F_ + k)
    nb = _cpu_lists(coords, k, r, include_self=k > 1).cuda()           # k = 1: the one entry is the nearest OTHER point
    if N > 1:
        assert int(((nb >= 0) & (nb != _own(B, N))).sum()) > B * N // 2, "the lists hold more than the points themselves"
    g = _upstream(B, N, gen)
    args = (coords.cuda(), nb, feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    _assert_matches_torch_path(_fused(*args), _torch_path(*args), f"B{B} N{N} F{F_} k{k}")


def _query_lists(coords, k=8, r=2, grid=True):
    """neighbour lists of the product's own query (npcd.losses.self_neighbour_lists) on the reference's grid configuration"""
    from npcd.hip.render import HipVoxelGrid
    from npcd.losses import self_neighbour_lists
    B, N = coords.shape[:2]
    vg = None
    if grid:
        vg = HipVoxelGrid((0.04,) * 3, (2,) * 3, (3,) * 3, 4, 5000, (-1, -1, -1, 1, 1, 1))
        vg.set_pointset(coords, torch.full((B,), N, dtype=torch.int, device="cuda"))
    return self_neighbour_lists(types.SimpleNamespace(voxel_grid=vg, k=k, r=r), coords), vg


def _own(B, N):
    return (torch.arange(N)[None, :, None] + (torch.arange(B) * N)[:, None, None]).cuda()


def test_duplicate_positions_with_different_features():
    """exact duplicates: distance 0, w = 1e5 -- the largest weight the formula can produce"""
    B, N, F_ = 2, 96, 32
    coords, feats, mean, log_var, gen = _inputs(B, N, F_, seed=7)
    coords = coords * 0.5
    coords[:, 1::2] = coords[:, 0::2]                                # every point has one exact duplicate
    nb, _ = _query_lists(coords.cuda(), grid=False, r=0.3)
    g = _upstream(B, N, gen)
    args = (coords.cuda(), nb, feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    got, ref = _fused(*args), _torch_path(*args)
    assert float(got["tv_pw"].min()) > 1e4, "every point sees its duplicate at w = 1e5"
    _assert_matches_torch_path(got, ref, "duplicates")


def test_lost_points_outside_the_grid_have_empty_lists():
    B, N, F_ = 2, 96, 32
    coords, feats, mean, log_var, gen = _inputs(B, N, F_, seed=8)
    coords = coords * 0.25                                                        # dense enough for neighbours inside 0.08
    coords[:, ::3] = coords[:, ::3] + 1.3 * torch.sign(coords[:, ::3])            # a third of the points outside +-1
    nb, _ = _query_lists(coords.cuda())
    empty = (nb < 0).all(dim=-1)
    assert bool(empty[:, ::3].all()) and int(((nb >= 0).sum(dim=-1) > 1).sum()) > 8
    g = _upstream(B, N, gen)
    args = (coords.cuda(), nb, feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    got, ref = _fused(*args), _torch_path(*args)
    assert float(got["tv_pw"][empty].abs().max()) == 0.0
    _assert_matches_torch_path(got, ref, "lost points")


def test_point_dropped_from_a_crowded_cell_finds_neighbours_and_not_itself():
    """more than four points in one 0.08 cell of the scaled grid: the fifth is dropped from the grid, yet its own query position
    lies in an occupied cell -- it finds the others and not itself"""
    B, N, F_ = 1, 64, 32
    coords, feats, mean, log_var, gen = _inputs(B, N, F_, seed=9)
    coords[0, :6] = torch.tensor([0.05, 0.05, 0.05]) + torch.rand(6, 3, generator=gen) * 0.06      # six points in the cell [0.04, 0.12)^3
    nb, vg = _query_lists(coords.cuda())
    assert vg.grid_level == "scaled"
    has_self = (nb == _own(B, N)).any(dim=-1)
    dropped = (~has_self) & (nb >= 0).any(dim=-1)
    assert bool(dropped[0, 4:6].all()) and not bool(dropped[0, :4].any()), "the fifth and sixth point of the cell have neighbours and not themselves"
    g = _upstream(B, N, gen)
    args = (coords.cuda(), nb, feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    _assert_matches_torch_path(_fused(*args), _torch_path(*args), "crowded cell")


def test_entries_of_another_cloud_or_past_the_end_are_padding():
    B, N, F_, k = 2, 65, 32, 8
    coords, feats, mean, log_var, gen = _inputs(B, N, F_, seed=10)
    clean = _cpu_lists(coords, k, 0.6)
    assert int((clean[:, :, 3] >= 0).sum()) > 0
    bad = clean.clone()
    bad[0, :, 2] = torch.arange(N, dtype=torch.int32) + N                # cloud 0 names points of cloud 1
    bad[1, :, 3] = B * N + torch.arange(N, dtype=torch.int32) * 1000      # past the end of every table
    bad[1, 0, 4] = 2 ** 31 - 1
    bad[1, 1, 4] = 5                                                      # cloud 1 names a point of cloud 0
    clean[0, :, 2] = -1
    clean[1, :, 3] = -1
    clean[1, :2, 4] = -1
    g = _upstream(B, N, gen)
    a = _fused(coords.cuda(), bad.cuda(), feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    b = _fused(coords.cuda(), clean.cuda(), feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    torch.cuda.synchronize()
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_strided_slot_view_gives_the_bits_of_a_contiguous_copy():
    B, N, F_, k = 2, 65, 32, 8
    coords, feats, mean, log_var, gen = _inputs(B, N, F_, seed=11)
    dense = torch.full((B, N, 50, k), -7, dtype=torch.int32)
    dense[:, :, 0] = _cpu_lists(coords, k, 0.6)
    view = dense.cuda()[:, :, 0]
    assert not view.is_contiguous()
    # the mean / log-variance halves of an embedding row are strided views too
    table = torch.cat((mean, log_var), dim=-1).cuda()
    g = _upstream(B, N, gen)
    a = _fused(coords.cuda(), view, feats.cuda(), table[..., :F_], table[..., F_:], 0.5, 0.25, g)
    b = _fused(coords.cuda(), view.contiguous(), feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    for key in a:
        assert torch.equal(a[key], b[key]), key


# ---- 3. reproducibility -------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    B, N, F_, k = 3, 512, 32, 8
    coords, feats, mean, log_var, gen = _inputs(B, N, F_, seed=12)
    nb = _cpu_lists(coords, k, 0.25).cuda()
    g = _upstream(B, N, gen)
    args = (coords.cuda(), nb, feats.cuda(), mean.cuda(), log_var.cuda(), 0.5, 0.25, g)
    a, b = _fused(*args), _fused(*args)
    assert float(a["dfeats"].abs().max()) > 0
    for key in a:
        assert torch.equal(a[key], b[key]), key


# ---- 4. no host wait ----------------------------------------------------------------------------------------------------------------
def test_fused_regularisers_do_not_wait_on_the_host():
    from npcd.losses import PointNeRFLoss
    from npcd.utils import AttrDict
    B, N, F_ = 2, 512, 32
    coords, feats = orr.synthetic_cloud(N, F_, B, seed=6)
    net = _model(F_, N)
    net.pointnerf.voxel_grid.set_pointset(coords.cuda(), torch.full((B,), N, dtype=torch.int, device="cuda"))
    loss = PointNeRFLoss(net, 1, 1e-7, 3.5e-7, fused_regularisers=True)
    table = torch.randn(B, N, 2 * F_, device="cuda").requires_grad_(True)
    aux = {"coords": coords.cuda(), "feats": table[..., :F_], "feats_mean": table[..., :F_], "feats_log_var": table[..., F_:]}
    img = torch.rand(B, 1, 3, 8, 8, device="cuda")
    pred = AttrDict(channels=torch.rand(B, 1, 64, 3, device="cuda"))
    total, sub, _ = loss({"images": img}, pred, aux, 0)                  # warm-up: first launches load the code objects
    total.backward()
    torch.cuda.synchronize()
    mask = torch.rand(64, device="cuda") > 0.5
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tripped = False
        try:
            torch.nonzero(mask)
        except RuntimeError:
            tripped = True
        if tripped:
            table.grad = None
            total, sub, _ = loss({"images": img}, pred, aux, 0)
            total.backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not tripped:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not trip on torch.nonzero on this torch build")
    assert set(sub) == {"00_image_reconstruction_loss", "01_neural_point_cloud_kl", "02_neural_point_cloud_tv"}
    assert float(table.grad.abs().max()) > 0 and float(sub["02_neural_point_cloud_tv"]) > 0


# ---- 5. trainer level -----------------------------------------------------------------------------------------------------------------
def test_trainer_with_fused_losses_follows_the_torch_path():
    """2 objects x 2 views, 64 points, 32^2 images, three steps from the same state and the same random draws, fused_losses on and off:
    every sub loss of every step within rtol 1e-4, the updated feature table (and what the three steps changed in it) within the
    relative-L2 rule of the gradients."""
    from npcd.train import PointNeRFTrainer
    B, Tn, N, F_, res = 2, 2, 64, 32, 32
    coords, feats = orr.synthetic_cloud(N, F_, B, seed=5)
    extr = torch.stack([orr.look_at_pose(40 + 70 * i, 10) for i in range(Tn)])[None].expand(B, -1, -1, -1).contiguous().cuda()
    K = orr.srn_intrinsics().clone()
    K[0, 0] = K[1, 1] = 131.25 * res / 128
    K[0, 2] = K[1, 2] = res / 2
    intr = K[None, None].expand(B, Tn, 3, 3).contiguous().cuda()
    sample = {"images": torch.rand(B, Tn, 3, res, res, generator=torch.Generator().manual_seed(3)).cuda(), "intrinsics": intr, "extrinsics": extr,
              "obj_idx": torch.arange(B, device="cuda")}
    start = torch.cat((feats, torch.full_like(feats, -4.0)), dim=-1).reshape(B, -1)
    result = {}
    for fused in (False, True):
        net = _model(F_, N, n_obj=B)
        pn = net.pointnerf
        pn.opt.sizes.default_resolution = res
        pn.set_all_coords(coords.cuda())
        with torch.no_grad():
            pn.feats.get_emb().weight.copy_(start)
        trainer = PointNeRFTrainer(net, fused_losses=fused)
        assert ("csrc/stage1_losses.hip" in trainer.describe()) == fused, trainer.describe()
        torch.manual_seed(0)
        subs = [trainer.step(sample)[1] for _ in range(3)]
        result[fused] = ([{k: float(v) for k, v in s.items()} for s in subs], pn.feats.get_emb().weight.detach().clone())
    for step, (a, b) in enumerate(zip(result[True][0], result[False][0])):
        assert set(a) == set(b) == {"00_image_reconstruction_loss", "01_neural_point_cloud_kl", "02_neural_point_cloud_tv"}
        for key in a:
            print(f"step {step} {key}: fused {a[key]:.9e} torch path {b[key]:.9e}")
            np.testing.assert_allclose(a[key], b[key], rtol=1e-4, err_msg=f"step {step} {key}")
        assert a["02_neural_point_cloud_tv"] > 0
    moved = float((result[False][1].cpu() - start).abs().max())
    assert moved > 0
    _grad_close(result[True][1], result[False][1], "feature table")
    _grad_close(result[True][1].cpu() - start, result[False][1].cpu() - start, "change of the feature table")


# ---- 6. loud failures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["N4097", "F129", "float64", "pairs"])
def test_unsupported_inputs_raise(case):
    from npcd.hip.losses import stage1_regularisers
    B, N, F_, k, dt = {"N4097": (1, 4097, 4, 2, torch.float32), "F129": (1, 8, 129, 2, torch.float32),
                       "float64": (1, 8, 4, 2, torch.float64), "pairs": (1, 4096, 4, 9, torch.float32)}[case]
    coords = torch.zeros(B, N, 3, device="cuda", dtype=dt)
    feats = torch.zeros(B, N, F_, device="cuda", dtype=dt)
    nb = torch.full((B, N, k), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        stage1_regularisers(coords, nb, feats, feats, feats)
    if case != "float64":
        # the library's own launcher refuses the same shapes before any launch
        from npcd import hip
        rc = hip.lib().npcd_stage1_reg_fwd(hip.ptr(coords), hip.ptr(nb), k, hip.ptr(feats), F_, None, None, 0, B, N, k, F_, 1.0, 1.0, hip.NPCD_F32,
                                           hip.ptr(feats), hip.ptr(feats), None, None, hip.ptr(feats), hip.stream_ptr())
        assert rc == -2, rc
    else:
        from npcd import hip
        f32 = torch.zeros(B, N, F_, device="cuda")
        rc = hip.lib().npcd_stage1_reg_fwd(hip.ptr(f32), hip.ptr(nb), k, hip.ptr(f32), F_, None, None, 0, B, N, k, F_, 1.0, 1.0, hip.NPCD_BF16,
                                           hip.ptr(f32), hip.ptr(f32), None, None, hip.ptr(f32), hip.stream_ptr())
        assert rc == -2, rc
