"""The stage-1 regularisers on their own kernels (csrc/stage1_losses.hip): the TV loss over each point's neighbour list and the KL
loss of the variational feature embedding, one launch forward (plus its one-wave fixed-order sum of the clouds) and one backward,
with no host wait anywhere: the lists are read in place with their -1 padding, nothing is compacted, no count reaches the host.

There is no CPU fallback: a non-GPU tensor, a dtype other than fp32 or a shape outside the kernels' set raises RuntimeError.
"""
from typing import Optional

import torch

from . import NPCD_F32, check, lib, ptr, require_gpu, stream_ptr

MAX_POINTS, MAX_PAIRS, MAX_FEATS = 4096, 32768, 128          # csrc/stage1_losses.hip: N, k N, F


def _rows(t: torch.Tensor, B: int, N: int):
    """[B, N, F] tensor -> (tensor to read, row stride in elements): a view whose rows are evenly spaced in memory (a column slice of
    the embedding table, slot 0 of the dense query result) is read in place, anything else through a contiguous copy."""
    if t.stride(2) == 1 and t.stride(1) >= t.shape[2] and (B == 1 or t.stride(0) == N * t.stride(1)):
        return t, t.stride(1)
    t = t.contiguous()
    return t, t.shape[2]


def _validate(coords, nb, feats, mean, log_var):
    if (nb is None) != (feats is None) or (mean is None) != (log_var is None) or (nb is None and mean is None):
        raise ValueError("stage1_regularisers: give (coords, nb, feats) for the TV term and / or (mean, log_var) for the KL term")
    require_gpu(coords, nb, feats, mean, log_var)
    lead = feats if feats is not None else mean
    if lead.dim() != 3:
        raise RuntimeError(f"stage1_regularisers: unsupported shape {tuple(lead.shape)}; expected [B, N, F]")
    B, N, F_ = lead.shape
    for name, t in (("coords", coords if nb is not None else None), ("feats", feats), ("feats_mean", mean), ("feats_log_var", log_var)):
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError(f"stage1_regularisers: unsupported dtype {t.dtype} of {name} (the kernels are fp32)")
        want = (B, N, 3) if name == "coords" else (B, N, F_)
        if tuple(t.shape) != want:
            raise RuntimeError(f"stage1_regularisers: unsupported shape {tuple(t.shape)} of {name}; expected {want}")
    k = 0
    if nb is not None:
        if nb.dtype != torch.int32 or nb.dim() != 3 or tuple(nb.shape[:2]) != (B, N) or nb.shape[2] < 1:
            raise RuntimeError(f"stage1_regularisers: unsupported neighbour lists {nb.dtype} {tuple(nb.shape)}; expected int32 [B, N, k]")
        k = nb.shape[2]
    if N < 1 or N > MAX_POINTS or F_ < 1 or F_ > MAX_FEATS or k * N > MAX_PAIRS:
        raise RuntimeError(f"stage1_regularisers: unsupported shape N={N}, k={k}, F={F_} (N <= {MAX_POINTS}, k N <= {MAX_PAIRS}, "
                           f"F <= {MAX_FEATS})")
    return B, N, F_, k


class _Stage1Regularisers(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, nb, feats, mean, log_var, weight_tv, weight_kl):
        B, N, F_, k = _validate(coords, nb, feats, mean, log_var)
        dev = (feats if feats is not None else mean).device
        f32 = torch.float32
        nb_ld = feats_ld = kl_ld = 0
        if nb is not None:
            coords = coords.detach().contiguous()
            nb, nb_ld = _rows(nb, B, N)
            feats, feats_ld = _rows(feats.detach(), B, N)
        if mean is not None:
            mean, kl_ld = _rows(mean.detach(), B, N)
            log_var, lv_ld = _rows(log_var.detach(), B, N)
            if lv_ld != kl_ld:
                mean, log_var, kl_ld = mean.contiguous(), log_var.contiguous(), F_
        tv_pw = tv_tot = kl_pw = kl_tot = None
        if nb is not None:
            tv_pw, tv_tot = torch.empty((B, N), dtype=f32, device=dev), torch.empty((), dtype=f32, device=dev)
        if mean is not None:
            kl_pw, kl_tot = torch.empty((B, N), dtype=f32, device=dev), torch.empty((), dtype=f32, device=dev)
        L = lib()
        ws = torch.empty(L.npcd_stage1_reg_workspace_floats(B), dtype=f32, device=dev)
        with torch.cuda.device(dev):
            check(L.npcd_stage1_reg_fwd(ptr(coords if nb is not None else None), ptr(nb), nb_ld, ptr(feats), feats_ld, ptr(mean), ptr(log_var),
                                        kl_ld, B, N, k, F_, float(weight_tv), float(weight_kl), NPCD_F32, ptr(tv_pw), ptr(tv_tot), ptr(kl_pw),
                                        ptr(kl_tot), ptr(ws), stream_ptr()), "npcd_stage1_reg_fwd")
        ctx.save_for_backward(coords if nb is not None else None, nb, feats, mean, log_var)
        ctx.geom = (B, N, F_, k, nb_ld, feats_ld, kl_ld, float(weight_tv), float(weight_kl))
        ctx.set_materialize_grads(False)
        return tv_tot, tv_pw, kl_tot, kl_pw

    @staticmethod
    def backward(ctx, g_tv_tot, g_tv_pw, g_kl_tot, g_kl_pw):
        coords, nb, feats, mean, log_var = ctx.saved_tensors
        B, N, F_, k, nb_ld, feats_ld, kl_ld, weight_tv, weight_kl = ctx.geom
        f32 = torch.float32
        want_tv = nb is not None and ctx.needs_input_grad[2]
        want_kl = mean is not None and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        if not want_tv and not want_kl:
            return (None,) * 7
        dev = (feats if feats is not None else mean).device
        g = [None if t is None else t.to(f32).contiguous() for t in (g_tv_tot, g_tv_pw, g_kl_tot, g_kl_pw)]
        dfeats = torch.empty((B, N, F_), dtype=f32, device=dev) if want_tv else None
        dmean = torch.empty((B, N, F_), dtype=f32, device=dev) if want_kl else None
        dlv = torch.empty((B, N, F_), dtype=f32, device=dev) if want_kl else None
        with torch.cuda.device(dev):
            check(lib().npcd_stage1_reg_bwd(ptr(coords if want_tv else None), ptr(nb if want_tv else None), nb_ld, ptr(feats if want_tv else None),
                                            feats_ld, ptr(mean if want_kl else None), ptr(log_var if want_kl else None), kl_ld, B, N, k, F_,
                                            weight_tv, weight_kl, NPCD_F32, ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(dfeats), ptr(dmean),
                                            ptr(dlv), stream_ptr()), "npcd_stage1_reg_bwd")
        return (None, None, dfeats, dmean if ctx.needs_input_grad[3] else None, dlv if ctx.needs_input_grad[4] else None, None, None)


def stage1_regularisers(coords: Optional[torch.Tensor] = None, nb: Optional[torch.Tensor] = None, feats: Optional[torch.Tensor] = None,
                        feats_mean: Optional[torch.Tensor] = None, feats_log_var: Optional[torch.Tensor] = None,
                        weight_tv: float = 1.0, weight_kl: float = 1.0):
    """-> (tv_total [], tv_pointwise [B, N], kl_total [], kl_pointwise [B, N]); the pair of a term that was not asked for is None.

    TV term: coords [B, N, 3] (no gradient: detached like the reference's), nb [B, N, k] int32 global indices b N + j padded with -1
    (may be the strided view idx[:, :, 0] of a dense query result [B, N, M, k]), feats [B, N, F].  An entry of a list is skipped when
    it is negative, the point itself, or outside its own cloud.  KL term: feats_mean / feats_log_var [B, N, F].
    fp32, N <= 4096, k N <= 32768, F <= 128; differentiable w.r.t. feats, feats_mean and feats_log_var."""
    return _Stage1Regularisers.apply(coords, nb, feats, feats_mean, feats_log_var, weight_tv, weight_kl)
