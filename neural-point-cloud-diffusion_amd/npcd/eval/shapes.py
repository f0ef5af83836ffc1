"""Shape metrics of generated point clouds: MMD-CD, COV-CD and 1-NNA-CD (Achlioptas et al. 2018; Yang et al. 2019, PointFlow) between a
generated set and a reference set, through the all-pairs Chamfer kernel of npcd/hip/chamfer.py.  They need no outside
assets: the reference set can be the stage-1 clouds (`model.pointnerf.get_all_coords()`) or the subsampled dataset clouds of
npcd/data/pointclouds.py.

Definitions follow PointFlow's evaluation: squared distances, means over points, CD(X, Y) = mean_x min_y d + mean_y min_x d.
  MMD-CD    mean over the reference clouds of the distance to the nearest generated cloud            (lower is better)
  COV-CD    share of the reference clouds that are the nearest reference of some generated cloud      (higher is better)
  1-NNA-CD  leave-one-out accuracy of the 1-nearest-neighbour classifier "generated or reference?" on the union (0.5 is best)
The fourth number of that protocol is set-level and pairs no clouds: JSD, the Jensen-Shannon divergence between the occupancy
distributions of the two sets on a lattice, through the occupancy-grid kernel of npcd/hip/occupancy.py.
  JSD       base-2 Jensen-Shannon divergence of the two point-per-cell histograms, in [0, 1]                 (lower is better)
This module imports without a GPU; only `shape_metrics`, `jensen_shannon_divergence` and `evaluate_shapes` need one.
"""
import time
from typing import Dict, Optional

import torch


def _first_argmin(m: torch.Tensor) -> torch.Tensor:
    """Row-wise arg-min, the LOWEST index among equal minima (torch.argmin does not promise which one it returns)."""
    cols = torch.arange(m.shape[1], device=m.device)
    return torch.where(m == m.min(dim=1, keepdim=True).values, cols, m.shape[1]).min(dim=1).values


def _reduce(cd_union: torch.Tensor, num_generated: int, who: str):
    """The three reductions on a symmetric distance matrix of the union set -> (mmd, matched, correct, M, N)."""
    if cd_union.dim() != 2 or cd_union.shape[0] != cd_union.shape[1]:
        raise ValueError(f"{who}: cd_union must be square; got {tuple(cd_union.shape)}")
    T, M = cd_union.shape[0], int(num_generated)
    N = T - M
    if M < 1 or N < 1:
        raise ValueError(f"{who}: {M} generated and {N} reference clouds in a union of {T}")
    cd = cd_union.detach().double()
    gen_ref = cd[:M, M:]
    mmd = gen_ref.min(dim=0).values.mean()
    hit = torch.zeros(N, dtype=torch.float64, device=cd.device)
    hit[_first_argmin(gen_ref)] = 1.0
    others = cd.clone()
    others.fill_diagonal_(float("inf"))
    nearest = _first_argmin(others)
    side = torch.arange(T, device=cd.device) < M
    correct = (side[nearest] == side).double().sum()
    mmd, matched, correct = torch.stack([mmd, hit.sum(), correct]).tolist()
    return mmd, int(round(matched)), int(round(correct)), M, N


def metrics_from_chamfer(cd_union: torch.Tensor, num_generated: int) -> Dict:
    """cd_union [T, T]: the symmetric Chamfer matrix of the union set, rows and columns [:M] the generated clouds, [M:] the N
    reference clouds (M = num_generated).  Device-agnostic torch; the reductions run in float64, ties go to the lowest index, one
    small host read at the end.  -> mmd_cd, cov_cd = cov_matched / N, nna_cd = nna_correct / (M + N), the two counts, num_generated,
    num_reference."""
    mmd, matched, correct, M, N = _reduce(cd_union, num_generated, "metrics_from_chamfer")
    return {"mmd_cd": mmd, "cov_cd": matched / N, "nna_cd": correct / (M + N), "cov_matched": matched, "nna_correct": correct,
            "num_generated": M, "num_reference": N}


def metrics_from_distance(matrix: torch.Tensor, num_generated: int, name: str) -> Dict:
    """The reductions of `metrics_from_chamfer` on the symmetric union matrix of any distance, keys suffixed with `name`:
    mmd_<name>, cov_<name>, nna_<name>, cov_matched_<name>, nna_correct_<name>, and num_generated, num_reference."""
    mmd, matched, correct, M, N = _reduce(matrix, num_generated, "metrics_from_distance")
    return {f"mmd_{name}": mmd, f"cov_{name}": matched / N, f"nna_{name}": correct / (M + N), f"cov_matched_{name}": matched,
            f"nna_correct_{name}": correct, "num_generated": M, "num_reference": N}


def normalize_clouds(clouds: torch.Tensor, mode: Optional[str] = "bbox") -> torch.Tensor:
    """clouds [n, P, 3].  mode "bbox": every cloud shifted by the centre of its axis-aligned bounding box and divided by half its
    longest side (it then fits [-1, 1]^3 and touches it on one axis).  None: unchanged.  Plain torch."""
    if mode is None:
        return clouds
    if mode != "bbox":
        raise ValueError(f"normalize_clouds: unknown mode {mode!r} (None or 'bbox')")
    if clouds.dim() != 3 or clouds.shape[2] != 3:
        raise ValueError(f"normalize_clouds: clouds must be [n, P, 3]; got {tuple(clouds.shape)}")
    lo, hi = clouds.min(dim=1, keepdim=True).values, clouds.max(dim=1, keepdim=True).values
    half = (hi - lo).max(dim=2, keepdim=True).values * 0.5
    return (clouds - (lo + hi) * 0.5) / half


def _union_matrix(mod, matrix: str, directed: str, combine, generated, reference, gen_lengths, ref_lengths):
    """The symmetric matrix of the union set from the kernels of `mod` (looked up at the call): one launch when P = Q and no lengths
    are given, else the four directed blocks, the cross block `combine`d from its two directions."""
    matrix, directed = getattr(mod, matrix), getattr(mod, directed)
    if generated.dim() == 3 and generated.shape[1:] == reference.shape[1:] and gen_lengths is None and ref_lengths is None:
        return matrix(torch.cat([generated, reference]))
    gg = matrix(generated, None, gen_lengths)
    rr = matrix(reference, None, ref_lengths)
    gr = combine(directed(generated, reference, gen_lengths, ref_lengths), directed(reference, generated, ref_lengths, gen_lengths).t())
    return torch.cat([torch.cat([gg, gr], dim=1), torch.cat([gr.t(), rr], dim=1)])


def _emd_metrics(generated, reference, gen_lengths, ref_lengths) -> Dict:
    """The EMD keys of `shape_metrics` on clouds that are already normalised."""
    from ..hip import emd as emd_mod
    return metrics_from_distance(_union_matrix(emd_mod, "emd_matrix", "emd_directed", lambda a, b: 0.5 * (a + b), generated, reference,
                                               gen_lengths, ref_lengths), generated.shape[0], "emd")


def _entropy_bits(p: torch.Tensor) -> torch.Tensor:
    """Base-2 entropy of a float64 distribution, 0 log 0 = 0."""
    return -(p * torch.where(p > 0, p, torch.ones_like(p)).log2()).sum()


def jsd_from_counts(a: torch.Tensor, b: torch.Tensor) -> float:
    """The Jensen-Shannon divergence of two histograms of one shape (counts, any integer or float dtype, any device):
    H((p + q) / 2) - (H(p) + H(q)) / 2 with p = a / sum a, q = b / sum b and H the base-2 entropy, 0 log 0 = 0; float64, one small
    host read at the end.  In [0, 1]: 0.0 for equal histograms (then (p + q) / 2 is p, bit for bit), 1 for disjoint supports."""
    if a.shape != b.shape:
        raise ValueError(f"jsd_from_counts: the two histograms differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    sa, sb = a.sum(), b.sum()
    p, q = a / sa, b / sb
    value = _entropy_bits(0.5 * (p + q)) - 0.5 * (_entropy_bits(p) + _entropy_bits(q))
    sa, sb, value = torch.stack([sa, sb, value]).tolist()
    if not (sa > 0 and sb > 0):
        raise ValueError(f"jsd_from_counts: a histogram is empty (sums {sa:g} and {sb:g})")
    return min(max(value, 0.0), 1.0)


def occupancy_entropy(cloud_counts: torch.Tensor, num_clouds: int, mask: torch.Tensor) -> float:
    """The occupancy entropy of Achlioptas et al.: cloud_counts[cell] = c clouds of num_clouds = n have a point in the cell, a
    Bernoulli variable of entropy -(c / n) ln(c / n) - (1 - c / n) ln(1 - c / n) (natural logarithm); summed over the cells with
    c > 0 and divided by the number of valid cells (`mask`, bool, the shape of cloud_counts).  float64."""
    if cloud_counts.shape != mask.shape:
        raise ValueError(f"occupancy_entropy: counts {tuple(cloud_counts.shape)} and mask {tuple(mask.shape)} differ in shape")
    n, valid = int(num_clouds), int(mask.sum())
    if n < 1 or valid < 1:
        raise ValueError(f"occupancy_entropy: {n} clouds and {valid} valid cells")
    p = cloud_counts.detach().double().reshape(-1) / n
    q = 1.0 - p
    h = -(p * torch.where(p > 0, p, torch.ones_like(p)).log() + q * torch.where(q > 0, q, torch.ones_like(q)).log())
    return float(h.sum()) / valid


def _jsd_metrics(generated, reference, resolution, extent, in_sphere, gen_lengths, ref_lengths) -> Dict:
    from ..hip import occupancy as occ
    mask = occ.grid_mask(resolution, extent, in_sphere)
    g_points, g_clouds = occ.occupancy_grid(generated, gen_lengths, resolution, extent, in_sphere)
    r_points, r_clouds = occ.occupancy_grid(reference, ref_lengths, resolution, extent, in_sphere)
    occupied_g, occupied_r = torch.stack([(g_points > 0).sum(), (r_points > 0).sum()]).tolist()
    return {"jsd": jsd_from_counts(g_points, r_points),
            "occupancy_entropy_generated": occupancy_entropy(g_clouds, generated.shape[0], mask),
            "occupancy_entropy_reference": occupancy_entropy(r_clouds, reference.shape[0], mask),
            "occupied_cells_generated": int(occupied_g), "occupied_cells_reference": int(occupied_r)}


def jensen_shannon_divergence(generated: torch.Tensor, reference: torch.Tensor, resolution: int = 28, extent: float = 0.5,
                              in_sphere: bool = True, gen_lengths=None, ref_lengths=None) -> Dict:
    """generated [M, P, 3], reference [N, Q, 3] fp32 on the GPU -> jsd, the Jensen-Shannon divergence between the two sets'
    points-per-cell histograms on the `resolution`^3 lattice of half-width `extent` (its cells inside the inscribed sphere when
    in_sphere, the protocol's default: points outside go to the nearest cell inside); occupancy_entropy_generated / _reference,
    the protocol's occupancy entropy of either set; occupied_cells_generated / _reference, the cells holding a point.  One launch of
    npcd.hip.occupancy per set; lengths as for `shape_metrics`.  The clouds are taken as they are: the protocol's
    extent 0.5 expects them in the unit cube."""
    return _jsd_metrics(generated, reference, resolution, extent, in_sphere, gen_lengths, ref_lengths)


def _jsd_extent(jsd_extent, normalize) -> float:
    return (1.0 if normalize == "bbox" else 0.5) if jsd_extent is None else jsd_extent


def shape_metrics(generated: torch.Tensor, reference: torch.Tensor, normalize: Optional[str] = None, gen_lengths=None,
                  ref_lengths=None, emd: bool = False, jsd: bool = False, jsd_resolution: int = 28, jsd_extent: Optional[float] = None) -> Dict:
    """generated [M, P, 3], reference [N, Q, 3] fp32 on the GPU (P != Q allowed), optional valid lengths per cloud as for
    npcd.hip.chamfer -> the dict of `metrics_from_chamfer`.  One kernel launch on the union set when P = Q and no lengths are given,
    the four directed blocks otherwise.  `normalize` is applied to whole clouds and so cannot be combined with lengths.
    emd = True adds mmd_emd, cov_emd, nna_emd, cov_matched_emd and nna_correct_emd, the same reductions on the approximate earth
    mover's distance of npcd.hip.emd (clouds of up to 2,048 points), computed the same way; the other keys are
    untouched.
    jsd = True adds the keys of `jensen_shannon_divergence` on the (normalised) clouds, lattice resolution `jsd_resolution` and
    half-width `jsd_extent`; None means 1.0 under normalize="bbox" (those clouds fill [-1, 1]^3) and 0.5 otherwise.  The other keys
    are untouched."""
    from ..hip import chamfer as chamfer_mod
    if normalize is not None:
        if gen_lengths is not None or ref_lengths is not None:
            raise ValueError("shape_metrics: normalize works on whole clouds; normalise the valid rows yourself when lengths are given")
        generated, reference = normalize_clouds(generated, normalize), normalize_clouds(reference, normalize)
    M = generated.shape[0]
    out = metrics_from_chamfer(_union_matrix(chamfer_mod, "chamfer_matrix", "chamfer_directed", lambda a, b: a + b, generated,
                                             reference, gen_lengths, ref_lengths), M)
    if emd:
        out.update(_emd_metrics(generated, reference, gen_lengths, ref_lengths))
    if jsd:
        out.update(_jsd_metrics(generated, reference, jsd_resolution, _jsd_extent(jsd_extent, normalize), True, gen_lengths, ref_lengths))
    return out


@torch.no_grad()
def evaluate_shapes(model, reference: torch.Tensor, num_samples: int, generate_batch_size: int = 8, normalize: Optional[str] = None,
                    return_clouds: bool = False, emd: bool = False, jsd: bool = False, **generate_kwargs) -> Dict:
    """Sample `num_samples` clouds with model.diffusion.generate (`model`: an NPCD, or its DiffusionModel itself;
    `generate_batch_size` at a time; dtype, use_graph, sampling_steps, eta ... pass through untouched) and compare their shape
    halves with `reference` [N, Q, 3].  -> the dict of
    `shape_metrics` plus generate_seconds / metric_seconds (device-synchronised walls) and, with return_clouds, `clouds` [M, P, 3].
    emd = True adds the EMD keys of `shape_metrics` and emd_seconds, the wall of the EMD part alone (metric_seconds stays the
    wall of the Chamfer part).  jsd = True adds the keys of `jensen_shannon_divergence` (28^3 lattice, the extent that
    `shape_metrics` takes for `normalize`) and jsd_seconds, the wall of that part alone."""
    model.eval()
    sampler = getattr(model, "diffusion", model)
    dev = next(sampler.parameters()).device
    clouds = []
    t_gen = 0.0
    for s0 in range(0, num_samples, generate_batch_size):
        n = min(generate_batch_size, num_samples - s0)
        torch.cuda.synchronize()
        t0 = time.time()
        coords, _ = sampler.generate(num=n, batch_size=n, progress=False, **generate_kwargs)
        torch.cuda.synchronize()
        t_gen += time.time() - t0
        clouds.append(torch.stack(list(coords)).permute(0, 2, 1))          # [n, 3, P] -> [n, P, 3]
    generated = torch.cat(clouds).float().contiguous()
    torch.cuda.synchronize()
    t0 = time.time()
    out = shape_metrics(generated, reference.to(dev).float(), normalize=normalize)
    torch.cuda.synchronize()
    out.update(generate_seconds=t_gen, metric_seconds=time.time() - t0)
    if emd:
        t0 = time.time()
        out.update(_emd_metrics(normalize_clouds(generated, normalize), normalize_clouds(reference.to(dev).float(), normalize), None, None))
        torch.cuda.synchronize()
        out["emd_seconds"] = time.time() - t0
    if jsd:
        t0 = time.time()
        out.update(_jsd_metrics(normalize_clouds(generated, normalize), normalize_clouds(reference.to(dev).float(), normalize), 28,
                                _jsd_extent(None, normalize), True, None, None))
        torch.cuda.synchronize()
        out["jsd_seconds"] = time.time() - t0
    if return_clouds:
        out["clouds"] = generated
    return out
