"""Connected components of a density volume above a level on their own kernels (csrc/components.hip): what drops the
floaters from a volume before it is meshed.  `connected_components_reference`, `select_components` and
`filter_components_reference` of npcd/eval/mesh.py restate the specification on the CPU.

Two inside nodes (volume > level, NaN outside) are adjacent iff they are the two ends of one edge of the isosurface's Kuhn
triangulation: 14 neighbours a node.  Integer minima and additions only: the same volume gives the same bits on every run.  There is
no CPU fallback: a non-GPU tensor or a dtype other than fp32 raises RuntimeError.
"""
from typing import List, Optional, Tuple

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

# the brick of nodes (x, y, z) a workgroup labels in LDS (kCcBrickX, kCcBrickY, kCcBrickZ of csrc/components.h)
BRICK = (16, 8, 8)


def workspace_bytes(B: int, gz: int, gy: int, gx: int) -> int:
    """Bytes of device workspace for B volumes of gz x gy x gx nodes."""
    got = lib().npcd_components_ws_bytes(B, gz, gy, gx)
    check(min(got, 0), "npcd_components_ws_bytes")
    return got


def _batch(volume, who: str) -> torch.Tensor:
    if not isinstance(volume, torch.Tensor) or volume.dim() not in (3, 4):
        raise ValueError(f"{who}: volume must be a tensor [B, Gz, Gy, Gx] or [Gz, Gy, Gx]")
    require_gpu(volume)
    if volume.dtype != torch.float32:
        raise RuntimeError(f"{who}: the volume must be fp32; got {volume.dtype}")
    vol = (volume if volume.dim() == 4 else volume[None]).detach().contiguous()
    B, gz, gy, gx = vol.shape
    if min(B, gz, gy, gx) < 1 or min(gz, gy, gx) < 2:
        raise ValueError(f"{who}: every axis needs at least 2 nodes; got {tuple(vol.shape)}")
    return vol


def _label(vol: torch.Tensor, level: float) -> Tuple[torch.Tensor, torch.Tensor]:
    B, gz, gy, gx = vol.shape
    with torch.cuda.device(vol.device):
        ws = torch.empty(workspace_bytes(B, gz, gy, gx), dtype=torch.uint8, device=vol.device)
        labels = torch.empty(vol.shape, dtype=torch.int32, device=vol.device)
        sizes = torch.empty(vol.shape, dtype=torch.int32, device=vol.device)
        check(lib().npcd_components_label(ptr(vol), B, gz, gy, gx, float(level), ptr(ws), ptr(labels), ptr(sizes), stream_ptr()),
              "npcd_components_label")
    return labels, sizes


def label_components(volume: torch.Tensor, level: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """volume [B, Gz, Gy, Gx] or [Gz, Gy, Gx] fp32 on the GPU, x fastest -> (labels, sizes), int32 of the volume's shape.

    labels: -1 where volume > level does not hold, otherwise the smallest node index (z Gy + y) Gx + x of the node's component, local
    to its volume.  sizes: the component's number of nodes at its root node, 0 everywhere else.  Every axis has at least 2 nodes and
    Gz Gy Gx < 2^31."""
    labels, sizes = _label(_batch(volume, "label_components"), level)
    return (labels, sizes) if volume.dim() == 4 else (labels[0], sizes[0])


def filter_components_counted(volume: torch.Tensor, level: float, largest: Optional[int] = None,
                              min_nodes: Optional[int] = None) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """filter_components, and per volume of the batch the kept components' node counts in descending order (int64, on the GPU)."""
    if largest is not None and int(largest) < 1:
        raise ValueError(f"filter_components: largest must be at least 1; got {largest}")
    if min_nodes is not None and int(min_nodes) < 1:
        raise ValueError(f"filter_components: min_nodes must be at least 1; got {min_nodes}")
    vol = _batch(volume, "filter_components")
    labels, sizes = _label(vol, level)
    B, n = vol.shape[0], vol[0].numel()
    removed = torch.empty(vol.shape, dtype=torch.bool, device=vol.device)
    kept_nodes = []
    for b in range(B):
        size = sizes[b].reshape(-1).to(torch.int64)
        roots = torch.nonzero(size > 0)[:, 0]
        # candidates by one integer key of (-size, root): the keys are distinct, so no tie rule of a sort is relied on
        order = torch.sort((n - size[roots]) * n + roots)[1]
        if largest is not None:
            order = order[:int(largest)]
        kept = roots[order]
        if min_nodes is not None:
            kept = kept[size[kept] >= int(min_nodes)]
        kept_nodes.append(size[kept])
        keep_root = torch.zeros(n, dtype=torch.bool, device=vol.device)
        keep_root[kept] = True
        label = labels[b].to(torch.int64)
        removed[b] = (label >= 0) & ~keep_root[label.clamp(min=0).reshape(-1)].reshape(label.shape)
    out = torch.where(removed, torch.tensor(float(level), dtype=torch.float32, device=vol.device), vol)
    return (out if volume.dim() == 4 else out[0]), kept_nodes


def filter_components(volume: torch.Tensor, level: float, largest: Optional[int] = None, min_nodes: Optional[int] = None) -> torch.Tensor:
    """volume [B, Gz, Gy, Gx] or [Gz, Gy, Gx] fp32 on the GPU -> the volume with every inside node of a component that is not kept
    set to float32(level), everything else bit for bit (filter_components_reference).

    largest=k keeps the k components with the most nodes of every volume, ties to the smaller root; min_nodes=m those with at least
    m nodes; both the intersection, neither all.  The isosurface of the result is the isosurface of the volume without the removed
    components' vertices and faces."""
    return filter_components_counted(volume, level, largest, min_nodes)[0]
