"""How often every ray crosses a triangle mesh, per facing, on its own kernel (csrc/crossings.hip), and from it
which side of a closed surface a point lies on.  What voxelize_mesh, mesh_volume_iou, mesh_signed_distance and
extract_mesh(enclosure=True) of npcd/eval/mesh.py rest on.  `crossings_reference` of npcd/eval/mesh.py restates the specification on
the CPU.

The corners, edge functions and t of a pair are those of npcd.hip.raycast.cast_rays; where that rule is inclusive (a ray through a
shared edge hits every face around it, so that none slips through), this one is half open: each edge belongs to one of its faces, by
the rasteriser's top-left rule, so every crossing of a closed surface counts once.  The outputs are integer counts: the same with and
without culling.  No host read.  There is no CPU fallback: a non-GPU tensor or a wrong dtype raises RuntimeError.
"""
from typing import Dict, Optional, Sequence

import torch

from . import check, lib, ptr, stream_ptr
from .raycast import checked_rays, ray_workspace

RULES = ("parity", "winding")


def count_crossings(origins: torch.Tensor, directions: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, t_min: float = 0.0,
                    t_max: float = float("inf"), cull: bool = True, stats: bool = False, boxes: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """origins, directions [R, 3], vertices [V, 3] fp32 and faces [F, 3] int32 on the GPU -> {"front" [R], "back" [R] int32}, the
    counts of npcd.eval.mesh.crossings_reference: the faces that the ray crosses with t in [t_min, t_max], those whose normal
    (B - A) x (C - A) points against the ray and those whose normal points along it.

    A face takes part if its indices lie in [0, V).  A ray with a component that is not finite or a zero direction gets (0, 0).
    cull=True skips tiles of TILE_FACES consecutive faces whose box no ray segment [t_min, t_max] of a wave reaches: rays that are
    neighbours in the array should be neighbours in space (the call does not reorder them).  It changes no count.  stats=True adds
    "evaluated", an int64 word on the GPU: the (wave, tile) pairs that were evaluated.  boxes= takes mesh_boxes(vertices, faces) from
    an earlier call.  No host read.

    Unspecified: on which side of a face a ray falls that passes it within rounding (the fp32 shear moves a corner by a few ulp), so
    also the count of a ray whose origin lies within rounding of the surface."""
    who = "count_crossings"
    origins, directions, vertices, faces = checked_rays(who, origins, directions, vertices, faces, boxes)
    R, V, F = int(origins.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    dev = origins.device
    with torch.cuda.device(dev):
        out = {"front": torch.zeros((R,), dtype=torch.int32, device=dev), "back": torch.zeros((R,), dtype=torch.int32, device=dev)}
        evaluated = torch.zeros(1, dtype=torch.int64, device=dev) if stats else None
        if stats:
            out["evaluated"] = evaluated
        if R == 0 or F == 0:
            return out
        boxes = ray_workspace(who, vertices, faces, boxes)
        check(lib().npcd_crossings_query(ptr(origins), ptr(directions), R, ptr(vertices), V, ptr(faces), F, ptr(boxes), float(t_min),
                                         float(t_max), 1 if cull else 0, ptr(out["front"]), ptr(out["back"]), ptr(evaluated), stream_ptr()),
              "npcd_crossings_query")
    return out


def mesh_contains(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, direction: Sequence[float] = (1.0, 0.0, 0.0),
                  rule: str = "parity", boxes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """points [N, 3], vertices [V, 3] fp32 and faces [F, 3] int32 on the GPU -> bool [N]: whether the point lies inside the closed
    surface, from the crossings of the ray from the point along `direction` (count_crossings with t in [0, +inf)).

    rule="parity": front + back is odd; it does not depend on how the faces are wound.  rule="winding": back - front != 0, for
    consistently wound surfaces, where a region that two shells cover is inside.  Any direction gives the same answer for a closed
    surface and a point off it; points that are neighbours in the array should be neighbours in space.  No host read.

    Unspecified: a point within rounding of the surface, and a mesh that is not closed -- parity then means nothing."""
    if rule not in RULES:
        raise ValueError(f"mesh_contains: rule must be one of {RULES}; got {rule!r}")
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"mesh_contains: points must be a [N, 3] tensor; got {tuple(points.shape) if isinstance(points, torch.Tensor) else type(points)}")
    if len(direction) != 3:
        raise ValueError(f"mesh_contains: direction must hold three numbers; got {direction!r}")
    # filled on the device: a copy of host numbers to the GPU would wait for the stream
    d = torch.stack([torch.full((), float(x), dtype=torch.float32, device=points.device) for x in direction])
    got = count_crossings(points, d.expand(points.shape[0], 3), vertices, faces, boxes=boxes)
    return ((got["front"] + got["back"]) & 1).bool() if rule == "parity" else got["back"] != got["front"]
