"""The first intersection of every ray with a triangle mesh on its own kernel (csrc/raycast.hip): the ray parameter,
the face, the barycentric weights and the facing.  What render_mesh and mesh_render_agreement of npcd/eval/mesh.py look at a mesh
with, and the basis of anything that needs visibility.  `ray_mesh_reference` of npcd/eval/mesh.py restates the specification on the
CPU.

Every pair is the watertight ray / triangle test of Woop, Benthin and Wald with fp32 sheared corners and float64 edge functions as
written, and the winner is the lexicographic minimum of (t, face): the outputs are the same bits whether tiles of faces are culled or
not.  The call makes no host read: every size is known from the shapes.  There is no CPU fallback: a non-GPU tensor or a wrong dtype
raises RuntimeError.
"""
from typing import Dict, Optional

import torch

from . import check, lib, ptr, stream_ptr
from .mesh_distance import MAX_FACES, MAX_VERTICES, TILE_FACES, _checked, mesh_boxes

# rays per wave (kRcThreads of csrc/raycast.h); the tiles are those of mesh_distance (kMdTile): culling decides per (wave, tile)
WAVE_RAYS = 64
MAX_RAYS = 2 ** 31


def checked_rays(who: str, origins, directions, vertices, faces, boxes):
    """The argument checks of cast_rays, which npcd.hip.crossings.count_crossings shares -> the four tensors, detached and contiguous."""
    def sizes():
        R, V, F = int(origins.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
        if directions.shape[0] != R:
            raise ValueError(f"{who}: {R} origins and {int(directions.shape[0])} directions")
        if V >= MAX_VERTICES or F >= MAX_FACES or R >= MAX_RAYS:
            raise ValueError(f"{who}: {R} rays, {V} vertices and {F} faces; rays and vertices must stay below 2^31 and faces below 2^28 = {MAX_FACES}")
    return _checked(who, {"origins": origins, "directions": directions, "vertices": vertices, "faces": faces}, sizes, boxes)


def ray_workspace(who: str, vertices: torch.Tensor, faces: torch.Tensor, boxes: Optional[torch.Tensor]) -> torch.Tensor:
    """boxes= of cast_rays and count_crossings: mesh_boxes(vertices, faces) where none is given, else the given one if it can be
    that of this mesh (ValueError otherwise).  Inside torch.cuda.device of the mesh."""
    if boxes is None:
        return mesh_boxes(vertices, faces)
    need = lib().npcd_mesh_distance_ws_bytes(int(vertices.shape[0]), int(faces.shape[0]))
    check(min(need, 0), "npcd_mesh_distance_ws_bytes")
    if boxes.dtype != torch.int64 or boxes.dim() != 1 or not boxes.is_contiguous() or boxes.numel() * 8 < need:
        raise ValueError(f"{who}: boxes must be what mesh_boxes returned for these vertices and faces ({need} bytes as int64)")
    return boxes


def cast_rays(origins: torch.Tensor, directions: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, t_min: float = 0.0,
              t_max: float = float("inf"), cull: bool = True, stats: bool = False, boxes: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """origins, directions [R, 3], vertices [V, 3] fp32 and faces [F, 3] int32 on the GPU -> {"t" [R] fp32, "face" [R] int32, "bary"
    [R, 3] fp32, "front" [R] int8}, the bits of npcd.eval.mesh.ray_mesh_reference.

    A face takes part if its indices lie in [0, V).  Per ray the hit with the smallest t in [t_min, t_max] wins, the lowest face
    index among equal ones (t as a signed float, t_min may be negative); the point is origin + t direction, directions need not be
    unit; bary weighs the face's three corners and front is 1 where the face's normal (B - A) x (C - A) points against the ray.  A
    ray with a component that is not finite or a zero direction, and a ray that hits nothing, gets (+inf, -1, zeros, 0).  cull=True
    skips tiles of TILE_FACES consecutive faces whose box no ray of a wave reaches before what the wave has found: rays that are
    neighbours in the array should be neighbours in space (the call does not reorder them).  It changes no bit of the outputs.
    stats=True adds "evaluated", an int64 word on the GPU: the (wave, tile) pairs that were evaluated, of ceil(R / WAVE_RAYS)
    ceil(F / TILE_FACES).  boxes= takes mesh_boxes(vertices, faces) from an earlier call.  No host read."""
    who = "cast_rays"
    origins, directions, vertices, faces = checked_rays(who, origins, directions, vertices, faces, boxes)
    R, V, F = int(origins.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    dev = origins.device
    L = lib()
    with torch.cuda.device(dev):
        out = {"t": torch.full((R,), float("inf"), dtype=torch.float32, device=dev),
               "face": torch.full((R,), -1, dtype=torch.int32, device=dev),
               "bary": torch.zeros((R, 3), dtype=torch.float32, device=dev),
               "front": torch.zeros((R,), dtype=torch.int8, device=dev)}
        evaluated = torch.zeros(1, dtype=torch.int64, device=dev) if stats else None
        if stats:
            out["evaluated"] = evaluated
        if R == 0 or F == 0:
            return out
        boxes = ray_workspace(who, vertices, faces, boxes)
        check(L.npcd_raycast_query(ptr(origins), ptr(directions), R, ptr(vertices), V, ptr(faces), F, ptr(boxes), float(t_min), float(t_max),
                                   1 if cull else 0, ptr(out["t"]), ptr(out["face"]), ptr(out["bary"]), ptr(out["front"]), ptr(evaluated),
                                   stream_ptr()), "npcd_raycast_query")
    return out
