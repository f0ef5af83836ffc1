"""The closest point of a triangle mesh to every query point on its own kernels (csrc/mesh_distance.hip): the
squared distance, the face and the point on it.  What mesh_deviation and cloud_mesh_distance of npcd/eval/mesh.py measure with, and
the first step of carrying attributes from one mesh to another.  `point_mesh_distance_reference` of npcd/eval/mesh.py restates the
specification on the CPU.

Every pair is the region form of Ericson's closest point on a triangle in fp32 as written, and the winner is the lexicographic minimum
of (dist2, face): the outputs are the same bits whether tiles of faces are culled or not and whether the queries are sorted or not.
The call makes no host read: every size is known from the shapes.  There is no CPU fallback: a non-GPU tensor or a wrong dtype raises
RuntimeError.
"""
from typing import Callable, Dict, List, Optional

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

# faces per tile and query points per wave (kMdTile and kMdThreads of csrc/mesh_distance.h): culling decides per (wave, tile)
TILE_FACES = 256
WAVE_POINTS = 64
MAX_VERTICES, MAX_FACES, MAX_POINTS = 2 ** 31, 2 ** 28, 2 ** 31
SORT_GRID = 1024          # cells per axis of the grid whose Morton key orders the queries


def _spread(c: torch.Tensor) -> torch.Tensor:
    """10-bit integers (int64) -> their bits two apart."""
    c = (c | (c << 16)) & 0x030000FF
    c = (c | (c << 8)) & 0x0300F00F
    c = (c | (c << 4)) & 0x030C30C3
    return (c | (c << 2)) & 0x09249249


def sort_order(points: torch.Tensor, vertices: torch.Tensor) -> torch.Tensor:
    """The order of the queries by the Morton key of their cell on a SORT_GRID^3 grid over the bounds of the finite vertices: the 64
    points of a wave are then neighbours.  Torch operators on the device, no host read; any order gives the same outputs."""
    inf = torch.full((), float("inf"), dtype=torch.float32, device=vertices.device)
    finite = torch.isfinite(vertices)
    lo = torch.where(finite, vertices, inf).amin(dim=0)
    hi = torch.where(finite, vertices, -inf).amax(dim=0)
    u = (points - lo) / (hi - lo) * SORT_GRID
    cell = torch.nan_to_num(u, nan=0.0, posinf=SORT_GRID - 1.0, neginf=0.0).clamp(0, SORT_GRID - 1).to(torch.int64)
    key = _spread(cell[:, 0]) | (_spread(cell[:, 1]) << 1) | (_spread(cell[:, 2]) << 2)
    return torch.sort(key)[1]


def _checked(who: str, tensors: Dict[str, torch.Tensor], sizes: Callable[[], None], boxes: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """The checks that mesh_boxes, closest_on_mesh and npcd.hip.raycast.cast_rays share, in their order.  tensors: name -> argument,
    int32 for "faces" and fp32 for every other.  Each must be a [N, 3] tensor (ValueError); sizes() then raises ValueError for row
    counts that the caller cannot take; then they must lie on the GPU, have these dtypes and share one device, with boxes where
    given (RuntimeError).  -> the tensors, detached and contiguous."""
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a tensor")
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{who}: {name} must be [N, 3]; got {tuple(t.shape)}")
    sizes()
    require_gpu(*tensors.values(), boxes)
    if any(t.dtype != (torch.int32 if name == "faces" else torch.float32) for name, t in tensors.items()):
        raise RuntimeError(f"{who}: faces must be int32 and the others fp32; got " + ", ".join(f"{name} {t.dtype}" for name, t in tensors.items()))
    if len({t.device for t in (*tensors.values(), boxes) if t is not None}) != 1:
        raise RuntimeError(f"{who}: " + ", ".join(f"{name} on {t.device}" for name, t in tensors.items()))
    return [t.detach().contiguous() for t in tensors.values()]


def mesh_boxes(vertices: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """vertices [V, 3] fp32 and faces [F, 3] int32 on the GPU, F >= 1 -> the workspace that npcd_mesh_distance_boxes leaves (the
    corners of every face and the box of every tile of TILE_FACES faces) as an int64 tensor: what npcd.hip.raycast.cast_rays takes as
    boxes=, so that many calls on one mesh build it once.  It belongs to these vertices and faces.  One launch, no host read."""
    who = "mesh_boxes"

    def sizes():
        V, F = int(vertices.shape[0]), int(faces.shape[0])
        if V >= MAX_VERTICES or not 1 <= F < MAX_FACES:
            raise ValueError(f"{who}: {V} vertices and {F} faces; vertices must stay below 2^31 and faces in [1, 2^28 = {MAX_FACES})")
    vertices, faces = _checked(who, {"vertices": vertices, "faces": faces}, sizes)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    L = lib()
    with torch.cuda.device(vertices.device):
        got = L.npcd_mesh_distance_ws_bytes(V, F)
        check(min(got, 0), "npcd_mesh_distance_ws_bytes")
        ws = torch.empty(got // 8 + 2, dtype=torch.int64, device=vertices.device)          # a fresh allocation: aligned well beyond 16 bytes
        check(L.npcd_mesh_distance_boxes(ptr(vertices), V, ptr(faces), F, ptr(ws), stream_ptr()), "npcd_mesh_distance_boxes")
    return ws


def closest_on_mesh(points: torch.Tensor, vertices: torch.Tensor, faces: torch.Tensor, cull: bool = True, sort_points: bool = True,
                    stats: bool = False) -> Dict[str, torch.Tensor]:
    """points [S, 3], vertices [V, 3] fp32 and faces [F, 3] int32 on the GPU -> {"sqdist" [S] fp32, "face" [S] int32, "closest"
    [S, 3] fp32}, the bits of npcd.eval.mesh.point_mesh_distance_reference.

    A face takes part if its indices lie in [0, V).  Per point the face with the smallest squared distance wins, the lowest index
    among equal ones; a NaN distance (a vertex that is not finite, a zero-area face seen from beside) never wins, and a point that no
    face wins gets (+inf, -1, zeros).  cull=True skips tiles of TILE_FACES consecutive faces whose box is farther from every point of
    a wave than what the wave has found; sort_points=True orders the queries so that a wave's points are neighbours, which is what
    makes culling pay, and scatters the results back.  Neither changes a bit of the outputs.  stats=True adds "evaluated", an int64
    word on the GPU: the (wave, tile) pairs that were evaluated, of ceil(S / WAVE_POINTS) ceil(F / TILE_FACES).  No host read."""
    who = "closest_on_mesh"

    def sizes():
        S, V, F = int(points.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
        if V >= MAX_VERTICES or F >= MAX_FACES or S >= MAX_POINTS:
            raise ValueError(f"{who}: {S} points, {V} vertices and {F} faces; points and vertices must stay below 2^31 and faces below 2^28 = {MAX_FACES}")
    points, vertices, faces = _checked(who, {"points": points, "vertices": vertices, "faces": faces}, sizes)
    S, V, F = int(points.shape[0]), int(vertices.shape[0]), int(faces.shape[0])
    dev = points.device
    L = lib()
    with torch.cuda.device(dev):
        out = {"sqdist": torch.full((S,), float("inf"), dtype=torch.float32, device=dev),
               "face": torch.full((S,), -1, dtype=torch.int32, device=dev),
               "closest": torch.zeros((S, 3), dtype=torch.float32, device=dev)}
        evaluated = torch.zeros(1, dtype=torch.int64, device=dev) if stats else None
        if stats:
            out["evaluated"] = evaluated
        if S == 0 or F == 0:
            return out
        ws = mesh_boxes(vertices, faces)
        order = sort_order(points, vertices) if sort_points and V > 0 and S > 1 else None
        queries = points if order is None else points[order].contiguous()
        res = out if order is None else {k: torch.empty_like(out[k]) for k in ("sqdist", "face", "closest")}
        check(L.npcd_mesh_distance_query(ptr(queries), S, ptr(vertices), V, ptr(faces), F, ptr(ws), 1 if cull else 0, ptr(res["sqdist"]),
                                         ptr(res["face"]), ptr(res["closest"]), ptr(evaluated), stream_ptr()), "npcd_mesh_distance_query")
        if order is not None:
            for k in ("sqdist", "face", "closest"):
                out[k][order] = res[k]
    return out
