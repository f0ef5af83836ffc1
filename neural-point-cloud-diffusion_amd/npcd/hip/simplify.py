"""Simplification of a triangle mesh by vertex clustering on its own kernels (csrc/simplify.hip): every vertex falls
into a cell of a regular grid, the vertices of a cell become one vertex at their mean, the faces are rewritten onto the new vertices,
and faces that collapse or repeat go.  What brings the meshes of npcd.hip.isosurface / npcd.eval.mesh.extract_mesh down to a
triangle count that can be used.  `simplify_reference` of npcd/eval/mesh.py restates the specification on the CPU.

The places of the vertices inside their cells and the attributes are made integers before they are summed, so a cluster's sums -- and
with them every output -- do not depend on the order of an atomic or a scan: the same mesh gives the same bits on every run.  The sizes
of the result depend on the data: one host read, of (V', F').  A grid that is not given is taken from the bounds of the finite
vertices, which is a second read.  There is no CPU fallback: a non-GPU tensor or a wrong dtype raises RuntimeError.
"""
import ctypes
from typing import Dict, Optional

import torch

from . import check, lib, ptr, require_gpu, stream_ptr
from .surface import MAX_CHANNELS

# bitmap words and face marks per strip of the two-level prefix sums (kSimpStrip of csrc/simplify.h): a grid of more than
# 32 * STRIP_WORDS cells has more than one strip
STRIP_WORDS = 256
# one packed int64 key holds the sorted triple of a face while the cluster ids stay below 2^21 (kSimpPackedIds)
PACKED_IDS = 2 ** 21


def workspace_bytes(V: int, F: int, C: int, dims) -> int:
    """Bytes of device workspace for a mesh of V vertices with C attribute channels and F faces on a grid of dims cells."""
    got = lib().npcd_simplify_ws_bytes(V, F, C, (ctypes.c_int * 3)(*[int(d) for d in dims]))
    check(min(got, 0), "npcd_simplify_ws_bytes")
    return got


def _empty(dev, V: int, C: Optional[int]) -> Dict[str, torch.Tensor]:
    out = {"vertices": torch.zeros((0, 3), dtype=torch.float32, device=dev), "faces": torch.zeros((0, 3), dtype=torch.int32, device=dev),
           "vertex_cluster": torch.full((V,), -1, dtype=torch.int32, device=dev), "face_source": torch.zeros((0,), dtype=torch.int32, device=dev)}
    if C is not None:
        out["attributes"] = torch.zeros((0, C), dtype=torch.float32, device=dev)
    return out


def simplify_mesh(vertices: torch.Tensor, faces: torch.Tensor, cell, origin=None, dims=None, attributes: Optional[torch.Tensor] = None,
                  two_pass_sort: Optional[bool] = None) -> Dict[str, torch.Tensor]:
    """vertices [V, 3] fp32, faces [F, 3] int32 on the GPU -> {"vertices" [V', 3] fp32, "faces" [F', 3] int32, "vertex_cluster" [V]
    int32 (-1: a lost vertex), "face_source" [F'] int32, and "attributes" [V', C] fp32 where given}, the bits of
    npcd.eval.mesh.simplify_reference.

    cell: the size of a grid cell, a float or three (x, y, z).  origin (three floats) and dims (three ints, at most 2^30 cells
    together) place the grid; vertices outside it fall into its border cells.  origin=None takes the smallest coordinates of the finite
    vertices, dims=None the cells that reach their largest (npcd.eval.mesh.clustering_grid).  attributes [V, C] fp32, 1 <= C <= 16
    (colours, normals): averaged per cluster, a value that is not finite counting as 0.  A vertex with a coordinate that is not finite
    is lost, and its faces go.  The kept faces keep their corner order and the input order.  The result may be non-manifold.
    two_pass_sort forces (True) or forbids (False) the two stable sorting passes that more than 2^21 clusters need."""
    who = "simplify_mesh"
    if not isinstance(vertices, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise ValueError(f"{who}: vertices and faces must be tensors")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V, 3] and faces [F, 3]; got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    require_gpu(vertices, faces)
    if vertices.dtype != torch.float32 or faces.dtype != torch.int32:
        raise RuntimeError(f"{who}: vertices must be fp32 and faces int32; got {vertices.dtype} and {faces.dtype}")
    if faces.device != vertices.device:
        raise RuntimeError(f"{who}: vertices on {vertices.device}, faces on {faces.device}")
    V, F, dev = int(vertices.shape[0]), int(faces.shape[0]), vertices.device
    if V >= 2 ** 31 or F >= 2 ** 31:
        raise ValueError(f"{who}: {V} vertices and {F} faces; each must stay below 2^31")
    C = None
    if attributes is not None:
        if not isinstance(attributes, torch.Tensor) or attributes.dim() != 2 or attributes.shape[0] != V:
            raise ValueError(f"{who}: attributes must be [{V}, C]; got {tuple(attributes.shape) if isinstance(attributes, torch.Tensor) else type(attributes)}")
        C = int(attributes.shape[1])
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"{who}: attributes must have 1 to {MAX_CHANNELS} channels; got {C}")
        require_gpu(attributes)
        if attributes.dtype != torch.float32 or attributes.device != dev:
            raise RuntimeError(f"{who}: attributes must be fp32 on the mesh's device; got {attributes.dtype} on {attributes.device}")
        attributes = attributes.detach().contiguous()
    vertices, faces = vertices.detach().contiguous(), faces.contiguous()
    from ..eval.mesh import clustering_grid
    lower = upper = None
    if V and (origin is None or dims is None):          # the bounds of the finite vertices: one read of six numbers
        whole = torch.isfinite(vertices).all(dim=1, keepdim=True)
        bounds = torch.stack((torch.where(whole, vertices, float("inf")).amin(dim=0), torch.where(whole, vertices, float("-inf")).amax(dim=0))).cpu()
        if bool(torch.isfinite(bounds).all()):
            lower, upper = bounds[0].double().numpy(), bounds[1].double().numpy()
    origin, cell, dims = clustering_grid(cell, origin, dims, lower, upper)
    if V == 0:
        return _empty(dev, 0, C)
    channels = C or 0
    rows = min(V, dims[0] * dims[1] * dims[2])
    two_keys = rows > PACKED_IDS if two_pass_sort is None else bool(two_pass_sort)
    if not two_keys and rows > PACKED_IDS:
        raise ValueError(f"{who}: up to {rows} clusters do not fit one packed key (at most 2^21 = {PACKED_IDS}); two_pass_sort=False cannot hold")
    org, step, size = (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*cell), (ctypes.c_int * 3)(*dims)
    L = lib()
    with torch.cuda.device(dev):
        ws = torch.empty(workspace_bytes(V, F, channels, dims) // 8 + 1, dtype=torch.int64, device=dev)
        cluster = torch.empty(V, dtype=torch.int32, device=dev)
        counts = torch.zeros(2, dtype=torch.int64, device=dev)
        check(L.npcd_simplify_cluster(ptr(vertices), V, F, ptr(attributes), channels, org, step, size, ptr(ws), ptr(cluster), ptr(counts),
                                      stream_ptr()), "npcd_simplify_cluster")
        if F:
            key_lo = torch.empty(F, dtype=torch.int64, device=dev)
            key_hi = torch.empty(F, dtype=torch.int64, device=dev) if two_keys else None
            check(L.npcd_simplify_faces(ptr(faces), V, F, channels, size, ptr(cluster), ptr(ws), ptr(key_hi), ptr(key_lo), stream_ptr()),
                  "npcd_simplify_faces")
            order = torch.sort(key_lo, stable=True)[1]
            if two_keys:
                order = order[torch.sort(key_hi[order], stable=True)[1]]
            check(L.npcd_simplify_unique(ptr(order), V, F, channels, size, ptr(ws), ptr(counts), stream_ptr()), "npcd_simplify_unique")
        n_vert, n_face = (int(c) for c in counts.cpu())          # the one host read
        if n_vert == 0:          # every vertex is lost
            return _empty(dev, V, C)
        out = {"vertices": torch.empty((n_vert, 3), dtype=torch.float32, device=dev),
               "faces": torch.empty((n_face, 3), dtype=torch.int32, device=dev), "vertex_cluster": cluster,
               "face_source": torch.empty((n_face,), dtype=torch.int32, device=dev)}
        if C is not None:
            out["attributes"] = torch.empty((n_vert, C), dtype=torch.float32, device=dev)
        check(L.npcd_simplify_emit(V, F, channels, org, step, size, ptr(ws), n_vert, n_face, ptr(out["vertices"]), ptr(out.get("attributes")),
                                   ptr(out["faces"]) if n_face else None, ptr(out["face_source"]) if n_face else None, stream_ptr()),
              "npcd_simplify_emit")
    return out
