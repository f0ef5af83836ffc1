"""The edges of a triangle mesh and Taubin smoothing on their own kernels (csrc/smooth.hip).  `mesh_edges` builds what
says what a mesh's connectivity is: its unique edges with the number of faces on each, the vertex adjacency in CSR form and the
topology counts.  `smooth_mesh` runs Taubin's lambda | mu smoothing over that adjacency: an umbrella Laplacian step with lam > 0, then
one with mu < 0, so that the shape does not shrink.  `mesh_edges_reference` and `smooth_reference` of npcd/eval/mesh.py restate both
specifications on the CPU.

The smoothing's state is an integer lattice, 2^30 steps to the largest coordinate, so a vertex's neighbour sum -- and with it every
output -- is the same in any order: the same mesh gives the same bits on every run.  Ordering the 6F edge keys is one torch.sort; the
sizes of the edge arrays depend on the data: one host read, of the counts.  smooth_mesh on a dict of mesh_edges makes none.  There is
no CPU fallback: a non-GPU tensor or a wrong dtype raises RuntimeError.
"""
from typing import Dict, Optional

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

# key positions per strip of the two-level prefix sums (kSmStrip of csrc/smooth.h): a mesh of more than STRIP_KEYS / 6 faces has more
# than one strip
STRIP_KEYS = 256
MAX_VERTICES, MAX_FACES, MAX_ITERATIONS = 2 ** 31, 2 ** 28, 1000
EDGE_KEYS = ("row_start", "neighbours", "edges", "edge_faces", "edge_forward", "boundary_vertex", "counts")


def _faces(who: str, num_vertices, faces) -> int:
    if not isinstance(faces, torch.Tensor):
        raise ValueError(f"{who}: faces must be a tensor")
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: faces must be [F, 3]; got {tuple(faces.shape)}")
    V, F = int(num_vertices), int(faces.shape[0])
    if V < 0:
        raise ValueError(f"{who}: {V} vertices")
    if V >= MAX_VERTICES or F >= MAX_FACES:
        raise ValueError(f"{who}: {V} vertices and {F} faces; vertices must stay below 2^31 = {MAX_VERTICES} and faces below 2^28 = {MAX_FACES}")
    require_gpu(faces)
    if faces.dtype != torch.int32:
        raise RuntimeError(f"{who}: faces must be int32; got {faces.dtype}")
    return V


def mesh_edges(num_vertices: int, faces: torch.Tensor) -> Dict[str, torch.Tensor]:
    """faces [F, 3] int32 on the GPU over vertices 0 .. num_vertices - 1 -> {"row_start" [V + 1], "neighbours" [D], "edges" [E, 2],
    "edge_faces" [E], "edge_forward" [E] int32, "boundary_vertex" [V] uint8, "counts" [6] int64}, all on the GPU: the arrays of
    npcd.eval.mesh.mesh_edges_reference.

    A face with an index outside [0, V) or with two equal indices contributes nothing.  row_start and neighbours are the vertex
    adjacency in CSR form, a vertex's neighbours ascending; edges holds every edge once as (a, b) with a < b, edge_faces the faces on
    it and edge_forward those that traverse it as a -> b.  counts = (D, valid faces, used vertices, boundary edges, non-manifold
    edges, misoriented edges); npcd.eval.mesh.mesh_topology turns them into Python numbers.  One host read, of the counts."""
    who = "mesh_edges"
    V = _faces(who, num_vertices, faces)
    F, dev = int(faces.shape[0]), faces.device
    faces = faces.contiguous()
    L = lib()
    with torch.cuda.device(dev):
        counts = torch.zeros(6, dtype=torch.int64, device=dev)
        distinct = 0
        if F and V:
            keys = torch.empty(6 * F, dtype=torch.int64, device=dev)
            check(L.npcd_mesh_edges_keys(ptr(faces), V, F, ptr(keys), stream_ptr()), "npcd_mesh_edges_keys")
            keys = torch.sort(keys)[0]
            ws = torch.empty(workspace_bytes(V, F) // 8 + 1, dtype=torch.int64, device=dev)
            check(L.npcd_mesh_edges_unique(ptr(keys), V, F, ptr(ws), ptr(counts), stream_ptr()), "npcd_mesh_edges_unique")
            distinct = int(counts[0].item())          # the one host read
        out = {"row_start": torch.empty(V + 1, dtype=torch.int32, device=dev) if distinct else torch.zeros(V + 1, dtype=torch.int32, device=dev),
               "neighbours": torch.empty(distinct, dtype=torch.int32, device=dev),
               "edges": torch.empty((distinct // 2, 2), dtype=torch.int32, device=dev),
               "edge_faces": torch.empty(distinct // 2, dtype=torch.int32, device=dev),
               "edge_forward": torch.empty(distinct // 2, dtype=torch.int32, device=dev),
               "boundary_vertex": torch.empty(V, dtype=torch.uint8, device=dev) if distinct else torch.zeros(V, dtype=torch.uint8, device=dev),
               "counts": counts}
        if distinct:
            check(L.npcd_mesh_edges_emit(ptr(keys), V, F, ptr(ws), distinct, ptr(out["row_start"]), ptr(out["neighbours"]), ptr(out["edges"]),
                                         ptr(out["edge_faces"]), ptr(out["edge_forward"]), ptr(out["boundary_vertex"]), ptr(counts),
                                         stream_ptr()), "npcd_mesh_edges_emit")
    return out


def workspace_bytes(V: int, F: int) -> int:
    """Bytes of device workspace for the edges of a mesh of V vertices and F faces."""
    got = lib().npcd_mesh_edges_ws_bytes(V, F)
    check(min(got, 0), "npcd_mesh_edges_ws_bytes")
    return got


def smooth_mesh(vertices: torch.Tensor, faces: Optional[torch.Tensor], iterations: int = 10, lam: float = 0.5, mu: float = -0.53,
                fixed: Optional[torch.Tensor] = None, fix_boundary: bool = True, edges: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
    """vertices [V, 3] fp32, faces [F, 3] int32 on the GPU -> the smoothed vertices [V, 3] fp32, the bits of
    npcd.eval.mesh.smooth_reference.

    `iterations` (0 .. 1000) times a step with factor lam in (0, 1], then one with mu in [-1, 0]: Taubin's lambda | mu smoothing with
    uniform (umbrella) weights; mu = 0 is the plain Laplacian, which shrinks.  A step moves a vertex by the factor toward the mean of
    its neighbours, all vertices reading the old positions.  fixed [V] bool pins vertices; fix_boundary pins the vertices on an edge
    of one face.  A vertex with a coordinate that is not finite never moves and is no one's neighbour.  A vertex that does not move
    comes back with its input bits; one that moves lies on a lattice of 2^29 to 2^30 steps to the largest |coordinate| of the call.
    edges: the dict of mesh_edges(V, faces) to use again (faces may then be None); with it the call makes no host read."""
    who = "smooth_mesh"
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be a tensor [V, 3]; got {tuple(vertices.shape) if isinstance(vertices, torch.Tensor) else type(vertices)}")
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= MAX_ITERATIONS:
        raise ValueError(f"{who}: iterations must be an integer in [0, {MAX_ITERATIONS}]; got {iterations!r}")
    lam, mu = float(lam), float(mu)
    if not (0.0 < lam <= 1.0 and -1.0 <= mu <= 0.0):
        raise ValueError(f"{who}: lam must lie in (0, 1] and mu in [-1, 0]; got {lam} and {mu}")
    V, dev = int(vertices.shape[0]), vertices.device
    if fixed is not None and (not isinstance(fixed, torch.Tensor) or fixed.shape != (V,)):
        raise ValueError(f"{who}: fixed must be a tensor [{V}]; got {tuple(fixed.shape) if isinstance(fixed, torch.Tensor) else type(fixed)}")
    if edges is None:
        _faces(who, V, faces)
    else:
        if not isinstance(edges, dict) or any(k not in edges for k in EDGE_KEYS):
            raise ValueError(f"{who}: edges must be the dict of mesh_edges with {EDGE_KEYS}")
        if edges["row_start"].shape != (V + 1,) or edges["boundary_vertex"].shape != (V,):
            raise ValueError(f"{who}: edges are those of a mesh of {edges['row_start'].shape[0] - 1} vertices, not of {V}")
    require_gpu(vertices, fixed)
    if vertices.dtype != torch.float32:
        raise RuntimeError(f"{who}: vertices must be fp32; got {vertices.dtype}")
    if fixed is not None and (fixed.dtype != torch.bool or fixed.device != dev):
        raise RuntimeError(f"{who}: fixed must be bool on the mesh's device; got {fixed.dtype} on {fixed.device}")
    if edges is None:
        if faces.device != dev:
            raise RuntimeError(f"{who}: vertices on {dev}, faces on {faces.device}")
        edges = mesh_edges(V, faces)
    row_start, neighbours, boundary = edges["row_start"], edges["neighbours"], edges["boundary_vertex"]
    require_gpu(row_start, neighbours, boundary)
    if row_start.dtype != torch.int32 or neighbours.dtype != torch.int32 or boundary.dtype != torch.uint8 or row_start.device != dev:
        raise RuntimeError(f"{who}: edges must be the arrays of mesh_edges on the mesh's device")
    vertices = vertices.detach().contiguous()
    out = torch.empty_like(vertices)
    if V == 0:
        return out
    pinned = None if fixed is None else fixed.contiguous().view(torch.uint8)
    L = lib()
    with torch.cuda.device(dev):
        got = L.npcd_smooth_ws_bytes(V)
        check(min(got, 0), "npcd_smooth_ws_bytes")
        ws = torch.empty(got // 8 + 2, dtype=torch.int64, device=dev)          # a fresh allocation: aligned well beyond the 16 bytes asked for
        check(L.npcd_smooth_mesh(ptr(vertices), V, ptr(row_start.contiguous()), ptr(neighbours.contiguous()), int(neighbours.shape[0]),
                                 ptr(boundary.contiguous()) if fix_boundary else None, ptr(pinned), iterations, lam, mu, ptr(ws), ptr(out),
                                 stream_ptr()), "npcd_smooth_mesh")
    return out
