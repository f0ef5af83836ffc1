"""Isosurface of a density volume as an indexed triangle mesh on its own kernels (csrc/isosurface.hip): marching
tetrahedra on the Kuhn triangulation of the lattice.  The operator under npcd/eval/mesh.py, whose `marching_tetrahedra_reference`
restates the specification on the CPU.

Two passes with one host read between them -- the number of vertices and triangles depends on the data -- and no atomics: the same
volume gives the same bits on every run.  There is no CPU fallback: a non-GPU tensor or a dtype other than fp32 raises RuntimeError.

With normals=True a third launch (csrc/isosurface_normals.hip) writes a unit normal beside every vertex: minus the
gradient of the volume -- or of another field of its shape -- interpolated along the vertex's edge, the bits of
npcd.eval.mesh.vertex_normals_reference.
"""
import ctypes
from typing import List, Optional, Sequence, Tuple

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

# nodes per workgroup (kIsoThreads of csrc/isosurface.hip): a workgroup owns that many consecutive node indices, x fastest
STRIP_NODES = 1024


def _triple(v, name: str) -> Tuple[float, float, float]:
    v = [float(c) for c in (v.tolist() if isinstance(v, torch.Tensor) else v)]
    if len(v) != 3:
        raise ValueError(f"isosurface: {name} must hold three values (x, y, z); got {len(v)}")
    return v[0], v[1], v[2]


def workspace_bytes(B: int, gz: int, gy: int, gx: int) -> int:
    """Bytes of device workspace for B volumes of gz x gy x gx nodes."""
    got = lib().npcd_isosurface_ws_bytes(B, gz, gy, gx)
    check(min(got, 0), "npcd_isosurface_ws_bytes")
    return got


def isosurface(volume: torch.Tensor, level: float, origin: Sequence[float] = (0.0, 0.0, 0.0), spacing: Sequence[float] = (1.0, 1.0, 1.0),
               normals: bool = False, gradient_of: Optional[torch.Tensor] = None) -> List[Tuple[torch.Tensor, ...]]:
    """volume [B, Gz, Gy, Gx] or [Gz, Gy, Gx] fp32 on the GPU, x fastest -> per volume (vertices [V, 3] fp32, faces [F, 3] int32) on
    the GPU; with normals=True (vertices, faces, normals [V, 3] fp32).

    A node is inside where volume > level; node (x, y, z) lies at origin + spacing * (x, y, z), `origin` and `spacing` given as
    (x, y, z) host values.  Vertices are in ascending (node, edge type) order, triangles in ascending (cell, tetrahedron,
    triangle) order with the normal pointing from inside to outside, and a face's indices are local to its volume.  A volume that
    the level does not cut gives two empty tensors.  Every axis has at least 2 nodes and 7 Gz Gy Gx < 2^31.

    The normals are the unit vectors of npcd.eval.mesh.vertex_normals_reference: minus the gradient of
    `gradient_of` (default: the volume; the volume's shape, fp32, on its device), interpolated along the vertex's edge with the
    vertex's own t; (0, 0, 0) where that is not finite.  For a volume that filter_components has cleaned, pass the unfiltered one."""
    if not isinstance(volume, torch.Tensor) or volume.dim() not in (3, 4):
        raise ValueError("isosurface: volume must be a tensor [B, Gz, Gy, Gx] or [Gz, Gy, Gx]")
    require_gpu(volume)
    if volume.dtype != torch.float32:
        raise RuntimeError(f"isosurface: the volume must be fp32; got {volume.dtype}")
    vol = (volume if volume.dim() == 4 else volume[None]).detach().contiguous()
    B, gz, gy, gx = vol.shape
    if min(B, gz, gy, gx) < 1 or min(gz, gy, gx) < 2:
        raise ValueError(f"isosurface: every axis needs at least 2 nodes; got {tuple(vol.shape)}")
    field = vol
    if gradient_of is not None:
        if not normals:
            raise ValueError("isosurface: gradient_of is the field of the normals; it needs normals=True")
        if not isinstance(gradient_of, torch.Tensor) or tuple(gradient_of.shape) != tuple(volume.shape):
            raise ValueError(f"isosurface: gradient_of must have the volume's shape {tuple(volume.shape)}")
        require_gpu(gradient_of)
        if gradient_of.dtype != torch.float32 or gradient_of.device != volume.device:
            raise RuntimeError(f"isosurface: gradient_of must be fp32 on the volume's device; got {gradient_of.dtype} on {gradient_of.device}")
        field = gradient_of.detach().reshape(vol.shape).contiguous()
    org = (ctypes.c_float * 3)(*_triple(origin, "origin"))
    step = (ctypes.c_float * 3)(*_triple(spacing, "spacing"))
    dev = vol.device
    with torch.cuda.device(dev):
        ws = torch.empty(workspace_bytes(B, gz, gy, gx), dtype=torch.uint8, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
        check(lib().npcd_isosurface_count(ptr(vol), B, gz, gy, gx, float(level), ptr(ws), ptr(counts), stream_ptr()),
              "npcd_isosurface_count")
        offsets = (torch.cumsum(counts, dim=0) - counts).t().contiguous()          # [2, B] exclusive, on the device
        sizes = counts.cpu()                                                        # the one host read
        n_vert, n_face = (int(v) for v in sizes.sum(dim=0))
        vertices = torch.empty((n_vert, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((n_face, 3), dtype=torch.int32, device=dev)
        unit = torch.empty((n_vert, 3), dtype=torch.float32, device=dev) if normals else None
        if n_vert:          # (every crossed edge lies in a tetrahedron: vertices and faces are empty together)
            check(lib().npcd_isosurface_emit(ptr(vol), B, gz, gy, gx, float(level), org, step, ptr(ws), ptr(offsets[0]), ptr(offsets[1]),
                                             ptr(vertices), ptr(faces), stream_ptr()), "npcd_isosurface_emit")
            if normals:
                check(lib().npcd_isosurface_normals(ptr(vol), ptr(field), B, gz, gy, gx, float(level), step, ptr(ws), ptr(offsets[0]),
                                                    ptr(unit), stream_ptr()), "npcd_isosurface_normals")
    out, v0, f0 = [], 0, 0
    for nv, nf in sizes.tolist():
        out.append((vertices[v0:v0 + nv], faces[f0:f0 + nf]) + ((unit[v0:v0 + nv],) if normals else ()))
        v0, f0 = v0 + nv, f0 + nf
    return out
