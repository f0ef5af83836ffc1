"""Points on the surfaces of triangle meshes, uniform by area, on their own kernels (csrc/surface.hip): what reads the
meshes of npcd.hip.isosurface / npcd.eval.mesh.extract_mesh back as clouds -- the 2,048-point inputs of the shape metrics, and the
`points` / `normals` of a raw stage-1 cloud.  `face_weights_reference` and `surface_sample_reference` of npcd/eval/mesh.py restate
the specification on the CPU.

The face weights are made integers before they are summed, so the prefix sums -- and with them the face of every sample -- do not
depend on the order of a scan: the same meshes and draws give the same bits on every run.  Nothing is read back from the device:
every size comes from a tensor's shape.  There is no CPU fallback: a non-GPU tensor or a wrong dtype raises RuntimeError.
"""
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

# faces per tile of the two-level prefix sums (kSurfTile of csrc/surface.h), and the tiles whose sums a sampling workgroup searches in
# LDS (kSurfLdsTiles): a mesh of more than TILE_FACES * LDS_TILES faces is searched in global memory
TILE_FACES = 256
LDS_TILES = 4096
MAX_CHANNELS = 16

Mesh = Union[Tuple[torch.Tensor, ...], dict]


def workspace_bytes(B: int, F_total: int) -> int:
    """Bytes of device workspace for B meshes of F_total faces together."""
    got = lib().npcd_surface_ws_bytes(B, F_total)
    check(min(got, 0), "npcd_surface_ws_bytes")
    return got


def _pair(mesh, who: str) -> Tuple[torch.Tensor, torch.Tensor]:
    if isinstance(mesh, dict):
        mesh = (mesh["vertices"], mesh["faces"])
    if not isinstance(mesh, (tuple, list)) or len(mesh) < 2 or not all(isinstance(t, torch.Tensor) for t in mesh[:2]):
        raise ValueError(f"{who}: a mesh is a pair (vertices [V, 3], faces [F, 3]) or a dict that holds them")
    vertices, faces = mesh[0], mesh[1]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{who}: vertices must be [V, 3] and faces [F, 3]; got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    require_gpu(vertices, faces)
    if vertices.dtype != torch.float32 or faces.dtype != torch.int32:
        raise RuntimeError(f"{who}: vertices must be fp32 and faces int32; got {vertices.dtype} and {faces.dtype}")
    if faces.device != vertices.device:
        raise RuntimeError(f"{who}: vertices on {vertices.device}, faces on {faces.device}")
    return vertices.detach(), faces


def _is_one(meshes) -> bool:
    return isinstance(meshes, dict) or (isinstance(meshes, (tuple, list)) and len(meshes) >= 2 and isinstance(meshes[0], torch.Tensor))


def _rows(tensors: Sequence[torch.Tensor], width: int) -> torch.Tensor:
    """The members' rows in one tensor, never of size 0 -- its pointer goes to the library."""
    packed = tensors[0] if len(tensors) == 1 else torch.cat(list(tensors))
    if packed.shape[0] == 0:
        return torch.zeros((1, width), dtype=packed.dtype, device=packed.device)
    return packed.contiguous()


class _Packed:
    """A batch of meshes as the library takes it: concatenated vertices and faces, the offsets on the device, and the workspace."""

    def __init__(self, meshes, who: str):
        self.single = _is_one(meshes)
        pairs = [_pair(m, who) for m in ([meshes] if self.single else list(meshes))]
        if not pairs:
            raise ValueError(f"{who}: no meshes")
        self.device = pairs[0][0].device
        if any(v.device != self.device for v, _ in pairs):
            raise RuntimeError(f"{who}: the meshes lie on different devices")
        self.B = len(pairs)
        self.V = [int(v.shape[0]) for v, _ in pairs]
        self.F = [int(f.shape[0]) for _, f in pairs]
        self.V_total, self.F_total = sum(self.V), sum(self.F)
        if self.V_total >= 2 ** 31 or self.F_total >= 2 ** 31:
            raise ValueError(f"{who}: {self.V_total} vertices and {self.F_total} faces; each total must stay below 2^31")
        self.vertices = _rows([v for v, _ in pairs], 3)
        self.faces = _rows([f for _, f in pairs], 3)
        offsets = [[0], [0]]
        for nv, nf in zip(self.V, self.F):
            offsets[0].append(offsets[0][-1] + nv)
            offsets[1].append(offsets[1][-1] + nf)
        self.offsets = torch.tensor(offsets, dtype=torch.int32).to(self.device, non_blocking=True)          # [2, B + 1]
        self.ws = None

    def prepare(self) -> torch.Tensor:
        """-> area [B] float64; leaves the prefix sums in the workspace."""
        with torch.cuda.device(self.device):
            self.ws = torch.empty(workspace_bytes(self.B, self.F_total) // 8 + 1, dtype=torch.int64, device=self.device)
            area = torch.empty(self.B, dtype=torch.float64, device=self.device)
            check(lib().npcd_surface_prepare(ptr(self.vertices), ptr(self.faces), ptr(self.offsets[0]), ptr(self.offsets[1]), self.B,
                                             self.V_total, self.F_total, ptr(self.ws), ptr(area), stream_ptr()), "npcd_surface_prepare")
        return area

    def per_vertex(self, given, width: Optional[int], name: str, who: str) -> torch.Tensor:
        """`given`: one [V, width] tensor per mesh (or one tensor for a single mesh) -> the packed rows."""
        rows = [given] if isinstance(given, torch.Tensor) else list(given)
        if len(rows) != self.B:
            raise ValueError(f"{who}: {len(rows)} {name} tensors for {self.B} meshes")
        width = int(rows[0].shape[1]) if width is None and isinstance(rows[0], torch.Tensor) and rows[0].dim() == 2 else width
        for t, nv in zip(rows, self.V):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or tuple(t.shape) != (nv, width):
                raise ValueError(f"{who}: {name} must be [V, {width}] per mesh; got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} for V = {nv}")
            require_gpu(t)
            if t.dtype != torch.float32 or t.device != self.device:
                raise RuntimeError(f"{who}: {name} must be fp32 on the meshes' device; got {t.dtype} on {t.device}")
        return _rows([t.detach() for t in rows], width)


def surface_area(meshes) -> torch.Tensor:
    """meshes: one (vertices [V, 3] fp32, faces [F, 3] int32) pair on the GPU or a list of them -> area [B] float64 (a 0-dim tensor for
    one pair): 0.5 float64(W) 2^-k of the integer face weights, the area that the sampler is uniform on; 0 for a mesh without
    faces or measure."""
    packed = _Packed(meshes, "surface_area")
    area = packed.prepare()
    return area[0] if packed.single else area


def sample_surface(meshes, num_samples: int, u: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None,
                   normals=None, attributes=None, return_faces: bool = False):
    """meshes: one (vertices [V, 3] fp32, faces [F, 3] int32) pair on the GPU or a list of B of them (tuples as isosurface, dicts as
    extract_mesh returns them) -> (points [B, S, 3] fp32, area [B] float64) and then, in this order, whichever of
    normals [B, S, 3], attributes [B, S, C] and faces [B, S] int32 were asked for; without the leading B for one pair.

    S = num_samples points per mesh, uniform by area, the bits of npcd.eval.mesh.surface_sample_reference: the face of a sample from
    u[..., 0] through integer prefix sums of the face weights, the point from u[..., 1:] as (1 - s) v0 + s (1 - u2) v1 + s u2 v2 with
    s = sqrt(u1).  u [B, S, 3] ([S, 3] for one pair) fp32 on the device; None draws torch.rand((B, S, 3), generator=generator) there.
    normals="face": the unit normal of the sample's face, following its winding (outward for an isosurface); normals = a [V, 3] fp32
    tensor per mesh: the vertex normals interpolated at the sample and normalised, (0, 0, 0) where that is not finite.
    attributes = a [V, C] fp32 tensor per mesh, 1 <= C <= 16 (colours): interpolated, not normalised.  faces are local to their
    mesh.  A mesh without faces or without measure gives area 0, face -1 and zeros in every other row."""
    who = "sample_surface"
    S = int(num_samples)
    if S < 1:
        raise ValueError(f"{who}: num_samples must be at least 1; got {num_samples}")
    packed = _Packed(meshes, who)
    B, dev = packed.B, packed.device
    mode, vertex_normals = 0, None
    if isinstance(normals, str):
        if normals != "face":
            raise ValueError(f"{who}: normals is \"face\" or the meshes' vertex normals; got {normals!r}")
        mode = 1
    elif normals is not None:
        mode, vertex_normals = 2, packed.per_vertex(normals, 3, "normals", who)
    attrs, C = None, 0
    if attributes is not None:
        attrs = packed.per_vertex(attributes, None, "attributes", who)
        C = int(attrs.shape[1])
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"{who}: attributes must have 1 to {MAX_CHANNELS} channels; got {C}")
    if B * S * max(3, C) >= 2 ** 31:
        raise ValueError(f"{who}: {B} meshes x {S} samples x {max(3, C)} values must stay below 2^31")
    if u is None:
        u = torch.rand((B, S, 3), generator=generator, dtype=torch.float32, device=dev)
    else:
        if not isinstance(u, torch.Tensor) or tuple(u.shape) not in ([(B, S, 3)] + ([(S, 3)] if packed.single else [])):
            raise ValueError(f"{who}: u must be [{B}, {S}, 3]; got {tuple(u.shape) if isinstance(u, torch.Tensor) else type(u)}")
        require_gpu(u)
        if u.dtype != torch.float32 or u.device != dev:
            raise RuntimeError(f"{who}: u must be fp32 on the meshes' device; got {u.dtype} on {u.device}")
        u = u.detach().reshape(B, S, 3).contiguous()
    area = packed.prepare()
    with torch.cuda.device(dev):
        points = torch.empty((B, S, 3), dtype=torch.float32, device=dev)
        faces_out = torch.empty((B, S), dtype=torch.int32, device=dev) if return_faces else None
        normals_out = torch.empty((B, S, 3), dtype=torch.float32, device=dev) if mode else None
        attrs_out = torch.empty((B, S, C), dtype=torch.float32, device=dev) if C else None
        check(lib().npcd_surface_sample(ptr(packed.vertices), ptr(packed.faces), ptr(packed.offsets[0]), ptr(packed.offsets[1]), B,
                                        packed.V_total, packed.F_total, ptr(packed.ws), ptr(u), S, ptr(points), ptr(faces_out), mode,
                                        ptr(vertex_normals), ptr(normals_out), ptr(attrs), C, ptr(attrs_out), stream_ptr()),
              "npcd_surface_sample")
    out = [points, area] + [t for t in (normals_out, attrs_out, faces_out) if t is not None]
    return tuple(t[0] for t in out) if packed.single else tuple(out)
