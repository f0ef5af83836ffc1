"""Generated objects as triangle meshes: the density of a PointNeRF field on a lattice (PointNeRF.density_grid), its isosurface on
the GPU (npcd.hip.isosurface, csrc/isosurface.hip) and the field's colour at the vertices (PointNeRF.query_field), plus a PLY
writer.  `marching_tetrahedra_reference` restates the surface's specification in numpy; the kernel is held to it
bit for bit (tests/test_gpu_isosurface.py), and it is held to geometry (tests/test_isosurface_cpu.py).

This module imports without a GPU; only extract_mesh needs one."""
import itertools
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

# the seven edge types of a node as (dx, dy, dz); the lower end owns the edge
EDGE_TYPES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


def _oriented_polygon(chain: np.ndarray, inside: Sequence[int]):
    """The polygon that cuts the tetrahedron `chain` [4, 3] (integer corners) between its `inside` corners and the others, as a
    cycle of chain edges (u, v), wound so that its normal points from the inside corners to the outside ones.  Decided from the
    geometry of the edge midpoints in exact integer arithmetic (twice the midpoints): one decision per corner pattern, the same for
    every cell."""
    ins = [k for k in range(4) if k in inside]
    out = [k for k in range(4) if k not in inside]
    if len(ins) == 1:
        poly = [(ins[0], o) for o in out]
    elif len(ins) == 3:
        poly = [(i, out[0]) for i in ins]
    else:
        (i, j), (k, l) = ins, out
        poly = [(i, k), (i, l), (j, l), (j, k)]          # neighbours in the cycle share a corner of the tetrahedron
    mid = [chain[u] + chain[v] for u, v in poly]
    normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    toward = len(ins) * sum(chain[o] for o in out) - len(out) * sum(chain[i] for i in ins)          # centroid(out) - centroid(in), scaled
    side = int(np.dot(normal, toward))
    assert side != 0
    return poly if side > 0 else poly[::-1]


def marching_tetrahedra_reference(volume, level: float, origin: Sequence[float] = (0.0, 0.0, 0.0),
                                  spacing: Sequence[float] = (1.0, 1.0, 1.0)):
    """volume [Gz, Gy, Gx] (x fastest) -> (vertices [V, 3] float32, faces [F, 3] int32): the specification of the isosurface on the
    CPU, float32 arithmetic as written.

    Inside: f > level.  An edge of one of the seven EDGE_TYPES whose ends differ carries the vertex origin + spacing * (i + d t),
    t = (level - f_lo) / (f_hi - f_lo); vertices ascend in (node, type), node (x, y, z) = (z Gy + y) Gx + x.  A cell is cut into the six
    chains v0, v0 + e_a, v0 + e_a + e_b, v0 + e_a + e_b + e_c, (a, b, c) the permutations of (x, y, z) in lexicographic order; a
    chain with 1 or 3 corners inside gives a triangle, with 2 a quadrilateral, the normal pointing from inside to outside.  A
    triangle starts with its smallest index, a quadrilateral is split along the diagonal through its smallest index; triangles
    ascend in (cell, tetrahedron, triangle)."""
    f = np.ascontiguousarray(np.asarray(volume, dtype=np.float32))
    if f.ndim != 3 or min(f.shape) < 2:
        raise ValueError(f"marching_tetrahedra_reference: a volume [Gz, Gy, Gx] with at least 2 nodes per axis; got {f.shape}")
    gz, gy, gx = f.shape
    level = np.float32(level)
    origin = np.asarray(origin, dtype=np.float32)
    spacing = np.asarray(spacing, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        inside = f > level
    # ---- vertices: one per crossed edge --------------------------------------------------------------------------------------------
    vid = np.full((7, gz, gy, gx), -1, dtype=np.int64)
    keys, points, where = [], [], []
    for t, (dx, dy, dz) in enumerate(EDGE_TYPES):
        lo = (slice(0, gz - dz), slice(0, gy - dy), slice(0, gx - dx))
        hi = (slice(dz, gz), slice(dy, gy), slice(dx, gx))
        z, y, x = np.nonzero(inside[lo] != inside[hi])
        f_lo, f_hi = f[z, y, x], f[z + dz, y + dy, x + dx]
        with np.errstate(all="ignore"):
            s = (level - f_lo) / (f_hi - f_lo)
            zero = np.zeros_like(s)
            g = [i.astype(np.float32) + (s if d else zero) for i, d in ((x, dx), (y, dy), (z, dz))]
            points.append(np.stack([origin[a] + spacing[a] * g[a] for a in range(3)], axis=1).astype(np.float32))
        keys.append(((z * gy + y) * gx + x) * 7 + t)
        where.append(np.stack([np.full_like(z, t), z, y, x], axis=1))
    keys, points, where = np.concatenate(keys), np.concatenate(points), np.concatenate(where)
    order = np.argsort(keys, kind="stable")
    vertices = points[order]
    where = where[order]
    vid[where[:, 0], where[:, 1], where[:, 2], where[:, 3]] = np.arange(len(order))
    # ---- faces: six chains per cell ------------------------------------------------------------------------------------------------
    Z, Y, X = (a.reshape(-1) for a in np.meshgrid(np.arange(gz - 1), np.arange(gy - 1), np.arange(gx - 1), indexing="ij"))
    cell = (Z * gy + Y) * gx + X
    face_keys, face_rows = [], []
    for tet, perm in enumerate(itertools.permutations(range(3))):          # axis 0 = x, 1 = y, 2 = z
        chain = np.zeros((4, 3), dtype=np.int64)
        for step, axis in enumerate(perm):
            chain[step + 1] = chain[step]
            chain[step + 1, axis] += 1
        corner_in = [inside[Z + c[2], Y + c[1], X + c[0]] for c in chain]
        pattern = sum(corner_in[k].astype(np.int64) << k for k in range(4))
        for p in range(1, 15):
            sel = np.nonzero(pattern == p)[0]
            if sel.size == 0:
                continue
            poly = _oriented_polygon(chain, [k for k in range(4) if p >> k & 1])
            cols = []
            for u, v in poly:
                u, v = min(u, v), max(u, v)
                t = EDGE_TYPES.index(tuple(int(d) for d in chain[v] - chain[u]))
                cols.append(vid[t, Z[sel] + chain[u, 2], Y[sel] + chain[u, 1], X[sel] + chain[u, 0]])
            rows = np.stack(cols, axis=1)
            assert (rows >= 0).all()
            n = rows.shape[1]
            first = np.argmin(rows, axis=1)
            rows = np.take_along_axis(rows, (first[:, None] + np.arange(n)[None, :]) % n, axis=1)
            base = (cell[sel] * 6 + tet) * 2
            if n == 3:
                face_rows.append(rows)
                face_keys.append(base)
            else:
                face_rows += [rows[:, [0, 1, 2]], rows[:, [0, 2, 3]]]
                face_keys += [base, base + 1]
    if not face_rows:
        return vertices.reshape(-1, 3), np.zeros((0, 3), dtype=np.int32)
    face_keys, face_rows = np.concatenate(face_keys), np.concatenate(face_rows)
    faces = face_rows[np.argsort(face_keys, kind="stable")].astype(np.int32)
    return vertices, faces


def default_level(pointnerf) -> float:
    """ln 2 / (2 cube_scale / (depth_resolution - 1)): the density at which one depth step of an axis-parallel ray through the box
    is half opaque."""
    r = pointnerf.renderer
    return math.log(2.0) / (2.0 * float(r.cube_scale) / (int(r.depth_resolution) - 1))


@torch.no_grad()
def extract_mesh(pointnerf, coords: torch.Tensor, feats: torch.Tensor, resolution=128, level: Optional[float] = None, colors: bool = True,
                 bound: Optional[float] = None, mlp_dtype=None, view_dir: Optional[torch.Tensor] = None) -> List[Dict[str, torch.Tensor]]:
    """coords [B, N, 3], feats [B, N, F] on the GPU -> per cloud {"vertices" [V, 3] fp32, "faces" [F, 3] int32, "colors" [V, 3] fp32
    in [0, 1] (with colors=True)}, all on the GPU.

    The density on PointNeRF.density_grid(resolution, bound), its isosurface at `level` (npcd.hip.isosurface), and the field's
    colour at the vertices (PointNeRF.query_field; `view_dir` [3] for a field with view directions, `mlp_dtype` as for render).
    level=None takes default_level(pointnerf).  Nobody has looked at this default on trained weights: it is a statement about one
    depth step of the renderer, not about where a trained car's surface lies -- choose the level by eye."""
    from ..hip.isosurface import isosurface
    sigma, origin, spacing = pointnerf.density_grid(coords, feats, resolution=resolution, bound=bound, mlp_dtype=mlp_dtype)
    meshes = isosurface(sigma, default_level(pointnerf) if level is None else float(level), origin, spacing)
    out = []
    for b, (vertices, faces) in enumerate(meshes):
        mesh = {"vertices": vertices, "faces": faces}
        if colors:
            if vertices.shape[0]:
                mesh["colors"] = pointnerf.query_field(coords[b:b + 1], feats[b:b + 1], vertices[None], mlp_dtype=mlp_dtype,
                                                       view_dir=view_dir)[1][0]
            else:
                mesh["colors"] = torch.zeros((0, 3), dtype=torch.float32, device=vertices.device)
        out.append(mesh)
    return out


def colors_to_uint8(colors) -> np.ndarray:
    """[V, 3] colours as PLY stores them: uint8 as they are, floats in [0, 1] clipped and rounded to 0..255."""
    c = colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
    if c.dtype == np.uint8:
        return np.ascontiguousarray(c)
    return np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def write_ply(path, vertices, faces, colors=None) -> None:
    """Binary little-endian PLY, written on the host: float32 x y z, optional uchar red green blue, faces as `uchar int` lists."""
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    v = np.asarray(v, dtype="<f4").reshape(-1, 3)
    f = np.asarray(f, dtype="<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if colors is not None:
        c = colors_to_uint8(colors).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"write_ply: {len(v)} vertices and {len(c)} colours")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.empty(len(v), dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
