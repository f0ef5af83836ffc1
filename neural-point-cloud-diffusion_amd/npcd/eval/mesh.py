"""Generated objects as triangle meshes: the density of a PointNeRF field on a lattice (PointNeRF.density_grid), its isosurface on
the GPU (npcd.hip.isosurface, csrc/isosurface.hip) and the field's colour at the vertices (PointNeRF.query_field), plus a PLY
writer.  `marching_tetrahedra_reference` restates the surface's specification in numpy; the kernel is held to it
bit for bit (tests/test_gpu_isosurface.py), and it is held to geometry (tests/test_isosurface_cpu.py).  What finishes a mesh is
specified the same way: `connected_components_reference`, `select_components` and `filter_components_reference`
for dropping floaters from the volume, `vertex_normals_reference` for the normals.  Reading a mesh back as a cloud is specified the
same way: `face_weights_reference` and `surface_sample_reference` restate npcd.hip.surface, and
`sample_mesh_clouds` draws the clouds that the shape metrics take.  Bringing a mesh down to a usable triangle count likewise
(DESIGN.md 5.16): `simplify_reference` restates npcd.hip.simplify, exact vertex clustering, and extract_mesh(simplify=k) applies it.
What a mesh's connectivity is and Taubin smoothing likewise: `mesh_edges_reference` and `smooth_reference` restate
npcd.hip.smooth, `mesh_topology` reports edges, boundary and non-manifold edges and the Euler characteristic, and
extract_mesh(smooth=n, topology=True) applies both.  How far two surfaces lie apart likewise:
`point_mesh_distance_reference` restates npcd.hip.mesh_distance, `mesh_deviation` and `cloud_mesh_distance` report mean, rms and
maximum distances, and extract_mesh(deviation=n) says what simplifying and smoothing cost.  Looking at a mesh likewise (DESIGN.md
5.19): `ray_mesh_reference` restates npcd.hip.raycast, `render_mesh` gives mask, depth, face, normal and colour at the renderer's own
rays, `mesh_render_agreement` compares them with the field's render, and extract_mesh(agreement=cameras) reports it.  Telling
inside from outside likewise: `crossings_reference` restates npcd.hip.crossings, `voxelize_mesh`,
`mesh_signed_distance` and `mesh_volume_iou` rest on it, and extract_mesh(enclosure=True) reports whether the mesh encloses what the
field calls solid (`mesh_enclosure`).

This module imports without a GPU; only extract_mesh, sample_mesh_clouds, mesh_deviation, cloud_mesh_distance, render_mesh,
mesh_render_agreement, voxelize_mesh, mesh_signed_distance, mesh_volume_iou and mesh_enclosure need one."""
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


def _volume(volume, who: str) -> np.ndarray:
    f = np.ascontiguousarray(np.asarray(volume, dtype=np.float32))
    if f.ndim != 3 or min(f.shape) < 2:
        raise ValueError(f"{who}: a volume [Gz, Gy, Gx] with at least 2 nodes per axis; got {f.shape}")
    return f


def connected_components_reference(volume, level: float) -> np.ndarray:
    """volume [Gz, Gy, Gx] -> labels int64 [Gz, Gy, Gx]: the specification of the component labelling on the CPU.

    Inside: f > level, as in the isosurface (NaN is outside).  Two inside nodes are adjacent iff they are the two ends of one lattice
    edge of the seven EDGE_TYPES -- the edges of the Kuhn triangulation, 14 neighbours a node; the anti-diagonals do not connect.
    A node outside gets -1, a node inside the smallest node index (z Gy + y) Gx + x of its component.

    Hooking and pointer jumping: every edge whose ends carry different labels lowers the larger label's own entry to the smaller
    (a minimum, so the order of the edges does not matter), then every node takes its label's label until nothing changes; repeated
    until no edge has two labels.  At that point a label is constant on a component, is one of its nodes, and is at most every node
    that carries it: the smallest."""
    f = _volume(volume, "connected_components_reference")
    gz, gy, gx = f.shape
    with np.errstate(invalid="ignore"):
        inside = f > np.float32(level)
    index = np.arange(f.size, dtype=np.int64).reshape(f.shape)
    lower, upper = [], []
    for dx, dy, dz in EDGE_TYPES:
        lo = (slice(0, gz - dz), slice(0, gy - dy), slice(0, gx - dx))
        hi = (slice(dz, gz), slice(dy, gy), slice(dx, gx))
        both = inside[lo] & inside[hi]
        lower.append(index[lo][both])
        upper.append(index[hi][both])
    a, b = np.concatenate(lower), np.concatenate(upper)
    labels = np.where(inside, index, -1).reshape(-1)
    nodes = np.nonzero(inside.reshape(-1))[0]
    while a.size:
        la, lb = labels[a], labels[b]
        differ = la != lb
        a, b, la, lb = a[differ], b[differ], la[differ], lb[differ]          # equal labels stay equal: the edge is done
        np.minimum.at(labels, np.maximum(la, lb), np.minimum(la, lb))
        while True:
            jumped = labels[labels[nodes]]
            if np.array_equal(jumped, labels[nodes]):
                break
            labels[nodes] = jumped
    return labels.reshape(f.shape)


def select_components(labels, largest: Optional[int] = None, min_nodes: Optional[int] = None) -> np.ndarray:
    """labels as connected_components_reference gives them -> the roots of the kept components, ascending (int64).

    largest=k keeps the k components with the most nodes, ties to the smaller root; min_nodes=m those with at least m nodes; both
    the intersection, neither all."""
    if largest is not None and int(largest) < 1:
        raise ValueError(f"select_components: largest must be at least 1; got {largest}")
    if min_nodes is not None and int(min_nodes) < 1:
        raise ValueError(f"select_components: min_nodes must be at least 1; got {min_nodes}")
    labels = np.asarray(labels)
    roots, nodes = np.unique(labels[labels >= 0], return_counts=True)
    keep = np.ones(len(roots), dtype=bool)
    if largest is not None:
        keep[np.lexsort((roots, -nodes))[int(largest):]] = False          # by (-nodes, root)
    if min_nodes is not None:
        keep &= nodes >= int(min_nodes)
    return roots[keep].astype(np.int64)


def filter_components_reference(volume, level: float, largest: Optional[int] = None, min_nodes: Optional[int] = None) -> np.ndarray:
    """The volume with every inside node of a component that select_components does not keep set to float32(level) -- outside, and
    no crossing on an edge to another outside node; everything else bit for bit.  A removed node has no kept inside node on any of its
    Kuhn edges, so the isosurface of the result is the isosurface of the volume without the removed components' vertices and faces."""
    f = _volume(volume, "filter_components_reference")
    labels = connected_components_reference(f, level)
    kept = select_components(labels, largest, min_nodes)
    out = f.copy()
    out[(labels >= 0) & ~np.isin(labels, kept)] = np.float32(level)
    return out


def node_gradient_reference(field, spacing: Sequence[float]) -> np.ndarray:
    """field [Gz, Gy, Gx] -> [3, Gz, Gy, Gx] float32, the gradient (x, y, z) at the nodes as written: central differences
    (f[i + 1] - f[i - 1]) / (2 s) in the interior, one-sided (f[1] - f[0]) / (1 s) and (f[last] - f[last - 1]) / (1 s) at the borders."""
    f = _volume(field, "node_gradient_reference")
    spacing = np.asarray(spacing, dtype=np.float32)
    out = np.empty((3,) + f.shape, dtype=np.float32)
    with np.errstate(all="ignore"):
        for a in range(3):          # axis a = x, y, z is array axis 2 - a
            m = np.moveaxis(f, 2 - a, 0)
            g = np.moveaxis(out[a], 2 - a, 0)
            g[1:-1] = (m[2:] - m[:-2]) / (np.float32(2) * spacing[a])
            g[0] = (m[1] - m[0]) / (np.float32(1) * spacing[a])
            g[-1] = (m[-1] - m[-2]) / (np.float32(1) * spacing[a])
    return out


def vertex_normals_reference(volume, level: float, spacing: Sequence[float] = (1.0, 1.0, 1.0), gradient_of=None) -> np.ndarray:
    """-> [V, 3] float32 unit normals in the vertex order of marching_tetrahedra_reference(volume, level, ., spacing): the
    specification of the isosurface's vertex normals on the CPU, float32 arithmetic as written.

    The vertex on the edge (lo, hi) with the isosurface's t = (level - f_lo) / (f_hi - f_lo), f from `volume`, takes the gradient
    g = g_lo + t (g_hi - g_lo) of `gradient_of` (default: the volume; node_gradient_reference), n2 = (gx gx + gy gy) + gz gz and
    n = (-g) / sqrt(n2): the density falls toward the outside.  A vertex with a component that is not finite gets (+0, +0, +0)."""
    f = _volume(volume, "vertex_normals_reference")
    field = f if gradient_of is None else _volume(gradient_of, "vertex_normals_reference")
    if field.shape != f.shape:
        raise ValueError(f"vertex_normals_reference: gradient_of {field.shape} is not the volume's shape {f.shape}")
    gz, gy, gx = f.shape
    level = np.float32(level)
    grad = node_gradient_reference(field, spacing)
    with np.errstate(invalid="ignore"):
        inside = f > level
    keys, rows = [], []
    for t, (dx, dy, dz) in enumerate(EDGE_TYPES):
        lo = (slice(0, gz - dz), slice(0, gy - dy), slice(0, gx - dx))
        hi = (slice(dz, gz), slice(dy, gy), slice(dx, gx))
        z, y, x = np.nonzero(inside[lo] != inside[hi])
        with np.errstate(all="ignore"):
            s = (level - f[z, y, x]) / (f[z + dz, y + dy, x + dx] - f[z, y, x])
            g_lo, g_hi = grad[:, z, y, x], grad[:, z + dz, y + dy, x + dx]
            g = g_lo + s * (g_hi - g_lo)
            n2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
            rows.append(((-g) / np.sqrt(n2)).T.astype(np.float32))
        keys.append(((z * gy + y) * gx + x) * 7 + t)
    normals = np.concatenate(rows)[np.argsort(np.concatenate(keys), kind="stable")].reshape(-1, 3)
    normals[~np.isfinite(normals).all(axis=1)] = 0.0
    return normals


def _mesh_arrays(vertices, faces, who: str):
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32)).reshape(-1, 3)
    f = np.ascontiguousarray(np.asarray(faces)).reshape(-1, 3)
    if f.size and not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"{who}: faces must be integers; got {f.dtype}")
    return v, f.astype(np.int64)


def face_weights_reference(vertices, faces):
    """vertices [V, 3], faces [F, 3] -> (weights uint64 [F], k, d float32 [F], n float32 [F, 3]): the integer face weights of the
    surface sampler on the CPU, float32 arithmetic as written.

    e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2, d = sqrt((nx nx + ny ny) + nz nz) -- twice the area; d = +0 where it is not finite or
    an index lies outside [0, V).  d_max the largest d, k = 31 - floor(log2 d_max) from the exponent of float64(d_max), and
    w = floor(float64(d) 2^k): the scaling is exact, d_max maps into [2^31, 2^32), a face below 2^-31 of the largest weighs 0.  Integers,
    so every order of summation gives the same prefix sums.  k is None for a mesh without measure (all weights 0)."""
    v, f = _mesh_arrays(vertices, faces, "face_weights_reference")
    valid = ((f >= 0) & (f < len(v))).all(axis=1)
    safe = np.where(valid[:, None], f, 0) if len(v) else np.zeros_like(f)
    corners = v[safe] if len(v) else np.zeros((len(f), 3, 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        e1, e2 = corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1).astype(np.float32)
        d = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(np.float32)
    d = np.where(valid & np.isfinite(d), d, np.float32(0.0)).astype(np.float32)
    d_max = float(d.view(np.uint32).max().view(np.float32)) if len(d) else 0.0          # the integer maximum of the bits: d >= +0
    if d_max == 0.0:
        return np.zeros(len(f), dtype=np.uint64), None, d, n
    k = 31 - (math.frexp(d_max)[1] - 1)          # frexp: d_max = m 2^e with m in [0.5, 1), exact for denormals too
    weights = np.floor(np.ldexp(d.astype(np.float64), k)).astype(np.uint64)
    return weights, k, d, n


def surface_sample_reference(vertices, faces, u, normals=None, attributes=None) -> Dict[str, np.ndarray]:
    """One mesh (vertices [V, 3], faces [F, 3]) and uniform draws u [S, 3] -> {"points" [S, 3] float32, "face" [S] int32, "area"
    float64, and "normals" [S, 3] / "attributes" [S, C] float32 where asked for}: the specification of the surface sampler on the
    CPU, float32 arithmetic as written.

    With the weights w of face_weights_reference, C their inclusive sums (integers) and W the last: k0 = clamp(floor(u0 2^24), 0,
    2^24 - 1) (NaN: 0), r = floor(k0 W / 2^24) in exact integer arithmetic, the face the smallest i with C_i > r -- a face of weight 0
    is never chosen.  s = sqrt(u1), b = (1 - s, s (1 - u2), s u2), p = (b0 v0 + b1 v1) + b2 v2.  normals="face": n / d of the face;
    normals [V, 3]: g = (b0 g0 + b1 g1) + b2 g2, g / sqrt((gx gx + gy gy) + gz gz), (+0, +0, +0) where a component is not finite;
    attributes [V, C]: the same three-term expression.  area = 0.5 float64(W) 2^-k.  A mesh without faces or measure: area 0, face -1
    and +0 in every other row."""
    v, f = _mesh_arrays(vertices, faces, "surface_sample_reference")
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float32))
    if u.ndim != 2 or u.shape[1] != 3:
        raise ValueError(f"surface_sample_reference: u must be [S, 3]; got {u.shape}")
    S = len(u)
    face_mode = isinstance(normals, str)
    if face_mode and normals != "face":
        raise ValueError(f"surface_sample_reference: normals is \"face\" or a [V, 3] array; got {normals!r}")
    vn = None if normals is None or face_mode else np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    at = None if attributes is None else np.asarray(attributes, dtype=np.float32)
    if vn is not None and len(vn) != len(v):
        raise ValueError(f"surface_sample_reference: {len(v)} vertices and {len(vn)} normals")
    if at is not None and (at.ndim != 2 or len(at) != len(v)):
        raise ValueError(f"surface_sample_reference: attributes must be [{len(v)}, C]; got {at.shape}")
    weights, k, d, n = face_weights_reference(v, f)
    out = {"points": np.zeros((S, 3), dtype=np.float32), "face": np.full(S, -1, dtype=np.int32), "area": np.float64(0.0)}
    if normals is not None:
        out["normals"] = np.zeros((S, 3), dtype=np.float32)
    if at is not None:
        out["attributes"] = np.zeros((S, at.shape[1]), dtype=np.float32)
    if k is None:
        return out
    sums = np.cumsum(weights, dtype=np.uint64)
    W = int(sums[-1])
    out["area"] = np.float64(math.ldexp(0.5 * float(W), -k))          # float(W): the nearest float64, ties to even
    with np.errstate(invalid="ignore"):
        t = np.floor(u[:, 0] * np.float32(16777216.0))
    k0 = np.where(t > 0, np.minimum(t, np.float32(16777215.0)), np.float32(0.0)).astype(np.int64)          # NaN > 0 is false
    r = np.array([(int(q) * W) >> 24 for q in k0], dtype=np.uint64)
    face = np.searchsorted(sums, r, side="right")
    assert (face < len(f)).all() and (weights[face] > 0).all()
    out["face"] = face.astype(np.int32)

    def mix(rows):          # rows [S, 3 corners, C] float32
        return ((b0[:, None] * rows[:, 0] + b1[:, None] * rows[:, 1]) + b2[:, None] * rows[:, 2]).astype(np.float32)
    with np.errstate(all="ignore"):
        s = np.sqrt(u[:, 1]).astype(np.float32)
        one = np.float32(1.0)
        b0, b1, b2 = one - s, s * (one - u[:, 2]), s * u[:, 2]
        idx = f[face]
        out["points"] = mix(v[idx])
        if face_mode:
            out["normals"] = (n[face] / d[face][:, None]).astype(np.float32)
        elif vn is not None:
            g = mix(vn[idx])
            unit = (g / np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]).astype(np.float32)
            unit[~np.isfinite(unit).all(axis=1)] = 0.0
            out["normals"] = unit
        if at is not None:
            out["attributes"] = mix(at[idx])
    return out


MAX_CLUSTER_CELLS = 2 ** 30


def clustering_grid(cell, origin=None, dims=None, lower=None, upper=None):
    """The grid of simplify_reference / npcd.hip.simplify.simplify_mesh as host values -> (origin [3] float64, cell [3] float64,
    dims [3] int).  `cell`: a float or three (x, y, z), finite and positive.  origin=None takes `lower`, the smallest coordinates of
    the finite vertices; dims=None takes floor((upper - origin) / cell) + 1 per axis in float64, at least 1 -- the cells that reach the
    largest coordinates.  Without a finite vertex (lower and upper None) the origin is 0 and the grid one cell."""
    cell = np.array(np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,)))
    if not (np.isfinite(cell).all() and (cell > 0).all()):
        raise ValueError(f"clustering_grid: cell must be finite and positive; got {cell.tolist()}")
    if origin is None:
        origin = np.zeros(3) if lower is None else np.asarray(lower, dtype=np.float64)
    origin = np.array(np.broadcast_to(np.asarray(origin, dtype=np.float64), (3,)))
    if not np.isfinite(origin).all():
        raise ValueError(f"clustering_grid: origin must be finite; got {origin.tolist()}")
    if dims is None:
        if upper is None:
            dims = [1, 1, 1]
        else:
            reach = np.floor((np.asarray(upper, dtype=np.float64) - origin) / cell)
            dims = [int(min(max(d, 0.0), float(2 ** 31 - 2))) + 1 for d in reach]
    dims = [int(d) for d in dims]
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"clustering_grid: dims must be three positive integers; got {dims}")
    if dims[0] * dims[1] * dims[2] > MAX_CLUSTER_CELLS:
        raise ValueError(f"clustering_grid: {dims[0]} x {dims[1]} x {dims[2]} = {dims[0] * dims[1] * dims[2]} cells; at most 2^30 = "
                         f"{MAX_CLUSTER_CELLS} -- take a larger cell")
    return origin, cell, dims


def attribute_means_reference(attributes, cluster, num_clusters: int) -> np.ndarray:
    """attributes [V, C], cluster [V] (-1: none) -> the cluster means [num_clusters, C] as FLOAT64, before simplify_reference rounds
    them to float32.

    A = the largest finite |a| of the whole array, e = floor(log2 A), the quantum 2^(e - 30): q = rint(float64(a) 2^(30 - e)), an
    integer of at most 2^31 (a value that is not finite counts as 0; the product is exact), the sums of q over a cluster as signed
    64-bit integers, and the mean (float64(sum) / float64(n)) 2^(e - 30).  Every q is within half a quantum of its value, so the mean
    is within A 2^-31 of the exact one, and the one float64 division adds A 2^-53: inside A 2^-29."""
    a = np.ascontiguousarray(np.asarray(attributes, dtype=np.float32))
    cluster = np.asarray(cluster)
    out = np.zeros((num_clusters, a.shape[1]), dtype=np.float64)
    finite = np.isfinite(a)
    bits = np.where(finite, np.abs(a), np.float32(0.0)).astype(np.float32).view(np.uint32)
    top = float(bits.max().view(np.float32)) if a.size else 0.0          # the integer maximum of the bits: |a| >= +0
    if top == 0.0 or num_clusters == 0:
        return out
    shift = 30 - (math.frexp(top)[1] - 1)
    q = np.rint(np.ldexp(np.where(finite, a, np.float32(0.0)).astype(np.float64), shift)).astype(np.int64)
    member = cluster >= 0
    sums = np.zeros((num_clusters, a.shape[1]), dtype=np.int64)
    np.add.at(sums, cluster[member], q[member])
    n = np.bincount(cluster[member], minlength=num_clusters).astype(np.float64)
    return np.ldexp(sums.astype(np.float64) / n[:, None], -shift)


def simplify_reference(vertices, faces, cell, origin=None, dims=None, attributes=None) -> Dict[str, np.ndarray]:
    """One mesh (vertices [V, 3], faces [F, 3]) -> {"vertices" [V', 3] float32, "faces" [F', 3] int32, "vertex_cluster" [V] int32,
    "face_source" [F'] int32, and "attributes" [V', C] float32 where given}: the specification of vertex clustering (Rossignac and
    Borrel) on the CPU, float64 and integers.  The grid as clustering_grid makes it from cell, origin and dims.

    u = (float64(v) - origin) / cell per axis; a vertex with a u that is not finite is lost: cluster -1.  c = clamp(floor(u), 0,
    dims - 1), key = (cz dims_y + cy) dims_x + cx, and the cluster of a vertex is the rank of its key among the occupied cells, V' of
    them.  r = clamp(floor((u - c) 2^32), 0, 2^32 - 1), S the sum of r over the cluster and n its size, both integers: the
    representative is float32(origin + cell (c + (float64(S) / float64(n)) 2^-32)).  Attributes: attribute_means_reference, rounded
    to float32.  A face maps to its corners' clusters, corner order kept; it goes if an index lies outside [0, V), a corner is lost or
    two corners share a cluster, and among the others with the same SET of three clusters only the lowest input index stays.  The
    kept faces keep the input order; face_source holds their input indices.  The result may be non-manifold: clustering can pinch."""
    v, f = _mesh_arrays(vertices, faces, "simplify_reference")
    at = None if attributes is None else np.ascontiguousarray(np.asarray(attributes, dtype=np.float32))
    if at is not None and (at.ndim != 2 or len(at) != len(v) or not 1 <= at.shape[1] <= 16):
        raise ValueError(f"simplify_reference: attributes must be [{len(v)}, C] with 1 <= C <= 16; got {at.shape}")
    whole = np.isfinite(v).all(axis=1)
    lower, upper = (v[whole].min(axis=0), v[whole].max(axis=0)) if whole.any() else (None, None)
    origin, cell, dims = clustering_grid(cell, origin, dims, lower, upper)
    with np.errstate(all="ignore"):
        u = (v.astype(np.float64) - origin) / cell
        lost = ~np.isfinite(u).all(axis=1)
        top = np.asarray(dims, dtype=np.float64) - 1.0
        c = np.where(np.isfinite(u), np.minimum(np.maximum(np.floor(u), 0.0), top), 0.0)
        r = np.minimum(np.maximum(np.floor((u - c) * 4294967296.0), 0.0), 4294967295.0)
    r = np.where(np.isfinite(r), r, 0.0).astype(np.uint64)
    ci = c.astype(np.int64)
    key = np.where(lost, -1, (ci[:, 2] * dims[1] + ci[:, 1]) * dims[0] + ci[:, 0])
    occupied = np.unique(key[~lost])
    cluster = np.where(lost, -1, np.searchsorted(occupied, key)).astype(np.int64)
    count = len(occupied)
    S = np.zeros((count, 3), dtype=np.uint64)
    np.add.at(S, cluster[~lost], r[~lost])
    n = np.bincount(cluster[~lost], minlength=count).astype(np.uint64)
    cc = np.stack([occupied % dims[0], (occupied // dims[0]) % dims[1], occupied // dims[0] // dims[1]], axis=1).astype(np.float64)
    # np.float64(np.uint64): to the nearest float64, ties to even, as the device converts
    position = origin + cell * (cc + (S.astype(np.float64) / n.astype(np.float64)[:, None]) * 2.0 ** -32)
    out = {"vertices": position.astype(np.float32).reshape(-1, 3), "vertex_cluster": cluster.astype(np.int32)}
    if at is not None:
        out["attributes"] = attribute_means_reference(at, cluster, count).astype(np.float32)
    inside = ((f >= 0) & (f < len(v))).all(axis=1)
    m = cluster[np.where(inside[:, None], f, 0)] if len(v) else np.full_like(f, -1)
    valid = inside & (m >= 0).all(axis=1) & (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    source = np.nonzero(valid)[0]
    if len(source):
        _, first = np.unique(np.sort(m[source], axis=1), axis=0, return_index=True)          # the first row of every set of three
        source = source[np.sort(first)]
    out["faces"] = m[source].astype(np.int32).reshape(-1, 3)
    out["face_source"] = source.astype(np.int32)
    return out


MAX_EDGE_VERTICES, MAX_EDGE_FACES = 2 ** 31, 2 ** 28
COUNT_NAMES = ("distinct_pairs", "valid_faces", "used_vertices", "boundary_edges", "nonmanifold_edges", "misoriented_edges")


def mesh_edges_reference(num_vertices: int, faces) -> Dict[str, np.ndarray]:
    """faces [F, 3] over vertices 0 .. V - 1 -> {"row_start" [V + 1], "neighbours" [D], "edges" [E, 2], "edge_faces" [E], "edge_forward"
    [E] int32, "boundary_vertex" [V] uint8, "counts" [6] int64}: the specification of the mesh-edges operator on the CPU, integers only
    (DESIGN.md 5.17).

    A face is valid if its three indices lie in [0, V) and differ pairwise; every other face contributes nothing.  A valid face
    (i, j, k) gives the directed pairs i->j, j->k, k->i (forward) and the three reversed (backward); the key of a->b is a 2^31 + b.
    The D distinct keys in ascending order are the adjacency in CSR form: neighbours holds their b, row_start[v] the number of them
    with a < v, so a vertex's neighbours ascend and a vertex in no valid face has an empty row.  Those with a < b, in that order, are
    the E = D / 2 edges; edge_faces counts the valid faces that hold the edge, edge_forward those that traverse it as a->b.  counts =
    (D, valid faces, vertices with a row that is not empty, edges of one face, edges of three or more faces, edges of two faces that
    both traverse them the same way); boundary_vertex is 1 on the ends of an edge of one face."""
    V = int(num_vertices)
    f = np.ascontiguousarray(np.asarray(faces)).reshape(-1, 3)
    if f.size and not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"mesh_edges_reference: faces must be integers; got {f.dtype}")
    if not 0 <= V < MAX_EDGE_VERTICES or len(f) >= MAX_EDGE_FACES:
        raise ValueError(f"mesh_edges_reference: {V} vertices and {len(f)} faces; vertices must stay below 2^31 = {MAX_EDGE_VERTICES} and "
                         f"faces below 2^28 = {MAX_EDGE_FACES}")
    f = f.astype(np.int64)
    valid = ((f >= 0) & (f < V)).all(axis=1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    g = f[valid]
    a, b = g.reshape(-1), g[:, [1, 2, 0]].reshape(-1)
    forward = a * 2 ** 31 + b
    keys, runs = np.unique(np.concatenate([forward, b * 2 ** 31 + a]), return_counts=True)
    source, target = keys >> 31, keys & (2 ** 31 - 1)
    is_edge = source < target
    edge_keys = keys[is_edge]
    traversed = np.zeros(len(edge_keys), dtype=np.int64)
    np.add.at(traversed, np.searchsorted(edge_keys, forward[a < b]), 1)
    edge_faces = runs[is_edge]
    counts = np.array([len(keys), len(g), len(np.unique(source)), int((edge_faces == 1).sum()), int((edge_faces >= 3).sum()),
                       int(((edge_faces == 2) & (traversed != 1)).sum())], dtype=np.int64)
    edges = np.stack([source[is_edge], target[is_edge]], axis=1).astype(np.int32).reshape(-1, 2)
    boundary = np.zeros(V, dtype=np.uint8)
    boundary[edges[edge_faces == 1].reshape(-1)] = 1
    return {"row_start": np.searchsorted(source, np.arange(V + 1), side="left").astype(np.int32), "neighbours": target.astype(np.int32),
            "edges": edges, "edge_faces": edge_faces.astype(np.int32), "edge_forward": traversed.astype(np.int32),
            "boundary_vertex": boundary, "counts": counts}


def topology_from_counts(counts) -> Dict[str, object]:
    """The counts of mesh_edges_reference / npcd.hip.mesh_edges as Python numbers: edges, valid_faces, used_vertices, boundary_edges,
    nonmanifold_edges, misoriented_edges, euler_characteristic = used vertices - edges + valid faces, and closed = no boundary edge
    and no non-manifold edge.  Reading a device array here is one host read."""
    c = [int(x) for x in (counts.cpu() if isinstance(counts, torch.Tensor) else np.asarray(counts)).reshape(-1).tolist()]
    if len(c) != len(COUNT_NAMES):
        raise ValueError(f"topology_from_counts: {len(COUNT_NAMES)} counts {COUNT_NAMES}; got {len(c)}")
    distinct, valid_faces, used, boundary, nonmanifold, misoriented = c
    return {"edges": distinct // 2, "valid_faces": valid_faces, "used_vertices": used, "boundary_edges": boundary,
            "nonmanifold_edges": nonmanifold, "misoriented_edges": misoriented,
            "euler_characteristic": used - distinct // 2 + valid_faces, "closed": boundary == 0 and nonmanifold == 0}


def mesh_topology(num_vertices: int, faces, edges=None) -> Dict[str, object]:
    """What a mesh's connectivity is, as topology_from_counts gives it.  faces as a tensor: the counts of npcd.hip.mesh_edges (on the
    GPU; there is no CPU path for tensors); as a numpy array: those of mesh_edges_reference, the specification.  `edges`: a dict
    that either of them returned for this mesh, to use again."""
    if edges is None:
        if isinstance(faces, torch.Tensor):
            from ..hip.smooth import mesh_edges
            edges = mesh_edges(num_vertices, faces)
        else:
            edges = mesh_edges_reference(num_vertices, faces)
    return topology_from_counts(edges["counts"])


def smooth_reference(vertices, faces, iterations: int = 10, lam: float = 0.5, mu: float = -0.53, fixed=None, fix_boundary: bool = True):
    """One mesh (vertices [V, 3], faces [F, 3]) -> (vertices' [V, 3] float32, state [V, 3] int32, e): the specification of Taubin's
    lambda | mu smoothing on an integer lattice on the CPU, float64 and integers.  `state` is the lattice after the last
    step and e the exponent of its quantum 2^(e - 29) (None where the largest coordinate is 0): the stage before the fp32 rounding.

    A vertex with a coordinate that is not finite is lost: it never moves and is no one's neighbour.  A = the largest finite
    |coordinate| (an integer maximum on the bits), e = floor(log2 A), q = rint(float64(x) 2^(29 - e)), ties to even.  With the adjacency
    of mesh_edges_reference, d_i counts the neighbours of i that are not lost; i moves if it is not lost, d_i > 0, it is not in
    `fixed` [V] and, with fix_boundary, not a boundary vertex.  A step with factor f: S_i the integer sum of q over those neighbours,
    q_i' = clamp(q_i + rint(f (float64(S_i) / float64(d_i) - float64(q_i))), -(2^31 - 1), 2^31 - 1) per axis, every vertex reading the
    old state.  An iteration is a step with lam, then one with mu; mu = 0 leaves the second out.  A vertex that moves comes back as
    float32(float64(q) 2^(e - 29)), every other as its input bits -- as do all with iterations = 0 or A = 0."""
    v, f = _mesh_arrays(vertices, faces, "smooth_reference")
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if not 0 <= iterations <= 1000:
        raise ValueError(f"smooth_reference: iterations must lie in [0, 1000]; got {iterations}")
    if not (0.0 < lam <= 1.0 and -1.0 <= mu <= 0.0):
        raise ValueError(f"smooth_reference: lam must lie in (0, 1] and mu in [-1, 0]; got {lam} and {mu}")
    V = len(v)
    pinned = np.zeros(V, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool).reshape(-1)
    if len(pinned) != V:
        raise ValueError(f"smooth_reference: fixed must be [{V}]; got {len(pinned)}")
    adjacency = mesh_edges_reference(V, f)
    finite = np.isfinite(v)
    lost = ~finite.all(axis=1)
    bits = np.where(finite, np.abs(v), np.float32(0.0)).astype(np.float32).view(np.uint32)
    top = float(bits.max().view(np.float32)) if v.size else 0.0          # the integer maximum of the bits: |x| >= +0
    state = np.zeros((V, 3), dtype=np.int64)
    if top == 0.0:
        return v.copy(), state.astype(np.int32), None
    e = math.frexp(top)[1] - 1
    state[~lost] = np.rint(np.ldexp(v[~lost].astype(np.float64), 29 - e)).astype(np.int64)
    row, nb = adjacency["row_start"].astype(np.int64), adjacency["neighbours"].astype(np.int64)
    counted = ~lost[nb]

    def row_sums(values):          # [D, ...] -> [V, ...]: the sums over each vertex's row, in integers
        total = np.concatenate([np.zeros((1,) + values.shape[1:], dtype=np.int64), np.cumsum(values, axis=0, dtype=np.int64)])
        return total[row[1:]] - total[row[:-1]]
    degree = row_sums(counted.astype(np.int64))
    moves = ~lost & (degree > 0) & ~pinned
    if fix_boundary:
        moves &= adjacency["boundary_vertex"] == 0
    for _ in range(iterations):
        for factor in (lam, mu) if mu != 0.0 else (lam,):
            S = row_sums(np.where(counted[:, None], state[nb], 0))[moves]
            q = state[moves]
            step = np.rint(factor * (S.astype(np.float64) / degree[moves].astype(np.float64)[:, None] - q.astype(np.float64))).astype(np.int64)
            state[moves] = np.clip(q + step, -(2 ** 31 - 1), 2 ** 31 - 1)
    out = v.copy()
    if iterations:
        out[moves] = np.ldexp(state[moves].astype(np.float64), e - 29).astype(np.float32)
    return out, state.astype(np.int32), e


MAX_DISTANCE_FACES = 2 ** 28          # what npcd.hip.mesh_distance takes (kMdMaxFaces of csrc/mesh_distance.h)


def closest_on_triangles(p, a, b, c):
    """The region form of Ericson's closest point on a triangle, every operation rounded in the arrays' own dtype, in the order of
    DESIGN.md 5.18.  p, a, b, c broadcast to [..., 3] -> (dist2 [...], q [..., 3]).  With float32 arrays this is the specification of a
    pair; with float64 arrays the same algorithm is what the tests measure its error against."""
    dt = np.result_type(p, a, b, c)
    zero, one = dt.type(0), dt.type(1)

    def dot(u, v):
        return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        d43, d56 = d4 - d3, d5 - d6
        holds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d43 >= 0) & (d56 >= 0)]
        region = np.full(d1.shape, 6, dtype=np.int8)          # the first region that holds
        for k in range(5, -1, -1):
            region = np.where(holds[k], np.int8(k), region)
        t = d43 / (d43 + d56)
        den = one / ((va + vb) + vc)
        v = np.select([region == 1, region == 2, region == 5, region == 6], [one, d1 / (d1 - d3), one - t, vb * den], zero).astype(dt)
        w = np.select([region == 3, region == 4, region == 5, region == 6], [one, d2 / (d2 - d6), t, vc * den], zero).astype(dt)
        q = a + (v[..., None] * ab + w[..., None] * ac)
        e = p - q
        return dot(e, e), q


def point_mesh_distance_reference(points, vertices, faces, chunk: int = 256) -> Dict[str, np.ndarray]:
    """The specification of npcd.hip.mesh_distance.closest_on_mesh in numpy: brute force, fp32 as written, `chunk`
    faces at a time.  points [S, 3], vertices [V, 3], faces [F, 3] -> {"sqdist" [S] float32, "face" [S] int32, "closest" [S, 3]
    float32}.

    A face takes part if its three indices lie in [0, V).  In ascending face order a face replaces the best if its dist2 is below it,
    from best = +inf and face = -1: a NaN never wins and among equal bits the lowest face index stays.  closest is that face's q; a
    point that no face wins keeps (+inf, -1, (+0, +0, +0))."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32))
    f = np.asarray(faces)
    if p.ndim != 2 or p.shape[1] != 3 or v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"point_mesh_distance_reference: points, vertices and faces must be [N, 3]; got {p.shape}, {v.shape} and {f.shape}")
    if f.size and not np.issubdtype(f.dtype, np.integer):
        raise ValueError("point_mesh_distance_reference: faces must hold integers")
    f = f.astype(np.int64)
    S, V, F = len(p), len(v), len(f)
    if F >= MAX_DISTANCE_FACES:
        raise ValueError(f"point_mesh_distance_reference: {F} faces; they must stay below 2^28 = {MAX_DISTANCE_FACES}")
    best = np.full(S, np.inf, dtype=np.float32)
    face = np.full(S, -1, dtype=np.int32)
    closest = np.zeros((S, 3), dtype=np.float32)
    rows = np.arange(S)
    for first in range(0, F if S else 0, chunk):
        part = f[first:first + chunk]
        valid = ((part >= 0) & (part < V)).all(axis=1)
        if not valid.any():
            continue
        index = first + np.nonzero(valid)[0]
        corner = v[part[valid]]          # [n, 3 corners, 3]
        d, q = closest_on_triangles(p[:, None, :], corner[None, :, 0], corner[None, :, 1], corner[None, :, 2])
        d = np.where(np.isnan(d), np.float32(np.inf), d)
        at = np.argmin(d, axis=1)          # the first of equal minima: the lowest index
        least = d[rows, at]
        wins = least < best
        best[wins], face[wins], closest[wins] = least[wins], index[at[wins]].astype(np.int32), q[rows, at][wins]
    return {"sqdist": best, "face": face, "closest": closest}


def ray_axes(directions: np.ndarray):
    """directions [R, 3] float32 -> (kx, ky, kz [R] int64, usable [R] bool): step 1 of DESIGN.md 5.19.  kz is the axis of the largest
    |d|, the lowest among equal ones; kx = (kz + 1) % 3 and ky = (kx + 1) % 3, swapped where d[kz] < 0; usable: d finite and
    d[kz] != 0."""
    d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
    size = np.abs(d)
    kz = np.zeros(len(d), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        top = size[:, 0].copy()
        for k in (1, 2):
            larger = size[:, k] > top
            kz[larger], top[larger] = k, size[larger, k]
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        dz = d[np.arange(len(d)), kz]
        turned = dz < 0
        kx, ky = np.where(turned, ky, kx), np.where(turned, kx, ky)
        usable = np.isfinite(d).all(axis=1) & (dz != 0)
    return kx, ky, kz, usable


def _ray_face_chunks(who: str, origins, directions, vertices, faces, chunk: int):
    """Steps 1 to 3 of DESIGN.md 5.19, which ray_mesh_reference and crossings_reference share: checks the arrays and yields, per
    `chunk` faces that hold a face that takes part, (index [n] of those faces, x, y, z [R, n, 3 corners] float64: the fp32 sheared
    corners; U, V, W, det [R, n] float64; usable [R] bool: origin and direction finite, d[kz] != 0).  Run under np.errstate."""
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.float32))
    d = np.ascontiguousarray(np.asarray(directions, dtype=np.float32))
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float32))
    f = np.asarray(faces)
    if any(a.ndim != 2 or a.shape[1] != 3 for a in (o, d, v, f)) or len(o) != len(d):
        raise ValueError(f"{who}: origins and directions must be [R, 3], vertices and faces [N, 3]; got {o.shape}, {d.shape}, "
                         f"{v.shape} and {f.shape}")
    if f.size and not np.issubdtype(f.dtype, np.integer):
        raise ValueError(f"{who}: faces must hold integers")
    f = f.astype(np.int64)
    R, V, F = len(o), len(v), len(f)
    if F >= MAX_DISTANCE_FACES:
        raise ValueError(f"{who}: {F} faces; they must stay below 2^28 = {MAX_DISTANCE_FACES}")
    rows = np.arange(R)
    kx, ky, kz, usable = ray_axes(d)
    usable &= np.isfinite(o).all(axis=1)
    with np.errstate(all="ignore"):
        dz = d[rows, kz]
        Sx, Sy, Sz = d[rows, kx] / dz, d[rows, ky] / dz, np.float32(1.0) / dz

        def pick(p, k):          # p [R, n, 3 corners, 3] -> [R, n, 3 corners]: the component k [R] of every corner
            return np.take_along_axis(p, k[:, None, None, None], axis=3)[..., 0]
        for first in range(0, F if R else 0, chunk):
            part = f[first:first + chunk]
            valid = ((part >= 0) & (part < V)).all(axis=1)
            if not valid.any():
                continue
            p = v[part[valid]][None] - o[:, None, None, :]          # [R, n, 3 corners, 3] float32
            pz = pick(p, kz)
            x = (pick(p, kx) - Sx[:, None, None] * pz).astype(np.float64)
            y = (pick(p, ky) - Sy[:, None, None] * pz).astype(np.float64)
            z = (Sz[:, None, None] * pz).astype(np.float64)
            assert p.dtype == np.float32 and pz.dtype == np.float32
            U = x[..., 2] * y[..., 1] - y[..., 2] * x[..., 1]
            Vf = x[..., 0] * y[..., 2] - y[..., 0] * x[..., 2]
            W = x[..., 1] * y[..., 0] - y[..., 1] * x[..., 0]
            yield first + np.nonzero(valid)[0], x, y, z, U, Vf, W, (U + Vf) + W, usable


def ray_mesh_reference(origins, directions, vertices, faces, t_min: float = 0.0, t_max: float = float("inf"), chunk: int = 256) -> Dict[str, np.ndarray]:
    """The specification of npcd.hip.raycast.cast_rays in numpy: brute force, `chunk` faces at a time.  origins,
    directions [R, 3], vertices [V, 3], faces [F, 3] -> {"t" [R] float32, "face" [R] int32, "bary" [R, 3] float32, "front" [R] int8}.

    A face takes part if its three indices lie in [0, V).  With the axes of ray_axes, Sx = d[kx] / d[kz], Sy = d[ky] / d[kz] and Sz =
    1 / d[kz] in fp32; per corner p = P - o, px = p[kx] - Sx p[kz], py = p[ky] - Sy p[kz], pz = Sz p[kz] in fp32.  In float64 from those:
    U = cx by - cy bx, V = ax cy - ay cx, W = bx ay - by ax, det = (U + V) + W; a pair misses if one of U, V, W is below 0 and another
    above, if det == 0 or anything is NaN; T = (U az + V bz) + W cz, t = float32(T / det), a hit iff t_min <= t <= t_max and t < +inf.
    The winner is the lexicographic minimum of (t, face), t as a signed float (-0 == +0); bary = float32(U / det, V / det, W / det),
    front = det > 0.  A ray that is not usable (a component of o or d not finite, d[kz] == 0) or hits nothing keeps (+inf, -1, zeros,
    0)."""
    t_min, t_max = np.float32(t_min), np.float32(t_max)
    R = len(np.asarray(origins))
    out = {"t": np.full(R, np.inf, dtype=np.float32), "face": np.full(R, -1, dtype=np.int32), "bary": np.zeros((R, 3), dtype=np.float32),
           "front": np.zeros(R, dtype=np.int8)}
    rows = np.arange(R)
    with np.errstate(all="ignore"):
        for index, x, y, z, U, Vf, W, det, usable in _ray_face_chunks("ray_mesh_reference", origins, directions, vertices, faces, chunk):
            below, above = (U < 0) | (Vf < 0) | (W < 0), (U > 0) | (Vf > 0) | (W > 0)
            inside = usable[:, None] & ~(below & above) & (det != 0) & ~(np.isnan(U) | np.isnan(Vf) | np.isnan(W) | np.isnan(det))
            T = (U * z[..., 0] + Vf * z[..., 1]) + W * z[..., 2]
            t = (T / det).astype(np.float32)
            hit = inside & (t >= t_min) & (t <= t_max) & (t < np.float32(np.inf))
            key = np.where(hit, t, np.float32(np.inf))
            at = np.argmin(key, axis=1)          # the first of equal minima: the lowest index
            least = key[rows, at]
            wins = least < out["t"]
            w, a = rows[wins], at[wins]
            out["t"][w], out["face"][w] = least[wins], index[a].astype(np.int32)
            out["bary"][w] = np.stack([U[w, a] / det[w, a], Vf[w, a] / det[w, a], W[w, a] / det[w, a]], axis=1).astype(np.float32)
            out["front"][w] = (det[w, a] > 0).astype(np.int8)
    return out


def crossings_reference(origins, directions, vertices, faces, t_min: float = 0.0, t_max: float = float("inf"), chunk: int = 256,
                        inclusive: bool = False) -> Dict[str, np.ndarray]:
    """The specification of npcd.hip.crossings.count_crossings in numpy: brute force, `chunk` faces at a time.
    origins, directions [R, 3], vertices [V, 3], faces [F, 3] -> {"front" [R], "back" [R] int32}: how many faces the ray crosses
    with t in [t_min, t_max], those whose normal (B - A) x (C - A) points against the ray and those whose normal points along it.

    The sheared corners, U, V, W, det, T and t = float32(T / det) are those of ray_mesh_reference.  With s = sign(det), a pair
    crosses iff the ray is usable, nothing is NaN, det != 0 and each of the directed edges U: c -> b, V: a -> c, W: b -> a owns the
    origin: s E > 0, or E == 0 and, with (dx, dy) = s (end - start) in the fp32 sheared coordinates, their signs decided by comparing
    the coordinates, dy > 0 or (dy == 0 and dx < 0): the rasteriser's top-left rule.  An edge that two faces share from opposite
    sides is owned by one of them, a fan around a vertex covers the origin once, a face of no projected area never counts.  A
    crossing counts iff t_min <= t <= t_max and t < +inf; it is a front crossing if det > 0 and a back crossing if det < 0.  A ray
    that is not usable gets (0, 0).  inclusive=True counts the hits of ray_mesh_reference's pair rule instead, which counts a ray
    through a shared edge or a vertex once per face around it: what the rule above is there to avoid.

    Unspecified: which side a point within rounding of the surface falls on (the fp32 shear moves a corner by a few ulp), and what
    parity means for a mesh that is not closed."""
    t_min, t_max = np.float32(t_min), np.float32(t_max)
    R = len(np.asarray(origins))
    out = {"front": np.zeros(R, dtype=np.int32), "back": np.zeros(R, dtype=np.int32)}
    with np.errstate(all="ignore"):
        for _, x, y, z, U, Vf, W, det, usable in _ray_face_chunks("crossings_reference", origins, directions, vertices, faces, chunk):
            numbers = ~(np.isnan(U) | np.isnan(Vf) | np.isnan(W) | np.isnan(det))
            if inclusive:
                below, above = (U < 0) | (Vf < 0) | (W < 0), (U > 0) | (Vf > 0) | (W > 0)
                inside = ~(below & above)
            else:
                pos = det > 0

                def owns(E, start, end):
                    up = np.where(pos, y[..., end] > y[..., start], y[..., end] < y[..., start])
                    left = np.where(pos, x[..., end] < x[..., start], x[..., end] > x[..., start])
                    return np.where(pos, E > 0, E < 0) | ((E == 0) & (up | ((y[..., end] == y[..., start]) & left)))
                inside = owns(U, 2, 1) & owns(Vf, 0, 2) & owns(W, 1, 0)
            T = (U * z[..., 0] + Vf * z[..., 1]) + W * z[..., 2]
            t = (T / det).astype(np.float32)
            counted = usable[:, None] & numbers & (det != 0) & inside & (t >= t_min) & (t <= t_max) & (t < np.float32(np.inf))
            out["front"] += (counted & (det > 0)).sum(axis=1, dtype=np.int32)
            out["back"] += (counted & (det < 0)).sum(axis=1, dtype=np.int32)
    return out


def _mesh_parts(mesh):
    """(vertices, faces, normals or None) of a mesh as isosurface (a tuple) or extract_mesh (a dict) returns it."""
    if isinstance(mesh, dict):
        return mesh["vertices"], mesh["faces"], mesh.get("normals")
    return mesh[0], mesh[1], (mesh[2] if len(mesh) > 2 else None)


def _distance_stats(sqdist: torch.Tensor, usable: torch.Tensor) -> torch.Tensor:
    """sqdist [S] and usable [S] bool -> [mean, rms, max] of sqrt(float64(sqdist)) over the usable samples as a float64 tensor on
    their device; NaN without any."""
    d = torch.sqrt(sqdist.to(torch.float64))
    if d.numel() == 0:
        return torch.full((3,), float("nan"), dtype=torch.float64, device=sqdist.device)
    n = usable.sum().to(torch.float64)
    kept = torch.where(usable, d, torch.zeros_like(d))
    top = torch.where(usable, d, torch.full_like(d, -float("inf"))).max()
    return torch.stack([kept.sum() / n, torch.sqrt((kept * kept).sum() / n), torch.where(n > 0, top, torch.full_like(top, float("nan")))])


def _closest_operator(closest):
    if closest is None:
        from ..hip.mesh_distance import closest_on_mesh as closest
    return closest


_STAT_NAMES = ("mean", "rms", "max")


@torch.no_grad()
def mesh_deviation(a, b, num_samples: int = 100_000, generator: Optional[torch.Generator] = None, sampler=None, closest=None) -> Dict[str, object]:
    """How far two surfaces lie apart.  a, b: meshes on the GPU as isosurface (a tuple) or extract_mesh (a dict) return them.

    num_samples points are drawn by area on each (npcd.hip.surface.sample_surface) and each takes its distance to the
    other mesh (npcd.hip.mesh_distance.closest_on_mesh).  -> {"a_to_b", "b_to_a": {"mean", "rms", "max"} of
    sqrt(float64(sqdist)) over the samples that have a face on both sides, "hausdorff": the larger max, "mean": the mean of the two
    means, "diagonal": the bounding-box diagonal of a's finite vertices, "samples": num_samples}, Python floats.  A direction without
    a usable sample gives NaN.  The reductions are float64 on the device; one host read.  `sampler` and `closest` stand in for
    sample_surface and closest_on_mesh (tests of the host logic)."""
    n = int(num_samples)
    if n < 1:
        raise ValueError(f"mesh_deviation: num_samples must be at least 1; got {num_samples}")
    if sampler is None:
        from ..hip.surface import sample_surface as sampler
    closest = _closest_operator(closest)
    (va, fa, _), (vb, fb, _) = _mesh_parts(a), _mesh_parts(b)
    stats = []
    for (v_from, f_from), (v_to, f_to) in (((va, fa), (vb, fb)), ((vb, fb), (va, fa))):
        points, _, own = sampler((v_from, f_from), n, generator=generator, return_faces=True)
        got = closest(points, v_to, f_to)
        stats.append(_distance_stats(got["sqdist"], (own >= 0) & (got["face"] >= 0)))
    finite = torch.isfinite(va).all(dim=1)
    if va.shape[0]:
        v64 = va.to(torch.float64)
        lo = torch.where(finite[:, None], v64, torch.full_like(v64, float("inf"))).amin(dim=0)
        hi = torch.where(finite[:, None], v64, torch.full_like(v64, -float("inf"))).amax(dim=0)
        diagonal = torch.where(finite.any(), torch.sqrt(((hi - lo) ** 2).sum()), torch.full((), float("nan"), dtype=torch.float64, device=va.device))
    else:
        diagonal = torch.full((), float("nan"), dtype=torch.float64, device=va.device)
    flat = torch.cat([stats[0], stats[1], diagonal.reshape(1)]).cpu().tolist()          # the one host read
    a_to_b, b_to_a = dict(zip(_STAT_NAMES, flat[0:3])), dict(zip(_STAT_NAMES, flat[3:6]))
    both = (a_to_b["max"], b_to_a["max"])
    return {"a_to_b": a_to_b, "b_to_a": b_to_a, "hausdorff": float("nan") if any(math.isnan(x) for x in both) else max(both),
            "mean": 0.5 * (a_to_b["mean"] + b_to_a["mean"]), "diagonal": flat[6], "samples": n}


@torch.no_grad()
def cloud_mesh_distance(points: torch.Tensor, mesh, closest=None) -> Dict[str, float]:
    """How far the points [S, 3] of a generated cloud lie from an extracted surface: {"mean", "rms", "max"} of sqrt(float64(sqdist))
    over the points that a face wins (npcd.hip.mesh_distance.closest_on_mesh), Python floats; NaN without any.  One host read.
    `closest` stands in for closest_on_mesh."""
    closest = _closest_operator(closest)
    vertices, faces, _ = _mesh_parts(mesh)
    got = closest(points, vertices, faces)
    return dict(zip(_STAT_NAMES, _distance_stats(got["sqdist"], got["face"] >= 0).cpu().tolist()))


def _mix(bary: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """bary [..., 3] and rows [..., 3 corners, C] -> (b0 r0 + b1 r1) + b2 r2, in that order."""
    return (bary[..., 0:1] * rows[..., 0, :] + bary[..., 1:2] * rows[..., 1, :]) + bary[..., 2:3] * rows[..., 2, :]


def _unit(g: torch.Tensor) -> torch.Tensor:
    """g [..., 3] -> g / sqrt((gx gx + gy gy) + gz gz); (+0, +0, +0) where a component is not finite."""
    unit = g / torch.sqrt((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2])[..., None]
    return torch.where(torch.isfinite(unit).all(dim=-1, keepdim=True), unit, torch.zeros_like(unit))


def block_order(resolution: int, device, block: int = 8) -> torch.Tensor:
    """The row-major pixel numbers of a resolution^2 image in the order of its block x block pixel blocks, row-major within a block and
    among the blocks: 64 consecutive entries are neighbours in the image, which is what a wave of cast_rays wants.  int64 [R]."""
    row, col = torch.meshgrid(torch.arange(resolution, device=device), torch.arange(resolution, device=device), indexing="ij")
    across = (resolution + block - 1) // block
    key = ((row // block * across + col // block) * block + row % block) * block + col % block
    return torch.sort(key.reshape(-1))[1]


MESH_GREY = 0.75          # the albedo of a mesh without colours in render_mesh


@torch.no_grad()
def render_mesh(mesh, extrinsics: torch.Tensor, intrinsics: torch.Tensor, resolution: int, cube_scale: float, white_back: bool = True,
                light: str = "head", caster=None, raygen=None) -> Dict[str, torch.Tensor]:
    """A mesh on the GPU, as isosurface or extract_mesh return it, seen from the cameras extrinsics [T, 4, 4] (world to camera) and
    intrinsics [T, 3, 3] -> {"mask" [T, R, 1], "depth" [T, R, 1], "face" [T, R] int32, "normal" [T, R, 3], "channels" [T, R, 3]}, R =
    resolution^2 in row-major pixel order.

    The rays are those of npcd.hip.render.ray_gen(extrinsics, intrinsics, resolution, cube_scale), the very rays the volume renderer
    marches, and each takes its first hit on the mesh (npcd.hip.raycast.cast_rays) with t >= 0; they are cast in 8 x 8 pixel blocks
    and scattered back, a permutation that changes no bit.  mask is 1 on a hit; depth is the ray parameter t along ray_gen's
    direction -- the volume renderer's convention, the point is o + t d; ray_gen's d is unit, so t is also a distance -- and a ray that misses gets its own end
    t1, what the volume renderer gives a sample slot without a point.  normal is the unit normal of the face, (B - A) x (C - A)
    normalised, or with mesh["normals"] the barycentric mix of the vertex normals, normalised again; zeros on a miss.  channels is
    the barycentric mix of mesh["colors"], or without colours MESH_GREY |normal . d / |d||: a light at the camera, both sides lit;
    a miss gets the background, 1 with white_back and 0 without.  Torch on the device in a fixed order of operations: two calls give
    the same bits.  No host read.  `caster` and `raygen` stand in for cast_rays and ray_gen (tests of the host logic)."""
    if light != "head":
        raise ValueError(f"render_mesh: light must be \"head\" (a light at the camera); got {light!r}")
    if caster is None:
        from ..hip.raycast import cast_rays as caster
    if raygen is None:
        from ..hip.render import ray_gen as raygen
    vertices, faces, normals = _mesh_parts(mesh)
    colors = mesh.get("colors") if isinstance(mesh, dict) else None
    resolution = int(resolution)
    o, d, _, t1 = raygen(extrinsics, intrinsics, resolution, float(cube_scale))
    T, R = o.shape[0], o.shape[1]
    order = block_order(resolution, o.device)
    got = caster(o[:, order].reshape(-1, 3), d[:, order].reshape(-1, 3), vertices, faces)
    back = {k: torch.empty_like(got[k].reshape((T, R) + got[k].shape[1:])) for k in ("t", "face", "bary")}
    for k in back:
        back[k][:, order] = got[k].reshape(back[k].shape)
    face, bary = back["face"], back["bary"]
    hit = face >= 0
    depth = torch.where(hit, back["t"], t1)
    background = torch.full((T, R, 3), 1.0 if white_back else 0.0, dtype=torch.float32, device=o.device)
    if faces.shape[0] == 0:
        return {"mask": hit.to(torch.float32)[..., None], "depth": depth[..., None], "face": face, "normal": torch.zeros_like(background),
                "channels": background}
    corners = faces[face.clamp(min=0).long()].long()          # [T, R, 3]: a winner's indices lie in [0, V)
    if normals is None:
        c = vertices[corners]
        e1, e2 = c[..., 1, :] - c[..., 0, :], c[..., 2, :] - c[..., 0, :]
        n = torch.stack([e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                         e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]], dim=-1)
    else:
        n = _mix(bary, normals[corners])
    normal = torch.where(hit[..., None], _unit(n), torch.zeros_like(n))
    if colors is None:
        toward = _unit(d)
        lit = torch.abs((normal[..., 0] * toward[..., 0] + normal[..., 1] * toward[..., 1]) + normal[..., 2] * toward[..., 2])
        shade = (MESH_GREY * lit)[..., None].expand(-1, -1, 3)
    else:
        shade = _mix(bary, colors[corners])
    return {"mask": hit.to(torch.float32)[..., None], "depth": depth[..., None], "face": face, "normal": normal,
            "channels": torch.where(hit[..., None], shade, background)}


_AGREEMENT_NAMES = ("iou", "depth_mean", "depth_max", "psnr", "ssim")


@torch.no_grad()
def mesh_render_agreement(pointnerf, coords, feats, mesh, extrinsics: torch.Tensor, intrinsics: torch.Tensor, resolution: int = 128,
                          caster=None, raygen=None, renderer=None, metrics=None) -> Dict[str, object]:
    """Does a mesh look like the field it came from?  The field of one cloud (coords [N, 3] or [1, N, 3], feats likewise) through
    PointNeRF.render and the mesh through render_mesh, at the same cameras extrinsics [T, 4, 4] and intrinsics [T, 3, 3], the same
    rays, the renderer's cube_scale and background.

    -> {"views": per view {"iou", "depth_mean", "depth_max", "psnr", "ssim"}, and the same five over the views}, Python floats.  iou:
    the silhouettes, the field's mask above 0.5 against the mesh's, intersection over union (1 where both are empty).  depth_mean,
    depth_max: |depth difference| over the pixels inside both silhouettes, the ray parameter of either; NaN without such a pixel.
    psnr = 10 log10(1 / mse) and ssim of the two colour images through npcd.hip.image_metrics.  Over the views: the mean of the
    views that have a value, the maximum for depth_max.  float64 on the device; one host read, at the end.  `caster`, `raygen`,
    `renderer` (for pointnerf.render) and `metrics` (for image_metrics) stand in (tests of the host logic)."""
    if metrics is None:
        from ..hip.image_metrics import image_metrics as metrics
    resolution = int(resolution)
    batch = lambda x: x if x is None or x.dim() == 3 else x[None]
    seen = (pointnerf.render if renderer is None else renderer)(batch(coords), batch(feats), extrinsics[None], intrinsics[None], resolution=resolution)
    settings = pointnerf.renderer
    view = render_mesh(mesh, extrinsics, intrinsics, resolution, float(settings.cube_scale), white_back=bool(settings.white_back),
                       caster=caster, raygen=raygen)
    T = extrinsics.shape[0]
    f64 = torch.float64
    of_field, of_mesh = seen["mask"][0, :, :, 0] > 0.5, view["mask"][:, :, 0] > 0.5
    both, either = (of_field & of_mesh), (of_field | of_mesh)
    n_both, n_either = both.sum(dim=1).to(f64), either.sum(dim=1).to(f64)
    iou = torch.where(n_either > 0, n_both / n_either, torch.ones_like(n_either))
    gap = torch.abs(seen["depth"][0, :, :, 0].to(f64) - view["depth"][:, :, 0].to(f64))
    gap_mean = torch.where(both, gap, torch.zeros_like(gap)).sum(dim=1) / n_both          # 0 / 0: NaN without a common pixel
    gap_max = torch.where(both, gap, torch.full_like(gap, -float("inf"))).amax(dim=1)
    gap_max = torch.where(n_both > 0, gap_max, torch.full_like(gap_max, float("nan")))
    image = lambda c: c.reshape(T, resolution, resolution, 3).to(torch.float32).contiguous()
    measured = metrics(image(view["channels"]), image(seen["channels"][0]), layout="hwc")
    psnr = 10.0 * torch.log10(1.0 / measured.mse.to(f64))
    rows = torch.stack([iou, gap_mean, gap_max, psnr, measured.ssim.to(f64)], dim=1).cpu().tolist()          # the one host read
    views = [dict(zip(_AGREEMENT_NAMES, row)) for row in rows]
    out: Dict[str, object] = {"views": views}
    for name in _AGREEMENT_NAMES:
        values = [v[name] for v in views if not math.isnan(v[name])]
        out[name] = float("nan") if not values else (max(values) if name == "depth_max" else sum(values) / len(values))
    return out


# the lattice nodes that one wave of voxelize_mesh holds, (z, y, x), for rays along +x: PATCH_ACROSS, an 8 x 8 patch across the rays,
# or PATCH_BLOCK, a 4 x 4 x 4 block.  Which is faster, and whether an oblique direction beats +x, tools/probes/gpu_dev_crossings.py
# measures; the defaults below are first guesses until it has run (docs/experiments.md R39.1)
PATCH_ACROSS, PATCH_BLOCK = (8, 8, 1), (4, 4, 4)
VOXEL_PATCH = PATCH_ACROSS
VOXEL_DIRECTION = (1.0, 0.0, 0.0)


def patch_order(nodes: Sequence[int], patch: Sequence[int], device) -> torch.Tensor:
    """The row-major node numbers of a (Gz, Gy, Gx) lattice in the order of its patches of `patch` = (pz, py, px) nodes, row-major
    within a patch and among the patches: with 64 nodes to a patch, the 64 rays of a wave of count_crossings start at neighbours.
    int64 [Gz Gy Gx]; a patch that reaches past the lattice is shorter, so waves then straddle patches."""
    (gz, gy, gx), (pz, py, px) = (int(g) for g in nodes), (int(p) for p in patch)
    z, y, x = torch.meshgrid(torch.arange(gz, device=device), torch.arange(gy, device=device), torch.arange(gx, device=device), indexing="ij")
    ay, ax = (gy + py - 1) // py, (gx + px - 1) // px
    key = ((((z // pz * ay + y // py) * ax + x // px) * pz + z % pz) * py + y % py) * px + x % px
    return torch.sort(key.reshape(-1))[1]


def _on_device(triple, device) -> torch.Tensor:
    """Three numbers, host values or a tensor, as fp32 [3] on the device without a copy from the host, which would wait for the stream."""
    if isinstance(triple, torch.Tensor) and triple.device == device:
        return triple.to(torch.float32).reshape(3)
    values = triple.tolist() if isinstance(triple, torch.Tensor) else list(triple)
    if len(values) != 3:
        raise ValueError(f"voxelize_mesh: origin and spacing must hold three numbers; got {triple!r}")
    return torch.stack([torch.full((), float(x), dtype=torch.float32, device=device) for x in values])


@torch.no_grad()
def voxelize_mesh(mesh, origin, spacing, nodes: Sequence[int], direction: Sequence[float] = VOXEL_DIRECTION,
                  patch: Sequence[int] = VOXEL_PATCH, container=None) -> torch.Tensor:
    """Which nodes of a lattice lie inside a closed mesh on the GPU, as isosurface or extract_mesh return it -> bool [Gz, Gy, Gx],
    nodes = (Gz, Gy, Gx).  Node (x, y, z) lies at origin + spacing * (x, y, z) in fp32, as for npcd.hip.isosurface; origin and spacing
    are (x, y, z) host values or tensors.  Inside by the parity of the crossings of the ray from the node along `direction`
    (npcd.hip.crossings.mesh_contains); the nodes are cast in patches of `patch` = (pz, py, px) nodes (patch_order)
    and scattered back, a permutation that changes no bit.  No host read.  `container` stands in for mesh_contains (tests of the
    host logic).

    Unspecified: a node within rounding of the surface, and a mesh that is not closed (parity then means nothing)."""
    if container is None:
        from ..hip.crossings import mesh_contains as container
    vertices, faces, _ = _mesh_parts(mesh)
    gz, gy, gx = (int(g) for g in nodes)
    if min(gz, gy, gx) < 1:
        raise ValueError(f"voxelize_mesh: every axis needs at least 1 node; got {(gz, gy, gx)}")
    dev = vertices.device
    o, s = (_on_device(a, dev) for a in (origin, spacing))
    order = patch_order((gz, gy, gx), patch, dev)
    row = order // gx
    at = torch.stack([order - row * gx, row % gy, row // gy], dim=1).to(torch.float32)
    inside = container((o + s * at).contiguous(), vertices, faces, direction=direction)
    out = torch.empty(gz * gy * gx, dtype=torch.bool, device=dev)
    out[order] = inside
    return out.view(gz, gy, gx)


@torch.no_grad()
def mesh_signed_distance(points: torch.Tensor, mesh, closest=None, container=None) -> torch.Tensor:
    """points [S, 3] fp32 on the GPU -> [S] fp32: sqrt of the squared distance to the closest face of a closed mesh
    (npcd.hip.mesh_distance.closest_on_mesh), negative where the point lies inside (npcd.hip.crossings.mesh_contains,
    DESIGN.md 5.20); +inf for a mesh without a face that takes part.  No host read.  `closest` and `container` stand in.

    Unspecified: the sign of a point within rounding of the surface, where |d| is within rounding of 0, and every sign for a mesh
    that is not closed."""
    closest = _closest_operator(closest)
    if container is None:
        from ..hip.crossings import mesh_contains as container
    vertices, faces, _ = _mesh_parts(mesh)
    d = torch.sqrt(closest(points, vertices, faces)["sqdist"])
    return torch.where(container(points, vertices, faces), -d, d)


def _node_set_iou(a: torch.Tensor, b: torch.Tensor) -> List[torch.Tensor]:
    """Two bool lattices -> [|a|, |b|, |a and b|, |a or b|] as float64 words on their device."""
    return [x.sum().to(torch.float64) for x in (a, b, a & b, a | b)]


@torch.no_grad()
def mesh_volume_iou(a, b, resolution: int = 64, bound: Optional[float] = None, voxelizer=None) -> Dict[str, float]:
    """The volumetric intersection over union of two closed meshes on the GPU -> {"iou", "volume_a", "volume_b", "intersection",
    "union"}, Python floats.

    Both are voxelised (voxelize_mesh) on one lattice of resolution^3 cells over the union of the boxes of their finite vertices, or
    with `bound` over [-bound, bound]^3; a node sits at the centre of its cell, and a volume is a node count times the cell volume.
    iou is the ratio of the two node counts, 1 where both are empty.  float64 on the device; one host read.  `voxelizer` stands in
    for voxelize_mesh (tests of the host logic).  Unspecified for a mesh that is not closed."""
    G = int(resolution)
    if G < 1:
        raise ValueError(f"mesh_volume_iou: resolution must be at least 1; got {resolution}")
    voxelizer = voxelize_mesh if voxelizer is None else voxelizer
    va, vb = _mesh_parts(a)[0], _mesh_parts(b)[0]
    if bound is None:
        v = torch.cat([va, vb]).to(torch.float64)
        finite = torch.isfinite(v).all(dim=1, keepdim=True)
        lo = torch.where(finite, v, torch.full_like(v, float("inf"))).amin(dim=0) if v.shape[0] else torch.zeros(3, dtype=torch.float64, device=v.device)
        hi = torch.where(finite, v, torch.full_like(v, -float("inf"))).amax(dim=0) if v.shape[0] else torch.zeros(3, dtype=torch.float64, device=v.device)
        lo, hi = torch.where(hi >= lo, lo, torch.zeros_like(lo)), torch.where(hi >= lo, hi, torch.zeros_like(hi))          # no finite vertex
    else:
        if not float(bound) > 0:
            raise ValueError(f"mesh_volume_iou: bound must be positive; got {bound}")
        lo, hi = (torch.full((3,), x, dtype=torch.float64, device=va.device) for x in (-float(bound), float(bound)))
    cell = (hi - lo) / G
    origin, spacing = (lo + 0.5 * cell).to(torch.float32), cell.to(torch.float32)
    inside = [voxelizer(m, origin, spacing, (G, G, G)) for m in (a, b)]
    flat = torch.stack(_node_set_iou(*inside) + [spacing.to(torch.float64).prod()]).cpu().tolist()          # the one host read
    n_a, n_b, n_both, n_either, volume = flat
    return {"iou": n_both / n_either if n_either else 1.0, "volume_a": n_a * volume, "volume_b": n_b * volume,
            "intersection": n_both * volume, "union": n_either * volume}


@torch.no_grad()
def mesh_enclosure(mesh, origin, spacing, solid: torch.Tensor, voxelizer=None) -> Dict[str, object]:
    """Does a mesh enclose what its field calls solid?  solid: bool [Gz, Gy, Gx] on the GPU, the nodes of the lattice (origin, spacing)
    where the density lies above the level -> {"agree": the share of nodes where voxelize_mesh equals solid, "inside_nodes",
    "solid_nodes": the two counts, "iou": of the two node sets, 1 where both are empty}.  One host read.  An interpolated vertex
    can round onto a node, and such a node may fall on either side: agree may lie a few nodes below 1 for a correct mesh."""
    inside = (voxelize_mesh if voxelizer is None else voxelizer)(mesh, origin, spacing, tuple(solid.shape))
    n_in, n_solid, n_both, n_either, same = torch.stack(_node_set_iou(inside, solid) + [(inside == solid).sum().to(torch.float64)]).cpu().tolist()
    return {"agree": same / solid.numel(), "inside_nodes": int(n_in), "solid_nodes": int(n_solid), "iou": n_both / n_either if n_either else 1.0}


@torch.no_grad()
def sample_mesh_clouds(meshes, num_points: int, generator: Optional[torch.Generator] = None, normals: bool = False, sampler=None):
    """Meshes on the GPU, as isosurface or extract_mesh return them -> clouds [B, num_points, 3] fp32 drawn uniformly by area from
    their surfaces (npcd.hip.surface.sample_surface): what shape_metrics takes.  normals=True -> (clouds, normals
    [B, num_points, 3]), the meshes' vertex normals (extract_mesh(..., normals=True)) interpolated at the points.  A mesh without
    surface gives a cloud of zeros.  `sampler` stands in for sample_surface (tests of the host logic)."""
    if sampler is None:
        from ..hip.surface import sample_surface as sampler
    if isinstance(meshes, dict) or (len(meshes) and isinstance(meshes[0], torch.Tensor)):
        meshes = [meshes]
    parts = [_mesh_parts(m) for m in meshes]
    vertex_normals = None
    if normals:
        if any(p[2] is None for p in parts):
            raise ValueError("sample_mesh_clouds: normals=True needs meshes with vertex normals (extract_mesh(..., normals=True))")
        vertex_normals = [p[2] for p in parts]
    got = sampler([(p[0], p[1]) for p in parts], int(num_points), generator=generator, normals=vertex_normals)
    return (got[0], got[2]) if normals else got[0]


DEVIATION_SEED = 20260518          # of the samples of extract_mesh(deviation=n)


def default_level(pointnerf) -> float:
    """ln 2 / (2 cube_scale / (depth_resolution - 1)): the density at which one depth step of an axis-parallel ray through the box
    is half opaque."""
    r = pointnerf.renderer
    return math.log(2.0) / (2.0 * float(r.cube_scale) / (int(r.depth_resolution) - 1))


@torch.no_grad()
def extract_mesh(pointnerf, coords: torch.Tensor, feats: torch.Tensor, resolution=128, level: Optional[float] = None, colors: bool = True,
                 bound: Optional[float] = None, mlp_dtype=None, view_dir: Optional[torch.Tensor] = None, components: Optional[int] = None,
                 min_component_nodes: Optional[int] = None, normals: bool = False, simplify: Optional[float] = None,
                 simplifier=None, smooth: Optional[int] = None, smooth_lambda: float = 0.5, smooth_mu: float = -0.53,
                 topology: bool = False, smoother=None, deviation: Optional[int] = None, deviator=None, agreement=None,
                 agreer=None, enclosure: bool = False, encloser=None) -> List[Dict[str, torch.Tensor]]:
    """coords [B, N, 3], feats [B, N, F] on the GPU -> per cloud {"vertices" [V, 3] fp32, "faces" [F, 3] int32, "colors" [V, 3] fp32
    in [0, 1] (with colors=True)}, all on the GPU.

    The density on PointNeRF.density_grid(resolution, bound), its isosurface at `level` (npcd.hip.isosurface), and the field's
    colour at the vertices (PointNeRF.query_field; `view_dir` [3] for a field with view directions, `mlp_dtype` as for render).
    level=None takes default_level(pointnerf).  Nobody has looked at this default on trained weights: it is a statement about one
    depth step of the renderer, not about where a trained car's surface lies -- choose the level by eye.

    components=k keeps the k largest connected components of the density above the level, min_component_nodes=m those of at least m
    lattice nodes (npcd.hip.components.filter_components, between the density and the isosurface); the mesh then also holds
    "component_nodes", the kept components' node counts in descending order (int64, on the GPU).  normals=True adds "normals"
    [V, 3] fp32, the unit normals of vertex_normals_reference from the gradient of the unfiltered density.

    simplify=k > 0 clusters the vertices on a grid of k lattice spacings from the volume's own origin (npcd.hip.simplify.simplify_mesh,
    DESIGN.md 5.16): a mesh of roughly 1 / k^2 the triangles.  Colours and normals are averaged per cluster as attributes; the normals
    are normalised again, and a mean of zero stays zero.  The mesh then also holds "vertex_cluster" [V] and "face_source" [F'].
    `simplifier` stands in for simplify_mesh (tests of the host logic).  simplify=None leaves the mesh as the isosurface gave it.

    smooth=n runs n iterations of Taubin's smoothing with the factors smooth_lambda and smooth_mu last, after `simplify`
    (npcd.hip.smooth.smooth_mesh): boundary vertices stay where they are.  Only "vertices" changes: normals and
    colours are NOT recomputed -- the normals stay the gradient normals of the unsmoothed surface.  topology=True adds "topology", the
    dict of mesh_topology for the final mesh (one more host read per mesh).  `smoother` stands in for smooth_mesh (tests of the host
    logic); with it, topology=True takes the counts of mesh_edges_reference.  smooth=None, topology=False: the mesh as before.

    deviation=n, with simplify or smooth given, adds "deviation": mesh_deviation(the final mesh, the raw isosurface of the same cloud,
    n), what simplifying and smoothing cost in distance (one more host read per mesh).  Its samples come from a
    generator seeded with DEVIATION_SEED, so two calls agree.  `deviator` stands in for mesh_deviation (tests of the host logic).
    deviation=None: the mesh as before.

    agreement=(extrinsics [T, 4, 4], intrinsics [T, 3, 3]) or (extrinsics, intrinsics, image resolution) adds "agreement":
    mesh_render_agreement(pointnerf, the cloud, the final mesh, the cameras), whether the mesh looks like the field from those cameras
    (one more host read per mesh; the image resolution defaults to mesh_render_agreement's).  `agreer` stands in for
    mesh_render_agreement (tests of the host logic).  agreement=None: the mesh as before.

    enclosure=True adds "enclosure": mesh_enclosure(the final mesh, the lattice, filtered density > level), whether the mesh encloses
    exactly the nodes that the field calls solid (one more host read per mesh).  Simplifying and smoothing move the
    surface, so the report then says by how much in nodes.  `encloser` stands in for mesh_enclosure (tests of the host logic).
    enclosure=False: the mesh as before."""
    from ..hip.isosurface import isosurface
    if agreement is not None:
        if not (isinstance(agreement, (tuple, list)) and len(agreement) in (2, 3) and all(isinstance(t, torch.Tensor) for t in agreement[:2])
                and (len(agreement) == 2 or (isinstance(agreement[2], int) and not isinstance(agreement[2], bool) and agreement[2] > 0))):
            raise ValueError(f"extract_mesh: agreement must be (extrinsics, intrinsics) or (extrinsics, intrinsics, image resolution); got {agreement!r}")
    if deviation is not None:
        if isinstance(deviation, bool) or not isinstance(deviation, int) or deviation < 1:
            raise ValueError(f"extract_mesh: deviation must be a positive number of samples; got {deviation!r}")
        if simplify is None and smooth is None:
            raise ValueError("extract_mesh: deviation compares the final mesh with the raw isosurface; without simplify or smooth there is nothing to compare")
    if smooth is not None and not (isinstance(smooth, int) and not isinstance(smooth, bool) and 0 <= smooth <= 1000):
        raise ValueError(f"extract_mesh: smooth must be a number of iterations in [0, 1000]; got {smooth!r}")
    if smooth is not None and not (0.0 < float(smooth_lambda) <= 1.0 and -1.0 <= float(smooth_mu) <= 0.0):
        raise ValueError(f"extract_mesh: smooth_lambda must lie in (0, 1] and smooth_mu in [-1, 0]; got {smooth_lambda!r} and {smooth_mu!r}")
    if simplify is not None and not (isinstance(simplify, (int, float)) and math.isfinite(simplify) and simplify > 0):
        raise ValueError(f"extract_mesh: simplify must be a positive number of lattice spacings; got {simplify!r}")
    sigma, origin, spacing = pointnerf.density_grid(coords, feats, resolution=resolution, bound=bound, mlp_dtype=mlp_dtype)
    level = default_level(pointnerf) if level is None else float(level)
    filtered, kept_nodes = sigma, None
    if components is not None or min_component_nodes is not None:
        from ..hip.components import filter_components_counted
        filtered, kept_nodes = filter_components_counted(sigma, level, largest=components, min_nodes=min_component_nodes)
    meshes = isosurface(filtered, level, origin, spacing, normals=normals, gradient_of=sigma if normals else None)
    out = []
    for b, (vertices, faces, *rest) in enumerate(meshes):
        mesh = {"vertices": vertices, "faces": faces}
        if normals:
            mesh["normals"] = rest[0]
        if kept_nodes is not None:
            mesh["component_nodes"] = kept_nodes[b]
        if colors:
            if vertices.shape[0]:
                mesh["colors"] = pointnerf.query_field(coords[b:b + 1], feats[b:b + 1], vertices[None], mlp_dtype=mlp_dtype,
                                                       view_dir=view_dir)[1][0]
            else:
                mesh["colors"] = torch.zeros((0, 3), dtype=torch.float32, device=vertices.device)
        if simplify is not None:
            mesh = _simplified(mesh, float(simplify), origin, spacing, sigma.shape[1:], simplifier)
        if smooth is not None or topology:
            mesh = _smoothed(mesh, smooth, float(smooth_lambda), float(smooth_mu), topology, smoother)
        if deviation is not None:
            seeded = torch.Generator(device=vertices.device).manual_seed(DEVIATION_SEED)
            mesh["deviation"] = (mesh_deviation if deviator is None else deviator)(mesh, (vertices, faces), deviation, generator=seeded)
        if agreement is not None:
            size = {} if len(agreement) == 2 else {"resolution": agreement[2]}
            mesh["agreement"] = (mesh_render_agreement if agreer is None else agreer)(pointnerf, coords[b:b + 1], feats[b:b + 1], dict(mesh),
                                                                                       agreement[0], agreement[1], **size)
        if enclosure:
            mesh["enclosure"] = (mesh_enclosure if encloser is None else encloser)(dict(mesh), origin, spacing, filtered[b] > level)
        out.append(mesh)
    return out


def _smoothed(mesh: Dict[str, torch.Tensor], iterations: Optional[int], lam: float, mu: float, topology: bool, smoother=None):
    """The mesh of extract_mesh after `iterations` of smoothing (None: none), with its topology where asked for.  On the GPU the
    edges are built once and serve both."""
    out = dict(mesh)
    vertices, faces = mesh["vertices"], mesh["faces"]
    edges = None
    if smoother is None:
        from ..hip.smooth import mesh_edges, smooth_mesh as smoother
        edges = mesh_edges(vertices.shape[0], faces)
    if iterations is not None:
        out["vertices"] = smoother(vertices, faces, iterations=iterations, lam=lam, mu=mu, edges=edges)
    if topology:
        out["topology"] = mesh_topology(vertices.shape[0], faces.cpu().numpy() if edges is None else faces, edges=edges)
    return out


def _simplified(mesh: Dict[str, torch.Tensor], k: float, origin, spacing, nodes, simplifier=None) -> Dict[str, torch.Tensor]:
    """The mesh of extract_mesh clustered at k lattice spacings on the volume's origin; nodes = (Gz, Gy, Gx)."""
    if simplifier is None:
        from ..hip.simplify import simplify_mesh as simplifier
    cell = [k * float(s) for s in spacing]
    dims = [int(math.floor((g - 1) / k)) + 1 for g in (nodes[2], nodes[1], nodes[0])]          # the cells that reach the last node
    carried = [name for name in ("colors", "normals") if name in mesh]
    attributes = torch.cat([mesh[name] for name in carried], dim=1) if carried else None
    got = simplifier(mesh["vertices"], mesh["faces"], cell, origin=[float(o) for o in origin], dims=dims, attributes=attributes)
    out = dict(mesh)
    out.update(vertices=got["vertices"], faces=got["faces"], vertex_cluster=got["vertex_cluster"], face_source=got["face_source"])
    for i, name in enumerate(carried):
        out[name] = got["attributes"][:, 3 * i:3 * i + 3].contiguous()
    if "normals" in out:
        g = out["normals"]
        unit = g / torch.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])[:, None]
        out["normals"] = torch.where(torch.isfinite(unit).all(dim=1, keepdim=True), unit, torch.zeros_like(unit))
    return out


def colors_to_uint8(colors) -> np.ndarray:
    """[V, 3] colours as PLY stores them: uint8 as they are, floats in [0, 1] clipped and rounded to 0..255."""
    c = colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
    if c.dtype == np.uint8:
        return np.ascontiguousarray(c)
    return np.rint(np.clip(c.astype(np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def write_ply(path, vertices, faces, colors=None, normals=None) -> None:
    """Binary little-endian PLY, written on the host: float32 x y z, optional float32 nx ny nz, optional uchar red green blue, faces
    as `uchar int` lists."""
    v = vertices.detach().cpu().numpy() if isinstance(vertices, torch.Tensor) else np.asarray(vertices)
    f = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    v = np.asarray(v, dtype="<f4").reshape(-1, 3)
    f = np.asarray(f, dtype="<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
    if normals is not None:
        n = normals.detach().cpu().numpy() if isinstance(normals, torch.Tensor) else np.asarray(normals)
        n = np.asarray(n, dtype="<f4").reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError(f"write_ply: {len(v)} vertices and {len(n)} normals")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        c = colors_to_uint8(colors).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"write_ply: {len(v)} vertices and {len(c)} colours")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.empty(len(v), dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vert["nx"], vert["ny"], vert["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
    face["n"], face["v"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
