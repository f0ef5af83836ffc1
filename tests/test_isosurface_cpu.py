"""The CPU restatement of the isosurface's specification (npcd.eval.mesh.marching_tetrahedra_reference) against
geometry, not against itself: closed and consistently oriented surfaces of the right genus, normals, the linear-interpolation bound
of the vertices, the enclosed volume, the ordering conventions and the degenerate inputs; and the PLY writer.  The kernel is then
held to this restatement bit for bit (tests/test_gpu_isosurface.py), which imports the volumes below."""
import functools

import numpy as np
import pytest

from npcd.eval.mesh import EDGE_TYPES, colors_to_uint8, marching_tetrahedra_reference, write_ply

R, CENTRE = 0.6, np.array([0.013, -0.021, 0.034])


def lattice(shape, lo=-1.0, hi=1.0):
    """Node positions [Gz, Gy, Gx, 3] (x, y, z) of a lattice on [lo, hi]^3 in float64, with its origin and spacing."""
    gz, gy, gx = shape
    z, y, x = np.meshgrid(np.linspace(lo, hi, gz), np.linspace(lo, hi, gy), np.linspace(lo, hi, gx), indexing="ij")
    return np.stack([x, y, z], axis=-1), (lo, lo, lo), tuple((hi - lo) / (g - 1) for g in (gx, gy, gz))


def sphere_volume(shape, radius=R, centre=CENTRE):
    p, origin, spacing = lattice(shape)
    return (radius - np.linalg.norm(p - centre, axis=-1)).astype(np.float32), origin, spacing


def two_spheres_volume(G=17):
    p, origin, spacing = lattice((G, G, G))
    a = 0.33 - np.linalg.norm(p - np.array([-0.5, -0.1, 0.05]), axis=-1)
    b = 0.3 - np.linalg.norm(p - np.array([0.45, 0.2, -0.1]), axis=-1)
    return np.maximum(a, b).astype(np.float32), origin, spacing


def blobs_volume(shape, seed=0):
    """A sum of a few Gaussian blobs."""
    rng = np.random.default_rng(seed)
    p, origin, spacing = lattice(shape)
    f = np.zeros(shape)
    for _ in range(4):
        f += rng.uniform(0.5, 1.0) * np.exp(-np.sum((p - rng.uniform(-0.5, 0.5, 3)) ** 2, axis=-1) / rng.uniform(0.05, 0.2))
    return f.astype(np.float32), origin, spacing


@functools.lru_cache(maxsize=None)
def sphere_mesh(G):
    vol, origin, spacing = sphere_volume((G, G, G))
    v, f = marching_tetrahedra_reference(vol, 0.0, origin, spacing)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f, spacing[0]


def directed_edges(faces):
    f = faces.astype(np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def assert_closed_and_oriented(faces):
    """Every directed edge occurs once and its reverse occurs once.  -> the number of undirected edges."""
    e = directed_edges(faces)
    top = int(e.max()) + 1
    keys = e[:, 0] * top + e[:, 1]
    assert len(np.unique(keys)) == len(keys), "a directed edge occurs twice"
    assert np.array_equal(np.sort(keys), np.sort(e[:, 1] * top + e[:, 0])), "an edge without its reverse"
    return len(keys) // 2


def normals(vertices, faces):
    v = vertices.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3.0


# ---- the sphere ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G, shortfall, count", [(17, 0.04, (1270, 2536)), (33, 0.01, (5174, 10344))])
def test_sphere(G, shortfall, count):
    v, f, h = sphere_mesh(G)
    print(f"G {G}: {len(v)} vertices, {len(f)} faces")
    assert (len(v), len(f)) == count
    edges = assert_closed_and_oriented(f)
    assert len(v) - edges + len(f) == 2
    n, mid = normals(v, f)
    assert (np.linalg.norm(n, axis=1) > 0).all(), "a zero-area triangle"
    assert (np.sum(n * (mid - CENTRE), axis=1) > 0).all(), "a normal points toward the centre"
    # linear interpolation of f along the longest lattice edge, sqrt(3) h
    deviation = np.abs(np.linalg.norm(v.astype(np.float64) - CENTRE, axis=1) - R)
    bound = 3 * h * h / (8 * (R - np.sqrt(3) * h)) + 1e-6
    print(f"G {G}: max deviation {deviation.max():.5f}, bound {bound:.5f}")
    assert deviation.max() <= bound
    # the surface is inscribed: the enclosed volume falls short
    p = v.astype(np.float64) - CENTRE
    volume = np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0
    rel = volume / (4.0 * np.pi * R ** 3 / 3.0) - 1.0
    print(f"G {G}: enclosed volume {100 * rel:+.2f} %")
    assert -shortfall <= rel <= 0.0


def test_two_disjoint_spheres():
    vol, origin, spacing = two_spheres_volume()
    v, f = marching_tetrahedra_reference(vol, 0.0, origin, spacing)
    edges = assert_closed_and_oriented(f)
    assert len(v) - edges + len(f) == 4


# ---- conventions --------------------------------------------------------------------------------------------------------------------------
def owning_edges(vertices, origin, spacing, shape):
    """(node, edge type) of every vertex, recomputed from its coordinates: the axes along which it lies strictly between two nodes
    are the edge's direction, the node below is the owner."""
    g = (vertices.astype(np.float64) - np.asarray(origin)) / np.asarray(spacing)
    frac = g - np.floor(g)
    moving = (frac > 1e-4) & (frac < 1 - 1e-4)
    assert moving.any(axis=1).all() and (np.abs(g - np.rint(g))[~moving] < 1e-4).all(), "a vertex too near a node to tell its edge"
    lower = np.where(moving, np.floor(g), np.rint(g)).astype(np.int64)
    types = np.array([EDGE_TYPES.index(tuple(int(d) for d in row)) for row in moving])
    gz, gy, gx = shape
    return (lower[:, 2] * gy + lower[:, 1]) * gx + lower[:, 0], types


def test_order_of_vertices_and_start_of_triangles():
    for shape in ((17, 17, 17), (9, 12, 15)):
        vol, origin, spacing = sphere_volume(shape)
        v, f = marching_tetrahedra_reference(vol, 0.0, origin, spacing)
        assert len(f) and (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()
        node, types = owning_edges(v, origin, spacing, shape)
        keys = node * 7 + types
        assert (np.diff(keys) > 0).all()
        assert v.dtype == np.float32 and f.dtype == np.int32


# ---- degenerate inputs ----------------------------------------------------------------------------------------------------------------------
def test_uniform_volumes_are_empty():
    for value in (1.0, -1.0):
        v, f = marching_tetrahedra_reference(np.full((3, 4, 5), value, dtype=np.float32), 0.0)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == np.float32 and f.dtype == np.int32


@pytest.mark.parametrize("corner", [0, 7])
def test_one_inside_corner_of_a_single_cell(corner):
    vol = np.full(8, -1.0, dtype=np.float32)
    vol[corner] = 1.0
    v, f = marching_tetrahedra_reference(vol.reshape(2, 2, 2), 0.0)
    assert len(v) == 7 and len(f) == 6          # one vertex per edge at that corner, one triangle per tetrahedron
    assert np.allclose(np.abs(v - np.array([corner & 1, corner >> 1 & 1, corner >> 2])).max(axis=1), 0.5)
    n, mid = normals(v, f)
    away = mid - np.array([corner & 1, corner >> 1 & 1, corner >> 2])
    assert (np.sum(n * away, axis=1) > 0).all()


def test_a_sample_equal_to_the_level_is_outside():
    vol = np.full((3, 3, 3), -1.0, dtype=np.float32)
    vol[1, 1, 1] = 0.25
    v, f = marching_tetrahedra_reference(vol, 0.25)
    assert len(v) == 0 and len(f) == 0
    # beside inside nodes it is the outside end of its edges: the vertices lie on it, the triangles have no area and are kept
    vol = np.full((3, 3, 3), 1.0, dtype=np.float32)
    vol[1, 1, 1] = 0.25
    v, f = marching_tetrahedra_reference(vol, 0.25)
    assert len(v) == 14 and len(f) == 24 and (v == 1.0).all()
    assert_closed_and_oriented(f)
    assert (f[:, 0] < f[:, 1]).all() and (f[:, 0] < f[:, 2]).all()


def test_a_nan_sample_disturbs_its_own_edges_only():
    vol, origin, spacing = blobs_volume((6, 7, 8), seed=3)
    level = float(np.median(vol))
    plain = vol.copy()
    plain[2, 3, 4] = level - 1.0          # outside, like the NaN
    bad = vol.copy()
    bad[2, 3, 4] = np.nan
    v0, f0 = marching_tetrahedra_reference(plain, level, origin, spacing)
    v1, f1 = marching_tetrahedra_reference(bad, level, origin, spacing)
    assert np.array_equal(f0, f1) and v0.shape == v1.shape and f1.min() >= 0 and f1.max() < len(v1)
    broken = ~np.isfinite(v1).all(axis=1)
    assert broken.any() and np.array_equal(v0[~broken], v1[~broken])
    # the broken vertices are those of the edges that end in the node
    p = np.array([origin[0] + 4 * spacing[0], origin[1] + 3 * spacing[1], origin[2] + 2 * spacing[2]])
    assert (np.abs(v0[broken].astype(np.float64) - p).max(axis=1) <= np.max(spacing) + 1e-6).all()
    inside = plain > level
    touching = sum(int(inside[2 + s * dz, 3 + s * dy, 4 + s * dx]) for dx, dy, dz in EDGE_TYPES for s in (1, -1))
    assert int(broken.sum()) == touching


# ---- the kernels' resources, from the compiler's own output ----------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_the_wrapper_knows_the_strip(tmp_path):
    import re

    from npcd.hip.isosurface import STRIP_NODES
    from test_kernel_resources import CSRC, _compile
    source = open(f"{CSRC}/isosurface.hip").read()
    assert int(re.search(r"constexpr int kIsoThreads = (\d+);", source).group(1)) == STRIP_NODES
    kernels = _compile("isosurface.hip", str(tmp_path / "isosurface.s"))
    assert len(kernels) == 3, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (name, k)          # 1,024 lanes a workgroup: 16 waves, 128 registers each at most
        assert k["lds"] == 128, (name, k)                                 # the 16 wave totals of the scan


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    """A reader for what write_ply writes: parse the header, np.frombuffer the body."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln.split()[1:] for ln in lines if ln.startswith("property ")]
    kinds = {"float": "<f4", "uchar": "u1"}
    vertex = np.dtype([(p[1], kinds[p[0]]) for p in props if p[0] != "list"])
    assert ["list", "uchar", "int", "vertex_indices"] in props
    face = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    nv, nf = counts["vertex"], counts["face"]
    assert len(raw) == end + nv * vertex.itemsize + nf * face.itemsize
    vert = np.frombuffer(raw, dtype=vertex, count=nv, offset=end)
    faces = np.frombuffer(raw, dtype=face, count=nf, offset=end + nv * vertex.itemsize)
    assert (faces["n"] == 3).all()
    xyz = np.stack([vert["x"], vert["y"], vert["z"]], axis=1)
    rgb = np.stack([vert["red"], vert["green"], vert["blue"]], axis=1) if "red" in vertex.names else None
    return xyz, faces["v"], rgb


def test_write_ply(tmp_path):
    v, f, _ = sphere_mesh(17)
    colors = np.random.default_rng(0).uniform(-0.1, 1.1, (len(v), 3)).astype(np.float32)
    write_ply(tmp_path / "plain.ply", v, f)
    xyz, faces, rgb = read_ply(tmp_path / "plain.ply")
    assert rgb is None and np.array_equal(xyz, v) and np.array_equal(faces, f)
    write_ply(tmp_path / "coloured.ply", v, f, colors)
    xyz, faces, rgb = read_ply(tmp_path / "coloured.ply")
    assert np.array_equal(xyz, v) and np.array_equal(faces, f)
    want = np.rint(np.clip(colors.astype(np.float64), 0, 1) * 255).astype(np.uint8)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, want) and np.array_equal(colors_to_uint8(colors), want)
    write_ply(tmp_path / "bytes.ply", v, f, want)
    assert np.array_equal(read_ply(tmp_path / "bytes.ply")[2], want)
    write_ply(tmp_path / "empty.ply", np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    xyz, faces, _ = read_ply(tmp_path / "empty.ply")
    assert xyz.shape == (0, 3) and faces.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(tmp_path / "bad.ply", v, f, colors[:-1])
