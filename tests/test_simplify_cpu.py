"""Vertex clustering without a GPU: the CPU restatement npcd.eval.mesh.simplify_reference against geometry and the
exact cases of the specification, not against itself; the attribute means against the float64 mean; the per-lane code of
csrc/simplify.h, the code the kernels run, built for the host with sanitizers (csrc/simplify_host.cpp) and held bit for bit to the
reference on the meshes of the GPU test (tests/test_gpu_simplify.py, which imports them from here); the kernels' resources from the
compiler's own output, the entry points' refusals, the wrapper's argument errors and extract_mesh with stand-ins."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from npcd.eval.mesh import (attribute_means_reference, clustering_grid, marching_tetrahedra_reference, simplify_reference,
                            vertex_normals_reference)
from test_isosurface_cpu import sphere_volume
from test_kernel_resources import CSRC, _compile

STRIP = 256          # kSimpStrip of csrc/simplify.h; test_the_wrapper_knows_the_constants holds it to the source
FACES = (1, 4, 63, 64, 65, 255, 256, 257, 16387)
X_CELLS = (31, 32, 33, 65)
KEYS = ("vertices", "faces", "attributes", "vertex_cluster", "face_source")


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def soup(F, seed=0, plant=True):
    """A random triangle soup in the unit cube; every fifth face is a copy of an earlier one, rotated or turned over, so that faces
    repeat as sets whatever the grid."""
    rng = np.random.default_rng(1000 * seed + F)
    V = max(3, min(F, 20000) // 2 + 3)
    v = rng.random((V, 3)).astype(np.float32)
    f = rng.integers(0, V, (F, 3)).astype(np.int32)
    if plant:
        for i in range(4, F, 5):
            f[i] = f[rng.integers(0, i)][[[1, 2, 0], [2, 1, 0], [0, 2, 1]][i % 3]]
    return v, f


def sphere(G=24, radius=0.6):
    vol, origin, spacing = sphere_volume((G, G, G), radius=radius)
    v, f = marching_tetrahedra_reference(vol, 0.0, origin, spacing)
    return v, f, vertex_normals_reference(vol, 0.0, spacing), origin, spacing


def sphere_grid(G, k, origin, spacing):
    """The grid extract_mesh(simplify=k) takes."""
    return dict(cell=[k * float(s) for s in spacing], origin=[float(o) for o in origin], dims=[(G - 1) // k + 1] * 3)


def lattice_mesh(n=6, seed=3):
    """Vertices at the nodes of an integer lattice, moved by at most 0.2 per axis: two of them differ by at least 0.6 along some axis,
    so a cell of 0.25 holds at most one.  Faces: random triples of different vertices."""
    rng = np.random.default_rng(seed)
    nodes = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    v = (nodes + rng.uniform(-0.2, 0.2, nodes.shape)).astype(np.float32)
    f = np.stack([rng.choice(len(v), 3, replace=False) for _ in range(400)]).astype(np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(vertices, faces, cell, origin, dims, attributes, two_pass): the arguments of one call."""
    kind, _, arg = name.partition(":")
    c = dict(origin=None, dims=None, attributes=None, two_pass=None)
    rng = np.random.default_rng(len(name) * 7 + 1)
    if kind == "faces":          # wave and workgroup edges of the face launches, and of the vertex launches (V = F / 2 + 3)
        c["vertices"], c["faces"] = soup(int(arg))
        c.update(cell=0.13, origin=[0.0, 0.0, 0.0], dims=[8, 8, 8])
        c["attributes"] = rng.standard_normal((len(c["vertices"]), 3)).astype(np.float32)
    elif kind == "xcells":          # keys that straddle bitmap words
        x = int(arg)
        c["vertices"], c["faces"] = soup(700, seed=x)
        c.update(cell=[1.0 / x, 0.34, 0.5], origin=[0.0, 0.0, 0.0], dims=[x, 3, 2])
    elif kind == "strips":          # more bitmap words than `arg` strips and one word; vertices in the first and the last cell only
        words = int(arg) * STRIP + 2
        v = np.float32([[0.5, 0.5, 0.5], [0.25, 0.5, 0.75], [31.5, words - 0.5, 0.5], [31.75, words - 0.25, 0.25], [0.75, 0.25, 0.5]])
        c["vertices"], c["faces"] = v, np.int32([[0, 2, 1], [2, 0, 3], [0, 1, 4], [3, 4, 2]])
        c.update(cell=1.0, origin=[0.0, 0.0, 0.0], dims=[32, words, 1])
        c["attributes"] = np.float32([[1], [2], [3], [4], [6]])
    elif kind == "one_cell":
        c["vertices"], c["faces"] = soup(300, seed=2)
        c.update(cell=2.0, origin=[-0.5, -0.5, -0.5], dims=[1, 1, 1])
        c["attributes"] = rng.standard_normal((len(c["vertices"]), 2)).astype(np.float32)
    elif kind == "own_cells":
        c["vertices"], c["faces"] = lattice_mesh()
        c.update(cell=0.25)          # the grid from the bounds
        c["attributes"] = rng.standard_normal((len(c["vertices"]), 3)).astype(np.float32)
    elif kind == "lost":          # 1 % of the vertices have a coordinate that is not finite
        v, f = soup(3000, seed=4)
        bad = rng.choice(len(v), len(v) // 100, replace=False)
        v[bad, rng.integers(0, 3, len(bad))] = np.float32([np.nan, np.inf, -np.inf])[rng.integers(0, 3, len(bad))]
        at = rng.standard_normal((len(v), 3)).astype(np.float32)
        at[bad[0], 1], at[5, 0] = np.inf, np.nan
        c.update(vertices=v, faces=f, cell=0.07, attributes=at)          # the grid from the bounds of the finite vertices
    elif kind == "no_faces":
        c["vertices"], c["faces"] = soup(40)[0], np.zeros((0, 3), dtype=np.int32)
        c.update(cell=0.3, attributes=rng.standard_normal((len(c["vertices"]), 3)).astype(np.float32))
    elif kind == "no_vertices":
        c["vertices"], c["faces"] = np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)
        c.update(cell=0.3, attributes=np.zeros((0, 4), dtype=np.float32))
    elif kind == "all_lost":
        c["vertices"], c["faces"] = np.full((7, 3), np.nan, dtype=np.float32), np.int32([[0, 1, 2], [3, 4, 5]])
        c.update(cell=0.3)
    elif kind == "bad_indices":          # indices outside [0, V) are not followed
        v, f = soup(200, seed=6)
        f[3], f[50], f[120] = (-1, 2, 3), (1, len(v), 2), (1, 2, 2 ** 31 - 1)
        c.update(vertices=v, faces=f, cell=0.2)
    elif kind == "sphere":          # the 24^3 isosurface at k = arg, colours and normals as six channels
        v, f, normals, origin, spacing = sphere()
        colours = (0.5 + 0.5 * np.sin(7.0 * v)).astype(np.float32)
        c.update(vertices=v, faces=f, attributes=np.concatenate([colours, normals], axis=1), **sphere_grid(24, int(arg), origin, spacing))
    elif kind == "channels":
        c["vertices"], c["faces"] = soup(500, seed=8)
        scale = np.float32(2.0) ** rng.integers(-20, 21, (len(c["vertices"]), int(arg)))
        c.update(cell=0.21, attributes=(rng.standard_normal(scale.shape) * scale).astype(np.float32))
    elif kind == "two_pass":          # the same mesh by one packed key and by two stable passes
        c["vertices"], c["faces"] = soup(2000, seed=9)
        c.update(cell=0.11, two_pass=arg == "on")
    else:
        raise KeyError(name)
    return c


CASES = ([f"faces:{F}" for F in FACES] + [f"xcells:{x}" for x in X_CELLS] +
         ["strips:1", "strips:256", "one_cell", "own_cells", "lost", "no_faces", "no_vertices", "all_lost", "bad_indices", "sphere:2",
          "channels:1", "channels:16", "two_pass:on", "two_pass:off"])


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return simplify_reference(c["vertices"], c["faces"], c["cell"], c["origin"], c["dims"], c["attributes"])


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    raw = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    differ = np.nonzero(got.view(raw).reshape(-1) != want.view(raw).reshape(-1))[0]
    assert differ.size == 0, f"{what}: {differ.size} of {got.size} differ, first at {differ[0]}: {got.reshape(-1)[differ[0]]!r} != {want.reshape(-1)[differ[0]]!r}"


def hold(got, name, what):
    """got: key -> array; every output equals the reference's, bit for bit."""
    want = reference(name)
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key in want:
        same_bits(got[key], want[key], f"{what}: {key}")


def keys_of(v, origin, cell, dims):
    """The cell coordinates and keys of finite vertices on a grid whose arithmetic is exact in float64 for them."""
    c = np.clip(np.floor((v.astype(np.float64) - origin) / cell), 0, np.asarray(dims) - 1).astype(np.int64)
    return c, (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]


# ---- the reference against geometry ----------------------------------------------------------------------------------------------------------
def test_a_fine_grid_changes_nothing_but_the_numbering():
    v, f = lattice_mesh()
    v = np.concatenate([v, v[:5], np.float32([[np.nan, 0, 0]])])          # five vertices twice, one lost
    f = np.concatenate([f, np.int32([[len(v) - 1, 0, 1], [len(v) - 6, 7, 8]])])
    cell = 0.25
    out = simplify_reference(v, f, cell)
    cluster = out["vertex_cluster"]
    finite = np.isfinite(v).all(axis=1)
    assert len(out["vertices"]) == len(np.unique(v[finite], axis=0)) == len(v) - 6
    assert (cluster[~finite] == -1).all() and (cluster[finite] >= 0).all()
    assert np.array_equal(cluster[-6:-1], cluster[:5])
    # the faces are the input's, renumbered: only the face through the lost vertex goes (no other two share a set of corners)
    kept = np.arange(len(f)) != len(f) - 2
    assert np.array_equal(out["face_source"], np.nonzero(kept)[0])
    assert np.array_equal(out["faces"], cluster[f[kept]])
    # the mean of one place (or of the same place twice) is that place, floored to 2^-32 of the cell, then rounded to fp32
    moved = np.abs(out["vertices"][cluster[finite]].astype(np.float64) - v[finite].astype(np.float64))
    assert (moved <= cell * 2.0 ** -32 + np.spacing(np.abs(v[finite])).astype(np.float64)).all(), moved.max()


@pytest.mark.parametrize("name", ["faces:16387", "xcells:33", "one_cell", "own_cells", "lost", "sphere:2", "strips:1"])
def test_representatives_lie_in_their_cells(name):
    """origin + cell (c + m), m in [0, 1], ascends with m in float64, and so does the rounding to fp32: a representative lies between
    the fp32 roundings of its cell's two faces.  And vertex_cluster is a non-decreasing function of the key."""
    c, out = case(name), reference(name)
    v = c["vertices"]
    finite = np.isfinite(v).all(axis=1)
    lower, upper = (v[finite].min(axis=0), v[finite].max(axis=0))
    origin, cell, dims = clustering_grid(c["cell"], c["origin"], c["dims"], lower, upper)
    coords, key = keys_of(v[finite], origin, cell, dims)
    cluster = out["vertex_cluster"][finite].astype(np.int64)
    order = np.argsort(key, kind="stable")
    assert (np.diff(cluster[order]) >= 0).all()
    assert np.array_equal(np.diff(cluster[order]) > 0, np.diff(key[order]) > 0)
    assert len(out["vertices"]) == len(np.unique(key)) and cluster.max() == len(out["vertices"]) - 1
    cell_of = np.zeros((len(out["vertices"]), 3), dtype=np.int64)
    cell_of[cluster] = coords
    low = (origin + cell * cell_of.astype(np.float64)).astype(np.float32)
    high = (origin + cell * (cell_of.astype(np.float64) + 1.0)).astype(np.float32)
    assert ((out["vertices"] >= low) & (out["vertices"] <= high)).all()


@pytest.mark.parametrize("k", [2, 3])
def test_a_sphere_gets_coarser(k):
    v, f, _, origin, spacing = sphere()
    grid = sphere_grid(24, k, origin, spacing)
    out = simplify_reference(v, f, **grid)
    faces, cluster = out["faces"].astype(np.int64), out["vertex_cluster"]
    assert 0 < len(faces) < len(f) and len(out["vertices"]) < len(v)
    assert (cluster >= 0).all()
    diagonal = float(np.linalg.norm(grid["cell"]))
    assert (np.linalg.norm(out["vertices"][cluster].astype(np.float64) - v, axis=1) <= diagonal).all()
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    assert len(np.unique(np.sort(faces, axis=1), axis=0)) == len(faces)
    assert (np.diff(out["face_source"]) > 0).all()
    assert np.array_equal(faces, cluster[f[out["face_source"]]])
    # the sphere stays a sphere: every new vertex within a cell diagonal of the radius
    radius = np.linalg.norm(out["vertices"] - np.float32([0.013, -0.021, 0.034]), axis=1)
    assert (np.abs(radius - 0.6) < diagonal).all()


def test_exact_cases():
    unit = dict(cell=1.0, origin=[0.0, 0.0, 0.0])
    # two faces on the same three cells, wound against each other: the lower index stays, with its own corner order
    v = np.float32([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.25, 0.75, 0.5], [1.25, 0.25, 0.5], [0.75, 1.25, 0.5]])
    out = simplify_reference(v, np.int32([[4, 3, 5], [0, 1, 2], [2, 0, 1]]), dims=[2, 2, 1], **unit)
    assert out["vertex_cluster"].tolist() == [0, 1, 2, 0, 1, 2]
    assert out["faces"].tolist() == [[1, 0, 2]] and out["face_source"].tolist() == [0]
    assert out["vertices"].tolist() == [[0.375, 0.625, 0.5], [1.375, 0.375, 0.5], [0.625, 1.375, 0.5]]          # exact means
    # a face through a NaN vertex goes, and the vertex maps to -1
    w = v.copy()
    w[3, 1] = np.nan
    out = simplify_reference(w, np.int32([[4, 3, 5], [0, 1, 2]]), dims=[2, 2, 1], **unit)
    assert out["vertex_cluster"].tolist() == [0, 1, 2, -1, 1, 2]
    assert out["faces"].tolist() == [[0, 1, 2]] and out["face_source"].tolist() == [1]
    assert out["vertices"][0].tolist() == [0.5, 0.5, 0.5]
    # a vertex on a cell boundary belongs to the upper cell; on the far face of the grid, and beyond it, to the last cell
    b = np.float32([[1.0, 0.0, 0.0], [2.0, 0.5, 0.5], [0.999, 0.0, 0.0], [7.0, -3.0, 0.5]])
    out = simplify_reference(b, np.zeros((0, 3), np.int32), dims=[2, 1, 1], **unit)
    assert out["vertex_cluster"].tolist() == [1, 1, 0, 1]
    # the clamped places: (0, 0, 0), (1 - 2^-32, .5, .5), (1 - 2^-32, 0, .5) in the cell; their mean, rounded to fp32
    third = lambda *m: float(np.float32(sum(int(x * 2 ** 32) if x < 1 else 2 ** 32 - 1 for x in m) / 3 / 2 ** 32))
    assert out["vertices"][1].tolist() == [float(np.float32(1 + (2 * (2 ** 32 - 1) / 3) / 2 ** 32)), third(0, .5, 0), third(0, .5, .5)]
    assert out["faces"].shape == (0, 3) and out["face_source"].shape == (0,)
    # one cell takes everything
    one = reference("one_cell")
    assert len(one["vertices"]) == 1 and len(one["faces"]) == 0 and (one["vertex_cluster"] == 0).all()
    centroid = case("one_cell")["vertices"].astype(np.float64).mean(axis=0)
    assert np.abs(one["vertices"][0] - centroid).max() < 1e-6
    # nothing at all, and nothing finite
    for name in ("no_vertices", "all_lost"):
        empty = reference(name)
        assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and (empty["vertex_cluster"] == -1).all()
    # indices outside [0, V)
    assert not np.isin([3, 50, 120], reference("bad_indices")["face_source"]).any()
    # the same mesh by both sorting schemes is one case of the reference
    for key, value in reference("two_pass:on").items():
        same_bits(value, reference("two_pass:off")[key], key)


def test_outputs_of_the_reference():
    for name in CASES:
        c, out = case(name), reference(name)
        V, F = len(c["vertices"]), len(c["faces"])
        assert set(out) == set(KEYS) - (set() if c["attributes"] is not None else {"attributes"}), name
        assert out["vertices"].dtype == np.float32 and out["vertices"].ndim == 2 and out["vertices"].shape[1] == 3
        assert out["faces"].dtype == np.int32 and out["faces"].shape == (len(out["face_source"]), 3) and len(out["faces"]) <= F
        assert out["vertex_cluster"].dtype == np.int32 and out["vertex_cluster"].shape == (V,)
        assert out["face_source"].dtype == np.int32
        if c["attributes"] is not None:
            assert out["attributes"].dtype == np.float32 and out["attributes"].shape == (len(out["vertices"]), c["attributes"].shape[1])
        if name.startswith("faces:") and F >= 63:
            assert 0 < len(out["faces"]) < F, name          # something collapses or repeats, something stays


def test_attribute_means_are_within_their_bound():
    """Values spanning 2^-20 .. 2^20 with a NaN and an infinity: the float64 stage of the means lies within A 2^-29 of the exact mean
    (taken in float64 with math.fsum, the value that is not finite as 0), and simplify_reference returns its rounding to fp32."""
    import math
    rng = np.random.default_rng(11)
    V, C, K = 5000, 5, 37
    a = (rng.standard_normal((V, C)) * 2.0 ** rng.uniform(-20, 20, (V, C))).astype(np.float32)
    a[17, 2], a[400, 0] = np.nan, np.inf
    cluster = rng.integers(-1, K, V)
    clean = np.where(np.isfinite(a), a, 0).astype(np.float64)
    A = float(np.abs(clean).max())
    assert 2.0 ** 15 < A < 2.0 ** 26
    means = attribute_means_reference(a, cluster, K)
    assert means.dtype == np.float64 and means.shape == (K, C)
    worst = 0.0
    for k in range(K):
        rows = clean[cluster == k]
        for ch in range(C):
            worst = max(worst, abs(means[k, ch] - math.fsum(rows[:, ch]) / len(rows)))
    print(f"largest error of a mean {worst:.3e}, bound A 2^-29 = {A * 2.0 ** -29:.3e}")
    assert worst <= A * 2.0 ** -29
    # through simplify_reference: the same numbers, rounded to fp32 -- one cell per cluster along x
    v = np.stack([np.maximum(cluster, 0) + 0.5, np.full(V, 0.5), np.full(V, 0.5)], axis=1).astype(np.float32)
    v[cluster < 0] = np.nan
    out = simplify_reference(v, np.zeros((0, 3), np.int32), 1.0, origin=[0.0, 0.0, 0.0], dims=[K, 1, 1], attributes=a)
    assert np.array_equal(out["vertex_cluster"], cluster)
    same_bits(out["attributes"], means.astype(np.float32), "attributes")
    # all zero, and nothing finite: zeros
    assert not attribute_means_reference(np.full((4, 2), np.nan, np.float32), np.zeros(4, np.int64), 1).any()
    # a denormal largest value keeps its bits
    tiny = np.float32([[1e-45], [3e-45]])
    assert attribute_means_reference(tiny, np.int64([0, 1]), 2).astype(np.float32).tolist() == tiny.tolist()


def test_the_grid_from_the_bounds():
    origin, cell, dims = clustering_grid(0.25, None, None, lower=[0.0, -1.0, 2.0], upper=[1.0, -1.0, 2.74])
    assert origin.tolist() == [0.0, -1.0, 2.0] and cell.tolist() == [0.25] * 3 and dims == [5, 1, 3]
    assert clustering_grid([1, 2, 4])[2] == [1, 1, 1] and clustering_grid([1, 2, 4])[0].tolist() == [0.0] * 3
    assert clustering_grid(1.0, [0, 0, 0], [1024, 1024, 1024])[2] == [1024] * 3
    with pytest.raises(ValueError, match=r"1025 x 1024 x 1024 = 1074790400 cells"):
        clustering_grid(1.0, [0, 0, 0], [1025, 1024, 1024])
    with pytest.raises(ValueError, match="cells"):
        clustering_grid(1e-6, None, None, lower=[0, 0, 0], upper=[1, 1, 1])
    for bad in (0.0, -1.0, float("nan"), float("inf"), [1.0, 0.0, 1.0]):
        with pytest.raises(ValueError, match="cell"):
            clustering_grid(bad)
    with pytest.raises(ValueError, match="origin"):
        clustering_grid(1.0, [0.0, float("nan"), 0.0])
    with pytest.raises(ValueError, match="dims"):
        clustering_grid(1.0, [0, 0, 0], [4, 0, 4])


# ---- the per-lane code on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/simplify_host.cpp, the per-lane functions of csrc/simplify.h as plain loops, built with the host compiler, its address and
    undefined-behaviour sanitizers and without FMA contraction: a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("simplify_host") / "simplify_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CSRC, "simplify_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def grid_of(c):
    """The grid of a case as host values, as the wrapper makes it."""
    v = c["vertices"]
    finite = np.isfinite(v).all(axis=1)
    lower, upper = (v[finite].min(axis=0), v[finite].max(axis=0)) if finite.any() else (None, None)
    return clustering_grid(c["cell"], c["origin"], c["dims"], lower, upper)


def run_on_the_host(program, tmp_path, name, reverse):
    c = case(name)
    origin, cell, dims = grid_of(c)
    V, F = len(c["vertices"]), len(c["faces"])
    C = 0 if c["attributes"] is None else c["attributes"].shape[1]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([V, F, C, int(bool(c["two_pass"]))], dtype="<i4").tobytes() + origin.astype("<f8").tobytes() +
                 cell.astype("<f8").tobytes() + np.array(dims + [0], dtype="<i4").tobytes())
        for a in (c["vertices"], c["faces"], c["attributes"]):
            if a is not None:
                fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + (["reverse"] if reverse else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    Vp, Fp = (int(x) for x in np.frombuffer(raw, dtype="<i8", count=2))
    out, at_byte = {}, 16
    for key, dtype, shape in (("vertices", "<f4", (Vp, 3)), ("faces", "<i4", (Fp, 3)), ("attributes", "<f4", (Vp, C) if C else None),
                              ("vertex_cluster", "<i4", (V,)), ("face_source", "<i4", (Fp,))):
        if shape is None:
            continue
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype=dtype, count=count, offset=at_byte).reshape(shape)
        at_byte += count * np.dtype(dtype).itemsize
    assert at_byte == len(raw)
    return out


@pytest.mark.parametrize("name", CASES)
def test_the_lanes_on_the_host(host_program, tmp_path, name):
    for reverse in (False, True):
        hold(run_on_the_host(host_program, tmp_path, name, reverse), name, f"{name} reverse {reverse}")


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_knows_the_constants():
    from npcd import hip
    from npcd.hip import simplify, surface
    source = open(f"{CSRC}/simplify.h").read()
    assert int(re.search(r"constexpr int kSimpStrip = (\d+);", source).group(1)) == simplify.STRIP_WORDS == STRIP
    assert int(re.search(r"constexpr int kSimpThreads = (\d+);", source).group(1)) == STRIP          # one entry of a strip per lane
    assert int(re.search(r"constexpr int kSimpMaxChannels = (\d+);", source).group(1)) == simplify.MAX_CHANNELS == surface.MAX_CHANNELS
    assert "kSimpPackedIds = (int64_t)1 << 21" in source and simplify.PACKED_IDS == 2 ** 21
    assert hip.simplify_mesh is simplify.simplify_mesh


def test_kernels_use_no_scratch(tmp_path):
    kernels = _compile("simplify.hip", str(tmp_path / "simplify.s"))
    assert len(kernels) == 9, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 64, (name, k)
        # the four wave totals of a workgroup's scan (csrc/block_scan.h); the totals launch takes its carry from the scan's total
        want = 32 if ("simp_totals" in name or "simp_rank" in name or "simp_flags" in name) else 0
        assert k["lds"] == want, (name, k)
    text = open(tmp_path / "simplify.s").read()
    assert "global_atomic_add_x2" in text and "global_atomic_or" in text and "global_atomic_umax" in text
    assert "cmpswap" not in text          # every atomic is one instruction, not a compare-and-swap loop


def test_header_exports_and_signatures():
    from npcd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "npcd_hip.h")).read()
    L = hip.lib()
    names = ("npcd_simplify_ws_bytes", "npcd_simplify_cluster", "npcd_simplify_faces", "npcd_simplify_unique", "npcd_simplify_emit")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in hip.SIGNATURES and hasattr(L, name), name
    assert L.npcd_missing == () and L.npcd_abi_version() == 10
    assert hip.SIGNATURES["npcd_simplify_ws_bytes"][0] is ctypes.c_int64
    assert [len(hip.SIGNATURES[n][1]) for n in names] == [4, 12, 10, 8, 14]
    # the host-side refusals, which look at no pointer's target and launch nothing
    ints = lambda *d: (ctypes.c_int * 3)(*d)
    doubles = lambda *d: (ctypes.c_double * 3)(*d)
    V, F, C, dims = 1000, 3000, 3, ints(40, 30, 20)
    cells, words = 24000, 750
    assert L.npcd_simplify_ws_bytes(V, F, C, dims) == 8 * V * (3 + C) + 4 * (V + 1 + words) + 4 * (words + 3 + V + 3 * V + 3 * F + F + 12)
    assert L.npcd_simplify_ws_bytes(V, F, 0, ints(2, 2, 2)) == 8 * 8 * 3 + 4 * (8 + 1 + 1) + 4 * (1 + 1 + 8 + 3 * V + 4 * F + 12)
    assert L.npcd_simplify_ws_bytes(0, 0, 0, ints(1, 1, 1)) == 4 * 2 + 4 * 2
    assert L.npcd_simplify_ws_bytes(-1, F, C, dims) == -1 and L.npcd_simplify_ws_bytes(V, -1, C, dims) == -1
    assert L.npcd_simplify_ws_bytes(V, F, -1, dims) == -1 and L.npcd_simplify_ws_bytes(V, F, C, ints(4, 0, 4)) == -1
    assert L.npcd_simplify_ws_bytes(V, F, C, None) == -1
    assert L.npcd_simplify_ws_bytes(V, F, 17, dims) == -2 and L.npcd_simplify_ws_bytes(2 ** 31, F, C, dims) == -2
    assert L.npcd_simplify_ws_bytes(V, 2 ** 31, C, dims) == -2 and L.npcd_simplify_ws_bytes(V, F, C, ints(1025, 1024, 1024)) == -2
    assert L.npcd_simplify_ws_bytes(V, F, C, ints(1024, 1024, 1024)) > 0 and L.npcd_simplify_ws_bytes(V, F, C, ints(2 ** 30, 2, 1)) == -2
    one = ctypes.c_void_p(64)          # never followed: every call below is refused before a launch
    origin, cell = doubles(0, 0, 0), doubles(1, 1, 1)

    def refused(fn, args, **changed):
        a = list(args)
        for i, value in changed.items():
            a[int(i[1:])] = value
        return fn(*a)
    #          vertices, V, F, attributes, C, origin, cell, dims, ws, vertex_cluster, counts, stream
    cluster = [one, V, F, one, C, origin, cell, dims, one, one, one, None]
    for missing in (0, 3, 5, 6, 7, 8, 9, 10):
        assert refused(L.npcd_simplify_cluster, cluster, **{f"_{missing}": None}) == -1, missing
    assert refused(L.npcd_simplify_cluster, cluster, _1=0) == -1 and refused(L.npcd_simplify_cluster, cluster, _4=0) == -1          # attributes without channels
    assert refused(L.npcd_simplify_cluster, cluster, _6=doubles(1, 0, 1)) == -1 and refused(L.npcd_simplify_cluster, cluster, _6=doubles(1, float("nan"), 1)) == -1
    assert refused(L.npcd_simplify_cluster, cluster, _5=doubles(0, float("inf"), 0)) == -1
    assert refused(L.npcd_simplify_cluster, cluster, _8=ctypes.c_void_p(68)) == -1 and refused(L.npcd_simplify_cluster, cluster, _10=ctypes.c_void_p(68)) == -1
    assert refused(L.npcd_simplify_cluster, cluster, _4=17) == -2 and refused(L.npcd_simplify_cluster, cluster, _1=2 ** 31) == -2
    assert refused(L.npcd_simplify_cluster, cluster, _7=ints(1025, 1024, 1024)) == -2
    #        faces, V, F, C, dims, vertex_cluster, ws, key_hi, key_lo, stream
    faces = [one, V, F, C, dims, one, one, None, one, None]
    for missing in (0, 4, 5, 6, 8):
        assert refused(L.npcd_simplify_faces, faces, **{f"_{missing}": None}) == -1, missing
    assert refused(L.npcd_simplify_faces, faces, _2=0) == -1 and refused(L.npcd_simplify_faces, faces, _1=0) == -1
    assert refused(L.npcd_simplify_faces, faces, _8=ctypes.c_void_p(68)) == -1
    # one packed key cannot hold more than 2^21 cluster ids
    assert refused(L.npcd_simplify_faces, faces, _1=2 ** 21 + 1, _4=ints(1024, 1024, 4)) == -1
    #         order, V, F, C, dims, ws, counts, stream
    unique = [one, V, F, C, dims, one, one, None]
    for missing in (0, 4, 5, 6):
        assert refused(L.npcd_simplify_unique, unique, **{f"_{missing}": None}) == -1, missing
    assert refused(L.npcd_simplify_unique, unique, _2=0) == -1 and refused(L.npcd_simplify_unique, unique, _2=2 ** 31) == -2
    #       V, F, C, origin, cell, dims, ws, V_out, F_out, vertices_out, attributes_out, faces_out, face_source, stream
    emit = [V, F, C, origin, cell, dims, one, 10, 20, one, one, one, one, None]
    for missing in (3, 4, 5, 6, 9, 10, 11, 12):
        assert refused(L.npcd_simplify_emit, emit, **{f"_{missing}": None}) == -1, missing
    assert refused(L.npcd_simplify_emit, emit, _7=0) == -1 and refused(L.npcd_simplify_emit, emit, _7=V + 1) == -1
    assert refused(L.npcd_simplify_emit, emit, _8=F + 1) == -1 and refused(L.npcd_simplify_emit, emit, _8=-1) == -1
    assert refused(L.npcd_simplify_emit, emit, _8=0) == -1          # outputs for faces that do not exist
    assert refused(L.npcd_simplify_emit, emit, _2=0) == -1 and refused(L.npcd_simplify_emit, emit, _2=17) == -2


def test_wrapper_argument_errors():
    from npcd.hip.simplify import simplify_mesh
    v, f = (torch.from_numpy(a) for a in soup(10))
    with pytest.raises(RuntimeError, match="GPU"):
        simplify_mesh(v, f, 0.1)                                                   # not on the GPU: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        simplify_mesh(v, f, 0.1, attributes=torch.zeros(len(v), 3))
    with pytest.raises(ValueError):
        simplify_mesh(v[:, :2], f, 0.1)
    with pytest.raises(ValueError):
        simplify_mesh(v, f.reshape(-1), 0.1)
    with pytest.raises(ValueError):
        simplify_mesh(v.numpy(), f, 0.1)


class _Field:
    """Stands in for a PointNeRF: the density of a sphere on the lattice, the colour a function of the position."""

    def __init__(self):
        self.vol, self.origin, self.spacing = sphere_volume((12, 12, 12), radius=0.6)

    def density_grid(self, coords, feats, resolution=128, bound=None, mlp_dtype=None):
        return (torch.from_numpy(self.vol)[None], torch.tensor(self.origin, dtype=torch.float32), torch.tensor(self.spacing, dtype=torch.float32))

    def query_field(self, coords, feats, x, mlp_dtype=None, view_dir=None):
        return None, 0.5 + 0.5 * torch.sin(5.0 * x)


def test_extract_mesh_with_stand_ins(monkeypatch):
    """extract_mesh(simplify=None) gives what it gave before the option existed -- the isosurface, its normals and colours, untouched --
    and simplify=k hands the right grid and attributes to the simplifier and renormalises the normals."""
    import npcd.hip.isosurface as iso_module
    from npcd.eval.mesh import extract_mesh
    field = _Field()

    def isosurface(volume, level, origin, spacing, normals=False, gradient_of=None):
        v, f = marching_tetrahedra_reference(volume[0].numpy(), level, origin.numpy(), spacing.numpy())
        n = vertex_normals_reference(volume[0].numpy(), level, spacing.numpy())
        return [(torch.from_numpy(v), torch.from_numpy(f)) + ((torch.from_numpy(n),) if normals else ())]
    monkeypatch.setattr(iso_module, "isosurface", isosurface)
    coords, feats = torch.zeros(1, 4, 3), torch.zeros(1, 4, 8)
    v, f = marching_tetrahedra_reference(field.vol, 0.0, np.float32(field.origin), np.float32(field.spacing))
    n = vertex_normals_reference(field.vol, 0.0, np.float32(field.spacing))
    (plain,) = extract_mesh(field, coords, feats, resolution=12, level=0.0, normals=True)
    assert sorted(plain) == ["colors", "faces", "normals", "vertices"]
    assert plain["vertices"].numpy().tobytes() == v.tobytes() and plain["faces"].numpy().tobytes() == f.tobytes()
    assert plain["normals"].numpy().tobytes() == n.tobytes()
    assert plain["colors"].numpy().tobytes() == (0.5 + 0.5 * torch.sin(5.0 * torch.from_numpy(v))).numpy().tobytes()
    (again,) = extract_mesh(field, coords, feats, resolution=12, level=0.0, normals=True, simplify=None)
    assert all(again[k].numpy().tobytes() == plain[k].numpy().tobytes() for k in plain) and sorted(again) == sorted(plain)
    calls = []

    def simplifier(vertices, faces, cell, origin=None, dims=None, attributes=None):
        calls.append((cell, origin, dims, None if attributes is None else tuple(attributes.shape)))
        out = simplify_reference(vertices.numpy(), faces.numpy(), cell, origin, dims, None if attributes is None else attributes.numpy())
        return {k: torch.from_numpy(a) for k, a in out.items()}
    (coarse,) = extract_mesh(field, coords, feats, resolution=12, level=0.0, normals=True, simplify=2, simplifier=simplifier)
    spacing = [float(s) for s in torch.tensor(field.spacing, dtype=torch.float32)]
    assert calls == [([2 * s for s in spacing], [-1.0, -1.0, -1.0], [6, 6, 6], (len(v), 6))]
    assert sorted(coarse) == ["colors", "face_source", "faces", "normals", "vertex_cluster", "vertices"]
    want = simplify_reference(v, f, [2 * s for s in spacing], [-1.0] * 3, [6, 6, 6], np.concatenate([plain["colors"].numpy(), n], axis=1))
    assert coarse["vertices"].numpy().tobytes() == want["vertices"].tobytes() and coarse["faces"].numpy().tobytes() == want["faces"].tobytes()
    assert 0 < len(want["faces"]) < len(f)
    assert coarse["colors"].numpy().tobytes() == want["attributes"][:, :3].tobytes()
    length = torch.linalg.norm(coarse["normals"], dim=1)
    assert ((length - 1).abs() < 1e-6).all() and coarse["normals"].shape == (len(want["vertices"]), 3)
    (bare,) = extract_mesh(field, coords, feats, resolution=12, level=0.0, colors=False, simplify=2.5, simplifier=simplifier)
    assert calls[-1][2] == [5, 5, 5] and calls[-1][3] is None and sorted(bare) == ["face_source", "faces", "vertex_cluster", "vertices"]
    # a mean of zero stays zero
    from npcd.eval.mesh import _simplified
    flat = {"vertices": torch.tensor([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]]), "faces": torch.zeros((0, 3), dtype=torch.int32),
            "normals": torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])}
    assert _simplified(flat, 1.0, [0.0] * 3, [1.0] * 3, (2, 2, 2), simplifier)["normals"].tolist() == [[0.0, 0.0, 0.0]]
    for bad in (0, -1.0, float("nan"), "2"):
        with pytest.raises(ValueError, match="simplify"):
            extract_mesh(field, coords, feats, resolution=12, level=0.0, simplify=bad)
