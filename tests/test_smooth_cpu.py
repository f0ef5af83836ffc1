"""Mesh edges and Taubin smoothing without a GPU: the CPU restatements npcd.eval.mesh.mesh_edges_reference and
smooth_reference against geometry and the exact cases of the specification, not against themselves; the per-lane code of
csrc/smooth.h, the code the kernels run, built for the host with sanitizers (csrc/smooth_host.cpp) and held bit for bit to the
references on the meshes of the GPU test (tests/test_gpu_smooth.py, which imports them from here); the kernels' resources from the
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

from npcd.eval.mesh import (marching_tetrahedra_reference, mesh_edges_reference, mesh_topology, simplify_reference, smooth_reference,
                            topology_from_counts, vertex_normals_reference)
from test_kernel_resources import CSRC, _compile
from test_simplify_cpu import _Field, same_bits

STRIP = 256          # kSmStrip of csrc/smooth.h; test_the_wrapper_knows_the_constants holds it to the source
FACES = (1, 4, 42, 43, 63, 64, 65, 255, 256, 257, 16387)          # 42 and 43 faces: 252 and 258 keys, either side of one strip
EDGE_KEYS = ("row_start", "neighbours", "edges", "edge_faces", "edge_forward", "boundary_vertex", "counts")
CENTRE = np.array([11.4, 11.7, 11.2])


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def soup(F, seed=0):
    """A random triangle soup over so few vertices that edges repeat; every fifth face is a copy of an earlier one, rotated (a
    duplicate) or turned over (a reversed face)."""
    rng = np.random.default_rng(2000 * seed + F)
    V = max(4, min(F, 20000) // 3 + 3)
    v = rng.random((V, 3)).astype(np.float32)
    f = rng.integers(0, V, (F, 3)).astype(np.int32)
    for i in range(4, F, 5):
        f[i] = f[rng.integers(0, i)][[[1, 2, 0], [2, 1, 0], [0, 2, 1]][i % 3]]
    return v, f


@functools.lru_cache(maxsize=None)
def ball(radius=9.3, G=24):
    """The isosurface of radius - |p - CENTRE| on a G^3 lattice of unit spacing: closed at 9.3, open through the six sides at 14.5."""
    z, y, x = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    vol = (radius - np.sqrt((x - CENTRE[0]) ** 2 + (y - CENTRE[1]) ** 2 + (z - CENTRE[2]) ** 2)).astype(np.float32)
    return marching_tetrahedra_reference(vol, 0.0) + (vol,)


def coarse_ball(radius=9.3):
    v, f, _ = ball(radius)
    out = simplify_reference(v, f, 2.0, origin=[0.0, 0.0, 0.0], dims=[12, 12, 12])
    return out["vertices"], out["faces"]


def fan(n=300):
    """n faces round vertex 0, open: a degree above a wave and above a strip, and a rim of boundary vertices."""
    angle = np.linspace(0.0, 1.9 * np.pi, n + 1)
    v = np.concatenate([[[0.05, -0.02, 0.3]], np.stack([np.cos(angle), np.sin(angle), 0.1 * np.sin(5 * angle)], axis=1)]).astype(np.float32)
    f = np.stack([np.zeros(n, dtype=np.int64), np.arange(1, n + 1), np.arange(2, n + 2)], axis=1).astype(np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(vertices, faces, iterations, lam, mu, fixed, fix_boundary): the arguments of one call."""
    kind, _, arg = name.partition(":")
    c = dict(iterations=2, lam=0.5, mu=-0.53, fixed=None, fix_boundary=True)
    rng = np.random.default_rng(len(name) * 11 + 3)
    if kind == "faces":          # wave, workgroup and strip edges of the face and key launches; nothing is pinned, so the soup moves
        c["vertices"], c["faces"] = soup(int(arg))
        c.update(fix_boundary=False)
    elif kind == "fan":
        c["vertices"], c["faces"] = fan()
        c.update(fix_boundary=arg != "free", iterations=3)
    elif kind == "lost":          # 1 % of the vertices have a coordinate that is not finite
        v, f = soup(3000, seed=4)
        bad = rng.choice(len(v), len(v) // 100, replace=False)
        v[bad, rng.integers(0, 3, len(bad))] = np.float32([np.nan, np.inf, -np.inf])[rng.integers(0, 3, len(bad))]
        v[bad[0]] = (np.nan, 1e30, np.inf)          # the finite coordinate of a lost vertex is the largest of the call
        c.update(vertices=v, faces=f, fix_boundary=False)
    elif kind == "bad_indices":          # indices outside [0, V) are not followed; two equal indices make no face
        v, f = soup(200, seed=6)
        f[3], f[50], f[120], f[121], f[150] = (-1, 2, 3), (1, len(v), 2), (1, 2, 2 ** 31 - 1), (-2 ** 31, 0, 1), (7, 7, 9)
        c.update(vertices=v, faces=f, fix_boundary=False)
    elif kind == "no_faces":
        c["vertices"], c["faces"] = soup(40)[0], np.zeros((0, 3), dtype=np.int32)
    elif kind == "no_vertices":
        c["vertices"], c["faces"] = np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32)
    elif kind == "no_valid_faces":
        c["vertices"], c["faces"] = soup(40)[0], np.int32([[0, 0, 1], [5, 99, 2], [-1, 2, 3]])
    elif kind == "ends":          # the only valid faces sit at the first and the last vertices: long runs of empty rows
        v = rng.random((70001, 3)).astype(np.float32)
        c.update(vertices=v, faces=np.int32([[0, 70000, 1], [70000, 0, 69999], [5, 5, 6]]), fix_boundary=False)
    elif kind == "all_zero":          # A = 0: the output is the input, -0 included
        v, f = soup(64)
        c.update(vertices=np.where(rng.random(v.shape) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32), faces=f, fix_boundary=False)
    elif kind in ("ball", "open_ball", "coarse_ball", "coarse_open_ball"):          # n = arg iterations on the 24^3 sphere
        radius = 14.5 if "open" in kind else 9.3
        v, f = coarse_ball(radius) if kind.startswith("coarse") else ball(radius)[:2]
        c.update(vertices=v, faces=f, iterations=int(arg or 2))
    elif kind == "noisy":          # the sphere with noise: what smoothing is for
        v, f, _ = ball()
        c.update(vertices=(v + np.random.default_rng(0).normal(0, 0.15, v.shape)).astype(np.float32), faces=f, iterations=10)
        if arg == "laplace":
            c.update(mu=0.0)
        elif arg == "pinned":
            c.update(fixed=np.random.default_rng(5).random(len(v)) < 0.3, lam=0.33, mu=-0.34)
    elif kind == "far":          # coordinates of 2^100 and of 2^-100: the lattice follows the exponent
        v, f, _ = ball()
        c.update(vertices=(v * np.float32(2.0) ** int(arg)).astype(np.float32), faces=f, iterations=1)
    else:
        raise KeyError(name)
    return c


CASES = ([f"faces:{F}" for F in FACES] +
         ["fan:pinned", "fan:free", "lost", "bad_indices", "no_faces", "no_vertices", "no_valid_faces", "ends", "all_zero", "ball:0", "ball:1",
          "ball:2", "ball:10", "open_ball:2", "coarse_ball:2", "coarse_open_ball:2", "noisy", "noisy:laplace", "noisy:pinned", "far:100",
          "far:-100"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The edges of a case, plus "vertices" and "state" after its smoothing."""
    c = case(name)
    out = dict(mesh_edges_reference(len(c["vertices"]), c["faces"]))
    out["vertices"], out["state"], _ = smooth_reference(c["vertices"], c["faces"], c["iterations"], c["lam"], c["mu"], c["fixed"], c["fix_boundary"])
    return out


def hold(got, name, what, keys=EDGE_KEYS + ("vertices",)):
    """got: key -> array; every output named equals the reference's, bit for bit."""
    want = reference(name)
    assert set(keys) <= set(got), (what, sorted(got))
    for key in keys:
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        if g.dtype.itemsize == 1:
            assert g.dtype == w.dtype and np.array_equal(g, w), f"{what}: {key}"
        else:
            same_bits(g, w, f"{what}: {key}")


# ---- the edges against geometry ----------------------------------------------------------------------------------------------------------
def test_the_sphere_is_a_closed_surface():
    v, f, _ = ball()
    assert (len(v), len(f)) == (4850, 9696)
    e = mesh_edges_reference(len(v), f)
    t = mesh_topology(len(v), f)
    assert t == topology_from_counts(e["counts"])
    assert t == {"edges": 14544, "valid_faces": 9696, "used_vertices": 4850, "boundary_edges": 0, "nonmanifold_edges": 0,
                 "misoriented_edges": 0, "euler_characteristic": 2, "closed": True}
    assert int(np.diff(e["row_start"]).max()) == 10
    assert (e["edge_faces"] == 2).all() and (e["edge_forward"] == 1).all() and not e["boundary_vertex"].any()
    # the adjacency is symmetric, and a vertex's neighbours ascend without repeating
    source = np.repeat(np.arange(len(v)), np.diff(e["row_start"]))
    pairs = set(zip(source.tolist(), e["neighbours"].tolist()))
    assert len(pairs) == len(source) == 2 * 14544 and all((b, a) in pairs for a, b in pairs)
    same_row = np.diff(source) == 0
    assert (np.diff(e["neighbours"].astype(np.int64))[same_row] > 0).all()
    assert (e["edges"][:, 0] < e["edges"][:, 1]).all()
    # every edge is an edge of some face, and every face's edges are there
    of_faces = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    assert np.array_equal(np.unique(of_faces, axis=0), e["edges"])


def test_the_coarse_sphere_stays_closed_and_the_large_one_is_open():
    v, f = coarse_ball()
    assert (len(v), len(f)) == (406, 808)
    t = mesh_topology(len(v), f)
    assert t["closed"] and t["euler_characteristic"] == 2 and t["misoriented_edges"] == 0
    v, f, _ = ball(14.5)
    t = mesh_topology(len(v), f)
    assert (t["boundary_edges"], t["nonmanifold_edges"], t["misoriented_edges"], t["euler_characteristic"], t["closed"]) == (720, 0, 0, -4, False)
    e = mesh_edges_reference(len(v), f)
    on_a_side = ((v == 0) | (v == 23)).any(axis=1)
    assert np.array_equal(e["boundary_vertex"].astype(bool), on_a_side)


def test_exact_cases_of_the_edges():
    # two triangles sharing the edge (0, 1), wound alike: both traverse it as 0 -> 1
    e = mesh_edges_reference(4, np.int32([[0, 1, 2], [0, 1, 3]]))
    assert e["edges"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3]]
    assert e["edge_faces"].tolist() == [2, 1, 1, 1, 1] and e["edge_forward"].tolist() == [2, 0, 0, 1, 1]
    assert e["counts"].tolist() == [10, 2, 4, 4, 0, 1]
    assert e["row_start"].tolist() == [0, 3, 6, 8, 10] and e["neighbours"].tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 0, 1]
    # wound against each other across the edge: consistent
    e = mesh_edges_reference(4, np.int32([[0, 1, 2], [1, 0, 3]]))
    assert e["counts"].tolist() == [10, 2, 4, 4, 0, 0] and e["edge_forward"][0] == 1
    # three faces on one edge
    e = mesh_edges_reference(5, np.int32([[0, 1, 2], [1, 0, 3], [0, 1, 4]]))
    assert e["counts"].tolist() == [14, 3, 5, 6, 1, 0] and e["edge_faces"][0] == 3 and e["edge_forward"][0] == 2
    assert e["boundary_vertex"].tolist() == [1, 1, 1, 1, 1]
    # invalid and degenerate faces contribute nothing, isolated vertices have empty rows
    e = mesh_edges_reference(9, np.int32([[0, 0, 1], [2, 9, 3], [-1, 2, 3], [4, 6, 7], [3, 3, 3]]))
    assert e["counts"].tolist() == [6, 1, 3, 3, 0, 0] and e["edges"].tolist() == [[4, 6], [4, 7], [6, 7]]
    assert e["row_start"].tolist() == [0, 0, 0, 0, 0, 2, 2, 4, 6, 6] and e["boundary_vertex"].tolist() == [0, 0, 0, 0, 1, 0, 1, 1, 0]
    # a tetrahedron: closed, characteristic 2
    t = mesh_topology(4, np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]]))
    assert t["closed"] and t["euler_characteristic"] == 2 and t["misoriented_edges"] == 0 and t["edges"] == 6
    # nothing at all
    for V, faces in ((0, np.zeros((0, 3), np.int32)), (5, np.zeros((0, 3), np.int32)), (0, np.int32([[0, 1, 2]]))):
        e = mesh_edges_reference(V, faces)
        assert e["counts"].tolist() == [0] * 6 and e["row_start"].tolist() == [0] * (V + 1) and e["edges"].shape == (0, 2)
        assert e["neighbours"].shape == (0,) and e["boundary_vertex"].shape == (V,) and e["edge_faces"].dtype == np.int32
    assert mesh_topology(0, np.zeros((0, 3), np.int32)) == {"edges": 0, "valid_faces": 0, "used_vertices": 0, "boundary_edges": 0,
                                                           "nonmanifold_edges": 0, "misoriented_edges": 0, "euler_characteristic": 0, "closed": True}
    with pytest.raises(ValueError, match=rf"{2 ** 31} vertices and 1 faces"):
        mesh_edges_reference(2 ** 31, np.int32([[0, 1, 2]]))
    with pytest.raises(ValueError, match="6 counts"):
        topology_from_counts([1, 2, 3])


def test_outputs_of_the_references():
    for name in CASES:
        c, out = case(name), reference(name)
        V = len(c["vertices"])
        D = int(out["counts"][0])
        assert D % 2 == 0 and out["row_start"].shape == (V + 1,) and out["neighbours"].shape == (D,) and out["edges"].shape == (D // 2, 2)
        assert out["row_start"][0] == 0 and out["row_start"][-1] == D and (np.diff(out["row_start"]) >= 0).all()
        assert int(out["edge_faces"].sum()) == 3 * int(out["counts"][1])          # every valid face holds three edges
        assert out["vertices"].dtype == np.float32 and out["vertices"].shape == (V, 3) and out["state"].dtype == np.int32
        if name.startswith("faces:") and len(c["faces"]) >= 42:
            assert (out["edge_faces"] >= 3).any() and (out["edge_faces"] == 1).any(), name          # edges repeat
            assert (out["vertices"] != c["vertices"]).any(), name                                   # and something moves


# ---- the smoothing against geometry --------------------------------------------------------------------------------------------------------
def quantum_of(e):
    return 2.0 ** (e - 29)


@pytest.mark.parametrize("lam", [0.6, 0.5, 1.0])
def test_one_step_on_a_tetrahedron(lam):
    """Every vertex of a tetrahedron has the three others as neighbours: one step takes it to c + (1 - 4 lam / 3)(x - c), c the
    centroid.  On the lattice the quantisation of the vertex, that of its neighbours' mean and the step's own rint add up to one
    quantum; the fp32 output adds half an fp32 ulp."""
    v = (0.1 + 0.7 * np.concatenate([np.eye(3), np.zeros((1, 3))])).astype(np.float32)
    f = np.int32([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    out, state, e = smooth_reference(v, f, 1, lam, 0.0)
    assert e == -1 and state.dtype == np.int32 and np.abs(state).max() <= 2 ** 30          # A = 0.8
    x = v.astype(np.float64)
    want = x.mean(axis=0) + (1 - 4 * lam / 3) * (x - x.mean(axis=0))
    on_lattice = np.abs(state * quantum_of(e) - want).max() / quantum_of(e)
    of_output = np.abs(out.astype(np.float64) - want)
    print(f"lam {lam}: the lattice is {on_lattice:.3f} quanta off, the output {of_output.max() / quantum_of(e):.2f} quanta")
    assert on_lattice <= 1.0
    assert (of_output <= quantum_of(e) + 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).all()


def test_a_vertex_at_the_mean_of_its_neighbours_stays():
    ring = np.stack([np.cos(np.arange(6) * np.pi / 3), np.sin(np.arange(6) * np.pi / 3), np.full(6, 0.25)], axis=1)
    v = np.concatenate([ring.mean(axis=0, keepdims=True), ring]).astype(np.float32)
    f = np.int32([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)])
    for n, lam, mu in ((1, 0.5, 0.0), (1, 1.0, 0.0), (7, 0.5, -0.53)):
        out, state, e = smooth_reference(v, f, n, lam, mu)
        start = smooth_reference(v, f, 0, lam, mu)[1]
        assert np.abs(state[0].astype(np.int64) - start[0]).max() <= 1, (n, lam, mu)
        assert np.array_equal(state[1:], start[1:]) and out[1:].tobytes() == v[1:].tobytes()          # the rim is the boundary


def test_the_noisy_sphere_gets_smooth_and_keeps_its_size():
    c = case("noisy")
    v = c["vertices"]
    radius = lambda p: np.linalg.norm(p.astype(np.float64) - CENTRE, axis=1)
    before = radius(v)
    taubin = radius(reference("noisy")["vertices"])
    laplace = radius(reference("noisy:laplace")["vertices"])
    print(f"std r {before.std():.4f} -> {taubin.std():.4f} (Taubin), {laplace.std():.4f} (Laplacian); mean r {before.mean():.4f} -> "
          f"{taubin.mean():.4f}, {laplace.mean():.4f}")
    assert abs(before.std() - 0.1493) < 5e-4 and abs(before.mean() - 9.2972) < 5e-4          # the mesh the thresholds were set on
    assert taubin.std() < 0.5 * before.std()
    assert abs(taubin.mean() - before.mean()) < 0.005
    assert before.mean() - laplace.mean() > 0.05


def test_vertices_that_stand_still_return_their_bits():
    c = case("noisy:pinned")
    out = reference("noisy:pinned")["vertices"]
    pinned = c["fixed"]
    assert pinned.any() and not pinned.all()
    assert out[pinned].tobytes() == c["vertices"][pinned].tobytes() and (out[~pinned] != c["vertices"][~pinned]).any(axis=1).all()
    # iterations = 0: the input, whatever else is asked
    for name in ("ball:0", "lost"):
        k = case(name)
        assert smooth_reference(k["vertices"], k["faces"], 0)[0].tobytes() == k["vertices"].tobytes()
    # lost vertices keep their bits, NaN payloads included, and are no one's neighbour
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, 0.25, 5.0]])
    v[3, 1] = np.uint32(0x7fc12345).view(np.float32)
    f = np.int32([[0, 1, 2], [0, 1, 3], [1, 2, 3], [2, 0, 3]])
    out, state, e = smooth_reference(v, f, 1, 0.5, 0.0)
    assert out[3].tobytes() == v[3].tobytes() and e == 2 and state[3].tolist() == [0, 0, 0]          # A = 5: the finite coordinate counts
    assert out[:3].tolist() == [[0.25, 0.25, 0], [0.5, 0.25, 0], [0.25, 0.5, 0]]          # the means of the two others, not of three
    # boundary vertices: an open mesh moves only inside, unless asked otherwise
    k = case("open_ball:2")
    edges = mesh_edges_reference(len(k["vertices"]), k["faces"])
    rim = edges["boundary_vertex"].astype(bool)
    out = reference("open_ball:2")["vertices"]
    assert rim.sum() == 720 and out[rim].tobytes() == k["vertices"][rim].tobytes() and (out[~rim] != k["vertices"][~rim]).any()
    free = smooth_reference(k["vertices"], k["faces"], 2, fix_boundary=False)[0]
    assert (free[rim] != k["vertices"][rim]).any(axis=1).all()
    # isolated vertices and a mesh without faces
    k = case("ends")
    out = reference("ends")["vertices"]
    assert out[2:69999].tobytes() == k["vertices"][2:69999].tobytes() and (out[[0, 1, 69999, 70000]] != k["vertices"][[0, 1, 69999, 70000]]).any(axis=1).all()
    assert reference("no_faces")["vertices"].tobytes() == case("no_faces")["vertices"].tobytes()
    # A = 0
    assert reference("all_zero")["vertices"].tobytes() == case("all_zero")["vertices"].tobytes() and np.signbit(case("all_zero")["vertices"]).any()


def test_the_lattice_follows_the_exponent():
    """Scaling every coordinate by a power of two scales the output by it, bit for bit: the lattice is the same integers."""
    base = smooth_reference(*ball()[:2], 1)
    for power in (100, -100):
        c = case(f"far:{power}")
        out, state, e = smooth_reference(c["vertices"], c["faces"], 1)
        assert e == base[2] + power and np.array_equal(state, base[1])
        assert out.tobytes() == (base[0] * np.float32(2.0) ** power).astype(np.float32).tobytes()


def test_the_references_refuse():
    v, f = soup(10)
    for bad in (dict(iterations=-1), dict(iterations=1001), dict(lam=0.0), dict(lam=1.5), dict(mu=0.1), dict(mu=-1.5), dict(lam=float("nan"))):
        with pytest.raises(ValueError):
            smooth_reference(v, f, **bad)
    with pytest.raises(ValueError, match="fixed"):
        smooth_reference(v, f, fixed=np.zeros(3, dtype=bool))
    with pytest.raises(ValueError, match="integers"):
        mesh_edges_reference(5, np.float32([[0, 1, 2]]))


# ---- the per-lane code on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/smooth_host.cpp, the per-lane functions of csrc/smooth.h as plain loops, built with the host compiler, its address and
    undefined-behaviour sanitizers and without FMA contraction: a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("smooth_host") / "smooth_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CSRC, "smooth_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_on_the_host(program, tmp_path, name, reverse):
    c = case(name)
    V, F = len(c["vertices"]), len(c["faces"])
    flags = (1 if c["fixed"] is not None else 0) | (2 if c["fix_boundary"] else 0)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([V, F, c["iterations"], flags], dtype="<i4").tobytes() + np.array([c["lam"], c["mu"]], dtype="<f8").tobytes())
        fh.write(np.ascontiguousarray(c["vertices"]).tobytes() + np.ascontiguousarray(c["faces"]).tobytes())
        if c["fixed"] is not None:
            fh.write(c["fixed"].astype(np.uint8).tobytes())
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + (["reverse"] if reverse else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    counts = np.frombuffer(raw, dtype="<i8", count=6)
    D = int(counts[0])
    out, at_byte = {"counts": counts}, 48
    for key, dtype, shape in (("row_start", "<i4", (V + 1,)), ("neighbours", "<i4", (D,)), ("edges", "<i4", (D // 2, 2)),
                              ("edge_faces", "<i4", (D // 2,)), ("edge_forward", "<i4", (D // 2,)), ("boundary_vertex", "u1", (V,)),
                              ("vertices", "<f4", (V, 3)), ("state", "<i4", (V, 3))):
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype=dtype, count=count, offset=at_byte).reshape(shape)
        at_byte += count * np.dtype(dtype).itemsize
    assert at_byte == len(raw)
    return out


@pytest.mark.parametrize("name", CASES)
def test_the_lanes_on_the_host(host_program, tmp_path, name):
    for reverse in (False, True):
        hold(run_on_the_host(host_program, tmp_path, name, reverse), name, f"{name} reverse {reverse}", EDGE_KEYS + ("vertices", "state"))


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_knows_the_constants():
    from npcd import hip
    from npcd.eval import mesh
    from npcd.hip import smooth
    source = open(f"{CSRC}/smooth.h").read()
    assert int(re.search(r"constexpr int kSmStrip = (\d+);", source).group(1)) == smooth.STRIP_KEYS == STRIP
    assert int(re.search(r"constexpr int kSmThreads = (\d+);", source).group(1)) == STRIP          # one entry of a strip per lane
    assert int(re.search(r"constexpr int kSmMaxIterations = (\d+);", source).group(1)) == smooth.MAX_ITERATIONS == 1000
    assert "kSmMaxVertices = (int64_t)1 << 31" in source and smooth.MAX_VERTICES == mesh.MAX_EDGE_VERTICES == 2 ** 31
    assert "kSmMaxFaces = (int64_t)1 << 28" in source and smooth.MAX_FACES == mesh.MAX_EDGE_FACES == 2 ** 28
    assert hip.smooth_mesh is smooth.smooth_mesh and hip.mesh_edges is smooth.mesh_edges
    assert smooth.EDGE_KEYS == EDGE_KEYS and len(mesh.COUNT_NAMES) == 6


def test_kernels_use_no_scratch_and_the_step_no_atomics(tmp_path):
    kernels = _compile("smooth.hip", str(tmp_path / "smooth.s"))
    assert len(kernels) == 9, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 64, (name, k)
        # the four wave totals of a workgroup's scan (csrc/block_scan.h); the totals launch takes its carry from the scan's total
        want = 32 if ("sm_totals" in name or "sm_marks" in name or "sm_emit" in name or "sm_counts" in name) else 0
        assert k["lds"] == want, (name, k)
    # the body of the step kernel, from its label to the end of the function: a gather, no atomic instruction at all
    (step,) = [name for name in kernels if "sm_step_kernel" in name]
    text = open(tmp_path / "smooth.s").read()
    body = text.split(f"\n{step}:", 1)[1].split(".Lfunc_end", 1)[0]
    assert "s_endpgm" in body and "global_load" in body and "atomic" not in body


def test_header_exports_and_signatures():
    from npcd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "npcd_hip.h")).read()
    L = hip.lib()
    names = ("npcd_mesh_edges_ws_bytes", "npcd_mesh_edges_keys", "npcd_mesh_edges_unique", "npcd_mesh_edges_emit", "npcd_smooth_ws_bytes",
             "npcd_smooth_mesh")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in hip.SIGNATURES and hasattr(L, name), name
    assert L.npcd_missing == () and L.npcd_abi_version() == 10
    assert hip.SIGNATURES["npcd_mesh_edges_ws_bytes"][0] is ctypes.c_int64 and hip.SIGNATURES["npcd_smooth_ws_bytes"][0] is ctypes.c_int64
    assert [len(hip.SIGNATURES[n][1]) for n in names] == [2, 5, 6, 13, 1, 13]
    # the host-side refusals, which look at no pointer's target and launch nothing
    V, F = 1000, 3000
    assert L.npcd_mesh_edges_ws_bytes(V, F) == 16 * 71 + 4 * 6 * F          # 18,000 keys: 71 strips
    assert L.npcd_mesh_edges_ws_bytes(0, 0) == 0 and L.npcd_mesh_edges_ws_bytes(5, 43) == 16 * 2 + 4 * 258
    assert L.npcd_mesh_edges_ws_bytes(-1, F) == -1 and L.npcd_mesh_edges_ws_bytes(V, -1) == -1
    assert L.npcd_mesh_edges_ws_bytes(2 ** 31, F) == -2 and L.npcd_mesh_edges_ws_bytes(V, 2 ** 28) == -2
    assert L.npcd_mesh_edges_ws_bytes(2 ** 31 - 1, 2 ** 28 - 1) > 0
    assert L.npcd_smooth_ws_bytes(V) == 16 + 2 * 16 * V and L.npcd_smooth_ws_bytes(-1) == -1 and L.npcd_smooth_ws_bytes(2 ** 31) == -2
    one = ctypes.c_void_p(64)          # never followed: every call below is refused before a launch

    def refused(fn, args, **changed):
        a = list(args)
        for i, value in changed.items():
            a[int(i[1:])] = value
        return fn(*a)
    #       faces, V, F, keys, stream
    keys = [one, V, F, one, None]
    for missing in (0, 3):
        assert refused(L.npcd_mesh_edges_keys, keys, **{f"_{missing}": None}) == -1, missing
    assert refused(L.npcd_mesh_edges_keys, keys, _2=0) == -1 and refused(L.npcd_mesh_edges_keys, keys, _3=ctypes.c_void_p(68)) == -1
    assert refused(L.npcd_mesh_edges_keys, keys, _1=2 ** 31) == -2 and refused(L.npcd_mesh_edges_keys, keys, _2=2 ** 28) == -2
    #         sorted_keys, V, F, ws, counts, stream
    unique = [one, V, F, one, one, None]
    for missing in (0, 3, 4):
        assert refused(L.npcd_mesh_edges_unique, unique, **{f"_{missing}": None}) == -1, missing
    assert refused(L.npcd_mesh_edges_unique, unique, _2=0) == -1 and refused(L.npcd_mesh_edges_unique, unique, _2=2 ** 28) == -2
    assert refused(L.npcd_mesh_edges_unique, unique, _3=ctypes.c_void_p(68)) == -1 and refused(L.npcd_mesh_edges_unique, unique, _4=ctypes.c_void_p(68)) == -1
    #       sorted_keys, V, F, ws, D, row_start, neighbours, edges, edge_faces, edge_forward, boundary_vertex, counts, stream
    emit = [one, V, F, one, 100, one, one, one, one, one, one, one, None]
    for missing in (0, 3, 5, 6, 7, 8, 9, 10, 11):
        assert refused(L.npcd_mesh_edges_emit, emit, **{f"_{missing}": None}) == -1, missing
    for D in (0, -2, 101, 6 * F + 2):
        assert refused(L.npcd_mesh_edges_emit, emit, _4=D) == -1, D
    assert refused(L.npcd_mesh_edges_emit, emit, _1=0) == -1 and refused(L.npcd_mesh_edges_emit, emit, _2=0) == -1
    assert refused(L.npcd_mesh_edges_emit, emit, _5=ctypes.c_void_p(66)) == -1 and refused(L.npcd_mesh_edges_emit, emit, _1=2 ** 31) == -2
    #         vertices, V, row_start, neighbours, D, boundary_vertex, fixed, iterations, lam, mu, ws, vertices_out, stream
    smooth = [one, V, one, one, 100, one, one, 10, 0.5, -0.53, one, one, None]
    for missing in (0, 2, 3, 10, 11):
        assert refused(L.npcd_smooth_mesh, smooth, **{f"_{missing}": None}) == -1, missing
    for slot, bad in ((7, -1), (7, 1001), (8, 0.0), (8, 1.25), (8, float("nan")), (9, 0.25), (9, -1.25), (9, float("nan")), (4, -1), (1, 0)):
        assert refused(L.npcd_smooth_mesh, smooth, **{f"_{slot}": bad}) == -1, (slot, bad)
    assert refused(L.npcd_smooth_mesh, smooth, _10=ctypes.c_void_p(72)) == -1          # the workspace: 16-byte aligned
    assert refused(L.npcd_smooth_mesh, smooth, _1=2 ** 31) == -2


def test_wrapper_argument_errors():
    from npcd.hip.smooth import mesh_edges, smooth_mesh
    v, f = (torch.from_numpy(a) for a in soup(10))
    with pytest.raises(RuntimeError, match="GPU"):
        mesh_edges(len(v), f)                                                      # not on the GPU: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        smooth_mesh(v, f)
    with pytest.raises(RuntimeError, match="GPU"):
        mesh_topology(len(v), f)                                                   # a tensor goes to the kernels
    with pytest.raises(ValueError):
        mesh_edges(len(v), f.reshape(-1))
    with pytest.raises(ValueError):
        mesh_edges(len(v), f.numpy())
    with pytest.raises(ValueError):
        mesh_edges(-1, f)
    with pytest.raises(ValueError, match=rf"{2 ** 31} vertices and 10 faces"):
        mesh_edges(2 ** 31, f)
    with pytest.raises(ValueError, match=rf"{2 ** 28} faces"):
        mesh_edges(5, torch.zeros(1, 3, dtype=torch.int32).expand(2 ** 28, 3))
    with pytest.raises(ValueError):
        smooth_mesh(v[:, :2], f)
    with pytest.raises(ValueError):
        smooth_mesh(v.numpy(), f)
    for bad in (dict(iterations=-1), dict(iterations=1001), dict(iterations=2.0), dict(iterations=True), dict(lam=0.0), dict(lam=1.5),
                dict(mu=0.1), dict(mu=-1.5), dict(fixed=torch.zeros(3, dtype=torch.bool)), dict(edges={"row_start": f}),
                dict(edges={k: torch.zeros(3, dtype=torch.int32) for k in EDGE_KEYS})):
        with pytest.raises(ValueError):
            smooth_mesh(v, f, **bad)


def test_extract_mesh_with_stand_ins(monkeypatch):
    """extract_mesh with smooth=None and topology=False gives what it gave before the options existed; smooth=n hands the final
    mesh and the factors to the smoother, after the simplifier, and only the vertices change; topology=True describes the final mesh."""
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
    common = dict(resolution=12, level=0.0, normals=True)
    (plain,) = extract_mesh(field, coords, feats, **common)
    assert sorted(plain) == ["colors", "faces", "normals", "vertices"]
    assert plain["vertices"].numpy().tobytes() == v.tobytes() and plain["faces"].numpy().tobytes() == f.tobytes()
    assert plain["normals"].numpy().tobytes() == n.tobytes()
    (again,) = extract_mesh(field, coords, feats, smooth=None, smooth_lambda=0.9, smooth_mu=-0.1, topology=False, **common)
    assert all(again[k].numpy().tobytes() == plain[k].numpy().tobytes() for k in plain) and sorted(again) == sorted(plain)
    calls = []

    def smoother(vertices, faces, iterations=10, lam=0.5, mu=-0.53, edges=None):
        calls.append((tuple(vertices.shape), tuple(faces.shape), iterations, lam, mu, edges))
        return torch.from_numpy(smooth_reference(vertices.numpy(), faces.numpy(), iterations, lam, mu)[0])
    (smooth,) = extract_mesh(field, coords, feats, smooth=5, topology=True, smoother=smoother, **common)
    assert calls == [((len(v), 3), (len(f), 3), 5, 0.5, -0.53, None)]
    assert sorted(smooth) == ["colors", "faces", "normals", "topology", "vertices"]
    assert smooth["vertices"].numpy().tobytes() == smooth_reference(v, f, 5)[0].tobytes() != v.tobytes()
    for key in ("faces", "normals", "colors"):          # carried along unchanged: the normals are those of the unsmoothed surface
        assert smooth[key].numpy().tobytes() == plain[key].numpy().tobytes()
    assert smooth["topology"] == mesh_topology(len(v), f) and smooth["topology"]["closed"] and smooth["topology"]["euler_characteristic"] == 2

    def simplifier(vertices, faces, cell, origin=None, dims=None, attributes=None):
        out = simplify_reference(vertices.numpy(), faces.numpy(), cell, origin, dims, None if attributes is None else attributes.numpy())
        return {k: torch.from_numpy(a) for k, a in out.items()}
    (coarse,) = extract_mesh(field, coords, feats, simplify=2, simplifier=simplifier, **common)
    (both,) = extract_mesh(field, coords, feats, simplify=2, simplifier=simplifier, smooth=3, smooth_lambda=0.4, smooth_mu=0.0, topology=True,
                           smoother=smoother, **common)
    assert calls[-1] == (tuple(coarse["vertices"].shape), tuple(coarse["faces"].shape), 3, 0.4, 0.0, None)          # smoothing runs last
    want = smooth_reference(coarse["vertices"].numpy(), coarse["faces"].numpy(), 3, 0.4, 0.0)[0]
    assert both["vertices"].numpy().tobytes() == want.tobytes()
    assert all(both[k].numpy().tobytes() == coarse[k].numpy().tobytes() for k in coarse if k != "vertices")
    assert both["topology"] == mesh_topology(len(want), coarse["faces"].numpy())
    (only,) = extract_mesh(field, coords, feats, topology=True, smoother=smoother, **common)
    assert only["vertices"].numpy().tobytes() == v.tobytes() and only["topology"] == smooth["topology"] and len(calls) == 2
    for bad in (dict(smooth=-1), dict(smooth=1001), dict(smooth=2.5), dict(smooth=True), dict(smooth=1, smooth_lambda=0.0),
                dict(smooth=1, smooth_mu=0.5)):
        with pytest.raises(ValueError, match="smooth"):
            extract_mesh(field, coords, feats, resolution=12, level=0.0, **bad)
