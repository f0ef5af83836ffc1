"""Point-to-mesh distance without a GPU: the CPU restatement npcd.eval.mesh.point_mesh_distance_reference against
geometry and the exact cases of the specification, and against the same algorithm in float64; the per-lane code of
csrc/mesh_distance.h, the code the kernels run, built for the host with sanitizers (csrc/mesh_distance_host.cpp) and held bit for bit to
the reference on the cases of the GPU test (tests/test_gpu_mesh_distance.py, which imports them from here), with the box bound checked
against every rounded distance, and the tiles that waves of 64 points evaluate held to a table; the kernels' resources from the
compiler's own output, the entry points' refusals, the wrapper's argument errors, and mesh_deviation, cloud_mesh_distance and extract_mesh(deviation=) with stand-ins."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from npcd.eval.mesh import (closest_on_triangles, cloud_mesh_distance, marching_tetrahedra_reference, mesh_deviation,
                            point_mesh_distance_reference, simplify_reference, smooth_reference, surface_sample_reference,
                            vertex_normals_reference)
from test_kernel_resources import CSRC, _compile
from test_simplify_cpu import _Field, same_bits
from test_smooth_cpu import ball, coarse_ball, soup

TILE, WAVE = 256, 64          # kMdTile of csrc/mesh_tiles.h and kMdThreads of csrc/mesh_distance.h; test_the_wrapper_knows_the_constants holds them
FACES = (1, 255, 256, 257, 513, 16387)          # one below, at and above a tile, two tiles and one face, 65 tiles
POINTS = (1, 63, 64, 65, 257, 1024)             # one below, at and above a wave, five waves, sixteen
KEYS = ("sqdist", "face", "closest")
# the largest |sqrt(sqdist) - d64| in ulp of the largest |coordinate| that test_reference_against_float64 saw was 29.523 (the sphere)
# and 6.778 (the sphere shifted by +100), both at the centroid of a thin face; 0.693 on surface samples, 0.655 near the vertices.  Four
# times the largest, rounded up to a power of two
K_ULP = 128.0
# how far a sample of sample_surface lies from its own face, in ulp of the largest |coordinate| A.  p = (b0 v0 + b1 v1) + b2 v2 per
# coordinate: b0 = fl(1 - s), b1 = fl(s fl(1 - u2)) and b2 = fl(s u2) sum to 1 within 2^-25 + 2 2^-24 b1 + 2^-24 b2 <= 2.5 2^-24 (the
# rounding of s itself cancels), which moves a coordinate by less than 2.5 ulp(A) since A 2^-24 < ulp(A); the three products and the
# two sums, none above A, round by half an ulp(A) each, 2.5 more.  5 ulp(A) per coordinate, 5 sqrt(3) in the norm.  A sample's distance
# to its own mesh as the kernel computes it is therefore at most (SAMPLE_ULP + K_ULP) ulp(A): what "0" means for a sampled surface
SAMPLE_ULP = 5.0 * 3.0 ** 0.5
TRIANGLE = np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0]])


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def queries(v, f, S, seed):
    """S query points of a mesh in four kinds, interleaved: samples of its surface (sqdist near 0, where culling is most at risk), its
    vertices themselves, random points in its box and points far outside it."""
    rng = np.random.default_rng(seed)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    good = f[ok] if ok.any() else np.zeros((1, 3), dtype=np.int64)
    vv = v if len(v) else np.zeros((1, 3), dtype=np.float32)
    finite = vv[np.isfinite(vv).all(axis=1)]
    lo, hi = (finite.min(axis=0), finite.max(axis=0)) if len(finite) else (np.zeros(3, np.float32), np.ones(3, np.float32))
    size = np.maximum(hi - lo, np.float32(1e-30))
    b = rng.dirichlet((1.0, 1.0, 1.0), S).astype(np.float32)
    tri = vv[good[rng.integers(0, len(good), S)] % len(vv)]
    with np.errstate(all="ignore"):
        on_surface = (b[:, :1] * tri[:, 0] + b[:, 1:2] * tri[:, 1]) + b[:, 2:] * tri[:, 2]
        corners = vv[rng.integers(0, len(vv), S)]
        in_box = lo + rng.random((S, 3)).astype(np.float32) * size
        far = lo + (rng.random((S, 3)).astype(np.float32) * 40 - 20) * size
    kind = np.arange(S) % 4
    return np.where((kind == 0)[:, None], on_surface, np.where((kind == 1)[:, None], corners, np.where((kind == 2)[:, None], in_box, far))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (points [S, 3] float32, vertices [V, 3] float32, faces [F, 3] int32)."""
    kind, _, arg = name.partition(":")
    rng = np.random.default_rng(len(name) * 13 + 5)
    if kind == "soup":          # F x S: tile and wave edges
        F, S = (int(x) for x in arg.split("x"))
        v, f = soup(F, seed=2)
        return queries(v, f, S, F + S), v, f
    if kind in ("ball", "coarse_ball"):          # the 24^3 sphere, plain and simplified: arg is a shift or a power of two
        v, f = coarse_ball() if kind == "coarse_ball" else ball()[:2]
        if arg.startswith("+"):
            v = (v + np.float32(arg[1:])).astype(np.float32)
        elif arg.startswith("*"):
            v = (v * np.float32(2.0) ** int(arg[1:])).astype(np.float32)
        return queries(v, f, 257, 7), v, f.astype(np.int32)
    if kind == "duplicates":          # the faces of the first tile again in the third and the fifth: the lowest index wins
        v, f = soup(256, seed=3)
        f = np.concatenate([f, soup(256, seed=4)[1] % len(v), f[::-1], soup(256, seed=5)[1] % len(v), f]).astype(np.int32)
        return queries(v, f[:256], 257, 9), v, f
    if kind == "bad_indices":
        v, f = soup(600, seed=6)
        f = f.copy()
        f[3], f[50], f[300], f[301], f[599] = (-1, 2, 3), (1, len(v), 2), (1, 2, 2 ** 31 - 1), (-2 ** 31, 0, 1), (0, 1, -5)
        return queries(v, f, 257, 10), v, f
    if kind == "lost":          # 1 % of the vertices have a coordinate that is not finite
        v, f = soup(3000, seed=4)
        v = v.copy()
        bad = rng.choice(len(v), len(v) // 100, replace=False)
        v[bad, rng.integers(0, 3, len(bad))] = np.float32([np.nan, np.inf, -np.inf])[rng.integers(0, 3, len(bad))]
        return queries(v, f, 257, 11), v, f
    if kind == "nan_points":
        v, f = soup(513, seed=7)
        p = queries(v, f, 130, 12)
        rows = np.arange(0, len(p), 3)
        p[rows, rng.integers(0, 3, len(rows))] = np.nan
        p[1] = (np.inf, 0.5, 0.5)
        return p, v, f
    if kind == "all_invalid":          # 300 faces, none with three indices inside [0, V)
        v = soup(40)[0]
        f = rng.integers(0, len(v), (300, 3)).astype(np.int32)
        f[np.arange(300), rng.integers(0, 3, 300)] = np.where(rng.random(300) < 0.5, -1 - rng.integers(0, 9, 300), len(v) + rng.integers(0, 9, 300))
        return queries(v, f, 65, 13), v, f
    if kind == "no_vertices":
        return rng.random((5, 3)).astype(np.float32), np.zeros((0, 3), np.float32), np.int32([[0, 1, 2], [0, 0, 0]])
    if kind == "no_faces":
        return rng.random((65, 3)).astype(np.float32), soup(40)[0], np.zeros((0, 3), np.int32)
    if kind == "no_points":
        v, f = soup(300)
        return np.zeros((0, 3), np.float32), v, f
    if kind == "needles":          # zero-area faces (two or three equal corners) among ordinary ones
        v, f = soup(257, seed=8)
        f = f.copy()
        f[::3, 1] = f[::3, 0]
        f[1::9, 2] = f[1::9, 1] = f[1::9, 0]
        return queries(v, f, 257, 14), v, f
    raise KeyError(name)


CASES = ([f"soup:{F}x257" for F in FACES] + [f"soup:513x{S}" for S in POINTS if S != 257] + ["soup:16387x1024"] +
         ["ball", "coarse_ball", "ball:+100", "ball:*40", "ball:*-40", "duplicates", "bad_indices", "lost", "nan_points", "all_invalid",
          "no_vertices", "no_faces", "no_points", "needles"])


@functools.lru_cache(maxsize=None)
def reference(name):
    return point_mesh_distance_reference(*case(name))


def hold(got, name, what):
    """got: key -> array; sqdist, face and closest equal the reference's, bit for bit."""
    want = reference(name)
    for key in KEYS:
        same_bits(got[key], want[key], f"{what}: {key}")


def sphere_queries(v, f, S=256, seed=3):
    """3 S points on and near a mesh: S of its vertices, two in three moved off the surface to either side; S samples of its surface
    by area; and the centroids of its S thinnest faces, where the quotients of the pair formula are worst conditioned."""
    rng = np.random.default_rng(seed)
    near = v[rng.integers(0, len(v), S)].astype(np.float64) + (np.arange(S) % 3 != 0)[:, None] * rng.normal(0.0, 0.3, (S, 3))
    on = surface_sample_reference(v, f, rng.random((S, 3)).astype(np.float32))["points"]
    tri = v[f].astype(np.float64)
    longest = np.max([np.linalg.norm(tri[:, (k + 1) % 3] - tri[:, k], axis=1) for k in range(3)], axis=0)
    altitude = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) / np.maximum(longest, 1e-300)
    thin = np.argsort(altitude, kind="stable")[:S]
    centroids = ((v[f[thin, 0]] + v[f[thin, 1]]) + v[f[thin, 2]]) / np.float32(3.0)
    return np.concatenate([near.astype(np.float32), on, centroids.astype(np.float32)])


# ---- the reference against geometry --------------------------------------------------------------------------------------------------------
def test_the_seven_regions_of_one_triangle():
    f = np.int32([[0, 1, 2]])
    points_and_answers = [
        ((-1, -2, 0), (0, 0, 0), 5), ((-1, -2, 3), (0, 0, 0), 14),          # the corner a
        ((6, -1, 0), (4, 0, 0), 5), ((5, 0, -2), (4, 0, 0), 5),             # b
        ((-1, 7, 0), (0, 4, 0), 10), ((0, 5, 1), (0, 4, 0), 2),             # c
        ((1, -2, 0), (1, 0, 0), 4), ((3, -1, 2), (3, 0, 0), 5),             # the edge ab
        ((-3, 1, 0), (0, 1, 0), 9), ((-1, 3, -1), (0, 3, 0), 2),            # ac
        ((3, 3, 0), (2, 2, 0), 2), ((4, 2, 1), (3, 1, 0), 3),               # bc
        ((1, 1, 0), (1, 1, 0), 0), ((1, 2, 3), (1, 2, 0), 9), ((2, 1, -2), (2, 1, 0), 4),          # inside: on, above and below the plane
        ((0, 0, 0), (0, 0, 0), 0), ((4, 0, 0), (4, 0, 0), 0), ((0, 4, 0), (0, 4, 0), 0),          # on the corners
        ((2, 0, 0), (2, 0, 0), 0), ((0, 1, 0), (0, 1, 0), 0), ((1, 3, 0), (1, 3, 0), 0),          # on the edges
        ((0.5, 0.25, 0.125), (0.5, 0.25, 0), 0.015625)]
    p = np.float32([x[0] for x in points_and_answers])
    out = point_mesh_distance_reference(p, TRIANGLE, f)
    assert out["sqdist"].dtype == np.float32 and out["face"].dtype == np.int32 and out["closest"].dtype == np.float32
    assert out["sqdist"].tolist() == [float(x[2]) for x in points_and_answers]
    assert out["closest"].tolist() == [[float(c) for c in x[1]] for x in points_and_answers]
    assert (out["face"] == 0).all()
    # every winding of the same triangle gives the same distances
    for order in ([1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0], [1, 0, 2]):
        again = point_mesh_distance_reference(p, TRIANGLE, np.int32([order]))
        assert again["sqdist"].tolist() == out["sqdist"].tolist() and again["closest"].tolist() == out["closest"].tolist(), order


def test_ties_take_the_lowest_face():
    p = np.float32([[1, 1, 2], [2, 0, 3], [5, -1, 0]])
    # the same face twice
    assert point_mesh_distance_reference(p, TRIANGLE, np.int32([[0, 1, 2], [0, 1, 2]]))["face"].tolist() == [0, 0, 0]
    # two faces that share the edge ab (the second lies on the other side of it): the first point is nearer to the first face, the
    # second lies above the shared edge and the third is nearest to the shared corner b
    v = np.concatenate([TRIANGLE, np.float32([[0, -4, 0], [9, 9, 9]])])
    for faces, want in (([[0, 1, 2], [1, 0, 3]], [0, 0, 0]), ([[1, 0, 3], [0, 1, 2]], [1, 0, 0]), ([[4, 4, 4], [1, 0, 3], [0, 1, 2]], [2, 1, 1])):
        out = point_mesh_distance_reference(p, v, np.int32(faces))
        assert out["face"].tolist() == want and out["sqdist"].tolist() == [4.0, 9.0, 2.0], faces
    assert out["closest"].tolist() == [[1, 1, 0], [2, 0, 0], [4, 0, 0]]


def test_faces_and_points_that_do_not_count():
    p = np.float32([[1, 1, 3], [np.nan, 0, 0], [7, 7, np.inf]])
    v = np.concatenate([TRIANGLE, np.float32([[np.nan, 0, 0], [1, 1, 1]])])
    # indices outside [0, V) and a NaN vertex: only the last face is left
    out = point_mesh_distance_reference(p, v, np.int32([[0, 1, 5], [-1, 1, 2], [0, 3, 2], [2 ** 31 - 1, 0, 1], [0, 1, 2]]))
    assert out["face"].tolist() == [4, -1, -1] and out["sqdist"].tolist() == [9.0, np.inf, np.inf]
    assert out["closest"].tolist() == [[1, 1, 0], [0, 0, 0], [0, 0, 0]] and not np.signbit(out["closest"]).any()
    # a zero-area face with three coincident corners gives its corner; one with two gives the corner a, or nothing from beside
    out = point_mesh_distance_reference(p[:1], v, np.int32([[4, 4, 4]]))
    assert (out["face"].tolist(), out["sqdist"].tolist(), out["closest"].tolist()) == ([0], [4.0], [[1, 1, 1]])
    out = point_mesh_distance_reference(np.float32([[-1, -1, 0], [1, 1, 0]]), v, np.int32([[0, 0, 2]]))
    assert out["face"].tolist() == [0, -1] and out["sqdist"].tolist() == [2.0, np.inf]          # d2 <= 0: the corner; else 0 / 0
    # no faces, no valid faces, no vertices, no points
    for faces in (np.zeros((0, 3), np.int32), np.int32([[0, 1, 9]])):
        out = point_mesh_distance_reference(p, v, faces)
        assert out["face"].tolist() == [-1] * 3 and np.isposinf(out["sqdist"]).all() and not out["closest"].any()
    out = point_mesh_distance_reference(p, np.zeros((0, 3), np.float32), np.int32([[0, 0, 0]]))
    assert out["face"].tolist() == [-1] * 3
    out = point_mesh_distance_reference(np.zeros((0, 3), np.float32), v, np.int32([[0, 1, 2]]))
    assert out["sqdist"].shape == (0,) and out["face"].shape == (0,) and out["closest"].shape == (0, 3)
    with pytest.raises(ValueError):
        point_mesh_distance_reference(p[:, :2], v, np.int32([[0, 1, 2]]))
    with pytest.raises(ValueError, match="integers"):
        point_mesh_distance_reference(p, v, np.float32([[0, 1, 2]]))


def test_outputs_of_the_references():
    for name in CASES:
        (p, v, f), out = case(name), reference(name)
        assert out["sqdist"].shape == (len(p),) and out["face"].shape == (len(p),) and out["closest"].shape == (len(p), 3), name
        won = out["face"] >= 0
        assert np.isfinite(out["sqdist"][won]).all() and np.isposinf(out["sqdist"][~won]).all() and not out["closest"][~won].any(), name
        assert (out["face"] < len(f)).all(), name
        if name.startswith("soup") or name in ("ball", "coarse_ball", "ball:+100", "duplicates", "bad_indices", "needles"):
            assert won.all(), name
        if name in ("all_invalid", "no_vertices", "no_faces"):
            assert not won.any(), name
    copies = reference("duplicates")["face"] // TILE
    assert not np.isin(copies, (2, 4)).any() and (copies == 0).any()          # the copies in later tiles never win
    assert (~(reference("nan_points")["face"] >= 0)).sum() >= 44


# ---- the reference against float64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 100.0])
def test_reference_against_float64(shift):
    """The fp32 distance against the same algorithm in float64 on the inputs the fp32 one sees.  The error scales with the ulp of the
    largest coordinate, not with the distance: below one ulp near the vertices and on samples drawn by area, and tens of ulp inside
    the thinnest faces of the isosurface, where v and w are quotients of nearly cancelling products -- never more than the width of
    such a face, since its neighbours are that near."""
    v, f, _ = ball()
    v = (v + np.float32(shift)).astype(np.float32)
    p = sphere_queries(v, f)
    got = point_mesh_distance_reference(p, v, f)
    d64 = np.full(len(p), np.inf)
    for first in range(0, len(f), 512):
        c = v[f[first:first + 512]].astype(np.float64)
        d2, _ = closest_on_triangles(p.astype(np.float64)[:, None, :], c[None, :, 0], c[None, :, 1], c[None, :, 2])
        assert d2.dtype == np.float64
        d64 = np.minimum(d64, np.sqrt(np.where(np.isnan(d2), np.inf, d2).min(axis=1)))          # NaN: a zero-area face seen from beside
    ulp = float(np.spacing(np.float32(max(np.abs(v).max(), np.abs(p).max()))))
    ratio = np.abs(np.sqrt(got["sqdist"].astype(np.float64)) - d64) / ulp
    print(f"shift {shift}: the largest error of the distance is {ratio.max():.3f} ulp of the largest coordinate ({ulp:.3g}); k = {K_ULP}")
    for part, name in enumerate(("near the vertices", "surface samples", "centroids of the thinnest faces")):
        print(f"    {name}: {ratio[part * 256:(part + 1) * 256].max():.3f} ulp")
    assert (got["face"] >= 0).all() and (got["sqdist"] == 0).any() and d64.max() > 0.5
    assert ratio.max() <= K_ULP


# ---- the per-lane code on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/mesh_distance_host.cpp, the per-lane functions of csrc/mesh_distance.h as plain loops, built with the host compiler, its
    address and undefined-behaviour sanitizers and without FMA contraction: a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("mesh_distance_host") / "mesh_distance_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CSRC, "mesh_distance_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_on_the_host(program, tmp_path, name, reverse, wave=False):
    p, v, f = case(name)
    S = len(p)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([S, len(v), len(f)], dtype="<i4").tobytes())
        fh.write(np.ascontiguousarray(p).tobytes() + np.ascontiguousarray(v).tobytes() + np.ascontiguousarray(f, dtype="<i4").tobytes())
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + (["reverse"] if reverse else []) +
                       (["wave"] if wave else []), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 2 * 20 * S + 24
    results = []
    for half in range(2):
        at = half * 20 * S
        results.append({"sqdist": np.frombuffer(raw, "<f4", S, at), "face": np.frombuffer(raw, "<i4", S, at + 4 * S),
                        "closest": np.frombuffer(raw, "<f4", 3 * S, at + 8 * S).reshape(S, 3)})
    violations, evaluated, pairs = np.frombuffer(raw, "<i8", 3, 40 * S).tolist()
    return results[0], results[1], violations, evaluated, pairs


@pytest.mark.parametrize("name", CASES)
def test_the_lanes_on_the_host(host_program, tmp_path, name):
    """Every face through the packed-key minimum and the kernel's culled walk, forward and reversed, give the reference's bits; and
    for every (point, tile) the bound with its slack lies at or below every rounded dist2 of the tile's faces."""
    for reverse in (False, True):
        every, culled, violations, evaluated, pairs = run_on_the_host(host_program, tmp_path, name, reverse)
        hold(every, name, f"{name} reverse {reverse}, every face")
        hold(culled, name, f"{name} reverse {reverse}, culled")
        assert violations == 0, (name, reverse, violations)
        assert pairs == len(case(name)[0]) * -(-len(case(name)[2]) // TILE) and 0 <= evaluated <= pairs
    if name == "ball":
        print(f"{name}: a wave of one lane evaluates {evaluated} of {pairs} (point, tile) pairs")
        assert evaluated < pairs // 2


# The schedule of the culled walk, which no output bit shows: case -> the (wave, tile) pairs that the waves of WAVE
# consecutive points evaluate, as given, and the waves times the tiles they are out of.  The host program with `wave` counted them;
# test_the_schedule_of_a_wave holds the program to them and tests/test_gpu_mesh_distance.py the kernel.  The sphere's 257 points are
# of four kinds in turn, far ones among them, so a wave of them spans the whole sphere and needs most tiles: a wave of one lane
# evaluates 2141 of 9766
SCHEDULE = {"ball": (153, 5 * 38), "soup:257x257": (9, 5 * 2)}


def test_the_schedule_of_a_wave(host_program, tmp_path):
    for name, (count, pairs) in SCHEDULE.items():
        p, _, f = case(name)
        waves, tiles = -(-len(p) // WAVE), -(-len(f) // TILE)
        assert waves > 1 and tiles > 1 and pairs == waves * tiles and waves < count < pairs, name
        every, culled, violations, evaluated, of = run_on_the_host(host_program, tmp_path, name, False, wave=True)
        hold(every, name, f"{name} in waves, every face")
        hold(culled, name, f"{name} in waves, culled")
        print(f"{name}: waves of {WAVE} lanes evaluate {evaluated} of {of} (wave, tile) pairs")
        assert (violations, evaluated, of) == (0, count, pairs), name


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_knows_the_constants():
    from npcd import hip
    from npcd.eval import mesh
    from npcd.hip import mesh_distance
    source, tiles = open(f"{CSRC}/mesh_distance.h").read(), open(f"{CSRC}/mesh_tiles.h").read()
    assert int(re.search(r"constexpr int kMdTile = (\d+);", tiles).group(1)) == mesh_distance.TILE_FACES == TILE
    assert int(re.search(r"constexpr int kMdThreads = (\d+);", source).group(1)) == mesh_distance.WAVE_POINTS == WAVE
    assert "kMdMaxVertices = (int64_t)1 << 31" in tiles and mesh_distance.MAX_VERTICES == 2 ** 31
    assert "kMdMaxFaces = (int64_t)1 << 28" in tiles and mesh_distance.MAX_FACES == mesh.MAX_DISTANCE_FACES == 2 ** 28
    assert "kMdMaxPoints = (int64_t)1 << 31" in source and mesh_distance.MAX_POINTS == 2 ** 31
    assert hip.closest_on_mesh is mesh_distance.closest_on_mesh
    assert np.float32(1.0) - np.float32(2.0) ** -11 == np.float32(re.search(r"kMdShrink = ([0-9.]+)f;", source).group(1))


def test_kernels_use_no_scratch(tmp_path):
    kernels = _compile("mesh_distance.hip", str(tmp_path / "mesh_distance.s"))
    assert len(kernels) == 3, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0, (name, k)
        if "md_query_kernel" in name:          # one tile of corners, 256 faces x 3 x 16 bytes; 4 waves to a SIMD at up to 128 registers
            assert k["lds"] == TILE * 3 * 16 == 12288 and k["vgpr"] <= 128, (name, k)
        else:                                  # the four wave parts of a box: 4 x 8 floats
            assert "md_boxes_kernel" in name and k["lds"] == 128 and k["vgpr"] <= 64, (name, k)


def test_header_exports_and_signatures():
    from npcd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "npcd_hip.h")).read()
    L = hip.lib()
    names = ("npcd_mesh_distance_ws_bytes", "npcd_mesh_distance_boxes", "npcd_mesh_distance_query")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in hip.SIGNATURES and hasattr(L, name), name
    assert L.npcd_missing == () and L.npcd_abi_version() == 10
    assert hip.SIGNATURES["npcd_mesh_distance_ws_bytes"][0] is ctypes.c_int64
    assert [len(hip.SIGNATURES[n][1]) for n in names] == [2, 6, 13]
    # the host-side refusals, which look at no pointer's target and launch nothing
    V, F, S = 1000, 3000, 500
    assert L.npcd_mesh_distance_ws_bytes(V, F) == 12 * (32 + TILE * 48) and L.npcd_mesh_distance_ws_bytes(V, 256) == 32 + TILE * 48
    assert L.npcd_mesh_distance_ws_bytes(0, 0) == 0 and L.npcd_mesh_distance_ws_bytes(0, 1) == 32 + TILE * 48
    assert L.npcd_mesh_distance_ws_bytes(-1, F) == -1 and L.npcd_mesh_distance_ws_bytes(V, -1) == -1
    assert L.npcd_mesh_distance_ws_bytes(2 ** 31, F) == -2 and L.npcd_mesh_distance_ws_bytes(V, 2 ** 28) == -2
    assert L.npcd_mesh_distance_ws_bytes(2 ** 31, -1) == -1          # a negative size before a large one
    assert L.npcd_mesh_distance_ws_bytes(2 ** 31 - 1, 2 ** 28 - 1) > 0
    one = ctypes.c_void_p(64)          # never followed: every call below is refused before a launch

    def refused(fn, args, **changed):
        a = list(args)
        for i, value in changed.items():
            a[int(i[1:])] = value
        return fn(*a)
    #        vertices, V, faces, F, ws, stream
    boxes = [one, V, one, F, one, None]
    for missing in (0, 2, 4):
        assert refused(L.npcd_mesh_distance_boxes, boxes, **{f"_{missing}": None}) == -1, missing
    assert refused(L.npcd_mesh_distance_boxes, boxes, _3=0) == -1 and refused(L.npcd_mesh_distance_boxes, boxes, _1=-1) == -1
    assert refused(L.npcd_mesh_distance_boxes, boxes, _4=ctypes.c_void_p(72)) == -1          # the workspace: 16-byte aligned
    assert refused(L.npcd_mesh_distance_boxes, boxes, _2=ctypes.c_void_p(66)) == -1
    assert refused(L.npcd_mesh_distance_boxes, boxes, _1=2 ** 31) == -2 and refused(L.npcd_mesh_distance_boxes, boxes, _3=2 ** 28) == -2
    assert refused(L.npcd_mesh_distance_boxes, boxes, _1=2 ** 31, _4=None) == -2          # unsupported before a missing pointer
    #        points, S, vertices, V, faces, F, ws, cull, sqdist, face, closest, evaluated, stream
    query = [one, S, one, V, one, F, one, 1, one, one, one, None, None]
    for missing in (0, 6, 8, 9, 10):
        assert refused(L.npcd_mesh_distance_query, query, **{f"_{missing}": None}) == -1, missing
    for slot, bad in ((1, 0), (1, -1), (5, 0), (3, -1), (7, 2), (7, -1)):
        assert refused(L.npcd_mesh_distance_query, query, **{f"_{slot}": bad}) == -1, (slot, bad)
    assert refused(L.npcd_mesh_distance_query, query, _6=ctypes.c_void_p(72)) == -1
    assert refused(L.npcd_mesh_distance_query, query, _11=ctypes.c_void_p(68)) == -1          # the counter: 8-byte aligned
    assert refused(L.npcd_mesh_distance_query, query, _8=ctypes.c_void_p(66)) == -1
    for slot, bad in ((1, 2 ** 31), (3, 2 ** 31), (5, 2 ** 28)):
        assert refused(L.npcd_mesh_distance_query, query, **{f"_{slot}": bad}) == -2, (slot, bad)
    assert refused(L.npcd_mesh_distance_query, query, _1=2 ** 31, _0=None) == -2


def test_wrapper_argument_errors():
    from npcd.hip.mesh_distance import closest_on_mesh
    p, v, f = (torch.from_numpy(a) for a in case("soup:255x257"))
    with pytest.raises(RuntimeError, match="GPU"):
        closest_on_mesh(p, v, f)                                                   # not on the GPU: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        closest_on_mesh(p[:0], v, f)
    for bad in ((p.numpy(), v, f), (p, v.numpy(), f), (p, v, f.numpy()), (p[:, :2], v, f), (p, v.reshape(-1), f), (p, v, f[:, :2]),
                (p[None], v, f)):
        with pytest.raises(ValueError):
            closest_on_mesh(*bad)
    with pytest.raises(ValueError, match=rf"{2 ** 28} faces"):
        closest_on_mesh(p, v, torch.zeros(1, 3, dtype=torch.int32).expand(2 ** 28, 3))
    with pytest.raises(ValueError, match=rf"{2 ** 31} points"):
        closest_on_mesh(torch.zeros(1, 3).expand(2 ** 31, 3), v, f)


# ---- what users call, with stand-ins -------------------------------------------------------------------------------------------------------
def sampler(mesh, num_samples, generator=None, return_faces=False):
    """Stands in for npcd.hip.surface.sample_surface on one pair."""
    v, f = mesh
    u = torch.rand((num_samples, 3), generator=generator, dtype=torch.float32)
    got = surface_sample_reference(v.numpy(), f.numpy(), u.numpy())
    out = (torch.from_numpy(got["points"]), torch.tensor(float(got["area"]), dtype=torch.float64))
    return out + ((torch.from_numpy(got["face"]),) if return_faces else ())


def closest(points, vertices, faces):
    """Stands in for npcd.hip.mesh_distance.closest_on_mesh."""
    return {k: torch.from_numpy(a) for k, a in point_mesh_distance_reference(points.numpy(), vertices.numpy(), faces.numpy()).items()}


def test_mesh_deviation_with_stand_ins():
    v, f = (torch.from_numpy(a) for a in coarse_ball())
    same = mesh_deviation((v, f), {"vertices": v, "faces": f}, 300, generator=torch.Generator().manual_seed(1), sampler=sampler, closest=closest)
    nothing = (SAMPLE_ULP + K_ULP) * float(np.spacing(v.abs().max().numpy()))          # "0" of a sampled surface, see SAMPLE_ULP
    for d in (same["a_to_b"], same["b_to_a"]):
        assert 0 <= d["mean"] <= d["rms"] <= d["max"] <= nothing, d
    assert same["hausdorff"] == max(same["a_to_b"]["max"], same["b_to_a"]["max"]) and same["samples"] == 300
    # samples that are vertices of a mesh on small integers: 0 exactly
    grid = torch.from_numpy(np.float32([[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 2]]))
    two = torch.from_numpy(np.int32([[0, 1, 2], [1, 3, 2]]))
    exact = mesh_deviation((grid, two), (grid, two), 4, closest=closest,
                           sampler=lambda mesh, n, generator=None, return_faces=False: (mesh[0][:n], None, torch.zeros(n, dtype=torch.int32)))
    zero = {"mean": 0.0, "rms": 0.0, "max": 0.0}
    assert exact["a_to_b"] == zero and exact["b_to_a"] == zero and exact["hausdorff"] == 0.0 and exact["mean"] == 0.0 and exact["diagonal"] == 6.0
    lo, hi = v.double().amin(0), v.double().amax(0)
    assert same["diagonal"] == float(torch.sqrt(((hi - lo) ** 2).sum())) and all(isinstance(x, float) for x in same["a_to_b"].values())
    # a large square against a copy of itself shifted by (0, 0, 1), sampled at integer (x, y): every sample lies above or below the
    # other square, at distance 1 exactly.  (A sample of sample_surface has z = (b0 + b1) + b2, which is 1 only to an ulp.)
    quad = torch.from_numpy(np.int32([[0, 1, 2], [0, 2, 3]]))
    plane = torch.from_numpy(np.float32([[-32, -32, 0], [32, -32, 0], [32, 32, 0], [-32, 32, 0]]))
    lifted = plane + torch.tensor([0.0, 0.0, 1.0])

    def lattice_sampler(mesh, n, generator=None, return_faces=False):
        xy = torch.randint(-32, 33, (n, 2), generator=generator).float()
        return torch.cat([xy, mesh[0][:1, 2:].expand(n, 1)], dim=1), None, torch.zeros(n, dtype=torch.int32)
    got = mesh_deviation((lifted, quad), (plane, quad), 500, generator=torch.Generator().manual_seed(2), sampler=lattice_sampler, closest=closest)
    one = {"mean": 1.0, "rms": 1.0, "max": 1.0}
    assert got["a_to_b"] == one and got["b_to_a"] == one and got["hausdorff"] == 1.0 and got["mean"] == 1.0
    assert got["diagonal"] == pytest.approx(np.sqrt(64.0 ** 2 + 64.0 ** 2), rel=1e-14)
    # two calls with equal generators agree; a mesh without surface gives NaN both ways
    args = ((v, f), (v * 1.01, f), 200)
    first = mesh_deviation(*args, generator=torch.Generator().manual_seed(3), sampler=sampler, closest=closest)
    again = mesh_deviation(*args, generator=torch.Generator().manual_seed(3), sampler=sampler, closest=closest)
    assert first == again and 0 < first["a_to_b"]["mean"] <= first["a_to_b"]["rms"] <= first["a_to_b"]["max"] <= first["hausdorff"]
    assert first["hausdorff"] <= 0.01 * 3 ** 0.5 * float(v.abs().max()) * 1.001          # a point moves by 0.01 |x|, and every sample has a copy
    assert first["mean"] == 0.5 * (first["a_to_b"]["mean"] + first["b_to_a"]["mean"])
    empty = mesh_deviation((v, f), (v, f[:0]), 50, sampler=sampler, closest=closest)
    assert all(np.isnan(x) for d in (empty["a_to_b"], empty["b_to_a"]) for x in d.values()) and np.isnan(empty["hausdorff"]) and np.isnan(empty["mean"])
    assert np.isnan(mesh_deviation((v[:0], f[:0]), (v, f), 50, sampler=sampler, closest=closest)["diagonal"])
    with pytest.raises(ValueError, match="num_samples"):
        mesh_deviation((v, f), (v, f), 0, sampler=sampler, closest=closest)


def test_cloud_mesh_distance_with_stand_ins():
    plane = torch.from_numpy(np.float32([[-9, -9, 0], [9, -9, 0], [9, 9, 0], [-9, 9, 0]]))
    quad = torch.from_numpy(np.int32([[0, 1, 2], [0, 2, 3]]))
    cloud = torch.tensor([[0.0, 0, 1], [1, 2, -1], [3, 3, 1], [np.nan, 0, 0]])
    assert cloud_mesh_distance(cloud, (plane, quad), closest=closest) == {"mean": 1.0, "rms": 1.0, "max": 1.0}          # the NaN point has no face
    cloud = torch.tensor([[0.0, 0, 3], [1, 2, -4]])
    assert cloud_mesh_distance(cloud, {"vertices": plane, "faces": quad}, closest=closest) == {"mean": 3.5, "rms": 12.5 ** 0.5, "max": 4.0}
    for nothing in (cloud_mesh_distance(cloud[:0], (plane, quad), closest=closest), cloud_mesh_distance(cloud, (plane, quad[:0]), closest=closest)):
        assert sorted(nothing) == ["max", "mean", "rms"] and all(np.isnan(x) for x in nothing.values())


def test_extract_mesh_deviation_with_stand_ins(monkeypatch):
    """extract_mesh(deviation=None) gives what it gave before the option existed; deviation=n compares the final mesh with the raw
    isosurface; without simplify or smooth it raises."""
    import npcd.hip.isosurface as iso_module
    from npcd.eval.mesh import DEVIATION_SEED, extract_mesh
    field = _Field()

    def isosurface(volume, level, origin, spacing, normals=False, gradient_of=None):
        v, f = marching_tetrahedra_reference(volume[0].numpy(), level, origin.numpy(), spacing.numpy())
        n = vertex_normals_reference(volume[0].numpy(), level, spacing.numpy())
        return [(torch.from_numpy(v), torch.from_numpy(f)) + ((torch.from_numpy(n),) if normals else ())]
    monkeypatch.setattr(iso_module, "isosurface", isosurface)

    def simplifier(vertices, faces, cell, origin=None, dims=None, attributes=None):
        out = simplify_reference(vertices.numpy(), faces.numpy(), cell, origin, dims, None if attributes is None else attributes.numpy())
        return {k: torch.from_numpy(a) for k, a in out.items()}

    def smoother(vertices, faces, iterations=10, lam=0.5, mu=-0.53, edges=None):
        return torch.from_numpy(smooth_reference(vertices.numpy(), faces.numpy(), iterations, lam, mu)[0])

    def deviator(a, b, num_samples, generator=None):
        return mesh_deviation(a, b, num_samples, generator=generator, sampler=sampler, closest=closest)
    coords, feats = torch.zeros(1, 4, 3), torch.zeros(1, 4, 8)
    raw_v, raw_f = marching_tetrahedra_reference(field.vol, 0.0, np.float32(field.origin), np.float32(field.spacing))
    common = dict(resolution=12, level=0.0, simplifier=simplifier, smoother=smoother, deviator=deviator)
    (plain,) = extract_mesh(field, coords, feats, simplify=2, **common)
    (same,) = extract_mesh(field, coords, feats, simplify=2, deviation=None, **common)
    assert sorted(plain) == sorted(same) and "deviation" not in plain
    assert all(plain[k].numpy().tobytes() == same[k].numpy().tobytes() for k in plain)
    (coarse,) = extract_mesh(field, coords, feats, simplify=2, deviation=200, **common)
    assert set(coarse) == set(plain) | {"deviation"}
    assert all(coarse[k].numpy().tobytes() == plain[k].numpy().tobytes() for k in plain)
    want = mesh_deviation(plain, (torch.from_numpy(raw_v), torch.from_numpy(raw_f)), 200, generator=torch.Generator().manual_seed(DEVIATION_SEED),
                          sampler=sampler, closest=closest)
    assert coarse["deviation"] == want and want["samples"] == 200
    cell_diagonal = 2.0 * float(np.sqrt((np.float64(field.spacing) ** 2).sum()))          # a vertex moves at most a cell's diagonal
    assert 0 < want["hausdorff"] <= cell_diagonal
    (smooth,) = extract_mesh(field, coords, feats, smooth=3, deviation=100, **common)
    (again,) = extract_mesh(field, coords, feats, smooth=3, deviation=100, **common)
    assert smooth["deviation"] == again["deviation"] and 0 < smooth["deviation"]["hausdorff"] < cell_diagonal
    with pytest.raises(ValueError, match="nothing to compare"):
        extract_mesh(field, coords, feats, deviation=100, **common)
    for bad in (0, -5, 2.5, True):
        with pytest.raises(ValueError, match="deviation"):
            extract_mesh(field, coords, feats, simplify=2, deviation=bad, **common)
