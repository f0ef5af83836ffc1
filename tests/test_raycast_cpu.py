"""Rays against meshes without a GPU: the CPU restatement npcd.eval.mesh.ray_mesh_reference against an independent
float64 Moeller-Trumbore, against watertightness on a closed sphere and the exact cases of the specification; the per-lane code of
csrc/raycast.h, the code the kernel runs, built for the host with sanitizers (csrc/raycast_host.cpp) and held bit for bit to the
reference on the cases of the GPU test (tests/test_gpu_raycast.py, which imports them from here), with the culling bound checked
against every hit; the kernel's resources from the compiler's own output, the entry point's refusals, the wrapper's argument errors,
and render_mesh, mesh_render_agreement and extract_mesh(agreement=) with stand-ins."""
import ctypes
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from npcd.eval.mesh import (marching_tetrahedra_reference, mesh_edges_reference, mesh_render_agreement, ray_axes, ray_mesh_reference,
                            render_mesh, vertex_normals_reference)
from test_kernel_resources import CSRC, _compile
from test_simplify_cpu import _Field, same_bits
from test_smooth_cpu import CENTRE, ball, coarse_ball, soup

TILE, WAVE = 256, 64          # kMdTile of csrc/mesh_tiles.h and kRcThreads of csrc/raycast.h; test_the_wrapper_knows_the_constants holds them
FACES = (1, 255, 256, 257, 513)          # one below, at and above a tile, two tiles and one face
RAYS = (1, 63, 64, 65, 257)              # one below, at and above a wave, five waves
KEYS = ("t", "face", "bary", "front")
U24 = 2.0 ** -24
# How far the point o + t d of a hit lies from the face, per axis, in units of u M (u = 2^-24, M the largest |coordinate| of the origin
# and the face's corners; u M < ulp(M)).  Steps 2 to 6 of the specification: p = fl(P - o) is off by u |p| <= 2 u M per component;
# px = fl(p[kx] - fl(Sx p[kz])) rounds twice, u |Sx p[kz]| + u |px| <= 2 u M + 4 u M since |Sx| <= 1.  The hit says that 0 is a
# convex combination (weights U / det, V / det, W / det, exact but for 2^-53) of the projected corners, so o + t d differs from the
# same combination of the corners by: along kx or ky, 2 u M (p) + 6 u M (px) + 8 u M (t d[kz] carries the roundings of Sz, pz and t
# itself, 3 u, and d[kx] = Sx d[kz] that of Sx, 1 u, on a length of at most 2 M); along kz, 4 u on at most 2 M.  16 u M at most; the
# float64 operations add 2^-50 of that.  17 leaves room for the second-order terms.
HIT_UM = 17.0
SMALL = 3.3          # the radius of the small closed sphere: every vertex and every edge takes a ray


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def rays(v, f, R, seed):
    """R rays at a mesh in four kinds, interleaved: from far outside at samples of its surface (not normalised: t near 1), from outside
    exactly at its vertices (where edges meet), from inside its box in random unit directions, and from far away in random directions
    (most miss).  -> (origins, directions) float32."""
    rng = np.random.default_rng(seed)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    good = f[ok] if ok.any() else np.zeros((1, 3), dtype=np.int64)
    vv = v if len(v) else np.zeros((1, 3), dtype=np.float32)
    finite = vv[np.isfinite(vv).all(axis=1)]
    lo, hi = (finite.min(axis=0), finite.max(axis=0)) if len(finite) else (np.zeros(3, np.float32), np.ones(3, np.float32))
    size = np.maximum(hi - lo, np.float32(1e-30))
    b = rng.dirichlet((1.0, 1.0, 1.0), R).astype(np.float32)
    tri = vv[good[rng.integers(0, len(good), R)] % len(vv)]
    unit = rng.standard_normal((R, 3))
    unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(np.float32)
    with np.errstate(all="ignore"):
        on_surface = (b[:, :1] * tri[:, 0] + b[:, 1:2] * tri[:, 1]) + b[:, 2:] * tri[:, 2]
        corners = vv[rng.integers(0, len(vv), R)]
        far = (lo + hi) * np.float32(0.5) + np.float32(3.0) * size * unit
        inside = lo + rng.random((R, 3)).astype(np.float32) * size
        kind = (np.arange(R) % 4)[:, None]
        o = np.where(kind == 2, inside, far).astype(np.float32)
        d = np.where(kind == 0, on_surface - o, np.where(kind == 1, corners - o, rng.permutation(unit))).astype(np.float32)
    return np.where(np.isfinite(o), o, np.float32(0)), np.where(np.isfinite(d), d, np.float32(1))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (origins [R, 3], directions [R, 3], vertices [V, 3] float32, faces [F, 3] int32, t_min, t_max).  "reversed|name": the faces of
    `name` in descending order."""
    if name.startswith("reversed|"):
        o, d, v, f, t_min, t_max = case(name.partition("|")[2])
        return o, d, v, np.ascontiguousarray(f[::-1]), t_min, t_max
    kind, _, arg = name.partition(":")
    rng = np.random.default_rng(len(name) * 17 + 3)
    limits = (0.0, float("inf"))
    if kind == "soup":          # F x R: tile and wave edges
        F, R = (int(x) for x in arg.split("x"))
        v, f = soup(F, seed=2)
        return rays(v, f, R, F + R) + (v, f) + limits
    if kind in ("ball", "coarse_ball"):          # the 24^3 sphere, plain and simplified: arg is a shift or a power of two
        v, f = coarse_ball() if kind == "coarse_ball" else ball()[:2]
        if arg.startswith("+"):
            v = (v + np.float32(arg[1:])).astype(np.float32)
        elif arg.startswith("*"):
            v = (v * np.float32(2.0) ** int(arg[1:])).astype(np.float32)
        return rays(v, f, 257 if not arg else 129, 7) + (v, f.astype(np.int32)) + limits
    if kind == "duplicates":          # the faces of the first tile again in the third and the fifth: the lowest index wins
        v, f = soup(256, seed=3)
        f = np.concatenate([f, soup(256, seed=4)[1] % len(v), f[::-1], soup(256, seed=5)[1] % len(v), f]).astype(np.int32)
        return rays(v, f[:256], 257, 9) + (v, f) + limits
    if kind == "bad_indices":
        v, f = soup(600, seed=6)
        f = f.copy()
        f[3], f[50], f[300], f[301], f[599] = (-1, 2, 3), (1, len(v), 2), (1, 2, 2 ** 31 - 1), (-2 ** 31, 0, 1), (0, 1, -5)
        return rays(v, f, 257, 10) + (v, f) + limits
    if kind == "lost":          # 1 % of the vertices have a coordinate that is not finite
        v, f = soup(3000, seed=4)
        o, d = rays(v, f, 257, 11)
        v = v.copy()
        bad = rng.choice(len(v), len(v) // 100, replace=False)
        v[bad, rng.integers(0, 3, len(bad))] = np.float32([np.nan, np.inf, -np.inf])[rng.integers(0, 3, len(bad))]
        return o, d, v, f, *limits
    if kind == "bad_rays":          # NaN, infinite and zero directions, origins that are not finite, directions along one axis
        v, f = soup(513, seed=7)
        o, d = rays(v, f, 130, 12)
        rows = np.arange(0, len(o), 5)
        d[rows, rng.integers(0, 3, len(rows))] = np.nan
        d[1], d[6], d[11] = (0, 0, 0), (np.inf, 0.5, 0.5), (-0.0, 0.0, -0.0)
        o[2], o[7] = (np.nan, 0.5, 0.5), (0.5, -np.inf, 0.5)
        d[3], d[8], d[13] = (0, 0, 1), (0, -1, 0), (1, 0, 0)
        o[3], o[8], o[13] = (0.5, 0.5, -2), (0.5, 3, 0.5), (-2, 0.5, 0.5)
        return o, d, v, f, *limits
    if kind == "limits":          # t_min > 0 and a finite t_max: unit directions from inside the soup, so hits lie on both sides of either
        v, f = soup(513, seed=8)
        o, d = rays(v, f, 257, 13)
        return o, d, v, f, 0.25, 1.0
    if kind == "behind":          # a negative t_min: hits behind the origin count and order as signed numbers
        v, f = soup(257, seed=9)
        o, d = rays(v, f, 129, 14)
        return o, d, v, f, -0.5, 0.75
    if kind == "all_invalid":          # 300 faces, none with three indices inside [0, V)
        v = soup(40)[0]
        f = rng.integers(0, len(v), (300, 3)).astype(np.int32)
        f[np.arange(300), rng.integers(0, 3, 300)] = np.where(rng.random(300) < 0.5, -1 - rng.integers(0, 9, 300), len(v) + rng.integers(0, 9, 300))
        return rays(v, soup(40)[1], 65, 15) + (v, f) + limits
    if kind == "no_vertices":
        return rng.random((5, 3)).astype(np.float32), np.ones((5, 3), np.float32), np.zeros((0, 3), np.float32), np.int32([[0, 1, 2], [0, 0, 0]]), *limits
    if kind == "no_faces":
        return rng.random((65, 3)).astype(np.float32), np.ones((65, 3), np.float32), soup(40)[0], np.zeros((0, 3), np.int32), *limits
    if kind == "no_rays":
        v, f = soup(300)
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), v, f, *limits
    if kind == "needles":          # zero-area faces (two or three equal corners) among ordinary ones
        v, f = soup(257, seed=8)
        f = f.copy()
        f[::3, 1] = f[::3, 0]
        f[1::9, 2] = f[1::9, 1] = f[1::9, 0]
        return rays(v, f, 257, 16) + (v, f) + limits
    raise KeyError(name)


CASES = ([f"soup:{F}x257" for F in FACES] + [f"soup:513x{R}" for R in RAYS if R != 257] +
         ["ball", "coarse_ball", "ball:+100", "ball:*40", "ball:*-40", "duplicates", "bad_indices", "lost", "bad_rays", "limits", "behind",
          "all_invalid", "no_vertices", "no_faces", "no_rays", "needles"])


@functools.lru_cache(maxsize=None)
def reference(name):
    return ray_mesh_reference(*case(name))


def hold(got, name, what):
    """got: key -> array; t, face, bary and front equal the reference's, bit for bit."""
    want = reference(name)
    for key in KEYS:
        if key == "front":
            assert got[key].dtype == np.int8 and np.array_equal(got[key], want[key]), f"{what}: {key}"
        else:
            same_bits(got[key], want[key], f"{what}: {key}")


def small_ball():
    v, f, _ = ball(SMALL)
    return v, f.astype(np.int32)


def moeller_trumbore(o, d, v, f):
    """An independent restatement in float64 (Moeller and Trumbore 1997): o, d [R, 3], one mesh -> (t, u, v) [R, F] float64, t = +inf
    where the line misses the face or runs in its plane."""
    o, d, c = o.astype(np.float64), d.astype(np.float64), v[f].astype(np.float64)
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    with np.errstate(all="ignore"):
        pv = np.cross(d[:, None, :], e2[None])
        det = (e1[None] * pv).sum(-1)
        tv = o[:, None, :] - c[None, :, 0]
        uu = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1[None])
        vv = (d[:, None, :] * qv).sum(-1) / det
        t = (e2[None] * qv).sum(-1) / det
        inside = (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (det != 0)
    return np.where(inside, t, np.inf), uu, vv


# ---- the reference against an independent float64 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ball", "soup:513x257"])
def test_reference_against_float64(name):
    """Which face is hit, for rays whose float64 hit lies well inside a face and well before the next one; and t within the bound
    that HIT_UM gives: the point o + t d lies within e = HIT_UM u M per axis of the face, so n . ((t - t*) d) = n . e for the face's
    unit normal n and the exact t*: |t - t*| <= |n|_1 e / |n . d| <= sqrt(3) e / |n . d|."""
    _, _, v, f, _, _ = case(name)
    if name.startswith("soup"):
        f = f[np.arange(len(f)) % 5 != 4]          # without the planted copies, which tie with their originals by design
    o, d = rays(v, f, 344, 21)
    o, d = o[np.arange(344) % 4 != 1], d[np.arange(344) % 4 != 1]          # without the rays aimed at vertices: those graze by design
    got = ray_mesh_reference(o, d, v, f)
    t64, uu, vv = moeller_trumbore(o, d, v, f)
    t64 = np.where(t64 >= 0, t64, np.inf)
    order = np.argsort(t64, axis=1, kind="stable")
    rows = np.arange(len(o))
    first = order[:, 0]
    t_first, t_next = t64[rows, first], (t64[rows, order[:, 1]] if len(f) > 1 else np.full(len(o), np.inf))
    hits = np.isfinite(t_first)
    u1, v1 = uu[rows, first], vv[rows, first]
    with np.errstate(invalid="ignore"):
        well = hits & (np.minimum(np.minimum(u1, v1), 1 - u1 - v1) > 1e-4) & (t_next - t_first > 1e-4 * np.abs(t_first))
    grazing = hits & ~well
    share = grazing.sum() / max(hits.sum(), 1)
    print(f"{name}: {hits.sum()} of {len(o)} rays hit in float64; {grazing.sum()} ({100 * share:.2f} %) graze an edge or a second face and are left out")
    assert share <= 0.05 and well.sum() >= len(o) // 4
    assert np.array_equal(got["face"][well], first[well]), np.nonzero(well & (got["face"] != first))[0]
    assert (got["face"][~hits & np.isinf(t64).all(axis=1)] == -1).all()          # what float64 misses altogether, the rule misses
    c = v[f[first[well]]].astype(np.float64)
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    M = np.maximum(np.abs(o[well]).max(axis=1), np.abs(c).max(axis=(1, 2))).astype(np.float64)
    bound = math.sqrt(3.0) * HIT_UM * U24 * M / np.abs((n * d[well].astype(np.float64)).sum(axis=1))
    ratio = np.abs(got["t"][well].astype(np.float64) - t_first[well]) / bound
    print(f"{name}: the largest |t - t64| is {ratio.max():.4f} of its bound; in ulp of t at most {np.max(np.abs(got['t'][well] - t_first[well]) / np.spacing(got['t'][well])):.2f}")
    assert ratio.max() <= 1.0


# ---- watertightness --------------------------------------------------------------------------------------------------------------------------
def edge_midpoints(v, f):
    e = mesh_edges_reference(len(v), f)
    assert e["counts"][3] == 0 and e["counts"][4] == 0          # closed: no boundary edge, no edge of three faces
    return ((v[e["edges"][:, 0]] + v[e["edges"][:, 1]]) * np.float32(0.5)).astype(np.float32)


def test_watertight_through_vertices_and_edges():
    """From an interior point through every vertex and every edge midpoint of a closed sphere, rays in fp32: the fp32 direction does not
    pass through the vertex exactly, so the ray passes within rounding of an edge or a vertex -- and none slips through.  Exactly one
    t wins per ray, and its face holds the vertex or the edge, or is a neighbour within rounding.  The same targets from outside."""
    v, f = small_ball()
    targets = np.concatenate([v, edge_midpoints(v, f)])
    centre = np.float32(CENTRE)
    for origin in (centre, centre + np.float32([0.4, -0.3, 0.2])):
        d = (targets - origin).astype(np.float32)
        got = ray_mesh_reference(np.broadcast_to(origin, d.shape), d, v, f)
        assert (got["face"] >= 0).all() and np.isfinite(got["t"]).all(), np.nonzero(got["face"] < 0)[0]
        assert np.abs(got["t"] - 1).max() < 1e-5 and (got["front"] == 0).all()          # the target itself, seen from inside
    outside = (centre + np.float32(3.0) * (targets - centre)).astype(np.float32)
    got = ray_mesh_reference(outside, (centre - outside).astype(np.float32), v, f)
    assert (got["face"] >= 0).all() and (got["front"] == 1).all()
    assert np.abs(got["t"] - 2.0 / 3.0).max() < 1e-5
    print(f"{len(targets)} rays through {len(v)} vertices and {len(targets) - len(v)} edge midpoints of {len(f)} faces, from two interior points and from outside: none missed")


def test_watertight_in_random_directions():
    v, f, _ = ball()
    rng = np.random.default_rng(5)
    d = rng.standard_normal((600, 3)).astype(np.float32)
    o = np.broadcast_to(np.float32(CENTRE) + np.float32([1.5, -2.0, 0.7]), d.shape)
    got = ray_mesh_reference(o, d, v, f)
    assert (got["face"] >= 0).all() and (got["front"] == 0).all() and (got["t"] > 0).all()
    hit = o + got["t"][:, None] * d
    radius = np.linalg.norm(hit - np.float32(CENTRE), axis=1)
    assert 9.3 - 1.0 < radius.min() and radius.max() < 9.3 + 0.1          # on the faceted sphere of radius 9.3, unit spacing


# ---- the exact cases of the specification ------------------------------------------------------------------------------------------------------
LATTICE = np.float32([[0, -4, 5], [0, 4, 5], [-4, 0, 5], [4, 0, 5]])          # two faces that share the edge x = 0 in the plane z = 5


def test_axes():
    d = np.float32([[1, 2, 3], [1, -3, 2], [-2, 1, 2], [2, 2, 2], [0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, -1, 1]])
    kx, ky, kz, usable = ray_axes(d)
    assert kz.tolist() == [2, 1, 0, 0, 0, 0, 1, 1]          # the largest, the lowest among equal ones; nothing is larger than a NaN (not usable anyway)
    assert (kx[:4].tolist(), ky[:4].tolist()) == ([0, 0, 2, 1], [1, 2, 1, 2])          # swapped where d[kz] < 0
    assert usable.tolist() == [True, True, True, True, False, False, False, True]


def test_zero_edge_function_counts_for_both_faces():
    """A ray in the plane x = 0 of the shared edge: on these lattice coordinates every sheared corner is exact, the edge function of
    the shared edge is exactly 0 for both faces, both are hit at t = 5 and the lowest index wins, whichever face comes first."""
    o, d = np.float32([[0, 0, 0], [0, 1, 0], [0, 4, 0], [0, 0, 10]]), np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1]])
    for faces in ([[0, 1, 2], [1, 0, 3]], [[1, 0, 3], [0, 1, 2]], [[0, 1, 2], [0, 1, 3]]):          # the last: both wound alike
        got = ray_mesh_reference(o, d, LATTICE, np.int32(faces))
        assert got["face"].tolist() == [0, 0, 0, 0] and got["t"].tolist() == [5.0, 5.0, 5.0, 5.0], faces
        assert np.array_equal(got["bary"][0], np.float32([0.5, 0.5, 0])) and np.array_equal(got["bary"][2], np.float32([0, 1, 0]) if faces[0][0] == 0 else np.float32([1, 0, 0]))
    # each face alone is hit too: the edge belongs to both
    for face in ([0, 1, 2], [1, 0, 3]):
        assert ray_mesh_reference(o, d, LATTICE, np.int32([face]))["face"].tolist() == [0, 0, 0, 0]
    # a step to either side leaves one face
    got = ray_mesh_reference(np.float32([[-1, 0, 0], [1, 0, 0]]), d[:2], LATTICE, np.int32([[0, 1, 2], [1, 0, 3]]))
    assert got["face"].tolist() == [0, 1]


def test_ties_and_limits():
    tri = np.int32([[0, 1, 2]])
    o, d = np.float32([[-1, 0, 0]]), np.float32([[0, 0, 1]])
    # the same face three times, and wound the other way: the lowest index wins
    got = ray_mesh_reference(o, d, LATTICE, np.int32([[9, 9, 9], [0, 1, 2], [1, 2, 0], [1, 0, 2]]))
    assert (got["face"].tolist(), got["t"].tolist()) == ([1], [5.0])
    # inclusive limits
    below, above = np.nextafter(np.float32(5), np.float32(0)), np.nextafter(np.float32(5), np.float32(9))
    for t_min, t_max, hit in ((0, 5, True), (5, 5, True), (5, np.inf, True), (0, below, False), (above, np.inf, False), (6, 4, False), (np.nan, 9, False)):
        got = ray_mesh_reference(o, d, LATTICE, tri, t_min=t_min, t_max=t_max)
        assert got["face"].tolist() == [0 if hit else -1], (t_min, t_max)
        assert got["t"].tolist() == [5.0 if hit else np.inf] and got["front"].tolist() == [0] and got["bary"].sum() == (1.0 if hit else 0.0)
    # a hit behind the origin does not count at t_min = 0; with a negative t_min it does, and orders as a signed number
    back = np.float32([[0, 0, -1]])
    assert ray_mesh_reference(o, back, LATTICE, tri)["face"].tolist() == [-1]
    got = ray_mesh_reference(o, back, LATTICE, tri, t_min=-9.0)
    assert (got["face"].tolist(), got["t"].tolist()) == ([0], [-5.0])
    two = np.concatenate([LATTICE, LATTICE - np.float32([0, 0, 7])])          # a second sheet at z = -2
    got = ray_mesh_reference(o, d, two, np.int32([[0, 1, 2], [4, 5, 6]]), t_min=-9.0)
    assert (got["face"].tolist(), got["t"].tolist()) == ([1], [-2.0])
    # front: the normal (B - A) x (C - A) of (0, 1, 2) is (0, 0, -64)... it points against a ray that travels up
    n = np.cross(LATTICE[1] - LATTICE[0], LATTICE[2] - LATTICE[0])
    assert n[2] > 0          # so the face (0, 1, 2) is seen from behind by a ray that travels up, and from the front by one that comes down
    down_o, down = np.float32([[-1, 0, 9]]), np.float32([[0, 0, -1]])
    assert ray_mesh_reference(o, d, LATTICE, tri)["front"].tolist() == [0] and ray_mesh_reference(down_o, down, LATTICE, tri)["front"].tolist() == [1]
    assert ray_mesh_reference(o, d, LATTICE, tri[:, ::-1])["front"].tolist() == [1] and ray_mesh_reference(down_o, down, LATTICE, tri[:, ::-1])["front"].tolist() == [0]


def test_bary_and_hit_point():
    """bary sums to 1 within 2 ulp -- three float32 roundings of weights that sum to 1 within 2^-52 -- and o + t d lies within
    (HIT_UM + 2) u M per axis of the bary-mixed corners: HIT_UM for the rule (derived above), 1.5 for the roundings of the weights,
    each on a corner of at most M, the rest for the float64 evaluation here."""
    for name in ("ball", "ball:+100", "soup:513x257", "coarse_ball"):
        o, d, v, f, _, _ = case(name)
        got = reference(name)
        won = got["face"] >= 0
        assert won.sum() > len(o) // 4, name
        bary = got["bary"][won].astype(np.float64)
        assert np.abs(bary.sum(axis=1) - 1).max() <= 2 * 2.0 ** -23 and (bary >= 0).all(), name
        c = v[f[got["face"][won]]].astype(np.float64)
        mixed = (bary[:, :, None] * c).sum(axis=1)
        point = o[won].astype(np.float64) + got["t"][won].astype(np.float64)[:, None] * d[won].astype(np.float64)
        M = np.maximum(np.abs(o[won]).max(axis=1), np.abs(c).max(axis=(1, 2))).astype(np.float64)
        ratio = np.abs(point - mixed).max(axis=1) / (U24 * M)
        print(f"{name}: o + t d lies at most {ratio.max():.3f} u M from the mixed corners; the bound is {HIT_UM + 2}")
        assert ratio.max() <= HIT_UM + 2, name
        assert not got["bary"][~won].any() and not got["front"][~won].any() and np.isposinf(got["t"][~won]).all()


def test_what_does_not_count():
    o, d = np.float32([[-1, 0, 0], [1, 0, 0], [np.nan, 0, 0], [-1, 0, 0], [-1, 0, 0], [-1, np.inf, 0]]), np.float32([[0, 0, 1]] * 3 + [[0, 0, 0], [0, np.nan, 1], [0, 0, 1]])
    v = np.concatenate([LATTICE, np.float32([[np.nan, 0, 5], [np.inf, 0, 5], [0, 0, 5]])])
    # indices outside [0, V), NaN and infinite vertices, a face of no area (three corners in a line): only the last two faces are left
    faces = np.int32([[0, 1, 7], [-1, 1, 2], [0, 1, 4], [0, 1, 5], [2 ** 31 - 1, 0, 1], [0, 1, 6], [0, 0, 2], [0, 1, 2], [1, 0, 3]])
    got = ray_mesh_reference(o, d, v, faces)
    assert got["face"].tolist() == [7, 8, -1, -1, -1, -1] and got["t"].tolist() == [5.0, 5.0] + [np.inf] * 4
    assert not got["bary"][2:].any() and not np.signbit(got["bary"]).any() and got["front"].tolist() == [0] * 6          # the two faces are wound alike: both seen from behind
    for nothing in (np.zeros((0, 3), np.int32), faces[:7]):
        got = ray_mesh_reference(o, d, v, nothing)
        assert got["face"].tolist() == [-1] * 6 and np.isposinf(got["t"]).all() and not got["bary"].any() and not got["front"].any()
    assert ray_mesh_reference(o, d, np.zeros((0, 3), np.float32), np.int32([[0, 0, 0]]))["face"].tolist() == [-1] * 6
    got = ray_mesh_reference(o[:0], d[:0], v, faces)
    assert got["t"].shape == (0,) and got["face"].shape == (0,) and got["bary"].shape == (0, 3) and got["front"].shape == (0,)
    assert (got["t"].dtype, got["face"].dtype, got["bary"].dtype, got["front"].dtype) == (np.float32, np.int32, np.float32, np.int8)
    with pytest.raises(ValueError):
        ray_mesh_reference(o[:, :2], d, v, faces)
    with pytest.raises(ValueError):
        ray_mesh_reference(o, d[:3], v, faces)
    with pytest.raises(ValueError, match="integers"):
        ray_mesh_reference(o, d, v, np.float32([[0, 1, 2]]))


def test_outputs_of_the_references():
    for name in CASES:
        (o, d, v, f, t_min, t_max), out = case(name), reference(name)
        assert out["t"].shape == (len(o),) and out["face"].shape == (len(o),) and out["bary"].shape == (len(o), 3) and out["front"].shape == (len(o),), name
        won = out["face"] >= 0
        assert (out["t"][won] >= np.float32(t_min)).all() and (out["t"][won] <= np.float32(t_max)).all() and np.isposinf(out["t"][~won]).all(), name
        assert (out["face"] < len(f)).all(), name
        if name.startswith("soup:513") or name in ("ball", "coarse_ball", "duplicates", "bad_indices", "lost", "limits", "behind", "needles"):
            assert won.sum() >= max(1, len(o) // 8) and (~won).any() == (len(o) > 3), name          # the cases are not empty; rays of the fourth kind mostly miss
        if name in ("all_invalid", "no_vertices", "no_faces"):
            assert not won.any(), name
    copies = reference("duplicates")["face"] // TILE
    assert not np.isin(copies[copies >= 0], (2, 4)).any() and (copies == 0).any()          # the copies in later tiles never win
    assert (reference("behind")["t"] < 0).any() and (reference("behind")["t"] > 0).any()
    plain, cut = ray_mesh_reference(*case("limits")[:4]), reference("limits")
    assert ((plain["t"] < 0.25) & (plain["face"] >= 0)).any() and ((plain["t"] > 1.0) & (plain["face"] >= 0)).any()          # both limits cut something
    assert (cut["face"] != plain["face"]).any()
    assert (reference("bad_rays")["face"][[0, 1, 2, 5, 6, 7, 10, 11]] == -1).all() and (reference("bad_rays")["face"][[3, 8, 13]] >= 0).any()


# ---- the per-lane code on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/raycast_host.cpp, the per-lane functions of csrc/raycast.h as plain loops, built with the host compiler, its address and
    undefined-behaviour sanitizers and without FMA contraction: a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("raycast_host") / "raycast_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CSRC, "raycast_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_on_the_host(program, tmp_path, name, reverse, wave=False):
    o, d, v, f, t_min, t_max = case(name)
    R = len(o)
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([R, len(v), len(f)], dtype="<i4").tobytes() + np.array([t_min, t_max], dtype="<f4").tobytes())
        fh.write(np.ascontiguousarray(o).tobytes() + np.ascontiguousarray(d).tobytes() + np.ascontiguousarray(v).tobytes() +
                 np.ascontiguousarray(f, dtype="<i4").tobytes())
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + (["reverse"] if reverse else []) +
                       (["wave"] if wave else []), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    assert len(raw) == 2 * 21 * R + 24
    results = []
    for half in range(2):
        at = half * 21 * R
        results.append({"t": np.frombuffer(raw, "<f4", R, at), "face": np.frombuffer(raw, "<i4", R, at + 4 * R),
                        "bary": np.frombuffer(raw, "<f4", 3 * R, at + 8 * R).reshape(R, 3), "front": np.frombuffer(raw, "i1", R, at + 20 * R)})
    violations, evaluated, pairs = np.frombuffer(raw, "<i8", 3, 42 * R).tolist()
    return results[0], results[1], violations, evaluated, pairs


@pytest.mark.parametrize("name", CASES)
def test_the_lanes_on_the_host(host_program, tmp_path, name):
    """Every face through the packed-key minimum and the kernel's culled walk give the reference's bits, with the schedule forward and
    reversed and with the faces themselves in descending order (the reference of those faces: the answers are renumbered, and among
    equal t the lowest new index wins); and every hit of every (ray, face) lies in a tile that a lane with that t as its best keeps."""
    for faces in (name, "reversed|" + name):
        for reverse in (False, True):
            every, culled, violations, evaluated, pairs = run_on_the_host(host_program, tmp_path, faces, reverse)
            hold(every, faces, f"{faces} reverse {reverse}, every face")
            hold(culled, faces, f"{faces} reverse {reverse}, culled")
            assert violations == 0, (faces, reverse, violations)
            assert pairs == len(case(name)[0]) * -(-len(case(name)[3]) // TILE) and 0 <= evaluated <= pairs
    # the same rays see the same surface whichever way the faces are numbered: equal t (the faces may differ where two tie)
    assert np.array_equal(reference(name)["t"], reference("reversed|" + name)["t"]), name
    if name == "ball":
        print(f"{name}: a wave of one lane evaluates {evaluated} of {pairs} (ray, tile) pairs")
        assert evaluated < pairs // 2


# The schedule of the culled walk, which no output bit shows: case -> the (wave, tile) pairs that the waves of WAVE
# consecutive rays evaluate, as given, and the waves times the tiles they are out of.  The host program with `wave` counted them;
# test_the_schedule_of_a_wave holds the program to them and tests/test_gpu_raycast.py the kernel.  The sphere's 257 rays are of
# four kinds in turn, from all around it, so a wave of them reaches most tiles: a wave of one lane evaluates 1117 of 9766
SCHEDULE = {"ball": (151, 5 * 38), "soup:257x257": (9, 5 * 2)}


def test_the_schedule_of_a_wave(host_program, tmp_path):
    for name, (count, pairs) in SCHEDULE.items():
        o, _, _, f = case(name)[:4]
        waves, tiles = -(-len(o) // WAVE), -(-len(f) // TILE)
        assert waves > 1 and tiles > 1 and pairs == waves * tiles and waves < count < pairs, name
        every, culled, violations, evaluated, of = run_on_the_host(host_program, tmp_path, name, False, wave=True)
        hold(every, name, f"{name} in waves, every face")
        hold(culled, name, f"{name} in waves, culled")
        print(f"{name}: waves of {WAVE} lanes evaluate {evaluated} of {of} (wave, tile) pairs")
        assert (violations, evaluated, of) == (0, count, pairs), name


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_knows_the_constants():
    from npcd import hip
    from npcd.hip import mesh_distance, raycast
    source = open(f"{CSRC}/raycast.h").read()
    assert int(re.search(r"constexpr int kRcThreads = (\d+);", source).group(1)) == raycast.WAVE_RAYS == WAVE
    assert raycast.TILE_FACES == mesh_distance.TILE_FACES == TILE
    assert "kRcMaxRays = (int64_t)1 << 31" in source and raycast.MAX_RAYS == 2 ** 31
    assert raycast.MAX_FACES == mesh_distance.MAX_FACES and raycast.MAX_VERTICES == mesh_distance.MAX_VERTICES
    assert hip.cast_rays is raycast.cast_rays and hip.mesh_boxes is mesh_distance.mesh_boxes
    # the slack of DESIGN.md 5.19: 4 times the 8 ulp of mesh_distance.h, at least 2^-100; tame rays have 2^-40 <= |d[kz]| <= 2^40
    assert float(re.search(r"kRcSlack = ([0-9.]+)f;", source).group(1)) == 4.0
    bits = {k: int(x, 16) for k, x in re.findall(r"(kRc\w+Bits) = (0x[0-9a-f]+)u", source)}
    as_float = lambda u: float(np.uint32(u).view(np.float32))
    assert (as_float(bits["kRcSlackFloorBits"]), as_float(bits["kRcTameLoBits"]), as_float(bits["kRcTameHiBits"])) == (2.0 ** -100, 2.0 ** -40, 2.0 ** 40)


def test_kernels_use_no_scratch(tmp_path):
    kernels = _compile("raycast.hip", str(tmp_path / "raycast.s"))
    assert len(kernels) == 2, sorted(kernels)
    for name, k in kernels.items():          # one tile of corners, 256 faces x 3 x 16 bytes; 4 waves to a SIMD at up to 128 registers
        assert "rc_query_kernel" in name and k["scratch"] == 0 and k["lds"] == TILE * 3 * 16 == 12288 and k["vgpr"] <= 128, (name, k)


def test_header_exports_and_signatures():
    from npcd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "npcd_hip.h")).read()
    L = hip.lib()
    name = "npcd_raycast_query"
    assert re.search(rf"\b{name}\(", header) and name in hip.SIGNATURES and hasattr(L, name)
    assert L.npcd_missing == () and L.npcd_abi_version() == 10
    assert len(hip.SIGNATURES[name][1]) == 17 and hip.SIGNATURES[name][1][8:11] == [ctypes.c_float, ctypes.c_float, ctypes.c_int]
    # the host-side refusals, which look at no pointer's target and launch nothing
    V, F, R = 1000, 3000, 500
    one = ctypes.c_void_p(64)          # never followed: every call below is refused before a launch

    def refused(**changed):
        #    origins, directions, R, vertices, V, faces, F, ws, t_min, t_max, cull, t, face, bary, front, evaluated, stream
        a = [one, one, R, one, V, one, F, one, 0.0, 1.0, 1, one, one, one, one, None, None]
        for i, value in changed.items():
            a[int(i[1:])] = value
        return L.npcd_raycast_query(*a)
    for missing in (0, 1, 7, 11, 12, 13, 14):
        assert refused(**{f"_{missing}": None}) == -1, missing
    for slot, bad in ((2, 0), (2, -1), (6, 0), (4, -1), (10, 2), (10, -1)):
        assert refused(**{f"_{slot}": bad}) == -1, (slot, bad)
    assert refused(_7=ctypes.c_void_p(72)) == -1          # the workspace: 16-byte aligned
    assert refused(_15=ctypes.c_void_p(68)) == -1         # the counter: 8-byte aligned
    assert refused(_0=ctypes.c_void_p(66)) == -1 and refused(_13=ctypes.c_void_p(66)) == -1
    for slot, bad in ((2, 2 ** 31), (4, 2 ** 31), (6, 2 ** 28)):
        assert refused(**{f"_{slot}": bad}) == -2, (slot, bad)
    assert refused(_2=2 ** 31, _0=None) == -2          # unsupported before a missing pointer


def test_wrapper_argument_errors():
    from npcd.hip.mesh_distance import mesh_boxes
    from npcd.hip.raycast import cast_rays
    o, d, v, f = (torch.from_numpy(a) for a in case("soup:255x257")[:4])
    with pytest.raises(RuntimeError, match="GPU"):
        cast_rays(o, d, v, f)                                                   # not on the GPU: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        cast_rays(o[:0], d[:0], v, f)
    with pytest.raises(RuntimeError, match="GPU"):
        mesh_boxes(v, f)
    for bad in ((o.numpy(), d, v, f), (o, d.numpy(), v, f), (o, d, v.numpy(), f), (o, d, v, f.numpy()), (o[:, :2], d, v, f), (o, d[:, :2], v, f),
                (o, d, v.reshape(-1), f), (o, d, v, f[:, :2]), (o[None], d, v, f), (o, d[:5], v, f)):
        with pytest.raises(ValueError):
            cast_rays(*bad)
    for bad in ((v.numpy(), f), (v[:, :2], f), (v, f[:, :2]), (v, f[:0])):
        with pytest.raises(ValueError):
            mesh_boxes(*bad)
    with pytest.raises(ValueError, match=rf"{2 ** 28} faces"):
        cast_rays(o, d, v, torch.zeros(1, 3, dtype=torch.int32).expand(2 ** 28, 3))
    with pytest.raises(ValueError, match=rf"{2 ** 31} rays"):
        cast_rays(torch.zeros(1, 3).expand(2 ** 31, 3), torch.zeros(1, 3).expand(2 ** 31, 3), v, f)


# ---- what users call, with stand-ins -------------------------------------------------------------------------------------------------------
def caster(origins, directions, vertices, faces, boxes=None):
    """Stands in for npcd.hip.raycast.cast_rays."""
    return {k: torch.from_numpy(a) for k, a in ray_mesh_reference(origins.numpy(), directions.numpy(), vertices.numpy(), faces.numpy()).items()}


def raygen(extrinsics, intrinsics, resolution, box):
    """Stands in for npcd.hip.render.ray_gen with a parallel projection along +z: pixel (row, column) starts at (column, row, 0) and
    the ray ends at t1 = 10.  The cameras are not looked at."""
    T = extrinsics.shape[0]
    row, col = torch.meshgrid(torch.arange(resolution), torch.arange(resolution), indexing="ij")
    o = torch.stack([col.reshape(-1).float(), row.reshape(-1).float(), torch.zeros(resolution * resolution)], dim=1)
    d = torch.tensor([0.0, 0.0, 1.0]).expand_as(o)
    return o.expand(T, -1, -1), d.expand(T, -1, -1), torch.zeros(T, resolution * resolution), torch.full((T, resolution * resolution), 10.0)


# a square in the plane z = 5 over [-0.5, 1.5]^2: the parallel rays of a 4 x 4 image hit it at pixels (0..1, 0..1), four of sixteen
SQUARE = (torch.tensor([[-0.5, -0.5, 5.0], [1.5, -0.5, 5.0], [1.5, 1.5, 5.0], [-0.5, 1.5, 5.0]]), torch.tensor([[0, 2, 1], [0, 3, 2]], dtype=torch.int32))
CAMERAS = (torch.eye(4)[None].repeat(2, 1, 1), torch.eye(3)[None].repeat(2, 1, 1))


def test_render_mesh_with_stand_ins():
    colours = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 1.0]])
    view = render_mesh(SQUARE, *CAMERAS, resolution=4, cube_scale=1.0, caster=caster, raygen=raygen)
    assert {k: tuple(t.shape) for k, t in view.items()} == {"mask": (2, 16, 1), "depth": (2, 16, 1), "face": (2, 16), "normal": (2, 16, 3), "channels": (2, 16, 3)}
    covered = torch.zeros(4, 4, dtype=torch.bool)
    covered[:2, :2] = True
    for t in range(2):
        assert torch.equal(view["mask"][t, :, 0], covered.reshape(-1).float())
        assert torch.equal(view["depth"][t, :, 0], torch.where(covered.reshape(-1), torch.tensor(5.0), torch.tensor(10.0)))          # a miss: the ray's end
        assert torch.equal(view["face"][t] >= 0, covered.reshape(-1))
    # the faces are wound to face the rays: the unit normal is (0, 0, -1), and a head light gives the grey itself; misses are white
    hit = view["mask"][0, :, 0] > 0
    assert torch.equal(view["normal"][0][hit], torch.tensor([0.0, 0.0, -1.0]).expand(4, 3)) and not view["normal"][0][~hit].any()
    assert torch.equal(view["channels"][0][hit], torch.full((4, 3), 0.75)) and torch.equal(view["channels"][0][~hit], torch.ones(12, 3))
    black = render_mesh(SQUARE, *CAMERAS, resolution=4, cube_scale=1.0, white_back=False, caster=caster, raygen=raygen)
    assert not black["channels"][0][~hit].any() and torch.equal(black["channels"][0][hit], view["channels"][0][hit])
    # colours and normals of the mesh are mixed with the barycentric weights: pixel (0, 0) lies on the diagonal of the square, a
    # quarter of the way from corner 0 to corner 2
    mesh = {"vertices": SQUARE[0], "faces": SQUARE[1], "colors": colours, "normals": torch.tensor([[0.0, 0, -2.0]]).expand(4, 3).contiguous()}
    mixed = render_mesh(mesh, *CAMERAS, resolution=4, cube_scale=1.0, caster=caster, raygen=raygen)
    assert torch.allclose(mixed["channels"][0, 0], torch.tensor([0.75, 0.0, 0.25]), atol=1e-6)
    assert torch.equal(mixed["normal"][0][hit], torch.tensor([0.0, 0.0, -1.0]).expand(4, 3))          # normalised again
    again = render_mesh(mesh, *CAMERAS, resolution=4, cube_scale=1.0, caster=caster, raygen=raygen)
    assert all(torch.equal(mixed[k], again[k]) for k in mixed)
    # 8 x 8 blocks are a permutation: a 16 x 16 image (four blocks) against one cast in row-major order
    big = render_mesh(mesh, *CAMERAS, resolution=16, cube_scale=1.0, caster=caster, raygen=raygen)
    o, d, _, _ = raygen(CAMERAS[0], CAMERAS[1], 16, 1.0)
    assert torch.equal(big["face"][1], caster(o[1], d[1], *SQUARE)["face"]) and int((big["face"][1] >= 0).sum()) == 4
    with pytest.raises(ValueError, match="light"):
        render_mesh(SQUARE, *CAMERAS, resolution=4, cube_scale=1.0, light="sun", caster=caster, raygen=raygen)
    empty = render_mesh((SQUARE[0], SQUARE[1][:0]), *CAMERAS, resolution=4, cube_scale=1.0, caster=caster, raygen=raygen)
    assert not empty["mask"].any() and (empty["face"] == -1).all() and torch.equal(empty["channels"], torch.ones(2, 16, 3))


class _Rendered:
    """Stands in for PointNeRF: render() gives back the images it was made with; its renderer has the two settings render_mesh asks for."""
    class renderer:
        cube_scale, white_back = 1.0, True

    def __init__(self, mask, depth, channels):
        self.out = {"mask": mask[None], "depth": depth[None], "channels": channels[None]}

    def render(self, coords, feats, extrinsics, intrinsics, resolution=128):
        return self.out


def metrics(pred, target, layout="chw"):
    """Stands in for npcd.hip.image_metrics.image_metrics: the mean squared error in float64, and an SSIM of 1 where the images are
    equal and 0 elsewhere."""
    from npcd.hip.image_metrics import ImageMetrics
    assert layout == "hwc" and pred.shape == target.shape and pred.dim() == 4
    mse = ((pred.double() - target.double()) ** 2).flatten(1).mean(dim=1)
    return ImageMetrics(mse, (mse == 0).double(), None, None)


def test_mesh_render_agreement_with_stand_ins():
    kw = dict(resolution=4, caster=caster, raygen=raygen, metrics=metrics)
    view = render_mesh(SQUARE, *CAMERAS, resolution=4, cube_scale=1.0, caster=caster, raygen=raygen)
    same = mesh_render_agreement(_Rendered(view["mask"], view["depth"], view["channels"]), None, None, SQUARE, *CAMERAS, **kw)
    assert sorted(same) == ["depth_max", "depth_mean", "iou", "psnr", "ssim", "views"] and len(same["views"]) == 2
    assert same["iou"] == 1.0 and same["depth_mean"] == 0.0 and same["depth_max"] == 0.0 and same["ssim"] == 1.0 and same["psnr"] == math.inf
    assert all(v == {"iou": 1.0, "depth_mean": 0.0, "depth_max": 0.0, "psnr": math.inf, "ssim": 1.0} for v in same["views"])
    # renderer= stands in for pointnerf.render: the model then only says which cube and background its renderer has
    blank = _Rendered(torch.zeros(2, 16, 1), view["depth"], torch.zeros(2, 16, 3))
    assert mesh_render_agreement(blank, None, None, SQUARE, *CAMERAS, renderer=_Rendered(view["mask"], view["depth"], view["channels"]).render, **kw) == same
    # by hand: the mesh covers the pixels (0..1, 0..1), four; the field in view 0 covers rows 0..2 of column 1 above the 0.5 threshold and
    # (3, 3) below it: the intersection is {(0, 1), (1, 1)}, the union 4 + 3 - 2 = 5, IoU 2 / 5.  Its depths there are 5.5 and 7: |d|
    # = 0.5 and 2, mean 1.25, max 2.  In view 1 the field covers nothing: IoU 0 / 4, and no pixel to compare depths on.
    mask, depth = torch.zeros(2, 4, 4), torch.full((2, 4, 4), 10.0)
    mask[0, :3, 1], mask[0, 3, 3] = torch.tensor([0.9, 0.51, 1.0]), 0.5
    depth[0, :3, 1] = torch.tensor([5.5, 7.0, 3.0])
    channels = view["channels"].clone()
    channels[0, 0, 0] = 0.25          # one channel of one pixel moves by 0.5: mse = 0.25 / 48
    got = mesh_render_agreement(_Rendered(mask.reshape(2, 16, 1), depth.reshape(2, 16, 1), channels), None, None, SQUARE, *CAMERAS, **kw)
    first, second = got["views"]
    assert first["iou"] == 2 / 5 and first["depth_mean"] == 1.25 and first["depth_max"] == 2.0 and first["ssim"] == 0.0
    assert first["psnr"] == pytest.approx(10 * math.log10(48 / 0.25), rel=1e-12)
    assert second["iou"] == 0.0 and math.isnan(second["depth_mean"]) and math.isnan(second["depth_max"]) and second["psnr"] == math.inf
    assert got["iou"] == 0.2 and got["depth_mean"] == 1.25 and got["depth_max"] == 2.0 and got["ssim"] == 0.5          # means over the views that have a value
    # neither covers anything: the IoU of two empty silhouettes is 1
    nothing = mesh_render_agreement(_Rendered(torch.zeros(2, 16, 1), depth.reshape(2, 16, 1), channels), None, None, (SQUARE[0], SQUARE[1][:0]), *CAMERAS, **kw)
    assert nothing["iou"] == 1.0 and math.isnan(nothing["depth_mean"])


def test_extract_mesh_defaults_are_the_same_bytes(monkeypatch):
    """extract_mesh(agreement=None) gives what it gave before the option existed; agreement=(extrinsics, intrinsics) adds the report of
    mesh_render_agreement for the final mesh and changes nothing else."""
    import npcd.hip.isosurface as iso_module
    from npcd.eval.mesh import extract_mesh
    field = _Field()

    def isosurface(volume, level, origin, spacing, normals=False, gradient_of=None):
        v, f = marching_tetrahedra_reference(volume[0].numpy(), level, origin.numpy(), spacing.numpy())
        n = vertex_normals_reference(volume[0].numpy(), level, spacing.numpy())
        return [(torch.from_numpy(v), torch.from_numpy(f)) + ((torch.from_numpy(n),) if normals else ())]
    monkeypatch.setattr(iso_module, "isosurface", isosurface)
    seen = []

    def agreer(pointnerf, coords, feats, mesh, extrinsics, intrinsics, resolution=128):
        seen.append((mesh, extrinsics, intrinsics, resolution))
        return {"iou": 1.0}
    coords, feats = torch.zeros(1, 4, 3), torch.zeros(1, 4, 8)
    common = dict(resolution=12, level=0.0)
    (plain,) = extract_mesh(field, coords, feats, **common)
    (same,) = extract_mesh(field, coords, feats, agreement=None, **common)
    assert sorted(plain) == sorted(same) and "agreement" not in plain
    assert all(plain[k].numpy().tobytes() == same[k].numpy().tobytes() for k in plain)
    (asked,) = extract_mesh(field, coords, feats, agreement=CAMERAS, agreer=agreer, **common)
    assert set(asked) == set(plain) | {"agreement"} and asked["agreement"] == {"iou": 1.0}
    assert all(asked[k].numpy().tobytes() == plain[k].numpy().tobytes() for k in plain)
    assert len(seen) == 1 and seen[0][1] is CAMERAS[0] and seen[0][2] is CAMERAS[1] and torch.equal(seen[0][0]["vertices"], plain["vertices"])
    for bad in (CAMERAS[0], (CAMERAS[0],), 5):
        with pytest.raises(ValueError, match="agreement"):
            extract_mesh(field, coords, feats, agreement=bad, agreer=agreer, **common)
