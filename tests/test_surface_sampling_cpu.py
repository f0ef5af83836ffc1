"""Surface sampling without a GPU: the CPU restatement npcd.eval.mesh.surface_sample_reference against geometry and
statistics, not against itself -- points inside their faces, the area of a sphere, chi-square tests of uniformity -- and the exact
cases of the specification; the per-lane code of csrc/surface.h, the code the kernels run, built for the host with sanitizers
(csrc/surface_host.cpp) and held bit for bit to the reference on the meshes of the GPU test (tests/test_gpu_surface_sampling.py, which
imports them from here); the kernels' resources from the compiler's own output, the entry points' refusals, the wrappers' argument
errors and the raw point cloud file."""
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from npcd.eval.mesh import (face_weights_reference, marching_tetrahedra_reference, sample_mesh_clouds, surface_sample_reference,
                            vertex_normals_reference)
from test_isosurface_cpu import CENTRE, sphere_volume
from test_kernel_resources import CSRC, _compile

T, LDS_TILES = 256, 4096          # kSurfTile, kSurfLdsTiles of csrc/surface.h; test_the_wrappers_know_the_constants holds them to the source
SIZES = (1, 4, T - 1, T, T + 1, 2 * T + 1, 64 * T + 3)
SAMPLES = (1, 63, 64, 65, 2048)
BIG = T * LDS_TILES + 3          # one tile more than a sampling workgroup stages in LDS


# ---- meshes ------------------------------------------------------------------------------------------------------------------------------
def soup(F, seed=0, V=None):
    """A random triangle soup: fp32 vertices and random index triples (a repeated index gives a degenerate face)."""
    rng = np.random.default_rng(1000 * seed + F)
    V = V or max(3, min(F, 20000) // 2 + 3)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.integers(0, V, (F, 3)).astype(np.int32)


def dirty(F=300, seed=0):
    """A soup in which every third face is unusable: degenerate, through a NaN or an infinite vertex, or with an index outside [0, V)."""
    rng = np.random.default_rng(seed + 50)
    v = rng.standard_normal((64, 3)).astype(np.float32)
    f = np.stack([rng.choice(60, 3, replace=False) for _ in range(F)]).astype(np.int32)          # three different vertices, all finite
    v[60], v[61] = np.nan, np.inf
    bad = np.arange(0, F, 3)
    for j, i in enumerate(bad):
        f[i] = [(5, 5, 9), (60, 1, 2), (3, 61, 4), (-1, 2, 3), (1, 64, 2), (1, 2, 2 ** 31 - 1), (7, 8, 7)][j % 7]
    return v, f, bad


def sphere(G, radius=0.6):
    vol, origin, spacing = sphere_volume((G, G, G), radius=radius)
    v, f = marching_tetrahedra_reference(vol, 0.0, origin, spacing)
    return v, f, vertex_normals_reference(vol, 0.0, spacing)


def congruent(n=16):
    """n translates of one triangle with d = 1 exactly."""
    base = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    v = np.concatenate([base + np.float32([2 * j, 0, 0]) for j in range(n)])
    return v, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def one_large():
    """Face 2 has d = 2^40, the others d = 1: 2^-40 of the largest, weight 0."""
    v, f = congruent(5)
    v[6:9] = np.float32([[0, 0, 0], [2 ** 20, 0, 0], [0, 2 ** 20, 0]])
    return v, f


def draws(S, seed=1):
    """torch's fp32 uniform draws on the CPU: multiples of 2^-24 in [0, 1)."""
    return torch.rand((S, 3), generator=torch.Generator().manual_seed(seed)).numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(meshes: list of (vertices, faces), u [B, S, 3], normals: None, "face" or a list, attributes: None or a list).  The
    cases of the GPU test; the host program runs them first."""
    kind, _, arg = name.partition(":")
    normals = attributes = None
    if kind == "faces":          # every size at which the tiling takes another path
        meshes, S, normals = [soup(int(arg))], 65, "face"
    elif kind == "samples":
        meshes, S = [soup(2 * T + 1, 1)], int(arg)
    elif kind == "big":
        meshes, S = [soup(BIG)], 2048
    elif kind == "channels":
        meshes, S = [soup(2 * T + 1, 2)], 65
        attributes = [np.random.default_rng(int(arg)).standard_normal((len(meshes[0][0]), int(arg))).astype(np.float32)]
    elif kind == "batch":          # differing sizes, an empty and an all-degenerate member, vertex normals with rows that are not finite
        ball = sphere(9)
        empty = (np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32))
        flat = (soup(40)[0], np.full((40, 3), 7, np.int32))
        nothing = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
        meshes = [soup(700, 3), empty, ball[:2], flat, soup(1, 3), dirty()[:2], nothing, soup(T, 3), one_large()]
        S = 65
        rng = np.random.default_rng(7)
        normals = [ball[2] if b == 2 else rng.standard_normal(m[0].shape).astype(np.float32) for b, m in enumerate(meshes)]
        normals[0][::5] = 0.0          # a face whose three corners have no normal: 0 / 0
        normals[7][3], normals[7][4, 1] = np.nan, np.inf
        attributes = [rng.uniform(0, 1, (len(m[0]), 3)).astype(np.float32) for m in meshes]
    elif kind == "exact":
        tiny = (congruent(16)[0] * np.float32(2.0 ** -35), congruent(16)[1])          # n = 2^-70, n2 = 2^-140: a denormal under the root
        meshes, S = [congruent(16), dirty()[:2], one_large(), tiny], 16
    else:
        raise KeyError(name)
    u = np.stack([draws(S, seed=b + 1) for b in range(len(meshes))])
    if kind == "exact":
        u[:, :, 0] = np.arange(16, dtype=np.float32) / 16
        u[1:, 0, 0], u[1:, 15, 0] = 0.0, 1.0 - 2.0 ** -24
    elif S >= 4:          # the ends of the range, a draw beyond them and one that is no number
        u[:, 0, 0], u[:, 1, 0], u[:, 2, 0], u[:, 3, 0] = 0.0, 1.0 - 2.0 ** -24, 1.5, np.nan
    for a in [u] + [x for m in meshes for x in m]:
        a.setflags(write=False)
    return dict(meshes=meshes, u=u, normals=normals, attributes=attributes)


CASES = ([f"faces:{F}" for F in SIZES] + [f"samples:{S}" for S in SAMPLES] + [f"channels:{C}" for C in (1, 3, 16)] + ["batch", "exact", "big"])


def member_options(c, b):
    normals = c["normals"] if c["normals"] is None or isinstance(c["normals"], str) else c["normals"][b]
    return normals, (None if c["attributes"] is None else c["attributes"][b])


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> per member the dict of surface_sample_reference, computed once."""
    c = case(name)
    out = []
    for b, (v, f) in enumerate(c["meshes"]):
        normals, attributes = member_options(c, b)
        out.append(surface_sample_reference(v, f, c["u"][b], normals=normals, attributes=attributes))
    return out


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    as_int = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    np.testing.assert_array_equal(got.view(as_int), want.view(as_int), err_msg=what)


# ---- the reference against geometry --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [9, 17, 33])
def test_points_lie_in_their_faces(G):
    v, f, _ = sphere(G)
    got = surface_sample_reference(v, f, draws(4096, seed=G))
    p, face = got["points"].astype(np.float64), got["face"]
    assert got["points"].dtype == np.float32 and face.dtype == np.int32 and face.min() >= 0 and face.max() < len(f)
    c = v.astype(np.float64)[f[face]]
    e1, e2, q = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], p - c[:, 0]
    # q = a e1 + b e2 in the least-squares sense, by the normal equations in float64
    m11, m12, m22 = np.sum(e1 * e1, 1), np.sum(e1 * e2, 1), np.sum(e2 * e2, 1)
    r1, r2 = np.sum(q * e1, 1), np.sum(q * e2, 1)
    det = m11 * m22 - m12 * m12
    a, b = (m22 * r1 - m12 * r2) / det, (m11 * r2 - m12 * r1) / det
    bary = np.stack([1 - a - b, a, b], 1)
    off = np.linalg.norm(q - a[:, None] * e1 - b[:, None] * e2, axis=1).max()
    print(f"G {G}: barycentric coordinates in [{bary.min():.2e}, {bary.max():.7f}], off the plane by {off:.2e}")
    assert bary.min() >= -1e-6 and bary.max() <= 1 + 1e-6
    assert off < 1e-6


@pytest.mark.parametrize("radius", [0.6, 0.8])
def test_area_of_a_sphere(radius):
    v, f, _ = sphere(33, radius)
    area = surface_sample_reference(v, f, draws(1))["area"]
    exact = 4 * math.pi * radius ** 2
    # the mesh's own area in float64, to which the integer weights are exact to 2^-31 of the largest face each
    c = v.astype(np.float64)[f]
    mesh_area = 0.5 * np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1).sum()
    print(f"radius {radius}: area {area:.6f}, the mesh's in float64 {mesh_area:.6f}, 4 pi r^2 {exact:.6f} ({abs(area / exact - 1):.2%} off)")
    assert area.dtype == np.float64 and abs(area / exact - 1) < 0.01
    assert abs(area / mesh_area - 1) < 1e-5          # fp32 cross products of faces a 1/16 wide: a few 1e-7 each


def chi_square(observed, expected):
    keep = expected > 0
    assert observed[~keep].sum() == 0
    return float(np.sum((observed[keep] - expected[keep]) ** 2 / expected[keep]))


def test_the_reference_is_uniform_by_area():
    """65,536 draws on a sphere of radius 0.8.  By Archimedes' hat-box theorem z / r of a uniform point on a sphere is uniform on
    [-1, 1]: chi-square over 16 equal bins, 15 degrees of freedom, 0.999 quantile 37.70.  The counts of 64 groups of consecutive
    faces against their share of the weights: 63 degrees of freedom, 0.999 quantile 103.44."""
    radius, S = 0.8, 65536
    v, f, _ = sphere(33, radius)
    got = surface_sample_reference(v, f, draws(S, seed=1))
    z = (got["points"][:, 2].astype(np.float64) - CENTRE[2]) / radius
    bins = np.clip(np.floor((z + 1) * 8).astype(np.int64), 0, 15)
    by_height = chi_square(np.bincount(bins, minlength=16), np.full(16, S / 16))
    weights = face_weights_reference(v, f)[0].astype(np.float64)
    groups = np.array_split(np.arange(len(f)), 64)
    share = np.array([weights[g].sum() for g in groups]) / weights.sum()
    group_of = np.repeat(np.arange(64), [len(g) for g in groups])
    by_group = chi_square(np.bincount(group_of[got["face"]], minlength=64), S * share)
    print(f"chi-square of z / r in 16 bins {by_height:.1f} (bound 37.70), of 64 face groups {by_group:.1f} (bound 103.44)")
    assert by_height < 37.70
    assert by_group < 103.44


# ---- the exact cases -----------------------------------------------------------------------------------------------------------------------
def test_exact_cases():
    tri, messy, large, tiny = reference("exact")
    c = case("exact")
    # u0 = j / 16 on 16 congruent faces: r = j 2^31 is the sum before face j, which does not exceed it -- the boundary goes up
    assert tri["face"].tolist() == list(range(16))
    w, k, d, _ = face_weights_reference(*c["meshes"][0])
    assert k == 31 and (w == 2 ** 31).all() and (d == 1).all() and tri["area"] == 8.0
    # u0 = 0 and u0 = 1 - 2^-24: the first and the last face that weighs anything
    v, f, bad = dirty()
    w = face_weights_reference(v, f)[0]
    assert (w[bad] == 0).all() and bad[0] == 0 and np.count_nonzero(w) == len(f) - len(bad)
    usable = np.nonzero(w)[0]
    assert messy["face"][0] == usable[0] == 1 and messy["face"][15] == usable[-1]
    many = surface_sample_reference(v, f, draws(20000, seed=3))
    assert (w[many["face"]] > 0).all() and not np.isin(many["face"], bad).any() and np.isfinite(many["points"]).all()
    assert len(np.unique(many["face"])) > 150
    # one face 2^40 times the rest
    w, k, _, _ = face_weights_reference(*c["meshes"][2])
    assert w.tolist() == [0, 0, 2 ** 31, 0, 0] and k == 31 - 40
    assert (large["face"] == 2).all() and large["area"] == 2.0 ** 39
    # no measure
    for v, f in ((np.zeros((5, 3), np.float32), np.zeros((0, 3), np.int32)), (soup(40)[0], np.full((40, 3), 7, np.int32)),
                 (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), (np.zeros((0, 3), np.float32), np.zeros((4, 3), np.int32))):
        got = surface_sample_reference(v, f, draws(5), normals="face", attributes=np.ones((len(v), 2), np.float32))
        assert (got["face"] == -1).all() and got["area"] == 0.0 and got["area"].dtype == np.float64
        for key in ("points", "normals", "attributes"):
            assert got[key].dtype == np.float32 and (got[key].view(np.int32) == 0).all(), key
        assert got["attributes"].shape == (5, 2)
    # a draw outside [0, 1) is clamped, one that is no number counts as 0
    got = surface_sample_reference(*congruent(16), np.float32([[-3, .5, .5], [np.nan, .5, .5], [1, .5, .5], [7, .5, .5], [np.inf, .5, .5]]))
    assert got["face"].tolist() == [0, 0, 15, 15, 15]
    # a denormal n2 is not flushed: d = 2^-70 exactly, and the faces weigh what their translates weigh
    w, k, d, _ = face_weights_reference(*c["meshes"][3])
    assert (d == np.float32(2.0 ** -70)).all() and k == 31 + 70 and (w == 2 ** 31).all()
    assert tiny["face"].tolist() == list(range(16)) and tiny["area"] == 8.0 * 2.0 ** -70
    v, f = congruent(3)
    with pytest.raises(ValueError):
        surface_sample_reference(v, f, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        surface_sample_reference(v, f, draws(2), normals="vertex")


def test_outputs_of_the_reference():
    (got,) = reference("faces:513")
    v, f = case("faces:513")["meshes"][0]
    assert set(got) == {"points", "face", "area", "normals"}
    length = np.linalg.norm(got["normals"].astype(np.float64), axis=1)
    assert np.abs(length - 1).max() < 2e-7
    c = v.astype(np.float64)[f[got["face"]]]
    winding = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    assert (np.sum(winding * got["normals"], axis=1) > 0).all()
    # the sphere's vertex normals, interpolated, still point outward; colours stay inside their range
    sv, sf, sn = sphere(9)
    colours = np.random.default_rng(0).uniform(0, 1, (len(sv), 3)).astype(np.float32)
    got = surface_sample_reference(sv, sf, draws(500), normals=sn, attributes=colours)
    radial = got["points"].astype(np.float64) - CENTRE
    assert (np.sum(radial * got["normals"], axis=1) / np.linalg.norm(radial, axis=1) > 0.99).all()
    assert got["attributes"].min() >= 0 and got["attributes"].max() <= 1 + 1e-6
    # a batch member's zero and non-finite vertex normals give zero rows, by the bits
    batch = reference("batch")
    rows = batch[0]["normals"]
    zero = (rows.view(np.int32) == 0).all(axis=1)
    assert zero.any() and not zero.all() and np.isfinite(rows).all() and np.isfinite(batch[7]["normals"]).all()
    assert [int(m["face"].max()) for m in batch][1:4:2] == [-1, -1] and batch[6]["area"] == 0.0


# ---- the per-lane code on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/surface_host.cpp, the per-lane functions of csrc/surface.h as plain loops, built with the host compiler, its address and
    undefined-behaviour sanitizers and without FMA contraction: a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("surface_host") / "surface_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CSRC, "surface_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def pack(c):
    """-> (vertices, faces, vert_offsets, face_offsets, normals mode, vertex normals or None, attributes or None) of a case's batch."""
    meshes = c["meshes"]
    offsets = [np.cumsum([0] + [len(m[i]) for m in meshes]).astype(np.int32) for i in (0, 1)]
    vertices = np.concatenate([m[0] for m in meshes]).astype(np.float32).reshape(-1, 3)
    faces = np.concatenate([m[1] for m in meshes]).astype(np.int32).reshape(-1, 3)
    mode = 0 if c["normals"] is None else 1 if isinstance(c["normals"], str) else 2
    vn = np.concatenate(c["normals"]).astype(np.float32) if mode == 2 else None
    at = np.concatenate(c["attributes"]).astype(np.float32) if c["attributes"] is not None else None
    return vertices, faces, offsets[0], offsets[1], mode, vn, at


def run_on_the_host(program, tmp_path, name, reverse):
    c = case(name)
    vertices, faces, vo, fo, mode, vn, at = pack(c)
    B, S = c["u"].shape[:2]
    C = 0 if at is None else at.shape[1]
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array([B, S, C, mode, len(vertices), len(faces)], dtype="<i4").tobytes() + vo.tobytes() + fo.tobytes())
        for a in (vertices, faces, c["u"], vn, at):
            if a is not None:
                fh.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + (["reverse"] if reverse else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = open(tmp_path / "out.bin", "rb").read()
    out, at_byte = {}, 0
    for key, dtype, shape in (("area", "<f8", (B,)), ("points", "<f4", (B, S, 3)), ("face", "<i4", (B, S)),
                              ("normals", "<f4", (B, S, 3) if mode else None), ("attributes", "<f4", (B, S, C) if C else None)):
        if shape is None:
            continue
        count = int(np.prod(shape))
        out[key] = np.frombuffer(raw, dtype=dtype, count=count, offset=at_byte).reshape(shape)
        at_byte += count * np.dtype(dtype).itemsize
    assert at_byte == len(raw)
    return out


def hold(got, name, what):
    """got: key -> [B, ...] arrays of a whole batch; every output of every member equals the reference's, bit for bit."""
    for b, want in enumerate(reference(name)):
        assert set(got) == set(want), (what, sorted(got), sorted(want))
        for key in want:
            same_bits(got[key][b], want[key], f"{what}: {key} of member {b}")


@pytest.mark.parametrize("name", CASES)
def test_the_lanes_on_the_host(host_program, tmp_path, name):
    for reverse in (False, True):
        hold(run_on_the_host(host_program, tmp_path, name, reverse), name, f"{name} reverse {reverse}")


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrappers_know_the_constants():
    from npcd import hip
    from npcd.hip import surface
    source = open(f"{CSRC}/surface.h").read()
    assert int(re.search(r"constexpr int kSurfTile = (\d+);", source).group(1)) == surface.TILE_FACES == T
    assert int(re.search(r"constexpr int kSurfLdsTiles = (\d+);", source).group(1)) == surface.LDS_TILES == LDS_TILES
    assert int(re.search(r"constexpr int kSurfMaxChannels = (\d+);", source).group(1)) == surface.MAX_CHANNELS == 16


def test_kernels_use_no_scratch(tmp_path):
    kernels = _compile("surface.hip", str(tmp_path / "surface.s"))
    assert len(kernels) == 4, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (name, k)
        # the staged tile sums of the sample launch; the four wave totals of a workgroup's scan
        assert k["lds"] == (8 * LDS_TILES if "surf_sample" in name else 0 if "surf_measure" in name else 32), (name, k)
    text = open(tmp_path / "surface.s").read()
    assert "global_atomic_umax" in text and "cmpswap" not in text          # the one atomic is one instruction, not a compare-and-swap loop


def test_header_exports_and_signatures():
    import ctypes

    from npcd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "npcd_hip.h")).read()
    L = hip.lib()
    names = ("npcd_surface_ws_bytes", "npcd_surface_prepare", "npcd_surface_sample")
    for name in names:
        assert re.search(rf"\b{name}\(", header) and name in hip.SIGNATURES and hasattr(L, name), name
    assert L.npcd_missing == () and L.npcd_abi_version() == 10
    assert hip.SIGNATURES["npcd_surface_ws_bytes"][0] is ctypes.c_int64
    assert len(hip.SIGNATURES["npcd_surface_prepare"][1]) == 10 and len(hip.SIGNATURES["npcd_surface_sample"][1]) == 19
    # the host-side refusals, which look at no pointer's target and launch nothing
    F, B = 1000, 3
    slots = F // T + B
    assert L.npcd_surface_ws_bytes(B, F) == 8 * (F + slots + B) + 4 * (F + B)
    assert L.npcd_surface_ws_bytes(1, 0) == 8 * 2 + 4
    assert L.npcd_surface_ws_bytes(0, 10) == -1 and L.npcd_surface_ws_bytes(1, -1) == -1
    assert L.npcd_surface_ws_bytes(1, 2 ** 31) == -2 and L.npcd_surface_ws_bytes(1, 2 ** 31 - 1) > 0
    one = ctypes.c_void_p(64)          # never followed: every call below is refused before a launch
    prepare = [one] * 4 + [1, 10, 10, one, one, None]
    assert L.npcd_surface_prepare(*prepare[:4], 0, *prepare[5:]) == -1
    assert L.npcd_surface_prepare(*prepare[:5], 2 ** 31, *prepare[6:]) == -2
    assert L.npcd_surface_prepare(*prepare[:6], 2 ** 31, *prepare[7:]) == -2
    assert L.npcd_surface_prepare(*prepare[:5], -1, *prepare[6:]) == -1
    for missing in (0, 1, 2, 3, 7, 8):
        assert L.npcd_surface_prepare(*[None if i == missing else a for i, a in enumerate(prepare)]) == -1, missing
    assert L.npcd_surface_prepare(*prepare[:7], ctypes.c_void_p(68), *prepare[8:]) == -1          # ws not 8-byte aligned
    #        vertices .. face_offsets, B, V, F, ws, u, S, points, faces_out, mode, vertex normals, normals_out, attributes, C, attributes_out
    sample = [one] * 4 + [1, 10, 10, one, one, 5, one, None, 0, None, None, None, 0, None, None]
    def refused(**changed):
        a = list(sample)
        for i, value in changed.items():
            a[int(i[1:])] = value
        return L.npcd_surface_sample(*a)
    assert refused(_4=0) == -1 and refused(_9=0) == -1 and refused(_16=-1) == -1 and refused(_12=3) == -1
    assert refused(_16=17, _15=one, _17=one) == -2 and refused(_5=2 ** 31) == -2 and refused(_6=2 ** 31) == -2
    assert refused(_4=65536) == -2 and refused(_4=40000, _9=40000) == -2
    for missing in (0, 1, 2, 3, 7, 8, 10):
        assert refused(**{f"_{missing}": None}) == -1, missing
    assert refused(_12=1) == -1 and refused(_14=one) == -1                     # face normals without an output; an output without a mode
    assert refused(_12=2, _14=one) == -1 and refused(_12=1, _14=one, _13=one) == -1          # vertex mode without normals; face mode with them
    assert refused(_16=3, _15=one) == -1 and refused(_16=3, _17=one) == -1 and refused(_15=one, _17=one) == -1


def test_wrapper_argument_errors():
    from npcd.hip.surface import sample_surface, surface_area
    v, f = (torch.from_numpy(a) for a in soup(10))
    for call in (lambda m: sample_surface(m, 4), surface_area):
        with pytest.raises(RuntimeError, match="GPU"):
            call((v, f))                                                       # not on the GPU: there is no CPU path
        with pytest.raises(RuntimeError, match="GPU"):
            call([(v, f), {"vertices": v, "faces": f}])
        with pytest.raises(ValueError):
            call((v[:, :2], f))
        with pytest.raises(ValueError):
            call((v, f.reshape(-1)))
        with pytest.raises(ValueError):
            call([])
        with pytest.raises(ValueError):
            call([(v,)])
        with pytest.raises(ValueError):
            call("mesh")
    with pytest.raises(ValueError, match="num_samples"):
        sample_surface((v, f), 0)


def test_clouds_and_the_raw_point_cloud_file(tmp_path):
    """sample_mesh_clouds with the reference standing in for the kernels, write_raw_pointcloud, and load_pointclouds on the file."""
    from npcd.data.pointclouds import load_pointclouds, write_raw_pointcloud
    from test_fps_cpu import _FirstK
    calls = []

    def stand_in(meshes, num_samples, generator=None, normals=None):
        calls.append((len(meshes), num_samples, normals is not None))
        rows = [surface_sample_reference(v.numpy(), f.numpy(), draws(num_samples), normals=None if normals is None else normals[b].numpy())
                for b, (v, f) in enumerate(meshes)]
        out = [torch.from_numpy(np.stack([r["points"] for r in rows])), torch.tensor([float(r["area"]) for r in rows], dtype=torch.float64)]
        return tuple(out + ([torch.from_numpy(np.stack([r["normals"] for r in rows]))] if normals is not None else []))
    sv, sf, sn = (torch.from_numpy(a) for a in sphere(9))
    other = tuple(torch.from_numpy(a) for a in soup(50))
    clouds = sample_mesh_clouds([(sv, sf), other], 40, sampler=stand_in)
    assert clouds.shape == (2, 40, 3) and clouds.dtype == torch.float32 and calls == [(2, 40, False)]
    as_dicts = [{"vertices": sv, "faces": sf, "normals": sn}, {"vertices": sv, "faces": sf, "normals": -sn}]
    points, normals = sample_mesh_clouds(as_dicts, 40, normals=True, sampler=stand_in)
    assert points.shape == normals.shape == (2, 40, 3) and calls[-1] == (2, 40, True)
    assert torch.equal(points[0], clouds[0]) and torch.equal(normals[0], -normals[1])
    assert sample_mesh_clouds((sv, sf, sn), 7, normals=True, sampler=stand_in)[1].shape == (1, 7, 3)          # one mesh as isosurface returns it
    with pytest.raises(ValueError, match="vertex normals"):
        sample_mesh_clouds([(sv, sf)], 40, normals=True, sampler=stand_in)
    path = write_raw_pointcloud(str(tmp_path / "object"), points[0], normals[0].numpy())
    assert os.path.basename(path) == "pointcloud3.npz"
    with np.load(path) as z:
        assert sorted(z.files) == ["normals", "points"] and z["points"].dtype == np.float32 and z["normals"].dtype == np.float32
        np.testing.assert_array_equal(z["points"], points[0].numpy())
    (loaded,) = load_pointclouds([str(tmp_path / "object")], 8, sampler=_FirstK(), device="cpu")
    assert torch.equal(loaded["points"], points[0][:8]) and torch.equal(loaded["normals"], normals[0][:8])
    for bad in ((points[0][:, :2], normals[0]), (points[0], normals[0][:5]), (points, normals)):
        with pytest.raises(ValueError):
            write_raw_pointcloud(str(tmp_path / "bad"), *bad)
