"""Inside tests for meshes without a GPU: the CPU restatement npcd.eval.mesh.crossings_reference against geometry --
the parity and the signed count of its crossings equal `volume > level` at every node of lattice volumes, along rays that pass
exactly through vertices and edges, where counting the inclusive hits of the first-hit rule is wrong -- and against the exact
properties of the rule on closed solids with integer corners; the per-lane code of csrc/raycast.h, the code the kernel runs, built
for the host with sanitizers (csrc/crossings_host.cpp) and held bit for bit to the reference on the cases of the GPU test
(tests/test_gpu_crossings.py, which imports them from here), with the culling bound checked against every counted crossing; the
kernel's resources from the compiler's own output, the entry point's refusals, the wrapper's argument errors, and voxelize_mesh,
mesh_signed_distance, mesh_volume_iou, mesh_enclosure and extract_mesh(enclosure=) with stand-ins."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from npcd.eval.mesh import crossings_reference, marching_tetrahedra_reference, vertex_normals_reference
from test_kernel_resources import CSRC, _compile

TILE, WAVE = 256, 64          # kMdTile of csrc/mesh_tiles.h and kRcThreads of csrc/raycast.h
LEVEL = 1.5
VOLUMES = ((9, 0), (12, 1))          # (G, seed)
DIRECTIONS = ((1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1), (-1, 1, -1), (1, 2, 3), (0.3, -0.9, 0.2))
FACES = (1, 255, 256, 257)          # one face, one below, at and above a tile
RAYS = (1, 63, 64, 65)              # one ray, one below, at and above a wave
KEYS = ("front", "back")


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(G, seed):
    """-> (volume [G, G, G] float32: random integers 0..3 inside a ball about the centre and 0 outside, its isosurface at LEVEL
    (vertices, faces), the G^3 nodes [G^3, 3] float32 in row-major order, x fastest).  The surface passes midway between nodes of
    values 1 and 2 and elsewhere, so rays from the nodes along lattice directions pass exactly through vertices and edges."""
    z, y, x = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    c = (G - 1) / 2
    ball = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 < (0.38 * G) ** 2
    vol = np.where(ball, np.random.default_rng(seed).integers(0, 4, size=[G, G, G]), 0).astype(np.float32)
    v, f = marching_tetrahedra_reference(vol, LEVEL)
    nodes = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float32)
    return vol, v, f.astype(np.int32), nodes


def cube(at=(0, 0, 0), size=2):
    """An axis-parallel cube with integer corners, wound outward: (vertices [8, 3] float32, faces [12, 3] int32)."""
    v = np.float32([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]) * np.float32(size) + np.float32(at)
    f = np.int32([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]])
    return v, f


def octahedron(r=2):
    v = np.float32([[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]])
    f = np.int32([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v, f


@functools.lru_cache(maxsize=None)
def cube_soup():
    """27 cubes of size 2 on a 3 x 3 x 3 grid of pitch 2 -- neighbours share whole sides, edges and corners -- 324 faces: a closed
    solid cut into rooms, and a mesh of which any prefix of faces is a case of its own."""
    parts = [cube((2 * x, 2 * y, 2 * z)) for z in range(3) for y in range(3) for x in range(3)]
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] + 8 * i for i, p in enumerate(parts)]).astype(np.int32))


def probes(lo, hi):
    """Origins on every half-integer and integer position of [lo, hi]^3, float32."""
    axis = np.arange(2 * lo, 2 * hi + 1) / 2.0
    z, y, x = np.meshgrid(axis, axis, axis, indexing="ij")
    return np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (origins [R, 3], directions [R, 3], vertices [V, 3] float32, faces [F, 3] int32, t_min, t_max)."""
    kind, _, arg = name.partition(":")
    limits = (0.0, float("inf"))
    if kind == "lattice":          # lattice:G:k -- the nodes of the G^3 volume along DIRECTIONS[k]
        G, k = (int(x) for x in arg.split(":"))
        _, v, f, nodes = lattice(G, dict(VOLUMES)[G])
        return nodes, np.broadcast_to(np.float32(DIRECTIONS[k]), nodes.shape).copy(), v, f, *limits
    if kind == "rooms":          # rooms:FxR -- the first F faces of the cube soup, R probes of it in the eight directions in turn
        F, R = (int(x) for x in arg.split("x"))
        v, f = cube_soup()
        o = probes(-1, 7)
        o = o[np.random.default_rng(F + R).permutation(len(o))[:R]]
        d = np.float32(DIRECTIONS)[np.arange(R) % len(DIRECTIONS)]
        return o, d, v, np.ascontiguousarray(f[:F]), *limits
    if kind == "bad_rays":          # NaN, infinite and zero directions, origins that are not finite
        o, d, v, f, _, _ = case("rooms:324x65")
        o, d = o.copy(), d.copy()
        d[0], d[5], d[9], d[14] = (0, 0, 0), (np.nan, 1, 0), (np.inf, 0.5, 0.5), (-0.0, 0.0, -0.0)
        o[2], o[7] = (np.nan, 0.5, 0.5), (0.5, -np.inf, 0.5)
        return o, d, v, f, *limits
    if kind == "limits":          # t_min > 0 and a finite t_max cut crossings away on both sides; behind: a negative t_min
        o, d, v, f, _, _ = case("rooms:324x257")
        return o, d, v, f, 0.5, 3.0
    if kind == "behind":
        o, d, v, f, _, _ = case("rooms:324x257")
        return o, d, v, f, -2.0, 1.0
    if kind == "bad_indices":
        o, d, v, f, _, _ = case("rooms:324x65")
        f = f.copy()
        f[3], f[50], f[300] = (-1, 2, 3), (1, len(v), 2), (1, 2, 2 ** 31 - 1)
        return o, d, v, f, *limits
    if kind == "no_faces":
        o, d, v, f, _, _ = case("rooms:324x65")
        return o, d, v, f[:0], *limits
    if kind == "no_rays":
        o, d, v, f, _, _ = case("rooms:324x65")
        return o[:0], d[:0], v, f, *limits
    raise KeyError(name)


GEOMETRY = [f"lattice:{G}:{k}" for G, _ in VOLUMES for k in range(len(DIRECTIONS))]
GPU_LATTICE = [f"lattice:12:{k}" for k in range(len(DIRECTIONS))]          # 3,632 faces = 15 tiles with a tail tile; 1,728 rays = 27 waves
EDGES = [f"rooms:{F}x65" for F in FACES] + [f"rooms:324x{R}" for R in RAYS if R != 65]
OTHERS = ["rooms:324x257", "bad_rays", "limits", "behind", "bad_indices", "no_faces", "no_rays"]
HOST_CASES = ["lattice:9:0", "lattice:9:4", "lattice:9:7"] + GPU_LATTICE + EDGES + OTHERS
GPU_CASES = GPU_LATTICE + EDGES + OTHERS


@functools.lru_cache(maxsize=None)
def reference(name):
    return crossings_reference(*case(name))


def hold(got, name, what):
    want = reference(name)
    for key in KEYS:
        assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), f"{what}: {key} differs at {np.nonzero(got[key] != want[key])[0][:8]}"


# ---- the rule against geometry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOMETRY)
def test_parity_is_the_volume(name):
    """At EVERY node, the parity of the crossings and the signed count back - front say what the volume says, although the rays run
    through vertices and along edges of the surface; the inclusive hits of the first-hit rule, counted, do not."""
    G = int(name.split(":")[1])
    vol = lattice(G, dict(VOLUMES)[G])[0]
    solid = (vol > LEVEL).reshape(-1)
    o, d, v, f, _, _ = case(name)
    assert len(o) == G ** 3 and (len(f), len(o)) == ((3632, 1728) if G == 12 else (len(f), 729))
    got = reference(name)
    parity = (got["front"] + got["back"]) % 2 == 1
    assert np.array_equal(parity, solid), np.nonzero(parity != solid)[0]
    assert np.array_equal(got["back"] - got["front"], solid.astype(np.int32))
    inclusive = crossings_reference(o, d, v, f, inclusive=True)
    wrong = int((((inclusive["front"] + inclusive["back"]) % 2 == 1) != solid).sum())
    print(f"{name}: {solid.sum()} of {len(solid)} nodes are solid; the crossings agree at every node, the inclusive hits are wrong at {wrong}")
    assert wrong > 0 and (inclusive["front"] >= got["front"]).all() and (inclusive["back"] >= got["back"]).all()


# ---- closed solids with integer corners --------------------------------------------------------------------------------------------------
SOLIDS = {"cube": (cube(), lambda p: ((p > 0) & (p < 2)).all(axis=1), lambda p: ((p >= 0) & (p <= 2)).all(axis=1)),
          "octahedron": (octahedron(), lambda p: np.abs(p).sum(axis=1) < 2, lambda p: np.abs(p).sum(axis=1) <= 2)}
# along the faces' planes and edges, through corners, and oblique
SOLID_DIRECTIONS = DIRECTIONS + ((-1, 0, 0), (0, 1, 0), (0, 0, -1), (1, -1, 0), (0, 1, 1), (-1, -1, -1), (1, -1, 1), (2, 1, 0))


# those whose shear is exact in fp32 (Sx, Sy and Sz are 0, 1 or a half): on these solids every number of the rule is then exact, a
# probe on the surface has t == 0 exactly, and the rule's own properties can be asked bit for bit
EXACT_DIRECTIONS = tuple(d for d in SOLID_DIRECTIONS if d not in ((1, 2, 3), (0.3, -0.9, 0.2)))


@functools.lru_cache(maxsize=None)
def solid_rays(solid, exact=False):
    o = probes(-1, 3) if solid == "cube" else probes(-3, 3)
    directions = EXACT_DIRECTIONS if exact else SOLID_DIRECTIONS
    return np.tile(o, (len(directions), 1)), np.repeat(np.float32(directions), len(o), axis=0)


@pytest.mark.parametrize("solid", sorted(SOLIDS))
def test_a_point_off_the_surface_is_inside_or_outside(solid):
    (v, f), inside, closed = SOLIDS[solid]
    o, d = solid_rays(solid)
    off = inside(o) | ~closed(o)          # not on the surface
    got = crossings_reference(o, d, v, f)
    parity = (got["front"] + got["back"]) % 2 == 1
    assert off.sum() > len(o) // 2 and np.array_equal(parity[off], inside(o)[off]), np.nonzero(off & (parity != inside(o)))[0][:8]
    assert np.array_equal((got["back"] - got["front"])[off], inside(o)[off].astype(np.int32))          # wound outward: one way out
    # a convex solid: a ray from outside crosses in and out or not at all, one from inside only out
    assert set(zip(got["front"][off].tolist(), got["back"][off].tolist())) == {(0, 0), (1, 1), (0, 1)}


@pytest.mark.parametrize("solid", sorted(SOLIDS))
def test_renumbering_and_flipping(solid):
    (v, f), _, _ = SOLIDS[solid]
    o, d = solid_rays(solid, exact=True)
    got = crossings_reference(o, d, v, f)
    rng = np.random.default_rng(3)
    for _ in range(3):          # renumbering the faces changes nothing
        again = crossings_reference(o, d, v, f[rng.permutation(len(f))])
        assert all(np.array_equal(again[k], got[k]) for k in KEYS)
    for k in range(len(f)):          # a face wound the other way: its front crossings become back crossings, and the parity stays
        alone, flipped = crossings_reference(o, d, v, f[k:k + 1]), crossings_reference(o, d, v, f[k:k + 1, ::-1])
        assert np.array_equal(alone["front"], flipped["back"]) and np.array_equal(alone["back"], flipped["front"]), k
        assert (alone["front"] + alone["back"]).max() == 1
        mixed = f.copy()
        mixed[k] = mixed[k, ::-1]
        whole = crossings_reference(o, d, v, mixed)
        assert np.array_equal(whole["front"] + whole["back"], got["front"] + got["back"]), k
        assert np.array_equal(whole["front"], got["front"] - alone["front"] + alone["back"]), k


@pytest.mark.parametrize("solid", sorted(SOLIDS))
def test_the_segments_add_up(solid):
    """[t_min, m] and [nextafter(m), t_max] hold every crossing of [t_min, t_max] once, also where t == m exactly."""
    (v, f), _, _ = SOLIDS[solid]
    o, d = solid_rays(solid, exact=True)
    for t_min, t_max in ((0.0, np.inf), (-4.0, 4.0)):
        whole = crossings_reference(o, d, v, f, t_min=t_min, t_max=t_max)
        for m in (0.0, 0.5, 1.0, 2.0):          # every one is the t of a crossing of some ray, exactly
            near = crossings_reference(o, d, v, f, t_min=t_min, t_max=m)
            far = crossings_reference(o, d, v, f, t_min=np.nextafter(np.float32(m), np.float32(np.inf)), t_max=t_max)
            assert all(np.array_equal(near[k] + far[k], whole[k]) for k in KEYS), (t_min, t_max, m)
            assert near["back"].sum() > 0 and far["back"].sum() > 0
    behind = crossings_reference(o, d, v, f, t_min=-np.inf, t_max=np.inf)          # the whole line: even for a closed solid, off it or on it
    assert ((behind["front"] + behind["back"]) % 2 == 0).all() and np.array_equal(behind["front"], behind["back"])


def test_what_does_not_count():
    v, f = cube()
    o = np.float32([[1, 1, 1]] * 7)
    o[5], o[6] = (np.nan, 1, 1), (1, np.inf, 1)
    d = np.float32([[1, 0, 0], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [-0.0, 0, 0], [1, 0, 0], [1, 0, 0]])
    got = crossings_reference(o, d, v, f)
    assert got["back"].tolist() == [1, 0, 0, 0, 0, 0, 0] and not got["front"].any()
    assert got["front"].dtype == np.int32 and got["back"].dtype == np.int32
    # a face of no area, a face with a vertex that is not finite, indices outside [0, V): none counts
    bad = np.int32([[0, 0, 1], [0, 1, 1], [0, 1, 8], [-1, 1, 2], [0, 1, 9]])
    vv = np.concatenate([v, np.float32([[np.nan, 0, 0]])])
    assert not any(crossings_reference(o, d, vv, bad)[k].any() for k in KEYS)
    # a face seen edge-on has no projected area
    assert not any(crossings_reference(np.float32([[-1, 0, 1]]), np.float32([[1, 0, 0]]), v, f[4:6])[k].any() for k in KEYS)
    for nothing in (np.zeros((0, 3), np.int32),):
        assert not any(crossings_reference(o, d, v, nothing)[k].any() for k in KEYS)
    assert crossings_reference(o[:0], d[:0], v, f)["front"].shape == (0,)
    with pytest.raises(ValueError):
        crossings_reference(o[:, :2], d, v, f)
    with pytest.raises(ValueError):
        crossings_reference(o, d[:3], v, f)
    with pytest.raises(ValueError, match="integers"):
        crossings_reference(o, d, v, np.float32([[0, 1, 2]]))


def test_the_cases_are_not_empty():
    for name in HOST_CASES:
        (o, d, v, f, t_min, t_max), got = case(name), reference(name)
        assert got["front"].shape == got["back"].shape == (len(o),), name
        if name in ("no_faces", "no_rays"):
            assert not got["front"].any() and not got["back"].any()
        elif len(o) >= 63 and len(f) >= 255:
            assert got["front"].any() and got["back"].any() and (got["front"] + got["back"] == 0).any(), name
    assert [len(case(n)[3]) for n in EDGES[:4]] == list(FACES) and [len(case(n)[0]) for n in EDGES[4:]] == [1, 63, 64]
    plain = reference("rooms:324x257")
    for cut in ("limits", "behind"):
        assert any((reference(cut)[k] != plain[k]).any() for k in KEYS), cut
    assert reference("behind")["front"].sum() != reference("limits")["front"].sum()
    bad = reference("bad_rays")
    assert not any(bad[k][[0, 2, 5, 7, 9, 14]].any() for k in KEYS)
    assert (plain["front"] + plain["back"]).max() >= 4          # the rooms: a ray leaves one and enters the next


# ---- the per-lane code on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/crossings_host.cpp, the per-lane functions of csrc/raycast.h as plain loops, built with the host compiler, its address and
    undefined-behaviour sanitizers and without FMA contraction: a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("crossings_host") / "crossings_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CSRC, "crossings_host.cpp"), "-o", out]
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
    assert len(raw) == 2 * 8 * R + 24
    results = [{"front": np.frombuffer(raw, "<i4", R, half * 8 * R), "back": np.frombuffer(raw, "<i4", R, half * 8 * R + 4 * R)} for half in range(2)]
    violations, evaluated, pairs = np.frombuffer(raw, "<i8", 3, 16 * R).tolist()
    return results[0], results[1], violations, evaluated, pairs


@pytest.mark.parametrize("name", HOST_CASES)
def test_the_lanes_on_the_host(host_program, tmp_path, name):
    """Every face and the kernel's culled sweep give the reference's counts, with the schedule forward and reversed; and every counted
    crossing lies in a tile that its ray reaches."""
    for reverse in (False, True):
        every, culled, violations, evaluated, pairs = run_on_the_host(host_program, tmp_path, name, reverse)
        hold(every, name, f"{name} reverse {reverse}, every face")
        hold(culled, name, f"{name} reverse {reverse}, culled")
        assert violations == 0, (name, reverse, violations)
        assert pairs == len(case(name)[0]) * -(-len(case(name)[3]) // TILE) and 0 <= evaluated <= pairs
    if name == "lattice:12:0":
        print(f"{name}: a wave of one lane evaluates {evaluated} of {pairs} (ray, tile) pairs")
        assert evaluated < pairs


# The schedule of the culled sweep, which no output shows: case -> the (wave, tile) pairs that the waves of WAVE consecutive rays
# evaluate, out of the waves times the tiles.  The host program with `wave` counted them; test_the_schedule_of_a_wave holds the
# program to them and tests/test_gpu_crossings.py the kernel.  The nodes are in row-major order, so a wave is five rows and a bit
# of one slice of the lattice; the surface's faces are in the order of their cells, so a tile is a slab of about one slice
SCHEDULE = {"lattice:12:0": (80, 405), "lattice:12:1": (86, 405), "lattice:12:2": (241, 405), "lattice:12:3": (89, 405), "lattice:12:4": (224, 405),
            "lattice:12:5": (209, 405), "lattice:12:6": (232, 405), "lattice:12:7": (116, 405), "rooms:324x257": (9, 10)}


def test_the_schedule_of_a_wave(host_program, tmp_path):
    assert sorted(SCHEDULE) == sorted(GPU_LATTICE + ["rooms:324x257"])
    for name, (count, pairs) in SCHEDULE.items():
        o, _, _, f = case(name)[:4]
        waves, tiles = -(-len(o) // WAVE), -(-len(f) // TILE)
        assert waves > 1 and tiles > 1 and pairs == waves * tiles and 0 < count <= pairs, name
        every, culled, violations, evaluated, of = run_on_the_host(host_program, tmp_path, name, False, wave=True)
        hold(every, name, f"{name} in waves, every face")
        hold(culled, name, f"{name} in waves, culled")
        print(f"{name}: waves of {WAVE} lanes evaluate {evaluated} of {of} (wave, tile) pairs")
        assert (violations, evaluated, of) == (0, count, pairs), name
    assert sum(c for c, _ in SCHEDULE.values()) < sum(p for _, p in SCHEDULE.values())          # something is culled


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch(tmp_path):
    kernels = _compile("crossings.hip", str(tmp_path / "crossings.s"))
    assert len(kernels) == 2, sorted(kernels)
    for name, k in kernels.items():          # one tile of corners, 256 faces x 3 x 16 bytes; 4 waves to a SIMD at up to 128 registers
        assert "cr_query_kernel" in name and k["scratch"] == 0 and k["lds"] == TILE * 3 * 16 == 12288 and k["vgpr"] <= 128, (name, k)


def test_build_flags_are_those_of_raycast():
    from test_kernel_resources import _build_py
    sources = _build_py().SOURCES
    assert sources["crossings.hip"] == sources["raycast.hip"] == ["-ffp-contract=off", "-fno-slp-vectorize"]


def test_header_exports_and_signatures():
    from npcd import hip
    from npcd.hip import crossings
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "npcd_hip.h")).read()
    L = hip.lib()
    name = "npcd_crossings_query"
    assert re.search(rf"\b{name}\(", header) and name in hip.SIGNATURES and hasattr(L, name)
    assert L.npcd_missing == () and L.npcd_abi_version() == 10
    assert len(hip.SIGNATURES[name][1]) == 15 and hip.SIGNATURES[name][1][8:11] == [ctypes.c_float, ctypes.c_float, ctypes.c_int]
    assert hip.count_crossings is crossings.count_crossings and hip.mesh_contains is crossings.mesh_contains
    # the host-side refusals, which look at no pointer's target and launch nothing: those of npcd_raycast_query
    V, F, R = 1000, 3000, 500
    one = ctypes.c_void_p(64)          # never followed: every call below is refused before a launch

    def refused(**changed):
        #    origins, directions, R, vertices, V, faces, F, ws, t_min, t_max, cull, front, back, evaluated, stream
        a = [one, one, R, one, V, one, F, one, 0.0, 1.0, 1, one, one, None, None]
        for i, value in changed.items():
            a[int(i[1:])] = value
        return L.npcd_crossings_query(*a)
    for missing in (0, 1, 7, 11, 12):
        assert refused(**{f"_{missing}": None}) == -1, missing
    for slot, bad in ((2, 0), (2, -1), (6, 0), (4, -1), (10, 2), (10, -1)):
        assert refused(**{f"_{slot}": bad}) == -1, (slot, bad)
    assert refused(_7=ctypes.c_void_p(72)) == -1          # the workspace: 16-byte aligned
    assert refused(_13=ctypes.c_void_p(68)) == -1         # the counter: 8-byte aligned
    assert refused(_0=ctypes.c_void_p(66)) == -1 and refused(_12=ctypes.c_void_p(66)) == -1
    for slot, bad in ((2, 2 ** 31), (4, 2 ** 31), (6, 2 ** 28)):
        assert refused(**{f"_{slot}": bad}) == -2, (slot, bad)
    assert refused(_2=2 ** 31, _0=None) == -2          # unsupported before a missing pointer


def test_wrapper_argument_errors():
    from npcd.hip.crossings import count_crossings, mesh_contains
    o, d, v, f = (torch.from_numpy(a) for a in case("rooms:255x65")[:4])
    with pytest.raises(RuntimeError, match="GPU"):
        count_crossings(o, d, v, f)                                                   # not on the GPU: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        count_crossings(o[:0], d[:0], v, f)
    with pytest.raises(RuntimeError, match="GPU"):
        mesh_contains(o, v, f)
    for bad in ((o.numpy(), d, v, f), (o, d.numpy(), v, f), (o, d, v.numpy(), f), (o, d, v, f.numpy()), (o[:, :2], d, v, f), (o, d[:, :2], v, f),
                (o, d, v.reshape(-1), f), (o, d, v, f[:, :2]), (o[None], d, v, f), (o, d[:5], v, f)):
        with pytest.raises(ValueError):
            count_crossings(*bad)
    with pytest.raises(ValueError, match=rf"{2 ** 28} faces"):
        count_crossings(o, d, v, torch.zeros(1, 3, dtype=torch.int32).expand(2 ** 28, 3))
    with pytest.raises(ValueError, match="rule"):
        mesh_contains(o, v, f, rule="odd")
    with pytest.raises(ValueError, match="direction"):
        mesh_contains(o, v, f, direction=(1.0, 0.0))
    with pytest.raises(ValueError, match="points"):
        mesh_contains(o[:, :2], v, f)


# ---- what users call, with stand-ins -------------------------------------------------------------------------------------------------------
def container(points, vertices, faces, direction=(1.0, 0.0, 0.0), rule="parity", boxes=None):
    """Stands in for npcd.hip.crossings.mesh_contains."""
    d = np.broadcast_to(np.float32(direction), tuple(points.shape))
    got = crossings_reference(points.numpy(), d, vertices.numpy(), faces.numpy())
    return torch.from_numpy((got["front"] + got["back"]) % 2 == 1)


def test_patch_order_is_a_permutation_of_neighbours():
    from npcd.eval.mesh import PATCH_ACROSS, PATCH_BLOCK, VOXEL_PATCH, patch_order
    assert VOXEL_PATCH in (PATCH_ACROSS, PATCH_BLOCK) and PATCH_ACROSS == (8, 8, 1) and PATCH_BLOCK == (4, 4, 4)
    for nodes, patch in (((8, 16, 4), PATCH_ACROSS), ((8, 8, 8), PATCH_BLOCK), ((5, 9, 3), PATCH_ACROSS), ((7, 6, 5), PATCH_BLOCK), ((1, 1, 1), PATCH_BLOCK)):
        order = patch_order(nodes, patch, "cpu")
        total = nodes[0] * nodes[1] * nodes[2]
        assert order.dtype == torch.int64 and sorted(order.tolist()) == list(range(total))
        if all(g % p == 0 for g, p in zip(nodes, patch)):          # whole patches: every 64 consecutive entries are one patch
            for first in range(0, total, 64):
                part = order[first:first + 64]
                z, y, x = part // (nodes[1] * nodes[2]), part // nodes[2] % nodes[1], part % nodes[2]
                assert (int(z.max() - z.min()) + 1, int(y.max() - y.min()) + 1, int(x.max() - x.min()) + 1) == tuple(patch)
    assert patch_order((2, 2, 2), (1, 1, 1), "cpu").tolist() == list(range(8))


def test_voxelize_mesh_with_stand_ins():
    """The lattice of the G = 9 volume through the host logic: node positions, the patches and the scatter back."""
    from npcd.eval.mesh import PATCH_ACROSS, PATCH_BLOCK, voxelize_mesh
    vol, v, f, _ = lattice(9, 0)
    mesh = (torch.from_numpy(v), torch.from_numpy(f))
    solid = torch.from_numpy(vol > LEVEL)
    for patch in (PATCH_ACROSS, PATCH_BLOCK):
        for direction in ((1.0, 0.0, 0.0), (1.0, 2.0, 3.0)):
            got = voxelize_mesh(mesh, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (9, 9, 9), direction=direction, patch=patch, container=container)
            assert got.dtype == torch.bool and got.shape == (9, 9, 9) and torch.equal(got, solid)
    # a lattice that is not the volume's own: half the spacing from another origin, and not a cube; origin and spacing as tensors
    part = voxelize_mesh({"vertices": mesh[0], "faces": mesh[1]}, torch.tensor([2.0, 1.0, 3.0]), torch.tensor([1.0, 2.0, 1.0]), (5, 4, 6), container=container)
    assert part.shape == (5, 4, 6) and torch.equal(part, solid[3:8, 1:9:2, 2:8])
    empty = voxelize_mesh((mesh[0], mesh[1][:0]), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 3, 3), container=container)
    assert not empty.any()
    with pytest.raises(ValueError, match="node"):
        voxelize_mesh(mesh, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (3, 0, 3), container=container)


def test_signed_distance_with_stand_ins():
    from npcd.eval.mesh import mesh_signed_distance, point_mesh_distance_reference
    v, f = cube()
    mesh = (torch.from_numpy(v), torch.from_numpy(f))

    def closest(points, vertices, faces):
        return {k: torch.from_numpy(a) for k, a in point_mesh_distance_reference(points.numpy(), vertices.numpy(), faces.numpy()).items()}
    p = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.25], [3.0, 1.0, 1.0], [3.0, 3.0, 1.0], [-1.0, -2.0, -2.0], [0.5, 1.5, 1.0]])
    got = mesh_signed_distance(p, mesh, closest=closest, container=container)
    assert got.dtype == torch.float32 and got.tolist() == [-1.0, -0.25, 1.0, float(np.sqrt(np.float32(2.0))), 3.0, -0.5]
    nothing = mesh_signed_distance(p, (mesh[0], mesh[1][:0]), closest=closest, container=container)
    assert torch.isposinf(nothing).all()


def test_volume_iou_with_stand_ins():
    from npcd.eval.mesh import mesh_volume_iou, voxelize_mesh
    voxelizer = functools.partial(voxelize_mesh, container=container)
    as_mesh = lambda vf: (torch.from_numpy(vf[0]), torch.from_numpy(vf[1]))
    big, small, far = as_mesh(cube((0, 0, 0), 4)), as_mesh(cube((1, 1, 1), 2)), as_mesh(cube((8, 0, 0), 4))
    # the lattice of 8^3 cells over the big cube's box [0, 4]^3: cells of 0.5, centres at 0.25, 0.75, ...; the small cube [1, 3]^3 holds 4^3
    same = mesh_volume_iou(big, big, resolution=8, voxelizer=voxelizer)
    assert same == {"iou": 1.0, "volume_a": 64.0, "volume_b": 64.0, "intersection": 64.0, "union": 64.0}
    nested = mesh_volume_iou(big, small, resolution=8, voxelizer=voxelizer)
    assert nested == {"iou": 64 / 512, "volume_a": 64.0, "volume_b": 8.0, "intersection": 8.0, "union": 64.0}
    apart = mesh_volume_iou(big, far, resolution=6, voxelizer=voxelizer)          # over [0, 12] x [0, 4]^2: cells of 2 x 2/3 x 2/3
    assert apart["iou"] == 0.0 and apart["intersection"] == 0.0 and apart["volume_a"] == pytest.approx(64.0, rel=1e-6) and apart["volume_b"] == pytest.approx(64.0, rel=1e-6)
    assert apart["union"] == pytest.approx(128.0, rel=1e-6)
    bound = mesh_volume_iou(small, big, resolution=10, bound=5.0, voxelizer=voxelizer)          # cells of 1 over [-5, 5]^3, centres at halves
    assert bound == {"iou": 8 / 64, "volume_a": 8.0, "volume_b": 64.0, "intersection": 8.0, "union": 64.0}
    none = (big[0], big[1][:0])
    assert mesh_volume_iou(none, none, resolution=4, voxelizer=voxelizer)["iou"] == 1.0          # two empty sets
    assert mesh_volume_iou(big, none, resolution=4, voxelizer=voxelizer)["iou"] == 0.0
    seen = []
    mesh_volume_iou(big, small, resolution=8, voxelizer=lambda m, o, s, n: seen.append((m, o, s, n)) or torch.zeros(n, dtype=torch.bool))
    assert [x[0] for x in seen] == [big, small] and all(x[3] == (8, 8, 8) and x[1].tolist() == [0.25] * 3 and x[2].tolist() == [0.5] * 3 for x in seen)
    for bad in (dict(resolution=0), dict(bound=0.0), dict(bound=-1.0)):
        with pytest.raises(ValueError):
            mesh_volume_iou(big, small, voxelizer=voxelizer, **bad)


def test_enclosure_with_stand_ins():
    from npcd.eval.mesh import mesh_enclosure, voxelize_mesh
    voxelizer = functools.partial(voxelize_mesh, container=container)
    vol, v, f, _ = lattice(9, 0)
    mesh = {"vertices": torch.from_numpy(v), "faces": torch.from_numpy(f)}
    solid = torch.from_numpy(vol > LEVEL)
    n = int(solid.sum())
    assert mesh_enclosure(mesh, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), solid, voxelizer=voxelizer) == {"agree": 1.0, "inside_nodes": n, "solid_nodes": n, "iou": 1.0}
    other = solid.clone()
    other[4, 4, 4] = ~other[4, 4, 4]
    other[0, 0, 0] = True
    got = mesh_enclosure(mesh, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), other, voxelizer=voxelizer)
    both, either = int((solid & other).sum()), int((solid | other).sum())
    assert got == {"agree": (729 - 2) / 729, "inside_nodes": n, "solid_nodes": int(other.sum()), "iou": both / either}
    nothing = mesh_enclosure((mesh["vertices"], mesh["faces"][:0]), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), torch.zeros(3, 3, 3, dtype=torch.bool), voxelizer=voxelizer)
    assert nothing == {"agree": 1.0, "inside_nodes": 0, "solid_nodes": 0, "iou": 1.0}


def test_extract_mesh_defaults_are_the_same_bytes(monkeypatch):
    """extract_mesh(enclosure=False) gives what it gave before the option existed; enclosure=True adds the report of mesh_enclosure
    for the final mesh, on the filtered density, and changes nothing else."""
    import npcd.hip.isosurface as iso_module
    from npcd.eval.mesh import extract_mesh, mesh_enclosure, voxelize_mesh
    from test_simplify_cpu import _Field
    field = _Field()

    def isosurface(volume, level, origin, spacing, normals=False, gradient_of=None):
        v, f = marching_tetrahedra_reference(volume[0].numpy(), level, origin.numpy(), spacing.numpy())
        n = vertex_normals_reference(volume[0].numpy(), level, spacing.numpy())
        return [(torch.from_numpy(v), torch.from_numpy(f)) + ((torch.from_numpy(n),) if normals else ())]
    monkeypatch.setattr(iso_module, "isosurface", isosurface)
    seen = []

    def encloser(mesh, origin, spacing, solid):
        seen.append((mesh, origin, spacing, solid))
        return mesh_enclosure(mesh, origin, spacing, solid, voxelizer=functools.partial(voxelize_mesh, container=container))
    coords, feats = torch.zeros(1, 4, 3), torch.zeros(1, 4, 8)
    common = dict(resolution=12, level=0.0)
    (plain,) = extract_mesh(field, coords, feats, **common)
    (same,) = extract_mesh(field, coords, feats, enclosure=False, **common)
    assert sorted(plain) == sorted(same) and "enclosure" not in plain
    assert all(plain[k].numpy().tobytes() == same[k].numpy().tobytes() for k in plain)
    (asked,) = extract_mesh(field, coords, feats, enclosure=True, encloser=encloser, **common)
    assert set(asked) == set(plain) | {"enclosure"}
    assert all(asked[k].numpy().tobytes() == plain[k].numpy().tobytes() for k in plain)
    solid = torch.from_numpy(field.vol > 0.0)
    assert len(seen) == 1 and torch.equal(seen[0][0]["vertices"], plain["vertices"]) and torch.equal(seen[0][3], solid)
    report = asked["enclosure"]
    print(report)
    assert sorted(report) == ["agree", "inside_nodes", "iou", "solid_nodes"] and report["solid_nodes"] == int(solid.sum())
    assert report["agree"] == 1.0 and report["iou"] == 1.0 and report["inside_nodes"] == report["solid_nodes"]          # no vertex of this sphere lies on a node
