"""What finishes a mesh, without a GPU: the CPU restatements in npcd.eval.mesh -- connected_components_reference
against scipy and hand cases, select_components, the filter's subsequence property on the isosurface, vertex_normals_reference
against geometry -- the PLY writer with normals, the kernels' resources from the compiler's own output, and the labelling phases of
csrc/components.h, the code the kernels run, built for the host (csrc/components_host.cpp) and held to the reference on the volumes
of the GPU test (tests/test_gpu_components.py, which imports them from here)."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from npcd.eval.mesh import (EDGE_TYPES, connected_components_reference, filter_components_reference, marching_tetrahedra_reference,
                            select_components, vertex_normals_reference, write_ply)
from test_isosurface_cpu import CENTRE, blobs_volume, lattice, read_ply, sphere_mesh, sphere_volume, two_spheres_volume
from test_kernel_resources import CSRC, _compile

BRICK = (16, 8, 8)          # (x, y, z), kCcBrick* of csrc/components.h; test_the_wrappers_know_the_constants holds it to the source
BX, BY, BZ = BRICK
# [Gz, Gy, Gx]: the smallest volume, non-cubic ones with every axis in turn the long one, one node more than a brick on each axis in
# turn, and two bricks and a node on every axis
SHAPES = [(2, 2, 2), (3, 2, 2), (2, 3, 5), (5, 6, 7), (9, 8, 33), (33, 9, 8), (17, 17, 17),
          (2, 2, BX + 1), (2, BY + 1, 2), (BZ + 1, 2, 2), (2 * BZ + 1, 2 * BY + 1, 2 * BX + 1)]
KINDS = ("noise_0.5", "noise_0.85", "noise_1.3", "two_spheres", "serpentine", "stairs_111", "stairs_110", "even_lattice", "nonfinite",
         "level_is_a_sample")
BIG = (101, 103, 102)


def component_volume(shape, kind, member):
    """-> (volume [Gz, Gy, Gx] float32, level): member `member` of a batch."""
    gz, gy, gx = shape
    n = gz * gy * gx
    rng = np.random.default_rng(1000 * member + sum(shape))
    z, y, x = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    if kind.startswith("noise_"):
        # 0.5: one component with nearly all inside nodes; 0.85: near the percolation threshold of this neighbourhood, large tortuous
        # components across many bricks; 1.3: many tiny ones
        return rng.standard_normal(shape).astype(np.float32), float(kind[6:])
    if kind == "two_spheres":
        p = lattice(shape)[0]
        a = 0.33 + 0.02 * member - np.linalg.norm(p - np.array([-0.5, -0.1, 0.05]), axis=-1)
        b = 0.3 - np.linalg.norm(p - np.array([0.45, 0.2, -0.1]), axis=-1)
        return np.maximum(a, b).astype(np.float32), 0.0
    if kind == "serpentine":
        # every second x-row of every second slab, rows joined at alternate ends, slabs joined at alternate sides: one component, one
        # node wide, whose label travels the whole volume
        inside = (z % 2 == 0) & (y % 2 == 0)
        inside |= (z % 2 == 0) & (y % 2 == 1) & (y + 1 < gy) & (x == np.where(y // 2 % 2 == 0, gx - 1, 0))
        last = (gy - 1) // 2 * 2
        inside |= (z % 2 == 1) & (z + 1 < gz) & (x == 0) & (y == np.where(z // 2 % 2 == 0, last, 0))
        vol = np.where(inside, 1.0, -1.0).astype(np.float32)
        return np.ascontiguousarray(vol[:, :, ::-1] if member == 1 else vol[:, ::-1] if member == 2 else vol), 0.0
    if kind == "stairs_111":          # staircases three apart, joined through (1, 1, 1) steps only
        return np.where(((x - z + member) % 3 == 0) & ((y - z) % 3 == 0), 1.0, -1.0).astype(np.float32), 0.0
    if kind == "stairs_110":          # through (1, 1, 0) steps only
        return np.where(((x - y + member) % 3 == 0) & (z % 2 == 0), 1.0, -1.0).astype(np.float32), 0.0
    if kind == "even_lattice":          # about n / 8 singletons: the most roots a volume can have
        return np.where((x % 2 == member % 2) & (y % 2 == 0) & (z % 2 == 0), 1.0, -1.0).astype(np.float32), 0.0
    vol = rng.standard_normal(shape).astype(np.float32)
    if kind == "nonfinite":
        flat = vol.reshape(-1)
        flat[(n // 3 + member) % n], flat[(2 * n // 3 + member) % n], flat[(n // 2 + member) % n] = np.nan, np.inf, -np.inf
        return vol, 0.5
    assert kind == "level_is_a_sample"
    return vol, float(vol.reshape(-1)[n // 2])


@functools.lru_cache(maxsize=None)
def component_case(shape, kind, member, level=None):
    """-> (volume, level, labels int64, sizes int64 [n]: nodes of the component at its root, 0 elsewhere), computed once.  `level`
    overrides the member's own: a batch is cut at one level."""
    vol, own = component_volume(shape, kind, member)
    level = own if level is None else level
    labels = connected_components_reference(vol, level)
    sizes = np.bincount(labels[labels >= 0], minlength=vol.size)
    for a in (vol, labels, sizes):
        a.setflags(write=False)
    return vol, level, labels, sizes


def batch(shape, kind, B):
    """B members cut at the first one's level."""
    level = component_case(shape, kind, 0)[1]
    return [component_case(shape, kind, m, level) for m in range(B)]


def scipy_labels(volume, level):
    ndimage = pytest.importorskip("scipy").ndimage
    structure = np.zeros((3, 3, 3), dtype=bool)
    structure[1, 1, 1] = True
    for dx, dy, dz in EDGE_TYPES:
        structure[1 + dz, 1 + dy, 1 + dx] = structure[1 - dz, 1 - dy, 1 - dx] = True
    assert structure.sum() == 15
    with np.errstate(invalid="ignore"):
        lab, count = ndimage.label(np.asarray(volume, dtype=np.float32) > np.float32(level), structure=structure)
    if count == 0:
        return np.full(lab.shape, -1, dtype=np.int64)
    index = np.arange(lab.size, dtype=np.int64).reshape(lab.shape)
    smallest = np.asarray(ndimage.minimum(index, lab, np.arange(1, count + 1))).astype(np.int64)
    return np.where(lab > 0, smallest[np.maximum(lab, 1) - 1], -1)


# ---- connected_components_reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 8, 33), (17, 17, 17), (17, 17, 33)])
def test_reference_against_scipy(shape):
    for kind in KINDS:
        vol, level, labels, _ = component_case(shape, kind, 0)
        np.testing.assert_array_equal(labels, scipy_labels(vol, level), err_msg=f"{shape} {kind}")


def test_reference_against_scipy_on_a_million_nodes():
    vol, level, labels, sizes = component_case(BIG, "noise_0.5", 0)
    np.testing.assert_array_equal(labels, scipy_labels(vol, level))
    print(f"{BIG}: {np.count_nonzero(sizes)} components, the largest {sizes.max() / (labels >= 0).sum():.3f} of the inside nodes")


def test_hand_cases():
    def label(vol, level=0.0):
        return connected_components_reference(np.asarray(vol, dtype=np.float32), level)
    out = np.full((2, 2, 2), -1.0)
    anti = out.copy()
    anti[0, 0, 1] = anti[0, 1, 0] = 1.0          # (x, y) = (1, 0) and (0, 1): the anti-diagonal of the Kuhn triangulation
    assert label(anti).reshape(-1).tolist() == [-1, 1, 2, -1, -1, -1, -1, -1]
    body = out.copy()
    body[0, 0, 0] = body[1, 1, 1] = 1.0
    assert label(body).reshape(-1).tolist() == [0, -1, -1, -1, -1, -1, -1, 0]
    assert (label(np.ones((3, 4, 5))) == 0).all()
    assert (label(-np.ones((3, 4, 5))) == -1).all()
    assert (label(np.full((3, 4, 5), 0.25), 0.25) == -1).all()          # a sample equal to the level is outside
    bar = np.full((2, 2, 5), -1.0)
    bar[0, 0, :] = 1.0
    assert label(bar)[0, 0].tolist() == [0, 0, 0, 0, 0]
    bar[0, 0, 2] = np.nan
    assert label(bar)[0, 0].tolist() == [0, 0, -1, 3, 3]
    assert connected_components_reference(bar, 0.0).dtype == np.int64
    with pytest.raises(ValueError):
        label(np.ones((3, 1, 3)))


def test_label_invariants():
    for kind in KINDS:
        vol, level, labels, sizes = component_case((17, 17, 33), kind, 0)
        flat = labels.reshape(-1)
        inside = np.nonzero(flat >= 0)[0]
        with np.errstate(invalid="ignore"):
            assert np.array_equal(flat >= 0, vol.reshape(-1) > np.float32(level))
        assert (flat[inside] <= inside).all() and np.array_equal(flat[flat[inside]], flat[inside])
        assert sizes.sum() == len(inside) and np.array_equal(np.nonzero(sizes)[0], np.unique(flat[inside]))
    # what the kinds promise
    for shape in SHAPES:
        vol, _, labels, sizes = component_case(shape, "serpentine", 0)
        assert np.count_nonzero(sizes) == 1 and sizes[0] == (vol > 0).sum(), shape
        _, _, labels, sizes = component_case(shape, "even_lattice", 0)
        assert set(sizes.tolist()) <= {0, 1} and sizes.sum() == -(-shape[0] // 2) * -(-shape[1] // 2) * -(-shape[2] // 2)
        gz, gy, gx = shape
        _, _, labels, sizes = component_case(shape, "stairs_111", 0)          # a staircase through (0, 0, 0): min(shape) steps
        assert sizes[0] == min(shape)
        _, _, labels, sizes = component_case(shape, "stairs_110", 0)
        assert sizes[0] == min(gy, gx)


def test_select_components():
    labels = np.array([0, 0, -1, 3, 3, 5, -1, 7, 7, 7, 10, -1]).reshape(1, 1, -1)          # sizes 2, 2, 1, 3, 1 at 0, 3, 5, 7, 10
    assert select_components(labels).tolist() == [0, 3, 5, 7, 10]
    assert select_components(labels, largest=1).tolist() == [7]
    assert select_components(labels, largest=2).tolist() == [0, 7]                  # the tie of 0 and 3 goes to the smaller root
    assert select_components(labels, largest=3).tolist() == [0, 3, 7]
    assert select_components(labels, largest=4).tolist() == [0, 3, 5, 7]            # and the tie of 5 and 10
    assert select_components(labels, largest=9).tolist() == [0, 3, 5, 7, 10]
    assert select_components(labels, min_nodes=2).tolist() == [0, 3, 7]
    assert select_components(labels, largest=2, min_nodes=3).tolist() == [7]
    assert select_components(labels, largest=1, min_nodes=4).tolist() == []
    assert select_components(np.full((2, 2, 2), -1)).tolist() == []
    assert select_components(labels).dtype == np.int64
    for bad in (dict(largest=0), dict(min_nodes=0), dict(largest=-1), dict(largest=1, min_nodes=0)):
        with pytest.raises(ValueError):
            select_components(labels, **bad)


# ---- the filter and the isosurface ---------------------------------------------------------------------------------------------------------
def filter_volumes():
    rng = np.random.default_rng(5)
    yield "two spheres", two_spheres_volume()[0], 0.0
    vol = blobs_volume((20, 21, 22))[0]
    yield "blobs", vol, float(np.median(vol))
    for shape in ((5, 6, 7), (17, 17, 17), (9, 8, 33)):
        yield f"noise {shape}", rng.standard_normal(shape).astype(np.float32), 0.85
        vol = blobs_volume(shape, seed=2)[0]
        yield f"blobs and noise {shape}", (vol + 0.3 * rng.standard_normal(shape)).astype(np.float32), float(np.median(vol))


def test_the_filtered_surface_is_a_part_of_the_surface():
    """The vertices of the filtered volume's isosurface are, bit for bit and in order, a subsequence of the volume's, and its faces,
    renumbered, a subset in order."""
    origin, spacing = (-1.0, 0.3, 0.7), (0.11, 0.07, 0.13)
    for name, vol, level in filter_volumes():
        v0, f0 = marching_tetrahedra_reference(vol, level, origin, spacing)
        labels = connected_components_reference(vol, level)
        for options in (dict(largest=1), dict(largest=2), dict(min_nodes=3), dict(largest=3, min_nodes=2)):
            kept = select_components(labels, **options)
            filtered = filter_components_reference(vol, level, **options)
            changed = filtered.view(np.int32) != vol.view(np.int32)
            assert np.array_equal(changed, (labels >= 0) & ~np.isin(labels, kept)), (name, options)
            assert (filtered[changed] == np.float32(level)).all()
            v1, f1 = marching_tetrahedra_reference(filtered, level, origin, spacing)
            assert len(v1) <= len(v0) and (len(kept) == 0) == (len(v1) == 0)
            # match greedily in order: every vertex of the part is the next equal vertex of the whole
            key0 = [r.tobytes() for r in v0.view(np.int32)]
            at, new_index = 0, np.empty(len(v1), dtype=np.int64)
            for i, r in enumerate(v1.view(np.int32)):
                r = r.tobytes()
                while at < len(key0) and key0[at] != r:
                    at += 1
                assert at < len(key0), (name, options, "a vertex that the unfiltered surface does not have, or out of order")
                new_index[i] = at
                at += 1
            whole = {tuple(row) for row in f0.tolist()}
            assert all(tuple(row) in whole for row in new_index[f1].tolist()), (name, options)
            print(f"{name} {options}: {len(kept)} of {len(np.unique(labels)) - 1} components, {len(v1)} of {len(v0)} vertices")
    # neither option keeps everything
    vol = blobs_volume((6, 7, 8))[0]
    assert np.array_equal(filter_components_reference(vol, 0.3).view(np.int32), vol.view(np.int32))


# ---- vertex_normals_reference against geometry ------------------------------------------------------------------------------------------
def face_normals(v, f):
    v = v.astype(np.float64)
    return np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])


def worst_face_agreement(v, f, n):
    """The smallest cosine between a face's normal and the mean of its three vertex normals."""
    fn = face_normals(v, f)
    mean = n.astype(np.float64)[f].sum(axis=1)
    return (np.sum(fn * mean, axis=1) / (np.linalg.norm(fn, axis=1) * np.linalg.norm(mean, axis=1))).min()


@pytest.mark.parametrize("G, angle, agreement", [(9, 3.96, 0.92), (17, 1.18, 0.98), (33, 0.30, 0.995)])
def test_normals_of_a_sphere(G, angle, agreement):
    """The bars: 1.5 x the worst angle to the radial direction that a scratch version of the specification measured (3.96, 1.18 and
    0.30 degrees); unit length to 1.5 x its 1.2e-7 (three roundings of 2^-24 each); every vertex normal on the outside of every face
    it belongs to."""
    vol, origin, spacing = sphere_volume((G, G, G))
    v, f = marching_tetrahedra_reference(vol, 0.0, origin, spacing)
    n = vertex_normals_reference(vol, 0.0, spacing)
    assert n.shape == v.shape and n.dtype == np.float32 and np.isfinite(n).all()
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    radial = v.astype(np.float64) - CENTRE
    radial /= np.linalg.norm(radial, axis=1)[:, None]
    worst = np.degrees(np.arccos(np.clip(np.sum(n * radial, axis=1) / length, -1, 1))).max()
    each = np.sum(face_normals(v, f)[:, None, :] * n.astype(np.float64)[f], axis=2)          # [F, 3]: a face against its three corners
    print(f"G {G}: worst angle {worst:.3f} deg, |n| - 1 within {np.abs(length - 1).max():.2e}, face agreement {worst_face_agreement(v, f, n):.4f}"
          f" (measured before: {agreement})")
    assert worst <= 1.5 * angle
    assert np.abs(length - 1).max() <= 1.5 * 1.2e-7
    assert worst_face_agreement(v, f, n) > 0 and (each > 0).all()


def test_normals_of_blobs():
    vol, origin, spacing = blobs_volume((20, 21, 22))
    level = float(np.median(vol))
    v, f = marching_tetrahedra_reference(vol, level, origin, spacing)
    n = vertex_normals_reference(vol, level, spacing)
    each = np.sum(face_normals(v, f)[:, None, :] * n.astype(np.float64)[f], axis=2)
    print(f"blobs: face agreement {worst_face_agreement(v, f, n):.4f} (measured before: 0.64)")
    assert worst_face_agreement(v, f, n) > 0 and (each > 0).all()


def test_normals_degenerate_and_gradient_of():
    # a constant gradient: the normal is exact up to rounding, whatever t
    gz, gy, gx = 4, 5, 6
    z, y, x = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    spacing = (0.5, 0.25, 2.0)
    vol = (3.0 - 1.0 * x * spacing[0] - 2.0 * y * spacing[1] - 2.0 * z * spacing[2]).astype(np.float32)
    n = vertex_normals_reference(vol, 0.1, spacing)
    assert len(n) and np.abs(n - np.array([1.0, 2.0, 2.0]) / 3.0).max() < 1e-6
    # no gradient: 0 / 0 -> (+0, +0, +0), by the bits
    flat = np.full((3, 3, 3), 1.0, dtype=np.float32)
    flat[1, 1, 1] = 0.0
    other = np.zeros((3, 3, 3), dtype=np.float32)
    n = vertex_normals_reference(flat, 0.5, (1.0, 1.0, 1.0), gradient_of=other)
    assert n.shape == (14, 3) and (n.view(np.int32) == 0).all()
    # a NaN sample: zero rows exactly where a gradient or t touches it, unit rows elsewhere
    vol = blobs_volume((6, 7, 8), seed=3)[0]
    level = float(np.median(vol))
    bad = vol.copy()
    bad[2, 3, 4] = np.nan
    n = vertex_normals_reference(bad, level, (1.0, 1.0, 1.0))
    zero = (n.view(np.int32) == 0).all(axis=1)
    assert zero.any() and not zero.all() and np.abs(np.linalg.norm(n[~zero].astype(np.float64), axis=1) - 1).max() < 2e-7
    # gradient_of: the crossings and t of the volume, the gradients of the other field
    n = vertex_normals_reference(vol, level, (1.0, 1.0, 1.0), gradient_of=-vol)
    assert np.array_equal(n, -vertex_normals_reference(vol, level, (1.0, 1.0, 1.0)))
    with pytest.raises(ValueError):
        vertex_normals_reference(vol, level, (1.0, 1.0, 1.0), gradient_of=vol[1:])
    assert vertex_normals_reference(np.ones((2, 2, 2)), 0.0).shape == (0, 3)


# ---- PLY ------------------------------------------------------------------------------------------------------------------------------------
def test_write_ply_with_normals(tmp_path):
    v, f, _ = sphere_mesh(17)
    vol, _, spacing = sphere_volume((17, 17, 17))
    n = vertex_normals_reference(vol, 0.0, spacing)
    colors = np.random.default_rng(0).integers(0, 256, (len(v), 3)).astype(np.uint8)
    write_ply(tmp_path / "normals.ply", v, f, normals=n)
    raw = open(tmp_path / "normals.ply", "rb").read()
    header = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
    at = header.index("property float z")
    assert header[at + 1:at + 4] == ["property float nx", "property float ny", "property float nz"]
    body = np.frombuffer(raw, dtype="<f4", count=6 * len(v), offset=raw.index(b"end_header\n") + 11).reshape(-1, 6)
    assert np.array_equal(body[:, :3], v) and np.array_equal(body[:, 3:], n)
    xyz, faces, rgb = read_ply(tmp_path / "normals.ply")
    assert rgb is None and np.array_equal(xyz, v) and np.array_equal(faces, f)
    write_ply(tmp_path / "both.ply", v, f, colors, n)
    raw = open(tmp_path / "both.ply", "rb").read()
    header = raw[:raw.index(b"end_header\n")].decode("ascii").split("\n")
    assert header[header.index("property float nz") + 1] == "property uchar red"
    xyz, faces, rgb = read_ply(tmp_path / "both.ply")
    assert np.array_equal(xyz, v) and np.array_equal(faces, f) and np.array_equal(rgb, colors)
    with pytest.raises(ValueError):
        write_ply(tmp_path / "bad.ply", v, f, normals=n[:-1])
    # without normals: the bytes of the writer before it knew of them
    for name, c in (("plain", None), ("coloured", colors)):
        write_ply(tmp_path / f"{name}.ply", v, f, c)
        head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z"]
        head += ["property uchar red", "property uchar green", "property uchar blue"] if c is not None else []
        head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
        vert = np.empty(len(v), dtype=[("p", "<f4", (3,))] + ([("c", "u1", (3,))] if c is not None else []))
        vert["p"] = v
        if c is not None:
            vert["c"] = c
        face = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        face["n"], face["v"] = 3, f
        assert open(tmp_path / f"{name}.ply", "rb").read() == ("\n".join(head) + "\n").encode("ascii") + vert.tobytes() + face.tobytes()


# ---- the kernels' resources, from the compiler's own output ----------------------------------------------------------------------------
def test_the_wrappers_know_the_constants():
    from npcd.hip import components, isosurface
    source = open(f"{CSRC}/components.h").read()
    got = re.search(r"constexpr int kCcBrickX = (\d+), kCcBrickY = (\d+), kCcBrickZ = (\d+);", source)
    assert tuple(int(g) for g in got.groups()) == components.BRICK == BRICK
    # the normals kernel walks the strips of the isosurface's workspace
    strip = int(re.search(r"constexpr int kIsoStrip = (\d+);", open(f"{CSRC}/isosurface_normals.hip").read()).group(1))
    assert strip == int(re.search(r"constexpr int kIsoThreads = (\d+);", open(f"{CSRC}/isosurface.hip").read()).group(1)) == isosurface.STRIP_NODES


def test_kernels_use_no_scratch(tmp_path):
    kernels = _compile("components.hip", str(tmp_path / "components.s"))
    assert len(kernels) == 3, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128, (name, k)
        assert k["lds"] == (8 * BX * BY * BZ if "cc_tile_kernel" in name else 0), (name, k)          # the brick's labels and counts
    kernels = _compile("isosurface_normals.hip", str(tmp_path / "isosurface_normals.s"))
    assert len(kernels) == 1, sorted(kernels)
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["vgpr"] <= 128 and k["lds"] == 0, (name, k)          # 1,024 lanes a workgroup


def test_header_exports_and_signatures():
    import ctypes

    from npcd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "npcd_hip.h")).read()
    L = hip.lib()
    for name in ("npcd_components_ws_bytes", "npcd_components_label", "npcd_isosurface_normals"):
        assert re.search(rf"\b{name}\(", header) and name in hip.SIGNATURES and hasattr(L, name), name
    assert hip.SIGNATURES["npcd_components_ws_bytes"][0] is ctypes.c_int64
    assert len(hip.SIGNATURES["npcd_components_label"][1]) == 10 and len(hip.SIGNATURES["npcd_isosurface_normals"][1]) == 12
    assert L.npcd_abi_version() == 10
    # the host-side refusals, which look at no pointer's target and launch nothing
    assert L.npcd_components_ws_bytes(2, 5, 6, 7) == 2 * 4 * 210
    assert L.npcd_components_ws_bytes(1, 1024, 1024, 2047) == 4 * 1024 * 1024 * 2047
    assert L.npcd_components_ws_bytes(1, 1024, 1024, 2048) == -2          # 2^31 nodes
    for bad in ((1, 1, 4, 4), (1, 4, 1, 4), (1, 4, 4, 1), (0, 4, 4, 4), (1, 4, 4, -3)):
        assert L.npcd_components_ws_bytes(*bad) == -1
    assert L.npcd_components_label(None, 1, 4, 4, 4, 0.0, None, None, None, None) == -1
    assert L.npcd_components_label(None, 1, 1024, 1024, 2048, 0.0, None, None, None, None) == -2
    assert L.npcd_isosurface_normals(None, None, 1, 4, 4, 4, 0.0, None, None, None, None, None) == -1
    assert L.npcd_isosurface_normals(None, None, 1, 1024, 1024, 293, 0.0, None, None, None, None, None) == -2


# ---- the labelling phases on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """csrc/components_host.cpp, the phases of csrc/components.h as plain loops, built with the host compiler and its address and
    undefined-behaviour sanitizers: a stand-alone program."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    out = str(tmp_path_factory.mktemp("components_host") / "components_host")
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(CSRC, "components_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_on_the_host(program, tmp_path, members, level, reverse):
    vols = np.stack([m[0] for m in members])
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.array(vols.shape, dtype="<i4").tobytes() + np.float32(level).tobytes() + vols.astype("<f4").tobytes())
    r = subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")] + (["reverse"] if reverse else []),
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = np.fromfile(tmp_path / "out.bin", dtype="<i4").reshape(2, len(members), -1)
    return got[0], got[1]


@pytest.mark.parametrize("shape", SHAPES)
def test_the_phases_on_the_host(host_program, tmp_path, shape):
    for kind in KINDS:
        members = batch(shape, kind, 3)
        for reverse in (False, True):
            labels, sizes = run_on_the_host(host_program, tmp_path, members, members[0][1], reverse)
            for b, (_, _, want_labels, want_sizes) in enumerate(members):
                np.testing.assert_array_equal(labels[b], want_labels.reshape(-1), err_msg=f"{shape} {kind} member {b} reverse {reverse}")
                np.testing.assert_array_equal(sizes[b], want_sizes, err_msg=f"{shape} {kind} member {b} reverse {reverse}")


def test_the_phases_on_the_host_on_a_million_nodes(host_program, tmp_path):
    member = component_case(BIG, "noise_0.5", 0)
    labels, sizes = run_on_the_host(host_program, tmp_path, [member], member[1], False)
    np.testing.assert_array_equal(labels[0], member[2].reshape(-1))
    np.testing.assert_array_equal(sizes[0], member[3])
