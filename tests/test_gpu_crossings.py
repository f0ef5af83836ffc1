"""Inside tests for meshes on the GPU: count_crossings against crossings_reference, count for count, on the cases of
tests/test_crossings_cpu.py -- the nodes of the 12^3 lattice volume along eight directions, whose rays run through vertices and edges
of the surface, tile and wave edges on the cube soup, rays that are not usable, limits on t, invalid indices -- culled and not; the
schedule of the sweep held to the host's count; no host read; and what rests on it end to end: mesh_contains and voxelize_mesh on the
GPU's own isosurface against the volume, mesh_volume_iou, mesh_signed_distance and extract_mesh(enclosure=True) on the kernels."""
import math

import numpy as np
import pytest
import torch

from test_crossings_cpu import DIRECTIONS, GPU_CASES, KEYS, LEVEL, SCHEDULE, TILE, WAVE, case, cube, hold, lattice, reference

pytestmark = pytest.mark.gpu


def on_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(name, **options):
    from npcd.hip.crossings import count_crossings
    o, d, v, f, t_min, t_max = case(name)
    got = count_crossings(on_gpu(o), on_gpu(d), on_gpu(v), on_gpu(f), t_min=t_min, t_max=t_max, **options)
    assert all(t.is_cuda for t in got.values())
    return got


def as_mesh(vf):
    return on_gpu(vf[0]), on_gpu(vf[1])


@pytest.mark.parametrize("name", GPU_CASES)
def test_against_the_reference(name):
    reference(name)
    for cull in (True, False):
        got = run(name, cull=cull)
        assert set(got) == set(KEYS) and all(got[k].dtype == torch.int32 and got[k].shape == (len(case(name)[0]),) for k in KEYS)
        hold({k: t.cpu().numpy() for k, t in got.items()}, name, f"{name} cull {cull}")


@pytest.mark.parametrize("name", sorted(SCHEDULE))
def test_the_schedule_of_the_sweep(name):
    """The kernel's waves evaluate exactly the (wave, tile) pairs that the host's sweep over the same policy evaluates (SCHEDULE of
    tests/test_crossings_cpu.py), and every pair without culling."""
    count, pairs = SCHEDULE[name]
    culled, every = run(name, cull=True, stats=True), run(name, cull=False, stats=True)
    assert culled["evaluated"].dtype == torch.int64 and culled["evaluated"].shape == (1,)
    print(f"{name}: evaluated {int(culled['evaluated'])} of {int(every['evaluated'])} (wave, tile) pairs; the host's sweep {count} of {pairs}")
    assert int(culled["evaluated"]) == count
    assert int(every["evaluated"]) == pairs == -(-len(case(name)[0]) // WAVE) * -(-len(case(name)[3]) // TILE)
    hold({k: culled[k].cpu().numpy() for k in KEYS}, name, f"{name} with stats")


def test_no_host_read():
    from npcd.eval.mesh import voxelize_mesh
    from npcd.hip.crossings import count_crossings, mesh_contains
    from npcd.hip.mesh_distance import mesh_boxes
    for name in ("rooms:324x257", "bad_indices", "no_faces"):
        o, d, v, f = (on_gpu(a) for a in case(name)[:4])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")          # a host read would raise
        try:
            got = count_crossings(o, d, v, f, stats=True)
            inside = mesh_contains(o, v, f, direction=(1.0, 2.0, 3.0))
            voxels = voxelize_mesh((v, f), (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5), (5, 6, 7))
            if f.shape[0]:
                again = count_crossings(o, d, v, f, boxes=mesh_boxes(v, f))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        hold({k: got[k].cpu().numpy() for k in KEYS}, name, f"{name} without a host read")
        assert inside.dtype == torch.bool and inside.shape == (len(o),) and voxels.shape == (5, 6, 7)
        if f.shape[0]:
            hold({k: again[k].cpu().numpy() for k in KEYS}, name, f"{name} without a host read, boxes given")


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.crossings import count_crossings
    o, d, v, f = (on_gpu(a) for a in case("rooms:255x65")[:4])
    for bad in ((o.double(), d, v, f), (o, d.half(), v, f), (o, d, v.half(), f), (o, d, v, f.long()), (o.cpu(), d, v, f), (o, d, v, f.cpu()),
                (o, d.cpu(), v, f)):
        with pytest.raises(RuntimeError):
            count_crossings(*bad)
    for bad in ((o[:, :2], d, v, f), (o, d, v[None], f), (o, d, v, f.reshape(-1)), (o, d[:9], v, f)):
        with pytest.raises(ValueError):
            count_crossings(*bad)
    with pytest.raises(ValueError, match="boxes"):
        count_crossings(o, d, v, f, boxes=torch.zeros(8, dtype=torch.int64, device="cuda"))
    wide = torch.zeros(len(o), 5, device="cuda")          # strided inputs are what their contiguous copies are
    wide[:, 1:4] = d
    hold({k: t.cpu().numpy() for k, t in count_crossings(o, wide[:, 1:4], v, f).items()}, "rooms:255x65", "strided directions")


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_the_isosurface_encloses_its_volume():
    """The GPU's own isosurface of the 12^3 volume: mesh_contains at the nodes says `volume > level` at every node, by parity and by
    winding, along every direction; voxelize_mesh says the same in either patch order."""
    from npcd.eval.mesh import PATCH_ACROSS, PATCH_BLOCK, voxelize_mesh
    from npcd.hip.crossings import mesh_contains
    from npcd.hip.isosurface import isosurface
    from npcd.hip.mesh_distance import mesh_boxes
    vol, v_host, f_host, nodes = lattice(12, 1)
    (v, f), = isosurface(on_gpu(vol), LEVEL)
    assert np.array_equal(v.cpu().numpy(), v_host) and np.array_equal(f.cpu().numpy(), f_host)
    solid = on_gpu(vol > LEVEL)
    boxes = mesh_boxes(v, f)
    for direction in DIRECTIONS:
        for rule in ("parity", "winding"):
            got = mesh_contains(on_gpu(nodes), v, f, direction=direction, rule=rule, boxes=boxes)
            assert got.dtype == torch.bool and torch.equal(got, solid.reshape(-1)), (direction, rule)
    assert torch.equal(mesh_contains(on_gpu(nodes), v, f), solid.reshape(-1))
    for patch in (PATCH_ACROSS, PATCH_BLOCK):
        for direction in ((1.0, 0.0, 0.0), (1.0, 2.0, 3.0)):
            got = voxelize_mesh((v, f), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (12, 12, 12), direction=direction, patch=patch)
            assert got.dtype == torch.bool and got.shape == (12, 12, 12) and torch.equal(got, solid), (patch, direction)
    assert torch.equal(voxelize_mesh({"vertices": v, "faces": f}, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (12, 12, 12)), solid)


def test_volume_iou():
    from npcd.eval.mesh import mesh_volume_iou
    from npcd.hip.isosurface import isosurface
    vol = lattice(12, 1)[0]
    (v, f), = isosurface(on_gpu(vol), LEVEL)
    same = mesh_volume_iou((v, f), (v, f))
    assert same["iou"] == 1.0 and same["volume_a"] == same["volume_b"] == same["intersection"] == same["union"] > 0
    apart = mesh_volume_iou((v, f), (v + torch.tensor([20.0, 0.0, 0.0], device="cuda"), f), resolution=32)          # a translated, disjoint copy
    assert apart["iou"] == 0.0 and apart["intersection"] == 0.0 and apart["volume_a"] > 0 and apart["volume_b"] > 0
    assert apart["union"] == pytest.approx(apart["volume_a"] + apart["volume_b"], rel=1e-12)
    # nested cubes: 8^3 cells of 0.5 over [0, 4]^3, centres at 0.25, 0.75, ...: all 512 lie in the big cube, 4^3 in [1, 3]^3
    big, small = as_mesh(cube((0, 0, 0), 4)), as_mesh(cube((1, 1, 1), 2))
    assert mesh_volume_iou(big, small, resolution=8) == {"iou": 64 / 512, "volume_a": 64.0, "volume_b": 8.0, "intersection": 8.0, "union": 64.0}
    assert mesh_volume_iou(small, big, resolution=10, bound=5.0) == {"iou": 8 / 64, "volume_a": 8.0, "volume_b": 64.0, "intersection": 8.0, "union": 64.0}
    assert mesh_volume_iou(big, small, resolution=7)["iou"] == 27 / 343          # cells of 4 / 7: the centres 3, 4 and 5 of 0..6 lie in [1, 3]


def test_signed_distance_of_a_cube():
    from npcd.eval.mesh import mesh_signed_distance
    mesh = as_mesh(cube())          # [0, 2]^3
    p = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, 0.25], [3.0, 1.0, 1.0], [3.0, 3.0, 1.0], [-1.0, -2.0, -2.0], [0.5, 1.5, 1.0], [1.75, 0.5, 0.5]], device="cuda")
    got = mesh_signed_distance(p, mesh)
    assert got.dtype == torch.float32 and got.shape == (7,)
    assert got.tolist() == [-1.0, -0.25, 1.0, float(np.sqrt(np.float32(2.0))), 3.0, -0.5, -0.25]
    assert torch.isposinf(mesh_signed_distance(p, (mesh[0], mesh[1][:0]))).all()


def test_enclosure_on_the_kernels():
    """With untrained weights an interpolated vertex can round onto a node, so `agree` is not held to 1: the keys, the ranges, the
    counts against the volume and the repeatability are what is held, and that asking for the report changes nothing else."""
    from npcd.eval.mesh import extract_mesh, mesh_enclosure
    from test_gpu_field_query import _model, _on_gpu
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma, origin, spacing = m.density_grid(coords, feats, resolution=24)
    level = float(sigma[sigma > 0].median())          # a surface exists with untrained weights
    plain = extract_mesh(m, coords, feats, resolution=24, level=level)
    off = extract_mesh(m, coords, feats, resolution=24, level=level, enclosure=False)
    asked = extract_mesh(m, coords, feats, resolution=24, level=level, enclosure=True)
    again = extract_mesh(m, coords, feats, resolution=24, level=level, enclosure=True)
    same = lambda a, b: torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    for b in range(len(plain)):
        assert set(asked[b]) == set(plain[b]) | {"enclosure"} and set(off[b]) == set(plain[b]) and "enclosure" not in plain[b]
        assert all(same(t, asked[b][key]) and same(t, off[b][key]) for key, t in plain[b].items())
        report = asked[b]["enclosure"]
        print(f"cloud {b}: {report}")
        assert set(report) == {"agree", "inside_nodes", "solid_nodes", "iou"}
        assert 0.0 <= report["agree"] <= 1.0 and 0.0 <= report["iou"] <= 1.0 and math.isfinite(report["agree"])
        assert report["solid_nodes"] == int((sigma[b] > level).sum()) > 0 and 0 <= report["inside_nodes"] <= 24 ** 3
        assert report == again[b]["enclosure"]
        assert mesh_enclosure(plain[b], origin, spacing, sigma[b] > level) == report
