"""Point-to-mesh distance on the GPU: closest_on_mesh against point_mesh_distance_reference bit for bit on the cases
of tests/test_mesh_distance_cpu.py -- tile and wave edges, the sphere plain, simplified, shifted and scaled, planted duplicates,
invalid indices, NaN vertices and points -- for every combination of cull and sort_points, twice; culling that really culls, and
the schedule of the walk held to the host's count; no host read; and mesh_deviation, cloud_mesh_distance and
extract_mesh(deviation=) on the kernels."""
import math

import numpy as np
import pytest
import torch

from test_mesh_distance_cpu import CASES, K_ULP, KEYS, SAMPLE_ULP, SCHEDULE, TILE, WAVE, ball, case, hold, reference

pytestmark = pytest.mark.gpu


def on_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(name, **options):
    from npcd.hip.mesh_distance import closest_on_mesh
    got = closest_on_mesh(*(on_gpu(a) for a in case(name)), **options)
    assert all(t.is_cuda for t in got.values())
    return got


def sphere():
    v, f, _ = ball()
    return on_gpu(v), on_gpu(f.astype(np.int32))


@pytest.mark.parametrize("name", CASES)
def test_against_the_reference(name):
    reference(name)
    for cull in (True, False):
        for sort_points in (True, False):
            for attempt in range(2):
                got = run(name, cull=cull, sort_points=sort_points)
                assert set(got) == set(KEYS)
                hold({k: t.cpu().numpy() for k, t in got.items()}, name, f"{name} cull {cull} sort {sort_points} run {attempt}")


def test_culling_really_culls():
    from npcd.hip.mesh_distance import closest_on_mesh
    from npcd.hip.surface import sample_surface
    v, f = sphere()
    points = sample_surface((v, f), 4096, generator=torch.Generator(device="cuda").manual_seed(5))[0]
    waves, tiles = -(-4096 // WAVE), -(-f.shape[0] // TILE)
    counts = {}
    for cull in (True, False):
        for sort_points in (True, False):
            got = closest_on_mesh(points, v, f, cull=cull, sort_points=sort_points, stats=True)
            assert set(got) == set(KEYS) | {"evaluated"} and got["evaluated"].dtype == torch.int64 and got["evaluated"].shape == (1,)
            counts[cull, sort_points] = int(got["evaluated"])
            if (cull, sort_points) != (True, True):
                assert all(torch.equal(got[k].view(torch.int32), first[k].view(torch.int32)) for k in KEYS)
            first = got
    print(f"evaluated (wave, tile) pairs of {waves * tiles}: sorted and culled {counts[True, True]} ({counts[True, True] / (waves * tiles):.3f}), "
          f"culled only {counts[True, False]} ({counts[True, False] / (waves * tiles):.3f})")
    assert counts[False, True] == counts[False, False] == waves * tiles
    assert 0 < counts[True, True] < waves * tiles and counts[True, True] <= counts[True, False] <= waves * tiles
    # surface samples lie within a few ulp of the surface (SAMPLE_ULP of tests/test_mesh_distance_cpu.py)
    ulp = float(np.spacing(np.float32(v.abs().max().item())))
    print(f"the farthest sample lies {math.sqrt(float(first['sqdist'].max())) / ulp:.2f} ulp off its mesh")
    assert math.sqrt(float(first["sqdist"].max())) <= (SAMPLE_ULP + K_ULP) * ulp


@pytest.mark.parametrize("name", sorted(SCHEDULE))
def test_the_schedule_of_the_walk(name):
    """The kernel's waves evaluate exactly the (wave, tile) pairs that the host's walk over the same policy evaluates (SCHEDULE of
    tests/test_mesh_distance_cpu.py): points as given, so that a wave holds the host's 64 consecutive points; and every pair without
    culling."""
    count, pairs = SCHEDULE[name]
    culled = run(name, cull=True, sort_points=False, stats=True)
    every = run(name, cull=False, sort_points=False, stats=True)
    print(f"{name}: evaluated {int(culled['evaluated'])} of {int(every['evaluated'])} (wave, tile) pairs; the host's walk {count} of {pairs}")
    assert int(culled["evaluated"]) == count
    assert int(every["evaluated"]) == pairs == -(-len(case(name)[0]) // WAVE) * -(-len(case(name)[2]) // TILE)


def test_no_host_read():
    from npcd.hip.mesh_distance import closest_on_mesh
    for name in ("soup:513x257", "lost", "no_faces"):
        p, v, f = (on_gpu(a) for a in case(name))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")          # a host read would raise
        try:
            got = closest_on_mesh(p, v, f, sort_points=False, stats=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        hold({k: got[k].cpu().numpy() for k in KEYS}, name, f"{name} without a host read")


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.mesh_distance import closest_on_mesh
    p, v, f = (on_gpu(a) for a in case("soup:255x257"))
    for bad in ((p.double(), v, f), (p, v.half(), f), (p, v, f.long()), (p.cpu(), v, f), (p, v, f.cpu())):
        with pytest.raises(RuntimeError):
            closest_on_mesh(*bad)
    for bad in ((p[:, :2], v, f), (p, v[None], f), (p, v, f.reshape(-1))):
        with pytest.raises(ValueError):
            closest_on_mesh(*bad)
    # strided inputs are what their contiguous copies are
    wide = torch.zeros(len(p), 5, device="cuda")
    wide[:, 1:4] = p
    got = closest_on_mesh(wide[:, 1:4], v, f)
    hold({k: t.cpu().numpy() for k, t in got.items()}, "soup:255x257", "strided points")


def test_mesh_deviation_on_the_gpu():
    from npcd.eval.mesh import cloud_mesh_distance, mesh_deviation
    from npcd.hip.simplify import simplify_mesh
    from npcd.hip.smooth import smooth_mesh
    v, f = sphere()
    seeded = lambda: torch.Generator(device="cuda").manual_seed(11)
    ulp = float(np.spacing(np.float32(v.abs().max().item())))
    # against itself: "0" of a sampled surface is at most (SAMPLE_ULP + K_ULP) ulp(A), derived beside SAMPLE_ULP in
    # tests/test_mesh_distance_cpu.py
    same = mesh_deviation((v, f), {"vertices": v, "faces": f}, 4000, generator=seeded())
    print(f"the sphere against itself: {same}")
    assert 0 <= same["mean"] <= same["hausdorff"] <= (SAMPLE_ULP + K_ULP) * ulp and same["samples"] == 4000
    assert same["diagonal"] == pytest.approx(math.sqrt(3) * 2 * 9.3, rel=0.02)
    # against its simplification at 2 spacings: a vertex moves at most a cell's diagonal, so every point of either surface lies
    # within that of the other
    coarse = simplify_mesh(v, f, 2.0, origin=[0.0, 0.0, 0.0], dims=[12, 12, 12])
    dev = mesh_deviation((v, f), coarse, 4000, generator=seeded())
    print(f"the sphere against its simplification at 2 spacings: {dev}")
    assert 0 < dev["a_to_b"]["mean"] <= dev["a_to_b"]["rms"] <= dev["a_to_b"]["max"] <= dev["hausdorff"] <= math.sqrt(3) * 2
    assert dev["hausdorff"] == max(dev["a_to_b"]["max"], dev["b_to_a"]["max"]) and dev["mean"] == 0.5 * (dev["a_to_b"]["mean"] + dev["b_to_a"]["mean"])
    assert dev == mesh_deviation((v, f), coarse, 4000, generator=seeded())          # two calls give equal dicts
    # against itself smoothed 10 iterations
    smooth = smooth_mesh(v, f, iterations=10)
    moved = mesh_deviation((v, f), (smooth, f), 4000, generator=seeded())
    print(f"the sphere against itself after 10 iterations of smoothing: {moved}")
    assert all(math.isfinite(x) and x > 0 for x in (*moved["a_to_b"].values(), *moved["b_to_a"].values(), moved["hausdorff"], moved["mean"]))
    assert moved["b_to_a"]["mean"] < 1.0          # below the spacing
    # a cloud against the surface: points at radius 9.3 + 1 lie about 1 off the faceted sphere
    centre = torch.tensor([11.4, 11.7, 11.2], device="cuda")
    direction = torch.nn.functional.normalize(torch.randn(1000, 3, generator=seeded(), device="cuda"), dim=1)
    got = cloud_mesh_distance(centre + 10.3 * direction, (v, f))
    print(f"a cloud one spacing outside the sphere: {got}")
    assert 0.9 < got["mean"] <= got["rms"] <= got["max"] < 1.2


def test_extract_mesh_deviation():
    from npcd.eval.mesh import extract_mesh
    from test_gpu_field_query import _model, _on_gpu
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma, _, spacing = m.density_grid(coords, feats, resolution=24)
    level = float(sigma[sigma > 0].median())          # a surface exists with untrained weights
    plain = extract_mesh(m, coords, feats, resolution=24, level=level, simplify=2)
    asked = extract_mesh(m, coords, feats, resolution=24, level=level, simplify=2, deviation=2000)
    again = extract_mesh(m, coords, feats, resolution=24, level=level, simplify=2, deviation=2000)
    cell_diagonal = 2.0 * float(torch.sqrt((spacing.double() ** 2).sum()))
    for b in range(len(plain)):
        assert set(asked[b]) == set(plain[b]) | {"deviation"} and "deviation" not in plain[b]
        for key, t in plain[b].items():
            assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, asked[b][key].view(torch.int32) if t.dtype == torch.float32 else asked[b][key]), key
        d = asked[b]["deviation"]
        print(f"cloud {b}: {d}")
        assert d == again[b]["deviation"] and d["samples"] == 2000
        assert 0 < d["mean"] <= d["hausdorff"] < math.inf and d["diagonal"] > cell_diagonal
    with pytest.raises(ValueError, match="nothing to compare"):
        extract_mesh(m, coords, feats, resolution=24, level=level, deviation=2000)
