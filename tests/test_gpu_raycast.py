"""Rays against meshes on the GPU: cast_rays against ray_mesh_reference bit for bit on the cases of
tests/test_raycast_cpu.py -- tile and wave edges, the sphere plain, simplified, shifted and scaled, planted duplicates, invalid
indices, NaN vertices, NaN and zero directions, limits on t -- culled and not, twice; culling that really culls, and the schedule
of the walk held to the host's count; no host read; render_mesh of a sphere against the two spheres that enclose its facets; and
mesh_render_agreement and extract_mesh(agreement=) on the kernels."""
import math

import numpy as np
import pytest
import torch

from npcd.eval.mesh import point_mesh_distance_reference
from oracle import renderer as orr
from test_raycast_cpu import CASES, CENTRE, KEYS, SCHEDULE, TILE, WAVE, ball, case, hold, reference

pytestmark = pytest.mark.gpu

RADIUS = 0.6          # of the sphere in front of the cameras: the 24^3 sphere of radius 9.3 about CENTRE, scaled


def on_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(name, **options):
    from npcd.hip.raycast import cast_rays
    o, d, v, f, t_min, t_max = case(name)
    got = cast_rays(on_gpu(o), on_gpu(d), on_gpu(v), on_gpu(f), t_min=t_min, t_max=t_max, **options)
    assert all(t.is_cuda for t in got.values())
    return got


def sphere():
    """The sphere at the origin, inside the renderer's cube: (vertices, faces) on the GPU and as numpy."""
    v, f, _ = ball()
    v = ((v - np.float32(CENTRE)) * np.float32(RADIUS / 9.3)).astype(np.float32)
    return on_gpu(v), on_gpu(f.astype(np.int32)), v, f


def cameras(resolution, poses=((30.0, 20.0), (140.0, -35.0))):
    K = orr.srn_intrinsics().clone()
    K[0, 0] = K[1, 1] = 131.25 * resolution / 128
    K[0, 2] = K[1, 2] = resolution / 2
    return torch.stack([orr.look_at_pose(*p) for p in poses]).cuda(), K[None].repeat(len(poses), 1, 1).cuda()


@pytest.mark.parametrize("name", CASES)
def test_against_the_reference(name):
    reference(name)
    for cull in (True, False):
        for attempt in range(2):
            got = run(name, cull=cull)
            assert set(got) == set(KEYS)
            hold({k: t.cpu().numpy() for k, t in got.items()}, name, f"{name} cull {cull} run {attempt}")


def test_culling_really_culls():
    from npcd.hip.mesh_distance import mesh_boxes
    from npcd.hip.raycast import cast_rays
    from npcd.hip.render import ray_gen
    from npcd.eval.mesh import block_order
    v, f, _, _ = sphere()
    o, d, _, _ = ray_gen(*cameras(32, poses=((30.0, 20.0),)), 32, 1.0)
    order = block_order(32, o.device)
    o, d = o[0, order].contiguous(), d[0, order].contiguous()
    waves, tiles = -(-1024 // WAVE), -(-f.shape[0] // TILE)
    boxes = mesh_boxes(v, f)
    counts = {}
    for cull in (True, False):
        got = cast_rays(o, d, v, f, cull=cull, stats=True, boxes=boxes)
        assert set(got) == set(KEYS) | {"evaluated"} and got["evaluated"].dtype == torch.int64 and got["evaluated"].shape == (1,)
        counts[cull] = int(got["evaluated"])
        if not cull:
            assert all(torch.equal(got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k],
                                   first[k].view(torch.int32) if first[k].dtype == torch.float32 else first[k]) for k in KEYS)
        first = got
    print(f"evaluated (wave, tile) pairs of {waves * tiles}: culled {counts[True]} ({counts[True] / (waves * tiles):.3f})")
    assert 0 < counts[True] < waves * tiles == counts[False]
    assert int((first["face"] >= 0).sum()) > 100


@pytest.mark.parametrize("name", sorted(SCHEDULE))
def test_the_schedule_of_the_walk(name):
    """The kernel's waves evaluate exactly the (wave, tile) pairs that the host's walk over the same policy evaluates (SCHEDULE of
    tests/test_raycast_cpu.py): a wave holds the host's 64 consecutive rays; and every pair without culling."""
    count, pairs = SCHEDULE[name]
    culled, every = run(name, cull=True, stats=True), run(name, cull=False, stats=True)
    print(f"{name}: evaluated {int(culled['evaluated'])} of {int(every['evaluated'])} (wave, tile) pairs; the host's walk {count} of {pairs}")
    assert int(culled["evaluated"]) == count
    assert int(every["evaluated"]) == pairs == -(-len(case(name)[0]) // WAVE) * -(-len(case(name)[3]) // TILE)


def test_no_host_read():
    from npcd.hip.mesh_distance import mesh_boxes
    from npcd.hip.raycast import cast_rays
    for name in ("soup:513x257", "lost", "no_faces"):
        o, d, v, f = (on_gpu(a) for a in case(name)[:4])
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")          # a host read would raise
        try:
            got = cast_rays(o, d, v, f, stats=True)
            if f.shape[0]:
                again = cast_rays(o, d, v, f, boxes=mesh_boxes(v, f))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        hold({k: got[k].cpu().numpy() for k in KEYS}, name, f"{name} without a host read")
        if f.shape[0]:
            hold({k: again[k].cpu().numpy() for k in KEYS}, name, f"{name} without a host read, boxes given")


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.raycast import cast_rays
    o, d, v, f = (on_gpu(a) for a in case("soup:255x257")[:4])
    for bad in ((o.double(), d, v, f), (o, d.half(), v, f), (o, d, v.half(), f), (o, d, v, f.long()), (o.cpu(), d, v, f), (o, d, v, f.cpu()),
                (o, d.cpu(), v, f)):
        with pytest.raises(RuntimeError):
            cast_rays(*bad)
    for bad in ((o[:, :2], d, v, f), (o, d, v[None], f), (o, d, v, f.reshape(-1)), (o, d[:9], v, f)):
        with pytest.raises(ValueError):
            cast_rays(*bad)
    with pytest.raises(ValueError, match="boxes"):
        cast_rays(o, d, v, f, boxes=torch.zeros(8, dtype=torch.int64, device="cuda"))
    # strided inputs are what their contiguous copies are
    wide = torch.zeros(len(o), 5, device="cuda")
    wide[:, 1:4] = d
    got = cast_rays(o, wide[:, 1:4], v, f)
    hold({k: t.cpu().numpy() for k, t in got.items()}, "soup:255x257", "strided directions")


def test_render_mesh_of_the_sphere():
    """The facets of the sphere lie between two spheres about its centre: the inscribed one, whose radius is the distance from the
    centre to the nearest point of any face, and the circumscribed one through the farthest vertex.  A ray that passes the centre
    nearer than the first must hit the closed surface, one that passes farther than the second cannot, and a hit lies between the
    two: after the outer sphere's entry and, inside the inner sphere's silhouette, before the inner sphere's."""
    from npcd.eval.mesh import render_mesh
    from npcd.hip.raycast import cast_rays
    from npcd.hip.render import ray_gen
    v, f, v_host, f_host = sphere()
    r_in = math.sqrt(float(point_mesh_distance_reference(np.zeros((1, 3), np.float32), v_host, f_host)["sqdist"][0]))
    r_out = float(np.linalg.norm(v_host.astype(np.float64), axis=1).max())
    assert 0.9 * RADIUS < r_in < r_out < 1.01 * RADIUS
    extr, intr = cameras(32)
    view = render_mesh((v, f), extr, intr, 32, 1.0)
    again = render_mesh((v, f), extr, intr, 32, 1.0)
    assert {k: tuple(t.shape) for k, t in view.items()} == {"mask": (2, 1024, 1), "depth": (2, 1024, 1), "face": (2, 1024), "normal": (2, 1024, 3), "channels": (2, 1024, 3)}
    for k in view:
        assert torch.equal(view[k].view(torch.int32) if view[k].dtype == torch.float32 else view[k],
                           again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k]), k
    o, d, _, t1 = ray_gen(extr, intr, 32, 1.0)
    direct = cast_rays(o.reshape(-1, 3), d.reshape(-1, 3), v, f)
    assert torch.equal(view["face"].reshape(-1), direct["face"])
    assert torch.equal(view["depth"].reshape(-1).view(torch.int32), torch.where(direct["face"] >= 0, direct["t"], t1.reshape(-1)).view(torch.int32))
    o64, d64 = o.double().cpu().numpy(), d.double().cpu().numpy()
    along = -(o64 * d64).sum(-1) / (d64 * d64).sum(-1)          # the parameter of the point nearest to the centre
    passes = np.linalg.norm(o64 + along[..., None] * d64, axis=-1)
    length = np.linalg.norm(d64, axis=-1)
    covered = view["mask"][..., 0].cpu().numpy() > 0.5
    slop = 1e-5          # of fp32 rays at a distance near 1: the pixels within it of either silhouette are not asked
    assert covered[passes < r_in * (1 - slop)].all() and not covered[passes > r_out * (1 + slop)].any()
    assert (passes < r_in * (1 - slop)).sum() > 200 and (passes > r_out * (1 + slop)).sum() > 200
    depth = view["depth"][..., 0].double().cpu().numpy()
    enter = lambda r: along - np.sqrt(np.maximum(r * r - passes * passes, 0.0)) / length
    assert (depth[covered] >= enter(r_out)[covered] - slop).all()
    inner = covered & (passes < r_in * (1 - slop))
    assert (depth[inner] <= enter(r_in)[inner] + slop).all()
    print(f"32 x 32, two views: {covered.sum()} pixels covered; radii {r_in:.5f} and {r_out:.5f}; the hits lie "
          f"{(depth[inner] - enter(r_out)[inner]).max():.5f} at most behind the outer sphere")
    # seen from outside, every hit is a front face with a unit normal toward the camera; the shading is grey, the rest white
    normal, toward = view["normal"].double().cpu().numpy(), d64 / length[..., None]
    assert np.allclose(np.linalg.norm(normal[covered], axis=1), 1.0, atol=1e-6) and ((normal * toward).sum(-1)[covered] < 0).all()
    assert torch.equal(view["channels"][~(view["mask"][..., 0] > 0.5)], torch.ones(int((~covered).sum()), 3, device="cuda"))
    assert float(view["channels"][view["mask"][..., 0] > 0.5].max()) <= 0.75


def test_agreement_on_the_kernels():
    """With untrained weights nobody knows how well the mesh agrees with the field: the keys, the ranges and the repeatability are
    what is held, and that asking for the report changes nothing else."""
    from npcd.eval.mesh import extract_mesh, mesh_render_agreement
    from test_gpu_field_query import _model, _on_gpu
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma, _, _ = m.density_grid(coords, feats, resolution=24)
    level = float(sigma[sigma > 0].median())          # a surface exists with untrained weights
    extr, intr = cameras(24)
    plain = extract_mesh(m, coords, feats, resolution=24, level=level)
    asked = extract_mesh(m, coords, feats, resolution=24, level=level, agreement=(extr, intr, 24))
    again = extract_mesh(m, coords, feats, resolution=24, level=level, agreement=(extr, intr, 24))
    names = {"iou", "depth_mean", "depth_max", "psnr", "ssim"}
    for b in range(len(plain)):
        assert set(asked[b]) == set(plain[b]) | {"agreement"} and "agreement" not in plain[b]
        for key, t in plain[b].items():
            assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t, asked[b][key].view(torch.int32) if t.dtype == torch.float32 else asked[b][key]), key
        report = asked[b]["agreement"]
        print(f"cloud {b}: { {k: report[k] for k in sorted(names)} }")
        assert set(report) == names | {"views"} and len(report["views"]) == 2 and all(set(v) == names for v in report["views"])
        assert 0.0 <= report["iou"] <= 1.0 and all(0.0 <= v["iou"] <= 1.0 for v in report["views"])
        assert all(math.isfinite(report[k]) for k in ("iou", "psnr", "ssim")) and -1.0 <= report["ssim"] <= 1.0 and report["psnr"] > 0
        assert repr(report) == repr(again[b]["agreement"])          # equal dicts, NaN included
        direct = mesh_render_agreement(m, coords[b:b + 1], feats[b:b + 1], plain[b], extr, intr, resolution=24)
        assert repr(direct) == repr(report)
