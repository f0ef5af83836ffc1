"""The surface sampling kernels (csrc/surface.hip, npcd.hip.surface) against the CPU restatement of their specification
(npcd.eval.mesh.surface_sample_reference, itself held to geometry, statistics and the exact cases by
tests/test_surface_sampling_cpu.py): every output -- points, face, area, normals, attributes -- is equal bit for bit, and equal again
on a second run.

The meshes are those of tests/test_surface_sampling_cpu.py, where the kernels' per-lane code has already run on the host: random
triangle soups of 1, 4, T - 1, T, T + 1, 2 T + 1 and 64 T + 3 faces (T = TILE_FACES) and one of one tile more than a sampling
workgroup stages in LDS; 1, 63, 64, 65 and 2,048 samples; a batch of differing sizes with an empty and an all-degenerate member, a
small real isosurface, faces that must never be chosen and vertex normals that are not finite; 1, 3 and 16 attribute channels; the
exact cases of the specification."""
import numpy as np
import pytest
import torch

from test_surface_sampling_cpu import BIG, CASES, LDS_TILES, T, case, hold, pack, same_bits, soup

pytestmark = pytest.mark.gpu


def on_gpu(c):
    """-> (meshes, u, normals, attributes) of a case as the wrapper takes them."""
    meshes = [tuple(torch.from_numpy(np.array(a)).cuda() for a in m) for m in c["meshes"]]
    lift = lambda rows: None if rows is None or isinstance(rows, str) else [torch.from_numpy(np.array(r)).cuda() for r in rows]
    normals = c["normals"] if isinstance(c["normals"], str) else lift(c["normals"])
    return meshes, torch.from_numpy(np.array(c["u"])).cuda(), normals, lift(c["attributes"])


def sample(c, meshes, u, normals, attributes):
    from npcd.hip.surface import sample_surface
    got = list(sample_surface(meshes, u.shape[-2], u=u, normals=normals, attributes=attributes, return_faces=True))
    keys = ["points", "area"] + (["normals"] if normals is not None else []) + (["attributes"] if attributes is not None else []) + ["face"]
    assert len(got) == len(keys)
    assert all(t.is_cuda for t in got)
    return dict(zip(keys, got))


@pytest.mark.parametrize("name", CASES)
def test_against_the_reference(name):
    from npcd.hip.surface import TILE_FACES, LDS_TILES as wrapper_lds_tiles
    assert TILE_FACES == T and wrapper_lds_tiles == LDS_TILES and BIG > T * LDS_TILES
    c = case(name)
    args = on_gpu(c)
    got = sample(c, *args)
    again = sample(c, *args)
    for key in got:
        assert torch.equal(got[key].view(torch.int32 if got[key].dtype != torch.float64 else torch.int64),
                           again[key].view(torch.int32 if again[key].dtype != torch.float64 else torch.int64)), f"{name}: {key} differs between two runs"
    B, S = c["u"].shape[:2]
    assert got["points"].shape == (B, S, 3) and got["face"].shape == (B, S) and got["face"].dtype == torch.int32
    assert got["area"].shape == (B,) and got["area"].dtype == torch.float64
    hold({k: v.cpu().numpy() for k, v in got.items()}, name, name)


def test_every_member_equals_the_mesh_sampled_alone():
    from npcd.hip.surface import sample_surface, surface_area
    c = case("batch")
    meshes, u, normals, attributes = on_gpu(c)
    whole = sample_surface(meshes, u.shape[1], u=u, normals=normals, attributes=attributes, return_faces=True)
    areas = surface_area(meshes)
    assert torch.equal(areas, whole[1])
    for b, mesh in enumerate(meshes):
        alone = sample_surface(mesh, u.shape[1], u=u[b], normals=normals[b], attributes=attributes[b], return_faces=True)
        for key, one, batched in zip(("points", "area", "normals", "attributes", "face"), alone, whole):
            assert one.shape == batched[b].shape, (b, key)
            same_bits(one.cpu().numpy(), batched[b].cpu().numpy(), f"member {b}: {key}")
        same_bits(surface_area(mesh).cpu().numpy(), areas[b].cpu().numpy(), f"member {b}: surface_area")
    # as dicts, and with the face normals of the winding
    as_dicts = [{"vertices": v, "faces": f} for v, f in meshes]
    points, _, face_normals = sample_surface(as_dicts, u.shape[1], u=u, normals="face")
    assert torch.equal(points, whole[0])
    for b, (v, f) in enumerate(c["meshes"]):
        from npcd.eval.mesh import surface_sample_reference
        same_bits(face_normals[b].cpu().numpy(), surface_sample_reference(v, f, c["u"][b], normals="face")["normals"], f"member {b}: face normals")


def test_the_entry_points_write_their_outputs_and_nothing_else():
    """Direct C calls on another stream; every output and the workspace lie between guard bands and are poisoned before: a row that
    is not written shows, and so does a write outside."""
    from npcd import hip
    L = hip.lib()
    c = case("batch")
    vertices, faces, vo, fo, mode, vn, at = pack(c)
    B, S = c["u"].shape[:2]
    C = at.shape[1]
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    vertices, faces, vo, fo, vn, at, u = (dev(a) for a in (vertices, faces, vo, fo, vn, at, c["u"]))
    guard = 64
    poison = float(np.float32(-7.25))

    def banded(count, dtype, fill):
        return torch.full((guard + count + guard,), fill, dtype=dtype, device="cuda")
    ws_words = (L.npcd_surface_ws_bytes(B, faces.shape[0]) + 7) // 8
    ws = banded(ws_words, torch.int64, 0x5a5a5a5a5a5a5a5a)
    area = banded(B, torch.float64, poison)
    points, normals, attrs = banded(B * S * 3, torch.float32, poison), banded(B * S * 3, torch.float32, poison), banded(B * S * C, torch.float32, poison)
    face = banded(B * S, torch.int32, -7)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    P = hip.ptr
    with torch.cuda.stream(side):
        hip.check(L.npcd_surface_prepare(P(vertices), P(faces), P(vo), P(fo), B, vertices.shape[0], faces.shape[0], P(ws[guard:]), P(area[guard:]),
                                         hip.stream_ptr()), "npcd_surface_prepare")
        hip.check(L.npcd_surface_sample(P(vertices), P(faces), P(vo), P(fo), B, vertices.shape[0], faces.shape[0], P(ws[guard:]), P(u), S,
                                        P(points[guard:]), P(face[guard:]), mode, P(vn), P(normals[guard:]), P(at), C, P(attrs[guard:]),
                                        hip.stream_ptr()), "npcd_surface_sample")
    side.synchronize()
    for t, fill in ((ws, 0x5a5a5a5a5a5a5a5a), (area, poison), (points, poison), (normals, poison), (attrs, poison), (face, -7)):
        assert (t[:guard] == fill).all() and (t[-guard:] == fill).all()
    got = {"area": area[guard:-guard], "points": points[guard:-guard].reshape(B, S, 3), "face": face[guard:-guard].reshape(B, S),
           "normals": normals[guard:-guard].reshape(B, S, 3), "attributes": attrs[guard:-guard].reshape(B, S, C)}
    hold({k: v.cpu().numpy() for k, v in got.items()}, "batch", "direct calls")
    # the refusals launch nothing: the outputs keep their bits
    before = points.clone()
    assert L.npcd_surface_sample(P(vertices), P(faces), P(vo), P(fo), B, vertices.shape[0], faces.shape[0], P(ws[guard:]), P(u), 0,
                                 P(points[guard:]), None, 0, None, None, None, 0, None, hip.stream_ptr()) == -1
    assert L.npcd_surface_sample(P(vertices), P(faces), P(vo), P(fo), B, vertices.shape[0], faces.shape[0], P(ws[guard:]), P(u), S,
                                 P(points[guard:]), None, 0, None, None, P(at), 17, P(attrs[guard:]), hip.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert torch.equal(before, points)


def test_default_draws_and_the_generator():
    from npcd.hip.surface import sample_surface
    v, f = (torch.from_numpy(a).cuda() for a in soup(2 * T + 1, 1))
    g = torch.Generator(device="cuda").manual_seed(5)
    first = sample_surface([(v, f), (v, f)], 100, generator=g, return_faces=True)
    u = torch.rand((2, 100, 3), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    given = sample_surface([(v, f), (v, f)], 100, u=u, return_faces=True)
    for a, b in zip(first, given):
        assert torch.equal(a, b)
    assert not torch.equal(first[2][0], first[2][1])          # the members draw their own numbers
    assert first[0].shape == (2, 100, 3) and torch.isfinite(first[0]).all()


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.surface import sample_surface
    v, f = (torch.from_numpy(a).cuda() for a in soup(10))
    with pytest.raises(RuntimeError):
        sample_surface((v.double(), f), 4)
    with pytest.raises(RuntimeError):
        sample_surface((v, f.long()), 4)
    with pytest.raises(RuntimeError):
        sample_surface((v, f), 4, u=torch.rand(4, 3))                                      # u not on the GPU
    with pytest.raises(ValueError):
        sample_surface((v, f), 4, u=torch.rand(5, 3, device="cuda"))
    with pytest.raises(ValueError):
        sample_surface((v, f), 4, normals="vertex")
    with pytest.raises(ValueError):
        sample_surface((v, f), 4, normals=torch.zeros(len(v) + 1, 3, device="cuda"))
    with pytest.raises(ValueError):
        sample_surface((v, f), 4, attributes=torch.zeros(len(v), 17, device="cuda"))
    with pytest.raises(ValueError):
        sample_surface([(v, f), (v, f)], 4, attributes=[torch.zeros(len(v), 3, device="cuda")])
    with pytest.raises(RuntimeError):
        sample_surface((v, f), 4, attributes=torch.zeros(len(v), 3, dtype=torch.float64, device="cuda"))


def test_clouds_of_meshes_feed_the_shape_metrics():
    """isosurface -> sample_mesh_clouds -> shape_metrics, end to end on two tiny batches: spheres of slightly different radii."""
    from npcd.eval.mesh import sample_mesh_clouds
    from npcd.eval.shapes import shape_metrics
    from npcd.hip.isosurface import isosurface
    from test_isosurface_cpu import sphere_volume
    batches = []
    for shift in (0.0, 0.02):
        vols = np.stack([sphere_volume((17, 17, 17), radius=0.5 + shift + 0.03 * i)[0] for i in range(4)])
        _, origin, spacing = sphere_volume((17, 17, 17))
        meshes = isosurface(torch.from_numpy(vols).cuda(), 0.0, origin, spacing, normals=True)
        clouds, normals = sample_mesh_clouds(meshes, 256, generator=torch.Generator(device="cuda").manual_seed(3), normals=True)
        assert clouds.shape == normals.shape == (4, 256, 3) and clouds.is_cuda
        radius = torch.linalg.norm(clouds - torch.tensor([0.013, -0.021, 0.034], device="cuda"), dim=-1)
        want = torch.tensor([0.5 + shift + 0.03 * i for i in range(4)], device="cuda")[:, None]
        # faces an eighth wide: an edge is at most sqrt(3) / 8 long, its chord lies (sqrt(3) / 8)^2 / (8 r) = 0.012 inside the sphere at
        # r = 0.5, and the vertices lie off it by the interpolation of a distance field, far less: four times that
        assert ((radius - want).abs() < 0.05).all()
        assert (torch.linalg.norm(normals, dim=-1) - 1).abs().max() < 1e-6
        batches.append(clouds)
    assert sample_mesh_clouds(meshes[0], 16).shape == (1, 16, 3)          # one mesh as isosurface returns it
    metrics = shape_metrics(batches[0], batches[1], emd=True, jsd=True)
    assert metrics["num_generated"] == metrics["num_reference"] == 4
    for key in ("mmd_cd", "cov_cd", "nna_cd", "mmd_emd", "jsd"):
        assert np.isfinite(float(metrics[key])) and float(metrics[key]) >= 0, (key, metrics[key])
    same = shape_metrics(batches[0], batches[0])
    assert same["mmd_cd"] == 0.0 and metrics["mmd_cd"] > 0.0
