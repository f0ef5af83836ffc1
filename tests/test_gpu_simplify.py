"""The vertex clustering kernels (csrc/simplify.hip, npcd.hip.simplify) against the CPU restatement of their specification
(npcd.eval.mesh.simplify_reference, itself held to geometry and the exact cases by tests/test_simplify_cpu.py): every output --
vertices, faces, attributes, vertex_cluster, face_source -- is equal bit for bit, and equal again on a second run.

The meshes are those of tests/test_simplify_cpu.py, where the kernels' per-lane code has already run on the host: triangle soups of
1, 4, 63, 64, 65, 255, 256, 257 and 16,387 faces with planted duplicates; grids 31, 32, 33 and 65 cells wide, so that keys straddle
bitmap words; grids of one and of 256 scan strips plus two words with vertices in the first and the last cell only (the two-level
rank, and the carry of its second level); one cell for everything, a cell for every vertex, 1 % lost vertices, indices outside
[0, V), no faces, no vertices, nothing finite; the 24^3 sphere isosurface at k = 2 with colours and normals; 1 and 16 attribute
channels; the two-pass sort forced."""
import numpy as np
import pytest
import torch

from test_simplify_cpu import CASES, STRIP, case, grid_of, hold, reference, soup

pytestmark = pytest.mark.gpu


def on_gpu(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def simplify(c):
    from npcd.hip.simplify import simplify_mesh
    got = simplify_mesh(on_gpu(c["vertices"]), on_gpu(c["faces"]), c["cell"], origin=c["origin"], dims=c["dims"],
                        attributes=on_gpu(c["attributes"]), two_pass_sort=c["two_pass"])
    assert all(t.is_cuda for t in got.values())
    return got


@pytest.mark.parametrize("name", CASES)
def test_against_the_reference(name):
    from npcd.hip.simplify import STRIP_WORDS
    assert STRIP_WORDS == STRIP
    c = case(name)
    got, again = simplify(c), simplify(c)
    assert sorted(got) == sorted(again)
    for key in got:
        assert got[key].dtype == again[key].dtype and torch.equal(got[key].view(torch.int32), again[key].view(torch.int32)), \
            f"{name}: {key} differs between two runs"
    hold({k: v.cpu().numpy() for k, v in got.items()}, name, name)
    want = reference(name)
    for key in got:          # torch.equal, value for value (no NaN can arise: every mean is one of finite integers)
        assert torch.equal(got[key].cpu(), torch.from_numpy(want[key])), (name, key)


def test_the_sphere_from_the_gpu_isosurface():
    """isosurface -> simplify_mesh at k = 2 with colours and normals as six channels: the mesh is the reference's, so the result is
    the sphere:2 case's."""
    from npcd.hip.isosurface import isosurface
    from npcd.hip.simplify import simplify_mesh
    from test_isosurface_cpu import sphere_volume
    from test_simplify_cpu import sphere_grid
    vol, origin, spacing = sphere_volume((24, 24, 24), radius=0.6)
    ((v, f, n),) = isosurface(torch.from_numpy(vol).cuda(), 0.0, origin, spacing, normals=True)
    colours = on_gpu(case("sphere:2")["attributes"][:, :3])
    got = simplify_mesh(v, f, attributes=torch.cat([colours, n], dim=1), **sphere_grid(24, 2, origin, spacing))
    hold({k: t.cpu().numpy() for k, t in got.items()}, "sphere:2", "from the GPU isosurface")
    assert 0 < got["faces"].shape[0] < f.shape[0]


def test_two_pass_sort_equals_one_pass():
    one, two = simplify(case("two_pass:off")), simplify(case("two_pass:on"))
    for key in one:
        assert torch.equal(one[key], two[key]), key
    c = case("faces:16387")
    forced = simplify(dict(c, two_pass=True))
    hold({k: v.cpu().numpy() for k, v in forced.items()}, "faces:16387", "two passes")


def test_the_entry_points_write_their_outputs_and_nothing_else():
    """Direct C calls on another stream; every output and the workspace lie between guard bands and are poisoned before: a row that
    is not written shows, and so does a write outside."""
    import ctypes

    from npcd import hip
    L = hip.lib()
    name = "lost"
    c = case(name)
    want = reference(name)
    origin, cell, dims = grid_of(c)
    org, step, size = (ctypes.c_double * 3)(*origin), (ctypes.c_double * 3)(*cell), (ctypes.c_int * 3)(*dims)
    vertices, faces, attrs = on_gpu(c["vertices"]), on_gpu(c["faces"]), on_gpu(c["attributes"])
    V, F, C = vertices.shape[0], faces.shape[0], attrs.shape[1]
    Vp, Fp = len(want["vertices"]), len(want["faces"])
    guard = 64
    poison = float(np.float32(-7.25))

    def banded(count, dtype, fill):
        return torch.full((guard + count + guard,), fill, dtype=dtype, device="cuda")
    ws_words = (L.npcd_simplify_ws_bytes(V, F, C, size) + 7) // 8
    ws = banded(ws_words, torch.int64, 0x5a5a5a5a5a5a5a5a)
    cluster, counts = banded(V, torch.int32, -7), banded(2, torch.int64, -7)
    key_lo, key_hi = banded(F, torch.int64, -7), banded(F, torch.int64, -7)
    v_out, a_out = banded(Vp * 3, torch.float32, poison), banded(Vp * C, torch.float32, poison)
    f_out, source = banded(Fp * 3, torch.int32, -7), banded(Fp, torch.int32, -7)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    P = hip.ptr
    with torch.cuda.stream(side):
        hip.check(L.npcd_simplify_cluster(P(vertices), V, F, P(attrs), C, org, step, size, P(ws[guard:]), P(cluster[guard:]), P(counts[guard:]),
                                          hip.stream_ptr()), "npcd_simplify_cluster")
        hip.check(L.npcd_simplify_faces(P(faces), V, F, C, size, P(cluster[guard:]), P(ws[guard:]), P(key_hi[guard:]), P(key_lo[guard:]),
                                        hip.stream_ptr()), "npcd_simplify_faces")
        order = torch.sort(key_lo[guard:-guard], stable=True)[1]
        order = order[torch.sort(key_hi[guard:-guard][order], stable=True)[1]].contiguous()
        hip.check(L.npcd_simplify_unique(P(order), V, F, C, size, P(ws[guard:]), P(counts[guard:]), hip.stream_ptr()), "npcd_simplify_unique")
        assert counts[guard:-guard].tolist() == [Vp, Fp]
        hip.check(L.npcd_simplify_emit(V, F, C, org, step, size, P(ws[guard:]), Vp, Fp, P(v_out[guard:]), P(a_out[guard:]), P(f_out[guard:]),
                                       P(source[guard:]), hip.stream_ptr()), "npcd_simplify_emit")
    side.synchronize()
    for t, fill in ((ws, 0x5a5a5a5a5a5a5a5a), (cluster, -7), (counts, -7), (key_lo, -7), (key_hi, -7), (v_out, poison), (a_out, poison),
                    (f_out, -7), (source, -7)):
        assert (t[:guard] == fill).all() and (t[-guard:] == fill).all()
    got = {"vertices": v_out[guard:-guard].reshape(Vp, 3), "attributes": a_out[guard:-guard].reshape(Vp, C), "faces": f_out[guard:-guard].reshape(Fp, 3),
           "vertex_cluster": cluster[guard:-guard], "face_source": source[guard:-guard]}
    hold({k: v.cpu().numpy() for k, v in got.items()}, name, "direct calls")
    # the refusals launch nothing: the outputs keep their bits
    before = v_out.clone()
    assert L.npcd_simplify_emit(V, F, C, org, step, size, P(ws[guard:]), V + 1, Fp, P(v_out[guard:]), P(a_out[guard:]), P(f_out[guard:]),
                                P(source[guard:]), hip.stream_ptr()) == -1
    assert L.npcd_simplify_emit(V, F, 17, org, step, size, P(ws[guard:]), Vp, Fp, P(v_out[guard:]), P(a_out[guard:]), P(f_out[guard:]),
                                P(source[guard:]), hip.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert torch.equal(before, v_out)


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.simplify import simplify_mesh
    v, f = (torch.from_numpy(a).cuda() for a in soup(10))
    with pytest.raises(RuntimeError):
        simplify_mesh(v.double(), f, 0.1)
    with pytest.raises(RuntimeError):
        simplify_mesh(v, f.long(), 0.1)
    with pytest.raises(RuntimeError, match="GPU"):
        simplify_mesh(v, f, 0.1, attributes=torch.zeros(len(v), 3))
    with pytest.raises(RuntimeError):
        simplify_mesh(v, f, 0.1, attributes=torch.zeros(len(v), 3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        simplify_mesh(v, f, 0.1, attributes=torch.zeros(len(v), 17, device="cuda"))
    with pytest.raises(ValueError):
        simplify_mesh(v, f, 0.1, attributes=torch.zeros(len(v) + 1, 3, device="cuda"))
    with pytest.raises(ValueError, match="cell"):
        simplify_mesh(v, f, 0.0)
    with pytest.raises(ValueError, match=r"1025 x 1024 x 1024 = 1074790400 cells"):
        simplify_mesh(v, f, 1.0, origin=[0, 0, 0], dims=[1025, 1024, 1024])
    with pytest.raises(ValueError, match="cells"):
        simplify_mesh(v, f, 1e-7)                                                  # the grid from the bounds would be too large


def test_simplified_meshes_feed_the_samplers_and_the_file(tmp_path):
    """extract_mesh(simplify=2) -> sample_mesh_clouds -> shape_metrics on two tiny batches, and write_ply on one of the meshes."""
    from npcd.eval.mesh import extract_mesh, sample_mesh_clouds, write_ply
    from npcd.eval.shapes import shape_metrics
    from test_gpu_field_query import _model, _on_gpu
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma = m.density_grid(coords, feats, resolution=24)[0]
    level = float(sigma[sigma > 0].median())          # a surface exists with untrained weights
    plain = extract_mesh(m, coords, feats, resolution=24, level=level, normals=True)
    coarse = extract_mesh(m, coords, feats, resolution=24, level=level, normals=True, simplify=2)
    again = extract_mesh(m, coords, feats, resolution=24, level=level, normals=True, simplify=None)
    batches = []
    for full, same, mesh in zip(plain, again, coarse):
        assert all(torch.equal(full[k], same[k]) for k in full) and sorted(full) == sorted(same)
        assert 0 < mesh["faces"].shape[0] < full["faces"].shape[0] and mesh["vertices"].shape[0] < full["vertices"].shape[0]
        assert mesh["colors"].shape == mesh["normals"].shape == mesh["vertices"].shape
        assert mesh["vertex_cluster"].shape[0] == full["vertices"].shape[0] and int(mesh["faces"].max()) < mesh["vertices"].shape[0]
        length = torch.linalg.norm(mesh["normals"], dim=1)
        assert (((length - 1).abs() < 1e-5) | (length == 0)).all()
        assert float(mesh["colors"].min()) >= 0.0 and float(mesh["colors"].max()) <= 1.0
    for meshes in (plain, coarse):
        clouds, normals = sample_mesh_clouds(meshes, 256, generator=torch.Generator(device="cuda").manual_seed(3), normals=True)
        assert clouds.shape == normals.shape == (len(meshes), 256, 3) and torch.isfinite(clouds).all() and torch.isfinite(normals).all()
        batches.append(clouds)
    metrics = shape_metrics(batches[0], batches[1], emd=True, jsd=True)
    for key in ("mmd_cd", "cov_cd", "nna_cd", "mmd_emd", "jsd"):
        assert np.isfinite(float(metrics[key])) and float(metrics[key]) >= 0, (key, metrics[key])
    mesh = coarse[0]
    path = str(tmp_path / "coarse.ply")
    write_ply(path, mesh["vertices"], mesh["faces"], colors=mesh["colors"], normals=mesh["normals"])
    header = open(path, "rb").read(600).split(b"end_header")[0].decode("ascii")
    assert f"element vertex {mesh['vertices'].shape[0]}\n" in header and f"element face {mesh['faces'].shape[0]}\n" in header
