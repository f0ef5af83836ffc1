"""The mesh-edges and smoothing kernels (csrc/smooth.hip, npcd.hip.smooth) against the CPU restatements of their specification
(npcd.eval.mesh.mesh_edges_reference and smooth_reference, themselves held to geometry and the exact cases by
tests/test_smooth_cpu.py): every output -- row_start, neighbours, edges, edge_faces, edge_forward, boundary_vertex, counts and the
smoothed vertices -- is equal bit for bit, and equal again on a second run.

The meshes are those of tests/test_smooth_cpu.py, where the kernels' per-lane code has already run on the host: triangle soups of 1,
4, 42, 43, 63, 64, 65, 255, 256, 257 and 16,387 faces over so few vertices that edges repeat, with planted duplicate and reversed
faces (42 and 43 faces put 6F on both sides of a strip of 256 keys); a fan of 300 faces round one vertex; 1 % lost vertices; indices
outside [0, V); no faces, no vertices, no valid face; valid faces at the first and the last vertex only; the 24^3 sphere closed and
open, plain and simplified, at 0, 1, 2 and 10 iterations; mu = 0; pinned vertices; coordinates of 2^100 and 2^-100."""
import numpy as np
import pytest
import torch

from test_smooth_cpu import CASES, EDGE_KEYS, STRIP, ball, case, hold, reference, soup

pytestmark = pytest.mark.gpu


def on_gpu(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def run(c, edges=None):
    """-> the dict of mesh_edges plus "vertices", the smoothed ones."""
    from npcd.hip.smooth import mesh_edges, smooth_mesh
    vertices, faces = on_gpu(c["vertices"]), on_gpu(c["faces"])
    got = dict(mesh_edges(len(vertices), faces)) if edges is None else dict(edges)
    got["vertices"] = smooth_mesh(vertices, faces, c["iterations"], c["lam"], c["mu"], fixed=on_gpu(c["fixed"]), fix_boundary=c["fix_boundary"],
                                  edges=edges)
    assert all(t.is_cuda for t in got.values())
    return got


def raw(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", CASES)
def test_against_the_references(name):
    from npcd.hip.smooth import STRIP_KEYS
    assert STRIP_KEYS == STRIP
    c = case(name)
    got, again = run(c), run(c)
    assert sorted(got) == sorted(again) == sorted(EDGE_KEYS + ("vertices",))
    for key in got:
        assert got[key].dtype == again[key].dtype and torch.equal(raw(got[key]), raw(again[key])), f"{name}: {key} differs between two runs"
    hold({k: v.cpu().numpy() for k, v in got.items()}, name, name)


def test_the_sphere_from_the_gpu_isosurface():
    """isosurface -> mesh_edges, smooth_mesh, and simplify_mesh -> the same: the meshes are the references', so the results are those
    of the ball cases.  mesh_topology on tensors reads the kernels' counts."""
    from npcd.eval.mesh import mesh_topology
    from npcd.hip.isosurface import isosurface
    from npcd.hip.simplify import simplify_mesh
    from npcd.hip.smooth import mesh_edges, smooth_mesh
    for radius, plain, coarse, boundary in ((9.3, "ball:2", "coarse_ball:2", 0), (14.5, "open_ball:2", "coarse_open_ball:2", 720)):
        ((v, f),) = isosurface(torch.from_numpy(ball(radius)[2]).cuda(), 0.0, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
        got = dict(mesh_edges(len(v), f), vertices=smooth_mesh(v, f, 2))
        hold({k: t.cpu().numpy() for k, t in got.items()}, plain, f"{plain} from the GPU isosurface")
        t = mesh_topology(len(v), f)
        assert t["boundary_edges"] == boundary and t["closed"] == (boundary == 0) and t["euler_characteristic"] == (2 if boundary == 0 else -4)
        small = simplify_mesh(v, f, 2.0, origin=[0.0, 0.0, 0.0], dims=[12, 12, 12])
        got = dict(mesh_edges(len(small["vertices"]), small["faces"]), vertices=smooth_mesh(small["vertices"], small["faces"], 2))
        hold({k: t.cpu().numpy() for k, t in got.items()}, coarse, f"{coarse} from the GPU simplification")


def test_edges_given_equal_edges_recomputed_without_a_host_read():
    from npcd.hip.smooth import mesh_edges
    for name in ("noisy:pinned", "faces:257", "lost"):
        c = case(name)
        edges = mesh_edges(len(c["vertices"]), on_gpu(c["faces"]))
        vertices, fixed = on_gpu(c["vertices"]), on_gpu(c["fixed"])
        torch.cuda.synchronize()
        from npcd.hip.smooth import smooth_mesh
        torch.cuda.set_sync_debug_mode("error")          # a host read would raise
        try:
            given = smooth_mesh(vertices, None, c["iterations"], c["lam"], c["mu"], fixed=fixed, fix_boundary=c["fix_boundary"], edges=edges)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(raw(given), raw(run(c)["vertices"])), name
        hold({"vertices": given.cpu().numpy()}, name, f"{name} with edges given", keys=("vertices",))


def test_the_entry_points_write_their_outputs_and_nothing_else():
    """Direct C calls on another stream; every output and the workspaces lie between guard bands and are poisoned before: an entry that
    is not written shows, and so does a write outside."""
    from npcd import hip
    L = hip.lib()
    name = "lost"
    c, want = case(name), reference(name)
    vertices, faces = on_gpu(c["vertices"]), on_gpu(c["faces"])
    V, F = vertices.shape[0], faces.shape[0]
    D = int(want["counts"][0])
    guard = 64

    def banded(count, dtype, fill):
        return torch.full((guard + count + guard,), fill, dtype=dtype, device="cuda")
    poison = float(np.float32(-7.25))
    keys = banded(6 * F, torch.int64, -7)
    ws = banded((L.npcd_mesh_edges_ws_bytes(V, F) + 7) // 8, torch.int64, 0x5a5a5a5a5a5a5a5a)
    state = banded((L.npcd_smooth_ws_bytes(V) + 7) // 8, torch.int64, 0x5a5a5a5a5a5a5a5a)
    counts = banded(6, torch.int64, -7)
    row_start, neighbours = banded(V + 1, torch.int32, -7), banded(D, torch.int32, -7)
    edges, edge_faces, edge_forward = banded(D, torch.int32, -7), banded(D // 2, torch.int32, -7), banded(D // 2, torch.int32, -7)
    boundary, v_out = banded(V, torch.uint8, 7), banded(V * 3, torch.float32, poison)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    P = hip.ptr
    with torch.cuda.stream(side):
        hip.check(L.npcd_mesh_edges_keys(P(faces), V, F, P(keys[guard:]), hip.stream_ptr()), "npcd_mesh_edges_keys")
        ordered = torch.sort(keys[guard:-guard])[0].contiguous()
        hip.check(L.npcd_mesh_edges_unique(P(ordered), V, F, P(ws[guard:]), P(counts[guard:]), hip.stream_ptr()), "npcd_mesh_edges_unique")
        assert counts[guard:-guard].tolist() == [D, int(want["counts"][1]), 0, 0, 0, 0]
        hip.check(L.npcd_mesh_edges_emit(P(ordered), V, F, P(ws[guard:]), D, P(row_start[guard:]), P(neighbours[guard:]), P(edges[guard:]),
                                         P(edge_faces[guard:]), P(edge_forward[guard:]), P(boundary[guard:]), P(counts[guard:]),
                                         hip.stream_ptr()), "npcd_mesh_edges_emit")
        hip.check(L.npcd_smooth_mesh(P(vertices), V, P(row_start[guard:]), P(neighbours[guard:]), D, None, None, c["iterations"], c["lam"],
                                     c["mu"], P(state[guard:]), P(v_out[guard:]), hip.stream_ptr()), "npcd_smooth_mesh")
    side.synchronize()
    for t, fill in ((keys, -7), (ws, 0x5a5a5a5a5a5a5a5a), (state, 0x5a5a5a5a5a5a5a5a), (counts, -7), (row_start, -7), (neighbours, -7),
                    (edges, -7), (edge_faces, -7), (edge_forward, -7), (boundary, 7), (v_out, poison)):
        assert (t[:guard] == fill).all() and (t[-guard:] == fill).all()
    inner = lambda t: t[guard:-guard]
    got = {"row_start": inner(row_start), "neighbours": inner(neighbours), "edges": inner(edges).reshape(-1, 2), "edge_faces": inner(edge_faces),
           "edge_forward": inner(edge_forward), "boundary_vertex": inner(boundary), "counts": inner(counts), "vertices": inner(v_out).reshape(V, 3)}
    hold({k: v.cpu().numpy() for k, v in got.items()}, name, "direct calls")          # the case does not pin the boundary
    # the refusals launch nothing: the outputs keep their bits
    before = v_out.clone()
    assert L.npcd_smooth_mesh(P(vertices), V, P(row_start[guard:]), P(neighbours[guard:]), D, None, None, 1001, c["lam"], c["mu"],
                              P(state[guard:]), P(v_out[guard:]), hip.stream_ptr()) == -1
    assert L.npcd_smooth_mesh(P(vertices), 2 ** 31, P(row_start[guard:]), P(neighbours[guard:]), D, None, None, 1, c["lam"], c["mu"],
                              P(state[guard:]), P(v_out[guard:]), hip.stream_ptr()) == -2
    torch.cuda.synchronize()
    assert torch.equal(raw(before), raw(v_out))


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.smooth import mesh_edges, smooth_mesh
    v, f = (torch.from_numpy(a).cuda() for a in soup(10))
    with pytest.raises(RuntimeError):
        mesh_edges(len(v), f.long())
    with pytest.raises(RuntimeError):
        smooth_mesh(v.double(), f)
    with pytest.raises(RuntimeError):
        smooth_mesh(v, f.long())
    with pytest.raises(RuntimeError, match="GPU"):
        smooth_mesh(v, f, fixed=torch.zeros(len(v), dtype=torch.bool))
    with pytest.raises(RuntimeError):
        smooth_mesh(v, f, fixed=torch.zeros(len(v), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        smooth_mesh(v, f, edges=mesh_edges(len(v) + 1, f))


def test_smoothed_meshes_feed_the_samplers_and_the_file(tmp_path):
    """extract_mesh(simplify=2, smooth=5, topology=True) -> sample_mesh_clouds -> write_ply; the new arguments at their defaults
    give the bytes of before."""
    from npcd.eval.mesh import extract_mesh, mesh_topology, sample_mesh_clouds, write_ply
    from npcd.hip.smooth import smooth_mesh
    from test_gpu_field_query import _model, _on_gpu
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma = m.density_grid(coords, feats, resolution=24)[0]
    level = float(sigma[sigma > 0].median())          # a surface exists with untrained weights
    coarse = extract_mesh(m, coords, feats, resolution=24, level=level, normals=True, simplify=2)
    again = extract_mesh(m, coords, feats, resolution=24, level=level, normals=True, simplify=2, smooth=None, topology=False)
    smooth = extract_mesh(m, coords, feats, resolution=24, level=level, normals=True, simplify=2, smooth=5, topology=True)
    for before, same, mesh in zip(coarse, again, smooth):
        assert sorted(before) == sorted(same) and all(torch.equal(before[k], same[k]) for k in before)
        assert sorted(mesh) == sorted(list(before) + ["topology"])
        assert all(torch.equal(before[k], mesh[k]) for k in before if k != "vertices")
        assert torch.equal(raw(mesh["vertices"]), raw(smooth_mesh(before["vertices"], before["faces"], 5)))
        assert torch.isfinite(mesh["vertices"]).all() and not torch.equal(mesh["vertices"], before["vertices"])
        t = mesh["topology"]
        assert t == mesh_topology(len(before["vertices"]), before["faces"].cpu().numpy())          # the kernels' counts are the specification's
        assert t["valid_faces"] == before["faces"].shape[0] and t["used_vertices"] <= before["vertices"].shape[0]
    clouds, normals = sample_mesh_clouds(smooth, 256, generator=torch.Generator(device="cuda").manual_seed(3), normals=True)
    assert clouds.shape == normals.shape == (len(smooth), 256, 3) and torch.isfinite(clouds).all() and torch.isfinite(normals).all()
    mesh = smooth[0]
    path = str(tmp_path / "smooth.ply")
    write_ply(path, mesh["vertices"], mesh["faces"], colors=mesh["colors"], normals=mesh["normals"])
    header = open(path, "rb").read(600).split(b"end_header")[0].decode("ascii")
    assert f"element vertex {mesh['vertices'].shape[0]}\n" in header and f"element face {mesh['faces'].shape[0]}\n" in header
