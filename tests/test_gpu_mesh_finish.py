"""What finishes a mesh on the GPU: the vertex normals of npcd.hip.isosurface against
npcd.eval.mesh.vertex_normals_reference bit for bit -- the shapes and kinds of tests/test_gpu_isosurface.py, the zero rows of the
non-finite volumes included --, filter_components -> isosurface against the reference pipeline, and extract_mesh with its new options
on the small synthetic PointNeRF of tests/test_gpu_field_query.py."""
import ctypes

import numpy as np
import pytest
import torch

from npcd.eval.mesh import (connected_components_reference, filter_components_reference, marching_tetrahedra_reference, select_components,
                            vertex_normals_reference)
from test_gpu_isosurface import KINDS, ORIGIN, SHAPES, SPACING, _hold, case

pytestmark = pytest.mark.gpu


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_normals_against_the_reference(shape, B):
    from npcd.hip.isosurface import isosurface
    for kind in KINDS:
        vols = [case(shape, kind, m)[0] for m in range(B)]
        level = case(shape, kind, 0)[1]          # one level per call
        on_gpu = torch.from_numpy(np.stack(vols)).cuda()
        got = isosurface(on_gpu if B > 1 else on_gpu[0], level, ORIGIN, SPACING, normals=True)
        plain = isosurface(on_gpu, level, ORIGIN, SPACING)
        assert len(got) == B and all(len(g) == 3 for g in got) and all(len(p) == 2 for p in plain)
        for b, vol in enumerate(vols):
            v, f, n = got[b]
            assert torch.equal(v.view(torch.int32), plain[b][0].view(torch.int32)) and torch.equal(f, plain[b][1])
            want = vertex_normals_reference(vol, level, SPACING)
            assert n.dtype == torch.float32 and n.is_cuda and tuple(n.shape) == want.shape == tuple(v.shape), (shape, kind, b)
            np.testing.assert_array_equal(_bits(n), _bits(want), err_msg=f"{shape} {kind} member {b} of {B}")
            if kind == "nonfinite":
                assert (_bits(want) == 0).all(axis=1).any()          # the zero rows are there to be matched


def test_normals_of_another_field():
    from npcd.hip.isosurface import isosurface
    for shape in ((5, 6, 7), (9, 8, 33)):
        vols = [case(shape, "blobs", m)[0] for m in range(3)]
        fields = [case(shape, "noise", m)[0] for m in range(3)]
        level = case(shape, "blobs", 0)[1]
        got = isosurface(torch.from_numpy(np.stack(vols)).cuda(), level, ORIGIN, SPACING, normals=True,
                         gradient_of=torch.from_numpy(np.stack(fields)).cuda())
        for b in range(3):
            want = vertex_normals_reference(vols[b], level, SPACING, gradient_of=fields[b])
            assert not np.array_equal(want, vertex_normals_reference(vols[b], level, SPACING))
            np.testing.assert_array_equal(_bits(got[b][2]), _bits(want))
            _hold(got[b][:2], *marching_tetrahedra_reference(vols[b], level, ORIGIN, SPACING), f"{shape} member {b}")
    vol = torch.tensor(vols[0]).cuda()
    with pytest.raises(ValueError):
        isosurface(vol, level, gradient_of=vol)                              # without normals=True
    with pytest.raises(ValueError):
        isosurface(vol, level, normals=True, gradient_of=vol[1:])
    with pytest.raises(RuntimeError):
        isosurface(vol, level, normals=True, gradient_of=vol.cpu())
    with pytest.raises(RuntimeError):
        isosurface(vol, level, normals=True, gradient_of=vol.double())
    (v, f, n), = isosurface(torch.full((3, 4, 5), -1.0, device="cuda"), 0.0, normals=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3) and n.dtype == torch.float32


def test_normals_entry_point():
    """Its refusals before any launch, then a direct call on another stream with the normals between guard bands."""
    from npcd import hip
    L, P = hip.lib(), hip.ptr
    B, shape = 3, (5, 6, 7)
    members = [case(shape, "noise", m) for m in range(B)]
    vol = torch.from_numpy(np.stack([m[0] for m in members])).cuda()
    n_vert = sum(len(m[2]) for m in members)
    guard = 256
    ws = torch.zeros(L.npcd_isosurface_ws_bytes(B, *shape), dtype=torch.uint8, device="cuda")
    counts = torch.empty((B, 2), dtype=torch.int64, device="cuda")
    normals = torch.full((guard + 3 * n_vert + guard,), -7.0, device="cuda")
    step = (ctypes.c_float * 3)(*SPACING)
    hip.check(L.npcd_isosurface_count(P(vol), B, *shape, 0.1, P(ws), P(counts), hip.stream_ptr()), "npcd_isosurface_count")
    offsets = (torch.cumsum(counts, 0) - counts).t().contiguous()
    good = [vol, vol, step, ws, offsets[0], normals[guard:]]
    for missing in range(6):
        a = [None if i == missing else (t if i == 2 else P(t)) for i, t in enumerate(good)]
        assert L.npcd_isosurface_normals(a[0], a[1], B, *shape, 0.1, a[2], a[3], a[4], a[5], hip.stream_ptr()) == -1, missing
    for dims in ((1, 6, 7), (5, 1, 7), (5, 6, 1)):
        assert L.npcd_isosurface_normals(P(vol), P(vol), B, *dims, 0.1, step, P(ws), P(offsets[0]), P(normals[guard:]), hip.stream_ptr()) == -1
    assert L.npcd_isosurface_normals(P(vol), P(vol), B, *shape, 0.1, step, ctypes.c_void_p(ws.data_ptr() + 4), P(offsets[0]),
                                     P(normals[guard:]), hip.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert (normals == -7).all()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip.check(L.npcd_isosurface_normals(P(vol), P(vol), B, *shape, 0.1, step, P(ws), P(offsets[0]), P(normals[guard:]), hip.stream_ptr()),
                  "npcd_isosurface_normals")
    side.synchronize()
    assert (normals[:guard] == -7).all() and (normals[-guard:] == -7).all()
    want = np.concatenate([vertex_normals_reference(m[0], 0.1, SPACING) for m in members])
    np.testing.assert_array_equal(_bits(normals[guard:-guard].view(-1, 3)), _bits(want))


def test_filter_then_isosurface():
    from npcd.hip.components import filter_components
    from npcd.hip.isosurface import isosurface
    rng = np.random.default_rng(7)
    for shape in ((9, 8, 33), (17, 17, 33)):
        vols = [(case(shape, "blobs", m)[0] + 0.3 * rng.standard_normal(shape)).astype(np.float32) for m in range(3)]
        level = float(np.quantile(case(shape, "blobs", 0)[0], 0.85))          # an object and, from the noise, dozens of floaters around it
        on_gpu = torch.from_numpy(np.stack(vols)).cuda()
        for options in (dict(largest=1), dict(largest=2, min_nodes=3)):
            cleaned = filter_components(on_gpu, level, **options)
            got = isosurface(cleaned, level, ORIGIN, SPACING, normals=True, gradient_of=on_gpu)
            for b, vol in enumerate(vols):
                want = filter_components_reference(vol, level, **options)
                np.testing.assert_array_equal(_bits(cleaned[b]), _bits(want))
                want_v, want_f = marching_tetrahedra_reference(want, level, ORIGIN, SPACING)
                assert len(want_v) < len(marching_tetrahedra_reference(vol, level, ORIGIN, SPACING)[0])          # floaters went
                _hold(got[b][:2], want_v, want_f, f"{shape} {options} member {b}")
                np.testing.assert_array_equal(_bits(got[b][2]), _bits(vertex_normals_reference(want, level, SPACING, gradient_of=vol)))


def test_extract_mesh_options():
    from npcd.eval.mesh import extract_mesh
    from npcd.hip.isosurface import isosurface
    from test_gpu_field_query import _model, _on_gpu
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma, origin, spacing = m.density_grid(coords, feats, resolution=24)
    level = float(sigma[sigma > 0].median())          # a surface exists with untrained weights
    direct = isosurface(sigma, level, origin, spacing)
    default = extract_mesh(m, coords, feats, resolution=24, level=level, colors=False, components=None, normals=False)
    finished = extract_mesh(m, coords, feats, resolution=24, level=level, components=1, normals=True)
    host = sigma.cpu().numpy()
    org, step = [float(c) for c in origin], [float(c) for c in spacing]
    for b in range(2):
        assert set(default[b]) == {"vertices", "faces"}
        assert torch.equal(default[b]["vertices"].view(torch.int32), direct[b][0].view(torch.int32)) and torch.equal(default[b]["faces"], direct[b][1])
        mesh = finished[b]
        assert set(mesh) == {"vertices", "faces", "normals", "colors", "component_nodes"}
        labels = connected_components_reference(host[b], level)
        kept = select_components(labels, largest=1)
        cleaned = filter_components_reference(host[b], level, largest=1)
        want_v, want_f = marching_tetrahedra_reference(cleaned, level, org, step)
        print(f"cloud {b}: {len(np.unique(labels)) - 1} components, {len(want_v)} of {len(direct[b][0])} vertices kept")
        _hold((mesh["vertices"], mesh["faces"]), want_v, want_f, f"cloud {b}")
        np.testing.assert_array_equal(_bits(mesh["normals"]), _bits(vertex_normals_reference(cleaned, level, step, gradient_of=host[b])))
        assert mesh["component_nodes"].tolist() == [int((labels == kept[0]).sum())]
        assert mesh["colors"].shape == mesh["vertices"].shape
    sized = extract_mesh(m, coords, feats, resolution=24, level=level, colors=False, min_component_nodes=3)
    for b in range(2):
        labels = connected_components_reference(host[b], level)
        nodes = np.bincount(labels[labels >= 0])
        assert sized[b]["component_nodes"].tolist() == sorted(nodes[nodes >= 3].tolist(), reverse=True) and "normals" not in sized[b]
