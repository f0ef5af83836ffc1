"""The isosurface kernels (csrc/isosurface.hip, npcd.hip.isosurface) against the CPU restatement of their specification
(npcd.eval.mesh.marching_tetrahedra_reference, itself held to geometry by tests/test_isosurface_cpu.py): the numbers of vertices and
triangles and the faces are equal, the vertices are the same bits.

Shapes: the smallest volume, non-cubic ones with every axis in turn the long one, sizes that are no multiple of a wave or of the
1,024-node strip of a workgroup, a strip plus one node along x with two rows and two slabs (the strip is one node high and deep: one
node more than the tile on every axis), and one volume of more than 1,024 strips, where the scan over the strips' totals takes a
second round.  B = 1 and B = 3 with different volumes in the batch; a non-trivial origin and unequal spacings throughout."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from npcd.eval.mesh import marching_tetrahedra_reference
from npcd.hip.isosurface import STRIP_NODES as STRIP          # nodes per workgroup
from test_isosurface_cpu import blobs_volume, sphere_volume

pytestmark = pytest.mark.gpu

ORIGIN, SPACING = (-1.0, 0.3, 0.7), (0.11, 0.07, 0.13)
SHAPES = [(2, 2, 2), (3, 2, 2), (2, 3, 5), (5, 6, 7), (9, 8, 33), (33, 9, 8), (17, 17, 17), (2, 2, STRIP + 1)]
KINDS = ("noise", "blobs", "sphere", "level_is_a_sample", "nonfinite")


@functools.lru_cache(maxsize=None)
def case(shape, kind, member):
    """-> (volume, level, reference vertices, reference faces): member `member` of a batch, computed once."""
    rng = np.random.default_rng(1000 * member + sum(shape))
    n = int(np.prod(shape))
    if kind == "blobs":
        vol = blobs_volume(shape, seed=member)[0]
        level = float(np.median(vol))
    elif kind == "sphere":
        vol = sphere_volume(shape, radius=0.6 - 0.1 * member)[0]
        level = 0.0
    else:          # white noise: nearly every edge is crossed
        vol = rng.standard_normal(shape).astype(np.float32)
        level = 0.1
        if kind == "level_is_a_sample":
            level = float(vol.reshape(-1)[n // 2])
        elif kind == "nonfinite":
            vol.reshape(-1)[(n // 3 + member) % n] = np.nan
            vol.reshape(-1)[(2 * n // 3 + member) % n] = np.inf
    v, f = marching_tetrahedra_reference(vol, level, ORIGIN, SPACING)
    for a in (vol, v, f):
        a.setflags(write=False)
    return vol, level, v, f


def _hold(got, want_v, want_f, what):
    v, f = got
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda, what
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.shape == want_v.shape and f.shape == want_f.shape, (what, v.shape, want_v.shape, f.shape, want_f.shape)
    np.testing.assert_array_equal(f, want_f, err_msg=what)
    finite = np.isfinite(want_v)
    np.testing.assert_array_equal(np.isfinite(v), finite, err_msg=what)
    np.testing.assert_array_equal(v.view(np.int32)[finite], want_v.view(np.int32)[finite], err_msg=what)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_reference(shape, B):
    from npcd.hip.isosurface import isosurface
    for kind in KINDS:
        members = [case(shape, kind, m) for m in range(B)]
        level = members[0][1]          # one level per call: the batch's other members are cut at the first one's
        if kind in ("blobs", "level_is_a_sample"):
            members = [members[0]] + [(vol, level, *marching_tetrahedra_reference(vol, level, ORIGIN, SPACING)) for vol, _, _, _ in members[1:]]
        vols = torch.from_numpy(np.stack([m[0] for m in members])).cuda()
        got = isosurface(vols if B > 1 else vols[0], level, ORIGIN, SPACING)
        again = isosurface(vols, level, ORIGIN, SPACING)
        assert len(got) == len(again) == B
        print(f"{shape} B {B} {kind}: " + ", ".join(f"{len(v)} vertices {len(f)} faces" for v, f in got))
        for b, (vol, _, want_v, want_f) in enumerate(members):
            _hold(got[b], want_v, want_f, f"{shape} {kind} member {b} of {B}")
            assert torch.equal(got[b][1], again[b][1])
            assert torch.equal(got[b][0].view(torch.int32), again[b][0].view(torch.int32))          # the same bits on every call


def test_more_than_one_round_of_the_scan_over_the_strips():
    """1,061,106 nodes = 1,037 strips: the scan over the strips' totals carries over from its first 1,024 to the rest."""
    from npcd.hip.isosurface import isosurface
    shape = (101, 103, 102)
    assert -(-int(np.prod(shape)) // STRIP) > STRIP
    vol, level, want_v, want_f = case(shape, "sphere", 0)
    assert len(want_f) > 10000
    (got,) = isosurface(torch.tensor(vol).cuda(), level, ORIGIN, SPACING)
    _hold(got, want_v, want_f, "1,037 strips")


def test_a_volume_without_a_crossing():
    from npcd.hip.isosurface import isosurface
    outside = torch.full((5, 6, 7), -1.0, device="cuda")
    for vol in (outside, outside[None], torch.full((2, 2, 2), 3.0, device="cuda")):
        (v, f), = isosurface(vol, 0.0, ORIGIN, SPACING)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32
    vol, level, want_v, want_f = case((5, 6, 7), "noise", 0)
    for place in range(3):          # as the first, the middle and the last member of a batch
        batch = [torch.tensor(vol).cuda()] * 2
        batch.insert(place, outside + level)
        got = isosurface(torch.stack(batch), level, ORIGIN, SPACING)
        for b in range(3):
            if b == place:
                assert got[b][0].shape == (0, 3) and got[b][1].shape == (0, 3)
            else:
                _hold(got[b], want_v, want_f, f"beside an empty member at {place}")


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.isosurface import isosurface
    with pytest.raises(RuntimeError):
        isosurface(torch.zeros(4, 4, 4), 0.0)                                        # not on the GPU
    with pytest.raises(RuntimeError):
        isosurface(torch.zeros(4, 4, 4, dtype=torch.float64, device="cuda"), 0.0)
    with pytest.raises(ValueError):
        isosurface(torch.zeros(4, 1, 4, device="cuda"), 0.0)
    with pytest.raises(ValueError):
        isosurface(torch.zeros(4, 4, 4, device="cuda"), 0.0, origin=(0.0, 0.0))


def test_entry_points_check_their_arguments_before_any_launch():
    from npcd import hip
    L = hip.lib()
    assert L.npcd_isosurface_ws_bytes(1, 1024, 1024, 293) == -2          # 7 n = 2,150,629,376 >= 2^31
    assert L.npcd_isosurface_ws_bytes(1, 1024, 1024, 292) == 12 * 299008 + 4 * 1024 * 1024 * 292
    assert L.npcd_isosurface_ws_bytes(2, 5, 6, 7) == 2 * (12 + 4 * 210)
    for bad in ((1, 1, 4, 4), (1, 4, 1, 4), (1, 4, 4, 1), (0, 4, 4, 4), (1, 4, 4, -3)):
        assert L.npcd_isosurface_ws_bytes(*bad) == -1
    vol = torch.randn(2, 5, 6, 7, device="cuda")
    ws = torch.zeros(L.npcd_isosurface_ws_bytes(2, 5, 6, 7), dtype=torch.uint8, device="cuda")
    counts = torch.full((2, 2), -7, dtype=torch.int64, device="cuda")
    org, step = (ctypes.c_float * 3)(*ORIGIN), (ctypes.c_float * 3)(*SPACING)
    stream = hip.stream_ptr()
    P = hip.ptr
    for dims in ((1, 6, 7), (5, 1, 7), (5, 6, 1)):
        assert L.npcd_isosurface_count(P(vol), 2, *dims, 0.0, P(ws), P(counts), stream) == -1
    for args in ((None, ws, counts), (vol, None, counts), (vol, ws, None)):
        assert L.npcd_isosurface_count(P(args[0]), 2, 5, 6, 7, 0.0, P(args[1]), P(args[2]), stream) == -1
    assert L.npcd_isosurface_count(P(vol), 2, 5, 6, 7, 0.0, ctypes.c_void_p(ws.data_ptr() + 4), P(counts), stream) == -1
    torch.cuda.synchronize()
    assert (counts == -7).all() and not ws.any()
    hip.check(L.npcd_isosurface_count(P(vol), 2, 5, 6, 7, 0.0, P(ws), P(counts), stream), "npcd_isosurface_count")
    sizes = counts.cpu()
    offsets = (torch.cumsum(counts, 0) - counts).t().contiguous()
    vertices = torch.full((int(sizes[:, 0].sum()), 3), -7.0, device="cuda")
    faces = torch.full((int(sizes[:, 1].sum()), 3), -7, dtype=torch.int32, device="cuda")
    good = [vol, org, step, ws, offsets[0], offsets[1], vertices, faces]
    for missing in range(8):
        a = [None if i == missing else (t if i in (1, 2) else P(t)) for i, t in enumerate(good)]
        assert L.npcd_isosurface_emit(a[0], 2, 5, 6, 7, 0.0, a[1], a[2], a[3], a[4], a[5], a[6], a[7], stream) == -1, missing
    assert L.npcd_isosurface_emit(P(vol), 2, 5, 1, 7, 0.0, org, step, P(ws), P(offsets[0]), P(offsets[1]), P(vertices), P(faces), stream) == -1
    torch.cuda.synchronize()
    assert (vertices == -7).all() and (faces == -7).all()


def test_the_entry_points_write_their_outputs_and_nothing_else():
    """Direct C calls on another stream; counts, vertices and faces lie between guard bands."""
    from npcd import hip
    L = hip.lib()
    B, shape = 3, (5, 6, 7)
    members = [case(shape, "noise", m) for m in range(B)]
    vol = torch.from_numpy(np.stack([m[0] for m in members])).cuda()
    n_vert, n_face = sum(len(m[2]) for m in members), sum(len(m[3]) for m in members)
    guard = 256
    ws = torch.zeros(L.npcd_isosurface_ws_bytes(B, *shape) + 2 * guard, dtype=torch.uint8, device="cuda")
    ws[:guard], ws[-guard:] = 0x5a, 0x5a
    counts = torch.full((guard + 2 * B + guard,), -7, dtype=torch.int64, device="cuda")
    vertices = torch.full((guard + 3 * n_vert + guard,), -7.0, device="cuda")
    faces = torch.full((guard + 3 * n_face + guard,), -7, dtype=torch.int32, device="cuda")
    org, step = (ctypes.c_float * 3)(*ORIGIN), (ctypes.c_float * 3)(*SPACING)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip.check(L.npcd_isosurface_count(hip.ptr(vol), B, *shape, 0.1, hip.ptr(ws[guard:]), hip.ptr(counts[guard:]), hip.stream_ptr()),
                  "npcd_isosurface_count")
        mine = counts[guard:guard + 2 * B].view(B, 2)
        offsets = (torch.cumsum(mine, 0) - mine).t().contiguous()
        hip.check(L.npcd_isosurface_emit(hip.ptr(vol), B, *shape, 0.1, org, step, hip.ptr(ws[guard:]), hip.ptr(offsets[0]), hip.ptr(offsets[1]),
                                         hip.ptr(vertices[guard:]), hip.ptr(faces[guard:]), hip.stream_ptr()), "npcd_isosurface_emit")
    side.synchronize()
    assert mine.cpu().tolist() == [[len(m[2]), len(m[3])] for m in members]
    for t, fill in ((counts, -7), (vertices, -7.0), (faces, -7), (ws, 0x5a)):
        assert (t[:guard] == fill).all() and (t[-guard:] == fill).all()
    np.testing.assert_array_equal(vertices[guard:-guard].view(-1, 3).cpu().numpy().view(np.int32),
                                  np.concatenate([m[2] for m in members]).view(np.int32))
    np.testing.assert_array_equal(faces[guard:-guard].view(-1, 3).cpu().numpy(), np.concatenate([m[3] for m in members]))
