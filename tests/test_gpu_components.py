"""The component labelling kernels (csrc/components.hip, npcd.hip.components) against the CPU restatement of their specification
(npcd.eval.mesh.connected_components_reference, itself held to scipy and to hand cases by tests/test_components_cpu.py): labels and
sizes are equal, and equal again on a second run.

The volumes are those of tests/test_components_cpu.py, where the kernels' own phases have already run on the host: the smallest
volume, non-cubic ones, one node more than the 16 x 8 x 8 brick on each axis in turn, two bricks and a node on every axis; white noise
at three levels (one giant component, near the percolation threshold, many tiny ones), two spheres, a serpentine whose label travels
the whole volume, staircases joined through one diagonal edge type only, the lattice of singletons, NaN and infinities, the level
equal to a sample.  B = 1 and B = 3 with different members, whose labels are local to each volume."""
import numpy as np
import pytest
import torch

from npcd.eval.mesh import filter_components_reference
from test_components_cpu import BIG, KINDS, SHAPES, batch, component_case

pytestmark = pytest.mark.gpu


def _hold(labels, sizes, member, what):
    _, _, want_labels, want_sizes = member
    assert labels.dtype == torch.int32 and sizes.dtype == torch.int32 and labels.is_cuda and sizes.is_cuda, what
    assert tuple(labels.shape) == tuple(sizes.shape) == want_labels.shape, what
    np.testing.assert_array_equal(labels.cpu().numpy(), want_labels, err_msg=what)
    np.testing.assert_array_equal(sizes.cpu().numpy().reshape(-1), want_sizes, err_msg=what)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_reference(shape, B):
    from npcd.hip.components import label_components
    for kind in KINDS:
        members = batch(shape, kind, B)
        level = members[0][1]
        vols = torch.from_numpy(np.stack([m[0] for m in members])).cuda()
        labels, sizes = label_components(vols if B > 1 else vols[0], level)
        again = label_components(vols, level)
        print(f"{shape} B {B} {kind}: " + ", ".join(f"{np.count_nonzero(m[3])} components" for m in members))
        assert torch.equal(labels.reshape(again[0].shape), again[0]) and torch.equal(sizes.reshape(again[1].shape), again[1])
        for b, member in enumerate(members):
            _hold(*((labels[b], sizes[b]) if B > 1 else (labels, sizes)), member, f"{shape} {kind} member {b} of {B}")


def test_a_million_nodes():
    """101 x 103 x 102 noise at 0.5: 7 x 13 x 13 bricks, thousands of components and one that spans them all."""
    from npcd.hip.components import filter_components, label_components
    member = component_case(BIG, "noise_0.5", 0)
    vol, level = torch.tensor(member[0]).cuda(), member[1]
    labels, sizes = label_components(vol, level)
    _hold(labels, sizes, member, "a million nodes")
    again = label_components(vol, level)
    assert torch.equal(labels, again[0]) and torch.equal(sizes, again[1])
    assert np.count_nonzero(member[3]) > 1000
    got = filter_components(vol, level, largest=1)
    want = filter_components_reference(member[0], level, largest=1)
    np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def test_filter_components():
    from npcd.hip.components import filter_components, filter_components_counted
    shape = (17, 17, 33)
    for kind, options in (("noise_0.85", dict(largest=1)), ("noise_0.85", dict(largest=3, min_nodes=2)), ("noise_0.85", dict(min_nodes=4)),
                          ("noise_0.85", dict()), ("nonfinite", dict(largest=2)), ("even_lattice", dict(largest=5)),          # all ties
                          ("stairs_111", dict(largest=4)), ("noise_1.3", dict(largest=2, min_nodes=50)), ("level_is_a_sample", dict(largest=1))):
        members = batch(shape, kind, 3)
        level = members[0][1]
        vols = torch.from_numpy(np.stack([m[0] for m in members])).cuda()
        got, kept_nodes = filter_components_counted(vols, level, **options)
        assert got.dtype == torch.float32 and got.shape == vols.shape and len(kept_nodes) == 3
        for b, (vol, _, labels, sizes) in enumerate(members):
            want = filter_components_reference(vol, level, **options)
            np.testing.assert_array_equal(got[b].cpu().numpy().view(np.int32), want.view(np.int32), err_msg=f"{kind} {options} member {b}")
            from npcd.eval.mesh import select_components
            kept = select_components(labels, **options)
            assert kept_nodes[b].dtype == torch.int64 and kept_nodes[b].tolist() == sorted(sizes[kept].tolist(), reverse=True)
        one = filter_components(vols[1], level, **options)
        assert one.shape == vols[1].shape and torch.equal(one.view(torch.int32), got[1].view(torch.int32))


def test_wrapper_refuses_what_it_cannot_run():
    from npcd.hip.components import filter_components, label_components
    for call in (label_components, filter_components):
        with pytest.raises(RuntimeError):
            call(torch.zeros(4, 4, 4), 0.0)                                        # not on the GPU
        with pytest.raises(RuntimeError):
            call(torch.zeros(4, 4, 4, dtype=torch.float64, device="cuda"), 0.0)
        with pytest.raises(ValueError):
            call(torch.zeros(4, 1, 4, device="cuda"), 0.0)
        with pytest.raises(ValueError):
            call(torch.zeros(4, 4, device="cuda"), 0.0)
    for bad in (dict(largest=0), dict(min_nodes=0), dict(largest=2, min_nodes=-1)):
        with pytest.raises(ValueError):
            filter_components(torch.zeros(4, 4, 4, device="cuda"), 0.0, **bad)


def test_entry_point_checks_its_arguments_before_any_launch():
    import ctypes

    from npcd import hip
    L, P = hip.lib(), hip.ptr
    vol = torch.randn(2, 5, 6, 7, device="cuda")
    ws = torch.full((L.npcd_components_ws_bytes(2, 5, 6, 7),), 0x5a, dtype=torch.uint8, device="cuda")
    labels = torch.full((2, 5, 6, 7), -7, dtype=torch.int32, device="cuda")
    sizes = torch.full((2, 5, 6, 7), -7, dtype=torch.int32, device="cuda")
    stream = hip.stream_ptr()
    for dims in ((2, 1, 6, 7), (2, 5, 1, 7), (2, 5, 6, 1), (0, 5, 6, 7)):
        assert L.npcd_components_label(P(vol), *dims, 0.0, P(ws), P(labels), P(sizes), stream) == -1
    assert L.npcd_components_label(P(vol), 1, 1024, 1024, 2048, 0.0, P(ws), P(labels), P(sizes), stream) == -2
    good = [vol, ws, labels, sizes]
    for missing in range(4):
        a = [None if i == missing else P(t) for i, t in enumerate(good)]
        assert L.npcd_components_label(a[0], 2, 5, 6, 7, 0.0, a[1], a[2], a[3], stream) == -1, missing
    for odd in range(4):
        a = [ctypes.c_void_p(t.data_ptr() + 2) if i == odd else P(t) for i, t in enumerate(good)]
        assert L.npcd_components_label(a[0], 2, 5, 6, 7, 0.0, a[1], a[2], a[3], stream) == -1, odd
    torch.cuda.synchronize()
    assert (labels == -7).all() and (sizes == -7).all() and (ws == 0x5a).all()


def test_the_entry_point_writes_its_outputs_and_nothing_else():
    """A direct C call on another stream; labels, sizes and the workspace lie between guard bands."""
    from npcd import hip
    L = hip.lib()
    B, shape = 3, (9, 9, 17)          # two bricks on every axis, every second one cut by the volume's end
    members = batch(shape, "noise_0.85", B)
    n = int(np.prod(shape))
    vol = torch.from_numpy(np.stack([m[0] for m in members])).cuda()
    guard = 256
    ws = torch.full((L.npcd_components_ws_bytes(B, *shape) + 2 * guard,), 0x5a, dtype=torch.uint8, device="cuda")
    labels = torch.full((guard + B * n + guard,), -7, dtype=torch.int32, device="cuda")
    sizes = torch.full((guard + B * n + guard,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hip.check(L.npcd_components_label(hip.ptr(vol), B, *shape, members[0][1], hip.ptr(ws[guard:]), hip.ptr(labels[guard:]),
                                          hip.ptr(sizes[guard:]), hip.stream_ptr()), "npcd_components_label")
    side.synchronize()
    for t, fill in ((labels, -7), (sizes, -7), (ws, 0x5a)):
        assert (t[:guard] == fill).all() and (t[-guard:] == fill).all()
    np.testing.assert_array_equal(labels[guard:-guard].cpu().numpy(), np.concatenate([m[2].reshape(-1) for m in members]))
    np.testing.assert_array_equal(sizes[guard:-guard].cpu().numpy(), np.concatenate([m[3] for m in members]))
