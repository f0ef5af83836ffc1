"""Farthest point sampling on the GPU (csrc/fps.hip) against a numpy fp32 oracle written from the spec of DESIGN.md 5.6: the indices
are integers and must be EQUAL, the selected rows bit copies of the input rows.  The oracle evaluates the squared distance as
((dx dx + dy dy) + dz dz) in fp32 (numpy never contracts) and breaks ties by np.argmax's first index."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def fps_oracle(points, length=None, K=50, start=0):
    pts = np.asarray(points, dtype=np.float32)
    L = pts.shape[0] if length is None else int(length)
    n = min(int(K), L)
    out = np.full(n, -1, dtype=np.int64)
    if n == 0:
        return out
    v = pts[:L]
    md = np.full(L, np.inf, dtype=np.float32)
    cur = int(start)
    for k in range(n):
        out[k] = cur
        diff = v - v[cur]
        d = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
        md = np.minimum(md, d)
        cur = int(np.argmax(md))
    return out


def _run(points, **kw):
    from npcd.hip.fps import sample_farthest_points
    sel, idx = sample_farthest_points(torch.from_numpy(points).cuda(), **kw)
    return sel.cpu().numpy(), idx.cpu().numpy()


def _check(points, sel, idx, lengths=None, ks=None, starts=None):
    """Every cloud of a batch against the oracle; the slots after a cloud's picks hold -1 / 0.0; rows are bit copies."""
    N, Kmax = idx.shape
    assert idx.dtype == np.int64 and sel.dtype == np.float32 and sel.shape == (N, Kmax, 3)
    for i in range(N):
        L = points.shape[1] if lengths is None else lengths[i]
        K = Kmax if ks is None else ks[i]
        want = fps_oracle(points[i], L, K, 0 if starts is None else starts[i])
        n = len(want)
        np.testing.assert_array_equal(idx[i, :n], want, err_msg=f"cloud {i}")
        np.testing.assert_array_equal(idx[i, n:], -1, err_msg=f"cloud {i}")
        assert (idx[i, :n] < max(L, 1)).all()
        np.testing.assert_array_equal(sel[i, :n].view(np.uint32), points[i][want].view(np.uint32), err_msg=f"cloud {i}")
        np.testing.assert_array_equal(sel[i, n:].view(np.uint32), 0, err_msg=f"cloud {i}")


@functools.lru_cache(maxsize=None)
def _cloud(N, P, seed):
    return np.random.default_rng(seed).standard_normal((N, P, 3)).astype(np.float32)


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 1023, 1024, 1025])
def test_wave_and_workgroup_edges(P):
    points = _cloud(2, P, P)
    sel, idx = _run(points, K=min(P, 64))
    _check(points, sel, idx)


def _form_edges():
    from npcd.hip.fps import resident_points
    R = resident_points()
    # the resident form's limit, and the limit between the two streaming instantiations (kFpsStreamMid * 1024 of csrc/fps.hip)
    return [R - 1, R, R + 1, 32 * 1024, 32 * 1024 + 1]


@pytest.mark.parametrize("edge", range(5))
def test_form_edges(edge):
    P = _form_edges()[edge]
    points = _cloud(1, P, 1000 + edge)
    sel, idx = _run(points, K=128)
    _check(points, sel, idx)


def test_one_cloud_of_100000_points():
    from npcd.hip.fps import max_points
    assert max_points() >= 100000
    points = _cloud(1, 100000, 7)
    sel, idx = _run(points, K=512)
    _check(points, sel, idx)
    assert len(set(idx[0].tolist())) == 512


def test_ties_on_a_lattice():
    """2,000 points on the 9^3 sites of {-1, -0.75, ..., 1}^3 (exact in fp32): every distance is shared by many points, and at
    least 1,271 points sit on a site that an earlier point has too -- every pick is decided by the tie rule."""
    g = np.random.default_rng(11)
    points = (g.integers(0, 9, size=(1, 2000, 3)).astype(np.float32) * np.float32(0.25) - np.float32(1)).astype(np.float32)
    sel, idx = _run(points, K=512)
    _check(points, sel, idx)


def test_ties_after_the_distinct_sites_run_out():
    g = np.random.default_rng(12)
    points = (g.integers(0, 3, size=(1, 200, 3)).astype(np.float32) - np.float32(1)).astype(np.float32)
    sites = len({tuple(p) for p in points[0].tolist()})
    assert sites <= 27
    sel, idx = _run(points, K=64)
    _check(points, sel, idx)
    np.testing.assert_array_equal(idx[0, sites:], 0)           # every min_dist is 0: the lowest index wins, again and again
    assert len(set(idx[0, :sites].tolist())) == sites


def test_coincident_points():
    points = np.full((1, 70, 3), 0.3, dtype=np.float32)
    sel, idx = _run(points, K=5)
    np.testing.assert_array_equal(idx, [[0, 0, 0, 0, 0]])
    np.testing.assert_array_equal(sel, np.full((1, 5, 3), 0.3, dtype=np.float32))


LENGTHS, KS = [300, 0, 1, 17, 299], [64, 64, 64, 64, 10]


def _padded_batch():
    points = _cloud(5, 300, 21).copy()
    for i, n in enumerate(LENGTHS):
        points[i, n:] = 1e18          # large and finite (its square is too): a pick that ignored the length would land here
    return points


@pytest.mark.parametrize("on_device", [False, True])
def test_padding_lengths_and_per_cloud_k(on_device):
    points = _padded_batch()
    lengths = torch.tensor(LENGTHS, dtype=torch.int64).cuda() if on_device else LENGTHS
    sel, idx = _run(points, lengths=lengths, K=KS)
    assert idx.shape == (5, 64)
    _check(points, sel, idx, LENGTHS, KS)
    assert [int((idx[i] >= 0).sum()) for i in range(5)] == [64, 0, 1, 17, 10]
    assert float(np.abs(sel).max()) < 1e3


def test_start_idx_given():
    points = _padded_batch()
    starts = [299, 0, 0, 16, 150]
    for given in (starts, torch.tensor(starts, dtype=torch.int32).cuda()):
        sel, idx = _run(points, lengths=LENGTHS, K=KS, start_idx=given)
        _check(points, sel, idx, LENGTHS, KS, starts)
    assert idx[0, 0] == 299 and idx[3, 0] == 16 and idx[4, 0] == 150 and idx[1, 0] == -1


def test_random_start_point_under_a_fixed_seed():
    from npcd.hip.fps import draw_start_indices
    points = _padded_batch()
    torch.manual_seed(1234)
    starts = draw_start_indices(LENGTHS)
    assert all(0 <= s < max(n, 1) for s, n in zip(starts, LENGTHS)) and len(set(starts)) > 2
    torch.manual_seed(1234)
    sel, idx = _run(points, lengths=LENGTHS, K=KS, random_start_point=True)
    _check(points, sel, idx, LENGTHS, KS, starts)
    torch.manual_seed(1234)
    sel2, idx2 = _run(points, lengths=torch.tensor(LENGTHS).cuda(), K=KS, random_start_point=True)          # lengths read back once
    np.testing.assert_array_equal(idx2, idx)


def test_a_second_call_returns_the_same_bits():
    points = _cloud(3, 20000, 31)
    a = _run(points, K=256)
    b = _run(points, K=256)
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    _check(points[:1], a[0][:1], a[1][:1])


def test_non_contiguous_view():
    from npcd.hip.fps import sample_farthest_points
    buf = torch.from_numpy(np.random.default_rng(41).standard_normal((2, 777, 4)).astype(np.float32)).cuda()
    view = buf[:, :, :3]
    assert not view.is_contiguous()
    sel_v, idx_v = sample_farthest_points(view, K=100)
    sel_c, idx_c = sample_farthest_points(view.contiguous(), K=100)
    assert torch.equal(idx_v, idx_c) and torch.equal(sel_v, sel_c)
    _check(view.contiguous().cpu().numpy(), sel_v.cpu().numpy(), idx_v.cpu().numpy())


def test_every_pick_is_a_farthest_point_in_float64():
    """Without the oracle's arithmetic: in float64, each pick's distance to the nearest earlier pick is at least (1 - 1e-6) times the
    largest such distance over all points (fp32 rounding of a squared distance is 2e-7 relative)."""
    points = _cloud(2, 1025, 1025)
    sel, idx = _run(points, K=64)
    for i in range(2):
        p = points[i].astype(np.float64)
        md = np.full(1025, np.inf)
        for k in range(1, 64):
            md = np.minimum(md, ((p - p[idx[i, k - 1]]) ** 2).sum(1))
            assert md[idx[i, k]] >= (1 - 1e-6) * md.max(), (i, k)


def test_subsample_clouds_feeds_stage_one():
    from npcd.data.pointclouds import subsample_clouds
    from npcd.models.pointnerf import PointNeRF
    sizes = [5000, 12345, 20000]
    g = np.random.default_rng(51)
    clouds = [g.standard_normal((n, 3)).astype(np.float32) * np.float32(0.3) for n in sizes]
    normals = [g.standard_normal((n, 3)).astype(np.float32) for n in sizes]
    coords, picked, idx = subsample_clouds(clouds, 512, normals)
    assert coords.shape == (3, 512, 3) and picked.shape == (3, 512, 3) and idx.shape == (3, 512)
    for i in range(3):
        want = fps_oracle(clouds[i], K=512)
        np.testing.assert_array_equal(idx[i].numpy(), want)
        np.testing.assert_array_equal(coords[i].numpy(), clouds[i][want])
        np.testing.assert_array_equal(picked[i].numpy(), normals[i][want])
    net = PointNeRF(3, 32, 512, False).cuda()
    net.set_all_coords(coords.cuda())
    assert torch.equal(net.get_all_coords().detach().cpu(), coords)
