"""The all-pairs Chamfer kernel (csrc/chamfer.hip) and the shape metrics on it (npcd/eval/shapes.py) against the oracle and the
float64 metric implementation of tests/test_chamfer_cpu.py, both written from the spec of DESIGN.md 5.7.

Bar of an entry with Lx valid points: |got - ref| <= (Lx + 2) u ref, u = 2^-24.  Derived, not measured: the per-point minima are exact
(the oracle evaluates the same fp32 expression); any order of summing Lx non-negative fp32 terms errs by at most (Lx - 1) u
relatively, a division or a reciprocal-multiply adds at most 2 u.  chamfer_matrix adds two such entries: (max(Lx, Ly) + 3) u.  Every
test prints its worst error / bar ratio."""
import functools

import numpy as np
import pytest
import torch

from test_chamfer_cpu import (BAR_64, U, chamfer_float64, chamfer_matrix_oracle, chamfer_oracle, check_metrics, metric_matrices,
                              metric_sets, metrics_float64, normalize_bbox_numpy, smallest_argmin_gap)

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _clouds(n, P, seed):
    return np.random.default_rng(seed).standard_normal((n, P, 3)).astype(np.float32)


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _directed(x, y=None, x_len=None, y_len=None):
    from npcd.hip.chamfer import chamfer_directed
    out = chamfer_directed(_gpu(x), _gpu(y), x_len, y_len)
    assert out.dtype == torch.float32 and out.shape == (len(x), len(x if y is None else y))
    return out.cpu().numpy()


def _ratio(got, ref, terms):
    """Worst |got - ref| / bar over the entries; `terms`: the bar's count per row ([M] or a scalar), bar = terms u ref."""
    bar = np.broadcast_to(np.asarray(terms, dtype=np.float64).reshape(-1, 1), ref.shape) * U * ref
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all()
    return float(np.where(err == 0, 0.0, err / np.maximum(bar, 1e-300)).max())


def _check_directed(x, y, x_len=None, y_len=None, what=""):
    got = _directed(x, y, x_len, y_len)
    ref = chamfer_oracle(x, y, x_len, y_len)
    terms = (x.shape[1] if x_len is None else np.asarray(x_len)) + 2
    worst = _ratio(got, ref, terms)
    print(f"{what} M {len(x)} P {x.shape[1]} N {len(y)} Q {y.shape[1]}: worst error / bar = {worst:.3f}")
    assert worst <= 1.0, what
    return got


# owned-point instantiations of csrc/chamfer.hip: <1, 8> to 256 points, <2, 4> to 512, <4, 2> to 1,024, <8, 1> to 2,048, <16, 1> above
_P_ISSUE = [1, 2, 63, 64, 65, 255, 256, 257, 513]
_P_FORMS = [511, 512, 1023, 1024, 1025, 2047, 2048, 2049]
_Q_ISSUE = [1, 63, 64, 65, 257, 1025]
_Q_TILE = [511, 512, 513, 1023, 1024]          # kChamferTile = 512 rows, one and two tiles, each at +-1 (1025 is above)


@pytest.mark.parametrize("P", _P_ISSUE + _P_FORMS)
def test_edges(P):
    """M = 3, N = 5 at every Q of the issue; the limits between the instantiations meet the tile edges too."""
    x = _clouds(3, P, P)
    for Q in _Q_ISSUE + (_Q_TILE if P in (64, 512, 513, 2049) else []):
        _check_directed(x, _clouds(5, Q, 7000 + Q), what="edges")


@pytest.mark.parametrize("P, M", [(8, 7), (8, 8), (8, 9), (300, 3), (300, 4), (300, 5), (600, 1), (600, 2), (600, 3)])
def test_x_clouds_per_workgroup_edges(P, M):
    """A workgroup owns 8, 4 or 2 X clouds at these P: one group less one, one whole group, one group and one."""
    _check_directed(_clouds(M, P, 100 * P + M), _clouds(3, 70, 5), what="X group")


@pytest.mark.parametrize("M, N, P", [(520, 131, 8), (1024, 67, 4), (16384, 33, 2)])
def test_y_chunk_edges(M, N, P):
    """The launch gives a workgroup up to kCloudPairChunk = 32 Y clouds, halved until the grid has kCloudPairFill = 2,048 workgroups: here
    2, 4 and 32, and N is one more than a multiple so that the last workgroup of a row walks one cloud.  M = 16,384 is the number of
    clouds the launch geometry has to allow at least."""
    _check_directed(_clouds(M, P, M), _clouds(N, P, N), what="Y chunk")


def test_grid_edges():
    _check_directed(_clouds(70, 32, 70), _clouds(130, 32, 130), what="grid")


def test_the_entry_point_writes_all_of_out_and_nothing_else():
    """The C entry point with `out` between guard bands that start as a sentinel, the range itself as NaN."""
    from npcd import hip
    x, y = _clouds(13, 40, 31), _clouds(21, 50, 32)
    dx, dy = _gpu(x), _gpu(y)
    buf = torch.full((13 * 21 + 128,), 1536.0, device="cuda")
    out = buf[64:64 + 13 * 21].view(13, 21)
    out.fill_(float("nan"))
    hip.check(hip.lib().npcd_chamfer_directed(hip.ptr(dx), hip.ptr(None), hip.ptr(dy), hip.ptr(None), hip.ptr(out), 13, 40, 21, 50,
                                              hip.stream_ptr()), "npcd_chamfer_directed")
    assert bool((buf[:64] == 1536.0).all()) and bool((buf[-64:] == 1536.0).all())
    assert _ratio(out.cpu().numpy(), chamfer_oracle(x, y), 40 + 2) <= 1.0


def test_limit():
    from npcd.hip.chamfer import chamfer_directed, max_points
    P = max_points()
    assert P >= 4096
    _check_directed(_clouds(2, P, 1), _clouds(2, P, 2), what="limit")
    with pytest.raises(RuntimeError, match="up to"):
        chamfer_directed(torch.zeros(1, P + 1, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="up to"):
        chamfer_directed(torch.zeros(1, 8, 3, device="cuda"), torch.zeros(1, P + 1, 3, device="cuda"))


def test_one_valid_point_is_the_oracle_minimum_bit_for_bit():
    """x_lengths = 1: one term, division by 1 -- nothing rounds, so the entry IS the fp32 minimum."""
    for P, Q in ((5, 700), (300, 64), (2100, 513)):
        x, y = _clouds(6, P, 40 + P), _clouds(7, Q, 50 + Q)
        ref = chamfer_oracle(x, y, [1] * 6)
        assert (ref == ref.astype(np.float32)).all()
        for lengths in ([1] * 6, torch.ones(6, dtype=torch.int32).cuda()):
            got = _directed(x, y, lengths)
            np.testing.assert_array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))


X_LEN, Y_LEN = [70, 1, 64, 33], [600, 1, 513, 512, 37]


@functools.lru_cache(maxsize=None)
def _ragged():
    """Every padding row of Y is a copy of an X point: read one row too far and that point's minimum is 0.  In Y clouds 2 and 4 every
    valid row but the last is far away, so the last valid row (the first of the second tile; the first of a group of four) is the
    nearest point of every X point."""
    x, y = _clouds(4, 70, 61).copy(), _clouds(5, 600, 62).copy()
    for j in (2, 4):
        y[j, :Y_LEN[j] - 1] += np.float32(50)
    flat = x.reshape(-1, 3)
    for j, n in enumerate(Y_LEN):
        y[j, n:] = flat[(70 + np.arange(600 - n)) % len(flat)]          # the first of them is x[1, 0], all that is valid of X cloud 1
    return x, y


def test_ragged_lengths():
    """Given as host lists and as GPU tensors: the same bits, and the oracle's values."""
    x, y = _ragged()
    ref = chamfer_oracle(x, y, X_LEN, Y_LEN)
    # the trap is armed: X cloud 1 is the one point that the first padding row of every Y cloud copies
    one_too_far = chamfer_oracle(x, y, X_LEN, [min(n + 1, 600) for n in Y_LEN])
    assert (one_too_far[1, 1:] == 0.0).all() and (ref[1, 1:] > 1e-3).all()
    for j in (2, 4):          # the nearest point of every valid X point is the last valid row
        for i in range(4):
            a, b = x[i, :X_LEN[i]], y[j, :Y_LEN[j]]
            assert (((a[:, None] - b[None]) ** 2).sum(-1).argmin(axis=1) == Y_LEN[j] - 1).all()
    flipped = chamfer_oracle(y, x, Y_LEN, X_LEN)          # the other direction: Y owned with its lengths, X streamed with its own
    results = []
    for xl, yl in ((X_LEN, Y_LEN), (torch.tensor(X_LEN).cuda(), torch.tensor(Y_LEN, dtype=torch.int32).cuda())):
        results.append((_directed(x, y, xl, yl), _directed(y, x, yl, xl)))
        worst = _ratio(results[-1][0], ref, np.asarray(X_LEN) + 2), _ratio(results[-1][1], flipped, np.asarray(Y_LEN) + 2)
        print(f"ragged lengths ({'GPU tensors' if torch.is_tensor(xl) else 'host lists'}): worst error / bar = {worst[0]:.3f}, "
              f"transposed {worst[1]:.3f}")
        assert max(worst) <= 1.0
    for a, b in zip(*results):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_device_lengths_are_clamped():
    x, y = _ragged()
    got = _directed(x, y, torch.tensor([0, -3, 75, 70]).cuda(), torch.tensor([0, -3, 605, 600, 1 << 30]).cuda())
    want = _directed(x, y, [1, 1, 70, 70], [1, 1, 600, 600, 600])
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    assert _ratio(want, chamfer_oracle(x, y, [1, 1, 70, 70], [1, 1, 600, 600, 600]), np.asarray([1, 1, 70, 70]) + 2) <= 1.0


def test_self_matrix():
    from npcd.hip.chamfer import chamfer_directed, chamfer_matrix
    x = _gpu(_clouds(37, 100, 71))
    d, cd = chamfer_directed(x), chamfer_matrix(x)
    assert torch.equal(d.diagonal(), torch.zeros(37, device="cuda")) and torch.equal(cd.diagonal(), torch.zeros(37, device="cuda"))
    assert torch.equal(cd, cd.t())
    assert torch.equal(d, chamfer_directed(x, x.clone())) and torch.equal(cd, chamfer_matrix(x, x.clone()))
    worst = _ratio(cd.cpu().numpy(), chamfer_matrix_oracle(_clouds(37, 100, 71)), 100 + 3)
    print(f"self matrix: worst error / bar = {worst:.3f}")
    assert worst <= 1.0
    lengths = [100 - i for i in range(37)]
    cl = chamfer_matrix(x, x_lengths=lengths)
    assert torch.equal(cl, cl.t()) and torch.equal(cl, chamfer_matrix(x, x.clone(), lengths, lengths))
    ref = chamfer_matrix_oracle(_clouds(37, 100, 71), x_len=lengths)
    assert _ratio(cl.cpu().numpy(), ref, 100 + 3) <= 1.0


def test_far_from_the_origin():
    """Clouds at 100 + 1e-3 N(0, 1): the same bar.  The norm-expansion form evaluated in fp32 is off by thousands of times the VALUE
    here; the spec's direct-difference form, the oracle, is within 1e-5 of pure float64."""
    rng = np.random.default_rng(81)
    x = (np.float32(100) + np.float32(1e-3) * rng.standard_normal((4, 200, 3)).astype(np.float32)).astype(np.float32)
    y = (np.float32(100) + np.float32(1e-3) * rng.standard_normal((6, 300, 3)).astype(np.float32)).astype(np.float32)
    ref, exact = chamfer_oracle(x, y), chamfer_float64(x, y)
    assert (np.abs(ref - exact) <= 1e-5 * exact).all()
    sq = lambda a: (a * a).sum(-1, dtype=np.float32)
    expansion = np.stack([(sq(xi)[None, :, None] + sq(y)[:, None, :] - np.float32(2) * np.einsum("pc,nqc->npq", xi, y)).min(2).mean(1) for xi in x])
    print(f"expansion form in fp32: off by {np.abs(expansion - exact).max() / exact.max():.0f} x the value")
    assert np.abs(expansion - exact).max() > 100 * exact.max()
    _check_directed(x, y, what="far from the origin")


def test_repeatability_and_views():
    from npcd.hip.chamfer import chamfer_directed, chamfer_matrix
    x, y = _gpu(_clouds(9, 777, 91)), _gpu(_clouds(11, 300, 92))
    assert torch.equal(chamfer_directed(x, y), chamfer_directed(x, y)) and torch.equal(chamfer_matrix(x, y), chamfer_matrix(x, y))
    packed = _gpu(np.ascontiguousarray(_clouds(9, 777, 91).transpose(0, 2, 1)))          # [n, 3, N], as `generate` returns
    view = packed.permute(0, 2, 1)
    assert not view.is_contiguous() and torch.equal(view, x)
    assert torch.equal(chamfer_directed(view, y), chamfer_directed(x, y)) and torch.equal(chamfer_directed(y, view), chamfer_directed(y, x))
    worst = _ratio(chamfer_matrix(view, y).cpu().numpy(), chamfer_matrix_oracle(_clouds(9, 777, 91), _clouds(11, 300, 92)), 777 + 3)
    print(f"matrix P 777 Q 300: worst error / bar = {worst:.3f}")
    assert worst <= 1.0


# ---- the metrics ----------------------------------------------------------------------------------------------------------------------
def test_metrics_on_random_sets():
    from npcd.eval import shape_metrics
    gen, ref, _ = metric_sets()
    cd, _ = metric_matrices()
    assert smallest_argmin_gap(cd, 20) > 4 * BAR_64          # precondition, asserted
    check_metrics(shape_metrics(_gpu(gen), _gpu(ref)), metrics_float64(cd, 20), BAR_64)


def test_metrics_on_twins():
    from npcd.eval import shape_metrics
    _, ref, twins = metric_sets()
    _, cd = metric_matrices()
    assert smallest_argmin_gap(cd, 24) > 4 * BAR_64
    got = shape_metrics(_gpu(twins), _gpu(ref))
    assert got["nna_correct"] == 0 and got["cov_matched"] == 24 and got["num_generated"] + got["num_reference"] == 48
    check_metrics(got, metrics_float64(cd, 24), BAR_64)


def test_metrics_normalized():
    from npcd.eval import normalize_clouds, shape_metrics
    gen, ref, _ = metric_sets()
    gen, ref = gen * np.float32(2) + np.float32(1), ref * np.float32(0.5) - np.float32(1)
    on_gpu = normalize_clouds(_gpu(gen), "bbox")
    np.testing.assert_allclose(on_gpu.cpu().numpy(), normalize_bbox_numpy(gen), rtol=0, atol=4e-6)
    # the metrics of the normalised clouds, the fp32 clouds the kernel sees
    g, r = on_gpu.cpu().numpy(), normalize_clouds(_gpu(ref), "bbox").cpu().numpy()
    cd = chamfer_matrix_oracle(np.concatenate([g, r]))
    assert smallest_argmin_gap(cd, 20) > 4 * BAR_64
    check_metrics(shape_metrics(_gpu(gen), _gpu(ref), normalize="bbox"), metrics_float64(cd, 20), BAR_64)


def test_metrics_with_lengths_and_unequal_point_counts():
    from npcd.eval import shape_metrics
    gen, ref = _clouds(10, 48, 101) * np.float32(0.8), _clouds(12, 80, 102)
    gl, rl = [48 - 2 * i for i in range(10)], [80 - 3 * i for i in range(12)]
    cd = np.block([[chamfer_matrix_oracle(gen, x_len=gl), chamfer_matrix_oracle(gen, ref, gl, rl)],
                   [chamfer_matrix_oracle(ref, gen, rl, gl), chamfer_matrix_oracle(ref, x_len=rl)]])
    assert (cd == cd.T).all()
    bar = (80 + 3) * U
    assert smallest_argmin_gap(cd, 10) > 4 * bar
    check_metrics(shape_metrics(_gpu(gen), _gpu(ref), gen_lengths=gl, ref_lengths=torch.tensor(rl).cuda()), metrics_float64(cd, 10), bar)
    # unequal point counts without lengths: the four directed blocks again
    cd = np.block([[chamfer_matrix_oracle(gen), chamfer_matrix_oracle(gen, ref)], [chamfer_matrix_oracle(ref, gen), chamfer_matrix_oracle(ref)]])
    assert smallest_argmin_gap(cd, 10) > 4 * bar
    check_metrics(shape_metrics(_gpu(gen), _gpu(ref)), metrics_float64(cd, 10), bar)


def test_evaluate_shapes_end_to_end():
    from npcd.eval import evaluate_shapes
    from test_gpu_sampler_steps import _tiny_model
    m = _tiny_model()
    reference = _gpu(_clouds(8, 48, 111))
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        runs.append(evaluate_shapes(m, reference, num_samples=6, generate_batch_size=4, sampling_steps=4, eta=0.0, return_clouds=True))
    a, b = runs
    assert a["clouds"].shape == (6, 48, 3) and a["clouds"].dtype == torch.float32 and bool(torch.isfinite(a["clouds"]).all())
    assert torch.equal(a["clouds"], b["clouds"])
    timings = ("generate_seconds", "metric_seconds")
    assert all(a[k] > 0 and b[k] > 0 for k in timings)
    assert {k: v for k, v in a.items() if k not in timings + ("clouds",)} == {k: v for k, v in b.items() if k not in timings + ("clouds",)}
    cd = chamfer_matrix_oracle(np.concatenate([a["clouds"].cpu().numpy(), reference.cpu().numpy()]))
    bar = (48 + 3) * U
    assert smallest_argmin_gap(cd, 6) > 4 * bar
    check_metrics(a, metrics_float64(cd, 6), bar)
    assert (a["num_generated"], a["num_reference"]) == (6, 8)
