"""The approximate earth mover's distance kernel (csrc/emd.hip) and the -EMD shape metrics on it (npcd/eval/shapes.py) against the
float64 oracle of tests/test_emd_cpu.py, written from the spec of DESIGN.md 5.8.

Bar of a test: 4 x the largest relative difference between the fp32 oracle (sequential sums) and the float64 oracle on that test's
own inputs (test_emd_cpu.Case); it is derived from the two oracles and never from the kernel's output.  Every test prints its worst
error / bar ratio."""
import numpy as np
import pytest
import torch

from test_chamfer_cpu import metric_sets, smallest_argmin_gap
from test_emd_cpu import (DIRECTED_SHAPES, X_LEN, Y_LEN, check_metrics_emd, clamped_case, directed_case, far_case, metric_cases,
                          metrics_emd_float64, ragged_case, self_case, shifted_case, stream_case, strided_case)

pytestmark = pytest.mark.gpu


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _directed(x, y=None, x_len=None, y_len=None):
    from npcd.hip.emd import emd_directed
    out = emd_directed(_gpu(x), _gpu(y), x_len, y_len)
    assert out.dtype == torch.float32 and out.shape == (len(x), len(x if y is None else y))
    return out.cpu().numpy()


def _hold(got, case, what):
    """got against the case's float64 values, within the case's bar."""
    assert np.isfinite(got).all(), what
    err, on_diagonal = case.errors(got)
    ratio = err / case.bar if case.bar > 0 else (0.0 if err == 0 else float("inf"))
    print(f"{what}: error {err:.3g}, bar {case.bar:.3g}, error / bar = {ratio:.3f}")
    assert err <= case.bar, (what, err, case.bar)
    if on_diagonal is not None:          # a cloud against itself: an absolute bar (test_emd_cpu.Case)
        print(f"{what}: diagonal, error {on_diagonal:.3g}, bar {case.diagonal_bar:.3g}, error / bar = {on_diagonal / case.diagonal_bar:.3f}")
        assert on_diagonal <= case.diagonal_bar, (what, on_diagonal, case.diagonal_bar)


@pytest.mark.parametrize("P, Q, M, N", DIRECTED_SHAPES)
def test_directed(P, Q, M, N):
    case = directed_case(P, Q, M, N)
    _hold(_directed(case.x, case.y), case, f"directed P {P} Q {Q} M {M} N {N}")


def test_lengths_on_the_host_and_on_the_gpu():
    """Rows past the lengths are NaN; host lists and GPU tensors give the same bits and the oracle's values on the truncated clouds."""
    case = ragged_case()
    assert np.isnan(case.x[1, 1:]).all() and np.isnan(case.y[4, 37:]).all()
    on_host = _directed(case.x, case.y, X_LEN, Y_LEN)
    on_gpu = _directed(case.x, case.y, torch.tensor(X_LEN).cuda(), torch.tensor(Y_LEN, dtype=torch.int32).cuda())
    _hold(on_host, case, "ragged lengths")
    np.testing.assert_array_equal(on_host.view(np.uint32), on_gpu.view(np.uint32))


def test_device_lengths_are_clamped():
    """0 and -3 behave as 1, P + 7 and 2^30 as P."""
    case = clamped_case()
    got = _directed(case.x, case.y, torch.tensor([0, -3, 77, 70]).cuda(), torch.tensor([0, -3, 307, 300, 1 << 30]).cuda())
    want = _directed(case.x, case.y, case.x_len, case.y_len)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    _hold(got, case, "clamped lengths")


def test_self_matrix_symmetry_and_repeatability():
    from npcd.hip.emd import emd_directed, emd_matrix
    case = self_case()
    x = _gpu(case.x)
    d, m = emd_directed(x), emd_matrix(x)
    assert torch.equal(m, m.t())
    assert torch.equal(d, emd_directed(x)) and torch.equal(m, emd_matrix(x))                      # the same bits on every call
    assert torch.equal(d, emd_directed(x, x.clone())) and torch.equal(m, emd_matrix(x, x.clone()))          # one pointer or two
    _hold(m.cpu().numpy(), case, "self matrix")


def test_a_permuted_view_is_accepted():
    from npcd.hip.emd import emd_directed
    case = strided_case()
    packed = _gpu(np.ascontiguousarray(case.x.transpose(0, 2, 1)))          # [n, 3, P], as `generate` returns
    view = packed.permute(0, 2, 1)
    assert not view.is_contiguous()
    got = emd_directed(view, _gpu(case.y))
    assert torch.equal(got, emd_directed(_gpu(case.x), _gpu(case.y)))
    _hold(got.cpu().numpy(), case, "strided input")


def test_known_answer():
    case = shifted_case()
    got = _directed(case.x, case.y)
    _hold(got, case, "shifted copy")
    assert abs(float(got[0, 0]) - 0.01) <= (1e-5 + case.bar) * 0.01


def test_far_from_the_origin():
    """Clouds at 100 + 1e-3 N(0, 1): direct differences keep every digit that the inputs have."""
    case = far_case()
    _hold(_directed(case.x, case.y), case, "far from the origin")


def test_direct_c_call_on_another_stream():
    from npcd import hip
    case = stream_case()
    dx, dy = _gpu(case.x), _gpu(case.y)
    M, P, N, Q = 5, 40, 6, 50
    buf = torch.full((M * N + 128,), 1536.0, device="cuda")
    out = buf[64:64 + M * N].view(M, N)
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        hip.check(hip.lib().npcd_emd_directed(hip.ptr(dx), hip.ptr(None), hip.ptr(dy), hip.ptr(None), hip.ptr(out), M, P, N, Q,
                                              hip.stream_ptr()), "npcd_emd_directed")
    stream.synchronize()
    assert bool((buf[:64] == 1536.0).all()) and bool((buf[-64:] == 1536.0).all())
    _hold(out.cpu().numpy(), case, "direct C call")


# ---- the metrics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random", "twins"])
def test_metrics(which):
    from npcd.eval import shape_metrics
    gen, ref, twins = metric_sets()
    case = metric_cases()[which == "twins"]
    gen = twins if which == "twins" else gen
    M = len(gen)
    assert smallest_argmin_gap(case.ref, M) > 4 * case.bar          # precondition, asserted
    both = shape_metrics(_gpu(gen), _gpu(ref), emd=True)
    check_metrics_emd(both, metrics_emd_float64(case.ref, M), case.bar)
    plain = shape_metrics(_gpu(gen), _gpu(ref))
    assert set(both) - set(plain) == {"mmd_emd", "cov_emd", "nna_emd", "cov_matched_emd", "nna_correct_emd"}
    assert {k: both[k] for k in plain} == plain          # the CD keys, bit for bit


def test_metrics_through_the_four_blocks():
    """Lengths given (all full): the four directed blocks instead of one launch, the same matrix up to the bar."""
    from npcd.eval import shape_metrics
    gen, ref, _ = metric_sets()
    case = metric_cases()[0]
    got = shape_metrics(_gpu(gen), _gpu(ref), gen_lengths=[64] * 20, ref_lengths=[64] * 24, emd=True)
    check_metrics_emd(got, metrics_emd_float64(case.ref, 20), case.bar)


def test_evaluate_shapes_with_emd():
    from npcd.eval import evaluate_shapes
    from test_gpu_sampler_steps import _tiny_model
    m = _tiny_model()
    reference = _gpu(np.random.default_rng(111).standard_normal((8, 48, 3)).astype(np.float32))
    torch.manual_seed(7)
    a = evaluate_shapes(m, reference, num_samples=6, generate_batch_size=4, sampling_steps=4, eta=0.0, emd=True)
    torch.manual_seed(7)
    b = evaluate_shapes(m, reference, num_samples=6, generate_batch_size=4, sampling_steps=4, eta=0.0)
    assert a["emd_seconds"] > 0 and "emd_seconds" not in b and not [k for k in b if k.endswith("_emd")]
    timings = ("generate_seconds", "metric_seconds", "emd_seconds")
    assert {k: v for k, v in a.items() if k not in timings and not k.endswith("_emd")} == {k: v for k, v in b.items() if k not in timings}
    assert a["mmd_emd"] > 0 and 0 < a["cov_emd"] <= 1 and 0 <= a["nna_emd"] <= 1
