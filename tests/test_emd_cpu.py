"""The approximate earth mover's distance kernel and the -EMD shape metrics, everything that needs no GPU: the two oracles written from
the spec of DESIGN.md 5.8 (float64, and fp32 with sequential sums), the preconditions of the metric sets, the bars that
tests/test_gpu_emd.py holds the kernel to, metrics_from_distance, the wrapper's refusals, the host-side query and refusals of the C
entry point, the kernels' resources as the compiler reports them.

The bar.  For every input of the GPU tests, bar = 4 x max |emd_oracle_fp32 - emd_oracle| / emd_oracle over that input's entries:
the error that the spec evaluated in fp32 with sequential sums makes against float64, with a margin for a different but equally long
summation order and an exp of 1-2 ulp.  It comes from the two oracles alone, never from the kernel's output."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_chamfer_cpu import metric_sets, metrics_float64, smallest_argmin_gap
from test_kernel_resources import _compile

LEVELS = [-(4.0 ** e) for e in range(7, -2, -1)] + [0.0]          # -4^7 ... -4^0, -4^-1, 0
assert len(LEVELS) == 10 and LEVELS[0] == -16384.0 and LEVELS[-2] == -0.25


# ---- oracles, from the spec of DESIGN.md 5.8 ----------------------------------------------------------------------------------------
def _emd_pair(x, y, dt, total):
    """One pair of clouds x [Lx, 3], y [Ly, 3] (valid rows only) in the number format dt; total(a, axis) sums.  -> (cost / T,
    leftover remainL, leftover remainR, T)."""
    x, y = x.astype(dt), y.astype(dt)
    Lx, Ly = len(x), len(y)
    T = max(Lx, Ly)
    dx, dy, dz = (x[:, None, c] - y[None, :, c] for c in range(3))
    d = (dx * dx + dy * dy) + dz * dz
    root = np.sqrt(d)
    assert d.dtype == dt and root.dtype == dt
    remain_l = np.full(Lx, dt(T) / dt(Lx), dtype=dt)
    remain_r = np.full(Ly, dt(T) / dt(Ly), dtype=dt)
    cost, tiny = dt(0), dt(1e-9)
    for level in LEVELS:
        e = np.exp(dt(level) * d)
        ratio_l = remain_l / (tiny + total(e * remain_r[None, :], 1))                       # pass A
        sumr = remain_r * total(e * ratio_l[:, None], 0)                                    # pass B, remainR from before its update
        ratio_r = np.minimum(remain_r / (sumr + tiny), dt(1)) * remain_r
        remain_r = np.maximum(dt(0), remain_r - sumr)
        w = e * ratio_l[:, None] * ratio_r[None, :]                                         # pass C, the new ratioR
        cost = cost + total(total(w * root, 1), 0)
        remain_l = np.maximum(dt(0), remain_l - total(w, 1))
        assert e.dtype == dt and w.dtype == dt and remain_l.dtype == dt and remain_r.dtype == dt
    return cost / dt(T), remain_l, remain_r, T


def _sum64(a, axis):
    return a.sum(axis=axis)


def _sum32(a, axis):
    """fp32, one accumulator, index order."""
    return np.cumsum(a, axis=axis, dtype=np.float32).take(-1, axis=axis)


def _matrix(x, y, x_len, y_len, dt, total):
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    out = np.empty((len(x), len(y)), dtype=np.float64)
    for i in range(len(x)):
        for j in range(len(y)):
            a = x[i, :x.shape[1] if x_len is None else int(x_len[i])]
            b = y[j, :y.shape[1] if y_len is None else int(y_len[j])]
            out[i, j] = _emd_pair(a, b, dt, total)[0]
    return out


def emd_oracle(x, y, x_len=None, y_len=None):
    """Directed matrix [M, N], every operation of the spec in float64 on the fp32 inputs."""
    return _matrix(x, y, x_len, y_len, np.float64, _sum64)


def emd_oracle_fp32(x, y, x_len=None, y_len=None):
    """The same in numpy fp32 (numpy never contracts), every sum one accumulator in index order."""
    return _matrix(x, y, x_len, y_len, np.float32, _sum32)


def emd_matrix_oracle(x, y=None, x_len=None, y_len=None, oracle=emd_oracle):
    """The symmetric form of the metrics: 0.5 (directed(x, y) + directed(y, x).T)."""
    if y is None:
        d = oracle(x, x, x_len, x_len)
        return 0.5 * (d + d.T)
    return 0.5 * (oracle(x, y, x_len, y_len) + oracle(y, x, y_len, x_len).T)


def relative_gap(a, b, skip_diagonal=False):
    """max |a - b| / b over the entries with b > 0; entries where b = 0 must agree exactly up to 1e-12."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if skip_diagonal:
        off = ~np.eye(len(b), dtype=bool)
        a, b = a[off], b[off]
    zero = b == 0
    assert (np.abs(a[zero]) <= 1e-12).all()
    return float((np.abs(a - b)[~zero] / b[~zero]).max()) if (~zero).any() else 0.0


# ---- the inputs of the GPU tests, their float64 values and their bars, computed once ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def clouds(n, P, seed):
    return np.random.default_rng(seed).standard_normal((n, P, 3)).astype(np.float32)


# (P, Q, M, N): every instantiation boundary, P != Q, the mass ratio T / L; 3 x 5 clouds are no multiple of any chunk
DIRECTED_SHAPES = [(1, 1, 3, 5), (3, 5, 3, 5), (70, 50, 3, 5), (256, 256, 3, 5), (257, 300, 3, 5), (512, 512, 3, 5), (513, 1024, 3, 5),
                   (1025, 600, 3, 5), (2048, 2048, 1, 1), (2048, 1, 1, 1), (1, 2048, 1, 1)]


class Case:
    """x, y, lengths; ref: emd_oracle; bar: 4 x the measured fp32-against-float64 error, relative.

    A cloud against itself (the diagonal of a self matrix, y = None) is no relative quantity: its distance is what the 1e-9 guards
    of the spec leave, 1e-12 in float64 and 0 in fp32, and the metrics never read it.  There the same rule holds absolutely:
    diagonal_bar = 4 x max |fp32 - float64| over the diagonal, and `bar` is measured off the diagonal."""
    def __init__(self, x, y, x_len=None, y_len=None, symmetric=False):
        self.x, self.y, self.x_len, self.y_len = x, y, x_len, y_len
        self.self_matrix = y is None
        if symmetric:
            self.ref = emd_matrix_oracle(x, y, x_len, y_len)
            low = emd_matrix_oracle(x, y, x_len, y_len, oracle=emd_oracle_fp32)
        else:
            yy, yl = (x, x_len) if y is None else (y, y_len)
            self.ref, low = emd_oracle(x, yy, x_len, yl), emd_oracle_fp32(x, yy, x_len, yl)
        self.measured = relative_gap(low, self.ref, self.self_matrix)
        self.bar = 4 * self.measured
        self.diagonal_bar = 4 * float(np.abs(np.diag(low) - np.diag(self.ref)).max()) if self.self_matrix else None

    def errors(self, got):
        """-> (relative error off the diagonal of a self matrix or everywhere, absolute error on that diagonal or None)."""
        got = np.asarray(got, dtype=np.float64)
        return (relative_gap(got, self.ref, self.self_matrix),
                float(np.abs(np.diag(got) - np.diag(self.ref)).max()) if self.self_matrix else None)


@functools.lru_cache(maxsize=None)
def directed_case(P, Q, M, N):
    return Case(clouds(M, P, 1000 + P), clouds(N, Q, 2000 + Q))


X_LEN, Y_LEN = [70, 1, 64, 33], [300, 1, 257, 256, 37]


@functools.lru_cache(maxsize=None)
def ragged_case():
    """Rows at or after a cloud's length are NaN: one read too far and the entry is NaN."""
    x, y = clouds(4, 70, 61).copy(), clouds(5, 300, 62).copy()
    for c, lens in ((x, X_LEN), (y, Y_LEN)):
        for i, n in enumerate(lens):
            c[i, n:] = np.nan
    return Case(x, y, X_LEN, Y_LEN)


@functools.lru_cache(maxsize=None)
def clamped_case():
    """What GPU lengths of 0 and P + 7 must behave as: 1 and P."""
    x, y = clouds(4, 70, 61), clouds(5, 300, 62)
    return Case(x, y, [1, 1, 70, 70], [1, 1, 300, 300, 300])


@functools.lru_cache(maxsize=None)
def self_case():
    return Case(clouds(6, 100, 71), None, symmetric=True)


@functools.lru_cache(maxsize=None)
def strided_case():
    return Case(clouds(3, 130, 91), clouds(4, 70, 92))


def shifted_clouds():
    """128 points; the same points in another order, 0.01 further along x: the matching is the permutation, the distance 0.01."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 128, 3)).astype(np.float32)
    y = x[:, rng.permutation(128)].copy()
    y[..., 0] += np.float32(0.01)
    return x, y


@functools.lru_cache(maxsize=None)
def shifted_case():
    return Case(*shifted_clouds())


@functools.lru_cache(maxsize=None)
def far_case():
    rng = np.random.default_rng(81)
    x = (np.float32(100) + np.float32(1e-3) * rng.standard_normal((4, 200, 3)).astype(np.float32)).astype(np.float32)
    y = (np.float32(100) + np.float32(1e-3) * rng.standard_normal((6, 300, 3)).astype(np.float32)).astype(np.float32)
    return Case(x, y)


@functools.lru_cache(maxsize=None)
def stream_case():
    return Case(clouds(5, 40, 31), clouds(6, 50, 32))


@functools.lru_cache(maxsize=None)
def metric_cases():
    """The union sets of test_chamfer_cpu.metric_sets(): (generated, reference) and (twins, reference), symmetric EMD."""
    gen, ref, twins = metric_sets()
    return Case(np.concatenate([gen, ref]), None, symmetric=True), Case(np.concatenate([twins, ref]), None, symmetric=True)


def metrics_emd_float64(matrix, M):
    """The float64 metric implementation of test_chamfer_cpu under the EMD names."""
    got = metrics_float64(matrix, M)
    return {"mmd_emd": got["mmd_cd"], "cov_matched_emd": got["cov_matched"], "nna_correct_emd": got["nna_correct"],
            "num_generated": got["num_generated"], "num_reference": got["num_reference"]}


def check_metrics_emd(got, want, bar):
    """Counts equal, MMD within the relative bar; the derived ratios follow from the counts."""
    M, N = want["num_generated"], want["num_reference"]
    assert got["cov_matched_emd"] == want["cov_matched_emd"] and got["nna_correct_emd"] == want["nna_correct_emd"], (got, want)
    assert (got["num_generated"], got["num_reference"]) == (M, N)
    assert got["cov_emd"] == want["cov_matched_emd"] / N and got["nna_emd"] == want["nna_correct_emd"] / (M + N)
    err = abs(got["mmd_emd"] - want["mmd_emd"]) / want["mmd_emd"]
    print(f"mmd_emd {got['mmd_emd']:.8g} against {want['mmd_emd']:.8g}: error / bar = {err / bar:.3f}")
    assert err <= bar, (got["mmd_emd"], want["mmd_emd"], err, bar)


# ---- preconditions, asserted and never skipped ------------------------------------------------------------------------------------------
def test_the_metric_sets_meet_their_precondition():
    plain, twin = metric_cases()
    gap = smallest_argmin_gap(plain.ref, 20)
    want = metrics_float64(plain.ref, 20)
    print(f"metric sets: fp32 against float64 {plain.measured:.3g}, bar {plain.bar:.3g}, smallest gap {gap:.3g}; COV "
          f"{want['cov_matched']}/24, 1-NNA {want['nna_correct']}/44, MMD {want['mmd_cd']:.6f}")
    assert gap > 4 * plain.bar
    assert (want["cov_matched"], want["nna_correct"]) == (13, 23) and abs(want["mmd_cd"] - 0.904861) < 5e-6
    twin_gap = smallest_argmin_gap(twin.ref, 24)
    print(f"twin set: fp32 against float64 {twin.measured:.3g}, bar {twin.bar:.3g}, smallest gap {twin_gap:.3g}")
    assert twin_gap > 4 * twin.bar
    assert (plain.ref == plain.ref.T).all() and (twin.ref == twin.ref.T).all()


def test_leftover_mass_is_below_1e_6_of_the_total():
    gen, ref, _ = metric_sets()
    for x, y in ((gen[0], ref[0]), (gen[1][:50], ref[1]), (clouds(1, 300, 7)[0], clouds(1, 70, 8)[0])):
        _, remain_l, remain_r, T = _emd_pair(x, y, np.float64, _sum64)
        print(f"Lx {len(x)} Ly {len(y)}: leftover {remain_l.sum() / T:.3g} and {remain_r.sum() / T:.3g} of the mass")
        assert remain_l.sum() < 1e-6 * T and remain_r.sum() < 1e-6 * T


def test_a_permuted_and_shifted_cloud_is_its_shift_away():
    x, y = shifted_clouds()
    got = emd_oracle(x, y)[0, 0]
    print(f"permuted copy shifted by 0.01: {got:.10f}")
    assert abs(got - 0.01) <= 1e-5 * 0.01


def test_the_directed_distance_is_directed():
    a, b = emd_oracle(clouds(1, 70, 3), clouds(1, 50, 4))[0, 0], emd_oracle(clouds(1, 50, 4), clouds(1, 70, 3))[0, 0]
    assert abs(a - b) > 1e-6 * a


def test_the_bars_of_the_gpu_tests():
    """Measured here from the two oracles, printed, and written into DESIGN.md 5.8.  A bar is a positive number (the fp32 evaluation
    does differ from float64) and stays far below the quantity itself."""
    rows = [(f"directed P {P} Q {Q} M {M} N {N}", directed_case(P, Q, M, N)) for P, Q, M, N in DIRECTED_SHAPES]
    rows += [("ragged lengths", ragged_case()), ("clamped lengths", clamped_case()), ("self matrix", self_case()),
             ("strided input", strided_case()), ("shifted copy", shifted_case()), ("far from the origin", far_case()),
             ("direct C call", stream_case()), ("metric sets", metric_cases()[0]), ("twin set", metric_cases()[1])]
    for name, case in rows:
        print(f"{name}: fp32 against float64 {case.measured:.3g} -> bar {case.bar:.3g}")
        assert np.isfinite(case.ref).all() and (case.ref >= 0).all()
        assert case.bar < 1e-2, name
        if case.self_matrix:
            print(f"{name}: diagonal, fp32 against float64 {case.diagonal_bar / 4:.3g} absolute -> bar {case.diagonal_bar:.3g}")
            assert 0 < case.diagonal_bar < 1e-9 * case.ref.max(), name
        # a single point against a single point is exact in both formats: there the bar is 0 and the kernel has to be exact too
        assert case.bar > 0 or name.startswith("directed P 1 Q 1 "), name


# ---- the reductions -------------------------------------------------------------------------------------------------------------------
def test_metrics_from_distance_on_the_metric_sets():
    from npcd.eval import metrics_from_chamfer, metrics_from_distance
    for case, M in zip(metric_cases(), (20, 24)):
        for t in (torch.from_numpy(case.ref), torch.from_numpy(case.ref.astype(np.float32))):
            got = metrics_from_distance(t, M, "emd")
            check_metrics_emd(got, metrics_emd_float64(case.ref, M), 1e-15 if t.dtype == torch.float64 else 2.0 ** -24)
            assert isinstance(got["cov_matched_emd"], int) and isinstance(got["nna_correct_emd"], int) and isinstance(got["mmd_emd"], float)
            assert set(got) == {"mmd_emd", "cov_emd", "nna_emd", "cov_matched_emd", "nna_correct_emd", "num_generated", "num_reference"}
            # the Chamfer reduction is the same reduction under its present names
            cd = metrics_from_chamfer(t, M)
            assert set(cd) == {"mmd_cd", "cov_cd", "nna_cd", "cov_matched", "nna_correct", "num_generated", "num_reference"}
            assert (cd["mmd_cd"], cd["cov_cd"], cd["nna_cd"], cd["cov_matched"], cd["nna_correct"]) == (
                got["mmd_emd"], got["cov_emd"], got["nna_emd"], got["cov_matched_emd"], got["nna_correct_emd"])
    with pytest.raises(ValueError, match="square"):
        metrics_from_distance(torch.zeros(3, 4), 1, "emd")


def test_emd_false_leaves_the_dict_as_it_is(monkeypatch):
    """shape_metrics with stand-in matrices on the CPU: without emd the keys of today, with it the EMD keys beside them and the CD
    values untouched."""
    from npcd.eval import shape_metrics
    from npcd.hip import chamfer, emd
    plain, _ = metric_cases()
    cd = torch.from_numpy(np.random.default_rng(0).uniform(1, 2, (44, 44)))
    cd = cd + cd.t()
    calls = []
    monkeypatch.setattr(chamfer, "chamfer_matrix", lambda x, *a: calls.append("cd") or cd)
    monkeypatch.setattr(emd, "emd_matrix", lambda x, *a: calls.append("emd") or torch.from_numpy(plain.ref))
    gen, ref = torch.zeros(20, 64, 3), torch.zeros(24, 64, 3)
    today = {"mmd_cd", "cov_cd", "nna_cd", "cov_matched", "nna_correct", "num_generated", "num_reference"}
    without = shape_metrics(gen, ref)
    assert set(without) == today and calls == ["cd"]
    assert shape_metrics(gen, ref, emd=False) == without
    calls.clear()
    both = shape_metrics(gen, ref, emd=True)
    assert calls == ["cd", "emd"]          # one launch each on the union set
    assert set(both) == today | {"mmd_emd", "cov_emd", "nna_emd", "cov_matched_emd", "nna_correct_emd"}
    assert {k: both[k] for k in today} == without
    check_metrics_emd(both, metrics_emd_float64(plain.ref, 20), 1e-15)


def test_eval_exports_the_new_name_without_a_gpu():
    import npcd.eval
    from npcd.eval import shapes
    assert npcd.eval.metrics_from_distance is shapes.metrics_from_distance


# ---- the wrapper and the C entry point ------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    from npcd.hip.emd import emd_directed, emd_matrix
    from npcd.eval import shape_metrics
    with pytest.raises(RuntimeError, match="GPU"):
        emd_directed(torch.zeros(2, 10, 3))
    with pytest.raises(RuntimeError, match="GPU"):
        emd_matrix(torch.zeros(2, 10, 3), torch.zeros(3, 7, 3), x_lengths=[10, 3], y_lengths=torch.tensor([7, 1, 2]))
    with pytest.raises(RuntimeError, match="GPU"):
        shape_metrics(torch.zeros(2, 10, 3), torch.zeros(3, 10, 3), emd=True)


def test_bad_arguments_are_refused_on_the_host():
    from npcd.hip.emd import emd_directed, emd_matrix
    x, y = torch.zeros(2, 10, 3), torch.zeros(3, 7, 3)
    for fn in (emd_directed, emd_matrix):
        with pytest.raises(RuntimeError, match="supports fp32"):
            fn(x.double())
        with pytest.raises(RuntimeError, match="supports fp32"):
            fn(x, y.half())
        with pytest.raises(ValueError, match=r"emd: x must be \[n, P, 3\]"):
            fn(torch.zeros(2, 10, 2))
        with pytest.raises(ValueError, match=r"\[n, P, 3\]"):
            fn(x, torch.zeros(7, 3))
        with pytest.raises(ValueError, match=r"\[n, P, 3\]"):
            fn(torch.zeros(0, 10, 3))
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=[10, 11])
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=[0, 10])
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=torch.tensor([10, -1]))
        with pytest.raises(ValueError, match="lengths"):
            fn(x, x_lengths=[10])
        with pytest.raises(ValueError, match="y_lengths"):
            fn(x, y, y_lengths=[7, 7, 8])
        with pytest.raises(ValueError, match="y_lengths"):
            fn(x, y_lengths=[10, 10])


def test_host_side_query_and_refusals():
    from npcd import hip
    from npcd.hip import emd
    L = hip.lib()
    largest = L.npcd_emd_max_points()
    assert largest >= 2048 and emd.max_points() == largest
    null = ctypes.c_void_p(0)
    unsupported = -2
    # refused before any pointer is looked at and before any launch: null pointers, no GPU
    for M, P, N, Q in ((0, 8, 1, 8), (1, 0, 1, 8), (1, 8, 0, 8), (1, 8, 1, 0), (-1, 8, 1, 8), (1, -8, 1, 8), (1, 8, -1, 8), (1, 8, 1, -8),
                       (1, largest + 1, 1, 8), (1, 8, 1, largest + 1), (1 << 30, 8, 1, 8), (1, 8, 1 << 30, 8), (16385, 8, 1, 8), (1, 8, 16385, 8)):
        assert L.npcd_emd_directed(null, null, null, null, null, M, P, N, Q, null) == unsupported, (M, P, N, Q)
    assert L.npcd_emd_directed(null, null, null, null, null, 16384, largest, 16384, largest, null) == -1          # supported, but no buffers


# ---- the kernels' resources -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emd_kernels(tmp_path_factory):
    return _compile("emd.hip", str(tmp_path_factory.mktemp("emd_resources") / "emd.s"))


def test_emd_kernels_use_no_scratch_and_keep_four_waves_per_simd(emd_kernels):
    """Sixteen instantiations <owned X points per lane, owned Y points per lane>.  Scratch 0 everywhere; at most 128 registers, the
    bar for P <= 1,024, in every one of them (the 2,048-point forms too: 104 in <8, 8>, the table of DESIGN.md 5.8).  Static LDS is
    the four per-wave partial sums alone: the pair's images are dynamic LDS, 256 (16 PPL + 20 QPL) bytes, sized by the launch."""
    forms = {(p, q) for p in (1, 2, 4, 8) for q in (1, 2, 4, 8)}
    seen = set()
    for k, v in emd_kernels.items():
        tag = [f for f in forms if f"emd_kernelILi{f[0]}ELi{f[1]}EE" in k]
        assert len(tag) == 1, k
        seen.add(tag[0])
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] == 4 * 4, (k, v)
        assert v["vgpr"] <= 128, (k, v)
    assert seen == forms and len(emd_kernels) == 16


def test_emd_source_is_compiled_without_contraction():
    from test_kernel_resources import _build_py
    assert "-ffp-contract=off" in _build_py().SOURCES["emd.hip"]
