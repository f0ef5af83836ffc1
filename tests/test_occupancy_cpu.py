"""The occupancy-grid kernel and the Jensen-Shannon divergence on it, everything that needs no GPU: the float64 oracle written from the
spec of DESIGN.md 5.9 (lattice, mask, brute-force assignment with its bar, histograms, JSD, occupancy entropy), the host helpers, the
reductions on CPU tensors, the wrapper's refusals, the host-side query and refusals of the C entry point, the preconditions of the
sets that tests/test_gpu_occupancy.py uses, the kernel's resources as the compiler reports them.

The bar of an assignment is the spec's, derived there and not measured: with d_best the least float64 squared distance from the fp32
point to a valid centre and d_got that of the chosen cell, d_got - d_best <= 16 u d_best + 32 u e s, u = 2^-24, s = 2 e / (R - 1);
where the float64 gap between the best and the second-best valid cell exceeds 4 bars the cell must be the float64 arg-min."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_chamfer_cpu import metric_sets
from test_kernel_resources import _compile

U = 2.0 ** -24


# ---- oracle, from the spec of DESIGN.md 5.9 -------------------------------------------------------------------------------------------
def lattice_oracle(R, e):
    """g[a] = fp32(a (2 e / (R - 1)) - e), computed in float64 and rounded once."""
    return (np.arange(R, dtype=np.float64) * (2.0 * e / (R - 1)) - e).astype(np.float32)


def mask_oracle(R, e, in_sphere):
    """bool [R, R, R]: float64 on the fp32 table values."""
    if not in_sphere:
        return np.ones((R, R, R), dtype=bool)
    g = lattice_oracle(R, e).astype(np.float64)
    out = np.empty((R, R, R), dtype=bool)
    for i in range(R):
        for j in range(R):
            for k in range(R):
                out[i, j, k] = g[i] * g[i] + g[j] * g[j] + g[k] * g[k] <= e * e
    return out


def bar_of(d_best, R, e):
    return 16 * U * d_best + 32 * U * e * (2.0 * e / (R - 1))


def distances_to_cells(points, R, e):
    """float64 squared distances [N, R^3] from fp32 points [N, 3] to every centre, ((dx dx + dy dy) + dz dz)."""
    g = lattice_oracle(R, e).astype(np.float64)
    sq = (np.asarray(points, dtype=np.float32).astype(np.float64)[:, :, None] - g[None, None, :]) ** 2          # [N, 3, R]
    return ((sq[:, 0, :, None, None] + sq[:, 1, None, :, None]) + sq[:, 2, None, None, :]).reshape(len(points), -1)


def assign_oracles(points, R, e, masks, chunk=256):
    """Brute force over all valid centres, float64, for each of `masks` (in_sphere flags) on one evaluation of the distances.
    points [..., 3] fp32 (all finite) -> per mask, flat arrays over the points: `cell`, the arg-min; `d_best`; `gap` to the
    second-best valid cell (inf when only one is valid); `bar`."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    assert np.isfinite(pts).all()
    invalid = [~mask_oracle(R, e, m).reshape(-1) for m in masks]
    assert not any(i.all() for i in invalid)
    out = [tuple(np.empty(len(pts), dtype=t) for t in (np.int64, np.float64, np.float64)) for _ in masks]
    rows = np.arange(chunk)
    for p0 in range(0, len(pts), chunk):
        d = distances_to_cells(pts[p0:p0 + chunk], R, e)
        n = len(d)
        for bad, (cell, d_best, second) in sorted(zip(invalid, out), key=lambda t: t[0].sum()):          # masks only shrink
            d[:, bad] = np.inf
            best = d.argmin(axis=1)
            mine = d[rows[:n], best]
            cell[p0:p0 + n], d_best[p0:p0 + n] = best, mine
            d[rows[:n], best] = np.inf
            second[p0:p0 + n] = d.min(axis=1)
            d[rows[:n], best] = mine
    return [SimpleNamespace(cell=cell, d_best=d_best, gap=second - d_best, bar=bar_of(d_best, R, e)) for cell, d_best, second in out]


def assign_oracle(points, R, e, in_sphere):
    return assign_oracles(points, R, e, (in_sphere,))[0]


def distance_to_cell(points, cells, R, e):
    """float64 squared distance of every point to the centre of the cell given for it (flat index)."""
    g = lattice_oracle(R, e).astype(np.float64)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    cells = np.asarray(cells).reshape(-1)
    dx, dy, dz = pts[:, 0] - g[cells // (R * R)], pts[:, 1] - g[cells // R % R], pts[:, 2] - g[cells % R]
    return (dx * dx + dy * dy) + dz * dz


def histograms(cells, R):
    """cells [n, P] with -1 for points not counted -> (points per cell, clouds per cell), int64 [R^3]."""
    cells = np.asarray(cells)
    counts = np.bincount(cells[cells >= 0], minlength=R ** 3)
    clouds = np.zeros(R ** 3, dtype=np.int64)
    for row in cells:
        clouds[np.unique(row[row >= 0])] += 1
    return counts, clouds


def _entropy(p, log):
    p = p[p > 0]
    return float(-(p * log(p)).sum())


def jsd_oracle(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    p, q = a / a.sum(), b / b.sum()
    return _entropy(0.5 * (p + q), np.log2) - 0.5 * (_entropy(p, np.log2) + _entropy(q, np.log2))


def occupancy_entropy_oracle(clouds, n, mask):
    total = 0.0
    for c in np.asarray(clouds).reshape(-1):
        if c > 0:
            total += _entropy(np.array([c / n, 1.0 - c / n]), np.log)
    return total / int(np.asarray(mask).sum())


# ---- the sets of the GPU tests ----------------------------------------------------------------------------------------------------------
RANDOM_SHAPES = [(7, 300), (3, 1000), (16, 257)]
GRIDS = [(2, False), (5, False), (5, True), (28, False), (28, True), (32, False), (32, True)]          # (R, in_sphere); R = 2 cube only
EXTENTS = [0.5, 1.0]
UNDECIDED_CAP = 0.005


def random_set(n, P, extent, seed):
    """About 70 % of the points outside the inscribed sphere, four far points in every cloud."""
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-1.24, 1.24, (n, P, 3)) * extent).astype(np.float32)
    pts[:, :4] *= np.float32(6)
    return pts


def seed_of(n, P, R, extent):
    return 1000 * R + 10 * n + int(extent * 2)


@functools.lru_cache(maxsize=None)
def _random_cases(n, P, R, extent):
    pts = random_set(n, P, extent, seed_of(n, P, R, extent))
    masks = [m for r, m in GRIDS if r == R]
    cases = dict(zip(masks, assign_oracles(pts, R, extent, masks)))
    for c in cases.values():
        c.points = pts
    return cases


def random_case(n, P, R, in_sphere, extent):
    return _random_cases(n, P, R, extent)[in_sphere]


@functools.lru_cache(maxsize=None)
def normalized_metric_sets():
    """The sets of test_chamfer_cpu.metric_sets(), bbox-normalised in fp32 by the package's own normalize_clouds (plain torch)."""
    from npcd.eval import normalize_clouds
    return tuple(normalize_clouds(torch.from_numpy(c), "bbox").numpy() for c in metric_sets())


METRIC_JSD = 0.767828098          # oracle, generated against reference, R = 28, extent 1, sphere


@functools.lru_cache(maxsize=None)
def metric_case(in_sphere=True):
    gen, ref, twins = normalized_metric_sets()
    return tuple(assign_oracle(c, 28, 1.0, in_sphere) for c in (gen, ref, twins))


# ---- host helpers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R, e", [(2, 0.5), (5, 1.0), (28, 0.5), (28, 1.0), (32, 0.5), (7, 0.3)])
def test_lattice_and_mask_equal_the_oracle_bit_for_bit(R, e):
    from npcd.hip.occupancy import grid_lattice, grid_mask
    g = grid_lattice(R, e)
    assert g.dtype == torch.float32 and g.shape == (R,) and not g.is_cuda
    np.testing.assert_array_equal(g.numpy().view(np.uint32), lattice_oracle(R, e).view(np.uint32))
    for in_sphere in (False, True):
        m = grid_mask(R, e, in_sphere)
        assert m.dtype == torch.bool and m.shape == (R, R, R) and not m.is_cuda
        np.testing.assert_array_equal(m.numpy(), mask_oracle(R, e, in_sphere))


def test_the_protocol_grid():
    """R = 28 in the sphere: 10,144 of 21,952 cells, the same under every axis flip and permutation, every column one interval, and
    no cell nearer the sphere than 2.7e-3 in r^2 / e^2."""
    from npcd.hip.occupancy import _columns, grid_lattice, grid_mask
    for e in (0.5, 1.0):
        m = grid_mask(28, e, True).numpy()
        assert m.sum() == 10144 and m.size == 21952
        for axis in range(3):
            np.testing.assert_array_equal(m, np.flip(m, axis))
        for perm in ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
            np.testing.assert_array_equal(m, m.transpose(perm))
        lo, hi = _columns(m)
        k = np.arange(28)
        np.testing.assert_array_equal(m, (k >= lo.reshape(28, 28, 1)) & (k <= hi.reshape(28, 28, 1)))
        assert lo.dtype == np.uint8 and (lo > hi).sum() == (~m.any(axis=2)).sum() > 0
        g = grid_lattice(28, e).double().numpy() ** 2
        r2 = (g[:, None, None] + g[None, :, None] + g[None, None, :]) / (e * e)
        print(f"extent {e}: the cell closest to the sphere is {np.abs(r2 - 1).min():.3g} away in r^2 / e^2")
        assert np.abs(r2 - 1).min() > 2.5e-3
    assert grid_mask(28, 0.5, False).all()


def test_an_empty_mask_and_bad_grids_are_refused():
    from npcd.hip.occupancy import grid_lattice, grid_mask, occupancy_grid
    assert not grid_mask(2, 0.5, True).any() and grid_mask(2, 0.5, False).all()
    with pytest.raises(ValueError, match="no cell"):
        occupancy_grid(torch.zeros(2, 10, 3), resolution=2, in_sphere=True)
    for fn in (grid_lattice, grid_mask):
        with pytest.raises(ValueError, match="resolution"):
            fn(1, 0.5)
        for e in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="extent"):
                fn(28, e)


# ---- the reductions ---------------------------------------------------------------------------------------------------------------------
def test_jsd_from_counts():
    from npcd.eval import jsd_from_counts
    rng = np.random.default_rng(0)
    for shape in ((28, 28, 28), (125,)):
        a, b = rng.integers(0, 9, shape), rng.integers(0, 9, shape)
        a[rng.random(shape) < 0.4] = 0
        ta, tb = torch.from_numpy(a), torch.from_numpy(b)
        got, want = jsd_from_counts(ta, tb), jsd_oracle(a, b)
        print(f"{shape}: {got:.12f} against {want:.12f}")
        assert isinstance(got, float) and 0 < got < 1 and abs(got - want) <= 1e-12
        assert jsd_from_counts(ta, ta) == 0.0 and jsd_from_counts(tb.int(), tb.int()) == 0.0
        assert jsd_from_counts(tb, ta) == got                                      # symmetric
        assert abs(jsd_from_counts(ta, 7 * tb) - got) <= 1e-12                      # the scale of a side does not matter
        assert abs(jsd_from_counts(ta.float(), tb.int()) - got) <= 1e-12
    x, y = torch.zeros(50, dtype=torch.int32), torch.zeros(50, dtype=torch.int32)
    x[:20] = torch.arange(1, 21, dtype=torch.int32)
    y[30:] = 3
    assert abs(jsd_from_counts(x, y) - 1.0) <= 1e-12          # disjoint supports
    with pytest.raises(ValueError, match="empty"):
        jsd_from_counts(x, torch.zeros(50))
    with pytest.raises(ValueError, match="empty"):
        jsd_from_counts(torch.zeros(50), y)
    with pytest.raises(ValueError, match="shape"):
        jsd_from_counts(x, torch.ones(49))


def test_occupancy_entropy():
    from npcd.eval import occupancy_entropy
    from npcd.hip.occupancy import grid_mask
    rng = np.random.default_rng(1)
    mask = grid_mask(28, 0.5, True)
    clouds = rng.integers(0, 25, (28, 28, 28)) * mask.numpy()
    clouds[rng.random(clouds.shape) < 0.3] = 0
    got, want = occupancy_entropy(torch.from_numpy(clouds), 24, mask), occupancy_entropy_oracle(clouds, 24, mask.numpy())
    print(f"occupancy entropy {got:.12f} against {want:.12f}")
    assert isinstance(got, float) and got > 0 and abs(got - want) <= 1e-12
    # every cloud in a cell, or none, carries no entropy; half of them carry ln 2
    assert occupancy_entropy(torch.full((5, 5, 5), 24), 24, torch.ones(5, 5, 5, dtype=torch.bool)) == 0.0
    assert abs(occupancy_entropy(torch.full((5, 5, 5), 12), 24, torch.ones(5, 5, 5, dtype=torch.bool)) - np.log(2)) <= 1e-15
    with pytest.raises(ValueError, match="shape"):
        occupancy_entropy(torch.zeros(5, 5, 5), 3, torch.ones(5, 5, 4, dtype=torch.bool))


def test_eval_exports_the_new_names_without_a_gpu():
    import npcd.eval
    from npcd.eval import shapes
    for name in ("jsd_from_counts", "occupancy_entropy", "jensen_shannon_divergence"):
        assert getattr(npcd.eval, name) is getattr(shapes, name)


def test_jsd_false_leaves_the_dict_as_it_is(monkeypatch):
    """shape_metrics with stand-ins on the CPU: without jsd the keys of today; with it the five keys beside them, the extent chosen
    from `normalize`, and the other values untouched."""
    from npcd.eval import shape_metrics
    from npcd.hip import chamfer, occupancy
    cd = torch.from_numpy(np.random.default_rng(0).uniform(1, 2, (44, 44)))
    cd = cd + cd.t()
    calls = []

    def grid(points, lengths, resolution, extent, in_sphere):
        calls.append((points.shape[0], resolution, extent, in_sphere))
        h = torch.zeros(resolution, resolution, resolution, dtype=torch.int32)
        h[resolution // 2, resolution // 2, : points.shape[0] // 4] = 4
        return h, (h > 0).int() * 3

    monkeypatch.setattr(chamfer, "chamfer_matrix", lambda x, *a: cd)
    monkeypatch.setattr(occupancy, "occupancy_grid", grid)
    gen, ref = torch.zeros(20, 64, 3), torch.ones(24, 64, 3)
    today = {"mmd_cd", "cov_cd", "nna_cd", "cov_matched", "nna_correct", "num_generated", "num_reference"}
    new = {"jsd", "occupancy_entropy_generated", "occupancy_entropy_reference", "occupied_cells_generated", "occupied_cells_reference"}
    without = shape_metrics(gen, ref)
    assert set(without) == today and not calls and shape_metrics(gen, ref, jsd=False) == without
    both = shape_metrics(gen, ref, jsd=True)
    assert calls == [(20, 28, 0.5, True), (24, 28, 0.5, True)]
    assert set(both) == today | new and {k: both[k] for k in today} == without
    assert (both["occupied_cells_generated"], both["occupied_cells_reference"]) == (5, 6) and 0 < both["jsd"] < 1
    want = occupancy_entropy_oracle(np.full(5, 3), 20, np.ones(10144))
    assert abs(both["occupancy_entropy_generated"] - want) <= 1e-15
    calls.clear()
    shape_metrics(gen, ref, normalize="bbox", jsd=True, jsd_resolution=16)
    shape_metrics(gen, ref, normalize="bbox", jsd=True, jsd_extent=0.75)
    assert [c[1:] for c in calls] == [(16, 1.0, True)] * 2 + [(28, 0.75, True)] * 2


# ---- the wrapper and the C entry point --------------------------------------------------------------------------------------------------
def test_the_wrapper_refuses():
    from npcd.eval import jensen_shannon_divergence, shape_metrics
    from npcd.hip.occupancy import max_resolution, occupancy_grid
    x = torch.zeros(2, 10, 3)
    assert max_resolution() == 32
    with pytest.raises(RuntimeError, match="GPU"):
        occupancy_grid(x)
    with pytest.raises(RuntimeError, match="GPU"):
        occupancy_grid(x, lengths=[10, 3], return_cells=True)
    with pytest.raises(RuntimeError, match="GPU"):
        jensen_shannon_divergence(x, x)
    with pytest.raises(RuntimeError, match="GPU"):
        shape_metrics(x, x, jsd=True)
    with pytest.raises(RuntimeError, match="supports fp32"):
        occupancy_grid(x.double())
    for bad in (torch.zeros(2, 10, 2), torch.zeros(10, 3), torch.zeros(0, 10, 3), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError, match=r"occupancy_grid: points must be \[n, P, 3\]"):
            occupancy_grid(bad)
    for resolution in (1, 33, 0, -28, 28.0):
        with pytest.raises(ValueError, match="resolution"):
            occupancy_grid(x, resolution=resolution)
    for extent in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="extent"):
            occupancy_grid(x, extent=extent)
    for lengths in ([10], [10, 10, 10], [10, 11], [0, 10], torch.tensor([10, -1])):
        with pytest.raises(ValueError, match="lengths"):
            occupancy_grid(x, lengths=lengths)


def test_host_side_query_and_refusals():
    from npcd import hip
    L = hip.lib()
    assert L.npcd_occupancy_max_resolution() == 32
    null = ctypes.c_void_p(0)
    unsupported = -2
    # refused before any pointer is looked at and before any launch: null pointers, no GPU
    for n, P, R in ((0, 8, 28), (8, 0, 28), (-1, 8, 28), (8, -1, 28), (1 << 16, 1 << 15, 28), (1, 1 << 31, 28), (3, 1 << 30, 28), (8, 8, 1),
                    (8, 8, 33), (8, 8, 0), (8, 8, -28)):
        P = ctypes.c_int(P).value          # 2^31 arrives as a negative int
        assert L.npcd_occupancy_grid(null, null, null, null, null, null, null, null, n, P, R, null) == unsupported, (n, P, R)
        assert L.npcd_occupancy_clouds_per_workgroup(n, P, R) == unsupported, (n, P, R)
    for n, P, R in ((1, 1, 2), (1, (1 << 31) - 1, 32), ((1 << 31) - 1, 1, 28), (1 << 15, (1 << 16) - 1, 28)):
        assert L.npcd_occupancy_grid(null, null, null, null, null, null, null, null, n, P, R, null) == -1, (n, P, R)          # supported, no buffers
        assert 1 <= L.npcd_occupancy_clouds_per_workgroup(n, P, R) <= n
    assert [L.npcd_error_string(c) for c in (0, -1, -2, -3)] == [b"ok", b"invalid argument", b"unsupported shape or dtype", b"HIP runtime error"]


# ---- preconditions, asserted and never skipped ------------------------------------------------------------------------------------------
def test_the_metric_sets_meet_their_precondition():
    """Every point of the bbox-normalised generated and reference sets is decided by more than 4 bars, with and without the sphere: the kernel's
    histograms are then the oracle's exactly, and so is the JSD up to the float64 reduction."""
    for in_sphere in (True, False):
        cases = metric_case(in_sphere)[:2]          # generated and reference; the twins are compared with no oracle
        ratio = min(float((c.gap / c.bar).min()) for c in cases)
        print(f"in_sphere {in_sphere}: smallest gap / bar = {ratio:.1f}")
        assert ratio > 4
    gen, ref, twins = metric_case(True)
    outside = (np.concatenate(normalized_metric_sets()[:2]).astype(np.float64) ** 2).sum(-1).reshape(-1).__gt__(1).mean()
    value = jsd_oracle(histograms(gen.cell.reshape(20, 64), 28)[0], histograms(ref.cell.reshape(24, 64), 28)[0])
    near = jsd_oracle(histograms(twins.cell.reshape(24, 64), 28)[0], histograms(ref.cell.reshape(24, 64), 28)[0])
    print(f"JSD {value:.9f}, twins {near:.6f}; {100 * outside:.0f} % of the points lie outside the sphere")
    assert abs(value - METRIC_JSD) <= 5e-10 and near < 0.05


@pytest.mark.parametrize("n, P", RANDOM_SHAPES)
def test_the_random_sets_meet_their_precondition(n, P):
    """At most 0.5 % of a set's points may lie within 4 bars of a tie: the exact comparison then covers 99.5 % of the points and
    the bar covers all of them."""
    for extent in EXTENTS:
        for R, in_sphere in GRIDS:
            case = random_case(n, P, R, in_sphere, extent)
            undecided = int((case.gap <= 4 * case.bar).sum())
            outside = float(((case.points.astype(np.float64) ** 2).sum(-1) > extent * extent).mean())
            print(f"n {n} P {P} R {R} sphere {in_sphere} extent {extent}: {undecided} of {n * P} points undecided, "
                  f"{100 * outside:.0f} % outside the sphere")
            assert undecided <= UNDECIDED_CAP * n * P
            assert 0.6 < outside < 0.8 and float(np.abs(case.points[:, :4]).max()) > 5 * extent


# ---- the kernel's resources -------------------------------------------------------------------------------------------------------------
def test_occupancy_kernel_uses_no_scratch(tmp_path):
    """One kernel; no scratch; its LDS is dynamic, sized by the launch, so the static figure is 0; 1,024 lanes a
    workgroup allow 128 registers."""
    kernels = _compile("occupancy.hip", str(tmp_path / "occupancy.s"))
    assert len(kernels) == 1 and "occupancy_kernel" in next(iter(kernels)), sorted(kernels)
    for k, v in kernels.items():
        print(f"{k}: {v['vgpr']} VGPRs, {v['lds']} bytes of static LDS, {v['scratch']} bytes of scratch")
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgpr"] <= 128, (k, v)


def test_occupancy_source_is_compiled_without_contraction():
    from test_kernel_resources import _build_py
    assert "-ffp-contract=off" in _build_py().SOURCES["occupancy.hip"]
