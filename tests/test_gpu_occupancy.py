"""The occupancy-grid kernel (csrc/occupancy.hip) and the Jensen-Shannon divergence on it (npcd/eval/shapes.py) against the float64
oracle of tests/test_occupancy_cpu.py, written from the spec of DESIGN.md 5.9.

An assignment is held to the spec's bar, which is derived and not measured: d_got - d_best <= 16 u d_best + 32 u e s in float64, and
the oracle's arg-min exactly wherever the gap to the second-best valid cell exceeds 4 bars.  The histograms are integers and are
compared exactly.  Every assignment test prints its worst excess / bar and the number of points it could not compare exactly."""
import numpy as np
import pytest
import torch

from test_chamfer_cpu import metric_sets
from test_occupancy_cpu import (EXTENTS, GRIDS, METRIC_JSD, RANDOM_SHAPES, assign_oracle, distance_to_cell, histograms, jsd_oracle,
                                lattice_oracle, mask_oracle, occupancy_entropy_oracle, random_case, random_set)

pytestmark = pytest.mark.gpu


def _gpu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid(points, lengths=None, R=28, extent=0.5, in_sphere=True, **kw):
    """-> (counts, clouds, cells) as numpy arrays, through the wrapper."""
    from npcd.hip.occupancy import occupancy_grid
    pts = points if isinstance(points, torch.Tensor) else _gpu(points)
    counts, clouds, cells = occupancy_grid(pts, lengths, R, extent, in_sphere, return_cells=True, **kw)
    assert counts.shape == clouds.shape == (R, R, R) and cells.shape == pts.shape[:2]
    assert counts.dtype == clouds.dtype == cells.dtype == torch.int32
    return counts.cpu().numpy().reshape(-1), clouds.cpu().numpy().reshape(-1), cells.cpu().numpy()


def _hold_histograms(counts, clouds, cells, R):
    """The two histograms are those of the kernel's own cells, exactly."""
    want_counts, want_clouds = histograms(cells, R)
    np.testing.assert_array_equal(counts, want_counts)
    np.testing.assert_array_equal(clouds, want_clouds)
    assert counts.sum() == (cells >= 0).sum()


def _hold_assignment(cells, points, want, R, extent, in_sphere, what):
    """cells of the counted points (all of `points`) against the oracle's `want`: valid, within the bar, exact where decided."""
    cells = np.asarray(cells).reshape(-1)
    assert cells.min() >= 0 and cells.max() < R ** 3, what
    assert mask_oracle(R, extent, in_sphere).reshape(-1)[cells].all(), what
    excess = distance_to_cell(points, cells, R, extent) - want.d_best
    decided = want.gap > 4 * want.bar
    print(f"{what}: worst excess / bar = {float((excess / want.bar).max()):.3f}, {int((~decided).sum())} of {len(cells)} points undecided, "
          f"{int((cells != want.cell).sum())} differ from the float64 arg-min")
    assert (excess <= want.bar).all(), (what, float((excess / want.bar).max()))
    np.testing.assert_array_equal(cells[decided], want.cell[decided])


# ---- assignment against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS)
@pytest.mark.parametrize("R, in_sphere", GRIDS)
@pytest.mark.parametrize("n, P", RANDOM_SHAPES)
def test_assignment_on_the_random_sets(n, P, R, in_sphere, extent):
    want = random_case(n, P, R, in_sphere, extent)
    counts, clouds, cells = _grid(want.points, None, R, extent, in_sphere)
    _hold_assignment(cells, want.points, want, R, extent, in_sphere, f"n {n} P {P} R {R} sphere {in_sphere} extent {extent}")
    _hold_histograms(counts, clouds, cells, R)


def _centres(valid):
    g = lattice_oracle(28, 0.5)
    i, j, k = np.nonzero(mask_oracle(28, 0.5, True) == valid)
    return np.stack([g[i], g[j], g[k]], axis=1)[None], (i * 28 + j) * 28 + k


def test_the_valid_centres_land_in_their_own_cells():
    pts, own = _centres(True)
    assert pts.shape == (1, 10144, 3)
    counts, clouds, cells = _grid(pts)
    np.testing.assert_array_equal(cells[0], own)
    mask = mask_oracle(28, 0.5, True).reshape(-1).astype(np.int32)
    np.testing.assert_array_equal(counts, mask)
    np.testing.assert_array_equal(clouds, mask)


def test_the_invalid_centres_land_in_valid_cells():
    """Symmetry makes many of them ties: the bar is what holds."""
    pts, _ = _centres(False)
    assert pts.shape == (1, 11808, 3)
    counts, clouds, cells = _grid(pts)
    _hold_assignment(cells, pts, assign_oracle(pts, 28, 0.5, True), 28, 0.5, True, "the 11,808 centres outside the sphere")
    _hold_histograms(counts, clouds, cells, 28)


# ---- edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, P", [(1, 1), (3, 63), (3, 64), (3, 65), (3, 255), (3, 256), (3, 257), (2, 511), (2, 513), (1, 1025)])
def test_edges_of_the_team_sizes(n, P):
    pts = random_set(n, P, 0.5, 500 + P)
    for in_sphere in (True, False):
        counts, clouds, cells = _grid(pts, None, 28, 0.5, in_sphere)
        _hold_assignment(cells, pts, assign_oracle(pts, 28, 0.5, in_sphere), 28, 0.5, in_sphere, f"n {n} P {P} sphere {in_sphere}")
        _hold_histograms(counts, clouds, cells, 28)


@pytest.mark.parametrize("P", [40, 600])
def test_one_cloud_below_at_and_above_a_workgroup(P):
    from npcd.hip.occupancy import clouds_per_workgroup
    group = clouds_per_workgroup(4 * 16, P, 5)
    assert group == (16 if P == 40 else 1)
    for n in sorted({max(1, group - 1), group, group + 1, 2 * group + 1}):
        pts = random_set(n, P, 0.5, 700 + n)
        counts, clouds, cells = _grid(pts, None, 5, 0.5, True)
        print(f"n {n} P {P}: {clouds_per_workgroup(n, P, 5)} clouds per workgroup")
        _hold_assignment(cells, pts, assign_oracle(pts, 5, 0.5, True), 5, 0.5, True, f"n {n} P {P}")
        _hold_histograms(counts, clouds, cells, 5)


def test_many_small_clouds():
    """16,384 clouds of 2 points: 64 clouds per workgroup, four rounds of 16 teams."""
    from npcd.hip.occupancy import clouds_per_workgroup
    assert clouds_per_workgroup(16384, 2, 5) == 64
    pts = random_set(16384, 2, 0.5, 9)
    pts[:, 1] = pts[:, 0] * np.float32(0.3)          # a point inside the sphere beside the far one
    counts, clouds, cells = _grid(pts, None, 5, 0.5, True)
    _hold_assignment(cells, pts, assign_oracle(pts, 5, 0.5, True), 5, 0.5, True, "16,384 clouds of 2 points")
    _hold_histograms(counts, clouds, cells, 5)


def test_a_cloud_larger_than_a_cell_word():
    """70,000 points in one cloud: the cells' words are written out and zeroed on the way, the cloud is still counted once per
    cell; as 70 clouds of 1,000 points the same points give the same cells and counts."""
    pts = random_set(1, 70000, 0.5, 21)
    counts, clouds, cells = _grid(pts, None, 5, 0.5, True)
    _hold_assignment(cells, pts, assign_oracle(pts, 5, 0.5, True), 5, 0.5, True, "one cloud of 70,000 points")
    _hold_histograms(counts, clouds, cells, 5)
    assert clouds.max() == 1
    split_counts, split_clouds, split_cells = _grid(pts.reshape(70, 1000, 3), None, 5, 0.5, True)
    np.testing.assert_array_equal(split_cells.reshape(-1), cells.reshape(-1))
    np.testing.assert_array_equal(split_counts, counts)
    _hold_histograms(split_counts, split_clouds, split_cells, 5)
    # all of them in one cell: more than the low half of its word holds
    near = (pts * np.float32(1e-3)).astype(np.float32)
    counts, clouds, cells = _grid(near, None, 5, 0.5, True)
    assert (cells == 62).all() and counts[62] == 70000 and clouds[62] == 1 and counts.sum() == 70000 and clouds.sum() == 1


# ---- lengths, non-finite and huge points ------------------------------------------------------------------------------------------------
LENGTHS = [300, 1, 64, 65, 257, 299, 7]


def test_lengths_on_the_host_and_on_the_gpu():
    """Rows at or after the length hold ordinary points: counted by mistake they would show in the histograms."""
    want = random_case(7, 300, 28, True, 0.5)
    pts = want.points
    live = np.arange(300)[None, :] < np.asarray(LENGTHS)[:, None]
    on_host = _grid(pts, LENGTHS)
    for lengths in (torch.tensor(LENGTHS).cuda(), torch.tensor(LENGTHS, dtype=torch.int32).cuda(), torch.tensor(LENGTHS)):
        for a, b in zip(on_host, _grid(pts, lengths)):
            np.testing.assert_array_equal(a, b)
    counts, clouds, cells = on_host
    assert (cells[~live] == -1).all() and (cells[live] >= 0).all() and counts.sum() == sum(LENGTHS)
    np.testing.assert_array_equal(cells[live], _grid(pts)[2][live])
    picked = type(want)(**{k: getattr(want, k)[live.reshape(-1)] for k in ("cell", "d_best", "gap", "bar")})
    _hold_assignment(cells[live], pts[live], picked, 28, 0.5, True, "ragged lengths")
    _hold_histograms(counts, clouds, cells, 28)


def test_device_lengths_are_clamped():
    """0 and -3 behave as 1, P + 5 and 2^30 as P."""
    pts = random_case(7, 300, 28, True, 0.5).points
    got = _grid(pts, torch.tensor([0, -3, 305, 1 << 30, 300, 1, 17]).cuda())
    want = _grid(pts, [1, 1, 300, 300, 300, 1, 17])
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_non_finite_points_are_not_counted_and_huge_ones_are():
    pts = random_set(3, 200, 0.5, 33)
    skipped = np.zeros((3, 200), dtype=bool)
    for row, (i, p, c) in enumerate([(0, 0, 0), (0, 5, 1), (0, 199, 2), (1, 63, 0), (1, 64, 1), (2, 100, 2), (2, 101, 0), (2, 102, 1), (2, 103, 2)]):
        pts[i, p, c] = [np.nan, np.inf, -np.inf][row % 3]
        skipped[i, p] = True
    pts[1, 10] = [np.nan, np.inf, -np.inf]
    skipped[1, 10] = True
    huge = [(0, 7, (1e30, 0, 0)), (1, 8, (-1e30, 1e30, 3e38)), (2, 9, (0.1, -3.4e38, 0.2)), (2, 10, (600.0, 0.0, -700.0))]
    for i, p, v in huge:
        pts[i, p] = v
    for in_sphere in (True, False):
        counts, clouds, cells = _grid(pts, None, 28, 0.5, in_sphere)
        assert (cells[skipped] == -1).all() and (cells[~skipped] >= 0).all()
        assert counts.sum() == 600 - skipped.sum()
        valid = mask_oracle(28, 0.5, in_sphere).reshape(-1)
        assert cells.max() < 28 ** 3 and valid[cells[~skipped]].all()          # the huge ones: a valid cell is all that is asked
        _hold_histograms(counts, clouds, cells, 28)
        ordinary = ~skipped
        for i, p, _ in huge:
            ordinary[i, p] = False
        _hold_assignment(cells[ordinary], pts[ordinary], assign_oracle(pts[ordinary], 28, 0.5, in_sphere), 28, 0.5, in_sphere,
                         f"beside non-finite and huge points, sphere {in_sphere}")


# ---- accumulation, determinism, and nothing else written --------------------------------------------------------------------------------
def test_batches_accumulate_and_calls_repeat():
    from npcd.hip.occupancy import occupancy_grid
    pts = _gpu(random_case(16, 257, 28, True, 0.5).points)
    whole = occupancy_grid(pts, return_cells=True)
    again = occupancy_grid(pts, return_cells=True)
    for a, b in zip(whole, again):
        assert torch.equal(a, b)                                   # the same bits on every call
    out = (torch.zeros(28, 28, 28, dtype=torch.int32, device="cuda"), torch.zeros(28 ** 3, dtype=torch.int32, device="cuda"))
    first = occupancy_grid(pts[:5], out=out)
    assert first[0] is out[0] and first[1] is out[1]
    occupancy_grid(pts[5:], out=out)
    assert torch.equal(out[0], whole[0]) and torch.equal(out[1].view(28, 28, 28), whole[1])
    occupancy_grid(pts, out=out)
    assert torch.equal(out[0], 2 * whole[0]) and torch.equal(out[1].view(28, 28, 28), 2 * whole[1])
    with pytest.raises(ValueError, match="out"):
        occupancy_grid(pts, out=(out[0].long(), out[1]))
    with pytest.raises(ValueError, match="out"):
        occupancy_grid(pts, resolution=5, out=out)


@pytest.mark.parametrize("with_cells", [True, False])
def test_the_entry_point_writes_all_of_cells_and_nothing_else(with_cells):
    """A direct C call on another stream; counts, clouds and cells lie between guard bands in one buffer, cells prefilled."""
    from npcd import hip
    from npcd.hip.occupancy import _device_tables
    want = random_case(7, 300, 28, True, 0.5)
    n, P, R = 7, 300, 28
    lattice, lo, hi = _device_tables(R, 0.5, True, torch.device("cuda", torch.cuda.current_device()))
    pts = _gpu(want.points)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32).cuda()
    guard, sentinel = 256, -77
    buf = torch.full((4 * guard + 2 * R ** 3 + n * P,), sentinel, dtype=torch.int32, device="cuda")
    counts = buf[guard:guard + R ** 3]
    clouds = buf[2 * guard + R ** 3:2 * guard + 2 * R ** 3]
    cells = buf[3 * guard + 2 * R ** 3:3 * guard + 2 * R ** 3 + n * P]
    counts.zero_()
    clouds.zero_()
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        hip.check(hip.lib().npcd_occupancy_grid(hip.ptr(pts), hip.ptr(lengths), hip.ptr(lattice), hip.ptr(lo), hip.ptr(hi), hip.ptr(counts),
                                                hip.ptr(clouds), hip.ptr(cells if with_cells else None), n, P, R, hip.stream_ptr()),
                  "npcd_occupancy_grid")
    stream.synchronize()
    got = buf.cpu().numpy()
    for g in range(4):
        start = g * guard + min(g, 2) * R ** 3 + (n * P if g == 3 else 0)
        assert (got[start:start + guard] == sentinel).all(), g
    want_counts, want_clouds, want_cells = _grid(want.points, LENGTHS)
    np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)
    np.testing.assert_array_equal(clouds.cpu().numpy(), want_clouds)
    if with_cells:
        np.testing.assert_array_equal(cells.cpu().numpy().reshape(n, P), want_cells)          # every word overwritten: -1 or a cell
    else:
        assert (cells.cpu().numpy() == sentinel).all()


def test_offsets_past_2_to_the_31():
    """720 clouds of 2^20 points: the last coordinates lie past element 2^31 of the input.  The last cloud alone gives the same
    cells, and every point is counted."""
    from npcd.hip.occupancy import occupancy_grid
    n, P = 720, 1 << 20
    assert n * P < 1 << 31 < 3 * (n - 1) * P
    g = torch.Generator(device="cuda").manual_seed(5)
    pts = torch.rand((n, P, 3), device="cuda", generator=g).mul_(0.7).sub_(0.35)
    pts[:, :64].mul_(3)          # some of every cloud outside the lattice
    counts, clouds, cells = occupancy_grid(pts, return_cells=True)
    last_counts, last_clouds, last_cells = occupancy_grid(pts[n - 1:], return_cells=True)
    assert torch.equal(cells[n - 1:], last_cells) and int(cells.min()) >= 0
    assert int(counts.sum(dtype=torch.int64)) == n * P and int(clouds.max()) == n
    mask = torch.from_numpy(mask_oracle(28, 0.5, True)).cuda()
    assert not bool(counts[~mask].any()) and bool((last_counts <= counts).all())
    first_counts, _ = occupancy_grid(pts[:1])
    assert torch.equal(torch.bincount(cells[0].long(), minlength=28 ** 3).int().view(28, 28, 28), first_counts)
    assert torch.equal(torch.bincount(cells[n - 1].long(), minlength=28 ** 3).int().view(28, 28, 28), last_counts)


# ---- the metrics ------------------------------------------------------------------------------------------------------------------------
NEW_KEYS = {"jsd", "occupancy_entropy_generated", "occupancy_entropy_reference", "occupied_cells_generated", "occupied_cells_reference"}


def _normalized(c):
    """Normalised on the GPU, as shape_metrics does it, and brought back: the oracle sees the very points that the kernel gets."""
    from npcd.eval import normalize_clouds
    return normalize_clouds(_gpu(c), "bbox").cpu().numpy()


def test_metrics_on_the_metric_sets():
    """Under the precondition of test_occupancy_cpu, asserted here on the points as the GPU normalised them, every point of the two
    sets is decided by more than 4 bars: the kernel's histograms are the oracle's, and the JSD is the oracle's up to the float64
    reduction."""
    from npcd.eval import shape_metrics
    gen, ref, _ = metric_sets()
    on_gpu = [_normalized(c) for c in (gen, ref)]
    want_gen, want_ref = (assign_oracle(c, 28, 1.0, True) for c in on_gpu)
    assert min(float((c.gap / c.bar).min()) for c in (want_gen, want_ref)) > 4          # precondition, asserted
    (gen_counts, gen_clouds), (ref_counts, ref_clouds) = (histograms(c.cell.reshape(-1, 64), 28) for c in (want_gen, want_ref))
    want = jsd_oracle(gen_counts, ref_counts)
    assert abs(want - METRIC_JSD) <= 5e-10
    both = shape_metrics(_gpu(gen), _gpu(ref), normalize="bbox", jsd=True)
    plain = shape_metrics(_gpu(gen), _gpu(ref), normalize="bbox")
    print(f"jsd {both['jsd']:.12f} against {want:.12f}")
    assert set(both) - set(plain) == NEW_KEYS and {k: both[k] for k in plain} == plain          # the earlier keys, bit for bit
    assert abs(both["jsd"] - want) <= 1e-12
    mask = mask_oracle(28, 1.0, True)
    assert abs(both["occupancy_entropy_generated"] - occupancy_entropy_oracle(gen_clouds, 20, mask)) <= 1e-12
    assert abs(both["occupancy_entropy_reference"] - occupancy_entropy_oracle(ref_clouds, 24, mask)) <= 1e-12
    assert (both["occupied_cells_generated"], both["occupied_cells_reference"]) == (int((gen_counts > 0).sum()), int((ref_counts > 0).sum()))
    # with emd as well, and through jensen_shannon_divergence itself
    from npcd.eval import jensen_shannon_divergence
    direct = jensen_shannon_divergence(_gpu(on_gpu[0]), _gpu(on_gpu[1]), extent=1.0)
    assert set(direct) == NEW_KEYS and direct == {k: both[k] for k in NEW_KEYS}
    three = shape_metrics(_gpu(gen), _gpu(ref), normalize="bbox", emd=True, jsd=True)
    assert {k: three[k] for k in both} == both and "mmd_emd" in three


def test_a_set_against_itself_and_against_its_twins():
    from npcd.eval import jsd_from_counts, shape_metrics
    from npcd.hip.occupancy import occupancy_grid
    _, ref, twins = metric_sets()
    same = shape_metrics(_gpu(ref), _gpu(ref), normalize="bbox", jsd=True)
    assert same["jsd"] == 0.0 and same["occupancy_entropy_generated"] == same["occupancy_entropy_reference"]
    near = shape_metrics(_gpu(twins), _gpu(ref), normalize="bbox", jsd=True)
    print(f"twins against the reference: jsd {near['jsd']:.6f}")
    assert 0 < near["jsd"] < 0.05
    twin_points, ref_points = _gpu(_normalized(twins)), _gpu(_normalized(ref))
    a, b = occupancy_grid(twin_points, extent=1.0)[0], occupancy_grid(ref_points, extent=1.0)[0]
    assert near["jsd"] == jsd_from_counts(a, b)
    assert (near["occupied_cells_generated"], near["occupied_cells_reference"]) == (int((a > 0).sum()), int((b > 0).sum()))


def test_lengths_reach_the_metric():
    """The first 40 points of every cloud, given as lengths or cut out: the same dict."""
    from npcd.eval import jensen_shannon_divergence
    gen, ref, _ = (_gpu(_normalized(c)) for c in metric_sets())
    cut = jensen_shannon_divergence(gen[:, :40].contiguous(), ref[:, :33].contiguous(), extent=1.0)
    assert jensen_shannon_divergence(gen, ref, extent=1.0, gen_lengths=[40] * 20, ref_lengths=torch.full((24,), 33).cuda()) == cut


def test_evaluate_shapes_with_jsd():
    from npcd.eval import evaluate_shapes
    from test_gpu_sampler_steps import _tiny_model
    m = _tiny_model()
    reference = _gpu(np.random.default_rng(111).standard_normal((8, 48, 3)).astype(np.float32))
    torch.manual_seed(7)
    a = evaluate_shapes(m, reference, num_samples=6, generate_batch_size=4, sampling_steps=4, eta=0.0, normalize="bbox", jsd=True)
    torch.manual_seed(7)
    b = evaluate_shapes(m, reference, num_samples=6, generate_batch_size=4, sampling_steps=4, eta=0.0, normalize="bbox")
    assert a["jsd_seconds"] > 0 and "jsd_seconds" not in b and not NEW_KEYS & set(b) and NEW_KEYS <= set(a)
    timings = ("generate_seconds", "metric_seconds", "jsd_seconds")
    assert {k: v for k, v in a.items() if k not in timings and k not in NEW_KEYS} == {k: v for k, v in b.items() if k not in timings}
    assert 0 <= a["jsd"] <= 1 and a["occupied_cells_generated"] > 0 and a["occupancy_entropy_reference"] > 0
