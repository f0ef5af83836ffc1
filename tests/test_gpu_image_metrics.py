"""The image-metrics kernel (csrc/ssim.hip) and its surfaces npcd.hip.image_metrics, npcd.eval.ssim and evaluate_pointnerf(ssim=True)
against the float64 oracle of tests/test_image_metrics_cpu.py, written from the definition of DESIGN.md 5.10.

Bar: 1e-9 absolute on S at every valid position and on every view's ssim, ssim_channels and mse (relative where mse is not zero).
It is derived, not measured: a float64 window sum of w^2 <= 225 terms in [0, 1] errs by at most about 2^-53 w^2, and dividing by
C2 = 8.1e-4 gives about 1e-10 on S; the bar leaves 10 x over that.  Every comparison prints its worst figure before it asserts."""
import numpy as np
import pytest
import torch

from test_image_metrics_cpu import SHAPES, SIGMAS, WINDOWS, image_metrics_oracle, oracle_case, render_like

pytestmark = pytest.mark.gpu
BAR = 1e-9
W_OF = {"uniform": 7, "gaussian": 11}


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _hold(got, want, what, with_map=True):
    """One call's results against the oracle's, all of them."""
    mse, ssim, channels = got.mse.cpu().numpy(), got.ssim.cpu().numpy(), got.ssim_channels.cpu().numpy()
    assert got.mse.dtype == got.ssim.dtype == got.ssim_channels.dtype == torch.float64
    assert mse.shape == want.mse.shape and ssim.shape == want.ssim.shape and channels.shape == want.channels.shape
    figures = {"ssim": float(np.abs(ssim - want.ssim).max()), "channels": float(np.abs(channels - want.channels).max()),
               "mse": float((np.abs(mse - want.mse) / np.where(want.mse != 0, want.mse, 1.0)).max())}
    if with_map:
        assert got.map.dtype == torch.float64 and tuple(got.map.shape) == want.map.shape
        figures["map"] = float(np.abs(got.map.cpu().numpy() - want.map).max())
    else:
        assert got.map is None
    print(f"{what}: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    for k, v in figures.items():
        assert v <= BAR, (what, k, v)          # NaN fails too


def _pairs(shape, sigma=0.1):
    target, preds = render_like(*shape)
    return preds[sigma], target


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
def test_one_valid_position(window):
    from npcd.hip.image_metrics import image_metrics
    w = W_OF[window]
    pred, target = _pairs((1, 1, w, w))
    got = image_metrics(_gpu(pred), _gpu(target), window=window, return_map=True)
    assert tuple(got.map.shape) == (1, 1, 1, 1)
    _hold(got, image_metrics_oracle(pred, target, window), f"{window} {w} x {w}")


@pytest.mark.parametrize("layout", ["chw", "hwc"])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("window", WINDOWS)
def test_the_small_set_with_its_map(window, sigma, layout):
    from npcd.hip.image_metrics import image_metrics
    pred, target = _pairs(SHAPES[0], sigma)
    x, y = _gpu(pred), _gpu(target)
    if layout == "hwc":
        x, y = x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous()
    _hold(image_metrics(x, y, window=window, layout=layout, return_map=True), oracle_case(SHAPES[0], sigma, window),
          f"{window} sigma {sigma} {layout}")
    _hold(image_metrics(x, y, window=window, layout=layout), oracle_case(SHAPES[0], sigma, window), f"{window} sigma {sigma} {layout}, no map",
          with_map=False)


@pytest.mark.parametrize("axis", ["rows", "columns"])
@pytest.mark.parametrize("window", WINDOWS)
def test_valid_extents_around_the_tile(window, axis):
    """T - 1, T, T + 1, 2 T and 2 T + 1 valid positions along one axis, five along the other."""
    from npcd.hip.image_metrics import image_metrics, tile
    rows, cols = tile()
    w, T = W_OF[window], rows if axis == "rows" else cols
    for extent in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        H, W = (extent + w - 1, w + 4) if axis == "rows" else (w + 4, extent + w - 1)
        pred, target = _pairs((1, 1, H, W))
        got = image_metrics(_gpu(pred), _gpu(target), window=window, return_map=True)
        _hold(got, image_metrics_oracle(pred, target, window), f"{window} {H} x {W}: {extent} valid {axis}")


def test_the_view_size_of_the_workload():
    from npcd.hip.image_metrics import image_metrics
    pred, target = _pairs(SHAPES[1])
    _hold(image_metrics(_gpu(pred), _gpu(target), window="gaussian", return_map=True), oracle_case(SHAPES[1], 0.1, "gaussian"), "5 x 3 x 128 x 128")


def test_other_window_sizes_and_data_ranges():
    """The least and the largest window, and a data range that is not 1."""
    from npcd.hip.image_metrics import image_metrics
    pred, target = _pairs(SHAPES[0])
    for kw in (dict(win_size=3), dict(win_size=15), dict(window="gaussian", sigma=2.0), dict(data_range=2.0)):
        _hold(image_metrics(_gpu(pred), _gpu(target), return_map=True, **kw), image_metrics_oracle(pred, target, **kw), str(kw))


@pytest.mark.parametrize("window", WINDOWS)
def test_a_strided_view_of_the_renderers_channels_is_read_in_place(window):
    """[V, R, 3] inside a larger tensor, unflattened to [V, res, res, 3] as evaluate_pointnerf passes it, against a [V, 3, H, W] target
    seen as hwc: no copy is made on the way (the very storage is handed on), and the bits are those of the contiguous call."""
    from npcd.hip.image_metrics import as_views, image_metrics
    pred, target = _pairs((3, 3, 32, 32))
    buffer = torch.full((2, 5, 32 * 32, 3), 7.0, device="cuda")
    buffer[1, 1:4] = _gpu(pred).permute(0, 2, 3, 1).reshape(3, 32 * 32, 3)
    channels = buffer[1, 1:4]                                        # [3, R, 3], not contiguous with its neighbours
    x, y = channels.unflatten(1, (32, 32)), _gpu(target).permute(0, 2, 3, 1)
    assert not y.is_contiguous() and as_views(x, "hwc").data_ptr() == channels.data_ptr() and as_views(y, "hwc").data_ptr() == y.data_ptr()
    assert as_views(x, "hwc").untyped_storage().data_ptr() == buffer.untyped_storage().data_ptr()
    got = image_metrics(x, y, window=window, layout="hwc", return_map=True)
    plain = image_metrics(_gpu(pred), _gpu(target), window=window, return_map=True)
    for a, b in zip(got, plain):
        assert torch.equal(a, b)
    _hold(got, image_metrics_oracle(pred, target, window), f"{window} strided hwc")
    # leading dimensions are flattened
    five = image_metrics(_gpu(pred)[None], _gpu(target)[None], window=window)
    assert torch.equal(five.ssim, plain.ssim) and torch.equal(five.mse, plain.mse)


# ---- identical images, reproducibility, non-finite pixels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("window", WINDOWS)
def test_identical_images_give_exactly_one(window):
    import npcd.eval
    from npcd.hip.image_metrics import image_metrics
    for shape in SHAPES:
        target = _gpu(render_like(*shape)[0])
        got = image_metrics(target, target.clone(), window=window, return_map=True)
        assert bool((got.ssim == 1.0).all()) and bool((got.ssim_channels == 1.0).all()) and bool((got.map == 1.0).all())
        assert bool((got.mse == 0.0).all())
        assert npcd.eval.ssim(target, target, window=window) == 1.0


def test_eval_ssim_is_the_mean_over_the_views():
    import npcd.eval
    pred, target = _pairs(SHAPES[0])
    for window in WINDOWS:
        got, want = npcd.eval.ssim(_gpu(pred), _gpu(target), window=window), float(oracle_case(SHAPES[0], 0.1, window).ssim.mean())
        print(f"eval.ssim {window}: {got:.12f} against {want:.12f}")
        assert isinstance(got, float) and abs(got - want) <= BAR
    want = float(image_metrics_oracle(pred, target, "uniform", data_range=2.0).ssim.mean())
    assert abs(npcd.eval.ssim(_gpu(pred).permute(0, 2, 3, 1), _gpu(target).permute(0, 2, 3, 1), 2.0, layout="hwc") - want) <= BAR


def test_calls_repeat_and_a_view_does_not_depend_on_the_others():
    from npcd.hip.image_metrics import image_metrics
    pred, target = (_gpu(a) for a in _pairs(SHAPES[1]))
    for window in WINDOWS:
        whole = image_metrics(pred, target, window=window, return_map=True)
        again = image_metrics(pred, target, window=window, return_map=True)
        for a, b in zip(whole, again):
            assert torch.equal(a, b)
        for v in range(pred.shape[0]):
            alone = image_metrics(pred[v:v + 1], target[v:v + 1], window=window, return_map=True)
            for a, b in zip(whole, alone):
                assert torch.equal(a[v:v + 1], b), (window, v)


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
@pytest.mark.parametrize("window", WINDOWS)
def test_a_non_finite_pixel_stays_in_its_view(window, value):
    from npcd.hip.image_metrics import image_metrics
    pred, target = (_gpu(a) for a in _pairs((3, 3, 37, 45)))
    clean = image_metrics(pred, target, window=window)
    for side in ("pred", "target"):
        x, y = pred.clone(), target.clone()
        (x if side == "pred" else y)[1, 2, 20, 3] = value
        got = image_metrics(x, y, window=window)
        assert bool(got.mse[1].isnan()) and bool(got.ssim[1].isnan()) and bool(got.ssim_channels[1, 2].isnan())
        assert torch.equal(got.ssim_channels[1, :2], clean.ssim_channels[1, :2])
        for a, b in zip(got[:3], clean[:3]):
            assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def test_the_entry_point_writes_its_outputs_and_nothing_else():
    """A direct C call on another stream; mse, ssim and the map lie between guard bands in one buffer."""
    from npcd import hip
    from npcd.hip.image_metrics import ssim_window
    shape = SHAPES[0]
    pred, target = (_gpu(a) for a in _pairs(shape))
    V, C, H, W = shape
    taps_host, n = ssim_window("uniform")
    taps, w = torch.from_numpy(taps_host).cuda(), len(taps_host)
    cells = V * C * (H - w + 1) * (W - w + 1)
    guard, sentinel = 64, -77.0
    buf = torch.full((4 * guard + V + V * C + cells,), sentinel, dtype=torch.float64, device="cuda")
    mse = buf[guard:guard + V]
    ssim = buf[2 * guard + V:2 * guard + V + V * C]
    smap = buf[3 * guard + V + V * C:3 * guard + V + V * C + cells]
    workspace = torch.empty(hip.lib().npcd_image_metrics_workspace_bytes(V, C, H, W, w) // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        hip.check(hip.lib().npcd_image_metrics(hip.ptr(pred), hip.ptr(target), V, C, H, W, *pred.stride(), *target.stride(), hip.ptr(taps), w, n,
                                               1.0, hip.ptr(workspace), hip.ptr(mse), hip.ptr(ssim), hip.ptr(smap), hip.stream_ptr()),
                  "npcd_image_metrics")
    stream.synchronize()
    got = buf.cpu().numpy()
    assert (got == sentinel).sum() == 4 * guard
    for start in (0, guard + V, 2 * guard + V + V * C, 3 * guard + V + V * C + cells):
        assert (got[start:start + guard] == sentinel).all(), start
    want = oracle_case(shape, 0.1, "uniform")
    assert np.abs(mse.cpu().numpy() - want.mse).max() <= BAR * want.mse.max() and np.abs(ssim.cpu().numpy().reshape(V, C) - want.channels).max() <= BAR
    assert np.abs(smap.cpu().numpy().reshape(want.map.shape) - want.map).max() <= BAR


# ---- evaluate_pointnerf -----------------------------------------------------------------------------------------------------------------------
class _Recording:
    """The renderer with every batch of rendered channels kept, so that the oracle sees the very images that were measured."""

    def __init__(self, net):
        self.net, self.channels = net, []

    def parameters(self):
        return self.net.parameters()

    def __call__(self, *args, **kw):
        out = self.net(*args, **kw)
        self.channels.append(out[0]["channels"][0].clone())
        return out


@pytest.mark.parametrize("batch", [1, 2])
def test_evaluate_pointnerf_with_ssim(batch):
    """Two objects of three views at resolution 16 on a tiny field, built as test_gpu_render builds its own."""
    from npcd.eval import evaluate_pointnerf, psnr, unflatten_pred
    from npcd.models import NPCD
    from test_gpu_render import _scene
    res, n_obj, n_views = 16, 2, 3
    coords, feats, extr, intr = _scene(res, n_views, 512, 32, seed=3, B=1)
    net = NPCD(n_obj=n_obj, coords_dim=3, feats_dim=32, num_points=512, use_view_dir=False, width=64, layers=1, heads=1, pointnerf_only=True).cuda().eval()
    net.pointnerf.opt.sizes.default_resolution = res
    net.pointnerf.set_all_coords(coords.expand(n_obj, -1, -1).contiguous().cuda())
    with torch.no_grad():
        net.pointnerf.feats.get_emb().weight.view(n_obj, 512, 64)[:, :, :32] = feats.cuda() * torch.tensor([1.0, -0.5], device="cuda").view(2, 1, 1)
        for name, p_ in net.pointnerf.field.named_parameters():
            if "shape_net.2" in name:
                p_.mul_(8).add_(1.0)
    images = torch.from_numpy(render_like(n_views, 3, res, res)[0])[None]                    # [1, V, 3, res, res]
    samples = [{"obj_idx": torch.tensor([i]), "intrinsics": intr, "extrinsics": extr, "images": images} for i in range(n_obj)]

    plain_net = _Recording(net.pointnerf)
    plain = evaluate_pointnerf(plain_net, samples, eval_batch_size=batch, burn_in_samples=1)
    assert set(plain) == {"psnr", "runtime_model_in_msec", "views", "grid_level"} and len(plain["views"]) == n_obj * n_views
    rendered = [unflatten_pred(c) for c in plain_net.channels]                               # batches of [v, 3, res, res]
    per_view = [img for b in rendered for img in b]
    targets = [images[0, v].cuda() for _ in range(n_obj) for v in range(n_views)]
    for r, img, tgt in zip(plain["views"], per_view, targets):
        assert set(r) == {"sample", "view", "psnr", "runtime_model_in_msec"} and r["psnr"] == psnr(img, tgt)          # the floats of today
    assert plain["psnr"] == sum(r["psnr"] for r in plain["views"]) / len(plain["views"])

    for window in WINDOWS:
        with_net = _Recording(net.pointnerf)
        both = evaluate_pointnerf(with_net, samples, eval_batch_size=batch, burn_in_samples=1, ssim=True, ssim_window=window)
        assert set(both) == set(plain) | {"ssim", "ssim_window"} and both["ssim_window"] == window and both["grid_level"] == plain["grid_level"]
        assert [(r["sample"], r["view"]) for r in both["views"]] == [(r["sample"], r["view"]) for r in plain["views"]]
        measured = [img for c in with_net.channels for img in unflatten_pred(c)]
        worst_s = worst_p = 0.0
        for r, img, tgt in zip(both["views"], measured, targets):
            assert set(r) == {"sample", "view", "psnr", "ssim", "runtime_model_in_msec"}
            want = image_metrics_oracle(img[None].cpu().numpy(), tgt[None].cpu().numpy(), window)
            worst_s, worst_p = max(worst_s, abs(r["ssim"] - float(want.ssim[0]))), max(worst_p, abs(r["psnr"] - psnr(img, tgt)))
        print(f"batch {batch} {window}: ssim within {worst_s:.3g} of the oracle, psnr within {worst_p:.3g} dB of psnr(); "
              f"ssim {both['ssim']:.6f}, psnr {both['psnr']:.4f}")
        assert worst_s <= BAR and worst_p <= 1e-9
        assert both["ssim"] == sum(r["ssim"] for r in both["views"]) / len(both["views"])
        timed = [r for r in both["views"] if r["runtime_model_in_msec"] == r["runtime_model_in_msec"]]
        assert len(timed) == (n_views if batch == 1 else 0) and all(r["sample"] >= 1 for r in timed)
