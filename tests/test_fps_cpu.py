"""Farthest point sampling, everything that needs no GPU: the drop-in package, the wrapper's refusals, the host-side queries and
refusals of the C entry point, the kernels' scratch as the compiler reports it, and the dataset helper's padding / batching / cache
file logic with a stand-in for the GPU call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_kernel_resources import _compile


def test_drop_in_package_resolves_to_the_hip_wrapper():
    import pytorch3d
    import pytorch3d.ops
    from pytorch3d.ops import sample_farthest_points
    from npcd.hip import fps
    assert sample_farthest_points is fps.sample_farthest_points
    assert pytorch3d.ops.__all__ == ["sample_farthest_points"]
    assert "srn.py" in pytorch3d.ops.__doc__


def test_cpu_tensors_are_refused():
    from npcd.hip.fps import sample_farthest_points
    with pytest.raises(RuntimeError, match="GPU"):
        sample_farthest_points(torch.zeros(2, 10, 3), K=4)
    with pytest.raises(RuntimeError, match="GPU"):
        sample_farthest_points(torch.zeros(2, 10, 3), lengths=torch.tensor([10, 3]), K=[4, 2], start_idx=[0, 2])


def test_bad_arguments_are_refused_on_the_host():
    from npcd.hip.fps import sample_farthest_points
    with pytest.raises(RuntimeError, match="supports fp32"):
        sample_farthest_points(torch.zeros(2, 10, 3, dtype=torch.float64), K=4)
    with pytest.raises(RuntimeError, match="supports fp32"):
        sample_farthest_points(torch.zeros(2, 10, 3, dtype=torch.float16), K=4)
    with pytest.raises(ValueError, match=r"\[N, P, 3\]"):
        sample_farthest_points(torch.zeros(2, 10, 2), K=4)
    with pytest.raises(ValueError, match=r"\[N, P, 3\]"):
        sample_farthest_points(torch.zeros(10, 3), K=4)
    with pytest.raises(ValueError, match="lengths"):
        sample_farthest_points(torch.zeros(2, 10, 3), lengths=[10, 11], K=4)
    with pytest.raises(ValueError, match="lengths"):
        sample_farthest_points(torch.zeros(2, 10, 3), lengths=torch.tensor([-1, 10]), K=4)
    with pytest.raises(ValueError, match="lengths"):
        sample_farthest_points(torch.zeros(2, 10, 3), lengths=[10], K=4)
    with pytest.raises(ValueError, match="start_idx"):
        sample_farthest_points(torch.zeros(2, 10, 3), K=4, start_idx=[0, 10])
    with pytest.raises(ValueError, match="start_idx"):
        sample_farthest_points(torch.zeros(2, 10, 3), lengths=[10, 5], K=4, start_idx=[0, 5])
    with pytest.raises(ValueError, match="start_idx"):
        sample_farthest_points(torch.zeros(2, 10, 3), K=4, start_idx=[-1, 0])
    with pytest.raises(ValueError, match="not both"):
        sample_farthest_points(torch.zeros(2, 10, 3), K=4, start_idx=[0, 0], random_start_point=True)
    with pytest.raises(ValueError, match="K"):
        sample_farthest_points(torch.zeros(2, 10, 3), K=[4, 4, 4])
    with pytest.raises(ValueError, match="K"):
        sample_farthest_points(torch.zeros(2, 10, 3), K=0)


def test_host_side_queries_and_refusals():
    from npcd import hip
    from npcd.hip import fps
    L = hip.lib()
    resident, largest = L.npcd_fps_resident_points(), L.npcd_fps_max_points()
    assert 1 <= resident <= largest and largest >= 100000, (resident, largest)
    assert (fps.resident_points(), fps.max_points()) == (resident, largest)
    null = ctypes.c_void_p(0)
    unsupported = -2
    assert L.npcd_error_string(unsupported).decode() == "unsupported shape or dtype"
    # refused before any pointer is looked at and before any launch: null pointers, no GPU
    assert L.npcd_fps(null, null, null, null, null, null, 1, largest + 1, 8, null) == unsupported
    assert L.npcd_fps(null, null, null, null, null, null, 0, 100, 8, null) == unsupported
    assert L.npcd_fps(null, null, null, null, null, null, 1, 0, 8, null) == unsupported
    assert L.npcd_fps(null, null, null, null, null, null, 1, 100, 0, null) == unsupported
    assert L.npcd_fps(null, null, null, null, null, null, 1, 100, 8, null) == -1          # a supported shape, but no buffers


@pytest.fixture(scope="module")
def fps_kernels(tmp_path_factory):
    return _compile("fps.hip", str(tmp_path_factory.mktemp("fps_resources") / "fps.s"))


def test_no_kernel_of_fps_uses_scratch(fps_kernels):
    """The resident form and both streaming instantiations: min_dist (and the coordinates) live in registers, none in scratch."""
    assert len(fps_kernels) == 3, sorted(fps_kernels)
    assert all("fps_kernel" in k for k in fps_kernels), sorted(fps_kernels)
    spilling = {k: v["scratch"] for k, v in fps_kernels.items() if v["scratch"] != 0}
    assert not spilling, spilling


def test_fps_kernels_fit_a_1024_thread_workgroup(fps_kernels):
    """16 waves on 4 SIMDs are 4 waves per SIMD: at most 512 / 4 = 128 registers per lane."""
    for k, v in fps_kernels.items():
        assert v["vgpr"] <= 128, (k, v)
        assert v["lds"] == 2 * 16 * 8, (k, v)


def test_fps_source_is_compiled_without_contraction():
    from test_kernel_resources import _build_py
    assert "-ffp-contract=off" in _build_py().SOURCES["fps.hip"]


# ---- the dataset helper, with a stand-in for the GPU call ------------------------------------------------------------------------

class _FirstK:
    """Stand-in sampler: picks 0 .. K-1 of every cloud and records what it was called with."""

    def __init__(self):
        self.calls = []

    def __call__(self, points, lengths=None, K=50):
        self.calls.append((points.clone(), list(lengths), K))
        idx = torch.arange(K)[None].repeat(points.shape[0], 1)
        assert all(n >= K for n in lengths)
        return torch.stack([p[i] for p, i in zip(points, idx)]), idx


def _clouds(sizes, seed=0):
    g = np.random.default_rng(seed)
    return [g.standard_normal((n, 3)).astype(np.float32) for n in sizes], [g.standard_normal((n, 3)).astype(np.float32) for n in sizes]


def test_subsample_clouds_pads_and_batches():
    from npcd.data.pointclouds import subsample_clouds
    sizes = [40, 17, 33, 25, 60]
    clouds, normals = _clouds(sizes)
    stand_in = _FirstK()
    coords, picked, idx = subsample_clouds(clouds, 16, normals, batch=2, sampler=stand_in, device="cpu")
    assert [c[0].shape for c in stand_in.calls] == [(2, 40, 3), (2, 33, 3), (1, 60, 3)]          # padded to the batch's largest cloud
    assert [c[1] for c in stand_in.calls] == [[40, 17], [33, 25], [60]]
    assert all(c[2] == 16 for c in stand_in.calls)
    padded = stand_in.calls[0][0]
    np.testing.assert_array_equal(padded[1, :17].numpy(), clouds[1])
    assert float(padded[1, 17:].abs().max()) == 0.0
    assert coords.shape == (5, 16, 3) and coords.dtype == torch.float32 and idx.shape == (5, 16) and idx.dtype == torch.int64
    for i in range(5):
        np.testing.assert_array_equal(coords[i].numpy(), clouds[i][:16])
        np.testing.assert_array_equal(picked[i].numpy(), normals[i][:16])
    assert subsample_clouds(clouds, 16, None, batch=64, sampler=_FirstK(), device="cpu")[1] is None
    with pytest.raises(ValueError, match="fewer than 20"):
        subsample_clouds(clouds, 20, normals, batch=2, sampler=_FirstK(), device="cpu")
    with pytest.raises(ValueError, match=r"\[P, 3\]"):
        subsample_clouds([np.zeros((5, 2), np.float32)], 2, sampler=_FirstK(), device="cpu")


def test_load_pointcloud_writes_and_rereads_the_cache(tmp_path):
    from npcd.data.pointclouds import load_pointcloud, load_pointclouds
    sizes = [30, 50, 41]
    clouds, normals = _clouds(sizes, seed=1)
    paths = []
    for i, (c, m) in enumerate(zip(clouds, normals)):
        d = tmp_path / f"obj{i}"
        d.mkdir()
        np.savez(d / "pointcloud3.npz", points=c.astype(np.float64), normals=m)          # raw files may hold doubles: read as .float()
        paths.append(str(d))
    stand_in = _FirstK()
    first = load_pointcloud(paths[0], 8, sampler=stand_in, device="cpu")
    assert os.path.isfile(os.path.join(paths[0], "pointcloud3_8.npz")) and len(stand_in.calls) == 1
    with np.load(os.path.join(paths[0], "pointcloud3_8.npz")) as z:
        assert sorted(z.files) == ["normals", "points"]
        np.testing.assert_array_equal(z["points"], clouds[0][:8])
        np.testing.assert_array_equal(z["normals"], normals[0][:8])
    assert first["points"].dtype == torch.float32 and first["points"].shape == (8, 3)
    # the rest in one padded launch; object 0 comes from its cache
    every = load_pointclouds(paths, 8, batch=64, sampler=stand_in, device="cpu")
    assert len(stand_in.calls) == 2 and stand_in.calls[1][1] == [50, 41]
    for i in range(3):
        np.testing.assert_array_equal(every[i]["points"].numpy(), clouds[i][:8])
        np.testing.assert_array_equal(every[i]["normals"].numpy(), normals[i][:8])
    # all cached now: the sampler is not called, another num_points is another file
    again = load_pointclouds(paths, 8, sampler=None, device="cpu")
    assert all(torch.equal(a["points"], b["points"]) and torch.equal(a["normals"], b["normals"]) for a, b in zip(again, every))
    load_pointcloud(paths[1], 4, sampler=stand_in, device="cpu")
    assert os.path.isfile(os.path.join(paths[1], "pointcloud3_4.npz")) and len(stand_in.calls) == 3
