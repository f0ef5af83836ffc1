"""Host-side checks of the fused stage-1 regularisers (csrc/stage1_losses.hip, npcd.hip.losses): no CPU fallback, the switches' defaults,
and the kernels' scratch / LDS budget read from the compiler's output.  No GPU needed."""
import inspect

import pytest
import torch

from test_kernel_resources import _compile


def test_cpu_tensors_raise():
    from npcd.hip.losses import stage1_regularisers
    B, N, F_, k = 1, 8, 4, 2
    coords, feats = torch.zeros(B, N, 3), torch.zeros(B, N, F_, requires_grad=True)
    nb = torch.full((B, N, k), -1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        stage1_regularisers(coords, nb, feats)
    with pytest.raises(RuntimeError, match="GPU"):
        stage1_regularisers(feats_mean=feats, feats_log_var=feats)
    from npcd.losses import NeuralPointCloudKLLoss
    with pytest.raises(RuntimeError, match="GPU"):
        NeuralPointCloudKLLoss(None, 1.0, fused=True)(None, None, {"feats_mean": feats, "feats_log_var": feats}, 0)


def test_fused_path_is_opt_in(monkeypatch):
    """The default stays the torch-operator path the reference fixture pins; the environment variable only speaks for callers that do
    not pass the argument."""
    from npcd.losses import NeuralPointCloudKLLoss, NeuralPointCloudTVLoss, PointNeRFLoss
    from npcd.models import NPCD
    from npcd.train import PointNeRFTrainer
    for cls in (NeuralPointCloudKLLoss, NeuralPointCloudTVLoss):
        assert inspect.signature(cls).parameters["fused"].default is False
        assert cls(None, 1.0).fused is False
    assert inspect.signature(PointNeRFLoss).parameters["fused_regularisers"].default is False
    net = NPCD(n_obj=1, coords_dim=3, feats_dim=4, num_points=8, use_view_dir=False, width=64, layers=1, heads=1, pointnerf_only=True)

    def fused(**kw):
        tr = PointNeRFTrainer(net, **kw)
        on = tr.loss.neural_point_cloud_tv_loss.fused
        assert tr.loss.neural_point_cloud_kl_loss.fused == on
        return on
    monkeypatch.delenv("NPCD_FUSED_STAGE1_LOSSES", raising=False)
    assert not fused() and fused(fused_losses=True) and not fused(fused_losses=False)
    monkeypatch.setenv("NPCD_FUSED_STAGE1_LOSSES", "1")
    assert fused() and not fused(fused_losses=False)
    monkeypatch.setenv("NPCD_FUSED_STAGE1_LOSSES", "0")
    assert not fused()


def test_kernels_use_no_scratch_and_only_dynamic_lds(tmp_path):
    """Three kernels (forward, the one-wave sum of the clouds, backward), none spilling; all LDS is dynamic (sized from N and k by the
    launcher, checked against a CU's 160 KiB by static_assert in the source); 1024-thread workgroups need <= 128 registers."""
    found = _compile("stage1_losses.hip", str(tmp_path / "stage1_losses.s"))
    assert len(found) == 3, sorted(found)
    for name, v in found.items():
        assert v["scratch"] == 0 and v["lds"] == 0 and v["vgpr"] <= 128, (name, v)
