"""DiffusionTrainer(dtype="fp32_class") refuses what its fused node cannot train, with a clear message, before it touches the model.
Runs without a GPU."""
import pytest
import torch


def _model(width=256, heads=4):
    from npcd.models.diffusion import DiffusionModel
    return DiffusionModel(3, 8, 16, width, 1, heads, True)


def test_cpu_model_is_refused():
    from npcd.train import DiffusionTrainer
    m = _model()
    before = [p.data_ptr() for p in m.parameters()]
    with pytest.raises(ValueError, match="GPU"):
        DiffusionTrainer(m, dtype="fp32_class")
    assert [p.data_ptr() for p in m.parameters()] == before          # the parameters were not re-homed


def test_unfused_trainer_is_refused():
    from npcd.train import DiffusionTrainer
    with pytest.raises(ValueError, match="fused=True"):
        DiffusionTrainer(_model(), dtype="fp32_class", fused=False)


def test_head_dim_32_is_refused():
    from npcd.models.diffusion import fused
    from npcd.train import DiffusionTrainer
    with pytest.raises(ValueError, match="head dim 32"):
        DiffusionTrainer(_model(256, 8), dtype="fp32_class")
    assert fused.x2_supported(256, 4) is None and fused.x2_supported(1024, 16) is None


def test_unsupported_width_is_refused():
    from npcd.train import DiffusionTrainer
    with pytest.raises(ValueError, match="width 320"):
        DiffusionTrainer(_model(320, 5), dtype="fp32_class")


def test_other_dtype_strings_are_refused():
    from npcd.train import DiffusionTrainer
    with pytest.raises(ValueError, match="fp32_class"):
        DiffusionTrainer(_model(), dtype="fp32")
