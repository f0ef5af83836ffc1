"""CPU checks of the device-side loss scaler option: it refuses to run off the native HIP path (no silent fall-back to the host
bookkeeping), the host path keeps its attributes, and the Python view of the control record matches the header's layout."""
import os
import re

import pytest
import torch

from conftest import ROOT


def _model():
    from npcd.models.diffusion import DiffusionModel
    torch.manual_seed(0)
    return DiffusionModel(3, 8, 16, 64, 1, 2, True)


def test_device_scaler_on_a_cpu_model_raises():
    from npcd.train import DiffusionTrainer
    with pytest.raises(ValueError, match="device_scaler"):
        DiffusionTrainer(_model(), dtype=torch.float16, device_scaler=True)


def test_device_scaler_switch_on_a_cpu_model_raises(monkeypatch):
    from npcd.train import DiffusionTrainer
    monkeypatch.setenv("NPCD_DEVICE_SCALER", "1")
    with pytest.raises(ValueError, match="device_scaler"):
        DiffusionTrainer(_model(), dtype=None)
    monkeypatch.setenv("NPCD_DEVICE_SCALER", "0")
    assert DiffusionTrainer(_model(), dtype=None).comm_stats()["device_scaler"] is False


def test_host_bookkeeping_attributes_unchanged():
    from npcd.train import DiffusionTrainer
    tr = DiffusionTrainer(_model(), dtype=torch.float16)
    assert (tr.loss_scale, tr.iteration, tr.skipped_steps, tr.last_grad_norm) == (65536.0, 0, 0, None)
    tr.loss_scale = 2.0 ** 40
    tr.iteration = 5
    tr.skipped_steps = 2
    assert (tr.loss_scale, tr.iteration, tr.skipped_steps) == (2.0 ** 40, 5, 2)
    assert DiffusionTrainer(_model(), dtype=torch.bfloat16).loss_scale is None


def test_control_record_layout_matches_the_header():
    from npcd.hip import elementwise as ew
    header = open(os.path.join(ROOT, "include", "npcd_hip.h")).read()
    body = re.search(r"typedef struct NpcdScalerCtl \{(.*?)\} NpcdScalerCtl;", header, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for n in names.split(","):
            n = n.strip()
            m = re.fullmatch(r"(\w+)\[(\d+)\]", n)
            fields += [m.group(1)] * int(m.group(2)) if m else [n]
    assert len(fields) == ew.CTL_WORDS == 16
    for name in ("found_inf", "step", "growth_tracker", "skipped", "loss_scale", "inv_scale", "grad_norm", "clip_coef", "bc1", "bc2_sqrt"):
        assert fields.index(name) == getattr(ew, "CTL_" + name.upper()), name
