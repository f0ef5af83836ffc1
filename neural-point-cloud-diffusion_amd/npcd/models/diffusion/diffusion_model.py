"""DiffusionModel = DDPM process + transformer denoiser + the two data normalisers
(reference npcd/models/diffusion/diffusion_model.py)."""
import contextlib

import torch
import torch.nn as nn

from .gaussian_diffusion import GaussianDiffusion
from .transformer import NPCDTransformer


class _Normalization(nn.Module):
    """Shared state of the two normalisers: buffers min/max/shift/scale with the reference's shapes
    (reference :16-19, :53-56).  training: data -> model space; eval: model -> data space."""

    def __init__(self, dim, scale_per_axis=False, clip_per_axis=False):
        super().__init__()
        self.dim, self.scale_per_axis, self.clip_per_axis = dim, scale_per_axis, clip_per_axis
        self.register_buffer("min", torch.zeros(dim if clip_per_axis else 1))
        self.register_buffer("max", torch.zeros(dim if clip_per_axis else 1))
        self.register_buffer("shift", torch.zeros(dim))
        self.register_buffer("scale", torch.ones(dim if scale_per_axis else 1))

    def _flat(self, data):
        data = torch.as_tensor(data, device=self.shift.device).detach().float()
        assert data.shape[0] == self.dim
        return data.reshape(self.dim, -1)

    def _set_clip_range(self, data):
        z = (data - self.shift[:, None]) / self.scale[:, None]
        if self.clip_per_axis:
            self.min.copy_(z.min(dim=1).values)
            self.max.copy_(z.max(dim=1).values)
        else:
            self.min.fill_(z.min())
            self.max.fill_(z.max())

    def forward(self, x):
        shift, scale = self.shift[None, :, None], self.scale[None, :, None]
        return (x - shift) / scale if self.training else x * scale + shift


class UnitGaussianNormalization(_Normalization):
    @torch.no_grad()
    def set_from_all_data(self, data):
        d = self._flat(data)
        self.shift.copy_(d.mean(dim=1))
        self.scale.copy_(d.std(dim=1) if self.scale_per_axis else d.std().reshape(1))
        self._set_clip_range(d)


class MinusOneToOneNormalization(_Normalization):
    @torch.no_grad()
    def set_from_all_data(self, data):
        d = self._flat(data)
        lo, hi = d.min(dim=1).values, d.max(dim=1).values
        self.shift.copy_((lo + hi) / 2.0)
        half = (hi - lo) / 2.0
        self.scale.copy_(half if self.scale_per_axis else half.max().reshape(1))
        self._set_clip_range(d)


class DiffusionModel(nn.Module):
    def __init__(self, coords_dim, feats_dim, num_points, width, layers, heads, use_flash_attn):
        super().__init__()
        self.coords_dim, self.feats_dim, self.num_points = coords_dim, feats_dim, num_points
        self.diffusion_process = GaussianDiffusion()
        self.denoiser = NPCDTransformer(coords_dim=coords_dim, feats_dim=feats_dim, width=width, layers=layers,
                                        heads=heads, use_flash_attn=use_flash_attn)
        self.coords_normalization = UnitGaussianNormalization(dim=coords_dim)
        self.feats_normalization = MinusOneToOneNormalization(dim=feats_dim)

    def compute_loss(self, coords, feats, t=None, coords_noise=None, feats_noise=None, want_pointwise=True):
        """Reference :99-106.  t / noise may be injected (parity tests); by default they are drawn on
        the device like the reference does."""
        coords = self.coords_normalization(coords)
        feats = self.feats_normalization(feats)
        if t is None:
            t = torch.randint(0, self.diffusion_process.num_timesteps, size=(coords.shape[0],), device=coords.device)
        return self.diffusion_process.p_losses(self.denoiser, coords, feats, t, coords_noise, feats_noise, want_pointwise=want_pointwise)

    @torch.no_grad()
    def generate(self, num, batch_size=8, progress=True, dtype=None, use_graph=False, sampling_steps=None, eta=None, coords=None, feats=None,
                 keep_coords=None, keep_feats=None, keep=None, resample=None, spacing=None, solver=None):
        """Reference :108-133.  Two options the reference does not have: `dtype` (e.g. torch.bfloat16) runs the denoiser under
        autocast on the MFMA attention kernels -- 6x faster per reverse step than the reference's fp32 sampling, eps within the
        training-time bf16 tolerance; `use_graph` replays each reverse step from a captured HIP graph.

        Scheduled sampling (GaussianDiffusion.p_sample_loop(steps=, eta=, hold=); any of the four arguments selects it, none of them
        leaves today's loop and bits): `sampling_steps` levels of a strided schedule instead of all of them, `eta` in [0, 1] (0: the
        deterministic DDIM step, one launch and no noise; default 1), and ONE of `coords` [num, 3, N] / `feats` [num, F, N] in data
        space (what generate returns, stacked): that tensor is held -- at every level the denoiser sees it forward-noised -- and the
        other one is sampled; it comes back as the caller's values, unclipped, bit for bit.

        Per-point conditioning (p_sample_loop(keep=, resample=); completion, local edits): `keep_coords` / `keep_feats`, bool [num, N],
        mark the points of `coords` / `feats` that are kept; `keep` sets both masks.  A mask needs its tensor.  With at least one mask
        both tensors may be given, and a tensor given without a mask is kept at every point.  The result is where(mask, given,
        sampled): the caller's values at kept points, unclipped, bit for bit (the given values at free points are not read).
        `resample` = r >= 1 performs every transition r times with a re-noise in between, which is what makes the free points follow
        the kept ones (docs/experiments.md); it also works without masks.

        `spacing` / `solver` (p_sample_loop(spacing=, solver=), scheduled sampling too): spacing = "logsnr" places the `sampling_steps`
        levels uniformly in the log signal-to-noise ratio; solver = "dpmpp2m" is the second-order multistep step (DPM-Solver++ 2M),
        deterministic (eta None or 0) and on "logsnr" levels unless `spacing` says otherwise -- the same error as the DDIM step for
        a fraction of the denoiser forwards (docs/experiments.md).  It composes with held and kept tensors, not with resample > 1."""
        assert not self.training, "Model must be in eval mode for generation"
        if keep is not None:
            if keep_coords is not None or keep_feats is not None:
                raise ValueError("generate(keep=) sets both masks: give it alone, or keep_coords= / keep_feats=")
            keep_coords = keep_feats = keep
        masked = keep_coords is not None or keep_feats is not None
        if coords is not None and feats is not None and not masked:
            raise ValueError("generate(coords=, feats=): at most one of the two tensors can be held")
        for name, given, dim in (("coords", coords, self.coords_dim), ("feats", feats, self.feats_dim)):
            if given is not None and tuple(given.shape) != (num, dim, self.num_points):
                raise ValueError(f"generate({name}=...): expected shape {(num, dim, self.num_points)}, got {tuple(given.shape)}")
        for name, given, mask in (("coords", coords, keep_coords), ("feats", feats, keep_feats)):
            if mask is None:
                continue
            if given is None:
                raise ValueError(f"generate(keep_{name}=...) needs {name}=: the values of the kept points")
            if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (num, self.num_points):
                raise ValueError(f"generate(keep_{name}=...): expected a bool tensor of shape {(num, self.num_points)}")
        if resample is not None and (int(resample) != resample or resample < 1):
            raise ValueError(f"generate(resample=...): an integer >= 1 (got {resample!r})")
        device = next(self.parameters()).device
        sizes = [batch_size] * (num // batch_size) + ([num % batch_size] if num % batch_size else [])
        # dtype = "fp32_class": the reference's fp32 sampling with the backbone's Linear layers as split-operand bf16 GEMMs (two bf16 halves
        # per operand, three cross products, fp32 accumulation: 3e-6 relative per product; everything else fp32) -- fused.backbone_forward_x2
        fp32_class = isinstance(dtype, str)
        if fp32_class and dtype != "fp32_class":
            raise ValueError("generate(dtype=...): a torch dtype for autocast, 'fp32_class', or None")
        backbone = getattr(self.denoiser, "backbone", None)
        ctx = torch.autocast(device.type, dtype=dtype) if (dtype is not None and not fp32_class) else contextlib.nullcontext()
        prev_mode = getattr(backbone, "fp32_class", False)
        if backbone is not None:
            backbone.fp32_class = fp32_class
        try:
            return self._generate(sizes, device, ctx, progress, use_graph, sampling_steps, eta, coords, feats, keep_coords, keep_feats, resample,
                                  spacing, solver)
        finally:
            if backbone is not None:
                backbone.fp32_class = prev_mode

    def _generate(self, sizes, device, ctx, progress, use_graph, sampling_steps=None, eta=None, coords=None, feats=None, keep_coords=None,
                  keep_feats=None, resample=None, spacing=None, solver=None):
        coords_out, feats_out = [], []
        masked = keep_coords is not None or keep_feats is not None
        sides = (("coords", coords, keep_coords, self.coords_normalization), ("feats", feats, keep_feats, self.feats_normalization))
        scheduled = (sampling_steps is not None or eta is not None or coords is not None or feats is not None or resample is not None
                     or spacing is not None or solver is not None)
        done = 0
        for bs in sizes:
            c = torch.randn(bs, self.coords_dim, self.num_points, device=device)
            f = torch.randn(bs, self.feats_dim, self.num_points, device=device)
            new = dict(steps=sampling_steps, eta=1.0 if (eta is None and solver is None) else eta) if scheduled else {}
            if resample is not None:
                new["resample"] = resample
            if spacing is not None:
                new["spacing"] = spacing
            if solver is not None:                     # deterministic: eta stays None (or the caller's 0)
                new["solver"] = solver
            given = {}
            for name, full, mask, norm in sides:
                if full is None:
                    continue
                part = full[done:done + bs].to(device=device, dtype=torch.float32)
                # data -> model space, written out: the modules are in eval mode, where their forward is the inverse map
                known = (part - norm.shift[None, :, None]) / norm.scale[None, :, None]
                m = None
                if not masked:
                    new["hold"] = (name, known)
                else:                                  # a tensor given without a mask beside a masked one: every point is kept
                    m = (torch.ones(bs, self.num_points, dtype=torch.bool, device=device) if mask is None
                         else mask[done:done + bs].to(device))
                    new.setdefault("keep", {})[name] = (known, m)
                given[name] = (full[done:done + bs], m)
            with ctx:
                c, f = self.diffusion_process.p_sample_loop(
                    self.denoiser, c, f,
                    coords_clip_range=(self.coords_normalization.min, self.coords_normalization.max),
                    feats_clip_range=(self.feats_normalization.min, self.feats_normalization.max), progress=progress,
                    use_graph=use_graph, **new)
            out = {"coords": self.coords_normalization(c), "feats": self.feats_normalization(f)}
            for name, (part, m) in given.items():      # the caller's own values: the round trip through model space is not exact
                part = part.to(out[name])
                out[name] = part if m is None else torch.where(m[:, None, :], part, out[name])
            coords_out += list(out["coords"].unbind())
            feats_out += list(out["feats"].unbind())
            done += bs
        return coords_out, feats_out
