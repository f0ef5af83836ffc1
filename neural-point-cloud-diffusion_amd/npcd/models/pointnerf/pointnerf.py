"""PointNeRF auto-decoder renderer (reference npcd/models/pointnerf/pointnerf.py) on the HIP kernels."""
import torch
import torch.nn as nn

from ...hip.render import HipVoxelGrid
from ...utils import AttrDict
from .embeddings import Embedding, VariationalEmbedding
from .field import Field
from .renderer import VolumeRenderer


def _get_pointnerf_options() -> AttrDict:
    """The hard-coded option tree of the reference (pointnerf.py:134-194)."""
    return AttrDict(
        model=dict(
            kp=dict(num=512, feat_dim=32),
            embedding=dict(type="VariationalEmbedding", kwargs=dict(gpu=True)),
            voxel_grid=dict(voxel_size=(0.04, 0.04, 0.04), voxel_scale=(2, 2, 2), kernel_size=(3, 3, 3),
                            max_points_per_voxel=4, max_occ_voxels_per_example=5000,
                            ranges=(-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)),
            field=dict(network="MLP", nerf=True,
                       kwargs=dict(feat_freqs=0, dir_freqs=8, channel_layers=[256, 256, 256, 256], shape_layers=[256],
                                   activation="LeakyReLU", layer_norm=False, use_dir=False),
                       aggregator=dict(network="MLP",
                                       kwargs=dict(k=8, r=2, max_shading_pts=50, ray_subsamples=128, n_freqs=10, freq_mult=1,
                                                   out_dim=256, layers=[256, 256, 256, 256], activation="LeakyReLU",
                                                   layer_norm=False))),
            renderer=dict(network="VolumeRenderer",
                          kwargs=dict(depth_resolution=128, disparity_space_sampling=False, white_back=True, cube_scale=1.0,
                                      ray_subsamples=112, ray_limits=None))),
        sizes=dict(default_resolution=128))


class PointNeRF(nn.Module):
    def __init__(self, n_obj: int, feats_dim: int, num_points: int, use_view_dir: bool):
        super().__init__()
        opt = _get_pointnerf_options()
        opt.model.field.kwargs.use_dir = use_view_dir
        opt.model.kp.feat_dim = feats_dim
        opt.model.kp.num = num_points
        self.opt = opt
        self.voxel_grid = HipVoxelGrid(**opt.model.voxel_grid)
        emb_cls = {"VariationalEmbedding": VariationalEmbedding, "Embedding": Embedding}[opt.model.embedding.type]
        self.feats = emb_cls(num_points, feats_dim, n_obj, **opt.model.embedding.kwargs)
        self.coords = Embedding(num_points, 3, n_obj, **opt.model.embedding.kwargs)
        self.coords.freeze(True)
        self.field = Field(feats_dim, self.voxel_grid, opt.model.field.aggregator, **opt.model.field.kwargs,
                           nerf=opt.model.field.nerf)
        self.renderer = VolumeRenderer(self.field, **opt.model.renderer.kwargs)

    def train(self, mode=True):
        super().train(mode)
        self.renderer.randomize_depth_samples = mode
        return self

    @torch.no_grad()
    def set_all_coords(self, coords):
        self.coords.get_emb().weight.copy_(coords.reshape(coords.shape[0], -1))

    def get_all_coords(self):
        w = self.coords.get_emb().weight
        return w.reshape(w.shape[0], self.opt.model.kp.num, 3)

    def get_all_feats(self):
        w = self.feats.get_emb().weight
        F_ = self.opt.model.kp.feat_dim
        if self.opt.model.embedding.type == "VariationalEmbedding":
            return w.reshape(w.shape[0], self.opt.model.kp.num, 2 * F_)[:, :, :F_]
        return w.reshape(w.shape[0], self.opt.model.kp.num, F_)

    def _set_pointset(self, coords):
        # every cloud holds all of its kp.num points (the reference passes that count per example, pointnerf.py:67): the HIP grid
        # takes "no counts" as exactly that, and can then recognise an unchanged cloud from one view to the next
        if coords.shape[1] != self.opt.model.kp.num:
            counts = torch.full((coords.shape[0],), self.opt.model.kp.num, device=coords.device, dtype=torch.int)
            self.voxel_grid.set_pointset(coords.detach(), counts)
        else:
            self.voxel_grid.set_pointset(coords.detach())

    def forward(self, obj_idx, intrinsics, extrinsics, sample_rays: bool, rng=None):
        """reference pointnerf.py:56-105 -> (pred AttrDict, aux dict).  `rng` (tests) replays given random draws:
        eps (feature reparametrisation), ray_perm, jitter, valid_perm (npcd.models.pointnerf.train_path)."""
        rng = rng or {}
        feats = self.feats(idx=obj_idx, eps=rng["eps"]) if "eps" in rng else self.feats(idx=obj_idx)
        coords = self.coords(idx=obj_idx)
        self._set_pointset(coords)
        if hasattr(self.feats, "get_mean_log_var_std"):
            mean, log_var, std = self.feats.get_mean_log_var_std(idx=obj_idx)
            aux = {"coords": coords, "feats": mean, "feats_mean": mean, "feats_log_var": log_var, "feats_std": std}
        else:
            aux = {"coords": coords, "feats": feats}
        pred = self.renderer(coords, feats, extrinsics, intrinsics, resolution=self.opt.sizes.default_resolution,
                             sample=sample_rays, return_channels=True, rng=rng)
        return pred, aux

    def render(self, coords, feats, extrinsics, intrinsics, resolution=128, max_shading_points=None, sample_rays=False, mlp_dtype=None):
        """reference pointnerf.py:107-131.  mlp_dtype (not in the reference): None = the fused fp16-operand shading kernels with their
        range guard (out["shading_status"]); torch.float32 = the reference's numerics class for the field MLPs (the evaluation
        scripts run them in fp32): fp32-class matrix-core per-pair layers + fp32 heads, VolumeRenderer.shade_dtype."""
        agg = self.field.aggregator
        prev, prev_dtype = agg.max_shading_pts, self.renderer.shade_dtype
        if max_shading_points is not None:
            agg.max_shading_pts = max_shading_points
        if mlp_dtype is not None:
            if mlp_dtype != torch.float32 or not self.field.fp32_class_ok():
                raise ValueError("render(mlp_dtype=...): torch.float32 on the published field architecture, or None")
            self.renderer.shade_dtype = mlp_dtype
        try:
            self._set_pointset(coords)
            return self.renderer(coords, feats, extrinsics, intrinsics, resolution, sample_rays)
        finally:
            agg.max_shading_pts, self.renderer.shade_dtype = prev, prev_dtype

    # ---- the field at explicit positions (not in the reference, which reaches it through camera rays only) ---------------------------
    def _field_numerics(self, mlp_dtype, what: str) -> bool:
        """-> shade in the fp32 class?  The conditions of render(mlp_dtype=...)."""
        if mlp_dtype is None:
            return False
        if mlp_dtype != torch.float32 or not self.field.fp32_class_ok():
            raise ValueError(f"{what}(mlp_dtype=...): torch.float32 on the published field architecture, or None")
        return True

    def _shade_positions(self, coords, feats, x, fp32: bool, view_dir, status):
        """One chunk: x [B, q, 3] contiguous -> sigma [B, q], rgb [B, q, 3].  The grid holds `coords` already.  view_dir: None,
        [3] or [B, q, 3]."""
        field, agg = self.field, self.field.aggregator
        B, q = x.shape[:2]
        idx, loc, _, _ = self.voxel_grid.query_dense(agg.k, agg.r, 1, x=x.view(B, q, 1, 3), mode=0, points=coords)
        valid = (idx[..., 0] >= 0).view(B * q)
        nb = idx.view(B * q, agg.k)[valid]                            # compact, row-major over [cloud, position]
        pts = loc.view(B * q, 3)[valid]
        sigma = torch.zeros(B * q, dtype=torch.float32, device=x.device)
        rgb = torch.zeros((B * q, 3), dtype=torch.float32, device=x.device)
        if nb.shape[0]:
            per_point = view_dir is not None and view_dir.dim() == 3
            if fp32:
                point_dir = None
                if view_dir is not None:
                    point_dir = view_dir.reshape(-1, 3)[valid] if per_point else view_dir.expand(nb.shape[0], 3)
                s, c = field.shade_fp32(nb, pts, coords, feats, point_dir)
            else:
                dir_bias = point_ray = None
                if view_dir is not None:          # one bias row per direction; a compact point names its row
                    dir_bias = field.dir_bias(view_dir.reshape(-1, 3)[valid] if per_point else view_dir.view(1, 3))
                    point_ray = (torch.arange(nb.shape[0], dtype=torch.int32, device=x.device) if per_point
                                 else torch.zeros(nb.shape[0], dtype=torch.int32, device=x.device))
                s, c = field.shade(nb, pts, coords, feats, dir_bias, point_ray, status=status)
            sigma[valid], rgb[valid] = s, c
        return sigma.view(B, q), rgb.view(B, q, 3)

    def _view_dir(self, view_dir, B, Q, what: str):
        if not self.field.use_dir:
            return None          # a field without view directions ignores the argument
        if view_dir is None:
            raise ValueError(f"{what}: this field was built with use_view_dir and needs view_dir ([3] or [B, Q, 3], normalised)")
        if tuple(view_dir.shape) not in ((3,), (B, Q, 3)):
            raise ValueError(f"{what}: view_dir must be [3] or [B, Q, 3] = {(B, Q, 3)}; got {tuple(view_dir.shape)}")
        return view_dir.float()

    @torch.no_grad()
    def query_field(self, coords, feats, x, mlp_dtype=None, view_dir=None, chunk: int = 1 << 22):
        """The field at explicit positions: coords [B, N, 3], feats [B, N, F], x [B, Q, 3] -> sigma [B, Q], rgb [B, Q, 3], fp32.

        The path of the renderer's option branches with one position per "ray": the neighbour query of the aggregator (its k, r
        and the voxel grid), the positions that have a neighbour compacted by torch indexing, shaded by the fused fp16-operand
        kernels (mlp_dtype=None; their range guard acts as renderer.range_guard says, except that "promote" raises) or in the
        reference's fp32 class (mlp_dtype=torch.float32, as for render), and scattered into zeros: a position without a neighbour has
        sigma = 0 and rgb = 0, like an empty slot of the renderer.  `chunk` positions per cloud go through the kernels at a time; the
        result does not depend on it.  A field with view directions needs view_dir ([3], or [B, Q, 3] -- then every chunk holds one
        bias row of 256 floats per shaded position), normalised by the caller; the other fields ignore it.  No gradients."""
        if x.dim() != 3 or x.shape[0] != coords.shape[0] or x.shape[2] != 3:
            raise ValueError(f"query_field: x must be [B, Q, 3] with B = {coords.shape[0]}; got {tuple(x.shape)}")
        if chunk < 1:
            raise ValueError(f"query_field: chunk must be positive; got {chunk}")
        B, Q = x.shape[:2]
        fp32 = self._field_numerics(mlp_dtype, "query_field")
        view_dir = self._view_dir(view_dir, B, Q, "query_field")
        x = x.detach().float()
        self._set_pointset(coords)
        sigma = torch.zeros((B, Q), dtype=torch.float32, device=x.device)
        rgb = torch.zeros((B, Q, 3), dtype=torch.float32, device=x.device)
        status = torch.zeros(1, dtype=torch.int32, device=x.device)
        for q0 in range(0, Q, chunk):
            q1 = min(Q, q0 + chunk)
            dirs = view_dir if view_dir is None or view_dir.dim() == 1 else view_dir[:, q0:q1].contiguous()
            sigma[:, q0:q1], rgb[:, q0:q1] = self._shade_positions(coords, feats, x[:, q0:q1].contiguous(), fp32, dirs, status)
        if not fp32:
            self.renderer.check_shading_status(status)
        return sigma, rgb

    @torch.no_grad()
    def density_grid(self, coords, feats, resolution=128, bound=None, mlp_dtype=None, chunk: int = 1 << 22):
        """The density on a lattice: coords [B, N, 3], feats [B, N, F] -> (sigma [B, Gz, Gy, Gx] fp32 contiguous, x fastest,
        origin [3], spacing [3]).

        resolution: G, or (Gz, Gy, Gx).  Along every axis the nodes are torch.linspace(-bound, bound, G); bound defaults to the
        renderer's cube_scale.  sigma equals query_field at the node positions; the colour heads' direction input plays no part in
        the density, so a field with view directions is queried with a fixed one.  origin and spacing are fp32 host tensors in
        (x, y, z) order: origin = -bound, spacing = 2 bound / (G - 1) per axis -- what npcd.hip.isosurface takes.  The positions
        are made `chunk` nodes at a time: a 256^3 lattice never exists as a list."""
        if isinstance(resolution, int):
            resolution = (resolution,) * 3
        gz, gy, gx = (int(g) for g in resolution)
        if min(gz, gy, gx) < 2:
            raise ValueError(f"density_grid: every axis needs at least 2 nodes; got {(gz, gy, gx)}")
        bound = float(self.renderer.cube_scale if bound is None else bound)
        if not bound > 0:
            raise ValueError(f"density_grid: bound must be positive; got {bound}")
        fp32 = self._field_numerics(mlp_dtype, "density_grid")
        B, dev = coords.shape[0], coords.device
        view_dir = torch.tensor([0.0, 0.0, 1.0], device=dev) if self.field.use_dir else None
        lz, ly, lx = (torch.linspace(-bound, bound, g, dtype=torch.float32, device=dev) for g in (gz, gy, gx))
        self._set_pointset(coords)
        Q = gz * gy * gx
        sigma = torch.empty((B, Q), dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for q0 in range(0, Q, chunk):
            node = torch.arange(q0, min(Q, q0 + chunk), device=dev)
            row = node // gx
            x = torch.stack((lx[node - row * gx], ly[row % gy], lz[row // gy]), dim=-1)
            sigma[:, q0:q0 + chunk] = self._shade_positions(coords, feats, x[None].expand(B, -1, 3).contiguous(), fp32, view_dir, status)[0]
        if not fp32:
            self.renderer.check_shading_status(status)
        origin = torch.tensor([-bound] * 3, dtype=torch.float32)
        spacing = torch.tensor([2.0 * bound / (g - 1) for g in (gx, gy, gz)], dtype=torch.float32)
        return sigma.view(B, gz, gy, gx), origin, spacing
