"""The field at explicit positions (PointNeRF.query_field, PointNeRF.density_grid) against the CPU oracle -- the neighbour query of
oracle/voxel_grid.py with one position per "ray" and oracle.renderer.shade_points -- and the mesh export on top of it
(npcd.eval.mesh.extract_mesh).

Bars: the set of positions that have a neighbour is the oracle's, exactly.  fp16-operand kernels: sigma and rgb to 2e-3 absolute, the
bar of test_gpu_render.test_shading_matches_reference_golden.  mlp_dtype=torch.float32: sigma to 1e-4 of max(1, |sigma|) and rgb to
2e-5, the bars of test_gpu_render.test_fused_point_level_layers_in_the_fp32_class.  Every comparison prints its figure first."""
import functools

import numpy as np
import pytest
import torch

from oracle import renderer as orr
from oracle import voxel_grid as ovg
from test_isosurface_cpu import read_ply

pytestmark = pytest.mark.gpu

Q_NEAR, Q_FAR, JITTER = 2048, 2048, 0.02


def _params(dir_dim=0):
    p = orr.init_field_params(32, seed=2, dir_dim=dir_dim)
    for name in p:
        if "shape_net.2" in name:
            p[name] = p[name] * 8 + 1.0          # as test_render_in_the_reference_numerics_class: sigma is not flat
    if dir_dim:
        p["channel_net.0.weight"][:, 256:] *= 8.0          # the direction decides the colour by many bars (asserted where it is used)
    return p


def _model(N, use_dir=False):
    from npcd.models.pointnerf import PointNeRF
    m = PointNeRF(1, 32, N, use_dir)
    m.field.load_state_dict(_params(51 if use_dir else 0))
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def scene(N):
    """B = 2 clouds and Q = 4,096 positions per cloud: the cloud's own points, copies of them moved by up to 0.02 per axis (inside
    the query radius of 0.08), and uniform points of the box.  With what the oracle alone says about them, computed once."""
    coords, feats = orr.synthetic_cloud(N, 32, 2, seed=3)
    g = torch.Generator().manual_seed(11 + N)
    copies = coords[:, torch.randint(0, N, (Q_NEAR - N,), generator=g)]
    near = torch.cat((coords, copies + (torch.rand(copies.shape, generator=g) * 2 - 1) * JITTER), dim=1)
    far = torch.rand(2, Q_FAR, 3, generator=g) * 2 - 1
    x = torch.cat((near, far), dim=1).contiguous()
    from npcd.hip.render import DEFAULT_GRID_LEVEL          # the reading of the grid that PointNeRF's own grid follows
    grid = ovg.VoxelGridOracle(**dict(orr.DEFAULT_GRID, grid_level=DEFAULT_GRID_LEVEL))
    grid.set_pointset(coords.numpy(), np.full((2,), N, dtype=np.int32))
    idx = torch.from_numpy(grid.query_dense(x[:, :, None, :].numpy(), 8, 2.0, 1)[0].astype(np.int64)).view(-1, 8)
    valid = idx[:, 0] >= 0
    assert int(valid.sum()) >= 1000 and int((~valid).sum()) >= 1000          # conditions on the inputs, met by the oracle alone
    return coords, feats, x, idx, valid


@functools.lru_cache(maxsize=None)
def oracle_field(N):
    coords, feats, x, idx, valid = scene(N)
    s, c, _ = orr.shade_points(_params(), idx[valid], x.view(-1, 3)[valid], coords, feats)
    sigma, rgb = torch.zeros(x.shape[0] * x.shape[1]), torch.zeros(x.shape[0] * x.shape[1], 3)
    sigma[valid], rgb[valid] = s[:, 0], c
    return sigma.view(2, -1), rgb.view(2, -1, 3)


def _on_gpu(N):
    coords, feats, x, _, valid = scene(N)
    return coords.cuda(), feats.cuda(), x.cuda(), valid.view(2, -1)


@pytest.mark.parametrize("N", [64, 512])
def test_query_field_against_the_oracle(N):
    coords, feats, x, valid = _on_gpu(N)
    want_s, want_c = oracle_field(N)
    assert float(want_s.max()) - float(want_s[valid].min()) > 0.1          # sigma is not flat: it varies by 50 bars or more
    m = _model(N)
    m.renderer.range_guard = "raise"
    for dtype, bar_s, bar_c in ((None, None, 2e-3), (torch.float32, 1e-4, 2e-5)):
        sigma, rgb = m.query_field(coords, feats, x, mlp_dtype=dtype)
        assert sigma.shape == (2, 4096) and rgb.shape == (2, 4096, 3) and sigma.dtype == rgb.dtype == torch.float32
        sigma, rgb = sigma.cpu(), rgb.cpu()
        has = (sigma != 0) | (rgb != 0).any(dim=-1)          # (softplus and the sigmoid are positive where a position was shaded)
        assert torch.equal(has, valid)
        err_s, err_c = (sigma - want_s).abs(), float((rgb - want_c).abs().max())
        rel_s = float((err_s / want_s.abs().clamp_min(1.0)).max())
        print(f"N {N} mlp_dtype {dtype}: max |sigma - oracle| {float(err_s.max()):.3e} (relative to max(1, sigma) {rel_s:.3e}), "
              f"max |rgb - oracle| {err_c:.3e}, sigma in [{float(want_s[valid].min()):.3f}, {float(want_s.max()):.3f}]")
        if dtype is None:
            assert float(err_s.max()) <= 2e-3 and err_c <= bar_c
        else:
            assert rel_s < bar_s and err_c < bar_c
        assert float(sigma[~valid].abs().max()) == 0.0 and float(rgb[~valid].abs().max()) == 0.0


def test_chunks_give_the_same_bits():
    coords, feats, x, _ = _on_gpu(512)
    m = _model(512)
    for dtype in (None, torch.float32):
        whole = m.query_field(coords, feats, x, mlp_dtype=dtype)
        parts = m.query_field(coords, feats, x, mlp_dtype=dtype, chunk=1000)
        assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    with pytest.raises(ValueError):
        m.query_field(coords, feats, x, mlp_dtype=torch.float16)
    with pytest.raises(ValueError):
        m.query_field(coords, feats, x[:1])


def test_view_directions():
    """A field with view directions: ValueError without one; with one direction for all positions, and with one per position, the
    colours are the oracle's heads on [feat | enc(direction)] (oracle.renderer.shade_points gives feat and sigma)."""
    coords, feats, x, valid = _on_gpu(512)
    cpu_coords, cpu_feats, cpu_x, idx, flat_valid = scene(512)
    m = _model(512, use_dir=True)
    with pytest.raises(ValueError, match="view_dir"):
        m.query_field(coords, feats, x)
    with pytest.raises(ValueError, match="view_dir"):
        m.query_field(coords, feats, x, view_dir=torch.ones(2, 7, 3, device="cuda"))
    p = _params(51)
    cut = dict(p)
    cut["channel_net.0.weight"] = p["channel_net.0.weight"][:, :256]          # shade_points knows no directions: feat and sigma from it
    want_s, _, feat = orr.shade_points(cut, idx[flat_valid], cpu_x.view(-1, 3)[flat_valid], cpu_coords, cpu_feats)
    g = torch.Generator().manual_seed(5)
    one = torch.nn.functional.normalize(torch.tensor([0.3, -0.5, 0.8]), dim=0)
    each = torch.nn.functional.normalize(torch.randn(2, 4096, 3, generator=g), dim=-1)
    plain = _model(512).query_field(coords, feats, x)
    wanted = {}
    for name, dirs in (("one direction", one), ("a direction per position", each)):
        per_point = (dirs.expand(2, 4096, 3) if dirs.dim() == 1 else dirs).reshape(-1, 3)[flat_valid]
        want_c = wanted[name] = torch.sigmoid(orr.run_mlp(p, "channel_net", torch.cat((feat, orr.positional_encoding(per_point, 8)), dim=-1)))
        for dtype, bar_s, bar_c in ((None, 2e-3, 2e-3), (torch.float32, 1e-4, 2e-5)):
            sigma, rgb = m.query_field(coords, feats, x, mlp_dtype=dtype, view_dir=dirs.cuda())
            err_s = float(((sigma.cpu().view(-1)[flat_valid] - want_s[:, 0]).abs() / (want_s[:, 0].abs().clamp_min(1.0) if dtype else 1.0)).max())
            err_c = float((rgb.cpu().view(-1, 3)[flat_valid] - want_c).abs().max())
            print(f"{name}, mlp_dtype {dtype}: sigma {err_s:.3e}, rgb {err_c:.3e}")
            assert err_s <= bar_s and err_c <= bar_c
            assert float(rgb.cpu().view(-1, 3)[~flat_valid].abs().max()) == 0.0
    moved = float((wanted["one direction"] - wanted["a direction per position"]).abs().max())
    print(f"the direction moves the oracle's colours by up to {moved:.3e}")
    assert moved > 10 * 2e-3          # a condition on the inputs: a wrong or ignored direction misses every bar above
    # a field without view directions ignores the argument
    ignored = _model(512).query_field(coords, feats, x, view_dir=one.cuda())
    assert torch.equal(ignored[0], plain[0]) and torch.equal(ignored[1], plain[1])


@pytest.mark.parametrize("resolution, bound", [((5, 6, 7), 0.5), (24, None)])
def test_density_grid(resolution, bound):
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma, origin, spacing = m.density_grid(coords, feats, resolution=resolution, bound=bound)
    gz, gy, gx = (resolution,) * 3 if isinstance(resolution, int) else resolution
    b = 1.0 if bound is None else bound
    assert sigma.shape == (2, gz, gy, gx) and sigma.dtype == torch.float32 and sigma.is_contiguous()
    assert origin.tolist() == [-b] * 3
    assert spacing.tolist() == torch.tensor([2 * b / (gx - 1), 2 * b / (gy - 1), 2 * b / (gz - 1)], dtype=torch.float32).tolist()
    lz, ly, lx = (torch.linspace(-b, b, g, device="cuda") for g in (gz, gy, gx))
    Z, Y, X = torch.meshgrid(lz, ly, lx, indexing="ij")
    nodes = torch.stack((X, Y, Z), dim=-1).view(1, -1, 3).expand(2, -1, 3).contiguous()          # x fastest
    want = m.query_field(coords, feats, nodes)[0].view(2, gz, gy, gx)
    assert torch.equal(sigma, want) and int((sigma > 0).sum()) > 0
    parts = m.density_grid(coords, feats, resolution=resolution, bound=bound, chunk=100)[0]
    assert torch.equal(parts, sigma)
    s32 = m.density_grid(coords, feats, resolution=resolution, bound=bound, mlp_dtype=torch.float32)[0]
    assert torch.equal(s32, m.query_field(coords, feats, nodes, mlp_dtype=torch.float32)[0].view(2, gz, gy, gx))
    with pytest.raises(ValueError):
        m.density_grid(coords, feats, resolution=(5, 1, 7))


def test_extract_mesh(tmp_path):
    from npcd.eval.mesh import colors_to_uint8, default_level, extract_mesh, write_ply
    from npcd.hip.isosurface import isosurface
    coords, feats, _, _ = _on_gpu(512)
    m = _model(512)
    sigma, origin, spacing = m.density_grid(coords, feats, resolution=24)
    level = float(sigma[sigma > 0].median())          # a surface exists with untrained weights
    meshes = extract_mesh(m, coords, feats, resolution=24, level=level)
    direct = isosurface(sigma, level, origin, spacing)
    assert len(meshes) == 2
    for b, mesh in enumerate(meshes):
        v, f, c = mesh["vertices"], mesh["faces"], mesh["colors"]
        print(f"cloud {b}: level {level:.4f}, {len(v)} vertices, {len(f)} faces")
        assert len(v) > 20 and len(f) > 20 and c.shape == v.shape
        assert int(f.min()) >= 0 and int(f.max()) < len(v)
        assert float(v.abs().max()) <= 1.0
        assert torch.equal(v, direct[b][0]) and torch.equal(f, direct[b][1])
        want_s, want_c = m.query_field(coords[b:b + 1], feats[b:b + 1], v[None])
        assert torch.equal(c, want_c[0]) and float(c.min()) >= 0 and float(c.max()) <= 1
        write_ply(tmp_path / "mesh.ply", v, f, c)
        xyz, faces, rgb = read_ply(tmp_path / "mesh.ply")
        np.testing.assert_array_equal(xyz, v.cpu().numpy())
        np.testing.assert_array_equal(faces, f.cpu().numpy())
        np.testing.assert_array_equal(rgb, colors_to_uint8(c))
    bare = extract_mesh(m, coords, feats, resolution=24, level=level, colors=False)
    assert all(set(mesh) == {"vertices", "faces"} for mesh in bare) and torch.equal(bare[1]["faces"], meshes[1]["faces"])
    # the default level is the density at which one depth step through the box is half opaque
    assert abs(default_level(m) - np.log(2.0) / (2.0 / 127)) < 1e-9
    assert len(extract_mesh(m, coords, feats, resolution=8, colors=False)) == 2
