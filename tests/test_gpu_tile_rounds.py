"""The matrix-core kernels of the PointNeRF path where a workgroup takes SEVERAL tiles.

Every one of them launches a capped grid and lets a workgroup walk the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (the shade pair
kernel: by ticket).  That is the only regime of a 128^2 view or a training step, and the other kernel-level tests stay under it: their
shapes give every workgroup at most one tile.  What can be wrong only from the second tile on -- LDS rows left by the previous tile,
the barriers that close a tile, registers carried across tiles (the dW / db accumulators, the indices and gathered rows requested one
tile ahead, the restarted weight ring), the dealing of tiles, a ragged last tile in a round other workgroups have left -- is checked
here with three instruments:

  1. chunk identity, bit for bit: a tile's arithmetic reads only its own rows, so the whole list in one call must give the same bits
     as the list cut at tile boundaries into chunks small enough that every workgroup takes one tile (the regime the other tests
     hold to float64);
  2. the project's reference bars (float64 / same-rounding restatements) on the whole-list result;
  3. for dW / db, the only outputs that sum across tiles: an elementwise bound on the whole-list result against the float64 sum of
     the chunk results -- same operand bits, only the order of the fp32 additions differs:
         |dW - sum dW_chunk| <= (D_full + D_chunk) 2^-23 S,   S = |dZ|^T |A| in float64,
     D = the longest chain of fp32 additions a term passes through: (rows per tile) x (1 matrix product per fragment pair in bf16
     mode, 3 in the fp32 class) x (most tiles of a workgroup) + (slabs / 8 + 4) for the slab sum; for db (rows per tile / 16) x (most
     tiles) + 16 + (slabs / 8 + 4), S_b = sum |dZ|.  One corrupted 128-row tile of ~600 moves an element by ~1e4 x 2^-23 S; a
     whole-tensor rel-L2 bar would see that only by luck.
"""
import copy
import ctypes
import math

import pytest
import torch

from oracle import renderer as orr
from test_gpu_render import shade_form  # noqa: F401  (fixture: the forms of the shading kernels)
from test_gpu_train_render import (PAIR_NAMES, bf16_backward_restatement, bf16_forward_vs_restatement, pair_case, pair_rel,
                                   x2_backward_restatement, x2_float64_network, x2_forward_vs_float64)

pytestmark = pytest.mark.gpu

BF16, X2 = 0, 1                                            # `precision` of the npcd_pair_mlp_* entry points
FWD_CAP = {BF16: 512, X2: 256}                              # grid caps of pair_mlp_fwd_kernel (16-point tiles)
BWD_CAP = 256                                               # ... of pair_mlp_bwd_kernel
BWD_ROWS = {BF16: 128, X2: 64}                              # pair rows per tile of pair_mlp_bwd_kernel
BWD_PRODUCTS = {BF16: 1, X2: 3}                             # matrix products per fragment pair
GRAD_BAR = {BF16: 2e-3, X2: 1e-4}                           # rel-L2 of every gradient against the restatement from the stored activations
EPS = 2.0 ** -23


def ceil_div(a, b):
    return -(-a // b)


# --------------------------------------------------------------------------------------------------------------------------------
# the per-pair MLP of the training path: raw calls
# --------------------------------------------------------------------------------------------------------------------------------
def pair_forward(cs, precision, wpack=None, lo=0, hi=None):
    """npcd_pair_mlp_fwd on the points [lo, hi) of the case (`off` rebased) -> pair_mlp_forward_raw's tuple"""
    from npcd.hip import render as hr
    hi = cs.P if hi is None else hi
    q0 = int(cs.off[lo])
    q1 = int(cs.off[hi]) if hi < cs.P else cs.Q
    with torch.no_grad():
        return hr.pair_mlp_forward_raw(cs.feat, cs.weights, cs.biases, cs.nb[lo:hi], cs.pts[lo:hi], cs.pos, cs.off[lo:hi] - q0, q1 - q0,
                                       precision, wpack=wpack)


def pair_backward_rows(cs, precision, raw, lo=0, hi=None, guard=3.0):
    """npcd_pair_mlp_bwd on the pair rows [lo, hi) of a whole-list forward `raw` -> (dfeat [rows, F], dact [2, planes, rows, 256] as it
    stands after the call: plane 0 = dA_0, plane 1 = dA_1, [dW_l], [db_l]).  The entry point derives the plane strides from n_pairs:
    the rows of x0 / acts are copied into contiguous buffers.  The per-row outputs start from `guard`, so that a row the kernel does not
    write differs between two calls with different guards."""
    from npcd.hip import check, lib, ptr, stream_ptr
    L = lib()
    _, wpack, x0, acts, wn = raw
    hi = cs.Q if hi is None else hi
    Q, F_ = hi - lo, cs.F
    x0c, actc = x0[..., lo:hi, :].contiguous(), acts[..., lo:hi, :].contiguous()
    dW = [torch.empty((256, F_ + 63 if l == 0 else 256), dtype=torch.float32, device="cuda") for l in range(4)]
    db = [torch.empty(256, dtype=torch.float32, device="cuda") for _ in range(4)]
    dact = torch.full((2, 2 if precision == X2 else 1, Q, 256), guard, dtype=torch.bfloat16, device="cuda")
    dfeat = torch.full((Q, F_), guard, dtype=torch.float32, device="cuda")
    part = torch.empty(L.npcd_pair_mlp_bwd_workspace_floats(F_, Q, precision), dtype=torch.float32, device="cuda")
    dWp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in dW])
    dbp = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in db])
    check(L.npcd_pair_mlp_bwd(ptr(wpack), F_, precision, ptr(cs.gout), ptr(cs.owner[lo:hi]), ptr(wn[lo:hi]), ptr(x0c), ptr(actc), Q, ptr(dact),
                              ptr(dfeat), ptr(part), dWp, dbp, stream_ptr()), "npcd_pair_mlp_bwd")
    return dfeat, dact, dW, db


def forward_checks(cs, precision, raw):
    """instrument 2, forward: the helpers' bars -> (worst figure / bar, layer inputs for the backward restatement)"""
    if precision == X2:
        G64, x0, _ = x2_float64_network(cs)
        return x2_forward_vs_float64(cs, raw, G64, x0)
    return bf16_forward_vs_restatement(cs, raw)


def backward_restatement(cs, precision, raw, layer_in):
    return (x2_backward_restatement if precision == X2 else bf16_backward_restatement)(cs, raw, layer_in)


def gradient_figures(cs, precision, emu, dfeat, dW, db):
    """instrument 2, backward: every gradient against the restatement from the stored activations (the feature rows through the same
    scatter, summed in float64) -> (worst rel-L2 / bar, {name: rel-L2}); the caller prints its figures, then asserts the ratio < 1"""
    tab = torch.zeros(cs.Nt, cs.F, device="cuda", dtype=torch.float64).index_add_(0, cs.flat, dfeat.double())
    got = [tab] + [t for pair in zip(dW, db) for t in pair]
    errs = {n: pair_rel(a, emu[n]) for n, a in zip(PAIR_NAMES, got)}
    return max(errs.values()) / GRAD_BAR[precision], errs


def lists_from_counts(cnt, k, Nt, gen):
    """[P, k] int64 neighbour lists with cnt[p] valid entries first, built without a loop over the points"""
    P = cnt.numel()
    nb = torch.randint(0, Nt, (P, k), generator=gen)
    nb[torch.arange(k)[None, :] >= cnt[:, None]] = -1
    return nb


# --------------------------------------------------------------------------------------------------------------------------------
# A. the per-pair MLP over several tiles per workgroup
# --------------------------------------------------------------------------------------------------------------------------------
A_POINTS, A_K, A_NT = 16981, 8, 300                        # 1062 forward tiles, the last one of 5 points


def a_counts(gen):
    """neighbour counts uniform in 1..8 with constructed tiles: full (16 x 8 = 128 rows), then a sparse one on the SAME workgroup
    (16 x 1 = 16 rows, one 32-row block: rows 16.. of the LDS tile still hold the full tile's activations), then a full one again --
    on workgroup 5 of the 512-workgroup grid and on workgroup 7 of the 256-workgroup grid"""
    cnt = torch.randint(1, A_K + 1, (A_POINTS,), generator=gen)
    triples = {}
    for first, cap in ((5, 512), (7, 256)):
        triples[cap] = (first, first + cap, first + 2 * cap)
        for t, c in zip(triples[cap], (8, 1, 8)):
            cnt[16 * t:16 * t + 16] = c
    return cnt, triples


@pytest.fixture(scope="module")
def a_lists():
    gen = torch.Generator().manual_seed(20)
    cnt, triples = a_counts(gen)
    return cnt, triples, lists_from_counts(cnt, A_K, A_NT, gen)


@pytest.mark.parametrize("precision", [BF16, X2], ids=["bf16", "x2"])
@pytest.mark.parametrize("F_", [32, 128])
def test_pair_mlp_over_several_tiles_per_workgroup(F_, precision, a_lists):
    """npcd_pair_mlp_fwd / npcd_pair_mlp_bwd on 16981 points (1062 forward tiles: three per workgroup on 38 workgroups of the 512, four
    or five on each of the 256 of the fp32 class; > 65536 pair rows: two or three 128-row backward tiles per workgroup, four or five
    64-row ones), full / sparse / full tiles in a row on one workgroup, a partial last tile.
    Forward: G, x0, the four activation planes and wn are the bits of the chunked calls (4096 / 2048 points: one tile per workgroup)
    and hold the helpers' bars.  Backward: the dfeat rows and both planes of the dact workspace are the bits of the chunked calls
    (200 tiles each); dW_l / db_l hold the elementwise accumulation bound of the module docstring and the helpers' rel-L2 bars; a
    second call gives the same bits.
    The bound assumes a relative error <= 2^-23 per fp32 addition of the matrix instruction's accumulation.  It held as stated, so no
    reference-against-reference value replaced D: worst |error| / bar measured 1.5e-3 for dW (D = 577 in bf16 mode, 1217 in the fp32
    class) and 1.1e-3 for db (D = 129 / 121), i.e. an order error of ~0.9 x 2^-23 S."""
    cnt, triples, nb = a_lists
    torch.manual_seed(100 + F_ + precision)
    cs = pair_case(nb, F_, A_NT)
    cap = FWD_CAP[precision]
    tiles = ceil_div(cs.P, 16)
    # ---- premises
    assert tiles > 2 * cap and cs.P % 16 == 5
    assert cs.Q > 65536 and cs.Q % 128 != 0
    for t, c in zip(triples[cap], (8, 1, 8)):
        assert t % cap == triples[cap][0] and t < tiles - 1 and bool((cs.c[16 * t:16 * t + 16] == c).all())
    btiles = ceil_div(cs.Q, BWD_ROWS[precision])
    bmax = ceil_div(btiles, BWD_CAP)
    if precision == BF16:
        assert btiles > 2 * BWD_CAP and bmax == 3                    # some workgroups take three 128-row tiles
    else:
        assert btiles // BWD_CAP == 4 and bmax == 5                  # every workgroup takes four or five 64-row tiles
    # ---- forward: whole list against chunks of one tile per workgroup
    raw = pair_forward(cs, precision)
    G, wpack, x0, acts, wn = raw
    step = {BF16: 4096, X2: 2048}[precision]
    assert ceil_div(step, 16) <= cap and step % 16 == 0
    for lo in range(0, cs.P, step):
        hi = min(lo + step, cs.P)
        q0, q1 = int(cs.off[lo]), int(cs.off[hi]) if hi < cs.P else cs.Q
        Gc, _, x0c, actc, wnc = pair_forward(cs, precision, wpack, lo, hi)
        assert torch.equal(Gc, G[lo:hi]), ("G", lo)
        assert torch.equal(x0c, x0[..., q0:q1, :]), ("x0", lo)
        assert torch.equal(actc, acts[..., q0:q1, :]), ("acts", lo)
        assert torch.equal(wnc, wn[q0:q1]), ("wn", lo)
    worst_f, layer_in = forward_checks(cs, precision, raw)
    # ---- backward: whole list against chunks of 200 tiles
    dfeat, dact, dW, db = pair_backward_rows(cs, precision, raw, guard=3.0)
    rows = BWD_ROWS[precision] * 200
    sumW = [torch.zeros_like(t, dtype=torch.float64) for t in dW]
    sumb = [torch.zeros_like(t, dtype=torch.float64) for t in db]
    chunk_slabs = 0
    for lo in range(0, cs.Q, rows):
        hi = min(lo + rows, cs.Q)
        dfc, dac, dWc, dbc = pair_backward_rows(cs, precision, raw, lo, hi, guard=5.0)
        assert torch.equal(dfc, dfeat[lo:hi]), ("dfeat", lo)
        assert torch.equal(dac, dact[:, :, lo:hi]), ("dact", lo)
        for l in range(4):
            sumW[l] += dWc[l].double()
            sumb[l] += dbc[l].double()
        chunk_slabs = max(chunk_slabs, ceil_div(hi - lo, BWD_ROWS[precision]))
    assert chunk_slabs <= BWD_CAP
    emu, dZs = backward_restatement(cs, precision, raw, layer_in)
    worst_g, errs = gradient_figures(cs, precision, emu, dfeat, dW, db)
    # ---- the accumulation bound
    R, m = BWD_ROWS[precision], BWD_PRODUCTS[precision]
    slabs = min(btiles, BWD_CAP)
    D_w = (R * m * bmax + slabs / 8 + 4) + (R * m * 1 + chunk_slabs / 8 + 4)
    D_b = (R / 16 * bmax + 16 + slabs / 8 + 4) + (R / 16 * 1 + 16 + chunk_slabs / 8 + 4)
    worst_w = worst_b = 0.0
    exact = True                                                     # an element without any term is the same in both
    for l in range(4):
        S = dZs[l].double().abs().t() @ layer_in[l].double().abs()
        err = (dW[l].double() - sumW[l]).abs()
        exact = exact and bool((err[S == 0] == 0).all())
        worst_w = max(worst_w, float((err / (D_w * EPS * S).clamp_min(1e-300)).max()))
        Sb = dZs[l].double().abs().sum(0)
        errb = (db[l].double() - sumb[l]).abs()
        exact = exact and bool((errb[Sb == 0] == 0).all())
        worst_b = max(worst_b, float((errb / (D_b * EPS * Sb).clamp_min(1e-300)).max()))
    print(f"pair MLP [F={F_}, precision {precision}]: {tiles} forward tiles on {cap} workgroups ({ceil_div(tiles, cap)} per workgroup), {cs.Q} pair "
          f"rows = {btiles} backward tiles on {slabs} ({bmax} per workgroup); forward / bar {worst_f:.3f}, gradients / bar {worst_g:.3f}, "
          f"dW order error / bar {worst_w:.2e} (D = {D_w:.0f}), db {worst_b:.2e} (D = {D_b:.0f})")
    assert worst_w <= 1.0 and worst_b <= 1.0 and exact, (worst_w, worst_b, exact)
    assert worst_g < 1.0, errs
    # ---- a second whole call: the same bits
    df2, da2, dW2, db2 = pair_backward_rows(cs, precision, raw, guard=3.0)
    assert torch.equal(df2, dfeat) and torch.equal(da2, dact)
    assert all(torch.equal(a, b) for a, b in zip(dW + db, dW2 + db2))


# --------------------------------------------------------------------------------------------------------------------------------
# B. small lists and the paths of the slab sum
# --------------------------------------------------------------------------------------------------------------------------------
def counts_for_pairs(Q):
    """Q pairs on ceil(Q / 8) points: eight neighbours each, the rest on the last one"""
    P = ceil_div(Q, 8)
    cnt = torch.full((P,), 8, dtype=torch.long)
    cnt[-1] = Q - 8 * (P - 1)
    return cnt


B_CASES = [("one pair", lambda R: torch.ones(1, dtype=torch.long), None),
           ("17 points of one pair", lambda R: torch.ones(17, dtype=torch.long), None),
           ("128 pairs", lambda R: counts_for_pairs(128), None),
           ("129 pairs", lambda R: counts_for_pairs(129), None)]
B_CASES += [(f"{n} slabs", (lambda n: lambda R: counts_for_pairs(R * (n - 1) + 37))(n), n) for n in (2, 4, 5, 8, 9, 13)]


@pytest.mark.parametrize("precision", [BF16, X2], ids=["bf16", "x2"])
@pytest.mark.parametrize("case", B_CASES, ids=[c[0].replace(" ", "-") for c in B_CASES])
def test_pair_mlp_small_lists_and_slab_sum_paths(case, precision):
    """The list sizes a sparse training step produces -- one pair, 17 pairs under one 32-row block, exactly one 128-row tile, one tile
    + 1 -- and the slab counts at which pair_slab_sum_kernel takes another path (1-4 slabs: the first add of each wave only; 5-8:
    one pass of the two-chain loop or its tail; >= 9: several): forward and backward hold the helpers' bars, a second call gives the
    same bits."""
    from npcd.hip import lib
    name, counts, want_slabs = case
    F_, k, Nt = 32, 8, 300
    gen = torch.Generator().manual_seed(31 + len(name))
    cnt = counts(BWD_ROWS[precision])
    torch.manual_seed(7 + precision)
    cs = pair_case(lists_from_counts(cnt, k, Nt, gen), F_, Nt)
    assert cs.Q == int(cnt.sum())
    slabs = lib().npcd_pair_mlp_bwd_slabs(cs.Q, precision)
    assert slabs == ceil_div(cs.Q, BWD_ROWS[precision]) and (want_slabs is None or slabs == want_slabs)
    raw = pair_forward(cs, precision)
    worst_f, layer_in = forward_checks(cs, precision, raw)
    dfeat, dact, dW, db = pair_backward_rows(cs, precision, raw, guard=3.0)
    emu, _ = backward_restatement(cs, precision, raw, layer_in)
    worst_g, errs = gradient_figures(cs, precision, emu, dfeat, dW, db)
    print(f"pair MLP [{name}, precision {precision}]: Q = {cs.Q}, {slabs} slabs, one tile per workgroup; forward / bar {worst_f:.3f}, "
          f"gradients / bar {worst_g:.3f}")
    assert worst_g < 1.0, errs
    raw2 = pair_forward(cs, precision, raw[1])
    assert all(torch.equal(a, b) for a, b in zip(raw, raw2))
    df2, da2, dW2, db2 = pair_backward_rows(cs, precision, raw, guard=3.0)
    assert torch.equal(df2, dfeat) and torch.equal(da2, dact)
    assert all(torch.equal(a, b) for a, b in zip(dW + db, dW2 + db2))


@pytest.mark.parametrize("precision", [BF16, X2], ids=["bf16", "x2"])
def test_pair_mlp_forward_without_any_pair(precision):
    """40 points without a neighbour (Q = 0): G is exactly zero and nothing but G is written (guard values before and behind G and
    in the buffers of the saved rows)."""
    from npcd.hip import check, lib, ptr, stream_ptr
    from npcd.hip import render as hr
    F_, k, Nt, P = 32, 8, 300, 40
    torch.manual_seed(3)
    cs = pair_case(torch.full((P, k), -1, dtype=torch.long), F_, Nt)
    assert cs.Q == 0
    wpack = hr.pair_mlp_pack(cs.weights, cs.biases, F_, precision, "cuda")
    guard = 7.5
    buf = torch.full(((P + 2) * 256,), guard, dtype=torch.float32, device="cuda")
    G = buf[256:(P + 1) * 256].view(P, 256)
    planes = 2 if precision == X2 else 1
    x0 = torch.full((planes, 1, F_ + 64), guard, dtype=torch.bfloat16, device="cuda")
    acts = torch.full((4, planes, 1, 256), guard, dtype=torch.bfloat16, device="cuda")
    wn = torch.full((1,), guard, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        check(lib().npcd_pair_mlp_fwd(ptr(wpack), F_, precision, ptr(cs.nb), ptr(cs.pts), ptr(cs.pos), ptr(cs.feat.detach()), ptr(cs.off), P, k, 0,
                                      ptr(x0), ptr(acts), ptr(wn), ptr(G), stream_ptr()), "npcd_pair_mlp_fwd")
    assert float(G.abs().max()) == 0.0
    assert bool((buf[:256] == guard).all()) and bool((buf[(P + 1) * 256:] == guard).all())
    assert bool((x0 == guard).all()) and bool((acts == guard).all()) and bool((wn == guard).all())
    print(f"pair MLP forward without a pair [precision {precision}]: {ceil_div(P, 16)} tiles, one per workgroup; G == 0, guards intact")


# --------------------------------------------------------------------------------------------------------------------------------
# C. the forward kernels of the fp32 class (csrc/points_x2.hip)
# --------------------------------------------------------------------------------------------------------------------------------
def _field(F_, seed, use_dir=False, scale=None):
    from npcd.models.pointnerf import PointNeRF
    p = orr.init_field_params(F_, seed=seed, dir_dim=51 if use_dir else 0)
    if scale is not None:
        for kname in p:
            if kname.endswith("weight"):
                p[kname] = p[kname] * scale
    m = PointNeRF(1, F_, 64, use_dir)
    m.field.load_state_dict(p)
    return m.cuda().eval().field


@pytest.mark.parametrize("F_", [32, 128])
def test_pairs_x2_over_several_tiles_per_workgroup(F_):
    """pairs_x2_kernel on 32859 points = 4108 eight-point tiles on 2048 workgroups (twelve take three): the neighbour indices and
    the gathered rows of a tile are requested while the previous tile of the workgroup is computed.  Holes anywhere in a row; on
    workgroup 5 a full tile (64 pairs), then a tile without any neighbour (nblk = 0, its prefetched indices all -1), then a full one.
    Chunks of 8192 points (one tile per workgroup) give the same bits; the whole result to 3e-5 rel-L2 of a float64 restatement and
    1e-5 of the training kernel of the same numerics class; rows of neighbour-less points exactly zero."""
    from npcd.hip import render as hr
    P, k, Ntab, cap = 2 * 16384 + 8 * 11 + 3, 8, 512, 2048
    tiles = ceil_div(P, 8)
    triple = (5, 5 + cap, 5 + 2 * cap)
    assert tiles == 4108 and tiles > 2 * cap and triple[2] < tiles - 1 and all(t % cap == 5 for t in triple)
    gen = torch.Generator().manual_seed(40 + F_)
    field = _field(F_, 2)
    nb = torch.randint(0, Ntab, (P, k), generator=gen, dtype=torch.int32)
    nb[torch.rand(P, k, generator=gen) < 0.35] = -1
    for t, full in zip(triple, (True, False, True)):
        nb[8 * t:8 * t + 8] = torch.randint(0, Ntab, (8, k), generator=gen, dtype=torch.int32) if full else -1
    assert all(bool(((nb[8 * t:8 * t + 8] >= 0) == full).all()) for t, full in zip(triple, (True, False, True)))
    nb = nb.cuda()
    pts = (torch.rand(P, 3, generator=gen) - 0.5).cuda()
    kp = (torch.rand(Ntab, 3, generator=gen) - 0.5).cuda()
    kf = torch.randn(Ntab, F_, generator=gen).cuda()
    wp = hr.pairs_x2_pack(field.state_dict(), F_, "cuda")
    G = hr.pairs_x2(wp, F_, nb, pts, kp, kf)
    assert bool(torch.isfinite(G).all())
    step = 8192
    assert ceil_div(step, 8) <= cap
    for lo in range(0, P, step):
        hi = min(lo + step, P)
        assert torch.equal(hr.pairs_x2(wp, F_, nb[lo:hi], pts[lo:hi], kp, kf), G[lo:hi]), lo
    # float64 restatement (aggregators/mlp.py:62-125)
    lf = [field.aggregator.local_field[i] for i in (0, 2, 4, 6)]
    valid = nb >= 0
    idx = nb.clamp_min(0).long()
    with torch.no_grad():
        rel = (pts[:, None, :] - kp[idx]).double()
        w = 1.0 / (rel.norm(dim=-1) + 1e-5) * valid
        freqs = (2.0 ** torch.arange(10, device="cuda", dtype=torch.float64)) * math.pi
        ang = rel[..., None] * freqs                                            # [P, k, 3, 10]
        enc = torch.cat((torch.sin(ang), torch.cos(ang)), dim=-1).flatten(-2)   # per coordinate: sin f0..9, cos f0..9
        x = torch.cat((kf[idx].double(), rel, enc), dim=-1)
        for l in lf:
            x = torch.nn.functional.leaky_relu(torch.nn.functional.linear(x, l.weight.double(), l.bias.double()), 0.01)
        wn = w / w.sum(dim=1, keepdim=True).clamp_min(1e-300)
        want = (x * wn[..., None]).sum(dim=1) * (valid.any(dim=1, keepdim=True))
        e64 = float((G.double() - want).norm() / want.norm())
        # the training kernel's forward on the same lists (valid entries first, as it expects)
        nbs = torch.gather(nb, 1, torch.argsort((~valid).int(), dim=1, stable=True))
        cnt = (nbs >= 0).sum(dim=1)
        off = torch.cumsum(cnt, 0) - cnt
        pack = hr.pair_mlp_pack([l.weight for l in lf], [l.bias for l in lf], F_, hr.PAIR_MLP_X2, "cuda")
        Gt = hr.pair_mlp_forward_raw(kf, None, None, nbs.long(), pts, kp, off, 0, hr.PAIR_MLP_X2, save=False, wpack=pack)[0]
    et = float((G - Gt).norm() / Gt.norm())
    print(f"pairs_x2 [F={F_}]: {tiles} tiles on {cap} workgroups ({ceil_div(tiles, cap)} per workgroup); rel-L2 vs float64 / bar {e64 / 3e-5:.3f}, "
          f"vs the training kernel / bar {et / 1e-5:.3f}")
    assert e64 < 3e-5 and et < 1e-5, (e64, et)
    empty = ~valid.any(dim=1)
    assert int(empty.sum()) >= 8 and float(G[empty].abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["plain", "dir", "save"])
def test_points_x2_over_several_tiles_per_workgroup(mode):
    """points_x2_kernel (inference without and with view-direction rows, and the training forward that saves its activations) on
    66125 points = 1034 tiles of 64 on 512 workgroups (ten take three; the weight ring restarts per tile): chunks of 16384 points give
    the same bits of sigma / rgb, of pre and of all six saved planes; the whole result to float64 at the bars of
    test_fused_point_level_layers_in_the_fp32_class (sigma 1e-4 of max(1, |sigma|), rgb 2e-5), the pre columns through softplus /
    sigmoid."""
    from npcd.hip import render as hr
    P, cap, step = 2 * 32768 + 64 * 9 + 13, 512, 16384
    tiles = ceil_div(P, 64)
    assert tiles == 1034 and tiles > 2 * cap and ceil_div(step, 64) <= cap
    use_dir = mode == "dir"
    gen = torch.Generator().manual_seed(50)
    field = _field(32, 1, use_dir, scale=1.7)
    G = (torch.randn(P, 256, generator=gen) * 4.0).cuda()
    wp = hr.points_x2_pack(field.state_dict(), "cuda")
    db = ray = pd = None
    if use_dir:
        from npcd.models.pointnerf.field import encode_dir
        n_rays = 4099
        rd = torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=gen), dim=-1).cuda()
        ray = torch.randint(0, n_rays, (P,), generator=gen, dtype=torch.int32).cuda()
        with torch.no_grad():
            db = (encode_dir(rd, field.dir_freqs) @ field.channel_net[0].weight[:, 256:].float().t()).contiguous()
        pd = rd[ray.long()]
    if mode == "save":
        pre, saved = hr.points_x2(wp, G, save=True)
        for lo in range(0, P, step):
            hi = min(lo + step, P)
            prec, savedc = hr.points_x2(wp, G[lo:hi], save=True)
            assert torch.equal(prec, pre[lo:hi]) and torch.equal(savedc, saved[:, lo:hi]), lo
        sig, rgb = torch.nn.functional.softplus(pre[:, 3] - 1.0), torch.sigmoid(pre[:, :3])
    else:
        sig, rgb = hr.points_x2(wp, G, db, ray)
        for lo in range(0, P, step):
            hi = min(lo + step, P)
            sc, cc = hr.points_x2(wp, G[lo:hi], db, None if ray is None else ray[lo:hi])
            assert torch.equal(sc, sig[lo:hi]) and torch.equal(cc, rgb[lo:hi]), lo
    f64 = copy.deepcopy(field).double()
    with torch.no_grad():
        feat = f64.aggregator.local_field[8](G.double())
        cin = feat if not use_dir else torch.cat((feat, encode_dir(pd.double(), field.dir_freqs)), dim=-1)
        want_s = torch.nn.functional.softplus(f64.shape_net(feat) - 1.0)[:, 0]
        want_c = torch.sigmoid(f64.channel_net(cin))
    es = float(((sig.double() - want_s).abs() / want_s.abs().clamp_min(1.0)).max())
    ec = float((rgb.double() - want_c).abs().max())
    print(f"points_x2 [{mode}]: {tiles} tiles on {cap} workgroups ({ceil_div(tiles, cap)} per workgroup); sigma / bar {es / 1e-4:.3f}, "
          f"rgb / bar {ec / 2e-5:.3f}")
    assert es < 1e-4 and ec < 2e-5, (es, ec)


# --------------------------------------------------------------------------------------------------------------------------------
# D. the fp16 shading kernels
# --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_", [32, 128])
def test_shading_over_several_tiles_per_workgroup(F_, shade_form, monkeypatch):
    """render.shade_points on 32997 points: 2063 pair tiles of 16 points dealt by ticket to 512 workgroups, 1032 point blocks of 32
    rows split two or three per workgroup; scaled-up weights and ragged neighbour counts as in test_shading_large_weights.
    The tile forms: chunks of 4096 points (one tile per workgroup) give the same bits.  The rows form aggregates in an order that
    depends on the position in the list: it is held to the tiles result at the fp16 bar of that test, 5e-3 of
    max(1, sigma) and 5e-3 abs.  The whole result to the oracle at the same bar on ~4000 points, every point of the last 64 tiles
    among them; the range guard stays clear."""
    from npcd.hip import render as hr
    P, cap, step, N = 2 * 16384 + 32 * 7 + 5, 512, 4096, 256
    tilesA, tilesB = ceil_div(P, 16), ceil_div(P, 32)
    assert (tilesA, tilesB) == (2063, 1032) and tilesA > 2 * cap and tilesB > 2 * cap and ceil_div(step, 16) <= cap
    p = orr.init_field_params(F_, seed=5)
    for kname in p:
        if kname.endswith("weight"):
            p[kname] = p[kname] * 1.7
    coords, feats = orr.synthetic_cloud(N, F_, 1, seed=2)
    gen = torch.Generator().manual_seed(60)
    n = P + P // 16
    base = coords[0][torch.randint(0, N, (n,), generator=gen)]
    pts = base + torch.randn(n, 3, generator=gen) * 0.02
    dist, nb = torch.topk(torch.cdist(pts, coords[0]), 8, largest=False)
    nb[dist >= 0.08] = -1
    nb[::7, 3:] = -1                                 # ragged neighbour counts
    keep = (nb >= 0).any(dim=1)
    assert int(keep.sum()) >= P
    nb, pts = nb[keep][:P], pts[keep][:P]
    wp = hr.pack_field_weights(p, F_, "cuda")
    nbd, ptd, kp, kf = nb.int().cuda(), pts.cuda(), coords[0].cuda(), feats[0].cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    sig, rgb = hr.shade_points(wp, F_, nbd, ptd, kp, kf, status=status)
    assert int(status) == 0
    bar = lambda s, c, s0, c0: max(float(((s - s0).abs() / s0.abs().clamp_min(1.0)).max()), float((c - c0).abs().max())) / 5e-3
    if shade_form == "rows":
        monkeypatch.delenv("NPCD_SHADE_ROWS")
        sig_t, rgb_t = hr.shade_points(wp, F_, nbd, ptd, kp, kf)
        monkeypatch.setenv("NPCD_SHADE_ROWS", "1")
        vs_tiles = bar(sig, rgb, sig_t, rgb_t)
        assert vs_tiles < 1.0, vs_tiles
        note = f"rows form vs tiles / bar {vs_tiles:.3f}"
    else:
        for lo in range(0, P, step):
            hi = min(lo + step, P)
            sc, cc = hr.shade_points(wp, F_, nbd[lo:hi], ptd[lo:hi], kp, kf)
            assert torch.equal(sc, sig[lo:hi]) and torch.equal(cc, rgb[lo:hi]), lo
        note = "chunks: the same bits"
    sub = torch.cat((torch.randperm(P - 64 * 16, generator=gen)[:3000].sort().values, torch.arange(P - 64 * 16, P)))
    sig_ref, rgb_ref, _ = orr.shade_points(p, nb[sub], pts[sub], coords, feats)
    vs_oracle = bar(sig.cpu()[sub], rgb.cpu()[sub], sig_ref[:, 0], rgb_ref)
    print(f"shading [{shade_form}, F={F_}]: {tilesA} pair tiles by ticket on {cap} workgroups (~{tilesA / cap:.0f} per workgroup), {tilesB} point "
          f"blocks ({tilesB // cap} or {ceil_div(tilesB, cap)} per workgroup); vs the oracle / bar {vs_oracle:.3f}; {note}")
    assert vs_oracle < 1.0, vs_oracle
