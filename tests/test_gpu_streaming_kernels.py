"""The HBM-bound kernels (csrc/elementwise.hip, csrc/split.hip) at the sizes a training step uses, against float64.

Every reference is plain float64 torch on the device, computed from the inputs after their rounding to the kernel's input type.
Every bar is built from (a) half an ulp of the 16-bit output type at the reference value, (b) a first-order forward-error bound of
the fp32 operation (number of roundings on the longest path x 2^-24 x the magnitudes involved; the path lengths are read off the
kernels and are upper bounds, so a legal change of the summation order stays inside), and (c) for the polynomial GELU the absolute
erf error its comment claims.  Outputs are allocated between sentinel-filled guard bands and start as NaN: a kernel must write
every element of its range and nothing else.  The large shapes run twice and must give the same bits.

REGIMES is the list of (kernel, path, shape): test_regime_table asserts from the launch geometry the library exports that each
shape reaches the path it is listed for; caps that are literals of the launch code are named there once.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                   # unit roundoff of fp32
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HALVES = [BF16, F16]
SENT = 1536.0                    # guard value (exact in bf16, f16 and fp32)
ERR_ARG, ERR_UNSUPPORTED = -1, -2

# ---- launch-code literals (name: value, where it comes from) ------------------------------------------------------------------------
LN_FWD_WG = 2048                 # ln_fwd_blocks(), elementwise.hip: 4 rows per workgroup -> a wave walks rows above T = 8192
LN_BWD_ROUND = 4 * 512           # ln_rows_per_wave(): rows per wave = ceil(T / 2048) up to 32, then 16 with a larger grid
ADAM_S = 8192 * 256              # npcd_adamw_ema_dt / _gated: float4 per grid sweep
GELU_S8 = 16384 * 256            # npcd_gelu_fwd_dt, npcd_split3_bf16, npcd_split_weights_bf16: 8-element groups per sweep
CAST_S = 8192 * 256              # npcd_cast_f32_dt: float4 per sweep
SLICES_S = 4096 * 256            # npcd_sum_slices: float4 per sweep
ALS_WG = 8192                    # npcd_add_ln_split3_stats_bf16: 4 rows per workgroup -> a wave walks rows above T = 32768
QS_WG, MSE_BWD_WG, DDPM_WG = 256, 2048, 1024     # npcd_q_sample, npcd_eps_mse_bwd, npcd_ddpm_reverse_step (256 elements per workgroup)

# (kernel, path, T, expected exported block count or None)
REGIMES = [
    ("ln_bwd", "one row per wave", 1, 1), ("ln_bwd", "one row per wave", 513, 129), ("ln_bwd", "one row per wave, full round", 2048, 512),
    ("ln_bwd", "A/B loop, 1 or 2 rows", 2049, 257), ("ln_bwd", "A/B loop, 2 rows", 4096, 512),
    ("ln_bwd", "A/B loop, 3 rows ragged", 4097, 342), ("ln_bwd", "A/B loop, 3 rows (a rank)", 4104, 342),
    ("ln_bwd", "A/B loop, 17 rows (benchmark)", 32832, 483), ("ln_bwd", "A/B loop, 32 rows: last one-round size", 65536, 512),
    ("ln_bwd", "fixed 16 rows, larger grid", 65537, 1025), ("ln_bwd", "fixed 16 rows, larger grid", 70001, 1094),
    ("colsum", "8 rows per band", 1, 1), ("colsum", "8 rows per band", 513, 65), ("colsum", "8 rows per band (a rank)", 4104, 513),
    ("colsum", "first T with 9 rows", 4608, 512), ("colsum", "64 rows: last T below the clamp", 32768, 512),
    ("colsum", "64 rows clamped (benchmark)", 32832, 513), ("colsum", "64 rows clamped", 40000, 625),
]
LN_BWD_T = [r[2] for r in REGIMES if r[0] == "ln_bwd"]
COLSUM_T = [r[2] for r in REGIMES if r[0] == "colsum"]


def _L():
    from npcd.hip import lib
    return lib()


def _ew():
    from npcd.hip import elementwise as ew
    return ew


def _sp():
    from npcd.hip import stream_ptr
    return stream_ptr()


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def code(dtype):
    return {BF16: 0, F16: 1, F32: 2}[dtype]


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


class Guarded:
    """A tensor of `shape` that starts as NaN (`fill`), between two guard bands of at least one row."""

    def __init__(self, shape, dtype, fill=math.nan):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        self.pad = (max(64, shape[-1]) + 63) // 64 * 64          # keeps the 16-byte alignment of the body
        self.buf = torch.full((n + 2 * self.pad,), SENT, dtype=dtype, device="cuda")
        self.t = self.buf[self.pad:self.pad + n].view(shape)
        self.t.fill_(fill)

    def check(self, name, written=True):
        g = torch.cat([self.buf[:self.pad], self.buf[-self.pad:]])
        assert bool((g == SENT).all()), f"{name}: a guard band was written"
        if written:
            assert not bool(torch.isnan(self.t).any()), f"{name}: elements of the range were not written"


def half_ulp(ref, dtype):
    """Half the spacing of `dtype` at the float64 values `ref` (subnormal spacing below the smallest normal)."""
    p, emin = (8, -126) if dtype == BF16 else (11, -14)
    _, e = torch.frexp(ref.abs())                     # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, torch.full_like(e, emin), e - 1).clamp_min(emin)
    return torch.ldexp(torch.ones_like(ref), e - (p - 1)) * 0.5


def close(name, got, ref, bar):
    """|got - ref| <= bar for EVERY element (float64); prints the worst ratio first."""
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
    worst = float(ratio.max())
    print(f"[bar] {name}: max |err| / bar = {worst:.3f}")
    assert worst <= 1.0, f"{name}: {int((ratio > 1).sum())} of {ratio.numel()} elements outside the bar, worst {worst:.3g} x at flat index {int(ratio.argmax())}"


def fin_depth(nblk):
    """Longest chain of fp32 additions in the column-sum finalisation of nblk partial rows (colsum_stage1/2_kernel)."""
    if nblk <= 32:
        return nblk
    per = -(-nblk // 16)
    return -(-per // 8) + 1 + 1 + 2 + 16


def finalize(part_full, nblk, N, out, accumulate=0):
    rc = _L().npcd_colsum_finalize(P(part_full), nblk, N, P(out), accumulate, _sp())
    assert rc == 0, rc


# =====================================================================================================================================
# 1. the regime table
# =====================================================================================================================================
def test_regime_table():
    L = _L()
    for kernel, path, T, blocks in REGIMES:
        got = L.npcd_ln_bwd_blocks(T) if kernel == "ln_bwd" else L.npcd_colsum_blocks(T)
        assert got == blocks, f"{kernel} at T = {T} ({path}): {got} blocks, the table expects {blocks}: a threshold moved"
    rpw = lambda T: -(-T // (4 * L.npcd_ln_bwd_blocks(T)))
    assert [rpw(T) for T in (2048, 2049, 4104, 32832, 65536, 65537)] == [1, 2, 3, 17, 32, 16]
    rows = lambda T: -(-T // L.npcd_colsum_blocks(T))
    assert [rows(T) for T in (513, 4104, 4608, 32768, 32832, 40000)] == [8, 8, 9, 64, 64, 64]
    assert L.npcd_colsum_scratch_rows() == 16
    assert L.npcd_small_wgrad_blocks(262144) == 1024 and L.npcd_small_wgrad_blocks(262145) == 1024 and L.npcd_small_wgrad_blocks(257) == 2
    assert L.npcd_grad_stats_blocks() == 512 and L.npcd_eps_mse_blocks() == 256
    # The literal caps named at the top (LN_FWD_WG, ADAM_S, GELU_S8, CAST_S, SLICES_S, ALS_WG, QS_WG, MSE_BWD_WG, DDPM_WG) are not
    # exported by the library: no test can verify them, they are kept in step with the launch code by hand.  What is asserted
    # here is only that the shape lists stand on both sides of the values named.
    ln_T, als_T = [T for T, _ in LN_FWD_SHAPES], [T for T, _ in ALS_SHAPES]
    assert 4 * LN_FWD_WG in ln_T and 4 * LN_FWD_WG + 1 in ln_T and max(ln_T) > 3 * 4 * LN_FWD_WG
    assert 4 * ALS_WG in als_T and 4 * ALS_WG + 1 in als_T and max(als_T) > 3 * 4 * ALS_WG


# =====================================================================================================================================
# 2. LayerNorm forward
# =====================================================================================================================================
LN_FWD_SHAPES = [(1, 4), (1, 2048), (4, 260), (513, 68), (513, 1024), (4104, 252), (4104, 1024), (8192, 260), (8193, 256), (16384, 768),
                 (16385, 1028), (24613, 2044), (32832, 1024), (9000, 2048)]


def ln_rows(T, W, g):
    """fp32 rows with distinct per-row scale and offset; four rows with hard statistics where there is room."""
    x = randn(g, T, W) * (0.5 + 2 * torch.rand(T, 1, device="cuda", generator=g)) + randn(g, T, 1)
    if T >= 4:
        idx = [1, T // 2, T - 2, T - 1] if T >= 8 else [0, 1, 2, 3]
        x[idx[0]] = 100.0 + 0.01 * randn(g, W)          # mean >> std
        x[idx[1]] = 3.0                                 # constant
        x[idx[2], W // 2] = 1e4                         # one outlier
        x[idx[3]] = 0.0                                 # zeros
    return x


def ln_fwd_ref(v32, gamma, beta, eps, dsum=20, dsq=25):
    """float64 LayerNorm of the fp32 rows v32 and the fp32 forward-error bars of mean, rstd and y (before the 16-bit rounding).
    dsum: roundings on the longest chain of the row sum -- add_ln_fwd_kernel: 2 (four values) + 8 (chunks) + 6 (lanes) + 1 (the
    division) = 17 -> 20.  dsq: the same for the sum of squares, + 2 for the difference, 1 for the square, 2 for / W and + eps."""
    v = v32.double()
    mu = v.mean(1, keepdim=True)
    d = v - mu
    var = (d * d).mean(1, keepdim=True)
    e64 = float(np.float32(eps))
    rstd = 1.0 / torch.sqrt(var + e64)
    dmu = dsum * U * v.abs().mean(1, keepdim=True)                       # |mean| and the row's magnitudes x 2^-24
    rel_rs = 0.5 * (dmu * dmu + dsq * U * var) / (var + e64) + 4 * U     # computed variance = true variance + dmu^2, then rsqrtf
    xh = d * rstd
    y = xh * gamma.double() + beta.double()
    ybar = gamma.double().abs() * (dmu * rstd + xh.abs() * (rel_rs + 3 * U)) + 2 * U * ((xh * gamma.double()).abs() + y.abs())
    return mu[:, 0], dmu[:, 0], rstd[:, 0], (rstd * rel_rs)[:, 0], y, ybar


def run_add_ln_fwd(x, delta, gamma, beta, want_sum, dtype, eps=1e-5):
    T, W = x.shape
    xo = Guarded((T, W), F32) if want_sum else None
    y, mean, rstd = Guarded((T, W), dtype), Guarded(T, F32), Guarded(T, F32)
    rc = _L().npcd_add_ln_fwd_dt(P(x), P(delta), P(gamma), P(beta), P(xo.t if xo else None), P(y.t), P(mean.t), P(rstd.t), T, W, eps,
                                 code(dtype), _sp())
    assert rc == 0, rc
    for n, o in (("x_out", xo), ("y", y), ("mean", mean), ("rstd", rstd)):
        if o is not None:
            o.check(f"add_ln_fwd {n}")
    return xo, y, mean, rstd


@pytest.mark.parametrize("dtype", HALVES, ids=["bf16", "f16"])
@pytest.mark.parametrize("form", ["add", "add_nosum", "plain"])
@pytest.mark.parametrize("T,W", LN_FWD_SHAPES)
def test_add_ln_fwd(T, W, form, dtype):
    g = gen(T * 4099 + W)
    x = ln_rows(T, W, g)
    delta = randn(g, T, W).to(dtype) if form != "plain" else None
    gamma, beta = 1 + 0.2 * randn(g, W), 0.1 * randn(g, W)
    xo, y, mean, rstd = run_add_ln_fwd(x, delta, gamma, beta, form == "add", dtype)
    v32 = x if delta is None else x + delta.float()
    if xo is not None:
        assert torch.equal(xo.t, v32), "x_out is not the fp32 sum bit for bit"
    mu, dmu, rs, drs, yr, ybar = ln_fwd_ref(v32, gamma, beta, 1e-5)
    tag = f"add_ln_fwd[{T}x{W},{form},{dtype}]"
    close(tag + " mean", mean.t, mu, dmu + 1e-300)
    close(tag + " rstd", rstd.t, rs, drs)
    close(tag + " y", y.t, yr, half_ulp(yr, dtype) + ybar)
    if T >= 4104:                                      # bitwise reproducible
        _, y2, m2, r2 = run_add_ln_fwd(x, delta, gamma, beta, False, dtype)
        assert torch.equal(y2.t, y.t) and torch.equal(m2.t, mean.t) and torch.equal(r2.t, rstd.t)


# =====================================================================================================================================
# 3. LayerNorm backward (16-bit dy, and the fp32-dy split form)
# =====================================================================================================================================
LN_BWD_W = {1: 4, 513: 1024, 2048: 68, 2049: 260, 4096: 256, 4097: 252, 4104: 1024, 32832: 1024, 65536: 68, 65537: 68, 70001: 256}
LN_BWD_SHAPES = [(T, LN_BWD_W[T]) for T in LN_BWD_T] + [(4, 2048), (4104, 768), (4104, 1028), (6181, 2044), (9000, 2048)]
# form -> (dres, dcol, the 16-bit output).  "full" and "bare" at every shape; the forms with one option on and the others off at one
# shape of each row-loop regime (one row, A/B loop, fixed 16 rows)
LN_BWD_FORMS = {"full": (True, True, True), "bare": (False, False, False), "dres": (True, False, False), "dcol": (False, True, False),
                "copy": (False, False, True)}
LN_BWD_CASES = [(T, W, f) for T, W in LN_BWD_SHAPES for f in ("full", "bare")] + \
               [(T, W, f) for T, W in ((513, 1024), (4104, 1028), (65537, 68)) for f in ("dres", "dcol", "copy")]


def run_ln_bwd(kind, dy, x, mean, rstd, gamma, dres, want_col, want_16):
    """kind: a 16-bit dtype (npcd_ln_bwd_dt) or "split" (npcd_ln_bwd_split3_bf16).  Returns dx, the 16-bit output, the three sums."""
    L = _L()
    T, W = x.shape
    nblk, scratch = L.npcd_ln_bwd_blocks(T), L.npcd_colsum_scratch_rows()
    dx = Guarded((T, W), F32)
    d16 = (Guarded((T, 3 * W), BF16) if kind == "split" else Guarded((T, W), kind)) if want_16 else None
    parts = [Guarded((nblk + scratch, W), F32) for _ in range(3)]
    pc = P(parts[2].t) if want_col else P(None)
    if kind == "split":
        rc = L.npcd_ln_bwd_split3_bf16(P(dy), P(x), P(mean), P(rstd), P(gamma), P(dres), P(dx.t), P(d16.t if d16 else None), P(parts[0].t),
                                       P(parts[1].t), pc, T, W, _sp())
    else:
        rc = L.npcd_ln_bwd_dt(P(dy), P(x), P(mean), P(rstd), P(gamma), P(dres), P(dx.t), P(d16.t if d16 else None), P(parts[0].t),
                              P(parts[1].t), pc, T, W, code(kind), _sp())
    assert rc == 0, rc
    dx.check("ln_bwd dx")
    if d16 is not None:
        d16.check("ln_bwd 16-bit dx")
    sums = []
    for q, part in enumerate(parts):
        part.check(f"ln_bwd partials {q}", written=False)
        wrote = ~torch.isnan(part.t).any(1)
        want = nblk if (q < 2 or want_col) else 0
        assert bool(wrote[:want].all()) and not bool(wrote[want:].any()), f"ln_bwd partials {q}: rows written {wrote.nonzero().flatten().tolist()[:8]}..., expected the first {want}"
        if want:
            out = Guarded(W, F32)
            finalize(part.t, nblk, W, out.t)
            out.check(f"ln_bwd sum {q}")
            part.check(f"ln_bwd partials {q} after the finalisation", written=False)
            sums.append(out.t)
        else:
            sums.append(None)
    return dx.t, (d16.t if d16 else None), sums


@pytest.mark.parametrize("kind", [BF16, F16, "split"], ids=["bf16", "f16", "split3"])
@pytest.mark.parametrize("T,W,form", LN_BWD_CASES)
def test_ln_bwd(T, W, form, kind):
    L = _L()
    g = gen(T * 4099 + W + 1)
    x = ln_rows(T, W, g)
    gamma = 1 + 0.2 * randn(g, W)
    xd = x.double()
    mean = xd.mean(1).float()
    rstd = (1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float()           # the kernel takes them as inputs
    dy = randn(g, T, W) * (0.5 + torch.rand(T, 1, device="cuda", generator=g))
    dy = dy if kind == "split" else dy.to(kind)
    with_dres, want_col, want_16 = LN_BWD_FORMS[form]
    dres = randn(g, T, W) if with_dres else None
    dx, d16, (dgam, dbet, dcol) = run_ln_bwd(kind, dy, x, mean, rstd, gamma, dres, want_col, want_16)
    # float64 reference and first-order bars (sums: 17-rounding chains -> 20; products and differences one rounding each)
    mu, rs, gm, dyd = mean.double()[:, None], rstd.double()[:, None], gamma.double(), dy.double()
    xh = (xd - mu) * rs
    gy = dyd * gm
    c1, c2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    o = (gy - c1 - xh * c2) * rs
    ref = o if dres is None else o + dres.double()
    dc1, dc2 = 21 * U * gy.abs().mean(1, keepdim=True), 24 * U * (gy * xh).abs().mean(1, keepdim=True)
    bar = rs * (dc1 + 2 * U * xh.abs() * c2.abs() + xh.abs() * dc2 + 4 * U * (gy.abs() + c1.abs() + (xh * c2).abs())) + 2 * U * (o.abs() + ref.abs())
    tag = f"ln_bwd[{T}x{W},{form},{kind}]"
    close(tag + " dx", dx, ref, bar + 1e-300)
    if d16 is not None and kind == "split":
        hi = dx.bfloat16()
        lo = (dx - hi.float()).bfloat16()
        assert torch.equal(d16, torch.cat([hi, lo, hi], 1)), "dx3 is not [hi | lo | hi] of the dx that was written"
    elif d16 is not None:
        assert torch.equal(d16, dx.to(kind)), "the 16-bit dx is not the rounding of the dx that was written"
        close(tag + " dx16", d16, ref, half_ulp(ref, kind) + bar)
    # column sums: a wave adds its rows in order, 4 waves in a tree, then the finalisation
    nblk = L.npcd_ln_bwd_blocks(T)
    R = -(-T // (4 * nblk)) + 2 + fin_depth(nblk)
    t_g = dyd * xh
    close(tag + " dgamma", dgam, t_g.sum(0), (R + 3) * U * t_g.abs().sum(0) + 1e-300)
    close(tag + " dbeta", dbet, dyd.sum(0), R * U * dyd.abs().sum(0) + 1e-300)
    if dcol is not None:
        close(tag + " dcol", dcol, dx.double().sum(0), R * U * dx.double().abs().sum(0) + 1e-300)      # the sum of the dx that was written
    if T >= 4104:
        dx2, d162, s2 = run_ln_bwd(kind, dy, x, mean, rstd, gamma, dres, want_col, want_16)
        assert torch.equal(dx2, dx) and (d16 is None or torch.equal(d162, d16))
        assert all(a is None or torch.equal(a, b) for a, b in zip(s2, (dgam, dbet, dcol)))


# =====================================================================================================================================
# 4. residual add + LayerNorm + split (fp32 class)
# =====================================================================================================================================
ALS_SHAPES = [(1, 256), (513, 768), (4104, 1024), (4104, 2048), (32768, 256), (32769, 256), (32832, 1024), (65537, 256), (98427, 256), (300, 4096)]


@pytest.mark.parametrize("stats", [False, True], ids=["nostats", "stats"])
@pytest.mark.parametrize("add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("T,W", ALS_SHAPES)
def test_add_ln_split3(T, W, add, stats):
    L = _L()
    g = gen(T * 4099 + W + 2)
    x = ln_rows(T, W, g)
    o, bias = (randn(g, T, W), 0.3 * randn(g, W)) if add else (None, None)
    gamma, beta = 1 + 0.2 * randn(g, W), 0.1 * randn(g, W)

    def run():
        xn = Guarded((T, W), F32) if add else None
        out = Guarded((T, 3 * W), BF16)
        mean, rstd = (Guarded(T, F32), Guarded(T, F32)) if stats else (None, None)
        if stats:
            rc = L.npcd_add_ln_split3_stats_bf16(P(x), P(o), P(bias), P(gamma), P(beta), P(xn.t if xn else None), P(out.t), P(mean.t), P(rstd.t),
                                                 T, W, 1e-5, _sp())
        else:
            rc = L.npcd_add_ln_split3_bf16(P(x), P(o), P(bias), P(gamma), P(beta), P(xn.t if xn else None), P(out.t), T, W, 1e-5, _sp())
        assert rc == 0, rc
        for n, b in (("xnew", xn), ("out", out), ("mean", mean), ("rstd", rstd)):
            if b is not None:
                b.check(f"add_ln_split3 {n}")
        return xn, out, mean, rstd
    xn, out, mean, rstd = run()
    v32 = x + (o + bias) if add else x                  # the kernel adds a + b first, then to x
    if add:
        assert torch.equal(xn.t, v32), "xnew is not x + (o + bias) in fp32 bit for bit"
    # add_ln_split3_kernel adds a lane's values in order: 2 + 16 (float4 groups at W = 4096) + 6 lanes + 1 -> 28; squares 64 + 6 + 5 -> 80
    mu, dmu, rs, drs, yr, ybar = ln_fwd_ref(v32, gamma, beta, 1e-5, dsum=28, dsq=80)
    tag = f"add_ln_split3[{T}x{W},{'add' if add else 'plain'}]"
    if stats:
        close(tag + " mean", mean.t, mu, dmu + 1e-300)
        close(tag + " rstd", rstd.t, rs, drs)
    hi, lo, hi2 = out.t[:, :W], out.t[:, W:2 * W], out.t[:, 2 * W:]
    assert torch.equal(hi, hi2), "the third band is not the hi band"
    close(tag + " hi", hi, yr, half_ulp(yr, BF16) + ybar)
    # hi + lo carries the fp32 y up to the rounding of lo (|lo| <= 2^-8 |y|, rounded to 8 bits -> 2^-17 |y|; lo below bf16's normal range: 2^-134)
    close(tag + " hi+lo", hi.double() + lo.double(), yr, 2.0 ** -17 * yr.abs() + ybar + 2.0 ** -134)
    if T >= 4104:
        _, out2, _, _ = run()
        assert torch.equal(out2.t, out.t)


def test_layernorm_kernels_decline_unsupported_shapes_and_write_nothing():
    L = _L()
    g = gen(5)
    T = 8
    for W, want in ((6, ERR_UNSUPPORTED), (2052, ERR_UNSUPPORTED), (4096, ERR_UNSUPPORTED), (64, ERR_ARG)):
        misalign = W == 64
        xb = randn(g, T * W + 4)
        x = xb[1:1 + T * W] if misalign else xb[:T * W]                      # 4-byte offset: not 16-byte aligned
        gamma, beta, mean, rstd = randn(g, W), randn(g, W), randn(g, T), randn(g, T).abs()
        for dtype in HALVES:
            y, m, r, xo = Guarded((T, W), dtype), Guarded(T, F32), Guarded(T, F32), Guarded((T, W), F32)
            d = randn(g, T, W).to(dtype)
            assert L.npcd_add_ln_fwd_dt(P(x), P(d), P(gamma), P(beta), P(xo.t), P(y.t), P(m.t), P(r.t), T, W, 1e-5, code(dtype), _sp()) == want
            dx, dxb, pg, pb = Guarded((T, W), F32), Guarded((T, W), dtype), Guarded((18, W), F32), Guarded((18, W), F32)
            assert L.npcd_ln_bwd_dt(P(d), P(x), P(mean), P(rstd), P(gamma), P(None), P(dx.t), P(dxb.t), P(pg.t), P(pb.t), P(None), T, W,
                                    code(dtype), _sp()) == want
            torch.cuda.synchronize()
            for b in (y, m, r, xo, dx, dxb, pg, pb):
                b.check("declined call", written=False)
                assert bool(torch.isnan(b.t).all()), "a declined call wrote to its output"
        dx, dx3, pg, pb = Guarded((T, W), F32), Guarded((T, 3 * W), BF16), Guarded((18, W), F32), Guarded((18, W), F32)
        assert L.npcd_ln_bwd_split3_bf16(P(randn(g, T, W)), P(x), P(mean), P(rstd), P(gamma), P(None), P(dx.t), P(dx3.t), P(pg.t), P(pb.t), P(None),
                                         T, W, _sp()) == want
        torch.cuda.synchronize()
        for b in (dx, dx3, pg, pb):
            b.check("declined split3 backward", written=False)
            assert bool(torch.isnan(b.t).all()), "a declined call wrote to its output"
    # the split forward: widths that are not 256 x {1, 2, 3, 4, 8, 16}, and a misaligned x
    for W, off in ((260, 0), (1280, 0), (8192, 0), (256, 1)):
        xb = randn(g, T * W + 4)
        xs, gm, bt = xb[off:off + T * W], randn(g, W), randn(g, W)
        out, out2, xn, m, r = Guarded((T, 3 * W), BF16), Guarded((T, 3 * W), BF16), Guarded((T, W), F32), Guarded(T, F32), Guarded(T, F32)
        assert L.npcd_add_ln_split3_bf16(P(xs), P(None), P(None), P(gm), P(bt), P(None), P(out.t), T, W, 1e-5, _sp()) == ERR_UNSUPPORTED
        assert L.npcd_add_ln_split3_stats_bf16(P(xs), P(randn(g, T, W)), P(randn(g, W)), P(gm), P(bt), P(xn.t), P(out2.t), P(m.t), P(r.t), T, W, 1e-5,
                                               _sp()) == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        for b in (out, out2, xn, m, r):
            b.check("declined split3 forward", written=False)
            assert bool(torch.isnan(b.t).all()), "a declined call wrote to its output"
    assert L.npcd_add_ln_fwd_dt(P(randn(g, 8, 64)), P(None), P(randn(g, 64)), P(randn(g, 64)), P(None), P(torch.empty(8, 64, device="cuda")),
                                P(torch.empty(8, device="cuda")), P(torch.empty(8, device="cuda")), 8, 64, 1e-5, 2, _sp()) == ERR_UNSUPPORTED   # fp32 is no activation type


# =====================================================================================================================================
# 5. GELU forward / backward, column sums
# =====================================================================================================================================
def phi_cdf(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5)))


def phi_pdf(x):
    return torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def gelu_fwd_bar(x, ref, dtype):
    """half an ulp of the output + the stated |Phi error| 7.5e-8 x |x| + two fp32 roundings of the result"""
    return half_ulp(ref, dtype) + 7.5e-8 * x.abs() + 2 * U * ref.abs()


def gelu_bwd_ref(dg, h, dtype):
    hd, dgd = h.double(), dg.double()
    gp = phi_cdf(hd) + hd * phi_pdf(hd)
    ref = dgd * gp
    # stated erf error 1.5e-7 (absolute, on gelu'), four fp32 roundings of its two terms, one of the product
    bar = half_ulp(ref, dtype) + dgd.abs() * (1.5e-7 + 4 * U * (phi_cdf(hd) + (hd * phi_pdf(hd)).abs())) + U * ref.abs()
    return ref, bar


def sweep_values(dtype):
    """every representable value of `dtype` in [-12, 12] (both zeros and all subnormals among them) and the largest finite ones"""
    bits = torch.arange(65536, device="cuda", dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype)
    fin = torch.isfinite(v)
    big = torch.finfo(dtype).max
    keep = fin & ((v.float().abs() <= 12.0) | (v.float().abs() == big))
    return v[keep]


def run_gelu_fwd(h):
    out = Guarded(h.shape, h.dtype)
    rc = _L().npcd_gelu_fwd_dt(P(h), P(out.t), h.numel(), code(h.dtype), _sp())
    assert rc == 0, rc
    out.check("gelu_fwd")
    return out.t


def run_gelu_bwd(dg, h, dh_fill=math.nan):
    """-> dh, the partial rows buffer (nblk + scratch rows, NaN where not written), nblk"""
    L = _L()
    T, N = h.shape
    nblk = L.npcd_colsum_blocks(T)
    dh, part = Guarded((T, N), h.dtype), Guarded((nblk + L.npcd_colsum_scratch_rows(), N), F32)
    rc = L.npcd_gelu_bwd_dt(P(dg), P(h), P(dh.t), P(part.t), T, N, code(h.dtype), _sp())
    assert rc == 0, rc
    dh.check("gelu_bwd dh")
    part.check("gelu_bwd partials", written=False)
    wrote = ~torch.isnan(part.t).any(1)
    assert bool(wrote[:nblk].all()) and not bool(wrote[nblk:].any()), "gelu_bwd did not write exactly npcd_colsum_blocks(T) partial rows"
    return dh.t, part, nblk


@pytest.mark.parametrize("dtype", HALVES, ids=["bf16", "f16"])
def test_gelu_sweep_of_every_value(dtype):
    v = sweep_values(dtype)
    n = v.numel()
    assert n > (33000 if dtype == BF16 else 37000)
    N = 264
    T = -(-n // N)
    h = torch.zeros(T * N, dtype=dtype, device="cuda")
    h[:n] = v
    h = h.view(T, N)
    y = run_gelu_fwd(h)
    hd = h.double()
    ref = hd * phi_cdf(hd)
    close(f"gelu_fwd sweep[{dtype}]", y, ref, gelu_fwd_bar(hd, ref, dtype))
    assert bool((y[h == 0] == 0).all())
    dg = 1 + 0.5 * randn(gen(11), T, N)
    # gelu' is 1 at the largest finite value and the kernel does not saturate: |dg| <= 1 there keeps dh = dg * max finite
    dg = torch.where(h.float().abs() == torch.finfo(dtype).max, dg.clamp(-1.0, 1.0), dg).to(dtype)
    assert int((h.float().abs() == torch.finfo(dtype).max).sum()) == 2
    dh, part, nblk = run_gelu_bwd(dg, h)
    dref, dbar = gelu_bwd_ref(dg, h, dtype)
    close(f"gelu_bwd sweep[{dtype}]", dh, dref, dbar)


@pytest.mark.parametrize("dtype", HALVES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n8", [GELU_S8, GELU_S8 + 1, 2 * GELU_S8, 2 * GELU_S8 + 1, 3 * GELU_S8 + 123, 1, 513 * 33])
def test_gelu_fwd_around_the_grid_cap(n8, dtype):
    h = (2 * randn(gen(n8 % 1000 + 3), n8 * 8)).to(dtype)
    y = run_gelu_fwd(h)
    hd = h.double()
    ref = hd * phi_cdf(hd)
    close(f"gelu_fwd[n8={n8},{dtype}]", y, ref, gelu_fwd_bar(hd, ref, dtype))
    if n8 >= GELU_S8:
        assert torch.equal(run_gelu_fwd(h), y)


COLSUM_N = {1: 4096, 513: 4096, 4104: 4096, 4608: 264, 32768: 8, 32832: 4096, 40000: 264}
COLSUM_SHAPES = [(T, COLSUM_N[T]) for T in COLSUM_T] + [(1, 8), (513, 264), (4104, 8), (32832, 264), (4609, 8)]


@pytest.mark.parametrize("dtype", HALVES, ids=["bf16", "f16"])
@pytest.mark.parametrize("T,N", COLSUM_SHAPES)
def test_gelu_bwd_and_colsum(T, N, dtype):
    L = _L()
    g = gen(T * 31 + N)
    h = (2 * randn(g, T, N)).to(dtype)
    dg = (randn(g, T, N) * (0.5 + torch.rand(T, 1, device="cuda", generator=g)) * (0.5 + torch.rand(1, N, device="cuda", generator=g))).to(dtype)
    dh, part, nblk = run_gelu_bwd(dg, h)
    ref, bar = gelu_bwd_ref(dg, h, dtype)
    tag = f"[{T}x{N},{dtype}]"
    close("gelu_bwd dh" + tag, dh, ref, bar)
    rows = -(-T // nblk)
    R = rows + fin_depth(nblk)                              # a thread adds its `rows` rows in order, then the finalisation
    db = Guarded(N, F32)
    finalize(part.t, nblk, N, db.t)
    db.check("gelu_bwd dbias")
    dhd = dh.double()
    close("gelu_bwd dbias" + tag, db.t, dhd.sum(0), R * U * dhd.abs().sum(0) + 1e-300)      # the sum of the ROUNDED dh that was written
    # the plain column sum of a 16-bit matrix
    part2 = Guarded((nblk + L.npcd_colsum_scratch_rows(), N), F32)
    assert L.npcd_colsum_dt(P(dg), P(part2.t), T, N, code(dtype), _sp()) == 0
    part2.check("colsum partials", written=False)
    wrote = ~torch.isnan(part2.t).any(1)
    assert bool(wrote[:nblk].all()) and not bool(wrote[nblk:].any())
    cs = Guarded(N, F32)
    finalize(part2.t, nblk, N, cs.t)
    cs.check("colsum out")
    dgd = dg.double()
    close("colsum" + tag, cs.t, dgd.sum(0), R * U * dgd.abs().sum(0) + 1e-300)
    # through the wrappers: the same bits; part_rows form reports the rows it wrote
    ew = _ew()
    db2, cs2 = torch.empty(N, device="cuda"), torch.empty(N, device="cuda")
    dh2 = ew.gelu_bwd(dg, h, db2)
    ew.colsum_bf16(dg, cs2)
    assert torch.equal(dh2, dh) and torch.equal(db2, db.t) and torch.equal(cs2, cs.t)
    pr = torch.full((nblk + 3, N), math.nan, device="cuda")
    dh3, wrote_rows = ew.gelu_bwd(dg, h, None, part_rows=pr)
    assert wrote_rows == nblk and torch.equal(pr[:nblk], part.t[:nblk]) and bool(torch.isnan(pr[nblk:]).all()) and torch.equal(dh3, dh)


# =====================================================================================================================================
# 6. split-operand helpers
# =====================================================================================================================================
def split_torch(y):
    hi = y.bfloat16()
    return hi, (y - hi.float()).bfloat16()


@pytest.mark.parametrize("gelu", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("T,K", [(1, 8), (513, 264), (4104, 1024), (4096, 8192), (4097, 8192), (32832, 1024), (8193, 8192), (12289, 8200), (32832, 4096)])
def test_split3(T, K, gelu):
    n8 = T * (K // 8)
    g = gen(T + K)
    x, bias = 2 * randn(g, T, K), 0.3 * randn(g, K)
    for b in (bias, None):
        out = Guarded((T, 3 * K), BF16)
        assert _L().npcd_split3_bf16(P(x), P(b), P(out.t), T, K, int(gelu), _sp()) == 0
        out.check("split3")
        hi, lo, hi2 = out.t[:, :K], out.t[:, K:2 * K], out.t[:, 2 * K:]
        assert torch.equal(hi, hi2)
        y32 = x if b is None else x + b
        if not gelu:
            rh, rl = split_torch(y32)
            assert torch.equal(hi, rh) and torch.equal(lo, rl), "split3 is not [hi | lo | hi] of the fp32 sum"
        else:
            yd = y32.double()
            ref = yd * phi_cdf(yd)
            # libm erff: up to 4 ulp of erf, i.e. absolute 4 x 2^-24 on 1 + erf, x |y| / 2; its rounded argument and the two
            # products: one more 2^-24 |y| and 2 x 2^-24 |result|; then hi + lo
            f32bar = 3 * U * yd.abs() + 2 * U * ref.abs()
            close(f"split3 gelu hi[{T}x{K}]", hi, ref, half_ulp(ref, BF16) + f32bar)
            close(f"split3 gelu hi+lo[{T}x{K}]", hi.double() + lo.double(), ref, 2.0 ** -17 * ref.abs() + f32bar + 2.0 ** -134)
        if n8 >= GELU_S8 and b is None:
            out2 = Guarded((T, 3 * K), BF16)
            assert _L().npcd_split3_bf16(P(x), P(b), P(out2.t), T, K, int(gelu), _sp()) == 0
            assert torch.equal(out2.t, out.t)


def test_split3_shapes_reach_both_sides_of_the_grid_cap():
    n8 = [T * (K // 8) for T, K in ((4096, 8192), (4097, 8192), (8193, 8192), (12289, 8200), (32832, 4096))]
    assert n8[0] == GELU_S8 and n8[1] > GELU_S8 and n8[2] > 2 * GELU_S8 and n8[3] > 3 * GELU_S8 and n8[4] > 4 * GELU_S8


def test_split_weights_past_the_grid_cap():
    ew = _ew()
    g = gen(17)
    shapes = [(4096, 4096), (1024, 3072), (8, 8), (4096, 4096), (1031, 264), (4096, 4096), (4096, 4096), (1, 8)]
    assert sum(n * (k // 8) for n, k in shapes) > 2 * GELU_S8 and sum(n * (k // 8) for n, k in shapes[:1]) < GELU_S8
    ws = [randn(g, n, k) * (0.02 + 0.1 * j) for j, (n, k) in enumerate(shapes)]
    outs = ew.split_weights(ws)
    outs2 = ew.split_weights(ws)
    for w, (f, d), (f2, d2) in zip(ws, outs, outs2):
        hi, lo = split_torch(w)
        assert torch.equal(f, torch.cat([hi, hi, lo], 1)) and torch.equal(d, torch.cat([hi, hi, lo], 0))
        assert torch.equal(f, f2) and torch.equal(d, d2)
    # guard bands, through lib(): one small and one ragged weight
    w = randn(g, 37, 264)
    f, d = Guarded((37, 3 * 264), BF16), Guarded((3 * 37, 264), BF16)
    arr = (ew.SplitWeight * 1)()
    arr[0].w, arr[0].fwd, arr[0].dgrad, arr[0].N, arr[0].K = w.data_ptr(), f.t.data_ptr(), d.t.data_ptr(), 37, 264
    assert _L().npcd_split_weights_bf16(ctypes.cast(arr, ctypes.c_void_p), 1, _sp()) == 0
    f.check("split_weights fwd")
    d.check("split_weights dgrad")
    hi, lo = split_torch(w)
    assert torch.equal(f.t, torch.cat([hi, hi, lo], 1)) and torch.equal(d.t, torch.cat([hi, hi, lo], 0))


@pytest.mark.parametrize("gelu", [False, True], ids=["plain", "gelu"])
@pytest.mark.parametrize("T,N", COLSUM_SHAPES)
def test_split3_colsum(T, N, gelu):
    L = _L()
    g = gen(T * 37 + N)
    a = randn(g, T, N) * (0.5 + torch.rand(T, 1, device="cuda", generator=g)) * (0.5 + torch.rand(1, N, device="cuda", generator=g))
    h, bias = (2 * randn(g, T, N), 0.3 * randn(g, N)) if gelu else (None, None)
    nblk = L.npcd_colsum_blocks(T)

    def run():
        out, part = Guarded((T, 3 * N), BF16), Guarded((nblk + L.npcd_colsum_scratch_rows(), N), F32)
        assert L.npcd_split3_colsum_bf16(P(a), P(h), P(bias), P(out.t), P(part.t), T, N, int(gelu), _sp()) == 0
        out.check("split3_colsum out")
        part.check("split3_colsum partials", written=False)
        wrote = ~torch.isnan(part.t).any(1)
        assert bool(wrote[:nblk].all()) and not bool(wrote[nblk:].any())
        cs = Guarded(N, F32)
        finalize(part.t, nblk, N, cs.t)
        cs.check("split3_colsum sum")
        return out.t, cs.t
    out, cs = run()
    hi, lo, hi2 = out[:, :N], out[:, N:2 * N], out[:, 2 * N:]
    assert torch.equal(hi, hi2)
    R = -(-T // nblk) + fin_depth(nblk)
    tag = f"[{T}x{N}]"
    if not gelu:
        rh, rl = split_torch(a)
        assert torch.equal(hi, rh) and torch.equal(lo, rl)
        ad = a.double()
        close("split3_colsum sum" + tag, cs, ad.sum(0), R * U * ad.abs().sum(0) + 1e-300)
    else:
        z32 = h + bias
        zd, ad = z32.double(), a.double()
        cdf, xpdf = phi_cdf(zd), zd * phi_pdf(zd)
        ref = ad * (cdf + xpdf)
        # z is rounded once (|gelu''| <= 1.13), libm erff / expf a few ulp on each term, the sum and the product one rounding each
        vbar = ad.abs() * (1.13 * U * zd.abs() + 4 * U * (cdf + xpdf.abs()) + 2 * U) + 2 * U * ref.abs()
        close("split3_colsum gelu hi" + tag, hi, ref, half_ulp(ref, BF16) + vbar)
        close("split3_colsum gelu hi+lo" + tag, hi.double() + lo.double(), ref, 2.0 ** -17 * ref.abs() + vbar + 2.0 ** -134)
        close("split3_colsum gelu sum" + tag, cs, ref.sum(0), vbar.sum(0) + R * U * ref.abs().sum(0))
    if T >= 4104:
        out2, cs2 = run()
        assert torch.equal(out2, out) and torch.equal(cs2, cs)


# =====================================================================================================================================
# 7. column-sum finalisation
# =====================================================================================================================================
FIN_NBLK = [1, 2, 31, 32, 33, 64, 65, 513, 4104]
FIN_N = [8, 63, 64, 65, 256, 257, 4096]


def fin_job(nblk, N, seed, accumulate):
    g = gen(seed)
    part = Guarded((nblk + 16, N), F32)
    part.t[:nblk] = randn(g, nblk, N) * (0.5 + torch.rand(1, N, device="cuda", generator=g))
    out = Guarded(N, F32, fill=0.0)
    out.t.copy_(randn(g, N) * 3)
    return part, out


def fin_check(name, part, out, out0, nblk, accumulate):
    part.check(name + " partials", written=False)
    out.check(name + " out")
    pd = part.t[:nblk].double()
    ref = pd.sum(0) + (out0.double() if accumulate else 0)
    bar = fin_depth(nblk) * U * pd.abs().sum(0) + (U * (out0.double().abs() + ref.abs()) if accumulate else 0)
    close(name, out.t, ref, bar + 1e-300)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("nblk", FIN_NBLK)
def test_colsum_finalize_single_jobs(nblk, accumulate):
    assert (nblk > 32) == (nblk in (33, 64, 65, 513, 4104))          # both sides of fin_two_stage (nblk > 2 * 16)
    for N in FIN_N:
        part, out = fin_job(nblk, N, nblk * 7 + N, accumulate)
        out0 = out.t.clone()
        rows0 = part.t[:nblk].clone()
        finalize(part.t, nblk, N, out.t, accumulate)
        fin_check(f"finalize[nblk={nblk},N={N},acc={accumulate}]", part, out, out0, nblk, accumulate)
        assert torch.equal(part.t[:nblk], rows0), "the finalisation changed the partial rows"


MIXED = [(513, 4096, 0), (2, 63, 1), (33, 65, 0), (32, 256, 1), (4104, 257, 0), (1, 8, 0), (65, 64, 1), (31, 4096, 0), (64, 1024, 1)]


def test_colsum_finalize_batches_equal_single_jobs_bit_for_bit():
    ew, L = _ew(), _L()
    jobs = [fin_job(nblk, N, 100 + j, acc) + (nblk, N, acc) for j, (nblk, N, acc) in enumerate(MIXED)]
    out0 = [o.t.clone() for _, o, *_ in jobs]
    single = []
    for (part, out, nblk, N, acc), o0 in zip(jobs, out0):
        finalize(part.t, nblk, N, out.t, acc)
        single.append(out.t.clone())
        fin_check(f"finalize single[{nblk},{N},{acc}]", part, out, o0, nblk, acc)
        out.t.copy_(o0)
        part.t[nblk:] = math.nan
    # 8 mixed jobs in one call
    arr = (ew.ColsumJob * 8)()
    for a, (part, out, nblk, N, acc) in zip(arr, jobs[:8]):
        a.part, a.out, a.nblk, a.N, a.accumulate, a.reserved = part.t.data_ptr(), out.t.data_ptr(), nblk, N, acc, 0
    assert L.npcd_colsum_finalize_batch(ctypes.cast(arr, ctypes.c_void_p), 8, _sp()) == 0
    for (part, out, nblk, N, acc), s, o0 in zip(jobs[:8], single, out0):
        part.check("batch partials", written=False)
        out.check("batch out")
        assert torch.equal(out.t, s), f"batched job ({nblk}, {N}, {acc}) differs from the single-job form"
        out.t.copy_(o0)
        part.t[nblk:] = math.nan
    assert L.npcd_colsum_finalize_batch(ctypes.cast(arr, ctypes.c_void_p), 9, _sp()) == ERR_ARG
    # 9 jobs through ColsumBatch.flush (8 + 1)
    b = ew.ColsumBatch()
    for part, out, nblk, N, acc in jobs:
        b.add(part.t, nblk, N, out.t, bool(acc))
    b.flush()
    assert b.jobs == []
    for (part, out, nblk, N, acc), s in zip(jobs, single):
        part.check("flush partials", written=False)
        out.check("flush out")
        assert torch.equal(out.t, s), f"ColsumBatch job ({nblk}, {N}, {acc}) differs from the single-job form"


# =====================================================================================================================================
# 8. AdamW + EMA (+ shadow, + gradient zeroing), plain and gated
# =====================================================================================================================================
ADAM_N4 = [ADAM_S, ADAM_S + 1, 2 * ADAM_S - 1, 2 * ADAM_S, 2 * ADAM_S + 1, 3 * ADAM_S + 123, 1, 3074]
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, decay=0.99)


def f32(x):
    return float(np.float32(x))


def host_bc(t):
    return (np.float32(1.0 - math.pow(f32(HP["beta1"]), t)), np.float32(math.sqrt(1.0 - math.pow(f32(HP["beta2"]), t))))


def opt_state(n, seed):
    g = gen(seed)
    p = randn(g, n)
    m = 1e-2 * randn(g, n)
    v = 1e-4 * torch.rand(n, device="cuda", generator=g) + 1e-8
    ema = p + 1e-2 * randn(g, n)
    return p, m, v, ema


class Adam64:
    """The documented update (elementwise.hip: torch.optim.AdamW semantics + EMA lerp) in float64 on the fp32-rounded hyperparameters,
    with a running first-order bound of what fp32 evaluation may differ by (each product, sum, quotient and square root one to three
    roundings; the bounds of m, v and p carry over from step to step)."""

    def __init__(self, p, m, v, ema):
        self.p, self.m, self.v = p.double(), m.double(), v.double()
        self.e = None if ema is None else ema.double()
        self.dp, self.dm, self.dv = (torch.zeros_like(self.p) for _ in range(3))
        self.de = torch.zeros_like(self.p)

    def step(self, g, t):
        lr, b1, b2, eps, wd = (f32(HP[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
        bc1, bc2 = (float(x) for x in host_bc(t))
        w = f32(1.0 - f32(HP["decay"]))
        g = g.double()
        t1, t2 = b1 * self.m, (1 - b1) * g
        self.dm = b1 * self.dm + 3 * U * (t1.abs() + t2.abs())
        self.m = t1 + t2
        t1, t2 = b2 * self.v, (1 - b2) * g * g
        self.dv = b2 * self.dv + 4 * U * (t1 + t2)
        self.v = t1 + t2
        p1 = self.p * (1 - lr * wd)
        dp1 = self.dp + 3 * U * p1.abs()
        sq = torch.sqrt(self.v)
        dsq = self.dv / (2 * sq) + 3 * U * sq
        den = sq / bc2 + eps
        dden = dsq / bc2 + 4 * U * den
        q = self.m / den
        dq = self.dm / den + q.abs() * dden / den + 3 * U * q.abs()
        step = lr / bc1
        upd = step * q
        self.p = p1 - upd
        self.dp = dp1 + step * dq + 3 * U * upd.abs() + U * self.p.abs()
        if self.e is not None:
            diff = self.p - self.e
            self.de = (1 - w) * self.de + w * self.dp + 3 * U * (self.e.abs() + w * diff.abs() + diff.abs() * w)
            self.e = self.e + diff * w


# form -> (ema, shadow dtype or None, zero_grad).  Everything on / everything off at every size; one option on and the others off at
# the size where some threads run the pair loop and others the tail, and at a small one
ADAM_FORMS = {"full_bf16": (True, BF16, True), "full_f16": (True, F16, True), "bare": (False, None, False), "ema": (True, None, False),
              "shadow": (False, F16, False), "zero": (False, None, True), "ema_zero": (True, None, True)}
ADAM_CASES = [(n4, f) for n4 in ADAM_N4 for f in ("full_bf16", "full_f16", "bare")] + \
             [(n4, f) for n4 in (2 * ADAM_S + 1, 3074) for f in ("ema", "shadow", "zero", "ema_zero")]


@pytest.mark.parametrize("n4,form", ADAM_CASES)
def test_adamw_ema_three_steps_against_float64(n4, form):
    ew = _ew()
    n = 4 * n4
    with_ema, half, zero = ADAM_FORMS[form]
    p0, m0, v0, e0 = opt_state(n, n4 % 997)
    bufs = {k: Guarded(n, F32) for k in ("p", "m", "v", "g")}
    for k, src in (("p", p0), ("m", m0), ("v", v0)):
        bufs[k].t.copy_(src)
    ema = Guarded(n, F32) if with_ema else None
    shadow = Guarded(n, half) if half is not None else None
    if with_ema:
        ema.t.copy_(e0)
    ref = Adam64(p0, m0, v0, e0 if with_ema else None)
    gg = gen(n4 % 991 + 1)
    for t in (1, 2, 3):
        grad = randn(gg, n) * (1.0 if t != 2 else 1e-3)
        bufs["g"].t.copy_(grad)
        ew.adamw_ema(bufs["p"].t, bufs["g"].t, bufs["m"].t, bufs["v"].t, ema.t if with_ema else None, shadow.t if shadow else None, HP["lr"],
                     HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], t, HP["decay"] if with_ema else None, zero_grad=zero)
        ref.step(grad, t)
        for k in bufs:
            bufs[k].check(f"adamw {k}")
        if with_ema:
            ema.check("adamw ema")
        if shadow is not None:
            shadow.check("adamw shadow")
            assert torch.equal(shadow.t, bufs["p"].t.to(half)), f"the shadow is not p.to({half}) at step {t}"
        if zero:
            assert not bool(bufs["g"].t.any()), "zero_grad left gradient elements"
        else:
            assert torch.equal(bufs["g"].t, grad), "the gradient was touched without zero_grad"
    tag = f"adamw[n4={n4},{form}]"
    close(tag + " m", bufs["m"].t, ref.m, ref.dm + 1e-300)
    close(tag + " v", bufs["v"].t, ref.v, ref.dv + 1e-300)
    close(tag + " p", bufs["p"].t, ref.p, ref.dp + 1e-300)
    if with_ema:
        close(tag + " ema", ema.t, ref.e, ref.de + 1e-300)


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
@pytest.mark.parametrize("n4", [2 * ADAM_S + 1, 3 * ADAM_S + 123])
def test_adamw_gives_the_same_bits_twice_past_the_grid_cap(n4, gated):
    ew = _ew()
    n = 4 * n4
    state = opt_state(n, n4 % 967)
    grad = randn(gen(n4 % 953), n)
    runs = []
    for _ in range(2):
        p, m, v, e = (x.clone() for x in state)
        g, sh = grad.clone(), torch.empty(n, dtype=BF16, device="cuda")
        if gated:
            ew.adamw_ema_gated(p, g, m, v, e, sh, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["decay"], record(0, 0.5, 0.9, 2),
                               zero_grad=True)
        else:
            ew.adamw_ema(p, g, m, v, e, sh, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], 2, HP["decay"], zero_grad=True)
        runs.append((p, m, v, e, sh, g))
    for a, b, name in zip(runs[0], runs[1], ("p", "m", "v", "ema", "shadow", "g")):
        assert torch.equal(a, b), f"{name} differs between two runs on the same inputs"
    assert not torch.equal(runs[0][0], state[0])


def record(found_inf, inv_scale, clip_coef, t):
    ew = _ew()
    ctl = ew.scaler_record("cuda", 1.0 / inv_scale, t)
    f = ctl.view(F32)
    ctl[ew.CTL_FOUND_INF] = int(found_inf)
    bc1, bc2 = host_bc(t)
    f[ew.CTL_INV_SCALE], f[ew.CTL_CLIP_COEF], f[ew.CTL_BC1], f[ew.CTL_BC2_SQRT] = inv_scale, clip_coef, float(bc1), float(bc2)
    return ctl


@pytest.mark.parametrize("half", HALVES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n4", ADAM_N4)
def test_gated_adamw_is_the_plain_kernel_on_the_prescaled_gradient(n4, half):
    ew = _ew()
    n = 4 * n4
    a = [x.clone() for x in opt_state(n, n4 % 983)]
    b = [x.clone() for x in a]
    sa, sb = torch.empty(n, dtype=half, device="cuda"), torch.empty(n, dtype=half, device="cuda")
    gg = gen(n4 % 977 + 2)
    inv, coef = 2.0 ** -12, 0.7131
    for t in (1, 2, 3):
        grad = randn(gg, n) * 4096.0
        ga = grad.clone()
        gb = (grad * inv) * f32(coef)                          # the two fp32 multiplies of the gated kernel, in its order
        ew.adamw_ema_gated(a[0], ga, a[1], a[2], a[3], sa, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], HP["decay"],
                           record(0, inv, coef, t), zero_grad=True)
        ew.adamw_ema(b[0], gb, b[1], b[2], b[3], sb, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], t, HP["decay"], zero_grad=True)
        for x, y, name in zip(a + [sa, ga], b + [sb, gb], ("p", "m", "v", "ema", "shadow", "g")):
            assert torch.equal(x, y), f"{name} differs at step {t}"
        assert not bool(ga.any())


@pytest.mark.parametrize("zero_grad", [True, False])
@pytest.mark.parametrize("n4", ADAM_N4)
def test_gated_adamw_skipped_step_moves_only_the_ema(n4, zero_grad):
    ew = _ew()
    n = 4 * n4
    p0, m0, v0, e0 = opt_state(n, n4 % 971)
    st = {k: Guarded(n, F32) for k in ("p", "m", "v", "ema", "g")}
    grad = randn(gen(3), n)
    grad[n - 1] = math.inf
    for k, src in (("p", p0), ("m", m0), ("v", v0), ("ema", e0), ("g", grad)):
        st[k].t.copy_(src)
    shadow = Guarded(n, F16)
    shadow.t.copy_(p0.to(F16))
    ew.adamw_ema_gated(st["p"].t, st["g"].t, st["m"].t, st["v"].t, st["ema"].t, shadow.t, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["wd"],
                       HP["decay"], record(1, 2.0 ** -12, 1.0, 4), zero_grad=zero_grad)
    for k in st:
        st[k].check(f"skipped step {k}", written=False)
    shadow.check("skipped step shadow")
    assert torch.equal(st["p"].t, p0) and torch.equal(st["m"].t, m0) and torch.equal(st["v"].t, v0) and torch.equal(shadow.t, p0.to(F16))
    assert (not bool(st["g"].t.any())) if zero_grad else torch.equal(st["g"].t, grad)
    w = float(np.float32(1.0 - HP["decay"]))                    # (float)(1 - decay), the documented weight of a skipped step
    ed, pd = e0.double(), p0.double()
    ref = ed + (pd - ed) * w
    close(f"skipped step ema[n4={n4}]", st["ema"].t, ref, 3 * U * (ed.abs() + (pd - ed).abs() * w) + U * ref.abs())
    assert not torch.equal(st["ema"].t, e0)


# =====================================================================================================================================
# 9. cast, ordered slice sum
# =====================================================================================================================================
def cast_specials(dtype):
    s = [0.0, -0.0, math.inf, -math.inf, math.nan, 65504.0, 65519.9, 65520.0, 65536.0, -70000.0, 3.4e38, -3.4e38, 1e-45, -1e-45, 1e-40, 5.9e-8,
         2.98e-8, 2.9802322387695312e-08, 2.981e-8, 6.1e-5, 6.0e-5, 1.1754942e-38, 9.2e-41, 4.6e-41, 4.5e-41]
    s += [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 - 2.0 ** -23]   # ties
    return torch.tensor(s, dtype=F32, device="cuda")


@pytest.mark.parametrize("dtype", HALVES, ids=["bf16", "f16"])
@pytest.mark.parametrize("n4", [CAST_S, CAST_S + 1, 2 * CAST_S, 2 * CAST_S + 1, 3 * CAST_S + 77, 1, 1027])
def test_cast_is_torchs_rounding_bit_for_bit(n4, dtype):
    n = 4 * n4
    g = gen(n4 % 1009)
    src = randn(g, n) * torch.exp2(torch.randint(-30, 18, (n,), device="cuda", generator=g).float())
    sp = cast_specials(dtype)
    k = min(sp.numel(), n)
    src[:k] = sp[:k]
    if n > 2 * sp.numel():
        src[n - sp.numel():] = sp.flip(0)
    dst = Guarded(n, dtype, fill=7.0)
    _ew().cast_f32_bf16(src, dst.t)
    dst.check("cast", written=False)
    ref = src.to(dtype)
    nan = torch.isnan(src)
    assert float(nan.sum()) <= 1e-3 * n or n < 4096           # NaN: compared as NaN, not by payload; below 0.1 % of the elements
    assert torch.equal(torch.isnan(dst.t), nan)
    got_bits, ref_bits = dst.t.view(torch.int16), ref.view(torch.int16)
    assert torch.equal(got_bits[~nan], ref_bits[~nan]), "cast differs from torch's .to(dtype)"


@pytest.mark.parametrize("S,n4", [(2, SLICES_S), (2, SLICES_S + 1), (2, 2 * SLICES_S), (2, 2 * SLICES_S + 1), (2, 3 * SLICES_S + 77), (4, 2 * SLICES_S + 1),
                                  (4, 3 * SLICES_S + 77), (8, SLICES_S), (8, 2 * SLICES_S + 1), (8, 3 * SLICES_S + 77), (8, 1), (4, 1027)])
def test_sum_slices_around_the_grid_cap(S, n4):
    n = 4 * n4
    part = randn(gen(S * 13 + n4 % 1013), S, n) * torch.arange(1, S + 1, device="cuda").float()[:, None]
    out = Guarded(n, F32)
    assert _ew().sum_slices(part, out.t)
    out.check("sum_slices")
    ref = part[0].clone()
    for s in range(1, S):
        ref = ref + part[s]
    assert torch.equal(out.t, ref), "sum_slices is not the ordered fp32 sum"


# =====================================================================================================================================
# 10. the plain streams of the diffusion process: one case above each grid cap, one with a ragged element count
# =====================================================================================================================================
def _tables(g, k):
    return [(0.05 + torch.rand(1000, device="cuda", generator=g)) for _ in range(k)]


@pytest.mark.parametrize("per_sample", [QS_WG * 256 * 2 + 4465, 70001, 255])
def test_q_sample_past_the_grid_cap(per_sample):
    g = gen(per_sample)
    B = 3
    x0, nz = randn(g, B, per_sample), randn(g, B, per_sample)
    ta, ts = _tables(g, 2)
    t = torch.tensor([0, 517, 999], device="cuda")
    out = _ew().q_sample(x0, nz, t, ta, ts)
    a, b = ta[t].double()[:, None] * x0.double(), ts[t].double()[:, None] * nz.double()
    close(f"q_sample[{per_sample}]", out, a + b, 2 * U * (a.abs() + b.abs()) + 1e-300)
    assert torch.equal(out, ta[t][:, None] * x0 + ts[t][:, None] * nz)              # the three separately rounded operations
    assert torch.equal(_ew().q_sample(x0, nz, t, ta, ts), out)                       # the same bits twice


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("numel", [MSE_BWD_WG * 256 * 2 + 4465, 600001, 255])
def test_eps_mse_past_the_grid_caps(numel, dtype):
    ew = _ew()
    g = gen(numel)
    nz = randn(g, numel)
    eps = (nz + 0.5 * randn(g, numel)).to(dtype).requires_grad_(True)
    loss, pw = ew.eps_mse(eps, nz, want_pointwise=True)
    d = nz.double() - eps.detach().double()
    pref = d * d * 0.5
    close(f"eps_mse pointwise[{numel}]", pw, pref, 3 * U * pref + 1e-300)
    R = -(-numel // (256 * 256)) + 6 + 2 + 4 + 6 + 1            # per-thread chain, lanes, waves, the finalisation, 1 / numel
    close(f"eps_mse loss[{numel}]", loss.detach().reshape(1), pref.mean().reshape(1), (R + 3) * U * pref.mean().reshape(1))
    (loss * 3.0).backward()
    gref = -d * (3.0 / numel)
    bar = 4 * U * gref.abs() + (half_ulp(gref, BF16) if dtype == BF16 else 0) + 1e-300
    close(f"eps_mse grad[{numel}]", eps.grad, gref, bar)
    loss2, _ = ew.eps_mse(eps.detach(), nz, want_pointwise=False)
    assert torch.equal(loss2, loss.detach())
    eps2 = eps.detach().clone().requires_grad_(True)                                 # the same bits twice, forward and backward
    loss3, pw3 = ew.eps_mse(eps2, nz, want_pointwise=True)
    (loss3 * 3.0).backward()
    assert torch.equal(loss3.detach(), loss.detach()) and torch.equal(pw3, pw) and torch.equal(eps2.grad, eps.grad)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("per_sample", [DDPM_WG * 256 * 2 + 4465, 300001, 255])
def test_ddpm_reverse_step_past_the_grid_cap(per_sample, dtype):
    g = gen(per_sample + 1)
    B = 2
    x, nz = randn(g, B, per_sample), randn(g, B, per_sample)
    eps = randn(g, B, per_sample).to(dtype)
    tabs = _tables(g, 5)
    tabs[4] = -3 * tabs[4]
    t = torch.tensor([0, 611], device="cuda")
    out, x0 = _ew().ddpm_reverse_step(x, eps, nz, t, tabs, clip=(-1.5, 1.5), want_x0=True)
    a, bb, c1, c2, lv = (tb[t].double()[:, None] for tb in tabs)
    xd = x.double()
    raw = a * xd - bb * eps.double()
    x0r = raw.clamp(-1.5, 1.5)
    x0bar = 3 * U * ((a * xd).abs() + (bb * eps.double()).abs())
    sd = torch.where(t[:, None] != 0, torch.exp(0.5 * lv), torch.zeros_like(lv))
    ref = c1 * x0r + c2 * xd + sd * nz.double()
    bar = c1 * x0bar + 4 * U * ((c1 * x0r).abs() + (c2 * xd).abs()) + 6 * U * (sd * nz.double()).abs()
    close(f"ddpm x0[{per_sample}]", x0, x0r, x0bar + 1e-300)
    close(f"ddpm x_prev[{per_sample}]", out, ref, bar + 1e-300)
    out2, x02 = _ew().ddpm_reverse_step(x, eps, nz, t, tabs, clip=(-1.5, 1.5), want_x0=True)
    assert torch.equal(out2, out) and torch.equal(x02, x0)                            # the same bits twice
