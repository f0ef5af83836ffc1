"""Per-element error bounds for the 16-bit attention kernels (a helper module: nothing here is collected).

The bound, at EVERY element of an output (none exempt, nothing clamped to the tensor's maximum):

    |kernel - reference| <= K * u * scale[element]

`reference` is float64 softmax attention and its backward on the 16-bit values the kernel was given, `u` the unit roundoff of the
16-bit type (2^-8 bf16, 2^-11 f16), and `scale[element]` the element's own sum of absolute terms (`scales`): a rounding of relative
size u at one point of the data path moves an output by at most u times that sum.

K is DERIVED, not fitted: the number of 16-bit roundings on the path to the output, read from the kernels, plus 0.5 for the fp32
arithmetic in between (fp32 accumulation of n <= 2049 terms: n 2^-24 / u <= 0.25 for f16; hardware exp2 and log).

  out  K = 2.5   1. P = exp2(s - m) is rounded to 16 bit before P.V      csrc/attention.hip:536 (32-row forward), :774 (64-row forward)
                 2. the stored row o / l                                  csrc/attention.hip:233-236 (store_rows_staged)
  dv   K = 2.5   1. P = exp2(s - lse) is rounded before dO^T P            csrc/attention.hip:1480 (dK/dV pass)
                 2. the stored row                                        csrc/attention.hip:1708 -> :233-236
  dq   K = 3.5   1. dS = P (dP - delta) is rounded before K^T dS^T        csrc/attention.hip:1169, :1220 (dQ pass)
                 2. delta = rowsum(dO * O) reads the 16-bit O             csrc/attention.hip:1292
                 3. the stored row                                        csrc/attention.hip:1364 -> :233-236
  dk   K = 3.5   1. dS rounded before Q^T dS                              csrc/attention.hip:1481
                 2. delta (from the dQ pass, as above)                    csrc/attention.hip:1292, :1300
                 3. the stored row                                        csrc/attention.hip:1707 -> :233-236

The other kernels round at the same points and at no further one, so they get the same K:

  generic family (d = 32, 128, and 64 under NPCD_ATTN_GEN): P csrc/attention_gen.hip:183 (pack8); stored rows :116 (store_row); dS :257
  (dQ pass) and :338 (dK/dV pass, P on the same line); delta from the 16-bit O :218-220.
  single-pass backward: P csrc/attention.hip:1897, dS :1898 (the same rounded dS feeds dK and, through LDS, dQ); delta from the 16-bit O
  :1965-1968; dQ is summed in fp32 between the 256-key passes (:1822, :1829) and rounded once at :1825-1826; dK / dV stored at :2118-2119.
  edge token (n = 128 j + 1): its three rows are fp32 sums of fp32 partials and are rounded once, csrc/attention.hip:2857; the seeded
  key / query (n = 64 j + 1) enters in fp32 (:1312, :1648): fewer roundings than K counts, never more.

f16 only: a P or dS entry below 2^-14 is subnormal and its rounding error is ABSOLUTE, at most eta = 2^-25 (half the subnormal spacing
2^-24), whatever its size.  That rounding happens once per entry, so the term enters the bound once, not K times: the bound for f16 is
K u c + eta S with S the sum of the absolute values of the other operand over the reduction index (`scales` folds it into the scale as
eta S / (K u)).  It assumes gradual underflow; a kernel that flushed those entries to zero would be off by up to 2^-14 S and fail the
`wide` family (the CPU model without the term: 21.3 units on dv at d = 32, n = 200, against 1.7 with it; the other outputs do not move).

lse is compared with float64 logsumexp of the scaled scores: LSE_BAR below.
"""
import functools
import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ETA = 2.0 ** -25
K = {"out": 2.5, "dv": 2.5, "dq": 3.5, "dk": 3.5}
# |lse - logsumexp| in absolute terms: four times the rounding model's own worst error over the cases of test_attention_bounds_cpu.py
# (scores rounded to fp32, lse = m + log(l) rounded to fp32).  Measured: 3.754e-6, the `wide` family at d = 32, n = 385, where lse reaches
# 60 and half an fp32 ulp is 1.9e-6.  The factor 4 is for a 64-term fp32 dot product, hardware exp2 and logf.
LSE_MODEL_WORST = 3.76e-6
LSE_BAR = 4 * LSE_MODEL_WORST

DEFECTS = ("fwd_tile", "fwd_bwd_tile", "last_key", "denominator", "swap_rows", "dq_tile", "dkdv_last_row", "dv_element")
FAMILIES = ("rand", "wide", "spike", "edge_dominant")


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_inputs(family, B, H, n, d, dtype, seed):
    """(qkv [B, n, H, 3 d], dout [B, n, H, d]) in `dtype` on the CPU: the packed layout the kernels consume."""
    gen = torch.Generator().manual_seed(seed)
    amp = 1.5 * (64 / d) ** 0.25
    if family in ("rand", "wide"):
        qkv = torch.randn(B, n, H, 3 * d, generator=gen) * amp
        if family == "wide":
            qkv[..., :d] *= 3.0
    elif family == "spike":
        # test_attention_forced_rescale / test_forced_rescale_at_other_head_dims: score 576 / sqrt(d); one key in the LAST 64-key tile
        # (the running maximum jumps late) and one in the first
        assert n >= 8
        qkv = torch.randn(B, n, H, 3 * d, generator=gen)
        big = 3.0 * (64 / d) ** 0.5
        late = n - 1 - ((n - 1) % 64) // 2
        qkv[:, 5, :, 0:d] = big
        qkv[:, late, :, d:2 * d] = big
        qkv[:, 6, :, 0:d] = -big
        qkv[:, 3, :, d:2 * d] = -big
    elif family == "edge_dominant":
        # test_attention_edge_token_extremes: the last key wins (almost) every row's softmax, the last query of head 0 is peaked on key 7
        assert n >= 8
        qkv = torch.randn(B, n, H, 3 * d, generator=gen)
        q, k = qkv[..., :d], qkv[..., d:2 * d]
        k[:, -1] = 0.35 * q.mean(dim=1) + 0.9
        q[:, -1, 0] = 4.0 * k[:, 7, 0]
    else:
        raise ValueError(family)
    dout = torch.randn(B, n, H, d, generator=gen)
    return qkv.to(dtype), dout.to(dtype)


def split(qkv):
    """packed [B, n, H, 3 d] -> q, k, v as [B, H, n, d] views"""
    d = qkv.shape[-1] // 3
    x = qkv.permute(0, 2, 1, 3)
    return x[..., :d], x[..., d:2 * d], x[..., 2 * d:]


def bhnd(x):
    """[B, n, H, d] (the kernels' layout) -> [B, H, n, d] (this module's)"""
    return x.permute(0, 2, 1, 3)


# --------------------------------------------------------------------------------------------------------------- reference
def reference(q, k, v, dout, scale):
    """float64 softmax attention with a free scale and its backward; q, k, v, dout [B, H, n, d] of any dtype.
    Returns out, lse, dq, dk, dv."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    s = scale * (q @ k.transpose(-1, -2))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    out = p @ v
    dp = dout @ v.transpose(-1, -2)
    delta = (dout * out).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    return out, lse, scale * (ds @ k), scale * (ds.transpose(-1, -2) @ q), p.transpose(-1, -2) @ dout


def scales(q, k, v, dout, scale, dtype):
    """The per-element error scales {out, dv, dq, dk} (float64, the outputs' shapes): sums of the absolute terms with the exact softmax p and
    E = p (|dP| + sum_d |dout out|); for f16 plus the subnormal term, written so that one K multiplies the sum:
    K u (c + eta S / (K u)) = K u c + eta S."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    s = scale * (q @ k.transpose(-1, -2))
    p = torch.softmax(s, -1)
    out = p @ v
    e = p * ((dout @ v.transpose(-1, -2)).abs() + (dout * out).abs().sum(-1, keepdim=True))
    c = {"out": p @ v.abs(), "dv": p.transpose(-1, -2) @ dout.abs(), "dq": scale * (e @ k.abs()), "dk": scale * (e.transpose(-1, -2) @ q.abs())}
    if dtype == torch.float16:
        u = U[dtype]
        sub = {"out": v.abs().sum(-2, keepdim=True), "dv": dout.abs().sum(-2, keepdim=True),
               "dq": scale * k.abs().sum(-2, keepdim=True), "dk": scale * q.abs().sum(-2, keepdim=True)}
        for name in c:
            c[name] = c[name] + ETA * sub[name] / (K[name] * u)
    return c


@functools.lru_cache(maxsize=None)
def case(family, B, H, n, d, dtype, seed, scale=None):
    """One input set with its reference and scales, computed once and shared (callers must not modify it).
    -> dict(qkv, dout, scale, ref {out, lse, dq, dk, dv}, c {out, dv, dq, dk}); everything [B, H, n, d] except qkv / dout (packed layout)."""
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    qkv, dout = make_inputs(family, B, H, n, d, dtype, seed)
    q, k, v = split(qkv)
    out, lse, dq, dk, dv = reference(q, k, v, bhnd(dout), scale)
    return {"qkv": qkv, "dout": dout, "scale": scale, "dtype": dtype, "ref": {"out": out, "lse": lse, "dq": dq, "dk": dk, "dv": dv},
            "c": scales(q, k, v, bhnd(dout), scale, dtype)}


# ---------------------------------------------------------------------------------------------------------- rounding model
def _tile_of(mass, n):
    """the 64-key tile with the largest share of `mass` [rows, n]: a lost tile that nobody attends to changes nothing by construction"""
    nt = (n + 63) // 64
    per = torch.stack([mass[:, 64 * t:64 * t + 64].sum() for t in range(nt)])
    return int(per.argmax())


def rounding_model(q, k, v, dout, scale, dtype, defect=None, **where):
    """Plain torch emulation of the kernels' arithmetic: float64 everywhere, rounded at exactly the points K counts -- scores to fp32; the
    unnormalised exp(s - m) to the 16-bit type before P.v (the row sum from the unrounded values); out, P, dS and the three gradients to the
    16-bit type; delta from the rounded out.  q, k, v, dout [B, H, n, d].  Returns out, lse, dq, dk, dv in float64.

    defect: None or one of DEFECTS, injected into batch B - 1, head H - 1 (last_key: everywhere).  `where` overrides the defect's default
    position (tile=, row=, key0=, elem=)."""
    assert defect is None or defect in DEFECTS, defect
    r16 = lambda x: x.to(dtype).double()
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    B, H, n, d = q.shape
    bb, hh = B - 1, H - 1
    s = (q @ k.transpose(-1, -2)).float().double() * scale
    p_exact = torch.softmax(s[bb, hh], -1)
    blk = slice(32, 64) if n >= 64 else slice(0, min(32, n))                  # the 32-row block of the tile defects
    fwd_keep = torch.ones(B, H, n, n, dtype=torch.bool)
    bwd_keep = torch.ones(B, H, n, n, dtype=torch.bool)                       # pairs that enter dq
    kv_keep = torch.ones(B, H, n, n, dtype=torch.bool)                        # pairs that enter dk / dv
    if defect in ("fwd_tile", "fwd_bwd_tile"):
        t = where.get("tile", _tile_of(p_exact[blk], n))
        fwd_keep[bb, hh, blk, 64 * t:64 * t + 64] = False
        if defect == "fwd_bwd_tile":
            bwd_keep[bb, hh, blk, 64 * t:64 * t + 64] = False
            kv_keep[bb, hh, blk, 64 * t:64 * t + 64] = False
    elif defect == "last_key":
        for keep in (fwd_keep, bwd_keep, kv_keep):
            keep[..., n - 1] = False
    elif defect == "dq_tile":
        t = where.get("tile", _tile_of(p_exact[blk], n))
        bwd_keep[bb, hh, blk, 64 * t:64 * t + 64] = False
    elif defect == "dkdv_last_row":
        t = where.get("tile", _tile_of(p_exact[n - 1:n], n))
        kv_keep[bb, hh, n - 1, 64 * t:64 * t + 64] = False

    # forward
    sm = s.masked_fill(~fwd_keep, -math.inf)
    m = sm.max(-1, keepdim=True).values
    e = torch.exp(sm - m)
    l = e.sum(-1, keepdim=True)
    if defect == "denominator":          # one row's denominator misses 16 keys (by default the 16-key group with the largest share of it)
        row = where.get("row", n // 2)
        grp = e[bb, hh, row].clone()
        pad = (-n) % 16
        share = torch.cat([grp, grp.new_zeros(pad)]).view(-1, 16).sum(-1)
        key0 = where.get("key0", 16 * int(share.argmax()))
        l[bb, hh, row] = l[bb, hh, row] - e[bb, hh, row, key0:key0 + 16].sum()
    out = r16((r16(e) @ v) / l)
    lse = (m + torch.log(l)).squeeze(-1).float().double()
    if defect == "swap_rows":
        i, j = where.get("row", n - 2), n - 1
        out[bb, hh, [i, j]] = out[bb, hh, [j, i]]

    # backward (reads the forward's 16-bit out and fp32 lse, as the kernels do)
    p = torch.exp(s - lse[..., None])
    dp = (dout @ v.transpose(-1, -2)).float().double()
    delta = (dout * out).sum(-1, keepdim=True).float().double()
    ds16 = r16(p * (dp - delta))
    p16 = r16(p)
    dq = r16(scale * (ds16.masked_fill(~bwd_keep, 0.0) @ k))
    dk = r16(scale * (ds16.masked_fill(~kv_keep, 0.0).transpose(-1, -2) @ q))
    dv = r16(p16.masked_fill(~kv_keep, 0.0).transpose(-1, -2) @ dout)
    if defect == "dv_element":           # one element 25 % off (by default the largest of key row n / 3)
        row = n // 3
        col = int(dv[bb, hh, row].abs().argmax())
        row, col = where.get("elem", (row, col))
        dv[bb, hh, row, col] = r16(dv[bb, hh, row, col] * 1.25)
    return out, lse, dq, dk, dv


# ---------------------------------------------------------------------------------------------------------------- checking
def regime(n, row):
    """where a row sits: its 128-row and 64-row tile, whether it is the last row and whether that is the edge token"""
    last = row == n - 1
    edge = last and (n & 127) == 1 and n > 128
    seeded = last and (n & 63) == 1 and n > 64
    return (f"128-row tile {row >> 7} of {(n + 127) >> 7}, 64-row tile {row >> 6} of {(n + 63) >> 6}, row {row & 63} of it"
            + (", LAST row" if last else "") + (", the EDGE token" if edge else "") + (", the seeded key" if seeded and not edge else ""))


def units(got, ref, scale, u):
    """|got - ref| / (u scale) per element (float64); an element whose scale is 0 must be exact"""
    err = (got.double().cpu() - ref).abs()
    den = u * scale
    return torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def worst(got, ref, scale, u):
    """(the worst units, its index)"""
    un = units(got, ref, scale, u)
    flat = int(un.argmax())
    idx = []
    for size in reversed(un.shape):
        idx.append(flat % size)
        flat //= size
    return float(un.max()), tuple(reversed(idx))


def assert_within(got, ref, scale, K_, u, tag, quiet=False):
    """got, ref, scale [B, H, n, d].  Prints the worst element's error in units of u scale (one line per call), and fails, naming that
    element and its regime, when it exceeds K_.  Returns the worst units."""
    assert got.shape == ref.shape == scale.shape, (tag, got.shape, ref.shape, scale.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{tag}: non-finite values"
    w, (b, h, row, col) = worst(got, ref, scale, u)
    n = ref.shape[2]
    if not quiet:
        print(f"[attention-bounds] {tag}: worst {w:.2f} units of u*scale (K = {K_}) at (b {b}, h {h}, row {row}, col {col})")
    assert w <= K_, (f"{tag}: element (b {b}, h {h}, row {row}, col {col}) is off by {w:.2f} units of u*scale, the derived bound is K = {K_}; "
                     f"got {float(got[b, h, row, col]):.6g}, reference {float(ref[b, h, row, col]):.6g}, scale {float(scale[b, h, row, col]):.6g}; "
                     f"n = {n}: {regime(n, row)}")
    return w


def row_units(got, ref, scale, u, row):
    """the worst units within one row (the edge token's lines)"""
    return float(units(got[:, :, row], ref[:, :, row], scale[:, :, row], u).max())


def assert_lse(got, ref, tag, quiet=False):
    """got, ref [B, H, n]"""
    err = (got.double().cpu() - ref).abs()
    w = float(err.max())
    flat = int(err.argmax())
    n = ref.shape[2]
    b, h, row = flat // (ref.shape[1] * n), flat // n % ref.shape[1], flat % n
    if not quiet:
        print(f"[attention-bounds] {tag}: lse worst {w:.2e} (bar {LSE_BAR:.2e}) at (b {b}, h {h}, row {row})")
    assert w <= LSE_BAR, f"{tag}: lse of (b {b}, h {h}, row {row}) is off by {w:.3e} > {LSE_BAR:.3e}; n = {n}: {regime(n, row)}"
    return w


# ----------------------------------------------------------------------------- the criteria of tests/test_gpu_attention.py::check
def old_criteria_pass(res, ref):
    """The whole-tensor bars of tests/test_gpu_attention.py::check, copied: forward rel-L2 < 1e-2 and max-abs < 2e-2 of the largest
    entry; each gradient rel-L2 < 2e-2, and < 3e-2 for the last token alone.  res / ref: dicts of [B, H, n, d] tensors."""
    def rel_l2(a, b):
        a, b = a.double(), b.double()
        return float((a - b).norm() / b.norm().clamp_min(1e-3 * max(1.0, b.numel() ** 0.5)))
    ok = rel_l2(res["out"], ref["out"]) < 1e-2 and float((res["out"] - ref["out"]).abs().max() / ref["out"].abs().max()) < 2e-2
    for name in ("dq", "dk", "dv"):
        ok = ok and rel_l2(res[name], ref[name]) < 2e-2 and rel_l2(res[name][:, :, -1], ref[name][:, :, -1]) < 3e-2
    return ok
