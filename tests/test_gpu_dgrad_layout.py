"""The data gradients of the 16-bit fused backbone against a TRANSPOSED shadow of the Linear weights (fused.FusedBackboneEngine):
the grouped transpose kernel (csrc/gemm_nt.hip, npcd_transpose16_group), the product in its transposed form against the product on the
weight as stored (NPCD_DGRAD_NN), the freshness of the transposed shadow after every kind of write to the weights, and its storage.

Bound of every comparison of the two forms: relative L2 <= 2^-8.  Both forms round fp32 sums over the SAME 16-bit operands to bf16;
the sums differ only in their order, so an element moves by at most one bf16 ulp (2^-8 relative at the bottom of a binade) and most do
not move at all.  A stale or wrongly indexed transposed weight is off by tens of per cent."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -8
W, H, L, F_, N, B = 128, 2, 2, 8, 16, 3          # the tiny trainer: n = 17 token rows per example, T = 51


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.fixture(autouse=True)
def _transposed_at_every_size(monkeypatch):
    """the default takes the transposed form from fused._DGRAD_T_MIN_T token rows on; these tests run it at their small shapes"""
    from npcd.models.diffusion import fused
    monkeypatch.setattr(fused, "_DGRAD_T_MIN_T", 0)
    monkeypatch.setattr(fused, "_DGRAD_NN", False)


# ---- 1. the grouped transpose ------------------------------------------------------------------------------------------------------

BLOCK_W64 = [(192, 64), (64, 64), (256, 64), (64, 256)]          # the four Linear weights of a block at width 64
RAGGED = [(70, 33), (1, 129), (65, 8)]
# full 64 x 64 tiles with ONE side on 16-byte accesses: a row count / column count that is no multiple of 8 makes the store / load side
# narrow (the packed-dword LDS store against the 2-byte LDS read, and the reverse); both have a ragged edge tile as well
ONE_SIDE = [(68, 64), (64, 68), (132, 128), (128, 132)]


def _bits(shape, dtype, seed, odd):
    """(whole buffer as int16, view of `shape` inside it): random 16-bit patterns (every bit pattern, NaNs included: compared as
    integers); odd: the view starts at element 1 of the buffer, i.e. 2-byte alignment only; aligned: at element 8"""
    g = torch.Generator().manual_seed(seed)
    n = shape[0] * shape[1]
    buf = torch.randint(-32768, 32768, (n + 16,), generator=g, dtype=torch.int32).to(torch.int16).cuda()
    off = 1 if odd else 8
    v = buf[off:off + n].view(dtype).view(shape)
    assert v.data_ptr() % 16 == (2 if odd else 0)
    return buf, v


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd_offset"])
@pytest.mark.parametrize("shapes", [BLOCK_W64, RAGGED, ONE_SIDE], ids=["block_w64", "ragged", "one_side_wide"])
def test_grouped_transpose_is_bit_exact(shapes, odd, dtype):
    """ONE launch over all matrices of `shapes`; the elements of a destination's buffer around the view keep their values."""
    _check_transpose(shapes, dtype, odd, odd)


@pytest.mark.parametrize("odd_src,odd_dst", [(False, True), (True, False)], ids=["aligned_to_odd", "odd_to_aligned"])
def test_grouped_transpose_with_one_side_unaligned(odd_src, odd_dst):
    """the block's shapes with the source or the destination alone at an odd element offset: one side on 16-byte accesses"""
    _check_transpose(BLOCK_W64, torch.bfloat16, odd_src, odd_dst)


def _check_transpose(shapes, dtype, odd_src, odd):
    from npcd.hip import linear as hlin
    src = [_bits(s, dtype, 11 + i, odd_src)[1] for i, s in enumerate(shapes)]
    dst = [_bits((s[1], s[0]), dtype, 31 + i, odd) for i, s in enumerate(shapes)]
    before = [buf.clone() for buf, _ in dst]
    want = [s.view(torch.int16).t().contiguous() for s in src]
    hlin.transpose16_group([(s, d) for s, (_, d) in zip(src, dst)])
    torch.cuda.synchronize()
    off = 1 if odd else 8
    for s, (buf, d), w_, b in zip(shapes, dst, want, before):
        n = s[0] * s[1]
        assert torch.equal(d.view(torch.int16), w_), s
        assert torch.equal(buf[:off], b[:off]) and torch.equal(buf[off + n:], b[off + n:]), s


def test_grouped_transpose_rejects_what_it_does_not_take():
    from npcd.hip import linear as hlin
    a = torch.zeros(8, 4, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        hlin.transpose16_group([(a, torch.zeros(8, 4, device="cuda", dtype=torch.bfloat16))])           # out is not [C, R]
    with pytest.raises(RuntimeError):
        hlin.transpose16_group([(a, torch.zeros(4, 8, device="cuda", dtype=torch.float16))])            # two types
    with pytest.raises(RuntimeError):
        hlin.transpose16_group([(a, torch.zeros(4, 8, device="cuda", dtype=torch.bfloat16))] * 5)       # more than four


# ---- 2. _dgrad across the token split ----------------------------------------------------------------------------------------------

def test_dgrad_transposed_form_across_the_token_split(monkeypatch):
    """T = 320 = one 256-row call + 64 left-over rows (fused._SPLIT_MIN = 0): both calls read the transposed weight."""
    from npcd.hip import linear as hlin
    from npcd.models.diffusion import fused
    monkeypatch.setattr(fused, "_SPLIT_MIN", 0)
    calls = []
    real = fused._split_gemm
    monkeypatch.setattr(fused, "_split_gemm", lambda fn, T, N=0: real(lambda r: (calls.append((r.start, r.stop)), fn(r))[1], T, N))
    g = torch.Generator().manual_seed(5)
    T = 320
    for (Nw, Kw) in BLOCK_W64:
        dy = torch.randn(T, Nw, generator=g).cuda().bfloat16()
        w = (torch.randn(Nw, Kw, generator=g) * 0.1).cuda().bfloat16()
        wT = torch.empty(Kw, Nw, device="cuda", dtype=torch.bfloat16)
        hlin.transpose16_group([(w, wT)])
        del calls[:]
        got = fused._dgrad(dy, w, wT)
        assert calls == [(0, 256), (256, 320)]
        nn = fused._dgrad(dy, w)
        ref = dy.double() @ w.double()
        torch.cuda.synchronize()
        e_form, e_t, e_nn = rel(got, nn), rel(got, ref), rel(nn, ref)
        print(f"dgrad {Nw}x{Kw}: transposed vs NN {e_form:.3e}, vs fp64 {e_t:.3e} (NN vs fp64 {e_nn:.3e})")
        assert e_form <= BOUND, (Nw, Kw, e_form)
        assert e_t <= BOUND and e_nn <= BOUND, (Nw, Kw, e_t, e_nn)       # (each is ONE bf16 rounding of the exact product: 2^-9 at most)


# ---- 3.-5. engine level ------------------------------------------------------------------------------------------------------------

def _trainer(seed=3):
    from oracle import denoiser as od
    from npcd.models.diffusion import DiffusionModel
    from npcd.train import DiffusionTrainer
    p = od.init_params(3, F_, W, L, H, seed=seed)
    g = torch.Generator().manual_seed(17)
    for k in p:
        if k.endswith(".bias"):
            p[k] = p[k] + torch.randn(p[k].shape, generator=g) * 0.05
    m = DiffusionModel(3, F_, N, W, L, H, True)
    m.denoiser.load_state_dict(p)
    m = m.cuda().train()
    tr = DiffusionTrainer(m, lr=1e-3, weight_decay=0.01, ema_decay=0.999, dtype=torch.bfloat16)
    assert tr.native and m.denoiser.backbone.fused_engine is not None
    return tr, p


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 3, N, generator=g).cuda(), torch.randn(B, F_, N, generator=g).cuda(), torch.randint(0, 1000, (B,), generator=g).cuda(),
            torch.randn(B, 3, N, generator=g).cuda(), torch.randn(B, F_, N, generator=g).cuda())


def _node(tr, x, gout, nn, monkeypatch):
    """one forward + backward of the fused backbone node: (input gradient, {block parameter gradient name: clone})"""
    from npcd.models.diffusion import fused
    monkeypatch.setattr(fused, "_DGRAD_NN", nn)
    eng = tr.model.denoiser.backbone.fused_engine
    tr.flat.zero_grad()
    tr.reducer.start_step()
    xin = x.clone().requires_grad_(True)
    eng(xin).backward(gout)
    torch.cuda.synchronize()
    grads = {f"{bi}.{k}": v.clone() for bi, e in enumerate(eng.blocks) for k, v in e.items() if k.endswith("_g")}
    monkeypatch.setattr(fused, "_DGRAD_NN", False)
    return xin.grad.clone(), grads


def _compare(tr, x, gout, monkeypatch, what):
    dx_t, g_t = _node(tr, x, gout, False, monkeypatch)
    dx_n, g_n = _node(tr, x, gout, True, monkeypatch)
    errs = {"dx": rel(dx_t, dx_n), **{k: rel(g_t[k], g_n[k]) for k in g_n}}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{what}: worst transposed-vs-NN rel-L2 {worst[1]:.3e} ({worst[0]})")
    assert len(g_n) == 12 * L and all(float(v.abs().sum()) > 0 for v in g_n.values())
    assert worst[1] <= BOUND, (what, errs)


def _xg(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N + 1, W, generator=g).cuda(), torch.randn(B, N + 1, W, generator=g).cuda()


def test_engine_gradients_match_the_nn_form(monkeypatch):
    tr, _ = _trainer()
    eng = tr.model.denoiser.backbone.fused_engine
    x, gout = _xg(7)
    _compare(tr, x, gout, monkeypatch, "tiny trainer")
    assert eng.transposed_refreshes == L
    for e in eng.blocks:
        for k in ("attn_c_qkv", "attn_c_proj", "mlp_c_fc", "mlp_c_proj"):
            assert torch.equal(e[k + "_weight_16T"], e[k + "_weight_16"].t())
    tr.close()


def test_transposed_shadow_follows_every_write_to_the_weights(monkeypatch):
    tr, params = _trainer()
    eng = tr.model.denoiser.backbone.fused_engine
    x, gout = _xg(8)
    _compare(tr, x, gout, monkeypatch, "initial state")
    count = eng.transposed_refreshes
    assert count == L
    _node(tr, x, gout, False, monkeypatch)                 # two more backwards, no shadow write between them: nothing is transposed
    _node(tr, x, gout, False, monkeypatch)
    assert eng.transposed_refreshes == count

    tr.step(*_batch(100))                                  # the optimizer pass writes the shadow (the step's own forward came before it)
    count = eng.transposed_refreshes
    _compare(tr, x, gout, monkeypatch, "after trainer.step")
    assert eng.transposed_refreshes == count + L

    other = {k: v * 1.5 + 0.01 for k, v in params.items()}
    tr.model.denoiser.load_state_dict(other)
    count = eng.transposed_refreshes
    _compare(tr, x, gout, monkeypatch, "after load_state_dict")
    assert eng.transposed_refreshes == count + L

    with torch.no_grad():
        tr.model.denoiser.backbone.resblocks[1].mlp.c_fc.weight.mul_(2)
    count = eng.transposed_refreshes
    _compare(tr, x, gout, monkeypatch, "after an in-place write")
    assert eng.transposed_refreshes == count + L
    e = eng.blocks[1]
    assert torch.equal(e["mlp_c_fc_weight_16T"], e["mlp_c_fc_weight_16"].t())
    assert torch.equal(e["mlp_c_fc_weight_16"].float(), e["mlp_c_fc_weight"].bfloat16().float())
    tr.close()


def test_transposed_shadow_is_not_an_arena_buffer():
    tr, _ = _trainer()
    eng = tr.model.denoiser.backbone.fused_engine
    assert eng.arena is not None and eng._shadowT is None          # (allocated by the first refresh)
    tr.step(*_batch(199))
    before = eng._shadowT.data_ptr()
    for i in range(2):
        tr.step(*_batch(200 + i))
    torch.cuda.synchronize()
    assert len(eng.arena.slots) > 0 and eng.arena.hits > 0          # the arena is active at this token count
    held = {s.untyped_storage().data_ptr() for s in eng.arena.slots}
    own = eng._shadowT.untyped_storage().data_ptr()
    assert own not in held and eng._shadowT.data_ptr() == before
    for e in eng.blocks:
        for k in ("attn_c_qkv", "attn_c_proj", "mlp_c_fc", "mlp_c_proj"):
            assert e[k + "_weight_16T"].untyped_storage().data_ptr() == own
    tr.close()
