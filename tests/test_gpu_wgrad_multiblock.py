"""The multi-block weight-gradient launch (round 18): npcd_wgrad_group with up to 16 products -- the four Linear layers of four residual
blocks in one launch, a workgroup per 256 x 256 tile over all token rows -- and the engine path that queues the (dy, x, out) triples of
G blocks for it (fused._WgradSchedule, NPCD_WGRAD_MULTIBLOCK).

Kernel level: 9 and 16 products (past the old limit of 8) with mixed N, K in {256, 512} over ragged token ranges (T = 33 is shorter than
the LDS ring's three-stage prologue; none is a multiple of 8, so the zero page of dma_subtile serves rows) against the single-product
launch (same tile body, same summation order: the same bits), against a second call, and against the float64 product of the rounded
operands (the bar of test_gpu_fused.py::test_grouped_weight_gradient_launch: 1e-5 of the largest entry); 17 products are an argument
error.

Engine level: a tiny trainer of 6 blocks (one group of four and a tail of two), switch on against switch off."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]


def _triples(count, T, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(count):
        N, K = (256, 512)[i % 2], (256, 512)[(i // 2 + i // 5) % 2]          # every (N, K) of {256, 512}^2 occurs among the first nine
        dy = torch.randn(T, N, generator=g).to(dtype).cuda()
        x = torch.randn(T, K, generator=g).to(dtype).cuda()
        out.append((dy, x, torch.full((N, K), float("nan"), device="cuda")))
    return out


@pytest.mark.parametrize("T", [33, 100, 513])
@pytest.mark.parametrize("count", [9, 16])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_more_than_eight_products_in_one_launch(count, T, dtype):
    from npcd.hip import elementwise as ew
    trip = _triples(count, T, dtype, seed=1000 * count + T)
    assert {(t[0].shape[1], t[1].shape[1]) for t in trip} == {(256, 256), (256, 512), (512, 256), (512, 512)}
    assert ew.wgrad_group(trip)
    again = [(dy, x, torch.full_like(out, float("nan"))) for dy, x, out in trip]
    assert ew.wgrad_group(again)
    for i, ((dy, x, out), (_, _, out2)) in enumerate(zip(trip, again)):
        one = torch.full_like(out, float("nan"))
        assert ew.wgrad_group([(dy, x, one)])
        assert torch.equal(out, one), (i, "differs from the single-product launch")
        assert torch.equal(out, out2), (i, "second call differs")
        ref = dy.double().t() @ x.double()
        err, big = float((out.double() - ref).abs().max()), float(ref.abs().max())
        assert err <= 1e-5 * big, (i, err, big)


def test_seventeen_products_are_an_argument_error():
    from npcd.hip import elementwise as ew
    from npcd.hip import lib, ptr, stream_ptr
    trip = _triples(17, 33, torch.bfloat16, seed=17)
    assert not ew.wgrad_group(trip)                          # the wrapper declines: the caller's per-product path
    n = len(trip)
    P, I = ctypes.c_void_p * n, ctypes.c_int * n
    rc = lib().npcd_wgrad_group(n, P(*[ptr(t[0]) for t in trip]), P(*[ptr(t[1]) for t in trip]), P(*[ptr(t[2]) for t in trip]),
                                I(*[t[0].shape[1] for t in trip]), I(*[t[1].shape[1] for t in trip]), 33, 0, stream_ptr())
    assert rc == -1                                          # NPCD_ERR_ARG
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t[2]).all()) for t in trip)  # nothing was launched


def test_fill_rule_on_this_device_matches_its_mirror():
    from npcd.hip import elementwise as ew
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for tiles in (12, 48, 192, 768):
        assert ew.lib().npcd_wgrad_group_blocks(tiles, 16, 4) == ew.wgrad_group_blocks_rule(tiles, 16, 4, cus), (tiles, cus)
    assert ew.lib().npcd_wgrad_group_blocks(192, 64, 4) == ew.wgrad_group_blocks_rule(192, 16, 4, cus)      # the kernel's limit caps it


# ---- engine level ----------------------------------------------------------------------------------------------------------------
W, H, L, F_, N, B = 256, 4, 6, 32, 16, 2
T = B * (N + 1)
WGRAD_NAMES = [f"backbone.resblocks.{i}.{n}.weight" for i in range(L) for n in ("attn.c_qkv", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")]


def _trainer(dtype):
    from oracle import denoiser as od
    from npcd.models.diffusion import DiffusionModel
    from npcd.train import DiffusionTrainer
    p = od.init_params(3, F_, W, L, H, seed=3)
    g = torch.Generator().manual_seed(17)
    for k in p:                                   # non-trivial biases and LayerNorm affines (the synthetic init has zeros and ones)
        if k.endswith(".bias"):
            p[k] = p[k] + torch.randn(p[k].shape, generator=g) * 0.05
        elif ".ln_" in k or k.startswith("ln_"):
            p[k] = p[k] + torch.randn(p[k].shape, generator=g) * 0.1
    m = DiffusionModel(3, F_, N, W, L, H, True)
    m.denoiser.load_state_dict(p)
    m = m.cuda().train()
    tr = DiffusionTrainer(m, lr=7e-5, weight_decay=0.01, ema_decay=0.9999, dtype=dtype)
    assert tr.native and m.denoiser.backbone.fused_engine is not None
    return tr


def _backward(tr, dtype, zero=True):
    """one forward + backward of the denoiser under autocast: ({name: gradient}, the gradient of the feature input)"""
    g = torch.Generator().manual_seed(5)
    coords, feats = torch.randn(B, 3, N, generator=g).cuda(), (torch.rand(B, F_, N, generator=g) * 2 - 1).cuda().requires_grad_(True)
    t = torch.randint(0, 1000, (B,), generator=g).cuda()
    gc, gf = torch.randn(B, 3, N, generator=g).cuda(), torch.randn(B, F_, N, generator=g).cuda()
    if zero:
        tr.flat.zero_grad()
    tr.reducer.start_step()
    den = tr.model.denoiser
    with torch.autocast("cuda", dtype=dtype):
        ec, ef = den(coords, feats, t)
        loss = (ec.float() * gc).sum() + (ef.float() * gf).sum()
    loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.clone() for n, p in den.named_parameters()}, feats.grad.clone()


@pytest.fixture()
def multiblock(monkeypatch):
    """NPCD_WGRAD_MULTIBLOCK=force, NPCD_WGRAD_MULTIBLOCK_MIN_T=0, side stream off -- as the module parsed them"""
    from npcd.models.diffusion import fused
    monkeypatch.setattr(fused, "_WGRAD_STREAM", False)
    monkeypatch.setattr(fused, "_WGRAD_MULTIBLOCK", "force")
    monkeypatch.setattr(fused, "_WGRAD_MULTIBLOCK_MIN_T", 0)
    return fused


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_engine_one_group_of_four_blocks_and_a_tail_of_two(multiblock, monkeypatch, dtype):
    """Switch on against off: one grouped call with 16 triples and eight per-product calls for the two tail blocks; every gradient
    that is not a Linear weight of a block (the input gradient, biases, LayerNorm affines, everything outside the backbone) is the
    same bits -- the critical path did not change; the 24 Linear weight gradients are two fp32 summation orders over the same 16-bit
    operands, held to the bounds tests/test_gpu_rank_step.py states for grouped against library (rel-L2 <= 2e-6, max-abs <= 4e-6 of
    the largest entry); a second backward with no optimizer step in between overwrites them with the same bits."""
    from npcd.hip import elementwise as ew
    fused = multiblock
    tr = _trainer(dtype)
    real_group, real_wgrad, groups, singles = ew.wgrad_group, fused._wgrad, [], []

    def counted_group(triples):
        ok = real_group(triples)
        groups.append((len(triples), ok))
        return ok

    def counted_wgrad(dy, x, out):
        singles.append(tuple(out.shape))
        return real_wgrad(dy, x, out)
    monkeypatch.setattr(ew, "wgrad_group", counted_group)
    monkeypatch.setattr(fused, "_wgrad", counted_wgrad)
    on, dfeat_on = _backward(tr, dtype)
    assert groups == [(16, True)], groups
    assert len(singles) == 8, singles
    second, _ = _backward(tr, dtype, zero=False)
    assert all(torch.equal(on[n], second[n]) for n in WGRAD_NAMES), "a second backward changed the weight gradients"
    del groups[:], singles[:]
    monkeypatch.setattr(fused, "_WGRAD_MULTIBLOCK", "off")
    off, dfeat_off = _backward(tr, dtype)
    assert groups == [] and len(singles) == 4 * L
    assert set(WGRAD_NAMES) < set(on) == set(off)
    assert torch.equal(dfeat_on, dfeat_off)
    for n in on:
        a, b = on[n], off[n]
        assert float(b.abs().max()) > 0, n
        if n not in WGRAD_NAMES:
            assert torch.equal(a, b), (n, "not the same bits")
            continue
        r = float((a.double() - b.double()).norm() / b.double().norm())
        m = float((a - b).abs().max() / b.abs().max())
        print(f"multi-block vs library {dtype} {n}: rel-L2 {r:.3e} max-abs/max {m:.3e}")
        assert r <= 2e-6 and m <= 4e-6, (n, r, m)
    tr.close()


def test_engine_hands_blocks_to_the_reducer_behind_their_launch(multiblock, monkeypatch):
    """With a recording stand-in for the reducer: no mark_ready of a block of the group precedes the grouped call that writes its
    weight gradients, and blocks are handed over in descending order."""
    from npcd.hip import elementwise as ew
    tr = _trainer(torch.bfloat16)
    eng = tr.model.denoiser.backbone.fused_engine
    block_of = {id(p): bi for bi, e in enumerate(eng.blocks) for p in e["params"]}
    events = []

    class Recorder:
        active = True

        def mark_ready(self, p):
            events.append(("ready", block_of[id(p)]))
    real = ew.wgrad_group

    def recorded(triples):
        outs = {t[2].data_ptr() for t in triples}
        events.append(("group", sorted(bi for bi, e in enumerate(eng.blocks) if e["mlp_c_fc_weight_g"].data_ptr() in outs)))
        return real(triples)
    monkeypatch.setattr(ew, "wgrad_group", recorded)
    monkeypatch.setattr(eng, "reducer", Recorder())
    _backward(tr, torch.bfloat16)
    launches = [i for i, ev in enumerate(events) if ev[0] == "group"]
    assert len(launches) == 1 and events[launches[0]][1] == [2, 3, 4, 5], events
    ready = [(i, ev[1]) for i, ev in enumerate(events) if ev[0] == "ready"]
    assert sorted({b for _, b in ready}) == list(range(L))
    assert all(i > launches[0] for i, b in ready if b >= 2), events
    order = [b for _, b in ready]
    assert order == sorted(order, reverse=True), order
    tr.close()


@pytest.mark.parametrize("join_per_block", [False, True], ids=["handover", "join"])
def test_side_stream_hands_blocks_to_the_reducer_behind_their_launch(monkeypatch, join_per_block):
    """The side stream (the module's default at this size), with the hand-over from the side stream and with the per-block join: one
    grouped call per block, from the last block down, each with that block's four outputs; block b >= 1 is handed to the reducer
    behind its own call and ahead of the call of block b - 1, block 0 last of all, in descending order."""
    from npcd.hip import elementwise as ew
    from npcd.models.diffusion import fused
    assert fused._wgrad_side_ok(T) and fused._WGRAD_GROUP and T <= fused._WGRAD_GROUP_MAX_T
    monkeypatch.setattr(fused, "_JOIN_PER_BLOCK", join_per_block)
    tr = _trainer(torch.bfloat16)
    eng = tr.model.denoiser.backbone.fused_engine
    block_of = {id(p): bi for bi, e in enumerate(eng.blocks) for p in e["params"]}
    outs_of = [sorted(e[k + "_weight_g"].data_ptr() for k in ("attn_c_qkv", "attn_c_proj", "mlp_c_fc", "mlp_c_proj")) for e in eng.blocks]
    events = []

    class Recorder:
        active = True

        def mark_ready(self, p):
            events.append(("ready", block_of[id(p)]))
    real = ew.wgrad_group

    def recorded(triples):
        events.append(("group", outs_of.index(sorted(t[2].data_ptr() for t in triples))))
        return real(triples)
    monkeypatch.setattr(ew, "wgrad_group", recorded)
    monkeypatch.setattr(eng, "reducer", Recorder())
    _backward(tr, torch.bfloat16)
    launch = {ev[1]: i for i, ev in enumerate(events) if ev[0] == "group"}
    assert [ev[1] for ev in events if ev[0] == "group"] == [5, 4, 3, 2, 1, 0], events
    ready = [(i, ev[1]) for i, ev in enumerate(events) if ev[0] == "ready"]
    assert sorted({b for _, b in ready}) == list(range(L)) and len(ready) == 12 * L
    for i, b in ready:
        assert i > launch[b], (b, events)
        if b >= 1:
            assert i < launch[b - 1], (b, events)
    assert all(ev == ("ready", 0) for ev in events[launch[0] + 1:]) and len(events) == launch[0] + 1 + 12
    order = [b for _, b in ready]
    assert order == sorted(order, reverse=True), order
    tr.close()
