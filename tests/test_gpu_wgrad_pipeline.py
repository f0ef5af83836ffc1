"""The 64-token pipeline of the weight-gradient tile body (csrc/gemm.hip wgrad_tile, docs/experiments.md R21.1) at every token count at
which its ring takes another path.

S = 64 tokens per barrier step (two 32-token DMA stages); the ring holds five stages = D = 2.5 steps = 160 tokens.  Token counts: one
stage and its neighbours (1, 31, 32, 33), one step (S - 1, S, S + 1), the ring (D S - 1, D S, D S + 1: the first refill of a slot),
(D + 1) S + 33 = 257 (past the first wrap, an odd number of stages -- the step padded with a stage of zeros -- and a ragged last stage)
and 513.  Products: one tile, two tiles, and nine products of mixed N, K in {256, 512} in one launch; bf16 and f16; standard normal
operands drawn on the CPU by tools/wgrad_bits.py.

Every result is held to 1e-5 of the largest entry of the float64 product of the rounded operands (the bar of test_gpu_fused.py and
test_gpu_wgrad_multiblock.py; a read of a stale ring slot is an O(1) error), to the bits of a second call, to the bits of the same
product through ew.wgrad where that runs unsliced, and to the bits of the commit BEFORE the pipeline: tests/golden/wgrad_bits_parent.json
is the output of tools/wgrad_bits.py on that commit (every accumulator still takes its 16-token groups in ascending token order, so
no bit may move).  The split-T form (ew.wgrad with 2 and 4 slices: arbitrary stage ranges, odd lengths) is held to the same bar, to
a second call and to the parent's bits."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

S, D = 64, 2.5
TOKENS = [1, 31, 32, 33, S - 1, S, S + 1, int(D * S) - 1, int(D * S), int(D * S) + 1, int((D + 1) * S) + 33, 513]
assert TOKENS == [1, 31, 32, 33, 63, 64, 65, 159, 160, 161, 257, 513]


def _tool():
    spec = importlib.util.spec_from_file_location("npcd_wgrad_bits", os.path.join(ROOT, "tools", "wgrad_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tool():
    return _tool()


@pytest.fixture(scope="module")
def parent_bits():
    with open(os.path.join(GOLDEN, "wgrad_bits_parent.json")) as f:
        return json.load(f)


def _within_bar(out, dy, x, what):
    ref = dy.cuda().double().t() @ x.cuda().double()
    err, big = float((out.double() - ref).abs().max()), float(ref.abs().max())
    print(f"{what}: max error {err:.3e}, largest entry {big:.3e}, ratio {err / big:.2e}")
    assert err <= 1e-5 * big, (what, err, big)


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_tile_body_at_every_path_of_the_ring(tool, parent_bits, dn, T):
    from npcd.hip import elementwise as ew
    todo = [c for c in tool.cases() if c[2] == T and c[3] == dn and c[1] != "sliced"]
    assert [c[1] for c in todo] == ["one", "n512", "group9"]
    for cid, kind, _, _, shapes, seed in todo:
        ops = tool.operands(T, shapes, tool.DTYPES[dn], seed)
        outs, again = tool.run(kind, ops), tool.run(kind, ops)
        assert len(outs) == len(shapes)
        for i, ((dy, x), out, out2) in enumerate(zip(ops, outs, again)):
            what = f"{cid}/{i}"
            _within_bar(out, dy, x, what)
            assert torch.equal(out, out2), (what, "second call differs")
            N, K = shapes[i]
            assert ew.lib().npcd_wgrad_slices(T, N, K) == 1
            single = torch.full_like(out, float("nan"))
            assert ew.wgrad(dy.cuda(), x.cuda(), single)
            assert torch.equal(out, single), (what, "differs from ew.wgrad")
            assert tool.digest(out) == parent_bits[what], (what, "not the bits of the parent commit")


@pytest.mark.parametrize("T", [1026, 2079])
@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_split_t_form_with_more_than_one_slice(tool, parent_bits, dn, T):
    from npcd.hip import elementwise as ew
    (cid, kind, _, _, shapes, seed), = [c for c in tool.cases() if c[2] == T and c[3] == dn]
    assert kind == "sliced" and shapes == ((256, 256),)
    assert ew.lib().npcd_wgrad_slices(T, 256, 256) > 1
    ops = tool.operands(T, shapes, tool.DTYPES[dn], seed)
    (out,), (out2,) = tool.run(kind, ops), tool.run(kind, ops)
    _within_bar(out, ops[0][0], ops[0][1], cid)
    assert torch.equal(out, out2), (cid, "second call differs")
    assert tool.digest(out) == parent_bits[f"{cid}/0"], (cid, "not the bits of the parent commit")
