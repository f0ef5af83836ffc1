"""The weight-gradient scheduler of the 16-bit backward (fused._WgradSchedule) in its two main-stream modes, driven the way
_BackboneFn._backward drives it -- per block four add() in the order mlp.c_proj, mlp.c_fc, attn.c_proj, attn.c_qkv, then
block_done(bi), from the last block down, then finish() -- with recorders in place of fused._wgrad, ew.wgrad_group and the
reducer.  The operands are placeholders; the whole event list is asserted literally.  No GPU."""
import pytest

from npcd.hip import elementwise as ew
from npcd.models.diffusion import fused

PRODUCTS = ("mlp.c_proj", "mlp.c_fc", "attn.c_proj", "attn.c_qkv")


class _Reducer:
    def __init__(self, events, active=True):
        self.events, self.active = events, active

    def mark_ready(self, p):
        self.events.append(("ready", p))


class _Engine:
    """what the scheduler reads of an engine: per block its parameters (here: the block's number, once), and the reducer"""

    def __init__(self, L, reducer):
        self.blocks = [{"params": [bi]} for bi in range(L)]
        self.reducer = reducer


def _triple(bi, name):
    return (("dy", bi, name), ("x", bi, name), ("out", bi, name))


def _singles(bi):
    return [("single", _triple(bi, name)) for name in PRODUCTS]


def _drive(monkeypatch, L, group, reducer="recording", group_accepts=True):
    """-> (events, per block_done a copy of the events so far, the scheduler); the queues are checked after every block_done"""
    events = []

    def group_call(triples):
        events.append(("group", list(triples)))
        return group_accepts
    monkeypatch.setattr(fused, "_wgrad", lambda dy, x, out: events.append(("single", (dy, x, out))))
    monkeypatch.setattr(ew, "wgrad_group", group_call)
    red = {"recording": _Reducer(events), "inactive": _Reducer(events, active=False), None: None}[reducer]
    sched = fused._WgradSchedule(_Engine(L, red), 34, 256, None, None, side=False, group=group)
    after = {}
    for bi in range(L - 1, -1, -1):
        for name in PRODUCTS:
            sched.add(*_triple(bi, name))
        launched = len(events)
        sched.block_done(bi)
        after[bi] = list(events)
        if len(events) > launched:              # a block_done that launched holds no operand any more
            assert sched.queue == [] and sched.waiting == [], bi
    held = len(sched.queue)
    sched.finish()
    assert len(events) == len(after[0]) and held == 0, "finish() adds nothing on the main stream, and nothing is left queued"
    return events, after, sched


def test_direct_three_blocks(monkeypatch):
    events, _, _ = _drive(monkeypatch, 3, 0)
    assert events == (_singles(2) + [("ready", 2)] + _singles(1) + [("ready", 1)] + _singles(0) + [("ready", 0)])


@pytest.mark.parametrize("reducer", [None, "inactive"])
def test_direct_without_a_reducing_reducer(monkeypatch, reducer):
    events, _, _ = _drive(monkeypatch, 3, 0, reducer=reducer)
    assert events == _singles(2) + _singles(1) + _singles(0)


def _group_of(blocks):
    return [_triple(bi, name) for bi in blocks for name in PRODUCTS]


def test_multiblock_six_blocks_in_groups_of_four(monkeypatch):
    events, after, _ = _drive(monkeypatch, 6, 4)
    assert after[5] == after[4] == after[3] == []                    # nothing before block 2 is done
    launch = [("group", _group_of((5, 4, 3, 2))), ("ready", 5), ("ready", 4), ("ready", 3), ("ready", 2)]
    assert after[2] == launch
    assert after[1] == launch + _singles(1) + [("ready", 1)]
    assert events == launch + _singles(1) + [("ready", 1)] + _singles(0) + [("ready", 0)]
    assert len(events[0][1]) == 16


def test_multiblock_group_call_declines(monkeypatch):
    events, after, _ = _drive(monkeypatch, 6, 4, group_accepts=False)
    assert after[3] == []
    fallback = [("single", t) for t in _group_of((5, 4, 3, 2))]
    assert len(fallback) == 16
    assert events == ([("group", _group_of((5, 4, 3, 2)))] + fallback + [("ready", 5), ("ready", 4), ("ready", 3), ("ready", 2)]
                      + _singles(1) + [("ready", 1)] + _singles(0) + [("ready", 0)])


def test_multiblock_no_tail(monkeypatch):
    events, after, _ = _drive(monkeypatch, 4, 4)
    assert after[1] == []
    assert events == [("group", _group_of((3, 2, 1, 0))), ("ready", 3), ("ready", 2), ("ready", 1), ("ready", 0)]


def test_multiblock_all_tail_equals_direct(monkeypatch):
    events, _, _ = _drive(monkeypatch, 3, 4)
    direct, _, _ = _drive(monkeypatch, 3, 0)
    assert events == direct == (_singles(2) + [("ready", 2)] + _singles(1) + [("ready", 1)] + _singles(0) + [("ready", 0)])


def test_multiblock_without_a_reducing_reducer(monkeypatch):
    events, _, _ = _drive(monkeypatch, 6, 4, reducer=None)
    assert events == [("group", _group_of((5, 4, 3, 2)))] + _singles(1) + _singles(0)
