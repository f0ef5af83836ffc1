"""Explicit forward/backward of the transformer backbone for the MI355X training step.

One autograd node for all L residual blocks (reference ResidualAttentionBlock, transformer.py:140-172)
instead of ~40 autograd nodes per block:
  * activations are saved explicitly, the backward is written out by hand;
  * GEMMs are hipBLASLt calls on a bf16 shadow copy of the flat fp32 parameter buffer (no per-step
    weight casts); weight gradients are produced in fp32 straight into the flat gradient buffer;
  * residual add + LayerNorm + cast, LayerNorm backward (+ bias-gradient column sums), GELU fwd/bwd are
    single HIP kernels (csrc/elementwise.hip); attention is csrc/attention.hip;
  * gradients never pass through AccumulateGrad; the gradient reducer is told explicitly when a
    block's gradients are final so the RCCL all-reduce overlaps with the rest of backward.
Numerics follow the reference's bf16-autocast step: bf16 GEMM inputs with fp32 accumulation, fp32
residual stream, fp32 LayerNorm statistics, exact-erf GELU.
"""
import contextlib
import math
import os

import torch

from ...hip import arena as harena
from ...hip import attention as hattn
from ...hip import elementwise as ew
from ...hip import linear as hlin

_bf16, _f32 = torch.bfloat16, torch.float32
_BLOCK_PARAMS = ("ln_1.weight", "ln_1.bias", "attn.c_qkv.weight", "attn.c_qkv.bias", "attn.c_proj.weight", "attn.c_proj.bias",
                 "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
_LINEARS = ("attn_c_qkv", "attn_c_proj", "mlp_c_fc", "mlp_c_proj")          # the four Linear layers of a block, in parameter order
_NULL = contextlib.nullcontext()


# ---- the switches: every environment variable this module reads, read once, here (README "Environment switches") --------------------
# They exist for A/B measurements; what each one selects, and what was measured, stands next to the code that uses it.
def _env_on(name):
    """An on/off switch that is off by default: unset, "" and "0" are off, anything else is on."""
    return os.environ.get(name, "") not in ("", "0")


def _env_not_off(name):
    """An on/off switch that is on by default: "0" is off, anything else (unset and "" too) is on."""
    return os.environ.get(name, "") != "0"


def _env_int(name, default):
    """An integer from the environment (unset: the default); anything that is no integer raises a ValueError that names the variable."""
    try:
        return int(os.environ.get(name, default))
    except ValueError:
        raise ValueError(f"{name}={os.environ[name]!r}: expected an integer") from None


def _parse_wgrad_stream(value):
    """NPCD_WGRAD_STREAM -> (enabled, max token rows): unset = on below 20,000 rows, "0" = off, "1" = on at every size, any other
    integer = on up to that many rows.  Parsed ONCE, here (it had been read twice with two meanings).  Anything else
    raises a ValueError that names the variable."""
    if value is None or value == "":
        return True, 20000
    if value == "0":
        return False, 0
    if value == "1":
        return True, 1 << 62
    try:
        return True, int(value)
    except ValueError:
        raise ValueError(f"NPCD_WGRAD_STREAM={value!r}: expected unset, 0 (off), 1 (on at every size) or a token-row limit") from None


def _parse_wgrad_multiblock(value):
    """NPCD_WGRAD_MULTIBLOCK -> "on" (unset, "", "1"), "off" ("0") or "force"; anything else raises a ValueError that names the
    variable.  Parsed once, here."""
    modes = {None: "on", "": "on", "1": "on", "0": "off", "force": "force"}
    if value not in modes:
        raise ValueError(f"NPCD_WGRAD_MULTIBLOCK={value!r}: expected unset, 0 (off), 1 (on) or force (skip the fill rule)")
    return modes[value]


# the token-dimension split of the forward / data-gradient GEMMs (_split_gemm)
_SPLIT = 0 if _env_on("NPCD_NO_GEMM_SPLIT") else 256
_SPLIT_MIN = _env_int("NPCD_GEMM_SPLIT_MIN", 16000)
_SPLIT_BIG_FIRST = not _env_on("NPCD_GEMM_SPLIT_SMALL_FIRST")
_SPLIT_WIDE_N = _env_int("NPCD_GEMM_SPLIT_WIDE_N", 4096)
# attn.c_proj at a rank's token count on the own 128 x 128-tile kernel (_linear)
_LIN128 = not _env_on("NPCD_NO_LIN128")
_LIN128_MAX_T = _env_int("NPCD_LIN128_MAX_T", 4200)
# the data gradients: the transposed weight shadow (FusedBackboneEngine), the own mlp.c_proj product with the GELU backward (_own_dgelu)
_DGRAD_NN = _env_on("NPCD_DGRAD_NN")
_DGRAD_T_MIN_T = _env_int("NPCD_DGRAD_T_MIN_T", 16000)
_OWN_DGELU = _env_on("NPCD_OWN_DGELU")
_ATTN_COLSUM = not _env_on("NPCD_NO_ATTN_COLSUM")     # c_qkv bias gradient from the attention backward itself
# one weight-gradient product (_wgrad)
_OWN_WGRAD = _env_on("NPCD_OWN_WGRAD")
_SUM_KERNEL = not _env_on("NPCD_NO_SUM_KERNEL")       # the weight-gradient partials summed by csrc/elementwise.hip
# where and when the weight gradients of the 16-bit backward are issued (_WgradSchedule)
_WGRAD_STREAM, _WGRAD_STREAM_MAX_T = _parse_wgrad_stream(os.environ.get("NPCD_WGRAD_STREAM"))
_WGRAD_STREAM_PRIO = _env_int("NPCD_WGRAD_STREAM_PRIO", 0)
_WGRAD_GROUP = _env_not_off("NPCD_WGRAD_GROUP")
_WGRAD_GROUP_MAX_T = _env_int("NPCD_WGRAD_GROUP_MAX_T", 17000)
_JOIN_PER_BLOCK = _env_on("NPCD_WGRAD_JOIN_PER_BLOCK")
_WGRAD_MULTIBLOCK = _parse_wgrad_multiblock(os.environ.get("NPCD_WGRAD_MULTIBLOCK"))
_WGRAD_MULTIBLOCK_MIN_T = _env_int("NPCD_WGRAD_MULTIBLOCK_MIN_T", 20000)
# the step arena of the 16-bit node (FusedBackboneEngine)
_STEP_ARENA = _env_not_off("NPCD_STEP_ARENA")
_STEP_ARENA_MAX_T = _env_int("NPCD_STEP_ARENA_MAX_T", 20000)
# the form of the fp32-class weight gradients (_BackboneX2Fn)
_X2_WGRAD = os.environ.get("NPCD_X2_WGRAD", "library")
if _X2_WGRAD not in ("library", "own"):
    raise ValueError(f"NPCD_X2_WGRAD={_X2_WGRAD!r}: expected library or own")
# ---- end of the switches ------------------------------------------------------------------------------------------------------------


# ---- token-dimension split of the forward / data-gradient GEMMs ---------------------------------------------------------------
# The token count of a step is B x (N + 1): the time token makes it 64 x 513 = 32,832 = 128.25 tiles of 256 rows, and hipBLASLt
# loses 12 % on that quarter tile (tools/probes/gpu_dev_gemm_m.py: 1683 -> 1475 us per block for the eight GEMMs).  A GEMM does not
# care which rows it gets, so every [T, K] x [K, N] product is issued as one call on the last T % 256 rows and one on the rest.
# Measured in situ (same box, tuned solutions for both): 10.78 -> 11.13 steps/s.  (Tried: the small call on a second stream --
# its workgroups queue behind the large GEMM's and the join waits for them: no gain at either stream priority.  Tried: a
# hand-written kernel for the 64 left-over rows of the forward -- one pass over the weights straight into MFMA fragments,
# split-K over 8 waves: 11.5 us per call in situ against the tuned library's 12.8 us, 0.2-0.5 % of a step; both are bound by
# pulling 2-8 MB of cold weights through a launch that is over before it has filled the chip.  Not kept.)  NPCD_NO_GEMM_SPLIT=1: no
# split; NPCD_GEMM_SPLIT_MIN: the token rows from which every product is split.
# Below _SPLIT_MIN only the products whose OUTPUT is at least _SPLIT_WIDE_N wide are split (round 5, R5.18): at T = 4,104 / 8,208 the
# left-over row of 256-row tiles turns the 4,096-wide products (c_fc forward, mlp.c_proj data gradient) from 256 / 512 tiles = one / two
# full rounds into 272 / 528.  Same box, alternating processes: a rank's step at per-GPU batch 8 18.51-18.57 -> 18.18-18.36 ms, at 16
# 28.71-28.75 -> 27.96-27.99 ms; with 3,072 (c_qkv too) 18.34.  NPCD_GEMM_SPLIT_WIDE_N=0 switches it off.
def _split_gemm(fn, T, N=0):
    """fn(rows) enqueues the product for a row range into a shared output."""
    # below ~16 k tokens the large call is short enough that the extra launch costs what the quarter tile did (measured at
    # per-GPU batch 8 and 16: 19.9 vs 20.2 ms and 30.8 vs 31.1 ms per step; at per-GPU batch 32 the split wins: 50.4 -> 48.9 ms)
    wide = _SPLIT_WIDE_N > 0 and N >= _SPLIT_WIDE_N and T > _SPLIT
    Tm = T - T % _SPLIT if (_SPLIT and (T >= _SPLIT_MIN or wide)) else T
    if Tm == 0 or Tm == T:
        fn(slice(0, T))
        return
    # the left-over rows go BEHIND the large call: they then find the weights in L2 / MALL (82.08 against 82.32 ms per step, two
    # alternating rounds, tools/run_split_order_ab.sh; NPCD_GEMM_SPLIT_SMALL_FIRST=1 restores the old order)
    big, rest = slice(0, Tm), slice(Tm, T)
    for rows in ((big, rest) if _SPLIT_BIG_FIRST else (rest, big)):
        fn(rows)


# The token counts of one rank of a 4- / 8-GPU job (8,208 / 4,104 rows): the square product of the block (attn.c_proj, N = K = 1,024:
# 64-68 tiles of 256 x 256 for 256 CUs in the library's form) goes to the own 128 x 128-tile kernel, which measured 1.3 x the tuned
# library there (17.6-18.1 against 23-29 us at T = 4,104; docs/experiments.md R4.7) and loses on every other shape of the block --
# selected by shape (up to _LIN128_MAX_T rows, NPCD_LIN128_MAX_T), NPCD_NO_LIN128=1 switches it off (A/B).
def _linear(bias, x, w16):
    """x [T, K] bf16, w16 [N, K] bf16, bias [N] bf16 -> x @ w16^T + bias, [T, N] bf16."""
    T = x.shape[0]
    out = harena.empty((T, w16.shape[0]), x.dtype, x.device)
    N, K = w16.shape
    if (_LIN128 and N == 1024 and K == 1024 and T <= _LIN128_MAX_T and x.is_cuda and x.is_contiguous() and w16.is_contiguous()
            and bias.is_contiguous() and x.dtype == w16.dtype == bias.dtype and hlin.supported128(T, N, K)):
        return hlin.linear128_fwd(x, w16, bias, out)
    wt = w16.t()
    _split_gemm(lambda r: torch.addmm(bias, x[r], wt, out=out[r]), T, N)
    return out


# The data gradients dy @ W read a TRANSPOSED 16-bit shadow of the four Linear weights of every block (FusedBackboneEngine), i.e. they
# are the forward's BLAS-TN form dy @ (W^T)^T instead of BLAS-NN against the weight as stored: the library's TN kernel is the faster
# one at these shapes (docs/experiments.md R10.1).  The shadow is re-transposed per block in the forward, one launch per block, only
# after the 16-bit shadow was written (once per optimizer step).  NPCD_DGRAD_NN=1: the product against the weight as stored, no
# transposed shadow kept up to date (A/B).  NPCD_DGRAD_T_MIN_T: the token rows from which the transposed form is used -- the
# saving grows with the token rows, the transposes (13 us per block) do not: at 4,104 rows the two cancel (13 us saved per block).
def _dgrad(dy, w16, wT=None):
    """dy [T, N] bf16, w16 [N, K] bf16 -> dy @ w16, [T, K] bf16.  wT [K, N]: w16 transposed (the engine's transposed shadow) -- the
    product then runs as dy @ wT^T, the forward's form; the large rows and the left-over rows of the split read the same buffer."""
    T = dy.shape[0]
    out = harena.empty((T, w16.shape[1]), dy.dtype, dy.device)
    b = w16 if wT is None else wT.t()
    _split_gemm(lambda r: torch.mm(dy[r], b, out=out[r]), T, w16.shape[1])
    return out


def _wgrad(dy, x, out):
    """out (fp32 view of the flat gradient) = dy^T @ x, fp32 accumulate AND fp32 output.

    The reduction dimension is the token count T (32,832 at cfg-D) while the output is only 1-4 M
    elements, i.e. 16-64 tiles of 256x256 for 256 CUs: the GEMM is split along T into S batched slices
    (hipBLASLt batched GEMM, S x more tiles in flight) whose fp32 partials are summed straight into the
    gradient view.  Measured on MI355X: c_qkv 350 -> 250 us, attn.c_proj 200 -> 87 us, c_fc 327 -> 259 us,
    mlp.c_proj 308 -> 255 us.
    (Tried: the weight gradients on a second HIP stream, so that they run beside the HBM-bound GELU / LayerNorm backward
    kernels of the critical path -- 84.39 -> 84.14 ms per step on the same box, i.e. nothing: the GEMM's workgroups hold
    every CU and the other stream's kernels are dispatched as they drain.)
    Round 18: at T = 32,832 the four products of a block take 874 us this way inside the step (slab sums included); from
    _WGRAD_MULTIBLOCK_MIN_T token rows on the backward sends whole groups of blocks to one ew.wgrad_group launch instead (773 us per
    block, docs/experiments.md R18.1) and this function serves the L mod G blocks at the bottom and the fallback."""
    # opt-in (NPCD_OWN_WGRAD=1): the own split-T kernel (csrc/gemm.hip: at parity with the library's row-split form -- both are bound
    # by the L2 -> LDS stream of a 256 x 256 tile -- bitwise reproducible, no library call)
    if _OWN_WGRAD and ew.wgrad(dy, x, out):
        return
    T = dy.shape[0]
    small = out.numel() <= (1 << 20)
    S = 8 if small else 4
    # keep >= 4096 rows per slice (2048 for the 1024 x 1024 output, 16 tiles: tools/probes/gpu_dev_wgrad_split.py at T = 4104 / 8208): short
    # reductions need no split
    S = min(S, max(1, T // (2048 if small else 4096)))
    while S > 1 and T % S:
        S //= 2
    if S == 1:
        torch.mm(dy.t(), x, out_dtype=_f32, out=out)
        return
    part = torch.bmm(dy.view(S, T // S, -1).transpose(1, 2), x.view(S, T // S, -1), out_dtype=_f32)
    if not (_SUM_KERNEL and ew.sum_slices(part, out)):
        torch.sum(part, dim=0, out=out)


# The weight gradients of a block on a second HIP stream, beside the data-gradient products and the HBM-bound GELU / LayerNorm backward
# kernels of the critical path; joined before the block's gradients are handed to the reducer.  Round 3 measured nothing at per-GPU
# batch 64 (docs/experiments.md R3.9); round 5 at the batches of a rank of the strong-scaling job, where a product is one partial
# round of tiles: 19.1 -> 18.6 ms per step at batch 8, 29.3 -> 28.7 at 16, 46.0 -> 45.6 at 32; at 64 it measures 84.4-84.5 against
# 82.9-84.3 ms (R5.11) -- the default below _WGRAD_STREAM_MAX_T token rows since.  NPCD_WGRAD_STREAM=0 / 1 forces it off / on at
# every size, NPCD_WGRAD_STREAM_PRIO=<priority> sets the side stream's priority.  Where the grouped launch below declines (a width
# that is not a multiple of 256, or more than _WGRAD_GROUP_MAX_T rows) both orders run the same kernels in the same order per tensor
# and the gradients are the same bits (tests/test_gpu_fused.py).  Where it engages -- the grouped launch exists on the side stream
# only -- side stream off runs the per-product library calls instead: two fp32 accumulation orders over the same 16-bit operands,
# NOT the same bits (tests/test_gpu_rank_step.py bounds the difference).
# Round 6: below _WGRAD_GROUP_MAX_T token rows the four weight gradients of a block are ONE launch of the own kernel (csrc/gemm.hip,
# npcd_wgrad_group: a workgroup per 256 x 256 tile over the whole token range; 192 tiles at width 1,024), beside the critical path on the
# side stream.  NPCD_WGRAD_GROUP=0 switches it off (the library's products), NPCD_WGRAD_GROUP_MAX_T sets the size limit.
# Round 6: the main stream no longer waits for the side stream once per block (a cross-queue dependency costs ~10 us of an idle chip per
# block even when it is already satisfied: tools/step_timeline.py on the rank step).  A block's gradients are handed to the reducer FROM the
# side stream instead -- behind the block's weight gradients in that stream's order, and behind the block's critical path through the fork's
# wait -- so a collective launched there depends on exactly what it reads; the main stream joins the side stream once, at the end of the
# backward.  NPCD_WGRAD_JOIN_PER_BLOCK=1 restores the per-block join (A/B).
_side = {}


def _side_stream(device):
    s = _side.get(device)
    if s is None:
        s = _side[device] = torch.cuda.Stream(device=device, priority=_WGRAD_STREAM_PRIO)
    return s


def _wgrad_side_ok(T):
    return _WGRAD_STREAM and T <= _WGRAD_STREAM_MAX_T


# Round 18: from _WGRAD_MULTIBLOCK_MIN_T token rows on -- where the side stream above is off and a product alone is 16-64 tiles for 256
# CUs -- the weight gradients of G blocks are ONE launch of the grouped kernel on the main stream (csrc/gemm.hip, npcd_wgrad_group
# with up to 16 products): at width 1,024 the four products of a block are 192 tiles of 256 x 256, four blocks 768 = three full rounds
# of 256 CUs, one workgroup per tile over all token rows -- no token slices, no fp32 slabs, no sum pass, one fixed summation order.  G
# comes from npcd_wgrad_group_blocks (0: no number of blocks fills the chip, the per-product path stays).  The (dy, x, out) triples of
# a block are queued where _wgrad was called and launched behind the critical path of every G-th block, counting down from the last;
# the L mod G blocks at the bottom keep the per-product calls.  The operands of up to G - 1 earlier blocks stay alive until their
# launch (~1.07 GB per block at T = 32,832, width 1,024).  NPCD_WGRAD_MULTIBLOCK=0: off, =force: G = 4 whatever the fill rule says
# (tests at small widths); NPCD_WGRAD_MULTIBLOCK_MIN_T: the threshold.  docs/experiments.md R18.1.
_multiblock_blocks = {}


def _wgrad_multiblock_blocks(T, W, dtype, device):
    """How many blocks share one grouped weight-gradient launch on the main stream at T token rows and width W; 0: none (the
    per-product calls of _wgrad)."""
    if (_WGRAD_MULTIBLOCK == "off" or T < _WGRAD_MULTIBLOCK_MIN_T or _wgrad_side_ok(T) or device.type != "cuda"
            or dtype not in (torch.bfloat16, torch.float16)):
        return 0
    if _WGRAD_MULTIBLOCK == "force":
        return ew.WGRAD_GROUP_MAX // len(_LINEARS)
    key = (W, device.index)
    if key not in _multiblock_blocks:
        with torch.cuda.device(device):
            _multiblock_blocks[key] = ew.wgrad_group_blocks([(3 * W, W), (W, W), (4 * W, W), (W, 4 * W)])
    return _multiblock_blocks[key]


def _mark_ready(eng, entry):
    """A block's gradients are final: its parameters, in _BLOCK_PARAMS order, go to the engine's reducer, if one is reducing."""
    if eng.reducer is not None and eng.reducer.active:
        for p in entry["params"]:
            eng.reducer.mark_ready(p)


# The three ways the weight gradients of a backward are issued:
#   side stream: a block's four products are queued and start on the side stream in block_done -- one fork per block (per product it
#     cost the host ~40 us of stream bookkeeping, 3.8 ms of a rank's step at per-GPU batch 8, which is host-bound:
#     tools/probes/gpu_dev_b8_hostprofile.py), as one grouped launch where that is on and takes them.  The block ABOVE is handed to the
#     reducer on the side stream ahead of them: behind its own weight gradients and, through the wait of the fork that started them,
#     behind its critical path; the main stream waits once, in finish().  (_JOIN_PER_BLOCK, the round-5 order: the main stream joins
#     per block -- the block above had this block's critical path to finish its weight gradients beside -- and hands it on itself.)
#     The grouped launch of ONE block runs only here: with the side stream off the same products are the per-product library calls
#     of _wgrad, a different fp32 summation order.
#   multi-block (group = G > 0): the products of blocks [L mod G, L) are queued and launched in runs of G blocks, counting down from
#     the last, on the main stream -- 4 x G products, one launch; the L mod G blocks at the bottom are direct.
#   direct: _wgrad at once.
class _WgradSchedule:
    """Where and when the weight gradients of ONE 16-bit backward are issued: add(dy, x, out) per product of the current block,
    block_done(bi) when the block's critical path has been enqueued, finish() after block 0.  In every mode a block goes to the
    reducer only behind the launch that wrote its weight gradients, and in descending block order."""

    def __init__(self, eng, T, W, dtype, device, side=None, group=None):
        # (`side`, `group`: given by tests without a GPU)
        self.eng, self.blocks, self.T = eng, eng.blocks, T
        self.side = _wgrad_side_ok(T) if side is None else side
        self.stream = _side_stream(device) if self.side else None
        self.group = group if group is not None else 0 if self.side else _wgrad_multiblock_blocks(T, W, dtype, device)
        self.tail = len(self.blocks) % self.group if self.group else len(self.blocks)
        self.bi = len(self.blocks) - 1             # the block whose products add() is being given
        # the (dy, x, out) triples not yet launched -- what keeps their operands alive, cleared at the launch; main stream: the
        # blocks not yet handed to the reducer
        self.queue, self.waiting = [], []

    def add(self, dy, x, out):
        if self.side or self.bi >= self.tail:
            self.queue.append((dy, x, out))
        else:
            _wgrad(dy, x, out)

    def _launch(self, grouped):
        if not (grouped and ew.wgrad_group(self.queue)):
            for t in self.queue:
                _wgrad(*t)
        self.queue.clear()

    def block_done(self, bi):
        L, side, self.bi = len(self.blocks), self.stream, bi - 1
        if not self.side:
            self.waiting.append(bi)
            if bi < self.tail or (L - bi) % self.group == 0:       # a direct block, or the last of a run of `group` blocks
                if self.queue:
                    self._launch(True)
                for b in self.waiting:             # (mlp.c_proj.bias of the lowest one was finished by the block above it / the tail)
                    _mark_ready(self.eng, self.blocks[b])
                self.waiting.clear()
            return
        if bi + 1 < L:                             # the block above: behind its weight gradients
            if _JOIN_PER_BLOCK:
                torch.cuda.current_stream().wait_stream(side)
            with (_NULL if _JOIN_PER_BLOCK else torch.cuda.stream(side)):
                _mark_ready(self.eng, self.blocks[bi + 1])
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for dy, x, out in self.queue:
                dy.record_stream(side)
                x.record_stream(side)
            self._launch(_WGRAD_GROUP and self.T <= _WGRAD_GROUP_MAX_T)

    def finish(self):
        if self.side:
            torch.cuda.current_stream().wait_stream(self.stream)
            _mark_ready(self.eng, self.blocks[0])


def _no_engine():
    return None


class _BlockViews:
    """What every fused backbone node of a trainer holds: per block the parameters, views of their fp32 masters and of their fp32
    gradients in the trainer's flat buffers, the reducer, and the hooks of a trainer with lazily gathered parameters."""
    fp32_class = False

    # the engine belongs to ONE trainer's flat buffers: a deep copy / pickle of the backbone carries None (the module path) instead
    def __deepcopy__(self, memo):
        return None

    def __reduce__(self):
        return (_no_engine, ())

    def __init__(self, backbone, flat, reducer=None):
        self.heads = backbone.resblocks[0].attn.heads
        self.width = backbone.width
        self.reducer = reducer
        self._offset = {id(p): off for p, off in zip(flat.params, flat.offsets)}
        self.blocks = []
        for blk in backbone.resblocks:
            named = dict(blk.named_parameters())
            entry = {"params": [named[n] for n in _BLOCK_PARAMS]}
            for n in _BLOCK_PARAMS:
                p = named[n]
                off = self._offset[id(p)]
                key = n.replace(".", "_")
                entry[key] = p.data                                              # fp32 master (LN affine is used in fp32)
                entry[key + "_g"] = flat.grad[off:off + p.numel()].view_as(p)   # fp32 gradient
            self.blocks.append(entry)
        self.block_ranges, self.wait_range = None, None      # set by a trainer with lazily gathered parameters (engine.py)

    def shadow_written(self):
        pass


class FusedBackboneEngine(_BlockViews):
    """The 16-bit node (bf16, or f16 with loss scaling): the block views plus views of the 16-bit shadow of the flat parameters."""

    def __init__(self, backbone, flat, shadow, reducer=None):
        super().__init__(backbone, flat, reducer)
        for blk, entry in zip(backbone.resblocks, self.blocks):
            named = dict(blk.named_parameters())
            for n in _BLOCK_PARAMS:
                p = named[n]
                off = self._offset[id(p)]
                entry[n.replace(".", "_") + "_16"] = shadow[off:off + p.numel()].view_as(p)     # bf16 shadow (GEMM operands)

        # The GEMMs read the bf16 SHADOW, which only the optimizer kernel (and load_trainer_state) refresh.  Any other in-place
        # write to a parameter -- model.load_state_dict, copying EMA weights in to sample from them -- bumps the parameter's
        # version counter (the optimizer kernel writes through raw pointers and does not): the stamp below notices that and the
        # shadow is re-cast from the fp32 masters before the next forward instead of silently running stale Linear weights
        # beside fresh LayerNorm ones.
        self._flat, self._shadow = flat, shadow
        self.dtype = shadow.dtype                            # the run's 16-bit activation type: bf16, or f16 (with loss scaling)
        self._stamped = [p for e in self.blocks for p in e["params"]]
        self._stamp = self._versions()
        # counts the writes to the 16-bit shadow (optimizer pass, parameter gather, re-cast): what a derivative of the shadow -- the
        # transposed shadow below -- is stamped with
        self.shadow_epoch = 0
        # The TRANSPOSED shadow: W^T of the four Linear weights of every block (12 W^2 16-bit elements per block), which the data
        # gradients read (_dgrad) and the NPCD_OWN_DGELU launch.  One buffer, allocated by the first refresh (an engine that never
        # reads it -- NPCD_DGRAD_NN, or only steps below _DGRAD_T_MIN_T rows -- never pays for it) and kept for the life of the
        # engine -- never from the step arena: its pointers stay put.  A block's part is rewritten by refresh_transposed(), in the
        # forward, when its stamp is not the shadow's epoch; its views appear in the block's entry (e["<name>_weight_16T"]) once
        # they hold the weights.  (With lazily gathered parameters every gather of a forward moves the epoch, so the blocks ahead of
        # the last gather are transposed once more by the NEXT forward although their weights did not change: correct, and one
        # launch per block per forward at the most.)
        self._shadowT, self._wT = None, None
        self._wT_stamp = [None] * len(self.blocks)
        self.transposed_refreshes = 0                        # launches of the grouped transpose, one per block and refresh
        # Round 6: below _STEP_ARENA_MAX_T token rows -- the token counts of a rank of the strong-scaling job, where the host side of a
        # step is as long as its GPU side -- the ~740 buffers a step of the fused node allocates are kept and handed out again in the
        # same order by the next step (npcd/hip/arena.py): 1.6 ms of host time per step at per-GPU batch 8.  The memory of a step then
        # stays allocated between steps (at 4,104 rows ~8 GB; the caching allocator would keep most of it anyway).  NPCD_STEP_ARENA=0: off.
        self.arena = harena.StepArena() if _STEP_ARENA else None

    def shadow_written(self):
        self.shadow_epoch += 1

    def wants_transposed(self, T):
        """Whether a step over T token rows reads the transposed shadow."""
        return _OWN_DGELU or (not _DGRAD_NN and T >= _DGRAD_T_MIN_T)

    def refresh_transposed(self, bi):
        """Block bi's part of the transposed shadow from its 16-bit shadow (which must be complete: behind wait_range), unless it
        already is that epoch's: one launch."""
        if self._wT_stamp[bi] == self.shadow_epoch:
            return
        if self._shadowT is None:
            sizes = [entry[k + "_weight_16"].numel() for entry in self.blocks for k in _LINEARS]
            self._shadowT = torch.empty(sum(sizes), dtype=self._shadow.dtype, device=self._shadow.device)      # (not an arena request)
            self._wT, off = [], 0
            for entry in self.blocks:
                views = []
                for k in _LINEARS:
                    N, K = entry[k + "_weight_16"].shape
                    views.append(self._shadowT[off:off + N * K].view(K, N))
                    off += N * K
                self._wT.append(views)
        e = self.blocks[bi]
        hlin.transpose16_group([(e[k + "_weight_16"], v) for k, v in zip(_LINEARS, self._wT[bi])])
        for k, v in zip(_LINEARS, self._wT[bi]):
            e[k + "_weight_16T"] = v
        self._wT_stamp[bi] = self.shadow_epoch
        self.transposed_refreshes += 1

    def _versions(self):
        return [p._version for p in self._stamped]

    def sync_shadow(self, force=False):
        """Re-cast fp32 masters -> bf16 shadow if a parameter was written outside the optimizer since the last check."""
        v = self._versions()
        if force or v != self._stamp:
            if self.wait_range is not None:
                self.wait_range()                                # every pending parameter gather first: the whole shadow is re-cast
            for p, off in zip(self._flat.params, self._flat.offsets):
                if p.data_ptr() != self._flat.flat.data_ptr() + off * self._flat.flat.element_size():
                    raise RuntimeError("a parameter of the fused backbone was re-homed outside the trainer's flat buffer "
                                       "(p.data replaced): build a new DiffusionTrainer for this model")
            ew.cast_f32_bf16(self._flat.flat, self._shadow)
            self.shadow_written()
            self._stamp = v

    def __call__(self, x):
        self.sync_shadow()
        return _BackboneFn.apply(x, self)


class _BlockWeights:
    """Per-block copies of the weights for the forward-only path of a backbone that is not attached to a trainer (sampling from a loaded
    checkpoint): rebuilt when a parameter was written to or replaced since the copy was taken.  A subclass converts one parameter."""

    def __init__(self, backbone):
        self.heads = backbone.resblocks[0].attn.heads
        self.params = [[dict(blk.named_parameters())[n] for n in _BLOCK_PARAMS] for blk in backbone.resblocks]
        self.stamp, self.blocks = None, None

    def current(self):
        stamp = [(p._version, p.data_ptr()) for ps in self.params for p in ps]
        if stamp != self.stamp:
            self.blocks = []
            for ps in self.params:
                e = {}
                for n, p in zip(_BLOCK_PARAMS, ps):
                    self.convert(e, n, n.replace(".", "_"), p.data)
                self.blocks.append(e)
            self.stamp = stamp
        return self.blocks


class InferenceWeights(_BlockWeights):
    """The parameters as they are (LayerNorm affines are used in fp32) and bf16 copies of the Linear weights and biases."""

    def convert(self, e, n, key, data):
        e[key] = data
        if not n.startswith("ln_"):
            e[key + "_16"] = data.to(_bf16)


class InferenceWeightsX2(_BlockWeights):
    """The split-operand form of the fp32-class forward (csrc/split.hip): per Linear layer [Wh | Wh | Wl] bf16 [N, 3 K] with
    W = Wh + Wl, the biases and LayerNorm parameters in fp32."""

    def convert(self, e, n, key, data):
        w = data.to(_f32)
        if n.endswith("weight") and not n.startswith("ln_"):
            hi = w.to(_bf16)
            lo = (w - hi.float()).to(_bf16)
            e[key + "_x3"] = torch.cat((hi, hi, lo), dim=1).contiguous()
        else:
            e[key] = w.contiguous()


def backbone_forward_x2(x, blocks, heads):
    """Forward only, in the reference's fp32 class (the sampler, diffusion_model.py:108-133, runs the denoiser in fp32): residual stream,
    LayerNorm, attention (the fp32 matrix-instruction kernels of csrc/attention.hip) and GELU in fp32; the four Linear layers of a
    block as ONE bf16 library GEMM each over the three cross products of split operands (csrc/split.hip, npcd_split3_bf16), fp32
    accumulation and output -- 3e-6 relative per product against float64 (an fp32 GEMM: 4e-7), at 2.3-3.5 x the fp32 GEMM's rate.
    x [B, n, W] fp32 -> [B, n, W] fp32.  `blocks`: InferenceWeightsX2.current()."""
    import torch.nn.functional as F
    B, n, W = x.shape
    T, d = B * n, W // heads
    scale = 1.0 / math.sqrt(d)
    f32 = _f32

    def lin(a3, e, name):           # [T, 3 K] bf16 x [N, 3 K]^T -> [T, N] fp32 (bias added by the consumer)
        return torch.mm(a3, e[name + "_weight_x3"].t(), out_dtype=f32)
    def ln_split(xs, e, ln, o=None, bias=None):      # (xs + o + bias, split(LayerNorm(.))): one kernel, or torch + split3 for other widths
        r = ew.add_ln_split3(xs, e[ln + "_weight"], e[ln + "_bias"], o, bias)
        if r is not None:
            return r
        if o is not None:
            xs = xs + o + bias
        return xs, ew.split3(F.layer_norm(xs, (W,), e[ln + "_weight"], e[ln + "_bias"]))
    with torch.autocast("cuda", enabled=False):
        xs = x.reshape(T, W).contiguous()
        o, ob = None, None               # the previous block's mlp.c_proj output and bias: added by the next LayerNorm kernel
        for e in blocks:
            xs, y1 = ln_split(xs, e, "ln_1", o, ob)
            qkv = lin(y1, e, "attn_c_qkv").add_(e["attn_c_qkv_bias"]).view(B, n, heads, 3 * d)
            a, _ = hattn._fwd(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], scale)
            xs, y2 = ln_split(xs, e, "ln_2", lin(ew.split3(a.reshape(T, W)), e, "attn_c_proj"), e["attn_c_proj_bias"])
            h = lin(y2, e, "mlp_c_fc")
            o, ob = lin(ew.split3(h, bias=e["mlp_c_fc_bias"], gelu=True), e, "mlp_c_proj"), e["mlp_c_proj_bias"]
        xs = xs + o + ob
    return xs.view(B, n, W)


def backbone_forward(x, blocks, heads, dtype=_bf16):
    """Forward only (sampler, evaluation): the kernels of the training forward, nothing kept for a backward.
    x [B, n, W] fp32 -> [B, n, W] fp32.  `dtype`: the 16-bit type of the weights in `blocks`."""
    B, n, W = x.shape
    T, d = B * n, W // heads
    scale = 1.0 / math.sqrt(d)
    with torch.autocast("cuda", enabled=False):
        xs = x.reshape(T, W).contiguous()
        delta = None
        for e in blocks:
            x1, y1, _, _ = ew.add_ln_fwd(xs, delta, e["ln_1_weight"], e["ln_1_bias"], dtype=dtype)
            x_cur = xs if x1 is None else x1
            q4 = _linear(e["attn_c_qkv_bias_16"], y1, e["attn_c_qkv_weight_16"]).view(B, n, heads, 3 * d)
            a, _ = hattn._fwd(q4[..., :d], q4[..., d:2 * d], q4[..., 2 * d:], scale)
            o = _linear(e["attn_c_proj_bias_16"], a.view(T, W), e["attn_c_proj_weight_16"])
            xs, y2, _, _ = ew.add_ln_fwd(x_cur, o, e["ln_2_weight"], e["ln_2_bias"])
            g = ew.gelu_fwd(_linear(e["mlp_c_fc_bias_16"], y2, e["mlp_c_fc_weight_16"]))
            delta = _linear(e["mlp_c_proj_bias_16"], g, e["mlp_c_proj_weight_16"])
        out = xs + delta
    return out.view(B, n, W)


# opt-in (NPCD_OWN_DGELU=1): the data gradient of mlp.c_proj as the own NT product with the GELU backward and the c_fc bias-gradient
# column sums in its epilogue (csrc/gemm_nt.hip, docs/experiments.md R4.1) on the full 256-row tiles of the token range; the remainder
# rows keep the library product + the separate kernel.  Reads the engine's transposed shadow of the weight, brought up to date by this
# step's forward.  The own launch only for what npcd_linear_dgelu_bwd takes -- contiguous 16-bit operands of one type; anything else
# goes through the caller's library product + gelu_bwd instead of raising, like NPCD_ERR_UNSUPPORTED would.
def _own_dgelu(e, dxb, h, dgrad_t, sums):
    """dh = gelu'(h) * (dxb @ mlp.c_proj.weight) of block entry `e`, its column sums added to `sums`; None: declined."""
    T, W = dxb.shape
    Tm = T - T % 256
    w2 = e["mlp_c_proj_weight_16"]
    if not (Tm > 0 and hlin.supported(Tm, 4 * W, W) and dxb.is_contiguous() and h.is_contiguous() and w2.is_contiguous()
            and dxb.dtype == w2.dtype == h.dtype and dxb.dtype in (torch.bfloat16, torch.float16)):
        return None
    wT = e["mlp_c_proj_weight_16T"]
    dh = harena.empty_like(h)
    extra = ew.lib().npcd_colsum_blocks(T - Tm) if Tm < T else 0
    _, part, rows = hlin.linear_dgelu_bwd(dxb[:Tm], wT, h[:Tm], out=dh[:Tm], extra_part_rows=extra)
    if Tm < T:       # remainder rows: library product + the separate kernel, partial rows behind the own kernel's
        dg = torch.mm(dxb[Tm:], wT.t() if dgrad_t else w2)
        ew.gelu_bwd(dg, h[Tm:], None, out=dh[Tm:], part_rows=part[rows:])
        del dg
    sums.add(part, rows + extra, 4 * W, e["mlp_c_fc_bias_g"])
    return dh


class _BackboneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eng):
        B, n, W = x.shape
        T = B * n
        arena = eng.arena if (eng.arena is not None and x.is_cuda and T <= _STEP_ARENA_MAX_T) else None
        token = arena.begin() if arena is not None else 0
        if not token:
            arena = None                       # (another step of this engine still holds its buffers: plain allocations for this one)
        ctx.arena, ctx.arena_token = arena, token
        if arena is None:
            return _BackboneFn._forward(ctx, x, eng)
        ctx.arena_guard = harena.StepGuard(arena, token)      # ends the step if the graph is dropped without a backward
        try:
            with arena.active():
                return _BackboneFn._forward(ctx, x, eng)
        except BaseException:
            arena.end(token)
            raise

    @staticmethod
    def _forward(ctx, x, eng):
        B, n, W = x.shape
        T, H = B * n, eng.heads
        d = W // H
        scale = 1.0 / math.sqrt(d)
        saved = []
        with torch.autocast("cuda", enabled=False):
            xs = x.reshape(T, W).contiguous()
            delta = None
            ctx.transposed = transposed = x.is_cuda and eng.wants_transposed(T)
            for bi, e in enumerate(eng.blocks):
                if eng.wait_range is not None:
                    eng.wait_range(*eng.block_ranges[bi])        # this block's parameters (gathered lazily by the sharded optimizer)
                if transposed:
                    eng.refresh_transposed(bi)                   # (behind the wait: a gathered block is transposed once it has arrived)
                x1, y1, mean1, rstd1 = ew.add_ln_fwd(xs, delta, e["ln_1_weight"], e["ln_1_bias"], dtype=eng.dtype)
                x_cur = xs if x1 is None else x1
                qkv = _linear(e["attn_c_qkv_bias_16"], y1, e["attn_c_qkv_weight_16"])
                q4 = qkv.view(B, n, H, 3 * d)
                a, lse = hattn._fwd(q4[..., :d], q4[..., d:2 * d], q4[..., 2 * d:], scale)
                a = a.view(T, W)
                o = _linear(e["attn_c_proj_bias_16"], a, e["attn_c_proj_weight_16"])
                x2, y2, mean2, rstd2 = ew.add_ln_fwd(x_cur, o, e["ln_2_weight"], e["ln_2_bias"])
                h = _linear(e["mlp_c_fc_bias_16"], y2, e["mlp_c_fc_weight_16"])
                g = ew.gelu_fwd(h)
                delta = _linear(e["mlp_c_proj_bias_16"], g, e["mlp_c_proj_weight_16"])
                saved.append((x_cur, mean1, rstd1, y1, qkv, a, lse, x2, mean2, rstd2, y2, h, g))
                xs = x2
            out = xs + delta                       # fp32 + bf16 -> fp32  (a torch operator: the node's output is never an arena buffer)
        ctx.eng, ctx.saved, ctx.dims, ctx.scale = eng, saved, (B, n, W, H, d), scale
        return out.view(B, n, W)

    @staticmethod
    def backward(ctx, dout):
        if any(s is None for s in ctx.saved):
            # (the backward frees each block's activations as it goes: a second pass over the same graph finds them gone)
            raise RuntimeError("the fused backbone engine does not support retain_graph / double backward: run a new forward "
                               "for every backward")
        arena = ctx.arena
        if arena is None:
            return _BackboneFn._backward(ctx, dout)
        try:
            with arena.active():           # (the engine's worker thread: the arena context is per thread)
                return _BackboneFn._backward(ctx, dout)
        finally:
            arena.end(ctx.arena_token)

    @staticmethod
    def _backward(ctx, dout):
        eng, (B, n, W, H, d), scale = ctx.eng, ctx.dims, ctx.scale
        T = B * n
        with torch.autocast("cuda", enabled=False):
            dx = dout.reshape(T, W).contiguous().float()
            dxb = dx.to(eng.dtype)
            last = eng.blocks[-1]
            last["mlp_c_proj_bias_g"].copy_(dx.sum(dim=0))
            # (the forward of this step brought the transposed shadow up to date, or did not: decided there, once)
            dgrad_t = ctx.transposed and not _DGRAD_NN and T >= _DGRAD_T_MIN_T
            wg = _WgradSchedule(eng, T, W, eng.dtype, dx.device)
            for bi in range(len(eng.blocks) - 1, -1, -1):
                e = eng.blocks[bi]
                x_cur, mean1, rstd1, y1, qkv, a, lse, x2, mean2, rstd2, y2, h, g = ctx.saved[bi]
                ctx.saved[bi] = None
                sums = ew.ColsumBatch()            # this block's 8 bias / LN-affine column sums: one finalize
                # ---- MLP branch: x3 = x2 + c_proj(gelu(c_fc(ln_2(x2)))) ------------------------------
                # (dh from the own launch where it is on and takes the shapes, else from the library product + gelu_bwd; the weight
                # gradient is issued right behind the data-gradient product either way)
                dh = _own_dgelu(e, dxb, h, dgrad_t, sums) if (_OWN_DGELU and ctx.transposed) else None
                dg = _dgrad(dxb, e["mlp_c_proj_weight_16"], e["mlp_c_proj_weight_16T"] if dgrad_t else None) if dh is None else None
                wg.add(dxb, g, e["mlp_c_proj_weight_g"])
                if dh is None:
                    dh = ew.gelu_bwd(dg, h, e["mlp_c_fc_bias_g"], batch=sums)
                del dg, g, h
                dy2 = _dgrad(dh, e["mlp_c_fc_weight_16"], e["mlp_c_fc_weight_16T"] if dgrad_t else None)
                wg.add(dh, y2, e["mlp_c_fc_weight_g"])
                del dh, y2
                dx2, dx2b = ew.ln_bwd(dy2, x2, mean2, rstd2, e["ln_2_weight"], dx, e["ln_2_weight_g"], e["ln_2_bias_g"],
                                      e["attn_c_proj_bias_g"], batch=sums)
                del dy2, x2, dx, dxb
                # ---- attention branch: x2 = x + c_proj(attn(c_qkv(ln_1(x)))) ---------------------------
                da = _dgrad(dx2b, e["attn_c_proj_weight_16"], e["attn_c_proj_weight_16T"] if dgrad_t else None)
                wg.add(dx2b, a, e["attn_c_proj_weight_g"])
                dqkv = harena.empty_like(qkv)
                q4, g4 = qkv.view(B, n, H, 3 * d), dqkv.view(B, n, H, 3 * d)
                # the c_qkv bias gradient (column sums of dqkv) is a by-product of the attention backward's row stores
                cpart = hattn.colsum_part_for(g4[..., :d]) if _ATTN_COLSUM else None
                hattn._bwd(q4[..., :d], q4[..., d:2 * d], q4[..., 2 * d:], a.view(B, n, H, d), da.view(B, n, H, d), lse,
                           g4[..., :d], g4[..., d:2 * d], g4[..., 2 * d:], scale, colsum_part=cpart[0] if cpart else None)
                del da, a, qkv, dx2b
                if cpart:
                    sums.add(cpart[0], cpart[1], 3 * W, e["attn_c_qkv_bias_g"])
                else:
                    ew.colsum_bf16(dqkv, e["attn_c_qkv_bias_g"], batch=sums)
                dy1 = _dgrad(dqkv, e["attn_c_qkv_weight_16"], e["attn_c_qkv_weight_16T"] if dgrad_t else None)
                wg.add(dqkv, y1, e["attn_c_qkv_weight_g"])
                del dqkv, y1
                prev_bias_g = eng.blocks[bi - 1]["mlp_c_proj_bias_g"] if bi > 0 else None
                # (the last block's dx is what the node returns: allocated outside the arena, like everything that outlives the step)
                with (harena.paused() if bi == 0 else _NULL):
                    dx, dxb = ew.ln_bwd(dy1, x_cur, mean1, rstd1, e["ln_1_weight"], dx2, e["ln_1_weight_g"], e["ln_1_bias_g"],
                                        prev_bias_g, want_bf16=bi > 0, batch=sums)
                del dy1, dx2
                sums.flush()
                wg.block_done(bi)
            wg.finish()
        return dx.view(B, n, W), None


# ---- fp32-class training: DiffusionTrainer(dtype="fp32_class") ---------------------------------------------------------------------------
# The reference's --dtype float32 (train_diffusion.py:78) on the bf16 matrix rate: every product of a block -- forward, data gradient and
# weight gradient -- is ONE bf16 GEMM (or, for a weight gradient, three) over the three cross products hi*hi + lo*hi + hi*lo of split
# operands (x = hi + lo, bf16 halves) with fp32 accumulation; the residual stream, LayerNorm, attention (the exact-fp32 kernels), GELU
# (exact erf) and every bias / LayerNorm-affine column sum in fp32.  The split weights are built from the fp32 masters inside the forward,
# block by block, right behind the wait for that block's parameters: nothing is cached between steps, so a lazily gathered parameter,
# load_state_dict or an EMA copy-in can never leave a stale operand behind.
SPLIT_WIDTHS = (256, 512, 768, 1024, 2048)          # add_ln_split3 (W / 256 in 1, 2, 3, 4, 8, 16) and the LayerNorm backward (W <= 2048)


def x2_supported(width, heads):
    """None, or why DiffusionTrainer(dtype="fp32_class") cannot train a backbone of this width / head count."""
    if heads <= 0 or width % heads or width // heads != 64:
        return (f"head dim {width // heads if heads > 0 and width % heads == 0 else width / max(heads, 1)}: the fp32 attention backward "
                f"is built for head dim 64 only")
    if width not in SPLIT_WIDTHS:
        return f"width {width}: the split-operand kernels take widths {', '.join(map(str, SPLIT_WIDTHS))}"
    return None


def _mm_x2(a3, w3):
    """[T, 3 K] bf16 x [3 K, N] bf16 (a transposed forward layout or a data-gradient layout) -> [T, N] fp32."""
    return torch.mm(a3, w3, out_dtype=_f32)


def _wgrad_x2(dy3, x3, out):
    """out [N, K] fp32 = dy^T x from the split operands dy3 [T, 3 N] = [dyh | dyl | dyh], x3 [T, 3 K] = [xh | xl | xh]: the three cross
    products as library GEMMs on strided views -- (dyh, xl) and (dyl, xh) as one batched call (slice strides N and K), (dyh, xh) as one
    more -- into fp32 slabs, added in a fixed order."""
    T, N = dy3.shape[0], out.shape[0]
    K = out.shape[1]
    d, x = dy3.view(T, 3, N), x3.view(T, 3, K)
    part = harena.empty((3, N, K), _f32, out.device)
    torch.bmm(d[:, 0:2].permute(1, 2, 0), x[:, 1:3].permute(1, 0, 2), out_dtype=_f32, out=part[0:2])
    torch.mm(d[:, 0].t(), x[:, 0], out_dtype=_f32, out=part[2])
    torch.sum(part, dim=0, out=out)


# The form of the weight gradients (A/B switch, NPCD_X2_WGRAD): "library" = _wgrad_x2 above; "own" = the own kernels of csrc/gemm.hip on
# the operands stacked along the token dimension -- dy [dyh ; dyl ; dyh] and x [xl ; xh ; xh], [3 T, N] / [3 T, K], one reduction over
# 3 T rows (the four products of a block in one npcd_wgrad_group launch up to _WGRAD_GROUP_MAX_T rows, else npcd_wgrad per product).
def _stack_x2(a3, lo_first):
    """[T, 3 N] = [hi | lo | hi] -> [3 T, N] bf16 stacked along the tokens: [hi ; lo ; hi], or (lo_first) [lo ; hi ; hi]."""
    T, N = a3.shape[0], a3.shape[1] // 3
    v = a3.view(T, 3, N)
    out = harena.empty((3, T, N), _bf16, a3.device)
    if lo_first:
        out[0].copy_(v[:, 1])
        out[1:].copy_(v[:, 0::2].transpose(0, 1))
    else:
        out.copy_(v.transpose(0, 1))
    return out.view(3 * T, N)


def _wgrad_own(pending):
    """The queued weight gradients of a block, (dy3, x3, out) each, on the own kernels (see _X2_WGRAD)."""
    triples = [(_stack_x2(dy3, False), _stack_x2(x3, True), out) for dy3, x3, out in pending]
    pending.clear()
    if triples[0][0].shape[0] <= _WGRAD_GROUP_MAX_T:
        ok = ew.wgrad_group(triples)
    else:
        ok = all(ew.wgrad(dy, x, out) for dy, x, out in triples)
    if not ok:
        raise RuntimeError("fp32-class weight gradients: the own kernels do not take these shapes (NPCD_X2_WGRAD=library does)")


class FusedBackboneEngineX2(_BlockViews):
    """The fused backbone node in the fp32 class: the block views only -- no 16-bit shadow (the split weights are derived from the fp32
    masters in every forward), no step arena.  transformer.py routes on `fp32_class`: grad enabled, autocast off."""
    fp32_class = True

    def __init__(self, backbone, flat, reducer=None):
        why = x2_supported(backbone.width, backbone.resblocks[0].attn.heads)
        if why is not None:
            raise ValueError(f"fp32_class training: {why}")
        super().__init__(backbone, flat, reducer)

    def __call__(self, x):
        return _BackboneX2Fn.apply(x, self)


class _BackboneX2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, eng):
        B, n, W = x.shape
        T, H = B * n, eng.heads
        d = W // H
        scale = 1.0 / math.sqrt(d)
        saved = []
        with torch.autocast("cuda", enabled=False):
            xs = x.reshape(T, W).contiguous().float()
            o, ob = None, None               # the previous block's mlp.c_proj output and bias: added by the next LayerNorm kernel
            for bi, e in enumerate(eng.blocks):
                if eng.wait_range is not None:
                    eng.wait_range(*eng.block_ranges[bi])        # this block's parameters (gathered lazily by the sharded optimizer)
                split = dict(zip(_LINEARS, ew.split_weights([e[k + "_weight"] for k in _LINEARS])))
                x_cur, y1, mean1, rstd1 = ew.add_ln_split3_stats(xs, e["ln_1_weight"], e["ln_1_bias"], o, ob)
                qkv = _mm_x2(y1, split["attn_c_qkv"][0].t()).add_(e["attn_c_qkv_bias"])
                q4 = qkv.view(B, n, H, 3 * d)
                a, lse = hattn._fwd_f32(q4[..., :d], q4[..., d:2 * d], q4[..., 2 * d:], scale, want_lse=True)
                a = a.view(T, W)
                o = _mm_x2(ew.split3(a), split["attn_c_proj"][0].t())
                x2, y2, mean2, rstd2 = ew.add_ln_split3_stats(x_cur, e["ln_2_weight"], e["ln_2_bias"], o, e["attn_c_proj_bias"])
                h = _mm_x2(y2, split["mlp_c_fc"][0].t())                  # without its bias: the split kernels add it
                o, ob = _mm_x2(ew.split3(h, bias=e["mlp_c_fc_bias"], gelu=True), split["mlp_c_proj"][0].t()), e["mlp_c_proj_bias"]
                # (the split GELU output is rebuilt from h in the backward; only the data-gradient layouts of the weights are kept)
                saved.append((x_cur, mean1, rstd1, y1, qkv, a, lse, x2, mean2, rstd2, y2, h, {k: v[1] for k, v in split.items()}))
                del split
                xs = x2
            out = xs + o + ob
        ctx.eng, ctx.saved, ctx.dims, ctx.scale = eng, saved, (B, n, W, H, d), scale
        return out.view(B, n, W)

    @staticmethod
    def backward(ctx, dout):
        if any(s is None for s in ctx.saved):
            raise RuntimeError("the fused backbone engine does not support retain_graph / double backward: run a new forward "
                               "for every backward")
        eng, (B, n, W, H, d), scale = ctx.eng, ctx.dims, ctx.scale
        T = B * n
        with torch.autocast("cuda", enabled=False):
            dx = dout.reshape(T, W).contiguous().float()
            eng.blocks[-1]["mlp_c_proj_bias_g"].copy_(dx.sum(dim=0))
            dx3 = ew.split3(dx)
            for bi in range(len(eng.blocks) - 1, -1, -1):
                e = eng.blocks[bi]
                x_cur, mean1, rstd1, y1, qkv, a, lse, x2, mean2, rstd2, y2, h, wd = ctx.saved[bi]
                ctx.saved[bi] = None
                sums = ew.ColsumBatch()            # this block's 8 bias / LN-affine column sums: one finalize
                pending = []
                wg = (lambda *t: pending.append(t)) if _X2_WGRAD == "own" else _wgrad_x2
                # ---- MLP branch: x3 = x2 + c_proj(gelu(c_fc(ln_2(x2)))) ------------------------------
                dg = _mm_x2(dx3, wd["mlp_c_proj"])
                wg(dx3, ew.split3(h, bias=e["mlp_c_fc_bias"], gelu=True), e["mlp_c_proj_weight_g"])
                dh3 = ew.split3_colsum(dg, e["mlp_c_fc_bias_g"], h=h, bias=e["mlp_c_fc_bias"], batch=sums)
                del dg, h
                dy2 = _mm_x2(dh3, wd["mlp_c_fc"])
                wg(dh3, y2, e["mlp_c_fc_weight_g"])
                del dh3, y2
                dx2, dx2_3 = ew.ln_bwd_split3(dy2, x2, mean2, rstd2, e["ln_2_weight"], dx, e["ln_2_weight_g"], e["ln_2_bias_g"],
                                              e["attn_c_proj_bias_g"], batch=sums)
                del dy2, x2, dx, dx3
                # ---- attention branch: x2 = x + c_proj(attn(c_qkv(ln_1(x)))) ---------------------------
                da = _mm_x2(dx2_3, wd["attn_c_proj"])
                wg(dx2_3, ew.split3(a), e["attn_c_proj_weight_g"])
                del dx2_3
                dqkv = torch.empty_like(qkv)
                q4, g4, a4 = qkv.view(B, n, H, 3 * d), dqkv.view(B, n, H, 3 * d), a.view(B, n, H, d)
                hattn._bwd_f32(q4[..., :d], q4[..., d:2 * d], q4[..., 2 * d:], a4, da.view(B, n, H, d), lse,
                               g4[..., :d], g4[..., d:2 * d], g4[..., 2 * d:], scale)
                del da, a, qkv, lse
                dqkv3 = ew.split3_colsum(dqkv, e["attn_c_qkv_bias_g"], batch=sums)
                del dqkv
                dy1 = _mm_x2(dqkv3, wd["attn_c_qkv"])
                wg(dqkv3, y1, e["attn_c_qkv_weight_g"])
                del dqkv3, y1
                prev_bias_g = eng.blocks[bi - 1]["mlp_c_proj_bias_g"] if bi > 0 else None
                dx, dx3 = ew.ln_bwd_split3(dy1, x_cur, mean1, rstd1, e["ln_1_weight"], dx2, e["ln_1_weight_g"], e["ln_1_bias_g"],
                                           prev_bias_g, want_split=bi > 0, batch=sums)
                del dy1, dx2
                if pending:
                    _wgrad_own(pending)
                sums.flush()
                _mark_ready(eng, e)                # this block's gradients are final (mlp.c_proj.bias: by the block above / the tail)
        return dx.view(B, n, W), None
