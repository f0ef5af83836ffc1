"""All-pairs Chamfer distances between two sets of point clouds on their own kernel (csrc/chamfer.hip): the matrix
under the shape metrics of npcd/eval/shapes.py.

One launch per directed matrix, one float written per cloud pair, the same bits on every run.  There is no CPU fallback: a non-GPU
tensor, a dtype other than fp32 or a cloud above `max_points()` raises RuntimeError.
"""
from typing import Optional, Sequence, Union

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

IntList = Union[int, Sequence[int], torch.Tensor]


def max_points() -> int:
    """Largest P (and Q) supported."""
    return lib().npcd_chamfer_max_points()


def _clouds(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        shape = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)
        raise ValueError(f"chamfer: {name} must be [n, P, 3] with n, P >= 1; got {shape}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"HIP Chamfer distance supports fp32 coordinates; got {t.dtype} for {name}")
    return t


def _lengths(v, n: int, P: int, name: str):
    """Valid points per cloud: host values (an int for every cloud, a sequence, a CPU tensor) are checked here and returned as a
    list; a GPU tensor is returned as it is, never read back (the kernel clamps it to [1, P])."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dim() != 1 or v.shape[0] != n or v.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"chamfer: {name} must be an integer tensor of shape [{n}]; got {v.dtype} {tuple(v.shape)}")
        return v
    if isinstance(v, int):
        v = [v] * n
    out = [int(a) for a in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)]
    if len(out) != n:
        raise ValueError(f"chamfer: {name} has {len(out)} entries for {n} clouds")
    if min(out) < 1 or max(out) > P:
        raise ValueError(f"chamfer: {name} must lie in [1, {P}]; got {out}")
    return out


def _device_i32(v, dev):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=torch.int32).contiguous()
    return torch.tensor(v, dtype=torch.int32).to(dev, non_blocking=True)


def _prepare(x, y, x_lengths, y_lengths):
    """Checked arguments -> (x, y, x_len, y_len) contiguous on the device; y is x itself (one tensor, one pointer) when not given."""
    x = _clouds(x, "x")
    xl = _lengths(x_lengths, x.shape[0], x.shape[1], "x_lengths")
    if y is None:
        if y_lengths is not None:
            raise ValueError("chamfer: y_lengths given without y (the lengths of y = x are x_lengths)")
        yl = xl
    else:
        y = _clouds(y, "y")
        yl = _lengths(y_lengths, y.shape[0], y.shape[1], "y_lengths")
    require_gpu(x, y, *(t for t in (xl, yl) if isinstance(t, torch.Tensor)))
    limit = lib().npcd_chamfer_max_points()
    if x.shape[1] > limit or (y is not None and y.shape[1] > limit):
        raise RuntimeError(f"HIP Chamfer distance supports clouds of up to {limit} points; got {x.shape[1]}"
                           + (f" and {y.shape[1]}" if y is not None else ""))
    dev = x.device
    x = x.detach().contiguous()
    d_xl = _device_i32(xl, dev)
    if y is None:
        return x, x, d_xl, d_xl
    if y.device != dev:
        raise RuntimeError(f"chamfer: x is on {dev}, y on {y.device}")
    return x, y.detach().contiguous(), d_xl, _device_i32(yl, dev)


def _directed(x, x_len, y, y_len):
    out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().npcd_chamfer_directed(ptr(x), ptr(x_len), ptr(y), ptr(y_len), ptr(out), x.shape[0], x.shape[1], y.shape[0],
                                          y.shape[1], stream_ptr()), "npcd_chamfer_directed")
    return out


def chamfer_directed(x: torch.Tensor, y: Optional[torch.Tensor] = None, x_lengths: Optional[IntList] = None,
                     y_lengths: Optional[IntList] = None) -> torch.Tensor:
    """-> [M, N] fp32: out[i, j] = mean over the valid points of x[i] of the squared distance to the nearest valid point of y[j].

    x [M, P, 3], y [N, Q, 3] fp32 on the GPU (any strides: a permuted [n, 3, P] tensor of `generate` is copied once); y = None means
    y = x, the same pointer passed twice.  The squared distance is ((dx dx + dy dy) + dz dz) in fp32 and every minimum is exact; the
    sum over a cloud's points has one fixed order.  x_lengths / y_lengths: valid points per cloud (default all).  Given on the host
    (an int, a list, a CPU tensor) they are checked here, 1 <= length <= P; given as GPU tensors they are never read back -- the call
    waits for nothing -- and the kernel clamps them to [1, P] instead."""
    x, y, xl, yl = _prepare(x, y, x_lengths, y_lengths)
    return _directed(x, xl, y, yl)


def chamfer_matrix(x: torch.Tensor, y: Optional[torch.Tensor] = None, x_lengths: Optional[IntList] = None,
                   y_lengths: Optional[IntList] = None) -> torch.Tensor:
    """-> [M, N] fp32, the symmetric Chamfer distance CD(x_i, y_j) = directed(x, y)[i, j] + directed(y, x)[j, i].  With y = None
    one launch, D + D.T, exactly symmetric with an exactly zero diagonal.  Arguments as for `chamfer_directed`."""
    self_matrix = y is None
    x, y, xl, yl = _prepare(x, y, x_lengths, y_lengths)
    d = _directed(x, xl, y, yl)
    return d + (d if self_matrix else _directed(y, yl, x, xl)).t()
