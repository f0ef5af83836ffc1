"""What the all-pairs cloud distances share (npcd/hip/chamfer.py, npcd/hip/emd.py): the argument preparation -- the same checks, the
same messages but for the operator's name -- and the operator pair itself, `directed` and `matrix` on one C entry point."""
from typing import Callable, Sequence, Union

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

IntList = Union[int, Sequence[int], torch.Tensor]


def clouds(t, name: str, op: str, title: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        shape = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)
        raise ValueError(f"{op}: {name} must be [n, P, 3] with n, P >= 1; got {shape}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"HIP {title} supports fp32 coordinates; got {t.dtype} for {name}")
    return t


def lengths(v, n: int, P: int, name: str, op: str):
    """Valid points per cloud: host values (an int for every cloud, a sequence, a CPU tensor) are checked here and returned as a
    list; a GPU tensor is returned as it is, never read back (the kernel clamps it to [1, P])."""
    if v is None:
        return None
    if isinstance(v, torch.Tensor) and v.is_cuda:
        if v.dim() != 1 or v.shape[0] != n or v.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{op}: {name} must be an integer tensor of shape [{n}]; got {v.dtype} {tuple(v.shape)}")
        return v
    if isinstance(v, int):
        v = [v] * n
    out = [int(a) for a in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)]
    if len(out) != n:
        raise ValueError(f"{op}: {name} has {len(out)} entries for {n} clouds")
    if min(out) < 1 or max(out) > P:
        raise ValueError(f"{op}: {name} must lie in [1, {P}]; got {out}")
    return out


def device_i32(v, dev):
    if v is None:
        return None
    if isinstance(v, torch.Tensor):
        return v.to(device=dev, dtype=torch.int32).contiguous()
    return torch.tensor(v, dtype=torch.int32).to(dev, non_blocking=True)


def prepare(x, y, x_lengths, y_lengths, op: str, title: str, limit):
    """Checked arguments -> (x, y, x_len, y_len) contiguous on the device; y is x itself (one tensor, one pointer) when not given.
    `limit()`: the largest supported cloud, asked of the library only once the arguments are on the GPU."""
    x = clouds(x, "x", op, title)
    xl = lengths(x_lengths, x.shape[0], x.shape[1], "x_lengths", op)
    if y is None:
        if y_lengths is not None:
            raise ValueError(f"{op}: y_lengths given without y (the lengths of y = x are x_lengths)")
        yl = xl
    else:
        y = clouds(y, "y", op, title)
        yl = lengths(y_lengths, y.shape[0], y.shape[1], "y_lengths", op)
    require_gpu(x, y, *(t for t in (xl, yl) if isinstance(t, torch.Tensor)))
    limit = limit()
    if x.shape[1] > limit or (y is not None and y.shape[1] > limit):
        raise RuntimeError(f"HIP {title} supports clouds of up to {limit} points; got {x.shape[1]}"
                           + (f" and {y.shape[1]}" if y is not None else ""))
    dev = x.device
    x = x.detach().contiguous()
    d_xl = device_i32(xl, dev)
    if y is None:
        return x, x, d_xl, d_xl
    if y.device != dev:
        raise RuntimeError(f"{op}: x is on {dev}, y on {y.device}")
    return x, y.detach().contiguous(), d_xl, device_i32(yl, dev)


def pair(op: str, title: str, max_points_symbol: str, directed_symbol: str, combine: Callable):
    """-> (max_points, directed, matrix) of one distance: `directed(x, y, x_lengths, y_lengths)` is one launch of the library's
    `directed_symbol`, `matrix` is combine(directed(x, y), directed(y, x).T), one launch when y is None."""
    def max_points() -> int:
        """Largest P (and Q) supported."""
        return getattr(lib(), max_points_symbol)()

    def launch(x, x_len, y, y_len):
        out = torch.empty((x.shape[0], y.shape[0]), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(getattr(lib(), directed_symbol)(ptr(x), ptr(x_len), ptr(y), ptr(y_len), ptr(out), x.shape[0], x.shape[1], y.shape[0],
                                                  y.shape[1], stream_ptr()), directed_symbol)
        return out

    def directed(x, y, x_lengths, y_lengths):
        x, y, xl, yl = prepare(x, y, x_lengths, y_lengths, op, title, max_points)
        return launch(x, xl, y, yl)

    def matrix(x, y, x_lengths, y_lengths):
        self_matrix = y is None
        x, y, xl, yl = prepare(x, y, x_lengths, y_lengths, op, title, max_points)
        d = launch(x, xl, y, yl)
        return combine(d, (d if self_matrix else launch(y, yl, x, xl)).t())

    return max_points, directed, matrix
