"""All-pairs Chamfer distances between two sets of point clouds on their own kernel (csrc/chamfer.hip): the matrix
under the shape metrics of npcd/eval/shapes.py.

One launch per directed matrix, one float written per cloud pair, the same bits on every run.  There is no CPU fallback: a non-GPU
tensor, a dtype other than fp32 or a cloud above `max_points()` raises RuntimeError.
"""
from typing import Optional

import torch

from ._clouds import IntList, pair

max_points, _directed, _matrix = pair("chamfer", "Chamfer distance", "npcd_chamfer_max_points", "npcd_chamfer_directed", lambda a, b: a + b)


def chamfer_directed(x: torch.Tensor, y: Optional[torch.Tensor] = None, x_lengths: Optional[IntList] = None,
                     y_lengths: Optional[IntList] = None) -> torch.Tensor:
    """-> [M, N] fp32: out[i, j] = mean over the valid points of x[i] of the squared distance to the nearest valid point of y[j].

    x [M, P, 3], y [N, Q, 3] fp32 on the GPU (any strides: a permuted [n, 3, P] tensor of `generate` is copied once); y = None means
    y = x, the same pointer passed twice.  The squared distance is ((dx dx + dy dy) + dz dz) in fp32 and every minimum is exact; the
    sum over a cloud's points has one fixed order.  x_lengths / y_lengths: valid points per cloud (default all).  Given on the host
    (an int, a list, a CPU tensor) they are checked here, 1 <= length <= P; given as GPU tensors they are never read back -- the call
    waits for nothing -- and the kernel clamps them to [1, P] instead."""
    return _directed(x, y, x_lengths, y_lengths)


def chamfer_matrix(x: torch.Tensor, y: Optional[torch.Tensor] = None, x_lengths: Optional[IntList] = None,
                   y_lengths: Optional[IntList] = None) -> torch.Tensor:
    """-> [M, N] fp32, the symmetric Chamfer distance CD(x_i, y_j) = directed(x, y)[i, j] + directed(y, x)[j, i].  With y = None
    one launch, D + D.T, exactly symmetric with an exactly zero diagonal.  Arguments as for `chamfer_directed`."""
    return _matrix(x, y, x_lengths, y_lengths)
