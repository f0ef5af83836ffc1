"""All-pairs approximate earth mover's distances between two sets of point clouds on their own kernel (csrc/emd.hip):
the second matrix under the shape metrics of npcd/eval/shapes.py, beside npcd/hip/chamfer.py.

One launch per directed matrix, one float written per cloud pair, the same bits on every run.  There is no CPU fallback: a non-GPU
tensor, a dtype other than fp32 or a cloud above `max_points()` raises RuntimeError.
"""
from typing import Optional

import torch

from ._clouds import IntList, pair

max_points, _directed, _matrix = pair("emd", "earth mover's distance", "npcd_emd_max_points", "npcd_emd_directed", lambda a, b: 0.5 * (a + b))


def emd_directed(x: torch.Tensor, y: Optional[torch.Tensor] = None, x_lengths: Optional[IntList] = None,
                 y_lengths: Optional[IntList] = None) -> torch.Tensor:
    """-> [M, N] fp32: out[i, j] = the cost of the approximate matching (Fan et al.: ten levels of exp(level d), three passes each)
    between the valid points of x[i] and of y[j], per point of the larger cloud.  Directed: out(x, y) != out(y, x) in general.

    x [M, P, 3], y [N, Q, 3] fp32 on the GPU (any strides: a permuted [n, 3, P] tensor of `generate` is copied once); y = None means
    y = x, the same pointer passed twice.  Distances are Euclidean (the square root of ((dx dx + dy dy) + dz dz)), all arithmetic is
    fp32 and every sum has one fixed order.  x_lengths / y_lengths: valid points per cloud (default all).  Given on the host (an int,
    a list, a CPU tensor) they are checked here, 1 <= length <= P; given as GPU tensors they are never read back -- the call waits
    for nothing -- and the kernel clamps them to [1, P] instead."""
    return _directed(x, y, x_lengths, y_lengths)


def emd_matrix(x: torch.Tensor, y: Optional[torch.Tensor] = None, x_lengths: Optional[IntList] = None,
               y_lengths: Optional[IntList] = None) -> torch.Tensor:
    """-> [M, N] fp32, the symmetric form EMD(x_i, y_j) = 0.5 (directed(x, y)[i, j] + directed(y, x)[j, i]).  With y = None one
    launch, 0.5 (D + D.T), exactly symmetric.  Arguments as for `emd_directed`."""
    return _matrix(x, y, x_lengths, y_lengths)
