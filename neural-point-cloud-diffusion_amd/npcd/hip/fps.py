"""Farthest point sampling on its own kernel (csrc/fps.hip): the operator of `pytorch3d.ops.sample_farthest_points`,
which the reference's dataset uses to cut every object's raw surface cloud down to num_points points (npcd/data/srn.py:179-188).

One launch, one workgroup per cloud, integer-exact and the same on every run.  There is no CPU fallback: a non-GPU tensor, a dtype
other than fp32 or a cloud above `max_points()` raises RuntimeError.
"""
import operator
from typing import Optional, Sequence, Union

import torch

from . import check, lib, ptr, require_gpu, stream_ptr

IntList = Union[int, Sequence[int], torch.Tensor]


def resident_points() -> int:
    """Largest P whose clouds stay in registers for the whole call."""
    return lib().npcd_fps_resident_points()


def max_points() -> int:
    """Largest P supported at all."""
    return lib().npcd_fps_max_points()


def _on_host(v) -> bool:
    return not (isinstance(v, torch.Tensor) and v.is_cuda)


def _host_list(v, N: int, name: str):
    """A per-cloud argument given on the host (int sequence or CPU tensor) -> list of N ints."""
    out = [int(x) for x in (v.reshape(-1).tolist() if isinstance(v, torch.Tensor) else v)]
    if len(out) != N:
        raise ValueError(f"sample_farthest_points: {name} has {len(out)} entries for {N} clouds")
    return out


def _device_i32(v, N: int, name: str, dev):
    """A per-cloud argument -> int32 [N] on `dev`: a device tensor is used as it is (never read back), host values are uploaded."""
    if _on_host(v):
        return torch.tensor(v, dtype=torch.int32).to(dev, non_blocking=True)
    if v.dim() != 1 or v.shape[0] != N or v.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"sample_farthest_points: {name} must be an integer tensor of shape [{N}]; got {v.dtype} {tuple(v.shape)}")
    return v.to(device=dev, dtype=torch.int32).contiguous()


def draw_start_indices(lengths: Sequence[int]):
    """The start indices of random_start_point=True: one draw per cloud from torch's default generator, uniform in [0, length),
    in cloud order (an empty cloud draws nothing and gets 0)."""
    return [int(torch.randint(int(n), (1,)).item()) if n > 0 else 0 for n in lengths]


def sample_farthest_points(points: torch.Tensor, lengths: Optional[IntList] = None, K: IntList = 50, random_start_point: bool = False,
                           start_idx: Optional[IntList] = None):
    """-> (selected [N, Kmax, 3] fp32, idx [N, Kmax] int64), Kmax = max(K).

    points [N, P, 3] fp32 on the GPU.  lengths: valid points per cloud (default P).  K: picks per cloud, one int or one per cloud.
    Cloud i makes min(K_i, length_i) picks: the start index (0; drawn on the host when random_start_point; start_idx [N] when given),
    then again and again the valid point farthest from the picks so far in squared fp32 distance ((dx dx + dy dy) + dz dz), the
    lowest index among equals.  Picked rows are bit copies of the input rows; the slots after a cloud's picks hold -1 and 0.0.

    lengths and start_idx given on the host (ints, a list, a CPU tensor) are checked here: 0 <= length <= P, 0 <= start < length.
    Given as GPU tensors they are never read back -- the call then waits for nothing -- and the kernel clamps them into those ranges
    instead.  random_start_point reads GPU lengths back once.  K decides the shape of the result: a GPU tensor K is read back.
    Coordinates are assumed finite; that is not checked."""
    if not isinstance(points, torch.Tensor) or points.dim() != 3 or points.shape[2] != 3:
        shape = tuple(points.shape) if isinstance(points, torch.Tensor) else type(points)
        raise ValueError(f"sample_farthest_points: points must be [N, P, 3]; got {shape} (dimensions other than 3 are not implemented)")
    if points.dtype != torch.float32:
        raise RuntimeError(f"HIP farthest point sampling supports fp32 coordinates; got {points.dtype}")
    N, P = points.shape[0], points.shape[1]
    if N < 1 or P < 1:
        raise ValueError(f"sample_farthest_points: empty input {tuple(points.shape)}")
    if random_start_point and start_idx is not None:
        raise ValueError("sample_farthest_points: give random_start_point or start_idx, not both")

    ks = None
    try:
        Kmax = operator.index(K)
    except TypeError:
        ks = _host_list(K.cpu() if isinstance(K, torch.Tensor) else K, N, "K")
        Kmax = max(ks)
        if min(ks) < 0:
            raise ValueError(f"sample_farthest_points: negative K in {ks}")
    if Kmax < 1:
        raise ValueError(f"sample_farthest_points: K must be at least 1; got {K}")

    host_lengths = None
    if lengths is not None and _on_host(lengths):
        host_lengths = lengths = _host_list(lengths, N, "lengths")
        if min(lengths) < 0 or max(lengths) > P:
            raise ValueError(f"sample_farthest_points: lengths must lie in [0, {P}]; got {lengths}")
    if start_idx is not None and _on_host(start_idx):
        start_idx = _host_list(start_idx, N, "start_idx")
        limit = host_lengths if host_lengths is not None else [P] * N
        for s, n in zip(start_idx, limit):
            if s < 0 or s >= max(n, 1):
                raise ValueError(f"sample_farthest_points: start_idx {start_idx} out of range for lengths {limit}")

    require_gpu(points, *(t for t in (lengths, start_idx) if isinstance(t, torch.Tensor)))
    L = lib()
    if P > L.npcd_fps_max_points():
        raise RuntimeError(f"HIP farthest point sampling supports clouds of up to {L.npcd_fps_max_points()} points; got {P}")
    dev = points.device
    if random_start_point:
        if lengths is None:
            host_lengths = [P] * N
        elif host_lengths is None:
            host_lengths = _host_list(lengths.cpu(), N, "lengths")
        start_idx = draw_start_indices(host_lengths)

    points = points.detach().contiguous()
    d_len = None if lengths is None else _device_i32(lengths, N, "lengths", dev)
    d_ks = None if ks is None else _device_i32(ks, N, "K", dev)
    d_start = None if start_idx is None else _device_i32(start_idx, N, "start_idx", dev)
    idx = torch.empty((N, Kmax), dtype=torch.int64, device=dev)
    sel = torch.empty((N, Kmax, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(L.npcd_fps(ptr(points), ptr(d_len), ptr(d_ks), ptr(d_start), ptr(idx), ptr(sel), N, P, Kmax, stream_ptr()), "npcd_fps")
    return sel, idx
