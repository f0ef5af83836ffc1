"""Feature statistics of the diffusion evaluation on their own kernels (csrc/feature_stats.hip): the mean and the
covariance behind the Frechet distance, accumulated on the device while features arrive, and the cubic-kernel subset sums behind the
kernel inception distance.  The operators under npcd.utils.fidkid.DeviceFIDKID.

Float64 arithmetic on the float64 matrix instruction, on fp32 or fp64 features, no float atomics: the same bits on every run.
`FeatureMoments` flushes whole blocks of rows of its device store, counted from row 0, so its result does not depend on how the
caller cut the stream into calls either.  Nothing is read back.  This module imports without a GPU (`moments_reference` and
`kid_sums_reference` are host restatements of the spec in numpy); only the launches need one.  There is no CPU fallback: a non-GPU
tensor or a dtype other than fp32 / fp64 raises RuntimeError.
"""
import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from . import NPCD_F32, NPCD_F64, check, lib, ptr, require_gpu, stream_ptr

_DTYPES = {torch.float32: NPCD_F32, torch.float64: NPCD_F64}


def tile() -> int:
    """Side of the square block of `gram` that one workgroup owns: entries (i, j) with j // tile >= i // tile are computed."""
    t = ctypes.c_int(0)
    check(lib().npcd_moments_tile(ctypes.byref(t)), "npcd_moments_tile")
    return t.value


def kid_tile() -> int:
    """Side of the square tile of a subset's kernel matrix that one workgroup reduces to one partial sum."""
    t = ctypes.c_int(0)
    check(lib().npcd_kid_tile(ctypes.byref(t)), "npcd_kid_tile")
    return t.value


def max_features() -> int:
    return lib().npcd_moments_max_features()


# ---- the spec, restated on the host ---------------------------------------------------------------------------------------------------------
def moments_reference(x: np.ndarray, shift: Optional[np.ndarray] = None):
    """-> (sum [D], gram [D, D], mean [D], cov [D, D]) in float64 numpy, as the kernels define them: the shifted raw moments, then
    mean = s + sum / n and cov = (gram - n m m^T) / (n - 1) with m = sum / n."""
    x = np.asarray(x, dtype=np.float64)
    n, D = x.shape
    s = np.zeros(D) if shift is None else np.asarray(shift, dtype=np.float64)
    z = x - s
    total, gram = z.sum(0), z.T @ z
    m = total / n
    cov = (gram - n * np.outer(m, m)) / (n - 1) if n > 1 else np.full((D, D), np.nan)
    return total, gram, s + m, cov


def kid_sums_reference(fake: np.ndarray, real: np.ndarray, idx_f: np.ndarray, idx_r: np.ndarray) -> np.ndarray:
    """-> float64 [S, 3]: per subset the sums over i != j of k(x_i, x_j) and of k(y_i, y_j) and the sum over all i, j of k(x_i, y_j),
    k(a, b) = ((a . b) / D + 1)^3, x = fake[idx_f[s]], y = real[idx_r[s]]."""
    fake, real = np.asarray(fake, dtype=np.float64), np.asarray(real, dtype=np.float64)
    D = fake.shape[1]
    out = np.empty((len(idx_f), 3))
    for s, (i_f, i_r) in enumerate(zip(idx_f, idx_r)):
        x, y = fake[i_f], real[i_r]
        off = ~np.eye(len(i_f), dtype=bool)
        kxx, kyy, kxy = ((a @ b.T / D + 1) ** 3 for a, b in ((x, x), (y, y), (x, y)))
        out[s] = kxx[off].sum(), kyy[off].sum(), kxy.sum()
    return out


def kid_from_sums(sums, m: int):
    """The reference's estimate from the three sums [S, 3]: mean over the subsets of (sxx + syy) / (m - 1) - 2 sxy / m, over m."""
    return ((sums[:, 0] + sums[:, 1]) / (m - 1) - 2 * sums[:, 2] / m).mean() / m


# ---- the launches --------------------------------------------------------------------------------------------------------------------------
def _features(op, name, t, D=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{op}: {name} must be features [n, D]; got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
    if D is not None and t.shape[1] != D:
        raise ValueError(f"{op}: {name} has {t.shape[1]} features, expected D = {D}")
    if t.dtype not in _DTYPES:
        raise RuntimeError(f"HIP feature statistics support fp32 and fp64 features; got {t.dtype} for {name}")
    return t.detach()


def _unit_columns(t):
    """Rows addressed by one stride, columns adjacent; only then a copy (on the device)."""
    columns = t.stride(1) == 1 or t.shape[1] == 1
    return t if columns and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _check_D(op, D):
    if isinstance(D, bool) or not isinstance(D, int) or D < 1:
        raise ValueError(f"{op}: D must be a positive integer; got {D!r}")
    if D > max_features():
        raise ValueError(f"{op}: D = {D} is above the {max_features()} features the kernels support")


def moments_update(x: torch.Tensor, r0: int, r1: int, shift: Optional[torch.Tensor], total: torch.Tensor, gram: torch.Tensor):
    """total [D] += the column sums and gram [D, D] += the Gram matrix (upper tiles only) of x[r0:r1] - shift, in place, one launch."""
    x = _unit_columns(x)
    D = x.shape[1]
    ld = x.stride(0) if x.shape[0] > 1 else max(x.stride(0), D)
    with torch.cuda.device(x.device):
        check(lib().npcd_moments_update(ptr(x), _DTYPES[x.dtype], ld, r0, r1, D, ptr(shift), ptr(total), ptr(gram), stream_ptr()),
              "npcd_moments_update")


def moments_finish(total: torch.Tensor, gram: torch.Tensor, shift: Optional[torch.Tensor], n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (mean [D], cov [D, D]) float64 on the device from the sums of n rows; cov is symmetric bit for bit."""
    D = total.shape[0]
    mean, cov = torch.empty_like(total), torch.empty_like(gram)
    with torch.cuda.device(total.device):
        check(lib().npcd_moments_finish(ptr(total), ptr(gram), ptr(shift), D, n, ptr(mean), ptr(cov), stream_ptr()), "npcd_moments_finish")
    return mean, cov


class FeatureMoments:
    """Streaming mean and covariance of D features on the device.

    `add(feats)` appends the rows to a device store [max_rows, D] (the first batch's dtype; allocated at the first add, doubled when
    max_rows is None and it runs full) with one device copy, and launches the moment update over whole blocks of `block_rows` rows
    of the store, counted from row 0.  `finalize()` flushes the remainder into a copy of the sums and returns (mean, cov) as float64
    device tensors.  Flush boundaries depend on the row index only: the bits of the result do not depend on how the stream was cut
    into calls.  `shift` [D] (float64; any estimate of the mean) is subtracted before the products, which keeps cov from cancelling
    against n m m^T.  With keep_features=False there is no store: every add is one update, and the result depends on the cut at
    rounding level.  `rows` is the host count of rows added here, `n` includes merged accumulators."""
    _OP = "FeatureMoments"

    def __init__(self, D: int, device, shift=None, max_rows: Optional[int] = None, block_rows: int = 1024, keep_features: bool = True):
        _check_D(self._OP, D)
        if isinstance(block_rows, bool) or not isinstance(block_rows, int) or block_rows < 1:
            raise ValueError(f"{self._OP}: block_rows must be a positive integer; got {block_rows!r}")
        if max_rows is not None and max_rows < 1:
            raise ValueError(f"{self._OP}: max_rows must be positive; got {max_rows!r}")
        self.D, self.device, self.block_rows, self.max_rows, self.keep_features = D, torch.device(device), block_rows, max_rows, keep_features
        self._shift_host = None if shift is None else np.array(torch.as_tensor(shift).detach().cpu().numpy(), dtype=np.float64)
        if self._shift_host is not None and self._shift_host.shape != (D,):
            raise ValueError(f"{self._OP}: shift must be [{D}]; got {self._shift_host.shape}")
        self.shift = self.sum = self.gram = self._store = None          # on the device from the first add
        self.rows = self.n = self._flushed = 0

    def _accumulators(self):
        if self.sum is None:
            if self.device.type != "cuda":
                raise RuntimeError(f"npcd.hip operators need a GPU device (MI355X); got {self.device}. There is no CPU fallback in the "
                                   "product path.")
            f64 = dict(dtype=torch.float64, device=self.device)
            self.shift = None if self._shift_host is None else torch.from_numpy(self._shift_host).to(self.device)
            self.sum, self.gram = torch.zeros(self.D, **f64), torch.zeros((self.D, self.D), **f64)

    def _room(self, dtype, need):
        if self._store is None:
            self._store = torch.empty((self.max_rows or max(need, self.block_rows), self.D), dtype=dtype, device=self.device)
        if need > self._store.shape[0]:
            if self.max_rows is not None:
                raise ValueError(f"{self._OP}: {need} rows exceed max_rows = {self.max_rows}")
            grown = torch.empty((max(need, 2 * self._store.shape[0]), self.D), dtype=dtype, device=self.device)
            grown[:self.rows].copy_(self._store[:self.rows])
            self._store = grown

    def add(self, feats: torch.Tensor) -> int:
        feats = _features(self._OP, "feats", feats, self.D)
        require_gpu(feats)
        self._accumulators()
        k = feats.shape[0]
        if k == 0:
            return 0
        if not self.keep_features:
            moments_update(feats, 0, k, self.shift, self.sum, self.gram)
            self.rows, self.n, self._flushed = self.rows + k, self.n + k, self.rows + k
            return k
        if self._store is not None and feats.dtype != self._store.dtype:
            raise RuntimeError(f"{self._OP}: the store holds {self._store.dtype}; got {feats.dtype} features")
        self._room(feats.dtype, self.rows + k)
        self._store[self.rows:self.rows + k].copy_(feats)
        self.rows, self.n = self.rows + k, self.n + k
        while self._flushed + self.block_rows <= self.rows:
            moments_update(self._store, self._flushed, self._flushed + self.block_rows, self.shift, self.sum, self.gram)
            self._flushed += self.block_rows
        return k

    def features(self) -> torch.Tensor:
        """The filled part of the store, a view [rows, D]."""
        if not self.keep_features:
            raise RuntimeError(f"{self._OP}: no features are kept with keep_features=False")
        if self._store is None:
            return torch.empty((0, self.D), dtype=torch.float32, device=self.device)
        return self._store[:self.rows]

    def totals(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(sum, gram) over every row so far: the accumulators themselves, or copies with the unflushed remainder added."""
        if self._flushed == self.rows:
            return self.sum, self.gram
        total, gram = self.sum.clone(), self.gram.clone()
        moments_update(self._store, self._flushed, self.rows, self.shift, total, gram)
        return total, gram

    def merge_(self, other: "FeatureMoments") -> "FeatureMoments":
        """Add the sums and the count of another accumulator with the same D and shift (what a rank would all-reduce).  The stores
        are not merged."""
        if not isinstance(other, FeatureMoments) or other.D != self.D:
            raise ValueError(f"{self._OP}: merge_ needs an accumulator with D = {self.D}")
        if (self._shift_host is None) != (other._shift_host is None) or \
                (self._shift_host is not None and not np.array_equal(self._shift_host, other._shift_host)):
            raise ValueError(f"{self._OP}: merge_ needs the same shift on both sides")
        if other.n == 0:
            return self
        self._accumulators()
        total, gram = other.totals()
        self.sum += total.to(self.device)
        self.gram += gram.to(self.device)
        self.n += other.n
        return self

    def finalize(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.n < 2:
            raise ValueError(f"{self._OP}: finalize needs at least 2 rows; got {self.n}")
        total, gram = self.totals()
        return moments_finish(total, gram, self.shift, self.n)


def kid_subsets(fake: torch.Tensor, real: torch.Tensor, idx_f, idx_r) -> torch.Tensor:
    """fake [Nf, D], real [Nr, D]: features on the GPU, one dtype; idx_f, idx_r: host integer arrays [S, m], rows of fake and of real,
    distinct within a subset -> float64 [S, 3] on the device: per subset the sums over i != j of k(x_i, x_j) and k(y_i, y_j) and over
    all i, j of k(x_i, y_j), k(a, b) = ((a . b) / D + 1)^3 (`kid_sums_reference`).  The indices are validated on the host and
    uploaded once; nothing is read back."""
    op = "kid_subsets"
    fake, real = _features(op, "fake", fake), _features(op, "real", real, fake.shape[1])
    D = fake.shape[1]
    _check_D(op, D)
    idx_f, idx_r = np.asarray(idx_f), np.asarray(idx_r)
    for name, idx, rows in (("idx_f", idx_f, fake.shape[0]), ("idx_r", idx_r, real.shape[0])):
        if idx.ndim != 2 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f"{op}: {name} must be an integer array [S, m]; got {idx.dtype} {idx.shape}")
    if idx_f.shape != idx_r.shape:
        raise ValueError(f"{op}: idx_f and idx_r must have one shape; got {idx_f.shape} and {idx_r.shape}")
    S, m = idx_f.shape
    if S < 1 or m < 2:
        raise ValueError(f"{op}: needs S >= 1 subsets of m >= 2 rows; got S = {S}, m = {m}")
    for name, idx, rows in (("idx_f", idx_f, fake.shape[0]), ("idx_r", idx_r, real.shape[0])):
        if int(idx.min()) < 0 or int(idx.max()) >= rows:
            raise ValueError(f"{op}: {name} is out of range: [{int(idx.min())}, {int(idx.max())}] for {rows} rows")
    if fake.dtype != real.dtype:
        raise RuntimeError(f"{op}: fake is {fake.dtype}, real {real.dtype}")
    require_gpu(fake, real)
    dev = fake.device
    if real.device != dev:
        raise RuntimeError(f"{op}: fake is on {dev}, real on {real.device}")
    fake, real = _unit_columns(fake), _unit_columns(real)
    L = lib()
    size = L.npcd_kid_workspace_bytes(S, m)
    if size < 0:
        raise ValueError(f"{op}: S = {S} subsets of m = {m} rows are more tiles than one launch takes")
    dev_idx = [torch.from_numpy(np.ascontiguousarray(i, dtype=np.int32)).to(dev, non_blocking=True) for i in (idx_f, idx_r)]
    workspace = torch.empty(size // 8, dtype=torch.float64, device=dev)
    out = torch.empty((S, 3), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(L.npcd_kid_subsets(ptr(fake), ptr(real), _DTYPES[fake.dtype], fake.shape[0], real.shape[0], D, max(fake.stride(0), D),
                                 max(real.stride(0), D), ptr(dev_idx[0]), ptr(dev_idx[1]), S, m, ptr(workspace), ptr(out), stream_ptr()),
              "npcd_kid_subsets")
    return out
