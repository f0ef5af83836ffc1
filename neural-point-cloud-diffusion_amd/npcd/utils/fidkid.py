"""FID / KID of the reference's diffusion evaluation (npcd/utils/fidkid.py:34-108 -> mmgen FID, pinned at mmgeneration v0.7.2 by the
reference's README.md:30; used by npcd/eval/diffusion_evaluation.py:122-126,179,183).

What is here: the STATISTICS -- feature accumulation, the reference statistics pickle (`mean`, `cov`, `feats_np`), the Frechet
distance and the kernel inception distance (cubic polynomial kernel, random subsets, x 1000) -- in float64.  What is NOT here: the
Inception-v3 network and its weights (`data/inception-2015-12-05.pt`, the per-dataset `*_inception_stylegan.pkl`): they are not part
of the reference repository and not available in this environment, so `feed` takes FEATURES, or images plus a caller-supplied
`feature_extractor`; without one it raises instead of guessing.  Hook for npcd.eval.sample_and_render:
`feed=lambda images: fidkid.feed(images * 2 - 1, "fakes")` (diffusion_evaluation.py:179).

`FIDKID` keeps the features and computes on the host.  `DeviceFIDKID` is the same surface with the statistics on the GPU
(npcd.hip.feature_stats): `feed` leaves nothing on the host and waits for nothing, `summary` reads back once.

With `prdc=True` both also report improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al.
2020) of the same features: `precision_recall_density_coverage` on the host, npcd.hip.feature_manifold on the GPU."""
import pickle
from typing import Callable, Optional

import numpy as np
import torch


def frechet_distance(fake_mean, fake_cov, real_mean, real_cov, eps: float = 1e-6):
    """(fid, mean term, trace term) = ||mu_f - mu_r||^2 + Tr C_f + Tr C_r - 2 Tr (C_f C_r)^(1/2), float64.  The trace of the matrix square
    root is the sum of the square roots of the eigenvalues of C_f^(1/2) C_r C_f^(1/2) (symmetric positive semi-definite: real, no
    complex square root to discard as in the scipy.linalg.sqrtm form of mmgen); a 1e-6 ridge when that is not finite."""
    fm, fc = torch.as_tensor(fake_mean, dtype=torch.float64), torch.as_tensor(fake_cov, dtype=torch.float64)
    rm, rc = torch.as_tensor(real_mean, dtype=torch.float64), torch.as_tensor(real_cov, dtype=torch.float64)

    def tr_sqrt(a, b):
        w, v = torch.linalg.eigh((a + a.T) / 2)
        root = (v * w.clamp_min(0).sqrt()) @ v.T
        m = root @ b @ root
        return torch.linalg.eigvalsh((m + m.T) / 2).clamp_min(0).sqrt().sum()

    t = tr_sqrt(fc, rc)
    if not bool(torch.isfinite(t)):
        ridge = torch.eye(fc.shape[0], dtype=torch.float64) * eps
        t = tr_sqrt(fc + ridge, rc + ridge)
    diff = fm - rm
    mean_norm = float(diff.dot(diff))
    trace = float(torch.trace(fc) + torch.trace(rc) - 2 * t)
    return mean_norm + trace, mean_norm, trace


def kernel_inception_distance(real_feat: np.ndarray, fake_feat: np.ndarray, num_subsets: int = 100, max_subset_size: int = 1000, rng=np.random) -> float:
    """reference fidkid.py:58-82 (without the x 1000 of :105): mean over `num_subsets` random subsets of the unbiased cubic-kernel MMD."""
    n = real_feat.shape[1]
    m = min(min(real_feat.shape[0], fake_feat.shape[0]), max_subset_size)
    t = 0.0
    for _ in range(num_subsets):
        x = torch.from_numpy(fake_feat[rng.choice(fake_feat.shape[0], m, replace=False)]).double()
        y = torch.from_numpy(real_feat[rng.choice(real_feat.shape[0], m, replace=False)]).double()
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += float((a.sum() - torch.diagonal(a).sum()) / (m - 1) - b.sum() * 2 / m)
    return t / num_subsets / m


def _sq_distance_blocks(x: torch.Tensor, y: torch.Tensor, block_rows: int):
    """Yields (i0, d2 [b, m]) over blocks of rows of x: max((|x_i|^2 + |y_j|^2) - 2 x_i . y_j, 0) in float64."""
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    for i0 in range(0, x.shape[0], block_rows):
        xb = x[i0:i0 + block_rows]
        yield i0, ((nx[i0:i0 + block_rows, None] + ny[None, :]) - 2 * (xb @ y.T)).clamp_min(0)


def _kth_self_distance(x: torch.Tensor, k: int, block_rows: int) -> torch.Tensor:
    """rho [n]: the k-th smallest squared distance of every row to the other rows, its own index left out (a duplicate row counts)."""
    rho = torch.empty(x.shape[0], dtype=torch.float64)
    for i0, d2 in _sq_distance_blocks(x, x, block_rows):
        rows = torch.arange(d2.shape[0])
        d2[rows, i0 + rows] = float("inf")
        rho[i0:i0 + d2.shape[0]] = torch.topk(d2, k, dim=1, largest=False).values[:, k - 1]
    return rho


def _prdc_rows(n: int, rows: Optional[int]):
    """The evenly strided rows int(i n / rows) that `prdc_rows` selects out of n (consecutive rows are views of one cloud), or None."""
    if rows is None:
        return None
    if isinstance(rows, bool) or not isinstance(rows, int) or rows < 1 or rows > n:
        raise ValueError(f"prdc_rows must be an integer in [1, {n}], the rows of a side; got {rows!r}")
    return [int(i * n / rows) for i in range(rows)]


def _check_nearest_k(nearest_k, n_real, n_fake):
    if isinstance(nearest_k, bool) or not isinstance(nearest_k, int) or nearest_k < 1:
        raise ValueError(f"nearest_k must be a positive integer; got {nearest_k!r}")
    if min(n_real, n_fake) < nearest_k + 1:
        raise ValueError(f"nearest_k = {nearest_k} needs at least {nearest_k + 1} rows a side; got {n_real} reals and {n_fake} fakes")


def precision_recall_density_coverage(real_feats, fake_feats, nearest_k: int = 5, block_rows: int = 1024) -> dict:
    """Improved precision and recall (Kynkaanniemi et al. 2019) and density and coverage (Naeem et al. 2020) of fake features [M, D]
    against real features [N, D], on the host in float64, `block_rows` rows of the distance matrix at a time.  With d2 the squared
    distance and rho_R[i] (rho_F[j]) the k-th smallest d2 of a real (fake) to the other reals (fakes), the index itself left out:
      precision = mean_j [some i: d2(f_j, r_i) < rho_R[i]]      recall = mean_i [some j: d2(r_i, f_j) < rho_F[j]]
      density = SUM_j #{i: d2(f_j, r_i) < rho_R[i]} / (k M)      coverage = mean_i [min_j d2(r_i, f_j) < rho_R[i]]
    The comparisons are strict, as in the prdc package of Naeem et al."""
    real = torch.as_tensor(np.asarray(real_feats, dtype=np.float64)).reshape(len(real_feats), -1)
    fake = torch.as_tensor(np.asarray(fake_feats, dtype=np.float64)).reshape(len(fake_feats), -1)
    N, M, k = real.shape[0], fake.shape[0], nearest_k
    _check_nearest_k(k, N, M)
    rho_r, rho_f = _kth_self_distance(real, k, block_rows), _kth_self_distance(fake, k, block_rows)
    in_real_balls = fake_inside = 0                     # SUM_j c_F[j], #{j : c_F[j] > 0}
    for _, d2 in _sq_distance_blocks(fake, real, block_rows):
        c = (d2 < rho_r[None, :]).sum(1)
        in_real_balls, fake_inside = in_real_balls + int(c.sum()), fake_inside + int((c > 0).sum())
    real_inside = real_covered = 0                      # #{i : c_R[i] > 0}, #{i : near_R[i] < rho_R[i]}
    for i0, d2 in _sq_distance_blocks(real, fake, block_rows):
        real_inside += int(((d2 < rho_f[None, :]).sum(1) > 0).sum())
        real_covered += int((d2.min(1).values < rho_r[i0:i0 + d2.shape[0]]).sum())
    return dict(precision=fake_inside / M, recall=real_inside / N, density=in_real_balls / (k * M), coverage=real_covered / N)


_PRDC_KEYS = ("precision", "recall", "density", "coverage")


def _prdc_str(prdc: dict) -> str:
    return ", P/R " + "/".join(f"{prdc[k]:.4f}" for k in _PRDC_KEYS[:2]) + ", D/C " + "/".join(f"{prdc[k]:.4f}" for k in _PRDC_KEYS[2:])


class FIDKID:
    """Same surface as the reference's FIDKID (fidkid.py:34-108): `prepare()` loads the reference statistics, `feed(batch, mode)` with
    mode "reals" / "fakes", `summary()` -> (fid, mean term, cov term, kid x 1000) and `_result_dict` / `_result_str`.  With prdc=True
    `summary()` also puts `precision_recall_density_coverage` of the features (`nearest_k`; `prdc_rows`: of that many evenly strided
    rows of each side) into `_result_dict` and behind `_result_str`; its return value stays the 4-tuple."""
    name = "FIDKID"

    def __init__(self, num_images: int, num_subsets: int = 100, max_subset_size: int = 1000, inception_pkl: Optional[str] = None,
                 feature_extractor: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, prdc: bool = False, nearest_k: int = 5,
                 prdc_rows: Optional[int] = None, **_):
        self.num_images, self.num_subsets, self.max_subset_size = num_images, num_subsets, max_subset_size
        self.prdc, self.nearest_k, self.prdc_rows = prdc, nearest_k, prdc_rows
        self.inception_pkl, self.feature_extractor = inception_pkl, feature_extractor
        self.real_feats, self.fake_feats = [], []
        self.real_mean = self.real_cov = self.real_feats_np = None
        self.num_real_feeded = self.num_fake_feeded = 0
        self._result_str, self._result_dict = None, None

    def prepare(self):
        if self.inception_pkl is not None:
            with open(self.inception_pkl, "rb") as f:
                ref = pickle.load(f)
            self.real_mean, self.real_cov, self.real_feats_np = ref["mean"], ref["cov"], ref["feats_np"]
            self.num_real_feeded = self.real_feats_np.shape[0]

    def _features(self, batch: torch.Tensor) -> torch.Tensor:
        if batch.dim() == 2:
            return batch.detach().double().cpu()                     # already features [n, D]
        if self.feature_extractor is None:
            raise RuntimeError("FIDKID.feed was given images but no feature_extractor: the Inception-v3 network of the reference's evaluation "
                               "(data/inception-2015-12-05.pt) is not part of this package -- pass feature_extractor= or feed features [n, D]")
        with torch.no_grad():
            return self.feature_extractor(batch).detach().double().cpu()

    def feed(self, batch: torch.Tensor, mode: str):
        """mode "reals" / "fakes"; at most num_images per side are kept (mmgen Metric.feed)."""
        if mode not in ("reals", "fakes"):
            raise ValueError(mode)
        if mode == "reals" and self.real_feats_np is not None:
            return 0
        have = self.num_real_feeded if mode == "reals" else self.num_fake_feeded
        take = min(batch.shape[0], self.num_images - have)
        if take <= 0:
            return 0
        feats = self._features(batch[:take])
        if mode == "reals":
            self.real_feats.append(feats); self.num_real_feeded += take
        else:
            self.fake_feats.append(feats); self.num_fake_feeded += take
        return take

    def summary(self):
        if self.real_feats_np is None:
            feats = torch.cat(self.real_feats, dim=0)
            assert feats.shape[0] >= self.num_images
            self.real_feats_np = feats[:self.num_images].numpy()
            self.real_mean = np.mean(self.real_feats_np, 0)
            self.real_cov = np.cov(self.real_feats_np, rowvar=False)
        fake = torch.cat(self.fake_feats, dim=0)
        assert fake.shape[0] == self.num_images
        fake_np = fake.numpy()
        fid, mean, cov = frechet_distance(np.mean(fake_np, 0), np.cov(fake_np, rowvar=False), self.real_mean, self.real_cov)
        kid = kernel_inception_distance(self.real_feats_np, fake_np, self.num_subsets, self.max_subset_size) * 1000
        self._result_str = f"{fid:.4f} ({mean:.5f}/{cov:.5f}), {kid:.4f}"
        self._result_dict = dict(fid=fid, fid_mean=mean, fid_cov=cov, kid=kid)
        if self.prdc:
            real_np = np.asarray(self.real_feats_np)
            pick_r, pick_f = _prdc_rows(real_np.shape[0], self.prdc_rows), _prdc_rows(fake_np.shape[0], self.prdc_rows)
            prdc = precision_recall_density_coverage(real_np if pick_r is None else real_np[pick_r],
                                                     fake_np if pick_f is None else fake_np[pick_f], self.nearest_k)
            self._result_dict.update(prdc)
            self._result_str += _prdc_str(prdc)
        return fid, mean, cov, kid


class DeviceFIDKID:
    """`FIDKID`'s surface with the statistics on the GPU.  `feed` keeps the features on the device -- a 2-D batch is
    features, images go through `feature_extractor` -- and accumulates their moments there; it issues no device-to-host copy and no
    host wait.  `summary()` finalises the moments, draws the KID subsets on the host from `rng` in the reference's order (per subset
    first choice(n_fake, m, replace=False), then choice(n_real, ...), so a seeded run reproduces `FIDKID`'s subsets), runs one
    `kid_subsets` launch, reads back once and calls `frechet_distance` in float64 on the host.

    With prdc=True `summary()` also computes precision, recall, density and coverage of the stored features on the device
    (npcd.hip.feature_manifold): two `knn_sq_distances` launches for the radii, two `ball_counts` launches with the
    roles swapped, a device reduction to four doubles that ride in the same read-back.  They go into `_result_dict` and behind
    `_result_str` as in `FIDKID`; the counts behind them are integers, so they equal `precision_recall_density_coverage`'s wherever
    no distance is within rounding of a radius.

    Hook for npcd.eval.sample_and_render: `feed=lambda im: m.feed(im * 2 - 1, "fakes")`."""
    name = "FIDKID"

    def __init__(self, num_images: int, num_subsets: int = 100, max_subset_size: int = 1000, inception_pkl: Optional[str] = None,
                 feature_extractor: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, device=None, block_rows: int = 1024,
                 rng=None, prdc: bool = False, nearest_k: int = 5, prdc_rows: Optional[int] = None, **_):
        self.num_images, self.num_subsets, self.max_subset_size = num_images, num_subsets, max_subset_size
        self.prdc, self.nearest_k, self.prdc_rows = prdc, nearest_k, prdc_rows
        self.inception_pkl, self.feature_extractor = inception_pkl, feature_extractor
        self.device = torch.device("cuda" if device is None else device)
        self.block_rows, self.rng = block_rows, rng
        self.real_mean = self.real_cov = self.real_feats_np = None
        self._real_feats = None                                          # the pickle's features on the device
        self._moments = {"reals": None, "fakes": None}                   # FeatureMoments, made at the first feed of a side
        self.num_real_feeded = self.num_fake_feeded = 0
        self._result_str, self._result_dict = None, None

    def prepare(self):
        if self.inception_pkl is not None:
            with open(self.inception_pkl, "rb") as f:
                ref = pickle.load(f)
            self.real_mean, self.real_cov, self.real_feats_np = ref["mean"], ref["cov"], ref["feats_np"]
            self.num_real_feeded = self.real_feats_np.shape[0]
            feats = np.ascontiguousarray(self.real_feats_np)
            if feats.dtype not in (np.float32, np.float64):
                feats = feats.astype(np.float64)
            self._real_feats = torch.from_numpy(feats).to(self.device)

    def _features(self, batch: torch.Tensor) -> torch.Tensor:
        if batch.dim() == 2:
            feats = batch.detach()                                       # already features [n, D]
        elif self.feature_extractor is None:
            raise RuntimeError("FIDKID.feed was given images but no feature_extractor: the Inception-v3 network of the reference's evaluation "
                               "(data/inception-2015-12-05.pt) is not part of this package -- pass feature_extractor= or feed features [n, D]")
        else:
            with torch.no_grad():
                feats = self.feature_extractor(batch).detach()
        return feats if feats.dtype in (torch.float32, torch.float64) else feats.float()

    def _accumulator(self, mode, feats):
        from npcd.hip.feature_stats import FeatureMoments
        if self._moments[mode] is None:
            # the reals' mean is known before the first fake arrives: the shift that keeps the raw moments from cancelling
            shift = self.real_mean if mode == "fakes" and self.real_mean is not None else None
            self._moments[mode] = FeatureMoments(feats.shape[1], feats.device, shift=shift, max_rows=self.num_images,
                                                 block_rows=self.block_rows)
        return self._moments[mode]

    def feed(self, batch: torch.Tensor, mode: str):
        """mode "reals" / "fakes"; at most num_images per side are kept (mmgen Metric.feed)."""
        if mode not in ("reals", "fakes"):
            raise ValueError(mode)
        if mode == "reals" and self.real_feats_np is not None:
            return 0
        have = self.num_real_feeded if mode == "reals" else self.num_fake_feeded
        take = min(batch.shape[0], self.num_images - have)
        if take <= 0:
            return 0
        feats = self._features(batch[:take])
        self._accumulator(mode, feats).add(feats)
        if mode == "reals":
            self.num_real_feeded += take
        else:
            self.num_fake_feeded += take
        return take

    def _prdc_on_device(self, real_feats, fake_feats):
        """-> float64 [4] on the device: precision, recall, density, coverage.  Nothing is read back here."""
        from npcd.hip.feature_manifold import ball_counts, knn_sq_distances
        k = self.nearest_k
        _check_nearest_k(k, real_feats.shape[0], fake_feats.shape[0])
        pick_r, pick_f = _prdc_rows(real_feats.shape[0], self.prdc_rows), _prdc_rows(fake_feats.shape[0], self.prdc_rows)
        if pick_r is not None:
            real_feats = real_feats[torch.tensor(pick_r, device=real_feats.device)]
            fake_feats = fake_feats[torch.tensor(pick_f, device=fake_feats.device)]
        N, M = real_feats.shape[0], fake_feats.shape[0]
        rho_r, rho_f = knn_sq_distances(real_feats, None, k)[:, k - 1], knn_sq_distances(fake_feats, None, k)[:, k - 1]
        c_f, _ = ball_counts(fake_feats, real_feats, rho_r)
        c_r, near_r = ball_counts(real_feats, fake_feats, rho_f)
        counts = torch.stack([(c_f > 0).sum(), (c_r > 0).sum(), c_f.sum(dtype=torch.int64), (near_r < rho_r).sum()]).double()
        return counts / torch.tensor([M, N, k * M, N], dtype=torch.float64, device=counts.device)

    def summary(self):
        from npcd.hip.feature_stats import kid_from_sums, kid_subsets
        fakes, reals = self._moments["fakes"], self._moments["reals"]
        assert fakes is not None and fakes.rows == self.num_images
        if self._real_feats is None:
            assert reals is not None and reals.rows >= self.num_images
            real_feats, real_stats = reals.features(), reals.finalize()
        else:
            real_feats, real_stats = self._real_feats, ()
        fake_feats = fakes.features()
        fake_mean, fake_cov = fakes.finalize()
        if real_feats.dtype != fake_feats.dtype:
            real_feats, fake_feats = real_feats.double(), fake_feats.double()
        rng = np.random if self.rng is None else self.rng
        n_fake, n_real = fake_feats.shape[0], real_feats.shape[0]
        m = min(min(n_real, n_fake), self.max_subset_size)
        idx_f, idx_r = np.empty((self.num_subsets, m), dtype=np.int64), np.empty((self.num_subsets, m), dtype=np.int64)
        for s in range(self.num_subsets):
            idx_f[s] = rng.choice(n_fake, m, replace=False)
            idx_r[s] = rng.choice(n_real, m, replace=False)
        sums = kid_subsets(fake_feats, real_feats, idx_f, idx_r)
        kid = (kid_from_sums(sums, m) * 1000).reshape(1)
        prdc = (self._prdc_on_device(real_feats, fake_feats),) if self.prdc else ()
        back = torch.cat([t.reshape(-1) for t in (kid, fake_mean, fake_cov, *real_stats, *prdc)]).cpu().numpy()   # the one read-back
        if prdc:
            back, prdc = back[:-4], dict(zip(_PRDC_KEYS, (float(v) for v in back[-4:])))
        D = fake_mean.shape[0]
        kid, fake_mean, fake_cov = float(back[0]), back[1:1 + D], back[1 + D:1 + D + D * D].reshape(D, D)
        if real_stats:
            rest = back[1 + D + D * D:]
            self.real_mean, self.real_cov = rest[:D], rest[D:].reshape(D, D)
        fid, mean, cov = frechet_distance(fake_mean, fake_cov, self.real_mean, self.real_cov)
        self._result_str = f"{fid:.4f} ({mean:.5f}/{cov:.5f}), {kid:.4f}"
        self._result_dict = dict(fid=fid, fid_mean=mean, fid_cov=cov, kid=kid)
        if prdc:
            self._result_dict.update(prdc)
            self._result_str += _prdc_str(prdc)
        return fid, mean, cov, kid
