"""FID / KID of the reference's diffusion evaluation (npcd/utils/fidkid.py:34-108 -> mmgen FID, pinned at mmgeneration v0.7.2 by the
reference's README.md:30; used by npcd/eval/diffusion_evaluation.py:122-126,179,183).

What is here: the STATISTICS -- feature accumulation, the reference statistics pickle (`mean`, `cov`, `feats_np`), the Frechet
distance and the kernel inception distance (cubic polynomial kernel, random subsets, x 1000) -- in float64.  What is NOT here: the
Inception-v3 network and its weights (`data/inception-2015-12-05.pt`, the per-dataset `*_inception_stylegan.pkl`): they are not part
of the reference repository and not available in this environment, so `feed` takes FEATURES, or images plus a caller-supplied
`feature_extractor`; without one it raises instead of guessing.  Hook for npcd.eval.sample_and_render:
`feed=lambda images: fidkid.feed(images * 2 - 1, "fakes")` (diffusion_evaluation.py:179).

`FIDKID` keeps the features and computes on the host.  `DeviceFIDKID` is the same surface with the statistics on the GPU
(npcd.hip.feature_stats): `feed` leaves nothing on the host and waits for nothing, `summary` reads back once."""
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


class FIDKID:
    """Same surface as the reference's FIDKID (fidkid.py:34-108): `prepare()` loads the reference statistics, `feed(batch, mode)` with
    mode "reals" / "fakes", `summary()` -> (fid, mean term, cov term, kid x 1000) and `_result_dict` / `_result_str`."""
    name = "FIDKID"

    def __init__(self, num_images: int, num_subsets: int = 100, max_subset_size: int = 1000, inception_pkl: Optional[str] = None,
                 feature_extractor: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, **_):
        self.num_images, self.num_subsets, self.max_subset_size = num_images, num_subsets, max_subset_size
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
        return fid, mean, cov, kid


class DeviceFIDKID:
    """`FIDKID`'s surface with the statistics on the GPU.  `feed` keeps the features on the device -- a 2-D batch is
    features, images go through `feature_extractor` -- and accumulates their moments there; it issues no device-to-host copy and no
    host wait.  `summary()` finalises the moments, draws the KID subsets on the host from `rng` in the reference's order (per subset
    first choice(n_fake, m, replace=False), then choice(n_real, ...), so a seeded run reproduces `FIDKID`'s subsets), runs one
    `kid_subsets` launch, reads back once and calls `frechet_distance` in float64 on the host.

    Hook for npcd.eval.sample_and_render: `feed=lambda im: m.feed(im * 2 - 1, "fakes")`."""
    name = "FIDKID"

    def __init__(self, num_images: int, num_subsets: int = 100, max_subset_size: int = 1000, inception_pkl: Optional[str] = None,
                 feature_extractor: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, device=None, block_rows: int = 1024,
                 rng=None, **_):
        self.num_images, self.num_subsets, self.max_subset_size = num_images, num_subsets, max_subset_size
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
        back = torch.cat([t.reshape(-1) for t in (kid, fake_mean, fake_cov, *real_stats)]).cpu().numpy()          # the one read-back
        D = fake_mean.shape[0]
        kid, fake_mean, fake_cov = float(back[0]), back[1:1 + D], back[1 + D:1 + D + D * D].reshape(D, D)
        if real_stats:
            rest = back[1 + D + D * D:]
            self.real_mean, self.real_cov = rest[:D], rest[D:].reshape(D, D)
        fid, mean, cov = frechet_distance(fake_mean, fake_cov, self.real_mean, self.real_cov)
        self._result_str = f"{fid:.4f} ({mean:.5f}/{cov:.5f}), {kid:.4f}"
        self._result_dict = dict(fid=fid, fid_mean=mean, fid_cov=cov, kid=kid)
        return fid, mean, cov, kid
