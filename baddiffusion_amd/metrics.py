"""Measure path (SURVEY f-3): MSE / SSIM against the backdoor target and the Frechet statistics, on the device.

Reference call sites: baddiffusion.py:536-547 (`nn.MSELoss`, `StructuralSimilarityIndexMeasure(data_range=1.0)` on
`[N,3,S,S]` images in [0,1]) and fid_score.py:150-230 (activation statistics + Frechet distance over pool3 features).
* `ActivationStats` accumulates sum and sum of outer products in fp64 ON THE GPU, batch by batch (no [N, 2048] host
  array); `frechet_distance` then needs one matrix square root of a d x d product, which stays on scipy / CPU.
* SSIM follows the published torchmetrics defaults the reference relies on (11x11 Gaussian, sigma 1.5, k1 0.01,
  k2 0.03, reflect padding, border crop, mean over C,H,W then over the batch) and exists only as the HIP kernel bd_ssim
  (csrc/metrics.hip).  torchmetrics is not installed in the build container, so SSIM parity against torchmetrics itself is
  UNPINNED; the kernel is checked against the independent fp64 scipy statement in oracle/metrics_ref.py.
  Frechet / statistics are pinned by G8.
* The Inception pool3 network (pytorch_fid weights) is an asset that does not travel: callers pass any feature
  extractor `f(images) -> [n, d]`.
"""
import numpy as np
import torch

from .likelihood import bits_per_dim  # noqa: F401  -- the variational bound in bits per dimension (likelihood.py, kernel bd_vb_terms)


def mse(a, b):
    """nn.MSELoss(reduction='mean') (baddiffusion.py:545) through the fused l2-loss kernel (bd_loss_fwd_bwd): the difference
    is taken in fp32, its squares are accumulated in fp64 partial sums folded in fixed order.  Device tensors only: there is
    no CPU path (tests pin the kernel against the fp64 formula in oracle/metrics_ref.py, |err| <= 1e-6 relative)."""
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError("metrics.mse: device tensors required (the measure path runs on the GPU; no CPU fallback)")
    if a.shape != b.shape:
        raise ValueError(f"mse: shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    from . import ops
    a32, b32 = a.float().contiguous(), b.float().contiguous()
    loss, _ = ops.loss_fwd_bwd(a32.reshape(-1, a32.shape[-1]), b32.reshape(-1, b32.shape[-1]), "l2", want_grad=False)
    return float(loss)


def ssim(preds, target, data_range=1.0):
    """Mean SSIM of two [N,C,H,W] batches with the torchmetrics defaults the reference relies on (baddiffusion.py:260,546):
    the HIP kernel bd_ssim.  Device tensors only; images must be larger than the 11-tap window."""
    if preds.shape != target.shape or preds.dim() != 4:
        raise ValueError(f"expected two [N,C,H,W] tensors of the same shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    if not (preds.is_cuda and target.is_cuda):
        raise RuntimeError("metrics.ssim: device tensors required (bd_ssim is a HIP kernel; no CPU fallback)")
    if min(preds.shape[-2:]) <= 10:
        raise ValueError("ssim: images must be larger than the 11x11 window")
    from . import ops
    return float(ops.ssim(preds.float(), target.float(), data_range))


def _need_device(who, *ts):
    if not all(t.is_cuda for t in ts):
        raise RuntimeError(f"metrics.{who}: device tensors required (the measure path runs on the GPU; no CPU fallback)")


def mse_per_image(preds, target):
    """The MSE of every image on its own: a float32 [N] DEVICE tensor, out[n] = mean((preds[n] - target[n])^2) (HIP kernel bd_image_loss:
    fp32 differences, fp64 sums).  preds: [N,C,H,W] in any memory format; target: [N,C,H,W], or [1,C,H,W] / [C,H,W] shared by all images
    (passed by stride, never expanded in memory).  An image's value does not depend on the storage order or on the batch around it."""
    _need_device("mse_per_image", preds, target)
    from . import ops
    return ops.image_loss(preds.float(), target.float(), "l2")


def ssim_per_image(preds, target, data_range=1.0):
    """The SSIM of every image on its own (the definition of `ssim`, HIP kernel bd_ssim_images): a float32 [N] DEVICE tensor.  Arguments
    and properties as for mse_per_image; images must be larger than the 11-tap window."""
    _need_device("ssim_per_image", preds, target)
    if preds.dim() != 4 or min(preds.shape[-2:]) <= 10:
        raise ValueError(f"ssim_per_image: [N,C,H,W] images larger than the 11x11 window are required, got {tuple(preds.shape)}")
    from . import ops
    return ops.ssim_images(preds.float(), target.float(), data_range)


def attack_success_rate(images, target, threshold):
    """(asr, mse): mse = mse_per_image(images, target), the [N] device tensor, and asr = count(mse < threshold) / N as a float -- the
    share of images whose OWN distance to the backdoor target is below the threshold (strict; counted on the device).  The threshold
    is the caller's: the literature uses values of the order of 1e-3 on [0, 1] images, and this project has fitted none."""
    per = mse_per_image(images, target)
    return int((per < float(threshold)).sum()) / per.numel(), per


def pairwise_sqdist(images):
    """[N, N] device tensor of squared Euclidean distances between the flattened images of an [N, ...] float batch: the HIP kernel
    bd_pairwise_sqdist, which subtracts in fp32 before it squares (never |a|^2 + |b|^2 - 2ab: that cancels on the near-identical
    images a backdoored model produces).  Symmetric bit for bit, exact zeros on the diagonal and between duplicates."""
    if not images.is_cuda:
        raise RuntimeError("metrics.pairwise_sqdist: device tensors required (bd_pairwise_sqdist is a HIP kernel; no CPU fallback)")
    if images.dim() < 1 or images.shape[0] < 1 or images.numel() == 0:
        raise ValueError(f"pairwise_sqdist: expected a non-empty [N, ...] batch, got {tuple(images.shape)}")
    from . import ops
    return ops.pairwise_sqdist(images.float().contiguous().reshape(images.shape[0], -1))


def uniformity(images):
    """Mean pairwise Euclidean distance of a batch: mean over the unordered pairs i < j of sqrt(d2[i][j]), the square root and the mean
    taken in fp64 on the device.  Small when the batch has collapsed onto one image (the backdoor target)."""
    n = images.shape[0] if images.dim() >= 1 else 0
    if n < 2:
        raise ValueError(f"uniformity: needs at least two images, got {n}")
    if not images.is_cuda:
        raise RuntimeError("metrics.uniformity: device tensors required (the measure path runs on the GPU; no CPU fallback)")
    d2 = pairwise_sqdist(images)
    i, j = torch.triu_indices(n, n, offset=1, device=d2.device)
    return float(d2[i, j].double().sqrt().mean())


def total_variation(images):
    """Mean over the batch of tv[n] / (C*H*W), tv[n] = the sum over channels of the absolute vertical and horizontal neighbour
    differences of image n (HIP kernel bd_total_variation: fp32 differences, fp64 sums).  [N,C,H,W] in either memory format."""
    if not images.is_cuda:
        raise RuntimeError("metrics.total_variation: device tensors required (bd_total_variation is a HIP kernel; no CPU fallback)")
    if images.dim() != 4 or images.numel() == 0:
        raise ValueError(f"total_variation: expected a non-empty [N,C,H,W] tensor, got {tuple(images.shape)}")
    from . import ops
    tv = ops.total_variation(images.float())
    return float(tv.double().mean() / (images.shape[1] * images.shape[2] * images.shape[3]))


class ActivationStats:
    """Running mean / covariance of feature rows, accumulated in fp64 on the features' device
    (fid_score.py:207-230: mu = mean(act, 0), sigma = np.cov(act, rowvar=False))."""

    def __init__(self, dim, device=None):
        self.n = 0
        self.s = torch.zeros(dim, dtype=torch.float64, device=device)
        self.ss = torch.zeros(dim, dim, dtype=torch.float64, device=device)

    def update(self, act):
        a = act.reshape(act.shape[0], -1).to(device=self.s.device, dtype=torch.float64)
        self.n += a.shape[0]
        self.s += a.sum(0)
        self.ss += a.t() @ a
        return self

    def finalize(self):
        if self.n < 2:
            raise ValueError("need at least two feature rows")
        mu = self.s / self.n
        cov = (self.ss - self.n * torch.outer(mu, mu)) / (self.n - 1)
        return mu.cpu().numpy(), cov.cpu().numpy()


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """Squared Frechet distance between N(mu1, sigma1) and N(mu2, sigma2):
    |mu1 - mu2|^2 + Tr(sigma1) + Tr(sigma2) - 2 Tr((sigma1 sigma2)^(1/2)).
    Behaviour kept from fid_score.py:150-204 (pinned by G8): a non-finite square root is retried once with eps added to both
    diagonals, and a complex root is accepted only if its diagonal is real to 1e-3."""
    from scipy import linalg
    m = [np.atleast_1d(np.asarray(v, np.float64)) for v in (mu1, mu2)]
    S = [np.atleast_2d(np.asarray(v, np.float64)) for v in (sigma1, sigma2)]
    if m[0].shape != m[1].shape:
        raise ValueError("Training and test mean vectors have different lengths")
    if S[0].shape != S[1].shape:
        raise ValueError("Training and test covariances have different dimensions")

    def root_of_product(jitter):
        r = linalg.sqrtm((S[0] + jitter) @ (S[1] + jitter), disp=False)
        return r[0] if isinstance(r, tuple) else r
    root = root_of_product(0.0)
    if not np.all(np.isfinite(root)):
        root = root_of_product(eps * np.eye(S[0].shape[0]))
    if np.iscomplexobj(root):
        worst = float(np.abs(np.diagonal(root).imag).max())
        if worst > 1e-3:
            raise ValueError(f"Imaginary component {worst}")
        root = root.real
    gap = m[0] - m[1]
    return float(gap @ gap + np.trace(S[0]) + np.trace(S[1]) - 2.0 * np.trace(root))


def fid_from_features(features_a, features_b, stores=None):
    """Frechet distance between two iterables of feature batches ([n, d] tensors).  stores: a pair of FeatureStore that keep the
    batches of the two sets for the metrics that need the rows themselves (prdc, kid)."""
    stats = []
    for which, feats in enumerate((features_a, features_b)):
        acc = None
        for f in feats:
            acc = acc or ActivationStats(f.reshape(f.shape[0], -1).shape[1], f.device)
            acc.update(f)
            if stores is not None:
                stores[which].update(f)
        stats.append(acc.finalize())
    return frechet_distance(stats[0][0], stats[0][1], stats[1][0], stats[1][1])


# ---------------------------------------------------------------------------------------------------- quality metrics on features
# Improved precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and KID (Binkowski et al. 2018) on
# [N, d] feature rows (pool3 features, or anything else a caller extracts).  The pairwise work runs in the strip kernels of
# csrc/quality.hip (direct differences, no N x M matrix); what is left here is O(N) per set.  DESIGN.md section 3.
def _features(who, *sets):
    out = []
    for f in sets:
        if not torch.is_tensor(f) or not f.is_cuda:
            raise RuntimeError(f"metrics.{who}: device tensors required (the pairwise kernels are HIP kernels; no CPU fallback)")
        if f.dim() < 2 or f.shape[0] < 1 or f.numel() == 0:
            raise ValueError(f"{who}: expected non-empty [N, d] features, got {tuple(f.shape)}")
        out.append(f.float().reshape(f.shape[0], -1).contiguous())
    if len({f.shape[1] for f in out}) != 1:
        raise ValueError(f"{who}: the feature dimensions differ: {[tuple(f.shape) for f in out]}")
    return out


def knn_sqradius(features, k):
    """float32 [N] device tensor: the squared distance from every row of `features` ([N, d], device) to its k-th nearest OTHER row
    (HIP kernel bd_knn_sqradius: self is left out by index, so a duplicate row has radius 0; 1 <= k <= min(16, N - 1))."""
    (f,) = _features("knn_sqradius", features)
    k = int(k)
    if not 1 <= k <= min(16, f.shape[0] - 1):
        raise ValueError(f"knn_sqradius: k={k} must be in [1, min(16, N - 1 = {f.shape[0] - 1})]")
    from . import ops
    return ops.knn_sqradius(f, k)


def _prdc_counts(real, fake, k):
    from . import ops
    r_real, r_fake = knn_sqradius(real, k), knn_sqradius(fake, k)       # once per set
    in_real, _ = ops.cross_count_min(fake, real, r_real)                 # per fake sample: the real balls it lies in
    in_fake, nearest_fake = ops.cross_count_min(real, fake, r_fake)      # per real sample: the fake balls it lies in; its nearest fake
    return r_real, in_real, in_fake, nearest_fake


def prdc(real, fake, k=5):
    """{"precision", "recall", "density", "coverage", "k"} of two feature sets ([N_real, d] and [N_fake, d] device tensors), Naeem et
    al. 2020 with the manifolds of Kynkaanniemi et al. 2019.  r_X(j) is the distance from x_j to its k-th nearest other member of X:
      precision = mean_i [ fake_i lies in some ball B(real_j, r_real(j)) ]       recall = the same with the roles exchanged
      density   = sum_i #{ j : fake_i in B(real_j, r_real(j)) } / (k N_fake)     coverage = mean_j [ min_i d(real_j, fake_i) <= r_real(j) ]
    Every comparison is on SQUARED distances and is `<=`.  The `prdc` package compares with strict `<`; the two differ only where a
    distance equals a radius exactly (duplicates, integer-valued features), where `<=` counts the k-th neighbour itself as inside its
    ball, which is what "within the k-NN radius" says.  Squared distances are bd_pairwise_sqdist's arithmetic (difference first), so
    near-duplicate samples -- a collapsed model -- do not cancel."""
    real, fake = _features("prdc", real, fake)
    k = int(k)
    r_real, in_real, in_fake, nearest_fake = _prdc_counts(real, fake, k)
    n_real, n_fake = real.shape[0], fake.shape[0]          # integer counts from the device, one correctly rounded division each on the host
    return {"precision": int((in_real > 0).sum()) / n_fake, "recall": int((in_fake > 0).sum()) / n_real,
            "density": int(in_real.sum(dtype=torch.int64)) / (k * n_fake), "coverage": int((nearest_fake <= r_real).sum()) / n_real, "k": k}


def precision_recall(real, fake, k=3):
    """{"precision", "recall", "k"}: improved precision and recall (Kynkaanniemi et al. 2019; k = 3 is that paper's default), the
    first two scores of `prdc` at that k."""
    res = prdc(real, fake, k)
    return {"precision": res["precision"], "recall": res["recall"], "k": res["k"]}


class KidResult(tuple):
    """(mean, std) of the per-subset MMD^2 estimates; also .mean, .std, .values (one per subset), .subsets, .subset_size and
    .warning (None, or why subset_size is not what was asked for)"""

    def __new__(cls, values, subset_size, warning):
        self = super().__new__(cls, (float(np.mean(values)), float(np.std(values))))
        self.values, self.subsets, self.subset_size, self.warning = list(values), len(values), int(subset_size), warning
        return self

    mean = property(lambda self: self[0])
    std = property(lambda self: self[1])


def kid_subset_indices(n_real, n_fake, subsets, subset_size, generator=None):
    """the rows of every KID subset: a list of (real rows, fake rows) int64 CPU tensors, each subset_size rows drawn without
    replacement as torch.randperm(n, generator=generator)[:subset_size], real first, subset after subset"""
    return [(torch.randperm(n_real, generator=generator)[:subset_size], torch.randperm(n_fake, generator=generator)[:subset_size])
            for _ in range(subsets)]


def kid(real, fake, subsets=100, subset_size=1000, generator=None):
    """Kernel Inception Distance (Binkowski et al. 2018): KidResult, which unpacks as (mean, std), over `subsets` draws of the
    unbiased MMD^2 with the kernel k(x, y) = (x.y / d + 1)^3 between subset_size rows of each set (kid_subset_indices; `generator`
    is a CPU torch.Generator):  S_xx / (m (m - 1)) + S_yy / (m (m - 1)) - 2 S_xy / m^2, the diagonal left out of S_xx and S_yy.
    The dot products are fp32 FMA chains, the kernel values and all sums fp64 (HIP kernel bd_poly3_rowsum).  subset_size is capped at
    the smaller set; the result's .warning says so.  std is the population standard deviation of the subset values."""
    real, fake = _features("kid", real, fake)
    subsets, subset_size = int(subsets), int(subset_size)
    if subsets < 1 or subset_size < 2:
        raise ValueError(f"kid: subsets={subsets} must be >= 1 and subset_size={subset_size} >= 2")
    warning = None
    smaller = min(real.shape[0], fake.shape[0])
    if subset_size > smaller:
        warning = f"subset_size {subset_size} capped at the smaller set's {smaller} rows"
        subset_size = smaller
        if subset_size < 2:
            raise ValueError("kid: both sets need at least two rows")
    from . import ops
    m = subset_size
    values = []
    for ri, fi in kid_subset_indices(real.shape[0], fake.shape[0], subsets, m, generator):
        x, y = real[ri.to(real.device)], fake[fi.to(fake.device)]
        s_xx, s_yy, s_xy = (ops.poly3_rowsum(x, x, True).sum(), ops.poly3_rowsum(y, y, True).sum(), ops.poly3_rowsum(x, y, False).sum())
        values.append(float(s_xx / (m * (m - 1)) + s_yy / (m * (m - 1)) - 2.0 * s_xy / (m * m)))
    return KidResult(values, m, warning)


class FeatureStore:
    """Feature batches ([n, d] device tensors) gathered into ONE float32 device tensor, so that the k-NN and KID kernels can read what
    ActivationStats only sums (80 MB at 10 000 x 2048).  update() appends (the buffer doubles when it is full); features() is the
    [N, d] view of what has arrived."""

    def __init__(self, capacity=0):
        self.n, self.buf, self.capacity = 0, None, int(capacity)

    def update(self, act):
        a = act.reshape(act.shape[0], -1).float()
        if self.buf is None:
            self.buf = torch.empty(max(self.capacity, a.shape[0]), a.shape[1], device=a.device)
        if a.shape[1] != self.buf.shape[1]:
            raise ValueError(f"FeatureStore: batch of width {a.shape[1]} after width {self.buf.shape[1]}")
        if self.n + a.shape[0] > self.buf.shape[0]:
            grown = torch.empty(max(2 * self.buf.shape[0], self.n + a.shape[0]), self.buf.shape[1], device=self.buf.device)
            grown[: self.n] = self.buf[: self.n]
            self.buf = grown
        self.buf[self.n: self.n + a.shape[0]] = a
        self.n += a.shape[0]
        return self

    def features(self):
        if self.buf is None:
            raise ValueError("FeatureStore: no features yet")
        return self.buf[: self.n]


def quality_scores(real, fake, prdc_k=None, kid_opts=None, generator=None):
    """the score.json / quality.json keys of the quality metrics asked for: precision / recall / density / coverage / PRDC_k with
    prdc_k, KID_mean / KID_std / KID_subsets / KID_subset_size (/ KID_warning) with kid_opts = {"subsets", "subset_size"}"""
    out = {}
    if prdc_k is not None:
        res = prdc(real, fake, prdc_k)
        out.update({n: res[n] for n in QUALITY_PRDC_KEYS[:4]}, PRDC_k=res["k"])
    if kid_opts is not None:
        res = kid(real, fake, generator=generator, **kid_opts)
        out.update(KID_mean=res.mean, KID_std=res.std, KID_subsets=res.subsets, KID_subset_size=res.subset_size)
        if res.warning:
            out["KID_warning"] = res.warning
    return out


QUALITY_PRDC_KEYS = ("precision", "recall", "density", "coverage", "PRDC_k")
QUALITY_KID_KEYS = ("KID_mean", "KID_std", "KID_subsets", "KID_subset_size")
