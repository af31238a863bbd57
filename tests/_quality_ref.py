"""fp64 numpy restatement of the quality metrics on features (k-NN radii, precision / recall / density / coverage, KID) on the SAME fp32
inputs the kernels read: the yardstick of test_quality.py and test_quality_host.py.  Squared distances and all comparisons on them."""
import numpy as np


def sqdist(a, b):
    """[Na, Nb] squared distances; the dtype of the inputs decides the arithmetic (float64 or int64)"""
    return np.stack([((a[i:i + 1] - b) ** 2).sum(1) for i in range(a.shape[0])])


def ksmallest(d2, k, self_col0=None):
    """[Na, k] ascending: the k smallest of each row, column i + self_col0 left out (None: none)"""
    rows = []
    for i in range(d2.shape[0]):
        r = d2[i]
        if self_col0 is not None and 0 <= i + self_col0 < r.shape[0]:
            r = np.delete(r, i + self_col0)
        r = np.sort(r)[:k].astype(np.float64)
        rows.append(np.concatenate([r, np.full(k - r.shape[0], np.inf)]))
    return np.stack(rows)


def knn_sqradius(x, k):
    return ksmallest(sqdist(x, x), k, 0)[:, k - 1]


def count_min(d2, radius2=None):
    return (None if radius2 is None else (d2 <= radius2[None, :]).sum(1)), d2.min(1)


def prdc(real, fake, k, radius_scale=1.0):
    """the definitions of metrics.prdc with every radius^2 multiplied by radius_scale"""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    r_real, r_fake = knn_sqradius(real, k) * radius_scale, knn_sqradius(fake, k) * radius_scale
    d2 = sqdist(fake, real)                                   # [fake, real]
    in_real = (d2 <= r_real[None, :]).sum(1)
    in_fake = (d2.T <= r_fake[None, :]).sum(1)
    return {"precision": float((in_real > 0).mean()), "recall": float((in_fake > 0).mean()),
            "density": float(in_real.sum() / (k * fake.shape[0])), "coverage": float((d2.min(0) <= r_real).mean()), "k": k}


def mmd2_poly3(x, y, dtype=np.float64):
    """(unbiased MMD^2 with k(x, y) = (x.y / d + 1)^3, the mean kernel value): the dot products in `dtype`, the rest in fp64"""
    d, m = x.shape[1], x.shape[0]
    x, y = x.astype(dtype), y.astype(dtype)
    kxx, kyy, kxy = ((np.matmul(p, q.T).astype(np.float64) / d + 1.0) ** 3 for p, q in ((x, x), (y, y), (x, y)))
    s_xx, s_yy, s_xy = kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()
    return s_xx / (m * (m - 1)) + s_yy / (m * (m - 1)) - 2.0 * s_xy / (m * m), (kxx.mean() + kyy.mean() + kxy.mean()) / 3.0


def kid(real, fake, index_pairs, dtype=np.float64):
    """(mean, std, mean kernel value) over the subsets given as (real rows, fake rows) index arrays"""
    vals = [mmd2_poly3(real[np.asarray(ri)], fake[np.asarray(fi)], dtype) for ri, fi in index_pairs]
    v = np.array([a for a, _ in vals])
    return float(v.mean()), float(v.std()), float(np.mean([s for _, s in vals])), v
