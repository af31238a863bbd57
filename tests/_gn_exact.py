"""Cases, exact-value data and fp64 references of the GroupNorm dispatch tests (tests/test_gn_exact_host.py proves the data rounding-free
on the CPU, tests/test_gn_dispatch.py runs the kernels on it).  numpy only: nothing here touches the library or a device.

Data set F (forward, eps 1e-6): x integer-valued in [-64, 64], random per element, fixed up so that every (sample, group) sums to m * n with
a small integer m(b, g) that differs between neighbouring groups and samples.  Then mean == m, the fp32 per-thread sums of x and x * x are
integers below 2^24, var = c2 / n - m * m is one rounded fp64 division, and y = fl(fl((x - m) * rstd) * gamma + beta) has two roundings
however the compiler contracts it, because gamma = +-2^k and beta is a multiple of 1/4.

Data set B (backward, eps 0): x = m + s * k with s(b, g) = 2^e and k a permutation, per (sample, group), of the 16-element pattern
6 x 0, 4 x +1, 4 x -1, +2, -2 (mean 0, mean square 1): mean = m, rstd = 1 / s and xhat = k exactly.  dy is integer-valued and random in
[-a, a]; the cases with long pixel columns get every per-(sample, channel) sum of dy fixed up to a small prescribed non-zero integer, so
that gamma * sum dz and (HW s1 + s2 sum xhat) / n share 24 bits (see `CASES`).  Every sum of the backward is then an integer or a multiple
of 1/2 far below 2^24 in any order, and where n = HW * C / G is a power of two so are dx and dx_colsum."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
EPS_F = 1e-6

# id: (B, HW, C, G, |dy| range of set B, fix the per-channel sums of dy, what the case is there for)
CASES = {
    "R1": (3, 64, 128, 32, 8, False, "smallest whole case: <4,256>, wave fold"),
    "R2": (2, 256, 384, 32, 8, False, "<16,256>, LDS walk, 4 idle threads, 294 row slots for 256 rows, 12 channels per group"),
    "R3": (2, 64, 768, 32, 8, False, "<4,256>, LDS walk, E 2, 24 channels per group (the 256x256 network)"),
    "R4": (5, 1024, 256, 32, 4, False, "forward <16,256> E 16, backward wide <8,512> (the 32x32 level of the CIFAR network)"),
    "R5": (3, 900, 128, 32, 4, False, "as R4 but ragged: forward E 15, backward 1024 row slots for 900 rows"),
    "R6": (2, 2000, 128, 32, 4, False, "<16,512> in both directions, ragged"),
    "R7": (515, 16, 128, 32, 8, False, "widest block (cb 128, q 32), one block per sample; grid 515: the tail of the XCD remap"),
    "R8": (513, 64, 256, 32, 8, False, "cb 256, q 64: one wave per group (fwd) / per channel (bwd, 56 idle lanes); grid 513"),
    "R9": (3, 16, 512, 32, 8, False, "E 1 with R 64 > HW: three quarters of the row slots masked"),
    "R10": (2, 1024, 24, 6, 4, False, "<16,512> with the LDS walk and idle threads (q 6, R 85); no planes (C % 32 != 0)"),
    "T1": (2, 4096, 64, 32, 2, True, "two-stage, S 128, 32 rows per split: half of each four-row trip masked; 2 channels per group"),
    "T2": (3, 4100, 128, 32, 2, True, "two-stage, S 128, 33 rows per split: the last splits are empty, one is short"),
    "T3": (2, 1024, 384, 32, 4, False, "two-stage at a resident-sized image (96-byte rows): 192 threads, r 2, S 32"),
    "T4": (40, 1024, 96, 8, 4, False, "two-stage, S 12 (not a power of two), 86 rows per split, ragged; 240 threads"),
    "T5": (2, 4096, 256, 2, 1, True, "128 channels per group: the looped group finalize (items 384 > 256)"),
    "T6": (1, 4096, 1024, 32, 1, True, "r 1: one pixel row per trip, 256 apply blocks"),
}

# what bd_gn_plan reports: ("res", nt, cb, q, R, E, emax) or ("two", S, threads, r, per), forward and backward (DESIGN.md "GroupNorm dispatch")
PLAN = {
    "R1": (("res", 256, 16, 4, 64, 1, 4), ("res", 256, 16, 4, 64, 1, 4)),
    "R2": (("res", 256, 24, 6, 42, 7, 16), ("res", 256, 24, 6, 42, 7, 16)),
    "R3": (("res", 256, 24, 6, 42, 2, 4), ("res", 256, 24, 6, 42, 2, 4)),
    "R4": (("res", 256, 16, 4, 64, 16, 16), ("res", 512, 16, 4, 128, 8, 8)),
    "R5": (("res", 256, 16, 4, 64, 15, 16), ("res", 512, 16, 4, 128, 8, 8)),
    "R6": (("res", 512, 16, 4, 128, 16, 16), ("res", 512, 16, 4, 128, 16, 16)),
    "R7": (("res", 256, 128, 32, 8, 2, 4), ("res", 256, 128, 32, 8, 2, 4)),
    "R8": (("res", 256, 256, 64, 4, 16, 16), ("res", 512, 256, 64, 8, 8, 8)),
    "R9": (("res", 256, 16, 4, 64, 1, 4), ("res", 256, 16, 4, 64, 1, 4)),
    "R10": (("res", 512, 24, 6, 85, 13, 16), ("res", 512, 24, 6, 85, 13, 16)),
    "T1": (("two", 128, 256, 16, 256),) * 2,
    "T2": (("two", 128, 256, 8, 128),) * 2,
    "T3": (("two", 32, 192, 2, 32),) * 2,
    "T4": (("two", 12, 240, 10, 160),) * 2,
    "T5": (("two", 128, 256, 4, 64),) * 2,
    "T6": (("two", 128, 256, 1, 16),) * 2,
}

PATTERN = np.array([0] * 6 + [1] * 4 + [-1] * 4 + [2, -2], dtype=np.int8)
STEP = 7919     # a prime that divides no n or HW of the table: j -> j * STEP mod n is a permutation


def shape(cid):
    return CASES[cid][:4]


def is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def group_size(cid):
    B, HW, C, G = shape(cid)
    return HW * (C // G)


def _rng(cid, salt):
    return np.random.default_rng([ord(cid[0]), int(cid[1:]), salt])


def _to_nhwc(a, B, HW, C, G):
    """[B, G, HW * cpg] (group-major, pixel then channel) -> [B, HW, C]"""
    return np.ascontiguousarray(a.reshape(B, G, HW, C // G).transpose(0, 2, 1, 3)).reshape(B, HW, C)


def per_channel(v, C):
    """[B, G] -> [B, C]"""
    return np.repeat(v, C // v.shape[1], axis=1)


def group_mean(B, G):
    """small integers, different for neighbouring groups and samples"""
    b, g = np.arange(B)[:, None], np.arange(G)[None, :]
    return ((5 * b + 3 * g) % 7 - 3).astype(F64)


def group_scale(B, G):
    b, g = np.arange(B)[:, None], np.arange(G)[None, :]
    return 2.0 ** ((b + 2 * g) % 4 - 2).astype(F64)


def params(cid):
    """gamma = +-2^k, k in {-1, 0, 1}; beta a multiple of 1/4 in [-2, 2]; both per channel"""
    C = shape(cid)[2]
    r = _rng(cid, 1)
    gamma = r.choice([-1.0, 1.0], C) * 2.0 ** r.integers(-1, 2, C)
    beta = r.integers(-8, 9, C) / 4.0
    return gamma.astype(F32), beta.astype(F32)


@functools.lru_cache(maxsize=2)
def set_f(cid):
    """-> x fp32 [B, HW, C] (integer-valued), m fp64 [B, G]"""
    B, HW, C, G = shape(cid)
    n = HW * (C // G)
    m = group_mean(B, G)
    u = _rng(cid, 2).integers(-48, 49, size=(B, G, n)).astype(np.int32)
    d = -u.sum(-1, dtype=np.int64)                    # what the group lacks to sum to 0
    q = d // n
    rem = d - q * n                                   # 0 <= rem < n: +1 on rem elements spread over the group
    pos = (np.arange(n, dtype=np.int64) * STEP) % n
    u += q[..., None].astype(np.int32) + (pos[None, None, :] < rem[..., None])
    x = u + m[..., None].astype(np.int32)
    assert np.abs(x).max() <= 64 and np.array_equal(x.sum(-1, dtype=np.int64), (m * n).astype(np.int64))
    return _to_nhwc(x, B, HW, C, G).astype(F32), m


@functools.lru_cache(maxsize=2)
def set_b(cid):
    """-> x fp32 [B, HW, C], dy fp32 [B, HW, C] (integer-valued), k int8 [B, HW, C], m, s fp64 [B, G]"""
    B, HW, C, G, a, fix = CASES[cid][:6]
    n = HW * (C // G)
    assert n % 16 == 0
    r = _rng(cid, 3)
    k = _to_nhwc(r.permuted(np.tile(PATTERN, (B, G, n // 16)), axis=-1), B, HW, C, G)
    m, s = group_mean(B, G), group_scale(B, G)
    x = per_channel(m, C)[:, None, :] + per_channel(s, C)[:, None, :] * k
    dy = r.integers(-a, a + 1, size=(B, HW, C)).astype(np.int32)
    if fix:
        b, c = np.arange(B)[:, None], np.arange(C)[None, :]
        want = ((b + c) % 3 + 1) * np.where(c % 2, 1, -1)          # per (sample, channel): +-1, +-2, +-3
        perm = (np.arange(HW) * STEP) % HW
        dp = dy[:, perm, :]
        d = want - dp.sum(1)
        sg = np.sign(d).astype(np.int32)[:, None, :]
        can = dp * sg < a                                            # elements that can still move towards the target
        take = can & (np.cumsum(can, axis=1, dtype=np.int32) <= np.abs(d)[:, None, :])
        dp += sg * take
        dy[:, perm, :] = dp
        assert np.array_equal(dy.sum(1), want) and np.abs(dy).max() <= a
    return x.astype(F32), dy.astype(F32), k, m, s


def reference(x, dy, gamma, beta, G, eps, silu):
    """fp64 GroupNorm (+ SiLU) forward and backward of fp32 inputs, with the intermediates the bounds need.  eps as the kernel sees it."""
    B, HW, C = x.shape
    cpg = C // G
    n = HW * cpg
    x = x.astype(F64)
    ga, be = gamma.astype(F64), beta.astype(F64)
    xg = x.reshape(B, HW, G, cpg)
    mean = xg.sum((1, 3)) / n
    c2 = (xg * xg).sum((1, 3))
    var = c2 / n - mean * mean
    rstd = 1.0 / np.sqrt(var + F64(F32(eps)))
    mc, rc = per_channel(mean, C)[:, None, :], per_channel(rstd, C)[:, None, :]
    xh = (x - mc) * rc
    z = xh * ga + be
    out = dict(mean=mean, var=var, rstd=rstd, n=n)
    if silu:
        sig = 1.0 / (1.0 + np.exp(-z))
        out["y"] = z * sig
    else:
        out["y"] = z
    if dy is None:
        return out
    dz = dy.astype(F64)
    if silu:
        dz = dz * (sig * (1.0 + z * (1.0 - sig)))
    sa, e, sh = dz.sum(1), (dz * xh).sum(1), xh.sum(1)              # [B, C]: sum dz, sum dz xhat, sum xhat
    s1 = (sa * ga).reshape(B, G, cpg).sum(-1)
    s2 = (e * ga).reshape(B, G, cpg).sum(-1)
    s1c, s2c = per_channel(s1, C), per_channel(s2, C)
    t = s1c[:, None, :] + xh * s2c[:, None, :]
    w = dz * ga - t / n
    T = HW * s1c + s2c * sh
    wc = sa * ga - T / n
    out.update(xh=xh, dz=dz, sa=sa, e=e, sh=sh, s1=s1, s2=s2, t=t, w=w, dx=rc * w, T=T, wc=wc, colsum=per_channel(rstd, C) * wc,
               dgamma=e.sum(0), dbeta=sa.sum(0), partials=np.stack([e, sa], axis=1))
    return out


def rounded_bound(t, w, rstd_c, n):
    """|fp32 evaluation of rstd (dz gamma - t inv_n) - exact| where inv_n = fl(1 / n) is rounded (n not a power of two), t, dz gamma and rstd
    exact: inv_n carries 2^-24 relative, the product t * inv_n another 2^-24 unless hipcc contracts it into the subtraction, the subtraction 2^-24
    of its result; the product with rstd = 2^-e is exact.  1 % on top for the second-order terms."""
    return 1.01 * 2.0 ** -24 * rstd_c * (2.0 * np.abs(t) / n + np.abs(w))
