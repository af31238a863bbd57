"""GPU: the strip kernels of csrc/quality.hip (bd_knn_sqradius, bd_cross_ksmallest, bd_cross_count_min, bd_poly3_rowsum), the metrics
built on them (metrics.knn_sqradius / prdc / precision_recall / kid), quality_eval.py and the measure-mode flags.

Yardstick: the fp64 formula on the same fp32 inputs (tests/_quality_ref.py), the basis test_defense.py uses for bd_pairwise_sqdist.
Bounds.  Integer-valued rows from {-3 ... 3}: every squared distance (<= 36 D < 2^24) and every dot product is exact in fp32, so radii,
counts and minima must equal the int64 results bit for bit, and the kernel row sums are fp64 roundings only (1e-12 relative).  Real
data: eps = (D + 2) 2^-24 relative per squared distance -- one rounding for the difference, one for the square, at most D - 1 for a sum
of non-negative terms in any order; order statistics and minima are monotone in every distance and inherit it; a count lies between
the fp64 counts at radius^2 / (1 + eps) and radius^2 (1 + eps).  KID: max(4e-6 S, 4 d32), S the mean kernel value (the scale at which
the three terms cancel) and d32 the deviation of the same formula with a numpy float32 matmul."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests import _quality_ref as R
from tests.golden import cases as C

U24 = 2.0 ** -24
# (Na, Nb, D): smallest legal | ragged edges | exact tile | one past the tile | several strips and tiles | few strips: the column tiles
# are split over workgroups | B smaller than a tile
SHAPES = [(1, 2, 1), (63, 65, 31), (64, 64, 32), (65, 130, 33), (130, 323, 70), (5, 1000, 2048), (200, 7, 100)]
KS = (1, 3, 5, 16)


@pytest.fixture(scope="module")
def bd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from baddiffusion_amd import _lib as L
    import baddiffusion_amd.ops as ops
    return L, ops


def layouts(x):
    """(name, view of the same values): contiguous and 16-byte aligned | row stride D + 3 starting one float in (4-byte aligned only)"""
    N, D = x.shape
    big = torch.zeros(N, D + 3, device="cuda")
    big[:, 1:1 + D] = x
    v = big[:, 1:1 + D]
    assert v.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0
    return [("aligned", x), ("offset", v)]


def _ws(nbytes):
    """a NaN-filled workspace (8-byte aligned) and its pointer"""
    ws = torch.full((max((nbytes + 7) // 8, 1),), float("nan"), device="cuda", dtype=torch.float64)
    return ws, (ws.data_ptr() if nbytes else None)


def _ld(x):
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def run_knn(L, x, k):
    lib = L.load()
    N, D = x.shape
    out = torch.full((N,), float("nan"), device="cuda")
    nbytes = lib.bd_knn_sqradius_workspace_bytes(N, D, k)
    ws, p = _ws(nbytes)
    L.check(lib.bd_knn_sqradius(x.data_ptr(), _ld(x), N, D, k, out.data_ptr(), p, nbytes, L.stream()), "bd_knn_sqradius")
    return out


def run_ksmallest(L, a, b, k, self_col0=None):
    lib = L.load()
    (Na, D), Nb = a.shape, b.shape[0]
    out = torch.full((Na, k), float("nan"), device="cuda")
    nbytes = lib.bd_cross_ksmallest_workspace_bytes(Na, Nb, D, k)
    ws, p = _ws(nbytes)
    L.check(lib.bd_cross_ksmallest(a.data_ptr(), _ld(a), Na, b.data_ptr(), _ld(b), Nb, D, k, -Na if self_col0 is None else self_col0,
                                   out.data_ptr(), p, nbytes, L.stream()), "bd_cross_ksmallest")
    return out


def run_count_min(L, a, b, radius2):
    lib = L.load()
    (Na, D), Nb = a.shape, b.shape[0]
    count = torch.full((Na,), -1, device="cuda", dtype=torch.int32)
    mn = torch.full((Na,), float("nan"), device="cuda")
    nbytes = lib.bd_cross_count_min_workspace_bytes(Na, Nb, D)
    ws, p = _ws(nbytes)
    L.check(lib.bd_cross_count_min(a.data_ptr(), _ld(a), Na, b.data_ptr(), _ld(b), Nb, D, None if radius2 is None else radius2.data_ptr(),
                                   None if radius2 is None else count.data_ptr(), mn.data_ptr(), p, nbytes, L.stream()), "bd_cross_count_min")
    return count, mn


def run_poly(L, a, b, exclude_diag):
    lib = L.load()
    (Na, D), Nb = a.shape, b.shape[0]
    out = torch.full((Na,), float("nan"), device="cuda", dtype=torch.float64)
    nbytes = lib.bd_poly3_rowsum_workspace_bytes(Na, Nb, D)
    ws, p = _ws(nbytes)
    L.check(lib.bd_poly3_rowsum(a.data_ptr(), _ld(a), Na, b.data_ptr(), _ld(b), Nb, D, int(exclude_diag), out.data_ptr(), p, nbytes,
                                L.stream()), "bd_poly3_rowsum")
    return out


def legal_ks(N):
    return [k for k in KS if k <= N - 1]


def test_plan_branches(bd):
    """which branch each shape takes: (5, 1000, 2048) must split its column tiles, the many-strip shapes of the benchmark must too, and
    a shape with one column tile cannot"""
    ops = bd[1]
    p = ops.cross_plan(5, 1000, 2048)
    assert p["strips"] == 1 and p["col_tiles"] == 16 and p["csplit"] > 1 and p["csplit"] * p["tiles_per_split"] >= 16
    assert ops.cross_plan(200, 7, 100)["csplit"] == 1 and ops.cross_plan(64, 64, 32)["csplit"] == 1
    assert ops.cross_plan(130, 323, 70)["csplit"] > 1 and ops.cross_plan(130, 323, 70)["strips"] == 3
    for Na, Nb, D in SHAPES:
        p = ops.cross_plan(Na, Nb, D)
        assert 1 <= p["csplit"] <= p["csplit_cap"] and (p["csplit"] - 1) * p["tiles_per_split"] < p["col_tiles"]     # no empty split


# ---------------------------------------------------------------------------------------------------- exact on integers
@pytest.mark.parametrize("Na,Nb,D", SHAPES)
def test_exact_on_integers(bd, Na, Nb, D):
    L = bd[0]
    g = np.random.default_rng(Na * 7 + Nb * 3 + D)
    for pattern in ("random", "first", "last"):
        ai, bi = g.integers(-3, 4, (Na, D)), g.integers(-3, 4, (Nb, D))
        if pattern != "random":          # all zero but one column: a dropped first or tail chunk gives zeros
            col = 0 if pattern == "first" else D - 1
            for m in (ai, bi):
                keep = m[:, col].copy()
                m[:] = 0
                m[:, col] = keep
        d_ab, d_aa = R.sqdist(ai, bi), R.sqdist(ai, ai)                                       # int64
        assert max(int(d_ab.max()), int(d_aa.max())) < 2 ** 24
        radius_i = np.sort(d_ab, 0)[d_ab.shape[0] // 2]                                       # per column: a distance that occurs, so `<=` has ties
        want_count, want_min = R.count_min(d_ab, radius_i)
        dots = ai @ bi.T
        want_sum = ((dots.astype(np.float64) / D + 1.0) ** 3).sum(1)
        want_sum_x = want_sum - (np.diagonal(dots)[: min(Na, Nb)].astype(np.float64) / D + 1.0) ** 3 if Na <= Nb else None
        radius = torch.from_numpy(radius_i).float().cuda()
        for name, a in layouts(torch.from_numpy(ai).float().cuda()):
            b = dict(layouts(torch.from_numpy(bi).float().cuda()))[name]
            for k in legal_ks(Na):
                r = run_knn(L, a, k)
                assert np.array_equal(r.cpu().numpy().astype(np.float64), R.ksmallest(d_aa, k, 0)[:, k - 1]), (pattern, name, k)
                assert torch.equal(run_knn(L, a, k), r)
            count, mn = run_count_min(L, a, b, radius)
            assert np.array_equal(count.cpu().numpy(), want_count) and np.array_equal(mn.cpu().numpy().astype(np.int64), want_min), (pattern, name)
            none, mn2 = run_count_min(L, a, b, None)
            assert torch.equal(mn2, mn) and bool((none == -1).all())                        # null radii: no count is written
            again = run_count_min(L, a, b, radius)
            assert torch.equal(again[0], count) and torch.equal(again[1], mn)
            s = run_poly(L, a, b, False)
            err = float(np.abs(s.cpu().numpy() - want_sum).max() / max(np.abs(want_sum).max(), 1e-300))
            assert np.all(np.abs(s.cpu().numpy() - want_sum) <= 1e-12 * np.abs(want_sum)), (pattern, name, err)
            assert torch.equal(run_poly(L, a, b, False), s)
            if want_sum_x is not None:
                sx = run_poly(L, a, b, True)
                assert np.all(np.abs(sx.cpu().numpy() - want_sum_x) <= 1e-12 * np.abs(want_sum_x)), (pattern, name)
            print(f"MEASURE quality_exact {(Na, Nb, D)} {pattern} {name} max d2 {int(d_ab.max())} rowsum rel err {err:.2e}")


# ---------------------------------------------------------------------------------------------------- real data
def close_rows(N, D, seed):
    """uniform [0, 1] rows with a duplicate (0, 1), a pair 1e-4 apart (2, 3) and four rows within 1e-3 of a constant (4 .. 7)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, D, generator=g)
    if N >= 2:
        x[1] = x[0]
    if N >= 4:
        x[3] = x[2] + 1e-4
    if N >= 8:
        x[4:8] = 0.5 + 1e-3 * torch.rand(4, D, generator=g)
    return x


def real_sets(Na, Nb, D):
    """a: close_rows; b: uniform rows, of which row 0 repeats a row of a, row 1 lies 1e-4 from one and the last lies in a's cluster"""
    a = close_rows(Na, D, 100 + Na)
    b = torch.rand(Nb, D, generator=torch.Generator().manual_seed(200 + Nb))
    b[0] = a[0]
    b[1] = a[Na - 1] + 1e-4
    if Na >= 8:
        b[Nb - 1] = 0.5 + 1e-3 * torch.rand(D, generator=torch.Generator().manual_seed(5))
    return a, b


def within(got, ref, eps):
    """exactly 0 where the fp64 value is 0, otherwise within eps relative of it"""
    got = got.astype(np.float64)
    return bool(np.all(np.where(ref == 0, got == 0, np.abs(got - ref) <= eps * ref)))


@pytest.mark.parametrize("Na,Nb,D", SHAPES)
def test_real_data_bounds(bd, Na, Nb, D):
    L = bd[0]
    eps = (D + 2) * U24
    a32, b32 = real_sets(Na, Nb, D)
    a64, b64 = a32.double().numpy(), b32.double().numpy()
    d_ab, d_aa = R.sqdist(a64, b64), R.sqdist(a64, a64)
    radius32 = np.sort(d_ab, 0)[d_ab.shape[0] // 2].astype(np.float32)                        # the radii handed to the kernel, as it reads them
    radius32[0] = 0.0                                                                         # b[0] repeats a[0]: d2 = 0 <= 0 must count
    r64 = radius32.astype(np.float64)
    lo, hi = (d_ab <= r64[None] / (1 + eps)).sum(1), (d_ab <= r64[None] * (1 + eps)).sum(1)
    assert d_ab[0, 0] == 0 and lo[0] >= 1
    for name, a in layouts(a32.cuda()):
        b = dict(layouts(b32.cuda()))[name]
        for k in legal_ks(Na):
            assert within(run_knn(L, a, k).cpu().numpy(), R.ksmallest(d_aa, k, 0)[:, k - 1], eps), (name, k)
        count, mn = run_count_min(L, a, b, torch.from_numpy(radius32).cuda())
        assert within(mn.cpu().numpy(), d_ab.min(1), eps), name
        c = count.cpu().numpy()
        assert np.all((lo <= c) & (c <= hi)), (name, int(((c < lo) | (c > hi)).sum()))          # every row
        print(f"MEASURE quality_real {(Na, Nb, D)} {name} rows with lo < hi {int((lo < hi).sum())} "
              f"min_d2 rel err {float(np.max(np.abs(mn.cpu().numpy() - d_ab.min(1)) / np.maximum(d_ab.min(1), 1e-300))):.2e} of eps {eps:.2e}")
    if Na >= 2:
        assert float(run_knn(L, a32.cuda(), 1)[0]) == 0.0                                     # the duplicate: self is left out by index


# ---------------------------------------------------------------------------------------------------- invariance, bit-exact
@pytest.mark.parametrize("Na,Nb,D", [(130, 323, 70), (5, 1000, 2048), (65, 130, 33)])
def test_invariance(bd, Na, Nb, D):
    L, ops = bd
    a32, b32 = real_sets(Na, Nb, D)
    a, b = a32.cuda(), b32.cuda()
    k = min(5, Na - 1)
    radius = run_ksmallest(L, b, b, 3, 0)[:, 2].contiguous()                                  # radii of b
    full_self = run_ksmallest(L, a, a, k, 0)
    assert torch.equal(run_knn(L, a, k), full_self[:, k - 1])
    full_cross = run_ksmallest(L, a, b, k)
    count, mn = run_count_min(L, a, b, radius)
    assert torch.equal(full_cross[:, 0], mn)
    # rows alone and in a strip of 64
    for lo_, hi_ in [(0, 1), (Na - 1, Na), (min(63, Na - 1), min(64, Na - 1) + 1), (max(Na - 64, 0), Na)]:
        rows = a[lo_:hi_]
        assert torch.equal(run_ksmallest(L, rows, a, k, lo_), full_self[lo_:hi_]), (lo_, hi_)
        c1, m1 = run_count_min(L, rows, b, radius)
        assert torch.equal(c1, count[lo_:hi_]) and torch.equal(m1, mn[lo_:hi_]), (lo_, hi_)
    # the columns of b cut in two calls (other splits, other tile boundaries)
    cut = Nb // 3 + 1
    parts = [(b[:cut], radius[:cut].contiguous()), (b[cut:], radius[cut:].contiguous())]
    cs, ms = zip(*(run_count_min(L, a, bp, rp) for bp, rp in parts))
    assert torch.equal(cs[0] + cs[1], count) and torch.equal(torch.minimum(ms[0], ms[1]), mn)
    kk = min(k, cut, Nb - cut)
    merged = torch.cat([run_ksmallest(L, a, bp, kk) for bp, _ in parts], 1).sort(1).values[:, :kk]
    assert torch.equal(merged, run_ksmallest(L, a, b, kk))
    # the nearest neighbour in [a; b] is the nearer of the nearest in a (self left out) and the nearest in b: one pair value in either role
    z = torch.cat([a, b])
    near = run_knn(L, z, 1)
    assert torch.equal(near[:Na], torch.minimum(full_self[:, 0], mn))
    _, back = run_count_min(L, b, a, None)
    assert torch.equal(near[Na:], torch.minimum(run_ksmallest(L, b, b, 1, 0)[:, 0], back))
    in_b = mn <= full_self[:, 0]
    assert bool(in_b.any()) and torch.equal(near[:Na][in_b], mn[in_b])
    # the wrappers are the same calls
    assert torch.equal(ops.knn_sqradius(a, k), full_self[:, k - 1]) and torch.equal(ops.cross_ksmallest(a, b, k), full_cross)
    oc, om = ops.cross_count_min(a, b, radius)
    assert torch.equal(oc, count) and torch.equal(om, mn)
    s = run_poly(L, a, b, False)
    assert torch.equal(ops.poly3_rowsum(a, b), s) and torch.equal(run_poly(L, a, b, False), s)


# ---------------------------------------------------------------------------------------------------- metrics
def test_prdc_exact_on_integer_features(bd):
    from baddiffusion_amd import metrics
    g = np.random.default_rng(3)
    real, fake = g.integers(-3, 4, (130, 70)), g.integers(-3, 4, (200, 70))
    fake[:40] = real[:40]                                   # exact ties: distance == radius and distance == 0
    got = metrics.prdc(torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda(), k=5)
    want = R.prdc(real, fake, 5)
    assert got == want, (got, want)
    pr = metrics.precision_recall(torch.from_numpy(real).float().cuda(), torch.from_numpy(fake).float().cuda())
    want3 = R.prdc(real, fake, 3)
    assert pr == {"precision": want3["precision"], "recall": want3["recall"], "k": 3}
    same = metrics.prdc(torch.from_numpy(real).float().cuda(), torch.from_numpy(real).float().cuda(), k=5)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0
    print(f"MEASURE prdc integers {got}")


@pytest.fixture(scope="module")
def gaussians():
    g = torch.Generator().manual_seed(17)
    real = torch.randn(300, 2048, generator=g)
    fake = torch.cat([real[:100] + 0.3 * torch.randn(100, 2048, generator=g), 1.1 * torch.randn(200, 2048, generator=g) + 0.02])
    return real, fake


def test_prdc_on_gaussian_features(bd, gaussians):
    from baddiffusion_amd import metrics
    real, fake = gaussians
    eps = (2048 + 2) * U24
    got = metrics.prdc(real.cuda(), fake.cuda(), k=5)
    lo, hi = R.prdc(real.numpy(), fake.numpy(), 5, 1 / (1 + eps)), R.prdc(real.numpy(), fake.numpy(), 5, 1 + eps)
    print(f"MEASURE prdc gaussians got {got} lo {lo} hi {hi}")
    for name in ("precision", "recall", "density", "coverage"):
        assert lo[name] <= got[name] <= hi[name], (name, lo[name], got[name], hi[name])


def test_kid_against_fp64(bd, gaussians):
    from baddiffusion_amd import metrics
    real, fake = (0.5 * t.abs() for t in gaussians)          # non-negative, of the size of pool3 features
    res = metrics.kid(real.cuda(), fake.cuda(), subsets=4, subset_size=100, generator=torch.Generator().manual_seed(5))
    pairs = [(r.numpy(), f.numpy()) for r, f in metrics.kid_subset_indices(300, 300, 4, 100, torch.Generator().manual_seed(5))]
    mean64, std64, S, v64 = R.kid(real.numpy(), fake.numpy(), pairs)
    mean32, std32, _, v32 = R.kid(real.numpy(), fake.numpy(), pairs, np.float32)
    mean, std = res
    for what, got, want, d32 in [("mean", mean, mean64, abs(mean32 - mean64)), ("std", std, std64, abs(std32 - std64))] + \
            [(f"subset {i}", res.values[i], v64[i], abs(v32[i] - v64[i])) for i in range(4)]:
        bound = max(4e-6 * S, 4 * d32)
        print(f"MEASURE kid {what}: {got:.9e} fp64 {want:.9e} |err| {abs(got - want):.3e} bound {bound:.3e} used {abs(got - want) / bound:.4f} "
              f"(S {S:.4f}, d32 {d32:.3e})")
        assert abs(got - want) <= bound, what
    assert res.subsets == 4 and res.subset_size == 100 and res.warning is None and res.mean == mean and res.std == std
    again = metrics.kid(real.cuda(), fake.cuda(), subsets=4, subset_size=100, generator=torch.Generator().manual_seed(5))
    assert again == res and again.values == res.values                                        # run to run: equal bits
    capped = metrics.kid(real[:50].cuda(), fake.cuda(), subsets=2, subset_size=1000, generator=torch.Generator().manual_seed(5))
    assert capped.subset_size == 50 and "capped" in capped.warning
    itself = metrics.kid(real.cuda(), real.cuda(), subsets=1, subset_size=300, generator=torch.Generator().manual_seed(5))
    assert abs(itself.mean - R.kid(real.numpy(), real.numpy(), [(np.arange(300), np.arange(300))])[0]) <= 4e-6 * S


def test_feature_store(bd):
    from baddiffusion_amd import metrics
    x = torch.rand(37, 12, generator=torch.Generator().manual_seed(1)).cuda()
    st = metrics.FeatureStore(8)
    for s in range(0, 37, 5):
        st.update(x[s:s + 5])
    assert torch.equal(st.features(), x) and st.n == 37
    fa, fb = metrics.FeatureStore(), metrics.FeatureStore()
    batches = lambda t: (t[s:s + 10] for s in range(0, t.shape[0], 10))
    y = x * 0.5 + 0.1
    assert metrics.fid_from_features(batches(x), batches(y), stores=(fa, fb)) == metrics.fid_from_features(batches(x), batches(y))
    assert torch.equal(fa.features(), x) and torch.equal(fb.features(), y)


# ---------------------------------------------------------------------------------------------------- command lines
def test_quality_eval_pixels_end_to_end(bd, tmp_path, monkeypatch):
    from PIL import Image
    import quality_eval
    from baddiffusion_amd import metrics
    g = np.random.default_rng(9)
    sets = {}
    base = g.integers(0, 226, (8, 32, 32, 3))                # eight motifs shared by both sets; the fake set misses two and is a little brighter
    for name, shift, motifs in (("real", 0, 8), ("fake", 1, 6)):
        os.makedirs(tmp_path / name)
        imgs = np.clip(base[g.integers(0, motifs, 64)] + g.integers(-12, 13, (64, 32, 32, 3)) + shift, 0, 255).astype(np.uint8)
        for i, im in enumerate(imgs):
            Image.fromarray(im).save(tmp_path / name / f"{i}.png")
        sets[name] = torch.from_numpy(imgs).cuda().reshape(64, -1).float() / 255.0
    out = tmp_path / "out"
    res = quality_eval.main(["--real", str(tmp_path / "real"), "--fake", str(tmp_path / "fake"), "--features", "pixels", "--k", "5", "--kid",
                             "--kid_subsets", "3", "--kid_subset_size", "32", "--seed", "4", "--output_dir", str(out)])
    assert res == json.load(open(out / "quality.json"))
    want = metrics.prdc(sets["real"], sets["fake"], 5)
    kid = metrics.kid(sets["real"], sets["fake"], subsets=3, subset_size=32, generator=torch.Generator().manual_seed(4))
    assert res == {"features": "pixels", "n_real": 64, "n_fake": 64, "dim": 3072, "precision": want["precision"], "recall": want["recall"],
                   "density": want["density"], "coverage": want["coverage"], "PRDC_k": 5, "KID_mean": kid.mean, "KID_std": kid.std,
                   "KID_subsets": 3, "KID_subset_size": 32}
    ref = R.prdc(sets["real"].cpu().numpy(), sets["fake"].cpu().numpy(), 5)
    print(f"MEASURE quality_eval pixels {res} fp64 restatement {ref}")
    assert 0 < res["precision"] <= 1 and 0 < res["recall"] < 1 and 0 < res["coverage"] < 1 and res["density"] > 0     # not a degenerate case
    plain = quality_eval.main(["--real", str(tmp_path / "real"), "--fake", str(tmp_path / "fake"), "--features", "pixels", "--k", "3",
                               "--output_dir", str(out)])
    assert set(plain) == {"features", "n_real", "n_fake", "dim", "precision", "recall", "density", "coverage", "PRDC_k"} and plain["PRDC_k"] == 3
    monkeypatch.delenv("BD_FID_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError, match="BD_FID_WEIGHTS"):
        quality_eval.main(["--real", str(tmp_path / "real"), "--fake", str(tmp_path / "fake"), "--output_dir", str(out)])


def test_measure_with_quality_flags_and_no_weights(bd, tmp_path, monkeypatch):
    """measure() with --measure_prdc_k / --measure_kid and no Inception weights: null keys and the reason; without the flags the keys of
    score.json are what they were"""
    import baddiffusion as cli
    from baddiffusion_amd.dataset import DatasetLoader
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDIMScheduler
    from baddiffusion_amd.unet import unet_from_config
    monkeypatch.delenv("BD_FID_WEIGHTS", raising=False)
    cfg_net = dataclasses.replace(C.SMALL_CFGS["small"], sample_size=32)
    model = unet_from_config(cfg_net).cuda()
    model.load_state_dict(U.gen_params(cfg_net, 7))
    dsl = DatasetLoader(root=None, name=DatasetLoader.CIFAR10, batch_size=8, seed=0, device=torch.device("cuda"), num_images=8)
    dsl.set_poison(trigger_type="BOX_14", target_type="CORNER", clean_rate=1.0, poison_rate=0.25).prepare_dataset(mode="FIXED")

    class Pipe(DDIMPipeline):
        def __call__(self, **kw):
            return super().__call__(num_inference_steps=2, **kw)

    def run(out, **opts):
        config = cli.TrainingConfig()
        config.output_dir = str(out); config.seed = 0; config.clip = False; config.sample_ep = None
        config.measure_sample_n = 8; config.eval_max_batch = 8
        for k, v in opts.items():
            setattr(config, k, v)
        os.makedirs(config.output_dir, exist_ok=True)
        return cli.measure(config, dsl, "measure", Pipe(model, DDIMScheduler(num_train_timesteps=1000, clip_sample=False)), rank=0, world=1)

    old_keys = {"FID", "FID_reason", "MSE", "SSIM", "inference_chunk"}
    plain = run(tmp_path / "plain")
    assert set(plain) == {k + "_noclip" for k in old_keys}
    score = run(tmp_path / "flags", measure_prdc_k=3, measure_kid=True, kid_subsets=7)
    new = {"precision", "recall", "density", "coverage", "PRDC_k", "KID_mean", "KID_std", "KID_subsets", "KID_subset_size", "quality_reason"}
    assert set(score) == {k + "_noclip" for k in old_keys | new}
    assert score == json.load(open(tmp_path / "flags" / "score.json"))
    for k in ("precision", "recall", "density", "coverage", "KID_mean", "KID_std"):
        assert score[k + "_noclip"] is None
    assert score["PRDC_k_noclip"] == 3 and score["KID_subsets_noclip"] == 7 and score["KID_subset_size_noclip"] == 1000
    assert "weights are absent" in score["quality_reason_noclip"]
    assert score["MSE_noclip"] == plain["MSE_noclip"]
