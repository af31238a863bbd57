"""CPU: the references of tests/_step_exact.py are tied to the golden vectors and to torch, its exact data is rounding-free, and its sizes
follow the constants in the sources.

1. The fp32 statements of the DDPM / DDIM steps reproduce every ddpm_* / ddim_* vector of tests/golden/sched.npz bit for bit, the q_sample
   statement the vectors of qsample.npz; the Adam statement agrees with torch.optim.Adam + clip_grad_norm_ at the tolerance of
   test_adam_clip_vs_torch.
2. Each fp32 statement stays within twice its measured distance (F64_DISTANCE below) of an fp64 statement of the same mathematics
   on the GPU cases' own inputs: a transcription that is wrong the way a kernel is wrong does not pass here.
3. Every "equal to fp64" case is rounding-free: the fp64 reference is representable in fp32 and equals an fp32 evaluation in another order.
4. TPB and the grid caps are read out of csrc/elementwise.hip, igemm.hip and conv_ps.hip; the second-trip sizes must be derived from them."""
import os
import re

import numpy as np
import pytest
import torch

from tests import _small_exact as S
from tests import _step_exact as X
from tests.test_small_exact_host import grid_caps, same, source

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
f32 = np.float32

# measured max |fp32 statement - fp64 statement| over the GPU cases' inputs (absolute), asserted at twice the value.  The large ones have a
# reason: rho_t cancels (1 - sqrt(alpha_t)); at t = 999 x0 = (x - sb e) / 0.0064 is of the order of 400; where v = 0 and g = 0 Adam divides
# by eps alone and p moves by lr m / eps, of the order of 200.
F64_DISTANCE = {"qsample": 1.84e-6, "ddpm": 1.74e-4, "ddim": 5.31e-5, "lincomb": 1.29e-6, "adam_p": 1.69e-4, "adam_m": 1.12e-9, "adam_v": 7.8e-12}


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


# ------------------------------------------------------------------------------------------------ 4. constants and derived sizes
def test_constants_and_derived_sizes():
    src = source("elementwise.hip")
    tpb = int(re.search(r"constexpr int TPB = (\d+);", src).group(1))
    assert tpb == X.TPB == S.TPB
    caps = grid_caps(src)
    assert caps["ddpm_step_kernel"] == caps["ddim_step_kernel"] == caps["lincomb_kernel"] == {str(X.STEP_CAP)}
    assert caps["adam_clip_kernel"] == {str(X.ADAM_CAP)}
    assert re.search(r"lincomb_kernel, dim3\(nblocks\(cdiv\(n, 4\), TPB, 4096\)\)", src)           # the cap counts float4s
    assert X.STEP_SECOND_TRIP == X.STEP_CAP * tpb + 77 and X.STEP_SECOND_TRIP in X.STEP_N and {1, 255, 257} <= set(X.STEP_N)
    assert X.LINCOMB_SECOND_TRIP == 4 * (X.STEP_CAP * tpb) + 4 * 77 + 3 and X.LINCOMB_SECOND_TRIP in X.LINCOMB_N
    assert {n & 3 for n in X.LINCOMB_N} == {0, 1, 2, 3} and {1, 2, 3, 4, 5, 7, 1023} <= set(X.LINCOMB_N)
    assert int(re.search(r"#define BD_LINCOMB_MAX (\d+)", open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "bd_hip.h")).read()).group(1)) \
        == X.LINCOMB_MAX
    cases = X.lincomb_cases()
    assert {(k, n) for n in X.LINCOMB_N for k in (1, X.LINCOMB_MAX)} <= set(cases) and {(k, 1023) for k in range(1, 7)} <= set(cases)
    assert X.ADAM_SECOND_TRIP == X.ADAM_CAP * tpb + 77 == 2097229 and X.ADAM_SECOND_TRIP in X.ADAM_N and {1, 5, 1023} <= set(X.ADAM_N)
    # the split launchers: 256 threads, 8 values each, blocks capped
    ig, ps = source("igemm.hip"), source("conv_ps.hip")
    m = re.search(r"bd_split_bf16\(.*?if \(nb > (\d+)\) nb = \1;\s*hipLaunchKernelGGL\(bd::split_bf16_kernel, dim3\(\(unsigned\)nb\), dim3\((\d+)\)", ig, re.S)
    assert (int(m.group(1)), int(m.group(2))) == (X.SPLIT_BF16_CAP, X.SPLIT_THREADS)
    for fn, kern in (("bd_split_rows", "split_rows_kernel"), ("bd_split_rows_ups2", "split_rows_ups2_kernel")):
        m = re.search(fn + r"\(const float.*?if \(nb > (\d+)\) nb = \1;\s*hipLaunchKernelGGL\(bd::" + kern + r", dim3\(\(unsigned\)nb\), dim3\((\d+)\)", ps, re.S)
        assert (int(m.group(1)), int(m.group(2))) == (X.SPLIT_ROWS_CAP, X.SPLIT_THREADS), fn
    assert X.SPLIT_BF16_SECOND_TRIP == 8 * (X.SPLIT_BF16_CAP * 256) + 96 and X.SPLIT_BF16_SECOND_TRIP in X.SPLIT_BF16_N
    assert {32, 96} <= set(X.SPLIT_BF16_N) and all(n % 32 == 0 for n in X.SPLIT_BF16_N)
    assert X.SPLIT_ROWS_SECOND_TRIP == X.SPLIT_ROWS_CAP * 256 * 8 // 32 + 3
    assert set(X.SPLIT_ROWS_CASES) == {(1, 32, 32, 32), (5, 64, 68, 64), (7, 96, 100, 128), (X.SPLIT_ROWS_SECOND_TRIP, 32, 32, 32)}
    assert set(X.SPLIT_UPS2_SHAPES) == {(1, 1, 1, 32), (2, 3, 5, 64), (1, 2, 3, 96)} and X.SPLIT_UPS2_LD_EXTRA == (0, 32)
    assert set(X.SPLIT_WT_SHAPES) == {(32, 32), (64, 32), (32, 96), (96, 64)}
    # q_sample: one thread per pixel, TPB pixels per block
    px = [B * H * W for B, C, H, W in X.QS_SHAPES]
    assert px[0] == 1 and px[1] < tpb and tpb < px[2] < 2 * tpb and px[2] % tpb and px[3] == 3 * tpb
    assert all(H != W for _, _, H, W in X.QS_SHAPES[1:]) and {C for _, C, _, _ in X.QS_SHAPES} >= {1, 2, 3, 4}
    assert X.QS_N_RESIDENT > max(B for B, *_ in X.QS_SHAPES) and X.QS_ROW_INDEX[0] == X.QS_N_RESIDENT - 1 and X.QS_ROW_INDEX[1] == X.QS_ROW_INDEX[2]
    # ANP: a row of one element, a ragged row over more than one trip of the block, a row shorter than a wave; no bias on the long one
    lens = {ln for _, _, _, ln, _ in X.ANP_ITEMS}
    assert lens == {1, tpb + 3, 27} and [b for _, b, _, _, _ in X.ANP_ITEMS if b < 0] == [-1]
    assert sum(c for _, _, c, _, _ in X.ANP_ITEMS) == X.ANP_TOTAL_ROWS == 9 and X.ANP_ITEMS[2][4] == 0 and X.ANP_ITEMS[0][4] > 0


def test_qsample_case_table():
    cases = X.qs_cases()
    for shape in X.QS_SHAPES:
        vs = [v for s, v in cases if s == shape]
        assert {v.u8 for v in vs} == {True, False} and {v.ld for v in vs} == {True, False} and {v.rows for v in vs} == {True, False}
        assert {v.flip for v in vs} >= {"mixed", "zeros", "ones", None} and {v.outs for v in vs} == {True, False}
        for v in vs:
            d = X.qs_data(shape, v)
            B, C, H, W = shape
            assert d.timesteps.size == B and (B == 1 or len(set(d.timesteps.tolist())) == B)
            if B >= 2:
                assert {0, 999} <= set(d.timesteps.tolist())
            if v.poison in ("mixed", "mixed0") and B >= 2:
                assert set(d.is_poison.tolist()) == {0, 1}
            if v.flip == "mixed" and B >= 2:
                assert set(d.flip.tolist()) == {0, 1}
            if v.rows:
                assert int(d.row_index.max()) == X.QS_N_RESIDENT - 1 and (B < 3 or len(set(d.row_index.tolist())) < B)
            g = d.trigger.reshape(-1)
            assert all(bool((g == p).any()) for p in d.planted[:min(3, g.size)])
            ref = X.poison_qsample_stmt(*X.tables(), d)
            assert ref.mask.dtype == np.int64 and set(np.unique(ref.mask).tolist()) <= {0, 1}
            if g.size >= 3:      # at vmin and below the mask is 1, one fp32 step above it is 0
                assert ref.mask.reshape(-1)[:3].tolist() == [1, 0, 1]
    one = [(s, v) for s, v in cases if s == (1, 1, 1, 1)]
    assert {int(X.qs_data(s, v).timesteps[0]) for s, v in one} >= {0, 999} and {int(X.qs_data(s, v).is_poison[0]) for s, v in one} == {0, 1}
    extra = [v.poison for s, v in cases if s == X.QS_EXTRA_AT]
    assert "none" in extra and "all" in extra


# ------------------------------------------------------------------------------------------------ 1. the statements and the reference
def test_step_statements_reproduce_golden():
    from tests.golden import cases as C
    g = golden("sched")
    _, ac = X.tables()
    x, eps, z = (t.numpy().reshape(-1) for t in C.sched_inputs())
    seen = set()

    def check(key, got):
        assert np.array_equal(got.reshape(g[key].shape), g[key]) and got.dtype == f32, (key, float(np.abs(got.reshape(g[key].shape) - g[key]).max()))
        seen.add(key)

    for vt in (0, 1):
        name = ("fixed_small", "fixed_large")[vt]
        for clip in (1, 0):
            for t in C.DDPM_TS:
                prev, x0 = X.ddpm_stmt(ac, X._dp(t, t - 1, vt, 1.0 if clip else None), x, eps, z)
                check(f"ddpm_{name}_{clip}_{t}_prev", prev)
                check(f"ddpm_{name}_{clip}_{t}_x0", x0)
    check("ddpm_clipdef_500_prev", X.ddpm_stmt(ac, X._dp(500, 499, 0, None, cdef=0.5), x, eps, z)[0])
    for clip in (1, 0):
        for t in C.DDIM_TS:
            check(f"ddim_{clip}_{t}_prev", X.ddim_stmt(ac, X._di(t, t - 20, 1.0, 0.0, 1.0 if clip else None), x, eps, z)[0])
        check(f"ddim_{clip}_500_eta_prev", X.ddim_stmt(ac, X._di(500, 480, 1.0, 0.5, 1.0 if clip else None), x, eps, z)[0])
    assert seen == {k for k in g.files if k.startswith(("ddpm_", "ddim_")) and k.endswith(("_prev", "_x0"))} and len(seen) == 41


def test_qsample_statement_reproduces_golden():
    from tests.golden import cases as C
    g = golden("qsample")
    a, ac = X.tables()
    x0, R, eps, t = C.qsample_inputs()
    xn, tg = X.qsample_stmt(a, ac, x0.numpy(), R.numpy(), eps.numpy(), t.numpy())
    dx = float(np.abs(xn.transpose(0, 3, 1, 2) - g["x_noisy"]).max())
    dt = float(np.abs(tg.transpose(0, 3, 1, 2) - g["target"]).max())
    print(f"q_sample statement against the golden vectors: max |d| x_noisy {dx:.3g}, target {dt:.3g}")
    assert np.array_equal(xn.transpose(0, 3, 1, 2), g["x_noisy"]) and np.array_equal(tg.transpose(0, 3, 1, 2), g["target"])


def test_adam_statement_against_torch():
    """the statement at n = 1023 on a random gradient with the clip active, against torch on the CPU: 1e-6 / 1e-7, as test_adam_clip_vs_torch"""
    for step in X.ADAM_STEPS:
        p, g, m, v, ss = X.adam_data(1023, "random", seed=step)
        pt, norm_t = X.adam_torch(p, g, m, v, 0.1, step)
        ps, _, _, norm = X.adam_stmt(p, g, m, v, ss, 0.1, step)
        assert float(norm) > 0.1                      # the clip is active
        np.testing.assert_allclose(float(norm), norm_t, rtol=1e-6)
        np.testing.assert_allclose(ps, pt.numpy(), rtol=1e-6, atol=1e-7)


def test_adam_perfect_squares():
    assert set(X.ADAM_ACTIVE) == set(X.ADAM_N)
    assert X.ADAM_ACTIVE[X.ADAM_SECOND_TRIP] == ((1, 1398204), (2, 699025)) and 1398204 + 4 * 699025 == 2048 ** 2
    for n in X.ADAM_N:
        k, s = X.adam_active_k(n)
        assert k * k == s and sum(c for _, c in X.ADAM_ACTIVE[n]) == n
        p, g, m, v, ss = X.adam_data(n, "active")
        # the sum of squares is K^2 2^-12 exactly, in any order, so the norm is K / 64 however the root is rounded
        assert ss == s * 2.0 ** -12 == float((g.double().flip(0) ** 2).sum())
        norm = X.adam_stmt(p, g, m, v, ss, X.ADAM_MAX_NORM_ACTIVE, 1)[3]
        assert float(norm) == k / 64 and float(norm) + 1e-6 > X.ADAM_MAX_NORM_ACTIVE
        assert bool((g != 0).all()) and set(torch.sign(g).tolist()) == ({-1.0, 1.0} if n > 1 else set(torch.sign(g).tolist()))
        for kind in ("random", "zero"):
            p, g, m, v, ss = X.adam_data(n, kind)
            norm = X.adam_stmt(p, g, m, v, ss, X.ADAM_MAX_NORM_INACTIVE, 1)[3]
            assert norm + f32(1e-6) <= f32(X.ADAM_MAX_NORM_INACTIVE) and bool((v >= 0).all())       # coef is exactly 1
            if kind == "random" and n > 1:
                assert bool(((v == 0) & (g == 0)).any())


# ------------------------------------------------------------------------------------------------ 2. fp32 statement against fp64 statement
def dist(a32, a64):
    return float(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64)).max())


def test_statements_against_fp64():
    a, ac = X.tables()
    worst = dict.fromkeys(F64_DISTANCE, 0.0)
    for shape, v in X.qs_cases():
        d = X.qs_data(shape, v)
        r32, r64 = X.poison_qsample_stmt(a, ac, d), X.poison_qsample_stmt(a, ac, d, np.float64)
        assert np.array_equal(r32.mask, r64.mask)
        worst["qsample"] = max([worst["qsample"]] + [dist(getattr(r32, k), getattr(r64, k)) for k in ("x_noisy", "target", "R", "x0", "image")])
    for name, cases, coef, stmt in (("ddpm", X.ddpm_cases(), X.ddpm_coef, X.ddpm_stmt), ("ddim", X.ddim_cases(), X.ddim_coef, X.ddim_stmt)):
        for i, c in enumerate(cases):
            sb, sa = coef(ac, c)[:2]
            x, e, z, _ = X.step_data(257, sb, sa, c.clip, i)
            # away from the clip boundaries, where a half-ulp of x0 decides between the clipped and the unclipped branch
            (p32, o32), (p64, o64) = stmt(ac, c, x, e, z), stmt(ac, c, x, e, z, np.float64)
            worst[name] = max(worst[name], dist(p32, p64), dist(o32, o64))
    for k, n in X.lincomb_cases():
        if n <= 1023:
            terms, coeffs = X.lincomb_terms(k, n, exact=False)
            worst["lincomb"] = max(worst["lincomb"], dist(X.lincomb_stmt(terms, coeffs, None).numpy(), X.lincomb_f64(terms, coeffs, None).numpy()))
    for n in X.ADAM_N[:3]:
        for step in X.ADAM_STEPS:
            for kind, mx in (("random", X.ADAM_MAX_NORM_INACTIVE), ("active", X.ADAM_MAX_NORM_ACTIVE)):
                args = X.adam_data(n, kind)
                r32, r64 = X.adam_stmt(*args, mx, step), X.adam_f64(*args, mx, step)
                for key, i in (("adam_p", 0), ("adam_m", 1), ("adam_v", 2)):
                    worst[key] = max(worst[key], dist(r32[i], r64[i]))
    print("fp32 statement against fp64 statement, max |d|: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 2 * F64_DISTANCE[k], (k, v)


# ------------------------------------------------------------------------------------------------ 3. the exact data is rounding-free
def test_qsample_routing_exact():
    x0, R, eps = X.qs_routing_data()
    t = np.array([0, 2, 1], dtype=np.int64)
    for r in X.QS_ROUTING:
        al, ac = np.full(3, r.al, dtype=f32), np.full(3, r.ac, dtype=f32)
        xn64, tg64 = X.qsample_stmt(al, ac, x0, R, eps, t, np.float64)
        xn, tg = X.qsample_stmt(al, ac, x0, R, eps, t)
        nhwc = lambda v: v.transpose(0, 2, 3, 1)
        want = (nhwc(x0), nhwc(eps)) if r.ac == 1.0 else (nhwc(eps + R), nhwc(R + eps))
        assert np.array_equal(xn64, want[0]) and np.array_equal(tg64, want[1]) and np.array_equal(xn, want[0]) and np.array_equal(tg, want[1]), r.why
    assert not np.array_equal(x0, R) and not np.array_equal(x0, eps) and not np.array_equal(R, eps)


def test_step_planted_values():
    _, ac = X.tables()
    for cases, coef, stmt in ((X.ddpm_cases(), X.ddpm_coef, X.ddpm_stmt), (X.ddim_cases(), X.ddim_coef, X.ddim_stmt)):
        assert any(c.clip == 1.0 for c in cases) and any(c.clip == 0.5 for c in cases) and any(c.clip is None for c in cases)
        for i, c in enumerate(cases):
            if c.clip is None:
                continue
            sb, sa = coef(ac, c)[:2]
            x, e, z, pairs = X.step_data(257, sb, sa, c.clip, i)
            r = f32(c.clip)
            unclipped = (x - sb * e) / sa
            got = set(unclipped[:len(pairs)].tolist())
            assert {float(r), float(-r)} <= got                                      # exactly on the boundary
            assert any(abs(u) < r for u in got) and any(abs(u) > r for u in got)      # one fp32 step inside and outside
            assert all(abs(abs(u) - r) <= 2 * np.spacing(r) for u in got)
            assert np.array_equal(unclipped[-len(pairs):], unclipped[:len(pairs)])
            x0 = stmt(ac, c, x, e, z)[1]
            assert float(np.abs(x0).max()) == float(r)
    d = X.ddpm_cases()
    assert {(c.t, c.prev_t) for c in d} >= {(999, 998), (500, 499), (1, 0), (0, -1), (500, 480), (500, -1)} and {c.vt for c in d} == {0, 1}
    assert any(c.cdef == 0.5 for c in d) and any(not c.x0 for c in d) and any(c.t == 0 and not c.noise for c in d)
    assert all(c.noise or c.t == 0 for c in d)
    # t > 0 with prev_t < 0: the posterior variance is 0 and the floor decides
    sd = X.ddpm_coef(ac, X._dp(500, -1, 0))[4]
    assert sd == np.sqrt(f32(1e-20)) and sd > 0
    m = X.ddim_cases()
    assert {(c.t, c.prev_t) for c in m} == {(980, 960), (500, 480), (0, -20)} and {c.eta for c in m} == {0.0, 0.5}
    assert {c.final for c in m if c.prev_t < 0} == {1.0, float(ac[0])}
    assert all(max(X.STEP_BIG_DDPM) < len(d) and max(X.STEP_BIG_DDIM) < len(m) for _ in (0,))


@pytest.mark.parametrize("k,n", [c for c in X.lincomb_cases() if c[1] <= 1023])
def test_lincomb_exact(k, n):
    terms, coeffs = X.lincomb_terms(k, n, exact=True)
    assert set(abs(c) for c in coeffs) <= {1.0, 0.5, 0.25, 2.0}
    for clip in (None, X.LINCOMB_CLIP):
        ref = X.lincomb_f64(terms, coeffs, clip)
        other = X.lincomb_stmt(terms[::-1], coeffs[::-1], clip)          # fp32, the terms in the other order
        assert same(ref, other) and torch.equal(X.lincomb_stmt(terms, coeffs, clip), other)
    if n >= 1023:
        assert float(X.lincomb_f64(terms, coeffs, None).abs().max()) > X.LINCOMB_CLIP            # the clip has something to do


def test_anp_exact():
    params, geff, pw, pb = X.anp_data()
    rows = X.anp_rows()
    assert len(rows) == X.ANP_TOTAL_ROWS and sorted(p for *_, p in rows) == list(range(X.ANP_TOTAL_ROWS))
    # the rows, their biases and the gaps do not overlap, and gaps lie before, between and after the items
    used = torch.zeros(X.ANP_NPARAMS, dtype=torch.int32)
    for woff, boff, ln, _ in rows:
        used[woff: woff + ln] += 1
        if boff >= 0:
            used[boff] += 1
    assert int(used.max()) == 1 and int(used[0]) == 0 and int(used[-1]) == 0
    firsts = [it[0] for it in X.ANP_ITEMS]
    assert all(bool((used[a + 1: b] == 0).any()) for a, b in zip(firsts, firsts[1:]))
    eff = X.anp_apply_ref(params, pw, pb)
    assert S.exact_in_fp32(eff) and torch.equal(eff[used == 0], params.double()[used == 0])
    gw, gb, rn = X.anp_grad_ref(params, geff, pw)
    gw2, gb2, rn2 = X.anp_grad_ref(params, geff, pw, flip=True)
    assert S.exact_in_fp32(gw) and torch.equal(gw, gw2) and torch.equal(gb, gb2) and torch.equal(rn, rn2)
    # a permuted fp32 sum gives the same integers
    for woff, boff, ln, p in rows:
        perm = torch.randperm(ln, generator=S.gen(ln))
        t = (geff[woff: woff + ln][perm] * params[woff: woff + ln][perm]).sum() + (geff[boff] * params[boff] if boff >= 0 else 0.0)
        q = (geff[woff: woff + ln][perm] ** 2).sum()
        assert float(t) == float(gw[p]) and float(q) == float((geff[woff: woff + ln].double() ** 2).sum()) < 2 ** 24
    assert set(pw.tolist()) <= {0.0, 0.5, -0.5, 1.0, 2.0} and bool((rn > 0).any())


def test_split_reference():
    x = torch.from_numpy(X.from_bits(X.SPLIT_PLANTED_BITS).copy())
    hi, lo = X.split_hi_lo(x)
    for b, h, l in zip(X.SPLIT_PLANTED_BITS, hi.tolist(), lo.tolist()):
        if b in X.SPLIT_PLANTED_HI:
            assert h & 0xFFFF == X.SPLIT_PLANTED_HI[b], hex(b)
    assert hi.tolist()[3:7] == [0, -0x8000, 0x3F80, 0xBF80 - 0x10000] and lo.tolist()[5:7] == [0, 0]
    # hi + lo carries 16 bits of the mantissa: |x - hi - lo| <= 2^-16 |x|
    d = X.split_data(4096, 3)
    h, l = X.unsplit(X.split_planes(d.view(64, 64)), 64)
    assert bool(((d.view(64, 64).double() - h.double() - l.double()).abs() <= d.view(64, 64).double().abs() * 2.0 ** -16).all())
    assert all(bool((d == v).any()) for v in x.tolist())
    # the layout: element e of a row at (e / 32) * 64 + e % 32, lo 32 further on, row stride 2 * ld_dst, the rest sentinel
    y = torch.arange(1, 2 * 96 + 1, dtype=torch.float32).view(2, 96)
    pl = X.split_planes(y, 128)
    assert pl.shape == (2, 256)
    for r in range(2):
        for e in (0, 31, 32, 95):
            want = int(torch.tensor(float(y[r, e])).to(torch.bfloat16).view(torch.int16))
            assert int(pl[r, (e // 32) * 64 + e % 32]) == want
    assert bool((pl[:, 192:] == torch.tensor(X.U16_SENTINEL, dtype=torch.int32).to(torch.int16)).all())
    nf = torch.from_numpy(X.from_bits(X.SPLIT_NONFINITE_BITS).copy())
    hi, lo = X.split_hi_lo(nf)
    assert hi.tolist()[3] & 0xFFFF == 0x7F80 and lo.tolist()[3] & 0xFFFF == 0xFF80        # hi rounds to inf, lo is -inf
    dn = torch.from_numpy(X.from_bits(X.SPLIT_DENORMAL_BITS).copy())
    assert bool((dn.abs() < 2.0 ** -126).all()) and bool((dn != 0).all())
    # bd_split_wt: named data is exact in bf16, and the reference is the planes of the transpose
    for Cin, Cout in X.SPLIT_WT_SHAPES:
        w = X.split_wt_data(Cin, Cout, True)
        assert float(w.max()) <= 256 and float(w.min()) >= 1 and torch.equal(w.to(torch.bfloat16).float(), w)
        ref = X.split_wt_ref(w)
        assert ref.shape == (Cin, 2 * 9 * Cout)
        h, l = X.unsplit(ref, 9 * Cout)
        assert torch.equal(h.view(Cin, 9, Cout), w.permute(2, 1, 0)) and not bool(l.any())
    u = X.ups2(torch.arange(2 * 3 * 5 * 1, dtype=torch.float32).view(2, 3, 5, 1))
    assert u.shape == (2, 6, 10, 1) and torch.equal(u[:, ::2, ::2], u[:, 1::2, 1::2]) and torch.equal(u[:, ::2, 1::2], u[:, 1::2, ::2])


# ------------------------------------------------------------------------------------------------ the dense vec4 driver and its buffer check
def test_vec4_sizes_and_statements():
    """the sizes of test_vec4_driver follow the launchers' grid, and the fp32 statements of the DPM / UniPC / sigma steps stay within a few
    roundings of the same formulas in fp64: every intermediate is below 32 in magnitude (clamps at 1.5 and 2, |inputs| <= 6, coefficients
    below 1 but sigma_in), at most 12 rounded operations lie behind an output, so 12 * 32 * 2^-24 = 2.3e-5 bounds the distance"""
    src = source("elementwise.hip")
    assert len(re.findall(r"nblocks\(cdiv\(d(?:->|\.)n, 4\), TPB, 4096\)", src)) == 3            # dpm, unipc, sigma
    assert len(re.findall(r"nblocks\(cdiv\(n, 4\), TPB, 4096\)", src)) == 2                      # lincomb, scale_input
    assert X.VEC4_SECOND_TRIP == 4 * X.TPB * X.STEP_CAP + 5 and X.VEC4_N[-1] == X.VEC4_SECOND_TRIP and {1, 3, 4, 7} <= set(X.VEC4_N)
    e, x, a, b, c, d = X.vec4_inputs(1023)
    assert max(float(np.abs(v).max()) for v in (e, x, a, b, c, d)) <= 6.0
    wide = [v.astype(np.float64) for v in (e, x, a, b, c, d)]
    f64 = lambda k: {n: np.float64(f32(v)) for n, v in k.items()}
    cl = lambda v, r: np.minimum(np.maximum(v, -r), r)
    k = f64(X.VEC4_DPM)
    m0 = cl((wide[1] - k["sigma_s"] * wide[0]) / k["alpha_s"], k["x0_range"])
    prev = cl(k["cx"] * wide[1] + k["c0"] * m0 + k["c1"] * wide[2] + k["c2"] * wide[3], k["clip_range"])
    got = X.dpm_stmt(X.VEC4_DPM, e, x, a, b)
    worst = max(dist(got[0], m0), dist(got[1], prev))
    k = f64(X.VEC4_UNIPC)
    xc = k["kl"] * wide[2] + k["k0"] * m0 + k["k1"] * wide[3] + k["k2"] * wide[4] + k["k3"] * wide[5]
    prev = cl(k["px"] * xc + k["p0"] * m0 + k["p1"] * wide[3] + k["p2"] * wide[4], k["clip_range"])
    got = X.unipc_stmt(X.VEC4_UNIPC, e, x, a, b, c, d)
    worst = max(worst, dist(got[0], m0), dist(got[1], xc), dist(got[2], prev))
    k = f64(X.VEC4_SIGMA)
    x0 = wide[1] - k["sigma_in"] * wide[0]
    sc = cl((wide[2] + k["c0"] * wide[0] + k["c1"] * wide[3] + k["c2"] * wide[4] + k["c3"] * wide[5]) / k["in_div"], k["clip_range"])
    got = X.sigma_stmt(X.VEC4_SIGMA, e, x, a, b, c, d)
    worst = max(worst, dist(got[0], x0), dist(got[1], wide[0]), dist(got[2], sc * k["in_div"]), dist(got[3], sc))
    assert all(g.dtype == f32 for g in got) and X.scale_input_stmt(x, *X.VEC4_SCALE).dtype == f32
    print(f"fp32 statements of the dpm / unipc / sigma steps against fp64, max |d|: {worst:.3g}")
    assert worst <= 12 * 32 * 2.0 ** -24


def test_step_buffer_check_under_host_sanitizers(tmp_path):
    """csrc/step_check.h (the alignment / overlap check of bd_lincomb, bd_dpm_step, bd_unipc_step, bd_sigma_step and bd_scale_input) with its
    own main, built with -fsanitize=address,undefined and run as a stand-alone program, as tests/test_ema_host.py runs ema_check.h"""
    import subprocess
    csrc = os.path.join(os.path.dirname(GOLDEN), "..", "baddiffusion_amd", "csrc")
    exe = str(tmp_path / "step_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", csrc, os.path.join(csrc, "step_check_main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "step_check: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
