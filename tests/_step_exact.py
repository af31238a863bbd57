"""Case tables, data builders and references of the exact-value tests of the kernels a training step and a sampling loop start and end with:
bd_poison_qsample / bd_qsample, bd_ddpm_step / bd_ddim_step / bd_lincomb, bd_adam_clip(_dev), bd_anp_apply / bd_anp_grad
(csrc/elementwise.hip) and the producers of split planes bd_split_bf16 (csrc/igemm.hip), bd_split_rows(_ups2), bd_split_wt
(csrc/conv_ps.hip).  tests/test_step_exact_host.py ties the references to the golden vectors and the sizes to the constants in the sources;
tests/test_step_exact.py runs the kernels.  Nothing here touches a device or imports the product's kernels.

elementwise.hip is compiled without FMA contraction and fp32 sqrt and division are correctly rounded, so the formula kernels are held to
EQUAL BITS against a numpy-float32 statement of the same formulas, one rounding per operation in the order of the kernels' comments (the
`*_stmt` functions).  An fp64 statement of the same mathematics (`*_f64`) cross-checks each transcription on the CPU.  Where the data is
small integers with power-of-two scales the fp64 result is exact and the assertion is torch.equal in any order.
DESIGN.md "Step, optimiser, ANP and split kernels: test cases" carries the same tables; whoever retunes a grid cap moves the cases with it."""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from tests._small_exact import gen, ints

f32 = np.float32
ONE = f32(1)

# ---- constants restated from the sources (test_step_exact_host.py parses them out of the text and compares)
TPB = 256                    # elementwise.hip: threads per block
STEP_CAP = 4096              # nblocks(.., TPB, 4096) of ddpm_step_kernel, ddim_step_kernel and lincomb_kernel
ADAM_CAP = 8192              # nblocks(n, TPB, 8192) of adam_clip_kernel
SPLIT_BF16_CAP = 4096        # igemm.hip: `if (nb > 4096) nb = 4096` of bd_split_bf16 (256 threads, 8 values each)
SPLIT_ROWS_CAP = 8192        # conv_ps.hip: `if (nb > 8192) nb = 8192` of bd_split_rows / bd_split_rows_ups2
SPLIT_THREADS, SPLIT_PER_THREAD = 256, 8

# ---- second trips: one full pass of the capped grid plus a ragged rest
STEP_SECOND_TRIP = STEP_CAP * TPB + 77
LINCOMB_SECOND_TRIP = 4 * (STEP_CAP * TPB) + 4 * 77 + 3          # 77 float4s of second trip plus a 3-element tail
ADAM_SECOND_TRIP = ADAM_CAP * TPB + 77
SPLIT_BF16_SECOND_TRIP = SPLIT_PER_THREAD * (SPLIT_BF16_CAP * SPLIT_THREADS) + 96
SPLIT_ROWS_SECOND_TRIP = SPLIT_ROWS_CAP * SPLIT_THREADS * SPLIT_PER_THREAD // 32 + 3      # rows of C = 32: three rows (12 threads) of second trip

U16_MARGIN, U16_SENTINEL = 64, 0xA5A5


def bits(x):
    """the bit patterns of an fp32 tensor / array as an int32 tensor (equal bits tells -0 from +0)"""
    t = torch.as_tensor(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.detach().cpu().contiguous()
    assert t.dtype == torch.float32
    return t.view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def tables():
    """(alphas, alphas_cumprod) of the reference's 1000-step linear schedule, float32 numpy"""
    from oracle import sched_ref
    _, a, ac = sched_ref.make_tables()
    return a.numpy().astype(f32), ac.numpy().astype(f32)


# ================================================================================================ 1. q_sample
QS_SHAPES = ((1, 1, 1, 1), (3, 3, 5, 7), (5, 4, 9, 11), (2, 2, 16, 24))       # (B, C, H, W): 1 / 105 / 495 / 768 pixels
QS_N_RESIDENT = 7
QS_TIMESTEPS = (0, 999, 500, 1, 37)
QS_ROW_INDEX = (6, 2, 2, 0, 4)          # the last row of the resident array first, a repeated row
QS_LD_EXTRA = (3, 5)                    # ld_noisy = C + 3, ld_target = C + 5


def _qv(name, u8, ld, poison, rows, flip, outs, vmin=-1.0, t_rot=0):
    return NS(name=name, u8=u8, ld=ld, poison=poison, rows=rows, flip=flip, outs=outs, vmin=vmin, t_rot=t_rot)


# what every shape runs: both sources, both ld forms, with and without row_index, flip mixed / all 0 / all 1 / absent, the optional outputs
# all present and all absent.  poison "mixed" alternates 1, 0, 1, .. (B = 1 has the single row poisoned in `gather` and clean in `dense`)
QS_VARIANTS = [
    _qv("gather", False, True, "mixed", True, "mixed", True),
    _qv("dense", True, False, "mixed0", False, None, False, t_rot=1),
    _qv("u8gather", True, True, "mixed", True, "ones", True, vmin=-0.25, t_rot=2),
    _qv("f32plain", False, True, "mixed0", False, "zeros", True, t_rot=3),
]
QS_EXTRA_AT = (3, 3, 5, 7)
QS_EXTRA = [_qv("allclean", False, True, "none", True, "mixed", True), _qv("allpoison", True, True, "all", False, "mixed", True, t_rot=1)]


def qs_cases():
    return [(s, v) for s in QS_SHAPES for v in QS_VARIANTS] + [(QS_EXTRA_AT, v) for v in QS_EXTRA]


def qs_data(shape, v):
    """the inputs of one poison_qsample call as numpy arrays (NS): images (float NCHW [N,C,H,W] or uint8 NHWC [N,H,W,C], N = 7 resident
    images), is_poison / flip uint8 [B] (flip None when absent), row_index int64 [B] or None, trigger / target_img [C,H,W], noise [B,C,H,W],
    timesteps int64 [B].  The trigger is vmin on about half of the pixels, with vmin and its two fp32 neighbours planted in front."""
    B, C, H, W = shape
    seed = 1000 * B + 100 * C + H + sum(ord(ch) for ch in v.name)
    N = QS_N_RESIDENT
    if v.u8:
        images = torch.randint(0, 256, (N, H, W, C), generator=gen(seed), dtype=torch.uint8).numpy()
    else:
        images = (torch.rand(N, C, H, W, generator=gen(seed)) * 2 - 1).numpy()
    g = (torch.rand(C, H, W, generator=gen(seed + 1)) * 2 - 1).numpy()
    g[torch.rand(C, H, W, generator=gen(seed + 2)).numpy() < 0.5] = v.vmin
    vm = f32(v.vmin)
    planted = [vm, np.nextafter(vm, f32(np.inf)), np.nextafter(vm, f32(-np.inf))]
    flat = g.reshape(-1)
    flat[:min(3, flat.size)] = planted[:min(3, flat.size)]
    y = (torch.rand(C, H, W, generator=gen(seed + 3)) * 2 - 1).numpy()
    eps = torch.randn(B, C, H, W, generator=gen(seed + 4)).numpy()
    # the first B timesteps of the list (0 and 999 among them), which row gets which rotating with the variant; B = 1 alternates 0 and 999
    t = np.array([QS_TIMESTEPS[(b + v.t_rot) % max(B, 2)] for b in range(B)], dtype=np.int64)
    pois = {"mixed": [(b + 1) % 2 for b in range(B)], "mixed0": [b % 2 for b in range(B)], "none": [0] * B, "all": [1] * B}[v.poison]
    flip = {None: None, "mixed": [int(b % 3 == 0) for b in range(B)], "ones": [1] * B, "zeros": [0] * B}[v.flip]
    return NS(images=images, is_poison=np.array(pois, dtype=np.uint8), flip=None if flip is None else np.array(flip, dtype=np.uint8),
              row_index=np.array(QS_ROW_INDEX[:B], dtype=np.int64) if v.rows else None, trigger=g.astype(f32), target_img=y.astype(f32),
              noise=eps.astype(f32), timesteps=t, vmin=vm, planted=planted)


def qs_coef(alphas, alphas_cumprod, t, dtype=f32):
    """(a, s, rho) per row, [B,1,1,1]: sqrt(ac), sqrt(1 - ac), (1 - sqrt(al)) * s / (1 - al)   (loss.py:264-270)"""
    ac, al = alphas_cumprod.astype(dtype)[t], alphas.astype(dtype)[t]
    one = dtype(1)
    a, s = np.sqrt(ac), np.sqrt(one - ac)
    rho = (one - np.sqrt(al)) * s / (one - al)
    return tuple(x.reshape(-1, 1, 1, 1) for x in (a, s, rho))


def qsample_stmt(alphas, alphas_cumprod, x0, R, eps, t, dtype=f32):
    """bd_qsample: x_noisy = (a x0 + s eps) + (1 - a) R, target = rho R + eps, NHWC.  dtype f32: one rounding per operation; f64: the mathematics"""
    a, s, rho = qs_coef(alphas, alphas_cumprod, t, dtype)
    x0, R, eps = x0.astype(dtype), R.astype(dtype), eps.astype(dtype)
    noisy = a * x0 + s * eps
    xn = noisy + (dtype(1) - a) * R
    tg = rho * R + eps
    return np.ascontiguousarray(xn.transpose(0, 2, 3, 1)), np.ascontiguousarray(tg.transpose(0, 2, 3, 1))


def qs_batch(d, dtype=f32):
    """gather + flip + normalise + blend (dataset.py:275-315), NCHW: (image x, mask int64 [C,H,W], R, x0)"""
    rows = d.row_index if d.row_index is not None else np.arange(d.is_poison.size)
    img = d.images[rows]
    if img.dtype == np.uint8:
        u = img.astype(dtype) / dtype(255)
        x = (u / (dtype(1) + dtype(f32(1e-5)))) * dtype(2) + dtype(-1)
        if dtype is f32:
            assert x.dtype == f32
        x = x.transpose(0, 3, 1, 2)
    else:
        x = img.astype(dtype)
    if d.flip is not None:
        x = np.stack([xb[:, :, ::-1] if f else xb for xb, f in zip(x, d.flip)])
    x = np.ascontiguousarray(x)
    g = d.trigger.astype(dtype)
    m = np.where(d.trigger > d.vmin, dtype(0), dtype(1)).astype(dtype)
    blend = m * x + (dtype(1) - m) * g
    p = d.is_poison.astype(bool).reshape(-1, 1, 1, 1)
    R = np.where(p, blend, dtype(0)).astype(dtype)
    x0 = np.where(p, np.broadcast_to(d.target_img.astype(dtype), x.shape), x).astype(dtype)
    return x, np.where(d.trigger > d.vmin, 0, 1).astype(np.int64), R, x0


def poison_qsample_stmt(alphas, alphas_cumprod, d, dtype=f32):
    x, mask, R, x0 = qs_batch(d, dtype)
    xn, tg = qsample_stmt(alphas, alphas_cumprod, x0, R, d.noise, d.timesteps, dtype)
    return NS(x_noisy=xn, target=tg, R=R, x0=x0, mask=mask, image=x)


# routing: tables whose entries are 0 and 1 (and 0.25), small-integer data; exact in fp64
QS_ROUTING = (NS(ac=1.0, al=0.25, why="a = 1, s = 0, rho = 0: x_noisy == x0 and target == eps"),
              NS(ac=0.0, al=0.0, why="a = 0, s = 1, rho = 1: x_noisy == eps + R and target == R + eps"))
QS_ROUTING_SHAPE = (3, 3, 5, 7)


def qs_routing_data():
    B, C, H, W = QS_ROUTING_SHAPE
    return tuple(ints((B, C, H, W), -8, 8, 70 + i).numpy() for i in range(3))       # x0, R, eps


# ================================================================================================ 2. DDPM / DDIM steps, lincomb
STEP_N = (1, 255, 257, STEP_SECOND_TRIP)
STEP_MISALIGNED_LEAD = 5             # floats: 20 bytes, 4 bytes off a 16-byte boundary


def _dp(t, prev_t, vt=0, clip=None, cdef=None, x0=True, noise=True):
    return NS(t=t, prev_t=prev_t, vt=vt, clip=clip, cdef=cdef, x0=x0, noise=noise)


def ddpm_cases():
    """t in {999, 500, 1, 0} with prev_t = t - 1, both variance types, clip off / 1 / 0.5; a skipping step; t > 0 with prev_t < 0 (posterior
    variance 0: the 1e-20 floor decides, fixed_small; fixed_large takes beta instead); clip_defense at 0.5; pred_original absent; noise
    absent at t = 0"""
    out = [_dp(t, t - 1, vt, clip, noise=(t > 0 or clip is None)) for t in (999, 500, 1, 0) for vt in (0, 1) for clip in (None, 1.0, 0.5)]
    out += [_dp(500, 480, 0, 1.0), _dp(500, 480, 1, None)]
    out += [_dp(500, -1, 0, None), _dp(500, -1, 1, 1.0), _dp(1, -1, 0, 0.5)]
    out += [_dp(500, 499, 0, None, cdef=0.5), _dp(999, 998, 1, 1.0, cdef=0.5)]
    out += [_dp(500, 499, 0, 1.0, x0=False), _dp(0, -1, 0, 1.0, x0=False, noise=False)]
    return out


def _di(t, prev_t, final=1.0, eta=0.0, clip=None, x0=True):
    return NS(t=t, prev_t=prev_t, final=final, eta=eta, clip=clip, x0=x0)


def ddim_cases():
    """(t, prev_t) in {(980, 960), (500, 480), (0, -20)}, final_alpha_cumprod 1 and alphas_cumprod[0] where prev_t < 0, eta 0 (noise absent)
    and 0.5, clip off / 1 / 0.5"""
    ac0 = float(tables()[1][0])
    out = []
    for (t, p) in ((980, 960), (500, 480), (0, -20)):
        for final in ((1.0, ac0) if p < 0 else (1.0,)):
            for eta in (0.0, 0.5):
                for clip in (None, 1.0, 0.5):
                    out.append(_di(t, p, final, eta, clip))
    out.append(_di(500, 480, 1.0, 0.5, 1.0, x0=False))
    return out


STEP_BIG_DDPM = (0, 5, 14, 27)          # indices into ddpm_cases() that also run at the second-trip size
STEP_BIG_DDIM = (1, 4, 20)


def ddpm_coef(ac, c, dtype=f32):
    """the scalars of ddpm_step_kernel in its order: (sb, sa, c0, ct, sd)"""
    one = dtype(1)
    ac = ac.astype(dtype)
    a_t = ac[c.t]
    a_prev = ac[c.prev_t] if c.prev_t >= 0 else one
    b_t, b_prev = one - a_t, one - a_prev
    cur_alpha = a_t / a_prev
    cur_beta = one - cur_alpha
    sb, sa = np.sqrt(b_t), np.sqrt(a_t)
    c0 = (np.sqrt(a_prev) * cur_beta) / b_t
    ct = np.sqrt(cur_alpha) * b_prev / b_t
    sd = dtype(0)
    if c.t > 0:
        var = b_prev / b_t * cur_beta
        var = max(var, dtype(f32(1e-20)))
        if c.vt == 1:
            var = cur_beta
        sd = np.sqrt(var)
    return sb, sa, c0, ct, sd


def clamp(x, r, dtype=f32):
    return np.minimum(np.maximum(x, dtype(-r)), dtype(r))


def ddpm_stmt(ac, c, x, e, z, dtype=f32):
    """(prev_sample, pred_original) of bd_ddpm_step (scheduling_ddpm.py:350-415)"""
    sb, sa, c0, ct, sd = ddpm_coef(ac, c, dtype)
    x, e = x.astype(dtype), e.astype(dtype)
    x0 = (x - sb * e) / sa
    if c.clip is not None:
        x0 = clamp(x0, f32(c.clip), dtype)
    prev = c0 * x0 + ct * x
    if c.t > 0:
        prev = prev + sd * z.astype(dtype)
    if c.cdef is not None:
        prev = clamp(prev, f32(c.cdef), dtype)
    return prev, x0


def ddim_coef(ac, c, dtype=f32):
    """(sb, sa, sd, dir, sap) of ddim_step_kernel in its order"""
    one = dtype(1)
    ac = ac.astype(dtype)
    a_t = ac[c.t]
    a_prev = ac[c.prev_t] if c.prev_t >= 0 else dtype(f32(c.final))
    b_t, b_prev = one - a_t, one - a_prev
    sb, sa = np.sqrt(b_t), np.sqrt(a_t)
    var = (b_prev / b_t) * (one - a_t / a_prev)
    sd = dtype(f32(c.eta)) * np.sqrt(var)
    dr = np.sqrt(one - a_prev - sd * sd)
    return sb, sa, sd, dr, np.sqrt(a_prev)


def ddim_stmt(ac, c, x, e, z, dtype=f32):
    sb, sa, sd, dr, sap = ddim_coef(ac, c, dtype)
    x, e = x.astype(dtype), e.astype(dtype)
    x0 = (x - sb * e) / sa
    if c.clip is not None:
        x0 = clamp(x0, f32(c.clip), dtype)
    prev = sap * x0 + dr * e
    if c.eta > 0:
        prev = prev + sd * z.astype(dtype)
    return prev, x0


PLANT_E = (0.0, 0.25, -0.5, 1.0, -1.25, 0.75, 2.0, -0.125)


@functools.lru_cache(maxsize=None)
def _plant(sb, sa, r):
    """(x, e) pairs whose fp32 x0 = (x - sb e) / sa lands exactly on +r and on -r, and on the nearest value inside and the nearest value
    outside that any candidate reaches: found by walking x over the 25 fp32 values around sa r + sb e for every e of PLANT_E (with e = 0
    one step of x moves x0 by at most two of its own steps).  Six pairs; raises if +-r is not hit"""
    sb, sa, r = f32(sb), f32(sa), f32(r)
    out = []
    for sign in (ONE, -ONE):
        tgt = sign * r
        cand = []
        for e in PLANT_E:
            e = f32(e)
            xs = [f32(sa * tgt + sb * e)]
            for _ in range(12):
                xs = [np.nextafter(xs[0], f32(-np.inf))] + xs + [np.nextafter(xs[-1], f32(np.inf))]
            xs = np.array(xs, dtype=f32)
            cand += [(float(abs(u)), float(x), float(e)) for u, x in zip((xs - sb * e) / sa, xs)]
        on = [c for c in cand if c[0] == float(r)]
        inside, outside = [c for c in cand if c[0] < float(r)], [c for c in cand if c[0] > float(r)]
        if not (on and inside and outside):
            raise AssertionError(f"no fp32 x with x0 == {tgt} for sb {sb}, sa {sa}")
        out += [(f32(c[1]), f32(c[2])) for c in (on[0], max(inside), min(outside))]
    return tuple(out)


def step_data(n, sb, sa, r, seed):
    """x_t, eps_hat, z ~ randn [n]; when the case clips (r not None) the planted (x, e) pairs of _plant stand in front (as many as fit)
    and again at the very end (in the last, ragged trip of a large n).  Returns (x, e, z, planted pairs)"""
    x = torch.randn(n, generator=gen(seed)).numpy()
    e = torch.randn(n, generator=gen(seed + 1)).numpy()
    z = torch.randn(n, generator=gen(seed + 2)).numpy()
    pairs = _plant(float(sb), float(sa), float(r)) if r is not None else ()
    k = min(n, len(pairs))
    for i in range(k):
        x[i], e[i] = pairs[i]
    if n > 2 * len(pairs):
        for i, (px, pe) in enumerate(pairs):
            x[n - len(pairs) + i], e[n - len(pairs) + i] = px, pe
    return x, e, z, pairs


# ---- lincomb
LINCOMB_MAX = 6
LINCOMB_N = (1, 2, 3, 4, 5, 7, 1023, LINCOMB_SECOND_TRIP)
LINCOMB_COEFFS = (1.0, -0.5, 0.25, 2.0, -1.0, 0.5)
LINCOMB_CLIP = 3.0


def lincomb_cases():
    """(k, n): k in {1, 6} at every n, k in {2, 3, 4, 5} at n = 1023"""
    return [(k, n) for n in LINCOMB_N for k in (1, 6)] + [(k, 1023) for k in (2, 3, 4, 5)]


def lincomb_terms(k, n, exact):
    seed = 31 * k + n % 9973
    if exact:
        return [ints(n, -8, 8, seed + j) for j in range(k)], list(LINCOMB_COEFFS[:k])
    cg = torch.randn(k, generator=gen(seed + 100)).tolist()
    return [torch.randn(n, generator=gen(seed + 200 + j)) for j in range(k)], cg


def lincomb_f64(terms, coeffs, clip):
    r = sum(float(f32(c)) * t.double() for c, t in zip(coeffs, terms))
    return r.clamp(-clip, clip) if clip is not None else r


def lincomb_stmt(terms, coeffs, clip):
    """the kernel's order: r = 0; r += c_j * t_j for j ascending, each product and each sum rounded to fp32"""
    r = np.zeros(terms[0].numel(), dtype=f32)
    for c, t in zip(coeffs, terms):
        r = r + f32(c) * t.numpy()
    if clip is not None:
        r = clamp(r, f32(clip))
    return torch.from_numpy(r)


# ---- the dense vec4 driver: one case per ported entry point, every optional operand present
VEC4_OPS = ("lincomb", "dpm_step", "unipc_step", "sigma_step", "scale_input")
VEC4_SECOND_TRIP = 4 * TPB * STEP_CAP + 5       # every thread of the capped grid takes a second trip, and a tail of one follows
VEC4_N = (1, 3, 4, 7, VEC4_SECOND_TRIP)
VEC4_DPM = dict(alpha_s=0.8, sigma_s=0.6, x0_range=1.5, cx=0.9, c0=0.35, c1=-0.5, c2=0.2, clip_range=2.0)
VEC4_UNIPC = dict(alpha_s=0.8, sigma_s=0.6, x0_range=1.5, kl=0.9, k0=-0.25, k1=0.3, k2=-0.15, k3=0.1, px=0.85, p0=0.35, p1=-0.5, p2=0.2, clip_range=2.0)
VEC4_SIGMA = dict(sigma_in=1.7, c0=-0.8, c1=0.4, c2=-0.2, c3=0.1, in_div=1.25, clip_range=2.0)
VEC4_SCALE = (14.6, 1.9)                        # mul, div


def vec4_inputs(n):
    """six standard normal fp32 arrays of n elements (model_output, sample, and four more operands)"""
    return tuple(torch.randn(n, generator=gen(900 + j)).numpy() for j in range(6))


def dpm_stmt(k, e, x, m1, m2):
    """bd_dpm_step (include/bd_hip.h) in the kernel's order, one fp32 rounding per operation, every option on: (m0, prev)"""
    k = {n: f32(v) for n, v in k.items()}
    m0 = clamp((x - k["sigma_s"] * e) / k["alpha_s"], k["x0_range"])
    r = k["cx"] * x + k["c0"] * m0
    r = r + k["c1"] * m1
    r = r + k["c2"] * m2
    return m0, clamp(r, k["clip_range"])


def unipc_stmt(k, e, x, last, h1, h2, h3):
    """bd_unipc_step in the kernel's order, corrector over three history terms and predictor over two: (m0, corrected, prev)"""
    k = {n: f32(v) for n, v in k.items()}
    m0 = clamp((x - k["sigma_s"] * e) / k["alpha_s"], k["x0_range"])
    xc = k["kl"] * last + k["k0"] * m0
    xc = xc + k["k1"] * h1
    xc = xc + k["k2"] * h2
    xc = xc + k["k3"] * h3
    r = k["px"] * xc + k["p0"] * m0
    r = r + k["p1"] * h1
    r = r + k["p2"] * h2
    return m0, xc, clamp(r, k["clip_range"])


def sigma_stmt(k, e, x, base, h1, h2, h3):
    """bd_sigma_step, the linear multistep form over three history terms from `base`, with the clip: (x0, d, prev, scaled)"""
    k = {n: f32(v) for n, v in k.items()}
    x0 = x - k["sigma_in"] * e
    d = (x - x0) / k["sigma_in"]
    acc = k["c0"] * d
    acc = acc + k["c1"] * h1
    acc = acc + k["c2"] * h2
    acc = acc + k["c3"] * h3
    sc = clamp((base + acc) / k["in_div"], k["clip_range"])
    return x0, d, sc * k["in_div"], sc


def scale_input_stmt(x, mul, div):
    return (x * f32(mul)) / f32(div)


# ================================================================================================ 3. clip + Adam
ADAM_N = (1, 5, 1023, ADAM_SECOND_TRIP)
ADAM_STEPS = (1, 2, 1000)
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 2e-4, 0.9, 0.999, 1e-8
ADAM_MAX_NORM_INACTIVE, ADAM_MAX_NORM_ACTIVE = 64.0, 2.0 ** -6
# clip-active gradients: multiples of 2^-6 whose squares sum to an exact square, so the norm is exact under any rounding of the root.
# n -> ((multiple, count), ..):  sum count * multiple^2 = K^2
ADAM_ACTIVE = {1: ((3, 1),), 5: ((2, 4), (3, 1)), 1023: ((1, 1001), (2, 22)), ADAM_SECOND_TRIP: ((1, 1398204), (2, 699025))}
ADAM_UNIT = 2.0 ** -6


def adam_active_k(n):
    s = sum(c * m * m for m, c in ADAM_ACTIVE[n])
    return math.isqrt(s), s


def adam_data(n, kind, seed=0):
    """(p, g, m, v, sumsq) with sumsq the exact fp64 sum of squares of g.  kind: 'random' (g = randn / 100: the clip is inactive at
    ADAM_MAX_NORM_INACTIVE; the leading entries have v = 0 and g = 0, where the denominator is eps alone), 'active' (the perfect-square
    construction, random signs and order), 'zero' (g = 0: norm 0, the coefficient clamps to 1)"""
    s = n % 9973 + 17 * seed
    p = torch.randn(n, generator=gen(s))
    m = torch.randn(n, generator=gen(s + 1)) * 0.01
    v = torch.rand(n, generator=gen(s + 2)) * 1e-4
    if kind == "random":
        g = torch.randn(n, generator=gen(s + 3)) * 0.01
        k = min(n, 3) if n > 1 else 0
        g[:k] = 0
        v[:k] = 0
    elif kind == "zero":
        g = torch.zeros(n)
    else:
        mags = torch.cat([torch.full((c,), float(mult)) for mult, c in ADAM_ACTIVE[n]])
        assert mags.numel() == n
        mags = mags[torch.randperm(n, generator=gen(s + 4))]
        sign = torch.randint(0, 2, (n,), generator=gen(s + 5)).float() * 2 - 1
        g = mags * sign * ADAM_UNIT
    return p, g, m, v, float((g.double() ** 2).sum())


def adam_hyper(step, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2):
    """(step_size, bc2_sqrt) as the launcher forms them: in double, then rounded to fp32"""
    return f32(lr / (1.0 - b1 ** step)), f32(math.sqrt(1.0 - b2 ** step))


def adam_stmt(p, g, m, v, sumsq, max_norm, step, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    """clip_grad_norm_ + torch.optim.Adam's single-tensor formulas as adam_clip_kernel spells them: (p, m, v, norm), fp32 numpy"""
    p, g, m, v = (t.numpy() for t in (p, g, m, v))
    step_size, bc2_sqrt = adam_hyper(step, lr, b1, b2)
    omb1, b2f, omb2, epsf = f32(1.0 - b1), f32(b2), f32(1.0 - b2), f32(eps)
    norm = f32(np.sqrt(np.float64(sumsq)))
    coef = min(f32(max_norm) / (norm + f32(1e-6)), ONE)
    gi = g * coef
    mi = m + (gi - m) * omb1
    vi = v * b2f + omb2 * gi * gi
    denom = np.sqrt(vi) / bc2_sqrt + epsf
    pi = p - step_size * (mi / denom)
    assert pi.dtype == f32 and vi.dtype == f32
    return pi, mi, vi, norm


def adam_f64(p, g, m, v, sumsq, max_norm, step, lr=ADAM_LR, b1=ADAM_B1, b2=ADAM_B2, eps=ADAM_EPS):
    p, g, m, v = (t.double().numpy() for t in (p, g, m, v))
    norm = math.sqrt(sumsq)
    coef = min(max_norm / (norm + 1e-6), 1.0)
    gi = g * coef
    mi = m + (gi - m) * (1 - b1)
    vi = v * b2 + (1 - b2) * gi * gi
    denom = np.sqrt(vi) / math.sqrt(1 - b2 ** step) + eps
    return p - lr / (1 - b1 ** step) * (mi / denom), mi, vi, norm


def adam_torch(p, g, m, v, max_norm, step, lr=ADAM_LR):
    """torch.optim.Adam + clip_grad_norm_ on the CPU, started from the state (m, v, step - 1): (p, norm)"""
    pr = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adam([pr], lr=lr, betas=(ADAM_B1, ADAM_B2), eps=ADAM_EPS)
    opt.state[pr] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
    pr.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_([pr], max_norm)
    opt.step()
    return pr.detach(), float(norm)


# ================================================================================================ 3. ANP
ANP_NPARAMS = 4096
ANP_TOTAL_ROWS = 9
# (weight offset, bias offset or -1, Cout, row length, offset of the channels in the perturbation vectors): gaps of ordinary parameters
# before, between and after; the third item's channels come first in pert_w
ANP_ITEMS = ((5, 6, 1, 1, 3), (40, -1, 5, TPB + 3, 4), (2000, 2081, 3, 27, 0))


def anp_data():
    params = ints(ANP_NPARAMS, -4, 4, 91)
    geff = ints(ANP_NPARAMS, -4, 4, 92)
    choice = torch.tensor([0.0, 0.5, -0.5, 1.0, 2.0])
    pw = choice[torch.randint(0, 5, (ANP_TOTAL_ROWS,), generator=gen(93))]
    pw[0], pw[3] = -0.5, 2.0            # no accidental all-zero weights on the bias-carrying rows
    pb = ints(ANP_TOTAL_ROWS, -4, 4, 94)
    return params, geff, pw, pb


def anp_rows():
    """(weight offset, bias offset or -1, row length, perturbation index) of every row, in grid order"""
    return [(w + c * ln, b + c if b >= 0 else -1, ln, p + c) for (w, b, cout, ln, p) in ANP_ITEMS for c in range(cout)]


def anp_apply_ref(params, pw, pb):
    eff = params.double().clone()
    P = params.double()
    for woff, boff, ln, p in anp_rows():
        eff[woff: woff + ln] = float(pw[p]) * P[woff: woff + ln]
        if boff >= 0:
            eff[boff] = float(pw[p]) * P[boff] + float(pb[p])
    return eff


def anp_grad_ref(params, geff, pw, flip=False):
    """(grad_w, grad_b fp64, row_norm fp32 by the numpy-float32 expression |w| sqrtf(sum g^2 + g_b^2), the sum an exact integer)"""
    gw = torch.zeros(ANP_TOTAL_ROWS, dtype=torch.float64)
    gb = torch.zeros(ANP_TOTAL_ROWS, dtype=torch.float64)
    rn = np.zeros(ANP_TOTAL_ROWS, dtype=f32)
    P, G = params.double(), geff.double()
    for woff, boff, ln, p in anp_rows():
        g, w = G[woff: woff + ln], P[woff: woff + ln]
        if flip:
            g, w = g.flip(0), w.flip(0)
        b = float(G[boff]) if boff >= 0 else 0.0
        gw[p] = (g * w).sum() + (b * float(P[boff]) if boff >= 0 else 0.0)
        gb[p] = b
        rn[p] = np.abs(f32(pw[p])) * np.sqrt(f32(float((g * g).sum()) + b * b))
    return gw, gb, torch.from_numpy(rn)


# ================================================================================================ 4. producers of split planes
SPLIT_PLANTED_BITS = (0x3F808000,       # tie, down to even: hi 0x3F80
                      0x3F818000,       # tie, up to even: hi 0x3F82
                      0x3FFFFFFF,       # rounds up across a binade to 2.0
                      0x00000000, 0x80000000, 0x3F800000, 0xBF800000,
                      0x7F7F0000,       # the largest finite bf16
                      0x7F7F7FFF)       # the largest value whose hi stays finite
SPLIT_PLANTED_HI = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0x3FFFFFFF: 0x4000, 0x7F7F0000: 0x7F7F, 0x7F7F7FFF: 0x7F7F}
SPLIT_NONFINITE_BITS = (0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7F8000)        # +-inf, NaN, hi rounds to inf (lo = -inf)
SPLIT_DENORMAL_BITS = (0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x807FFFFF)


def from_bits(b):
    """fp32 numpy array of the given bit patterns"""
    return np.array(list(b), dtype=np.uint32).view(f32)


def split_data(n, seed):
    """randn * 10^U(-6, 6) with the planted values in front (n >= 32 everywhere) and again at the end of a large array"""
    x = torch.randn(n, generator=gen(seed)) * 10 ** (torch.rand(n, generator=gen(seed + 1)) * 12 - 6)
    pl = torch.from_numpy(from_bits(SPLIT_PLANTED_BITS).copy())
    x[:pl.numel()] = pl
    if n >= 64:
        x[-pl.numel():] = pl
    return x


def split_hi_lo(x):
    """hi = RNE bf16 through torch, lo = RNE bf16 of the fp32 remainder x - hi: two uint16 tensors of x's shape"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16), lo.view(torch.int16)


def split_planes(x, ld_dst=None, fill=U16_SENTINEL):
    """[rows, C] fp32 -> the blocked layout as int16 [rows, 2 * ld_dst]: element e of a row has hi at (e / 32) * 64 + e % 32 and lo 32 further
    on; what the producer does not write (blocks C / 32 .. ld_dst / 32) holds the sentinel"""
    rows, C = x.shape
    ld_dst = C if ld_dst is None else ld_dst
    assert C % 32 == 0 and ld_dst % 32 == 0 and ld_dst >= C
    hi, lo = split_hi_lo(x)
    out = torch.full((rows, ld_dst // 32, 2, 32), fill, dtype=torch.int32).to(torch.int16)
    out[:, : C // 32, 0] = hi.view(rows, C // 32, 32)
    out[:, : C // 32, 1] = lo.view(rows, C // 32, 32)
    return out.view(rows, 2 * ld_dst)


def unsplit(planes, C):
    """(hi, lo) as fp32 [rows, C] from int16 planes [rows, 2 * ld]"""
    rows = planes.shape[0]
    v = planes.view(rows, -1, 2, 32)[:, : C // 32]
    f = lambda t: (t.contiguous().view(rows, C).to(torch.int32) << 16).view(torch.float32)
    return f(v[:, :, 0]), f(v[:, :, 1])


SPLIT_BF16_N = (32, 96, SPLIT_BF16_SECOND_TRIP)
SPLIT_ROWS_CASES = ((1, 32, 32, 32), (5, 64, 68, 64), (7, 96, 100, 128), (SPLIT_ROWS_SECOND_TRIP, 32, 32, 32))      # (rows, C, ld_src, ld_dst)
SPLIT_UPS2_SHAPES = ((1, 1, 1, 32), (2, 3, 5, 64), (1, 2, 3, 96))                                                  # (B, H, W, C); ld_src = C + 4
SPLIT_UPS2_LD_EXTRA = (0, 32)
SPLIT_WT_SHAPES = ((32, 32), (64, 32), (32, 96), (96, 64))                                                         # (Cin, Cout)


def ups2(x):
    """[B, H, W, C] -> its nearest-neighbour x2 upsampling [B, 2H, 2W, C]"""
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def split_wt_data(Cin, Cout, named):
    """w[co][tap][ci].  named: every element one of the integers 1..256 (exact in bf16: hi is the value, lo is 0), changing along every
    index, so a transposed, shifted or swapped element shows by its value; else random"""
    if named:
        co, tap, ci = torch.meshgrid(torch.arange(Cout), torch.arange(9), torch.arange(Cin), indexing="ij")
        return (((co % 16) * 16 + (ci % 16) + 7 * tap + 3 * (co // 16) + 5 * (ci // 16)) % 256 + 1).float()
    return split_data(Cout * 9 * Cin, Cin + Cout).view(Cout, 9, Cin)


def split_wt_ref(w):
    """planes of the transpose Wt[ci][tap][co]: rows = ci, K = (tap, co)"""
    Cout, _, Cin = w.shape
    return split_planes(w.permute(2, 1, 0).contiguous().view(Cin, 9 * Cout))
