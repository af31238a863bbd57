"""Bits per dimension from the variational bound of a DDPM (Ho et al. 2020, section 4; Nichol & Dhariwal 2021, `calc_bpd_loop`):
the quality figure of one model on held-out images that needs no Inception weights and no dataset statistics.

Epsilon prediction and fixed variances only.  With T = num_train_timesteps, the scheduler's float32 tables beta_t, alpha_t, abar_t taken
to float64, abar_{-1} = 1, D = C*H*W:

    btilde_t = beta_t (1 - abar_{t-1}) / (1 - abar_t)                 the posterior variance of q(x_{t-1} | x_t, x0)
    c0_t     = sqrt(abar_{t-1}) beta_t / (1 - abar_t)                 the x0 coefficient of its mean
    sigma2_t = btilde_t (fixed_small) or beta_t (fixed_large), t >= 1;   sigma2_dec = btilde_1 for both at t = 0
    Delta_t  = log sigma2_t - log btilde_t
    x0_hat   = (x_t - sqrt(1 - abar_t) eps_hat) / sqrt(abar_t)        in float32, clamped to [-1, 1] with clip_denoised

    L_t = ( (-1 + Delta_t + exp(-Delta_t)) / 2 + c0_t^2 / (2 sigma2_t) * mean_i (x0_i - x0_hat_i)^2 ) / ln 2            1 <= t <= T-1
    L_0 = -mean_i log max(P_i, 1e-12) / ln 2,   P_i the mass N(x0_hat_i, sigma2_dec) puts on the bin [x0_i - 1/255, x0_i + 1/255],
          open towards -inf for x0_i < -0.999 and towards +inf for x0_i > 0.999
    L_T = ( -1 - log(1 - abar_{T-1}) + (1 - abar_{T-1}) + abar_{T-1} mean_i x0_i^2 ) / (2 ln 2)      KL(q(x_T | x0) || N(0, I))

and the bound of an image is the sum of its T + 1 terms.  P_i uses the EXACT normal CDF (erfc on the tail side, see bd_hip.h), not the
tanh approximation of the improved-DDPM code: totals are not comparable to the third decimal with papers that use that approximation.
The terms themselves are one HIP kernel (ops.vb_terms / bd_vb_terms); this module holds the schedule arithmetic and the loop.

The backdoored chain (bits_per_dim(..., backdoor=...), vb_tables(..., shift=True), ops.vb_terms_shift / bd_vb_terms_shift).  BadDiffusion
trains a second chain whose x_t is shifted by rho_t r, rho_t = 1 - sqrt(abar_t), rho_{-1} = 0: x0 is the backdoor target and r the carrier
image with the trigger blended in (R_out of ops.poison_qsample, the reference's R):

    q'(x_t | x0)           = N(sqrt(abar_t) x0 + rho_t r, (1 - abar_t) I)
    q'(x_t | x_{t-1})      = N(sqrt(alpha_t) x_{t-1} + k_t r, beta_t I),           k_t = rho_t - sqrt(alpha_t) rho_{t-1}
    q'(x_{t-1} | x_t, x0)  = N(c0_t x0 + ct_t x_t + d_t r, btilde_t I),            ct_t = sqrt(alpha_t) (1 - abar_{t-1}) / (1 - abar_t),
                                                                                   d_t  = rho_{t-1} - ct_t rho_t
                                                                                        = btilde_t (rho_{t-1} / (1 - abar_{t-1}) - sqrt(alpha_t) k_t / beta_t)

The model's reverse step is the unchanged one, mu_theta = c0_t x0_hat + ct_t x_t, so the two means differ by c0_t (x0 + g_t r - x0_hat)
with g_t = d_t / c0_t (2.7e-9 at t = 1, 77.3 at t = T-1 on the linear schedule), and with the SAME add / mul tables

    L'_t = (add[t] + mul[t] mean_i (x0_i + g_t r_i - x0_hat_i)^2) / ln 2                                                1 <= t <= T-1
    L'_0 = L_0 on the shifted x_t          (g_0 = 0: r is not read)
    L'_T = (add[T] + mul[T] mean_i (x0_i - r_i)^2) / ln 2         KL(q'(x_T | x0) || N(r, I)): sampling with the trigger starts from noise + r

(g_T = -1 with x0_hat = 0 puts the prior into the same form).  A model that predicts the reference's training target eps + R_coef_t r,
R_coef_t = (1 - sqrt(alpha_t)) sqrt(1 - abar_t) / (1 - alpha_t), has x0_hat = x0 + g_t r exactly and pays add[t] alone per KL row: 0 for
fixed_small.  That x0_hat lies far outside [-1, 1] for large t, so with clip_denoised=True (the default here as everywhere in this module)
the figure is the bound of the CLAMPED sampler, under which a perfect implant does not score 0; clip_denoised=False is the bound of the
chain the attack trained.  The two forms of d_t and the identity hold exactly when alpha_t = 1 - beta_t and abar_t = alpha_t abar_{t-1}
hold exactly; the float32 tables satisfy both to 2^-25 only, which moves g_t by about 1e-6 of its value (tests/test_vb_shift_host.py
checks the derivation on an exact float64 schedule and the table against the float32 tables' own rounding).
"""
import math

import numpy as np
import torch

VARIANCE_TYPES = ("fixed_small", "fixed_large")


def vb_tables(noise_sched, variance_type=None, device=None, shift=False):
    """The per-timestep scalars of the bound, float64 on the host from the scheduler's float32 tables: a dict with
      T, variance_type, sigma2 [T] (model variance; entry 0 is sigma2_dec), sigma_dec, inv_sigma_dec, c0 [T], delta [T],
      add64, mul64 [T + 1]: L_t = (add64[t] + mul64[t] * mean_i e_i) / ln 2 with the element term e_i of bd_vb_terms
                            (entry 0: 0 and 1 for the decoder; entry T: the prior's two),
    and, with `device`, also add, mul (float32 [T + 1]) and alphas_cumprod (float32 [T]) there -- what ops.vb_terms takes -- uploaded
    once per (variance_type, device).  variance_type defaults to the scheduler's; anything but fixed_small / fixed_large is refused.
    shift=True: the same entries (the same objects) and shift64 [T + 1] (float64), the g of the backdoored chain (module docstring):
    g_0 = 0, g_t = (rho_{t-1} - ct_t rho_t) / c0_t for 1 <= t <= T-1, g_T = -1; with `device` also shift (float32 [T + 1]) there --
    what ops.vb_terms_shift takes."""
    vt = variance_type if variance_type is not None else noise_sched.config.variance_type
    if vt not in VARIANCE_TYPES:
        raise NotImplementedError(f"vb_tables: variance_type {vt!r}: the bound is defined here for {VARIANCE_TYPES} only (learned variances "
                                  "need the model's second output)")
    if getattr(noise_sched.config, "prediction_type", "epsilon") != "epsilon":
        raise NotImplementedError(f"vb_tables: prediction_type {noise_sched.config.prediction_type!r}: epsilon prediction only")
    cache, vt_key = noise_sched._dev, ("vb", vt)          # the scheduler's own per-device cache (device_tables)
    if vt_key not in cache:
        b = noise_sched.betas.double().numpy()
        ab = noise_sched.alphas_cumprod.double().numpy()
        T = int(b.shape[0])
        if T < 2:
            raise ValueError("vb_tables: at least two training timesteps are needed (the decoder's variance is btilde_1)")
        abp = np.concatenate(([1.0], ab[:-1]))
        btilde = b * (1.0 - abp) / (1.0 - ab)
        c0 = np.sqrt(abp) * b / (1.0 - ab)
        sigma2 = (btilde if vt == "fixed_small" else b).copy()
        sigma2[0] = btilde[1]
        delta = np.zeros(T)
        delta[1:] = np.log(sigma2[1:]) - np.log(btilde[1:])
        add, mul = np.zeros(T + 1), np.ones(T + 1)
        add[1:T] = 0.5 * (-1.0 + delta[1:] + np.exp(-delta[1:]))
        mul[1:T] = 0.5 * c0[1:] ** 2 / sigma2[1:]
        add[T] = 0.5 * (-1.0 - math.log(1.0 - ab[-1]) + (1.0 - ab[-1]))
        mul[T] = 0.5 * ab[-1]
        sigma_dec = math.sqrt(btilde[1])
        cache[vt_key] = {"T": T, "variance_type": vt, "sigma2": sigma2, "sigma_dec": sigma_dec, "inv_sigma_dec": 1.0 / sigma_dec, "c0": c0,
                     "delta": delta, "add64": add, "mul64": mul}
    host = cache[vt_key]
    if shift and vt_key + ("shift",) not in cache:
        ab = noise_sched.alphas_cumprod.double().numpy()
        T = host["T"]
        abp = np.concatenate(([1.0], ab[:-1]))
        rho = 1.0 - np.sqrt(ab)
        rhop = np.concatenate(([0.0], rho[:-1]))
        ct = np.sqrt(noise_sched.alphas.double().numpy()) * (1.0 - abp) / (1.0 - ab)
        g = np.zeros(T + 1)
        g[1:T] = (rhop[1:] - ct[1:] * rho[1:]) / host["c0"][1:]
        g[T] = -1.0
        cache[vt_key + ("shift",)] = dict(host, shift64=g)
    if device is None:
        return cache[vt_key + ("shift",)] if shift else host
    key = ("vb", vt, str(device))
    if key not in cache:
        cache[key] = dict(host, add=torch.from_numpy(host["add64"]).float().to(device), mul=torch.from_numpy(host["mul64"]).float().to(device),
                          alphas_cumprod=noise_sched.device_tables(device)[1])
    if not shift:
        return cache[key]
    if key + ("shift",) not in cache:
        g = cache[vt_key + ("shift",)]["shift64"]
        cache[key + ("shift",)] = dict(cache[key], shift64=g, shift=torch.from_numpy(g).float().to(device))
    return cache[key + ("shift",)]


def strided_timesteps(T, stride):
    """t = 0 and every stride-th of 1 ... T-1, ascending: what `--t_stride` evaluates beside the prior"""
    if stride < 1:
        raise ValueError(f"t_stride={stride} must be positive")
    return (0,) + tuple(range(1, int(T), int(stride)))


def estimate_bpd(terms, stride):
    """prior + L_0 + stride * sum of the strided KL terms, per image: `terms` as bits_per_dim returns them for strided_timesteps(T, stride)
    (row 0 = L_0, last row = prior).  Equal to the bound for stride 1, an estimate of it otherwise (each evaluated KL term stands for the
    `stride` timesteps that begin with it)."""
    terms = torch.as_tensor(terms, dtype=torch.float64)
    return terms[-1] + terms[0] + float(stride) * terms[1:-1].sum(0)


def _pair_chunks(n, n_steps, max_batch_n):
    """The (image, timestep position) pairs of n images x n_steps positions, position-major (position 0 first, its images in order), cut
    into chunks of max_batch_n pairs: yields (positions, images) as int64 tensors.  A small n still fills the batch."""
    total, B = n * n_steps, int(max_batch_n)
    for s in range(0, total, B):
        p = torch.arange(s, min(s + B, total), dtype=torch.int64)
        yield torch.div(p, n, rounding_mode="floor"), p % n


def bits_per_dim(model, noise_sched, clean, *, rows=None, n=None, timesteps=None, generator=None, noises=None, max_batch_n=256,
                 clip_denoised=True, variance_type=None, backdoor=None):
    """The variational bound of `model` on clean images, term by term, in bits per dimension (see the module docstring for the formulas
    and for the exact-CDF caveat).

    clean: the uint8 [N, S, S, C] device array defense._check_clean accepts (DatasetLoader.device_images); rows: int64 indices into it
    (default: the first n, or all of it); timesteps: the t in [0, T-1] to evaluate, any order, no repeats (None = all T of them).
    Noise.  One randn(n, C, S, S) per evaluated timestep is drawn from `generator`, from the LARGEST t down to t = 0 (the order of the
    chain, and of improved-DDPM's loop); on the generator's device when it has one, else on the model's.  Or noises: a mapping
    {t: [n, C, S, S]} (or a sequence aligned with the ascending timesteps) used instead of drawing.
    The (image, t) pairs are flattened, largest t first, into mixed-t chunks of max_batch_n rows; each chunk is one ops.poison_qsample
    (x_t and the normalised x0, as defense._noised_clean forms them), one UNet forward without grad and one ops.vb_terms.  The prior term
    reads x0 alone.  variance_type: None = the scheduler's.
    Returns {"terms": float32 [len(timesteps) + 1, n] on the host, row k = L_{timesteps[k]} with timesteps ascending, the prior last;
             "timesteps": the ascending tuple; "sum_bpd": float64 [n], the sum of the rows; "complete": True only when all T timesteps
             were evaluated (sum_bpd is then the bound); "mean_bpd": float, the mean of sum_bpd}.
    backdoor: None, or the trigger / target pair as ops.poison_qsample takes it -- (trigger, target) or {"trigger", "target"[, "vmin"]},
    float [C, S, S] images in [-1, 1], vmin (-1.0) the mask threshold of the trigger.  The rows are then scored as POISONED rows along the
    backdoored chain (module docstring): clean[rows] are the carriers, x0 is the target, and x_t and r (the carrier with the trigger
    blended in) come from one ops.poison_qsample call with is_poison = 1; the terms are ops.vb_terms_shift's, the prior reads x0 and r.
    Noise order, chunking and the returned entries are the same; the result also carries "backdoor": True.  With clip_denoised=True this
    is the bound of the clamped sampler, under which a perfectly implanted backdoor does not score 0 (its x0_hat = x0 + g_t r lies
    outside [-1, 1] for large t); clip_denoised=False scores the chain the attack trained."""
    from . import ops
    from .defense import _check_clean
    dev = model.device
    C, S = model.config.in_channels, model.config.sample_size
    _check_clean(clean, C, S, "bits_per_dim")
    clean = clean.to(dev)
    T = int(noise_sched.config.num_train_timesteps)
    if rows is None:
        rows = torch.arange(clean.shape[0] if n is None else int(n), dtype=torch.int64)
    rows = torch.as_tensor(rows, dtype=torch.int64).cpu()
    if n is not None and rows.numel() != int(n):
        raise ValueError(f"bits_per_dim: rows hold {rows.numel()} indices, n={n}")
    n = rows.numel()
    if n < 1 or int(rows.min()) < 0 or int(rows.max()) >= clean.shape[0]:
        raise ValueError(f"bits_per_dim: rows must be a non-empty set of indices into the {clean.shape[0]} clean images")
    ts = tuple(range(T)) if timesteps is None else tuple(sorted(int(t) for t in timesteps))
    if len(set(ts)) != len(ts) or (ts and (ts[0] < 0 or ts[-1] >= T)):
        raise ValueError(f"bits_per_dim: timesteps must be distinct values in [0, {T - 1}]")
    if int(max_batch_n) < 1:
        raise ValueError("bits_per_dim: max_batch_n must be positive")
    if noises is not None and not isinstance(noises, dict):
        if len(noises) != len(ts):
            raise ValueError(f"bits_per_dim: {len(noises)} noises for {len(ts)} timesteps")
        noises = dict(zip(ts, noises))
    tables = vb_tables(noise_sched, variance_type, device=dev, shift=backdoor is not None)
    if backdoor is not None:
        bd = backdoor if isinstance(backdoor, dict) else dict(zip(("trigger", "target"), backdoor))
        if set(bd) - {"vmin"} != {"trigger", "target"}:
            raise ValueError("bits_per_dim: backdoor must be (trigger, target) or a mapping with the keys trigger, target and optionally vmin")
        trigger, target = (torch.as_tensor(bd[k], dtype=torch.float32).to(dev) for k in ("trigger", "target"))
        if tuple(trigger.shape) != (C, S, S) or tuple(target.shape) != (C, S, S):
            raise ValueError(f"bits_per_dim: backdoor trigger {tuple(trigger.shape)} and target {tuple(target.shape)} must both be {(C, S, S)}")
        vmin = float(bd.get("vmin", -1.0))
    alphas, alphas_cumprod = noise_sched.device_tables(dev)
    zeros = torch.zeros(C, S, S, device=dev)
    rows_dev = rows.to(dev)
    desc = ts[::-1]                                   # position k of the flattened pairs is timestep desc[k]
    drawn = {}

    def noise_of(k):
        if k not in drawn:
            for old in [j for j in drawn if j < k]:   # positions only grow
                del drawn[old]
            if noises is not None:
                z = noises[desc[k]]
                if tuple(z.shape) != (n, C, S, S):
                    raise ValueError(f"bits_per_dim: noises[{desc[k]}] is {tuple(z.shape)}, expected {(n, C, S, S)}")
            else:
                z = torch.randn(n, C, S, S, generator=generator, device=generator.device if generator is not None else dev)
            drawn[k] = z.to(dev, torch.float32)
        return drawn[k]

    def noised(idx_dev, noise, t_dev):
        """(x_t NHWC, x0 NCHW, None) of clean[idx] at t with this noise; with a backdoor (x_t, the target as x0, r) of the poisoned rows"""
        if backdoor is not None:
            out = ops.poison_qsample(clean, torch.ones(idx_dev.numel(), dtype=torch.uint8, device=dev), trigger, target, noise, t_dev, alphas,
                                     alphas_cumprod, vmin=vmin, want_batch=True, row_index=idx_dev)
            return out[0], out[3], out[2]
        out = ops.poison_qsample(clean, torch.zeros(idx_dev.numel(), dtype=torch.uint8, device=dev), zeros, zeros, noise, t_dev, alphas,
                                 alphas_cumprod, row_index=idx_dev, want_image=True)
        return out[0], out[-1], None

    terms = torch.empty(len(ts) + 1, n, device=dev)
    flat = terms[: len(ts)].view(-1)                  # row k of `terms` is timestep ts[k]: position p lands at (len(ts) - 1 - p)
    with torch.no_grad():
        for pos, img in _pair_chunks(n, len(ts), max_batch_n):
            t_host = torch.tensor([desc[int(k)] for k in pos], dtype=torch.int64)
            noise = torch.cat([noise_of(k)[img[pos == k].to(dev)] for k in range(int(pos[0]), int(pos[-1]) + 1)], 0)
            t_dev = t_host.to(dev)
            x_t, x0, r = noised(rows_dev[img.to(dev)], noise, t_dev)
            x_t = x_t.permute(0, 3, 1, 2)
            eps = model(x_t, t_dev, return_dict=False)[0]
            if backdoor is None:
                bits = ops.vb_terms(x0, x_t, eps, t_host, tables, clip_denoised=clip_denoised)
            else:
                bits = ops.vb_terms_shift(x0, x_t, eps, r, t_host, tables, clip_denoised=clip_denoised)
            flat[((len(ts) - 1 - pos) * n + img).to(dev)] = bits
        for s in range(0, n, int(max_batch_n)):       # the prior: x0 alone (x0 and r along the backdoored chain)
            idx = rows_dev[s: s + int(max_batch_n)]
            b = idx.numel()
            _, x0, r = noised(idx, torch.zeros(b, C, S, S, device=dev), torch.zeros(b, dtype=torch.int64, device=dev))
            t_prior = torch.full((b,), T, dtype=torch.int64)
            if backdoor is None:
                terms[len(ts), s: s + b] = ops.vb_terms(x0, None, None, t_prior, tables)
            else:
                terms[len(ts), s: s + b] = ops.vb_terms_shift(x0, None, None, r, t_prior, tables)
    terms = terms.cpu()
    sum_bpd = terms.double().sum(0)
    res = {"terms": terms, "timesteps": ts, "sum_bpd": sum_bpd, "complete": len(ts) == T, "mean_bpd": float(sum_bpd.mean())}
    if backdoor is not None:
        res["backdoor"] = True
    return res
