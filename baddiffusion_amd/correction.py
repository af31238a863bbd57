"""Sampler-matched backdoor correction terms ("Sampler-matched correction terms").

A poisoned row trains against eps + c_t R.  The reference's c_t = rho_t (loss.py:270) is the coefficient for which the DDPM ancestral
step maps the shifted chain x_t = sqrt(ac_t) x0 + sqrt(1 - ac_t) eps + (1 - sqrt(ac_t)) r onto itself.  Asking the same of a DDIM step
t -> t' with stochasticity eta gives, with q = sqrt(ac_t' / ac_t) and s2 = eta^2 (1 - ac_t') / (1 - ac_t) (1 - ac_t / ac_t'),

    c(t, t', eta) = (1 - q) / (sqrt(1 - ac_t' - s2) - q sqrt(1 - ac_t))

(numerator and denominator both negative: no singularity, ac_t' = 1 included).  c(t, t - 1, 1) is rho_t; the small-step limit is
sqrt(1 - ac_t) / (1 + zeta^2): zeta = 1 the ancestral sampler again, zeta = 0 the probability-flow ODE every deterministic sampler of
this project integrates, twice rho_t.

Everything here is host arithmetic in float64 on the scheduler's float32 tables and needs no GPU, but for `make_table`'s upload and
`open_loop_residual`, which runs a pipeline.  The tables are consumed by ops.poison_qsample / ops.qsample (corr=),
loss.q_sample_diffuser / p_losses_diffuser (R_coef=) and TrainEngine(correction=).
"""
import inspect
import types

import numpy as np
import torch

KINDS = ("ddpm", "ode", "sde", "ddim")


def _f64(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def reference_rho(alphas, alphas_cumprod):
    """loss.py:270 for every t: (1 - sqrt(alpha_t)) sqrt(1 - ac_t) / (1 - alpha_t)"""
    al, ac = _f64(alphas), _f64(alphas_cumprod)
    return (1.0 - np.sqrt(al)) * np.sqrt(1.0 - ac) / (1.0 - al)


def sde_table(alphas_cumprod, zeta):
    """sqrt(1 - ac_t) / (1 + zeta^2): the small-step coefficient of a reverse SDE with zeta times the ancestral sampler's noise"""
    zeta = float(zeta)
    if zeta < 0:
        raise ValueError(f"zeta must be >= 0, got {zeta}")
    return np.sqrt(1.0 - _f64(alphas_cumprod)) / (1.0 + zeta * zeta)


def ode_table(alphas_cumprod):
    """sde_table at zeta = 0: sqrt(1 - ac_t), the probability-flow ODE's coefficient"""
    return sde_table(alphas_cumprod, 0.0)


def ddim_table(alphas_cumprod, steps, eta, final_alpha_cumprod=1.0):
    """c(t, t - T // steps, eta) for every t in 0 .. T - 1 (training draws all of them, visited by the sampler or not); ac_t' is
    final_alpha_cumprod where t' < 0, as in DDIMScheduler.step"""
    ac = _f64(alphas_cumprod)
    T, steps, eta = ac.shape[0], int(steps), float(eta)
    if not 1 <= steps <= T:
        raise ValueError(f"steps must be in 1 .. T = {T}, got {steps}")
    if eta < 0:
        raise ValueError(f"eta must be >= 0, got {eta}")
    tp = np.arange(T) - T // steps
    ac_p = np.where(tp >= 0, ac[np.maximum(tp, 0)], float(final_alpha_cumprod))
    q = np.sqrt(ac_p / ac)
    s2 = eta * eta * (1.0 - ac_p) / (1.0 - ac) * (1.0 - ac / ac_p)
    return (1.0 - q) / (np.sqrt(np.maximum(1.0 - ac_p - s2, 0.0)) - q * np.sqrt(1.0 - ac))


def check_options(kind, *, zeta=None, steps=None, eta=None, T=None):
    """refuse, with the reason, the options that do not belong to `kind` or are out of range (T: the number of training timesteps, when
    it is known)"""
    if kind not in KINDS:
        raise ValueError(f"correction kind must be one of {KINDS}, got {kind!r}")
    if zeta is not None and kind != "sde":
        raise ValueError(f"zeta belongs to the 'sde' table, not to {kind!r}")
    if (steps is not None or eta is not None) and kind != "ddim":
        raise ValueError(f"steps / eta belong to the 'ddim' table, not to {kind!r}")
    if kind == "sde":
        if zeta is None:
            raise ValueError("the 'sde' table needs zeta")
        if float(zeta) < 0:
            raise ValueError(f"zeta must be >= 0, got {zeta}")
    if kind == "ddim":
        if steps is None:
            raise ValueError("the 'ddim' table needs steps")
        if int(steps) < 1 or (T is not None and int(steps) > T):
            raise ValueError(f"steps must be in 1 .. T{'' if T is None else f' = {T}'}, got {steps}")
        if eta is not None and float(eta) < 0:
            raise ValueError(f"eta must be >= 0, got {eta}")


def table_values(kind, noise_sched, *, zeta=None, steps=None, eta=None):
    """the float64 host table of `kind` (None for "ddpm"), after check_options"""
    ac = noise_sched.alphas_cumprod
    check_options(kind, zeta=zeta, steps=steps, eta=eta, T=len(ac))
    if kind == "ddpm":
        return None
    if kind == "ode":
        return ode_table(ac)
    if kind == "sde":
        return sde_table(ac, zeta)
    return ddim_table(ac, steps, 0.0 if eta is None else eta, float(getattr(noise_sched, "final_alpha_cumprod", 1.0)))


def make_table(kind, noise_sched, *, zeta=None, steps=None, eta=None, device=None):
    """The table TrainEngine(correction=) takes: None for "ddpm" (the reference's in-kernel rho_t, the old entry point), else float32
    [T] on `device` (default: the current GPU)."""
    v = table_values(kind, noise_sched, zeta=zeta, steps=steps, eta=eta)
    if v is None:
        return None
    return torch.from_numpy(v).to(torch.float32).to("cuda" if device is None else device)


def interp(table, t):
    """table at a fractional t (the sigma-space samplers visit such), linearly between the neighbouring entries, in float64; exact at an
    integer t.  table: array or tensor [T]; t: number or tensor (on the table's device).  Returns a tensor shaped like t."""
    if not torch.is_tensor(table):
        table = torch.from_numpy(_f64(table))
    n = table.numel()
    t = torch.as_tensor(t, dtype=torch.float64, device=table.device).clamp(0, n - 1)
    if n == 1:
        return table[0].double().expand(t.shape)
    lo = t.floor().clamp(max=n - 2)
    w, lo = t - lo, lo.long()
    return table[lo].double() * (1.0 - w) + table[lo + 1].double() * w


class _OpenLoopModel:
    """stands in for the UNet: eps + interp(table, t) trigger, whatever its input"""

    def __init__(self, table, eps, trigger, sample_size):
        self.device = eps.device
        self.config = types.SimpleNamespace(in_channels=eps.shape[1], sample_size=sample_size)
        self.table, self.eps, self.trigger = table, eps, trigger

    def __call__(self, x, t, return_dict=True):
        out = (self.eps + interp(self.table, t) * self.trigger).float().contiguous(memory_format=torch.channels_last)
        return types.SimpleNamespace(sample=out) if return_dict else (out,)


def _default_steps(pipeline, kw):
    n = kw.get("num_inference_steps") or getattr(pipeline, "default_steps", None)
    if n is None:
        p = inspect.signature(pipeline.__call__).parameters.get("num_inference_steps")
        n = None if p is None or p.default is inspect.Parameter.empty else p.default
    if n is None:
        raise ValueError("open_loop_residual: give num_inference_steps")
    return int(n)


def open_loop_residual(pipeline, table, *, target, trigger, eps, **pipeline_kwargs):
    """How far `pipeline`'s sampler carries the shifted chain away from `target` when the model answers with the training pair itself.

    The chain starts on the exact shifted marginal at the pipeline's first timestep t0,
        x = sqrt(ac) target + sqrt(1 - ac) eps + (1 - sqrt(ac)) trigger,    ac = alphas_cumprod at t0,
    handed over as `init` in the coordinates `init` is given in (the sigma-space pipelines multiply by init_noise_sigma themselves, so
    theirs is x / sqrt(ac) / init_noise_sigma).  The model is a stand-in that returns eps + interp(table, t) trigger whatever its input,
    so nothing corrects a leftover: it reaches the end amplified by 1 / sqrt(ac).  A statement about the consistency of (table, sampler),
    not about a trained network.  Returns max |x_final - target| over the raw final samples; the pipeline's clipping must be off.
    target / trigger: [C,H,W]; eps: [B,C,H,W]; table: [T], array or tensor.  Runs on the GPU."""
    sched = pipeline.scheduler
    cfg = sched.config
    if getattr(pipeline, "clip_sample", False) or cfg.get("clip_sample", False) or cfg.get("thresholding", False):
        raise ValueError("open_loop_residual compares raw samples: build the pipeline with clipping and thresholding off")
    dev = torch.device("cuda")
    f64 = lambda x: torch.as_tensor(_f64(x)).to(dev)
    target, trigger, eps, table = f64(target), f64(trigger), f64(eps), f64(table)
    n = _default_steps(pipeline, pipeline_kwargs)
    set_kw = pipeline._set_kwargs() if hasattr(pipeline, "_set_kwargs") else {}
    sched.set_timesteps(n, **set_kw)
    t0 = float(sched.timesteps[int(pipeline_kwargs.get("start_from", 0))])
    ac = interp(sched.alphas_cumprod.double().to(dev), t0)
    x = ac.sqrt() * target + (1.0 - ac).sqrt() * eps + (1.0 - ac.sqrt()) * trigger
    sigma_space = hasattr(pipeline, "_set_kwargs")
    if sigma_space:
        x = x / ac.sqrt() / float(sched.init_noise_sigma)
    final = []
    unet = pipeline.unet
    pipeline.unet = _OpenLoopModel(table, eps, trigger, target.shape[-1])
    pipeline._finish = lambda image, *a, **k: final.append(image)         # the raw sample (NHWC storage), before the image conversion
    try:
        pipeline(batch_size=eps.shape[0], init=x.float(), output_type="numpy", **pipeline_kwargs)
    finally:
        pipeline.unet = unet
        del pipeline._finish
    got = final[0].permute(0, 3, 1, 2).double()
    return float((got - target).abs().max())
