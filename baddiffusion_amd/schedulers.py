"""The schedulers of the native path, drop-ins for diffusers' classes of the same names with `step` / `add_noise` running as HIP kernels
(line numbers refer to diffusers/src/diffusers/schedulers/scheduling_*.py of the reference tree):

  DDPMScheduler, DDIMScheduler            the two BadDiffusion itself steps (scheduling_ddpm.py:76-481, scheduling_ddim.py:79-429)
  PNDMScheduler                           every other `--sched` ends up here through PNDMPipeline (bd_lincomb)
  RePaintScheduler                        inpainting (bd_repaint_step / bd_repaint_undo)
  DPMSolverMultistepScheduler,            the multistep solvers in lambda, on _LambdaMultistep (bd_dpm_step, bd_unipc_step,
  UniPCMultistepScheduler,                bd_deis_step)
  DEISMultistepScheduler
  HeunDiscreteScheduler,                  the sigma-space samplers, on _SigmaScheduler (bd_sigma_step, bd_scale_input)
  LMSDiscreteScheduler
  EulerDiscreteScheduler,                 the stochastic sigma-space samplers and KDPM2, on _SigmaScheduler too (bd_sigma_step,
  EulerAncestralDiscreteScheduler,        bd_sigma_noise_step)
  KDPM2DiscreteScheduler,
  KDPM2AncestralDiscreteScheduler

_Base holds what they share: the beta tables and their device copies, `from_config` over `_KEYS`, the layout helpers `_align` /
`_fits`, and the opening (`_begin_step`) and closing (`_output`) of a `step`.

Kept surface of DDPM / DDIM: `.betas .alphas .alphas_cumprod .timesteps .config.{num_train_timesteps,
clip_sample (assignable), variance_type, ...} .init_noise_sigma .set_timesteps() .step(...).prev_sample
.add_noise() .previous_timestep() ._get_variance() __len__`.
Tables are built on the host exactly as the reference does (fp32 linspace + fp32 cumprod) and mirrored
once to the device; `step` reads its coefficients from that device table (no per-step host scalar math,
no host<->device sync; scheduling_ddpm.py:350-365 does ~7 host scalar extractions per step).
Only what BadDiffusion exercises is supported: epsilon prediction, linear betas, fixed_small /
fixed_large variance; anything else raises like the reference does for unknown options.
Dynamic thresholding (`thresholding=True`, any `sample_max_value`) runs in DDPM and DDIM: bd_abs_quantile ahead of the step launch (`_x0_quantile`).
DPM-Solver(++) is behind --native_sched, UniPC behind the UNIPC_O*-SCHED names, DEIS behind DEIS_O*-SCHED, Heun and LMS (fractional timesteps, scaled model
input and initial noise) behind HEUN_O2-SCHED and LMSD_O*-SCHED, Euler, Euler-ancestral, KDPM2 and KDPM2-ancestral behind EULER_O1-SCHED,
EULER_A_O1-SCHED, KDPM2_O2-SCHED and KDPM2_A_O2-SCHED.
"""
import numpy as np
import torch

from . import ops
from .unet import FrozenConfig


class SchedulerOutput:
    def __init__(self, prev_sample, pred_original_sample=None):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample


class ShardedGenerator:
    """Rows [lo, hi) of the noise a SINGLE process would draw for a chunk of `full_batch` chains (SURVEY hard-part 4; the reference draws every
    sampling noise from one CPU generator, chunk after chunk: model.py:517-523, scheduling_ddpm.py:400-404).  Handed to a pipeline as its
    `generator`, every randn_tensor(shape, ...) call draws the FULL chunk's tensor ((full_batch,) + shape[1:]) from `gen` -- so the stream
    advances exactly as in the unsharded run, on every rank -- and returns this rank's rows.  The price of reference-order noise on a sharded
    job: every rank draws all of it (host RNG time), which is why it is opt-in (batch_sampling_save(parity=True), BD_SHARDED_NOISE=reference)."""

    def __init__(self, gen, full_batch, lo, hi):
        if gen is None or gen.device.type != "cpu":
            raise ValueError("ShardedGenerator needs a CPU torch.Generator (the reference's sampling stream is a CPU generator)")
        if not (0 <= lo <= hi <= full_batch):
            raise ValueError(f"rows [{lo}, {hi}) outside a chunk of {full_batch}")
        self.gen, self.full_batch, self.lo, self.hi = gen, int(full_batch), int(lo), int(hi)
        self.device = gen.device


def randn_tensor(shape, generator=None, device=None, dtype=torch.float32):
    """utils/torch_utils.py:29-70: with a CPU generator the noise is drawn on the CPU (seed parity with
    the reference) and copied to the device."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    if isinstance(generator, ShardedGenerator):
        if shape[0] != generator.hi - generator.lo:
            raise ValueError(f"ShardedGenerator for rows [{generator.lo}, {generator.hi}) asked for a batch of {shape[0]}")
        full = torch.randn((generator.full_batch,) + tuple(shape[1:]), generator=generator.gen, device="cpu", dtype=dtype)
        return full[generator.lo: generator.hi].contiguous().to(device)
    if generator is not None and generator.device.type == "cpu" and device.type != "cpu":
        return torch.randn(shape, generator=generator, device="cpu", dtype=dtype).to(device)
    return torch.randn(shape, generator=generator, device=device, dtype=dtype)


class _Base:
    order = 1

    @classmethod
    def from_config(cls, config):
        """a scheduler of this class from any scheduler's config (pipeline_ddim.py:39-42, pipeline_pndm.py:46), for the classes that
        name the constructor arguments a config carries over in `_KEYS`"""
        return cls(**{k: config[k] for k in cls._KEYS if k in config})

    def _make_tables(self, num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas):
        if trained_betas is not None:
            self.betas = torch.tensor(trained_betas, dtype=torch.float32)
        elif beta_schedule == "linear":
            self.betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
        elif beta_schedule == "scaled_linear":
            self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        else:
            raise NotImplementedError(f"{beta_schedule} does is not implemented for {self.__class__}")
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.init_noise_sigma = 1.0
        self._dev = {}

    def device_tables(self, device):
        """(alphas, alphas_cumprod) on `device`, uploaded once."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.alphas.to(device), self.alphas_cumprod.to(device))
        return self._dev[key]

    def device_betas(self, device):
        """betas on `device`, uploaded once (the table RePaint's undo_step reads)"""
        key = ("betas", str(device))
        if key not in self._dev:
            self._dev[key] = self.betas.to(device)
        return self._dev[key]

    def scale_model_input(self, sample, timestep=None):
        return sample

    def __len__(self):
        return self.config.num_train_timesteps

    @property
    def num_train_timesteps(self):
        """`noise_sched.num_train_timesteps` (baddiffusion.py:600, anp_defense.py:131): diffusers' config attribute shortcut."""
        return self.config.num_train_timesteps

    def add_noise(self, original_samples, noise, timesteps):
        # scheduling_ddpm.py:422-443  (q_sample with R = 0)
        a, ac = self.device_tables(original_samples.device)
        xn, _ = ops.qsample(original_samples, torch.zeros_like(original_samples), noise, timesteps, a, ac)
        return xn.permute(0, 3, 1, 2)

    @staticmethod
    def _flat(x):
        """dense storage view of a (possibly channels_last) tensor: the step kernels are elementwise, so any
        layout works as long as model_output / sample / noise share it."""
        if x.is_contiguous():
            return x, None
        p = x.permute(0, 2, 3, 1)
        if p.is_contiguous():
            return p, "nhwc"
        return x.contiguous(), None

    def _align(self, *ts):
        """bring all tensors to one common dense layout; returns (tensors, restore_fn)."""
        first, tag = self._flat(ts[0])
        outs = [first]
        for t in ts[1:]:
            if t is None:
                outs.append(None)
            elif tag == "nhwc":
                q = t.permute(0, 2, 3, 1)
                outs.append(q if q.is_contiguous() else q.contiguous())
            else:
                outs.append(t.contiguous())
        restore = (lambda y: y.permute(0, 3, 1, 2)) if tag == "nhwc" else (lambda y: y)
        return outs, restore

    def _x0_quantile(self, eps, x, alphas_cumprod, t):
        """dynamic thresholding (DDPM / DDIM, scheduling_ddpm.py:381-382): per image the raw dynamic_thresholding_ratio quantile of
        |x0|, x0 formed inside the quantile kernel exactly as the step kernel then forms it -- one launch ahead of the step's; None
        when the config has thresholding off.  eps and x are in one of _align's layouts (dimension 0 outermost)."""
        if not self.config.thresholding:
            return None
        return ops.abs_quantile(x, self.config.dynamic_thresholding_ratio, model_output=eps, alphas_cumprod=alphas_cumprod, t=t)

    def _threshold_sample(self, sample):
        """scheduling_ddpm.py:290-322 / scheduling_ddim.py:203-235 on a device tensor [B,C,H,W]: s = the per-image quantile of |sample|
        (bd_abs_quantile) clamped to [1, sample_max_value]; clamp(sample, -s, s) / s.  `step` does not come through here (its clamp
        and division are inside the step kernel); this is the reference's method kept for callers that threshold a tensor of their own."""
        if not sample.is_cuda:
            raise RuntimeError(f"{type(self).__name__}._threshold_sample runs on the GPU only")
        dtype = sample.dtype
        x = sample if dtype == torch.float32 else sample.float()
        (x,), restore = self._align(x)
        s = ops.abs_quantile(x, self.config.dynamic_thresholding_ratio).clamp(min=1, max=self.config.sample_max_value)
        s = s.view(-1, *([1] * (x.dim() - 1)))
        return restore(torch.clamp(x, -s, s) / s).to(dtype)

    @staticmethod
    def _fits(h, x):
        """a stored buffer can stand beside the sample x in one launch: same shape, layout and device"""
        return h is not None and h.shape == x.shape and h.stride() == x.stride() and h.device == x.device

    def _begin_step(self, model_output, sample):
        """What `step` of the multistep and sigma-space schedulers opens with: the four refusals, then (model_output, sample) in one
        dense layout and the function that takes a result back to the caller's."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self.config.prediction_type != "epsilon":
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be `epsilon` on the HIP path")
        if not (model_output.is_cuda and sample.is_cuda):
            raise RuntimeError(f"{type(self).__name__}.step runs on the GPU only")
        (eps, x), restore = self._align(model_output, sample)
        if eps.dtype != torch.float32 or x.dtype != torch.float32:
            raise TypeError(f"{type(self).__name__}.step: float32 tensors only")
        return eps, x, restore

    @staticmethod
    def _output(prev, restore, return_dict, pred_original_sample=None, **more):
        """What `step` closes with: (prev_sample,) or a SchedulerOutput, every tensor back in the caller's layout; `more` become
        further attributes of the output (a None stays None)."""
        back = lambda v: None if v is None else restore(v)       # noqa: E731
        prev = restore(prev)
        if not return_dict:
            return (prev,)
        out = SchedulerOutput(prev_sample=prev, pred_original_sample=back(pred_original_sample))
        for name, v in more.items():
            setattr(out, name, back(v))
        return out


class DDPMScheduler(_Base):
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, variance_type="fixed_small", clip_sample=True, prediction_type="epsilon",
                 thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0,
                 clip_defense=False, clip_defense_range=1.0, **unused):
        self.config = FrozenConfig(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, variance_type=variance_type, clip_sample=clip_sample,
            prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, clip_sample_range=clip_sample_range,
            sample_max_value=sample_max_value, clip_defense=clip_defense, clip_defense_range=clip_defense_range)
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self.custom_timesteps = False
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())
        self.variance_type = variance_type

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        # scheduling_ddpm.py:197-248
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError("Can only pass one of `num_inference_steps` or `custom_timesteps`.")
        if timesteps is not None:
            for i in range(1, len(timesteps)):
                if timesteps[i] >= timesteps[i - 1]:
                    raise ValueError("`custom_timesteps` must be in descending order.")
            if timesteps[0] >= self.config.num_train_timesteps:
                raise ValueError(f"`timesteps` must start before `self.config.train_timesteps`: {self.config.num_train_timesteps}.")
            timesteps = np.array(timesteps, dtype=np.int64)
            self.custom_timesteps = True
        else:
            if num_inference_steps > self.config.num_train_timesteps:
                raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                                 f"`self.config.train_timesteps`: {self.config.num_train_timesteps}")
            self.num_inference_steps = num_inference_steps
            step_ratio = self.config.num_train_timesteps // self.num_inference_steps
            timesteps = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
            self.custom_timesteps = False
        self.timesteps = torch.from_numpy(timesteps).to(device)

    def previous_timestep(self, timestep):
        # scheduling_ddpm.py:468-481
        if self.custom_timesteps:
            index = (self.timesteps == timestep).nonzero(as_tuple=True)[0][0]
            return torch.tensor(-1) if index == self.timesteps.shape[0] - 1 else self.timesteps[index + 1]
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return timestep - self.config.num_train_timesteps // n

    def _get_variance(self, t, predicted_variance=None, variance_type=None):
        # scheduling_ddpm.py:250-288 (host scalar; kept for API parity and the reference's KATs)
        prev_t = self.previous_timestep(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        cur_beta = 1 - a_t / a_prev
        variance = torch.clamp((1 - a_prev) / (1 - a_t) * cur_beta, min=1e-20)
        variance_type = variance_type or self.config.variance_type
        if variance_type == "fixed_small":
            return variance
        if variance_type == "fixed_large":
            return cur_beta
        raise NotImplementedError(f"variance_type {variance_type}: only fixed_small / fixed_large are on the BadDiffusion path")

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None):
        # scheduling_ddpm.py:324-420
        if self.config.prediction_type != "epsilon":
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be `epsilon` on the HIP path")
        if not model_output.is_cuda:
            raise RuntimeError("DDPMScheduler.step runs on the GPU only")
        t = int(timestep)
        prev_t = int(self.previous_timestep(t))
        if t > 0 and noise is None:
            noise = randn_tensor(tuple(model_output.shape), generator=generator, device=model_output.device,
                                 dtype=model_output.dtype)
        (mo, sm, nz), restore = self._align(model_output, sample, noise if t > 0 else None)
        _, ac = self.device_tables(model_output.device)
        prev, x0 = ops.ddpm_step(mo, sm, nz, ac, t, prev_t, self.variance_type, self.config.clip_sample,
                                 self.config.clip_sample_range, self.config.clip_defense, self.config.clip_defense_range,
                                 want_x0=True, x0_quantile=self._x0_quantile(mo, sm, ac, t),
                                 sample_max_value=self.config.sample_max_value)
        return self._output(prev, restore, return_dict, pred_original_sample=x0)


class DDIMScheduler(_Base):
    _KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "clip_sample", "set_alpha_to_one",
             "steps_offset", "prediction_type", "thresholding", "dynamic_thresholding_ratio", "clip_sample_range", "sample_max_value")

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon",
                 thresholding=False, dynamic_thresholding_ratio=0.995, clip_sample_range=1.0, sample_max_value=1.0, **unused):
        self.config = FrozenConfig(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, clip_sample=clip_sample, set_alpha_to_one=set_alpha_to_one,
            steps_offset=steps_offset, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, clip_sample_range=clip_sample_range,
            sample_max_value=sample_max_value)
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps, device=None):
        # scheduling_ddim.py:237-259
        if num_inference_steps > self.config.num_train_timesteps:
            raise ValueError(f"`num_inference_steps`: {num_inference_steps} cannot be larger than "
                             f"`self.config.train_timesteps`: {self.config.num_train_timesteps}")
        self.num_inference_steps = num_inference_steps
        step_ratio = self.config.num_train_timesteps // self.num_inference_steps
        timesteps = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self.timesteps += self.config.steps_offset

    def _get_variance(self, timestep, prev_timestep):
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        return ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        # scheduling_ddim.py:261-381
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self.config.prediction_type != "epsilon":
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be `epsilon` on the HIP path")
        if use_clipped_model_output:
            raise NotImplementedError("use_clipped_model_output is not on the BadDiffusion path")
        if not model_output.is_cuda:
            raise RuntimeError("DDIMScheduler.step runs on the GPU only")
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        if eta > 0:
            if variance_noise is not None and generator is not None:
                raise ValueError("Cannot pass both generator and variance_noise.")
            if variance_noise is None:
                variance_noise = randn_tensor(tuple(model_output.shape), generator=generator, device=model_output.device,
                                              dtype=model_output.dtype)
        (mo, sm, nz), restore = self._align(model_output, sample, variance_noise if eta > 0 else None)
        _, ac = self.device_tables(model_output.device)
        prev, x0 = ops.ddim_step(mo, sm, ac, t, prev_t, eta=float(eta), noise=nz, clip_sample=self.config.clip_sample,
                                 clip_sample_range=self.config.clip_sample_range,
                                 final_alpha_cumprod=float(self.final_alpha_cumprod), want_x0=True,
                                 x0_quantile=self._x0_quantile(mo, sm, ac, t), sample_max_value=self.config.sample_max_value)
        return self._output(prev, restore, return_dict, pred_original_sample=x0)


class PNDMScheduler(_Base):
    """Pseudo numerical method scheduler (scheduling_pndm.py:60-426) on the GPU: 12 Runge-Kutta warm-up evaluations, then a
    4-step Adams-Bashforth tail, every update being `sample_coeff * x + eps_coeff * (combination of stored model outputs)`
    with formula (9) of the PNDM paper for the two scalars -- one fused `bd_lincomb` launch per update (plus one for the
    Runge-Kutta accumulator), coefficients computed on the host in fp32 like the reference's scalar tensor arithmetic.
    This is the scheduler every `--sched` other than DDPM / DDIM ends up as: PNDMPipeline re-creates it from whatever
    scheduler config it is given (pipeline_pndm.py:46).  `step(..., clip=r)` folds the pipeline's post-step clamp in."""
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon", steps_offset=0, **unused):
        self.config = FrozenConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                   beta_schedule=beta_schedule, trained_betas=trained_betas, skip_prk_steps=skip_prk_steps,
                                   set_alpha_to_one=set_alpha_to_one, prediction_type=prediction_type, steps_offset=steps_offset)
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.pndm_order = 4
        self.num_inference_steps = None
        self.prk_timesteps = self.plms_timesteps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))
        self._reset()

    _KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "skip_prk_steps",
             "set_alpha_to_one", "prediction_type", "steps_offset")

    def _reset(self):
        self.counter, self.ets, self.cur_sample, self._acc = 0, [], None, None

    def set_timesteps(self, num_inference_steps, device=None):
        # scheduling_pndm.py:150-190
        self.num_inference_steps = num_inference_steps
        ratio = self.config.num_train_timesteps // num_inference_steps
        base = (np.arange(0, num_inference_steps) * ratio).round() + self.config.steps_offset
        if self.config.skip_prk_steps:
            self.prk_timesteps = np.array([])
            self.plms_timesteps = np.concatenate([base[:-1], base[-2:-1], base[-1:]])[::-1].copy()
        else:
            stages = np.array(base[-self.pndm_order:]).repeat(2) + np.tile(np.array([0, ratio // 2]), self.pndm_order)
            self.prk_timesteps = (stages[:-1].repeat(2)[1:-1])[::-1].copy()
            self.plms_timesteps = base[:-3][::-1].copy()
        self.timesteps = torch.from_numpy(np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64)).to(device)
        self._reset()

    def _coeffs(self, t, prev_t):
        """(sample_coeff, eps_coeff) of formula (9) as fp32 scalars (scheduling_pndm.py:366-397)"""
        a_t = self.alphas_cumprod[t]
        a_p = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t, b_p = 1 - a_t, 1 - a_p
        denom = a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5
        return float((a_p / a_t) ** 0.5), float(-(a_p - a_t) / denom)

    def step(self, model_output, timestep, sample, return_dict=True, clip=None):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self.config.prediction_type != "epsilon":
            raise ValueError(f"prediction_type given as {self.config.prediction_type} must be `epsilon` on the HIP path")
        if not model_output.is_cuda:
            raise RuntimeError("PNDMScheduler.step runs on the GPU only")
        (eps, x), restore = self._align(model_output, sample)
        t = int(timestep)
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        if self.counter < len(self.prk_timesteps) and not self.config.skip_prk_steps:
            # Runge-Kutta stage r of the current transition: weights 1/6, 1/3, 1/3, 1/6
            r = self.counter % 4
            prev_t = t - (0 if self.counter % 2 else ratio // 2)
            t0 = int(self.prk_timesteps[self.counter // 4 * 4])
            sc, ec = self._coeffs(t0, prev_t)
            if r == 0:
                self._acc = ops.lincomb([eps], [1.0 / 6.0])
                self.ets.append(eps)
                self.cur_sample = x
            base = self.cur_sample if self.cur_sample is not None else x
            if r in (1, 2):
                self._acc = ops.lincomb([self._acc, eps], [1.0, 1.0 / 3.0])
            if r == 3:
                prev = ops.lincomb([base, self._acc, eps], [sc, ec, ec / 6.0], clip=clip)
                self._acc = None
            else:
                prev = ops.lincomb([base, eps], [sc, ec], clip=clip)
        else:
            # linear multistep (Adams-Bashforth) on the stored model outputs
            if not self.config.skip_prk_steps and len(self.ets) < 3:
                raise ValueError(f"{self.__class__} can only be run AFTER scheduler has been run in 'prk' mode for at least 12 "
                                 "iterations See: https://github.com/huggingface/diffusers/blob/main/src/diffusers/pipelines/"
                                 "pipeline_pndm.py for more information.")
            prev_t = t - ratio
            if self.counter != 1:
                self.ets = self.ets[-3:] + [eps]
            else:
                prev_t, t = t, t + ratio
            k = len(self.ets)
            if k == 1 and self.counter == 0:
                terms, w = [eps], [1.0]
                self.cur_sample = x
            elif k == 1 and self.counter == 1:
                terms, w = [eps, self.ets[-1]], [0.5, 0.5]
                x, self.cur_sample = self.cur_sample, None
            elif k == 2:
                terms, w = [self.ets[-1], self.ets[-2]], [1.5, -0.5]
            elif k == 3:
                terms, w = [self.ets[-1], self.ets[-2], self.ets[-3]], [23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0]
            else:
                terms, w = [self.ets[-1], self.ets[-2], self.ets[-3], self.ets[-4]], [55.0 / 24.0, -59.0 / 24.0, 37.0 / 24.0, -9.0 / 24.0]
            sc, ec = self._coeffs(t, prev_t)
            prev = ops.lincomb([x] + terms, [sc] + [ec * wi for wi in w], clip=clip)
        self.counter += 1
        return self._output(prev, restore, return_dict)


class RePaintSchedulerOutput(SchedulerOutput):
    pass


class RePaintScheduler(_Base):
    """RePaint inpainting scheduler (scheduling_repaint.py:75-329) on the GPU, epsilon prediction: the reverse step is the DDIM update
    blended by the mask with a re-noised copy of the original image (one `bd_repaint_step` launch), and `undo_step` is the forward
    recurrence of num_train_timesteps // num_inference_steps noising sub-steps that takes the chain back up ("time travel",
    `bd_repaint_undo`).  Noise is drawn on EVERY step, eta == 0 and t == 0 included, and once per sub-step, in the reference's order.
    `.eta` is an attribute the pipeline assigns (the reference reads self.eta, not a step argument).

    `shift=` (not in the reference) is the trigger-consistent variant: with shift = R, the BadDiffusion trigger image, the known region
    and the undo sub-steps follow the poisoned forward process x_t = sqrt(a) x0 + sqrt(1-a) eps + (1 - sqrt(a)) R (loss.py:275), for
    which x_t - R is a plain chain.  shift=None is exactly the reference."""
    order = 1
    _KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "eta", "trained_betas", "clip_sample")

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", eta=0.0, trained_betas=None,
                 clip_sample=True, **unused):
        self.config = FrozenConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                   beta_schedule=beta_schedule, eta=eta, trained_betas=trained_betas, clip_sample=clip_sample)
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())
        self.eta = eta

    def set_timesteps(self, num_inference_steps, jump_length=10, jump_n_sample=10, device=None):
        # scheduling_repaint.py:167-195
        num_inference_steps = min(self.config.num_train_timesteps, num_inference_steps)
        self.num_inference_steps = num_inference_steps
        timesteps = []
        jumps = {}
        for j in range(0, num_inference_steps - jump_length, jump_length):
            jumps[j] = jump_n_sample - 1
        t = num_inference_steps
        while t >= 1:
            t = t - 1
            timesteps.append(t)
            if jumps.get(t, 0) > 0:
                jumps[t] = jumps[t] - 1
                for _ in range(jump_length):
                    t = t + 1
                    timesteps.append(t)
        timesteps = np.array(timesteps) * (self.config.num_train_timesteps // self.num_inference_steps)
        self.timesteps = torch.from_numpy(timesteps).to(device)

    def _ratio(self):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        return self.config.num_train_timesteps // self.num_inference_steps

    def _get_variance(self, t):
        # scheduling_repaint.py:197-214 (host scalar, kept for API parity)
        prev_timestep = t - self._ratio()
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        return ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)

    def step(self, model_output, timestep, sample, original_image, mask, generator=None, return_dict=True, noise=None, shift=None):
        # scheduling_repaint.py:216-301
        if not (model_output.is_cuda and sample.is_cuda):
            raise RuntimeError("RePaintScheduler.step runs on the GPU only")
        t = int(timestep)
        prev_t = t - self._ratio()
        if noise is None:
            noise = randn_tensor(tuple(model_output.shape), generator=generator, device=model_output.device, dtype=model_output.dtype)
        dev = model_output.device
        _, ac = self.device_tables(dev)
        prev, x0 = ops.repaint_step(model_output, sample, noise, original_image.to(dev), mask.to(dev), ac, t, prev_t, eta=float(self.eta),
                                    clip_sample=self.config.clip_sample, clip_sample_range=1.0,
                                    final_alpha_cumprod=float(self.final_alpha_cumprod), shift=None if shift is None else shift.to(dev),
                                    want_x0=True)
        if not return_dict:
            return (prev, x0)
        return RePaintSchedulerOutput(prev_sample=prev, pred_original_sample=x0)

    def undo_step(self, sample, timestep, generator=None, noise=None, shift=None):
        # scheduling_repaint.py:303-318
        if not sample.is_cuda:
            raise RuntimeError("RePaintScheduler.undo_step runs on the GPU only")
        n = self._ratio()
        if noise is None:
            noise = [randn_tensor(tuple(sample.shape), generator=generator, device=sample.device, dtype=sample.dtype) for _ in range(n)]
        elif len(noise) != n:
            raise ValueError(f"undo_step: {n} noise tensors expected (num_train_timesteps // num_inference_steps), got {len(noise)}")
        return ops.repaint_undo(sample, list(noise), self.device_betas(sample.device), int(timestep),
                                shift=None if shift is None else shift.to(sample.device))

    def add_noise(self, original_samples, noise, timesteps):
        raise NotImplementedError("Use `DDPMScheduler.add_noise()` to train for sampling with RePaint.")


class _LambdaMultistep(_Base):
    """What the three multistep solvers in lambda = log(alpha / sigma) share (DPM-Solver(++), UniPC, DEIS):
    the alpha_t / sigma_t / lambda_t tables, the timesteps and the position of one by value, the per-chain cache of the host scalars
    of a step, the thresholding rule and the warm-up counter.  A subclass has `_plan_scalars`, the key of its cache entries, its ring
    of device buffers (`_reset`; `_history` serves the two that keep `solver_order` converted outputs) and the body of `step`."""

    def _refuse_thresholding(self, thresholding, sample_max_value):
        if thresholding and sample_max_value != 1.0:
            raise NotImplementedError(f"{type(self).__name__}: thresholding is on the HIP path for sample_max_value == 1.0 only "
                                      f"(where it is clamp(x0, -1, 1)), got {sample_max_value}")

    def _make_lambda_tables(self, num_train_timesteps):
        self.alpha_t = torch.sqrt(self.alphas_cumprod)          # scheduling_dpmsolver_multistep.py:162-164, scheduling_unipc_multistep.py:161-164
        self.sigma_t = torch.sqrt(1 - self.alphas_cumprod)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self._ts, self._index, self._plans = [], {}, {}
        self._reset()

    def set_timesteps(self, num_inference_steps, device=None):
        # scheduling_dpmsolver_multistep.py:200-226, scheduling_unipc_multistep.py:188-220
        timesteps = np.linspace(0, self.config.num_train_timesteps - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
        _, unique_indices = np.unique(timesteps, return_index=True)     # num_inference_steps == num_train_timesteps has duplicates
        timesteps = timesteps[np.sort(unique_indices)]
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self.num_inference_steps = len(timesteps)
        ts = [int(t) for t in timesteps]
        if ts != self._ts:
            self._ts, self._index, self._plans = ts, {t: i for i, t in enumerate(ts)}, {}
        self._reset()

    def _step_index(self, timestep):
        # by value; a timestep that is not in the table counts as the last one
        return self._index.get(int(timestep), len(self._index) - 1)

    def _cached_plan(self, key, *args):
        """_plan_scalars(*args), computed once per set of timesteps and `key`: the scalars depend on the tables, the timesteps, the
        position and the warm-up state alone, so a second chain of the same length (sampling runs chunk after chunk) spends no host
        time on ~40 scalar tensor operations per step"""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if key not in self._plans:
            self._plans[key] = self._plan_scalars(*args)
        return self._plans[key]

    def _history(self, order, x):
        """(m1, m2, oldest) of a step of `order` on the sample x, for the solvers whose ring holds `solver_order` converted outputs, oldest
        first: the buffers the update reads, which must fit x, and the one that takes this step's converted output -- the oldest of
        the ring (also while it is read as m2), or None for a first order solver, which never reads it back"""
        ring = self._ring
        for h in ring[len(ring) - order + 1:] if order > 1 else ():
            if not self._fits(h, x):
                raise ValueError(f"{type(self).__name__}.step: the stored model outputs do not have this sample's shape and layout "
                                 "(one chain per set_timesteps)")
        oldest = None
        if len(ring) > 1:
            oldest = ring[0] if self._fits(ring[0], x) else torch.empty_like(x)
        return (ring[-1] if order >= 2 else None), (ring[-2] if order >= 3 else None), oldest

    def _advance(self, written=None):
        """the bookkeeping of one step: the buffer of `_history` that the step wrote becomes the newest, the warm-up counter moves"""
        if written is not None:
            self._ring = self._ring[1:] + [written]
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1


class DPMSolverMultistepScheduler(_LambdaMultistep):
    """DPM-Solver / DPM-Solver++ multistep scheduler (scheduling_dpmsolver_multistep.py:127-573) on the GPU, epsilon prediction: a
    deterministic ODE sampler of order 1-3 that is normally run at 10-20 UNet evaluations.  Every step is ONE `bd_dpm_step` launch: the
    conversion of the model output (x0-prediction, optionally clamped, for dpmsolver++; eps for dpmsolver), the update and the
    pipeline's post-step clamp (`step(..., clip=r)`, as PNDMScheduler).  All scalar work is done on the host in fp32 torch scalars as
    the reference does it, with D1 / D2 of the second and third order updates expanded into the coefficients of the stored converted
    outputs m0, m1, m2 (`_plan`, no device access).  The history is a ring of `solver_order` device buffers; a step writes its m0 into
    the oldest.  `thresholding=True` is supported for sample_max_value == 1.0, where the reference's dynamic thresholding is exactly
    clamp(x0, -1, 1) (s is clamped to [1, 1], :250-256); Karras sigmas are not."""
    order = 1
    _KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "solver_order", "prediction_type",
             "thresholding", "dynamic_thresholding_ratio", "sample_max_value", "algorithm_type", "solver_type", "lower_order_final",
             "use_karras_sigmas")

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                 algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True, use_karras_sigmas=False, **unused):
        # scheduling_dpmsolver_multistep.py:170-180: a DEIS / UniPC config converts
        if algorithm_type not in ("dpmsolver", "dpmsolver++"):
            if algorithm_type != "deis":
                raise NotImplementedError(f"{algorithm_type} does is not implemented for {self.__class__}")
            algorithm_type = "dpmsolver++"
        if solver_type not in ("midpoint", "heun"):
            if solver_type not in ("logrho", "bh1", "bh2"):
                raise NotImplementedError(f"{solver_type} does is not implemented for {self.__class__}")
            solver_type = "midpoint"
        if solver_order not in (1, 2, 3):
            raise ValueError(f"solver_order must be 1, 2 or 3, got {solver_order}")
        if use_karras_sigmas:
            raise NotImplementedError("DPMSolverMultistepScheduler: use_karras_sigmas is not on the HIP path")
        self._refuse_thresholding(thresholding, sample_max_value)
        self.config = FrozenConfig(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value, algorithm_type=algorithm_type,
            solver_type=solver_type, lower_order_final=lower_order_final, use_karras_sigmas=False)
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self._make_lambda_tables(num_train_timesteps)

    def _reset(self):
        self.lower_order_nums = 0
        self._ring = [None] * self.config.solver_order      # converted model outputs, oldest first; [-1] is the previous step's

    def _plan(self, step_index):
        """Host part of the step at `step_index` given the current `lower_order_nums`: (order_used, alpha_s, sigma_s, cx, c0, c1, c2)
        with  m0 = (sample - sigma_s eps) / alpha_s  (dpmsolver++; m0 = eps for dpmsolver)  and
        prev = cx sample + c0 m0 + c1 m1 + c2 m2  (:383-505, D1 and D2 expanded).  fp32 torch scalars throughout, no device access."""
        cfg = self.config
        key = (step_index, self.lower_order_nums, cfg.algorithm_type, cfg.solver_type, cfg.solver_order, cfg.lower_order_final)
        return self._cached_plan(key, step_index)

    def _plan_scalars(self, step_index):
        ts, n, cfg = self._ts, len(self._ts), self.config
        last = step_index == n - 1
        prev_t = 0 if last else int(ts[step_index + 1])
        final = last and cfg.lower_order_final and n < 15
        second = step_index == n - 2 and cfg.lower_order_final and n < 15
        if cfg.solver_order == 1 or self.lower_order_nums < 1 or final:
            order = 1
        elif cfg.solver_order == 2 or self.lower_order_nums < 2 or second:
            order = 2
        else:
            order = 3
        s0 = int(ts[step_index])
        lam_t, lam_s0 = self.lambda_t[prev_t], self.lambda_t[s0]
        alpha_t, alpha_s0 = self.alpha_t[prev_t], self.alpha_t[s0]
        sigma_t, sigma_s0 = self.sigma_t[prev_t], self.sigma_t[s0]
        h = lam_t - lam_s0
        pp = cfg.algorithm_type == "dpmsolver++"
        if pp:
            cx, a0 = sigma_t / sigma_s0, -(alpha_t * (torch.exp(-h) - 1.0))
        else:
            cx, a0 = alpha_t / alpha_s0, -(sigma_t * (torch.exp(h) - 1.0))
        zero = torch.zeros(())
        if order == 1:
            c0, c1, c2 = a0, zero, zero
        elif order == 2:
            r0 = (lam_s0 - self.lambda_t[int(ts[step_index - 1])]) / h
            if cfg.solver_type == "midpoint":
                a1 = 0.5 * a0
            elif pp:
                a1 = alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)
            else:
                a1 = -(sigma_t * ((torch.exp(h) - 1.0) / h - 1.0))
            # D1 = (m0 - m1) / r0
            c0, c1, c2 = a0 + a1 / r0, -(a1 / r0), zero
        else:
            lam_s1, lam_s2 = self.lambda_t[int(ts[step_index - 1])], self.lambda_t[int(ts[step_index - 2])]
            r0, r1 = (lam_s0 - lam_s1) / h, (lam_s1 - lam_s2) / h
            if pp:
                a1 = alpha_t * ((torch.exp(-h) - 1.0) / h + 1.0)
                a2 = -(alpha_t * ((torch.exp(-h) - 1.0 + h) / h ** 2 - 0.5))
            else:
                a1 = -(sigma_t * ((torch.exp(h) - 1.0) / h - 1.0))
                a2 = -(sigma_t * ((torch.exp(h) - 1.0 - h) / h ** 2 - 0.5))
            # D1_0 = (m0 - m1) / r0, D1_1 = (m1 - m2) / r1, D1 = D1_0 + k (D1_0 - D1_1), D2 = q (D1_0 - D1_1)
            k, q = r0 / (r0 + r1), 1.0 / (r0 + r1)
            u, v = a1 * (1.0 + k) + a2 * q, -(a1 * k) - a2 * q          # coefficients of D1_0 and D1_1
            c0, c1, c2 = a0 + u / r0, v / r1 - u / r0, -(v / r1)
        return order, float(alpha_s0), float(sigma_s0), float(cx), float(c0), float(c1), float(c2)

    def step(self, model_output, timestep, sample, return_dict=True, clip=None):
        # scheduling_dpmsolver_multistep.py:529-573
        eps, x, restore = self._begin_step(model_output, sample)
        order, alpha_s, sigma_s, cx, c0, c1, c2 = self._plan(self._step_index(timestep))
        m1, m2, oldest = self._history(order, x)
        pp = self.config.algorithm_type == "dpmsolver++"
        prev = ops.dpm_step(eps, x, cx, c0, m1=m1, c1=c1, m2=m2, c2=c2, convert=(alpha_s, sigma_s) if pp else None,
                            x0_clip=1.0 if pp and self.config.thresholding else None, clip=clip, m0_out=oldest)
        self._advance(oldest)
        return self._output(prev, restore, return_dict)


class UniPCMultistepScheduler(_LambdaMultistep):
    """UniPC multistep scheduler (scheduling_unipc_multistep.py:126-601, B(h) version) on the GPU, epsilon prediction: a predictor
    (UniP) of order 1-3 plus a corrector (UniC) that reuses the model output of the current step, so every step gains one order of
    accuracy at no extra UNet evaluation.  Every step is ONE `bd_unipc_step` launch: conversion of the model output, the corrector
    over the history as it stood before the step, the predictor from the corrected sample, and the pipeline's post-step clamp
    (`step(..., clip=r)`).  All scalar work is done on the host in fp32 torch scalars as the reference does it (the order-3 linear
    solves included), with the D1 differences and the rho weights of both updates expanded into coefficients of the tensors (`_plan`,
    no device access).  State: a ring of `solver_order` device buffers of converted outputs (a step writes its own into the oldest),
    their timesteps, and `last_sample`, the corrected sample of the previous step (on a step without a corrector that is the
    incoming sample itself, which is kept by reference as the reference does; the scheduler never steps in place).
    `thresholding=True` is supported for sample_max_value == 1.0, where it is exactly clamp(x0, -1, 1) (as
    DPMSolverMultistepScheduler); `solver_p` and orders above 3 are not."""
    order = 1
    _KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "solver_order", "prediction_type",
             "thresholding", "dynamic_thresholding_ratio", "sample_max_value", "predict_x0", "solver_type", "lower_order_final",
             "disable_corrector")

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                 predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=(), solver_p=None, **unused):
        if solver_type not in ("bh1", "bh2"):                                       # scheduling_unipc_multistep.py:169-173
            if solver_type not in ("midpoint", "heun", "logrho"):
                raise NotImplementedError(f"{solver_type} does is not implemented for {self.__class__}")
            solver_type = "bh1"
        if solver_order < 1:
            raise ValueError(f"solver_order must be at least 1, got {solver_order}")
        if solver_order > 3:
            raise NotImplementedError(f"UniPCMultistepScheduler: solver_order {solver_order} is not on the HIP path (one launch carries "
                                      "three history tensors: orders 1-3)")
        if solver_p is not None:
            raise NotImplementedError("UniPCMultistepScheduler: solver_p is not on the HIP path (the predictor is UniP)")
        self._refuse_thresholding(thresholding, sample_max_value)
        self.config = FrozenConfig(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value, predict_x0=predict_x0,
            solver_type=solver_type, lower_order_final=lower_order_final, disable_corrector=list(disable_corrector))
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self._make_lambda_tables(num_train_timesteps)

    @classmethod
    def from_config(cls, config):
        if "solver_p" in config and config["solver_p"] is not None:
            raise NotImplementedError("UniPCMultistepScheduler: solver_p is not on the HIP path (the predictor is UniP)")
        return super().from_config(config)

    @property
    def predict_x0(self):
        return self.config.predict_x0

    @property
    def disable_corrector(self):
        return self.config.disable_corrector

    def _reset(self):
        self.lower_order_nums = 0
        self.this_order = 0                                   # order of the last predictor = order of the next corrector
        self._ring = [None] * self.config.solver_order        # converted model outputs, oldest first; [-1] is the previous step's
        self._ring_ts = [None] * self.config.solver_order     # and the timesteps they were taken at
        self.last_sample, self._last_owned = None, False

    def _plan(self, step_index, has_last=None):
        """Host part of the step at `step_index` given the current state (`lower_order_nums`, `this_order`, the timesteps of the
        ring): (order, corrector_order, alpha_s, sigma_s, (kl, k0, k1, k2, k3), (px, p0, p1, p2)) for bd_unipc_step's formula
        (include/bd_hip.h).  corrector_order is 0 when the step has no corrector: step 0, a step after one listed in
        `disable_corrector`, or no `last_sample` (has_last, by default whether one is stored).  fp32 torch scalars throughout, no
        device access; kept per set of timesteps, as DPMSolverMultistepScheduler._plan."""
        cfg = self.config
        if has_last is None:
            has_last = self.last_sample is not None
        corrector = step_index > 0 and step_index - 1 not in cfg.disable_corrector and bool(has_last)      # :555-557
        key = (step_index, self.lower_order_nums, self.this_order if corrector else 0, tuple(self._ring_ts), cfg.predict_x0,
               cfg.solver_type, cfg.solver_order, cfg.lower_order_final)
        return self._cached_plan(key, step_index, corrector)

    def _bh(self, s0, t, older, order):
        """what both updates share (:340-383 = :444-487) for the transition s0 -> t of order `order` over the timesteps `older` of the
        history entries behind s0, newest first: (cx, A, B_h, h_phi_1, rks, R, b)"""
        cfg, lam = self.config, self.lambda_t
        h = lam[t] - lam[s0]
        rks = [(lam[si] - lam[s0]) / h for si in older[:order - 1]]
        rks_all = torch.stack(rks + [torch.ones(())])
        hh = -h if cfg.predict_x0 else h
        h_phi_1 = torch.expm1(hh)
        h_phi_k = h_phi_1 / hh - 1
        factorial_i = 1
        if cfg.solver_type == "bh1":
            B_h = hh
        elif cfg.solver_type == "bh2":
            B_h = torch.expm1(hh)
        else:
            raise NotImplementedError()
        R, b = [], []
        for i in range(1, order + 1):
            R.append(torch.pow(rks_all, i - 1))
            b.append(h_phi_k * factorial_i / B_h)
            factorial_i *= i + 1
            h_phi_k = h_phi_k / hh - 1 / factorial_i
        if cfg.predict_x0:
            cx, A = self.sigma_t[t] / self.sigma_t[s0], self.alpha_t[t]
        else:
            cx, A = self.alpha_t[t] / self.alpha_t[s0], self.sigma_t[t]
        return cx, A, B_h, h_phi_1, rks, torch.stack(R), torch.stack(b)

    def _plan_scalars(self, step_index, corrector):
        ts, n, cfg = self._ts, len(self._ts), self.config
        t_now = int(ts[step_index])
        zero = torch.zeros(())
        # corrector (UniC, :413-517) on the lists BEFORE this step's shift: from the previous step's timestep to this one, at the order
        # the previous predictor used.  x_t = cx l - A h_phi_1 h1 - A B (sum_j rho_j (h_{j+1} - h1) / rk_j + rho_p (m0 - h1))
        kl, k = zero, [zero] * 4
        corr_order = self.this_order if corrector else 0
        if corr_order:
            older = [tt for tt in self._ring_ts[::-1]]                   # newest first: [0] is s0
            cx, A, B_h, h_phi_1, rks, R, b = self._bh(older[0], t_now, older[1:], corr_order)
            rhos = torch.tensor([0.5]) if corr_order == 1 else torch.linalg.solve(R, b)
            kl = cx
            k[0] = -(A * B_h) * rhos[-1]
            for j, rk in enumerate(rks):
                k[j + 2] = -(A * B_h) * rhos[j] / rk
            k[1] = -(A * h_phi_1) - k[0] - sum(k[2:], zero)
        # predictor (UniP, :308-411) AFTER the shift: from this step's timestep to the next one (0 at the end)
        prev_t = 0 if step_index == n - 1 else int(ts[step_index + 1])
        order = min(cfg.solver_order, n - step_index) if cfg.lower_order_final else cfg.solver_order      # :579-584
        order = min(order, self.lower_order_nums + 1)
        assert order > 0
        cx, A, B_h, h_phi_1, rks, R, b = self._bh(t_now, prev_t, self._ring_ts[::-1], order)
        p = [zero] * 3
        if order > 1:
            rhos = torch.tensor([0.5]) if order == 2 else torch.linalg.solve(R[:-1, :-1], b[:-1])
            for j, rk in enumerate(rks):
                p[j + 1] = -(A * B_h) * rhos[j] / rk
        p[0] = -(A * h_phi_1) - sum(p[1:], zero)
        return (order, corr_order, float(self.alpha_t[t_now]), float(self.sigma_t[t_now]), (float(kl),) + tuple(float(v) for v in k),
                (float(cx),) + tuple(float(v) for v in p))

    def _advance(self, step_index, order):
        """the bookkeeping of one step: the ring's timesteps shift, the predictor's order is remembered for the next corrector"""
        self._ring_ts = self._ring_ts[1:] + [int(self._ts[step_index])]
        self.this_order = order
        super()._advance()

    def step(self, model_output, timestep, sample, return_dict=True, clip=None):
        # scheduling_unipc_multistep.py:519-601
        eps, x, restore = self._begin_step(model_output, sample)
        step_index = self._step_index(timestep)
        order, corr_order, alpha_s, sigma_s, k, p = self._plan(step_index)
        ring = self._ring
        n_hist = max(corr_order, order - 1)                  # the corrector reads h1..h_p, the predictor h1..h_{p-1}
        hist = [ring[-1 - j] if j < n_hist else None for j in range(3)]
        for h in hist[:n_hist] + ([self.last_sample] if corr_order else []):
            if not self._fits(h, x):
                raise ValueError("UniPCMultistepScheduler.step: the stored model outputs / last sample do not have this sample's "
                                 "shape and layout (one chain per set_timesteps)")
        oldest = ring[0] if self._fits(ring[0], x) else torch.empty_like(x)       # takes this step's converted output
        corrected = None
        if corr_order:
            corrected = self.last_sample if self._last_owned else torch.empty_like(x)
        pp = bool(self.config.predict_x0)
        prev = ops.unipc_step(eps, x, p[0], p[1], h1=hist[0], p1=p[2], h2=hist[1], p2=p[3], h3=hist[2],
                              last_sample=self.last_sample if corr_order else None, kl=k[0], k0=k[1], k1=k[2], k2=k[3], k3=k[4],
                              convert=(alpha_s, sigma_s) if pp else None, x0_clip=1.0 if pp and self.config.thresholding else None,
                              clip=clip, m0_out=oldest, corrected_out=corrected)
        self._ring = ring[1:] + [oldest]
        # the sample the predictor started from: the corrected one, or the incoming one where no corrector ran
        self.last_sample, self._last_owned = (corrected, True) if corr_order else (x, False)
        self._advance(step_index, order)
        return self._output(prev, restore, return_dict)


class DEISMultistepScheduler(_LambdaMultistep):
    """DEIS multistep scheduler (scheduling_deis_multistep.py:61-473, log-rho version) on the GPU, epsilon prediction: an exponential
    integrator of order 1-3 whose coefficients are the integrals of the Lagrange basis polynomials in log(rho), rho = sigma / alpha,
    normally run at 10-20 UNet evaluations.  Every step is ONE `bd_deis_step` launch: the conversion of the model output (to the
    x0-prediction, optionally clamped, and back to an eps prediction, :255-274), the update (:303, :345, :401) and the pipeline's
    post-step clamp (`step(..., clip=r)`, as PNDMScheduler).  All scalar work is done on the host (`_plan`, no device access, kept
    per set of timesteps).  The history is a ring of `solver_order` device buffers; a step writes its converted output into the
    oldest.  `thresholding=True` is supported for sample_max_value == 1.0, where the reference's dynamic thresholding is exactly
    clamp(x0, -1, 1); a DPM-Solver / UniPC config converts as in the reference (:155-165).

    `coefficient_dtype` (this project's own, kept in the config) is the arithmetic of the host scalars:
      "float32" (default)  the reference's: fp32 torch scalars, np.log on them, its order of operations.  Parity is the contract.
      "float64"            the same expressions in float64 from the fp32 tables, rounded once to fp32.
    The reference's coefficients are differences ind_fn(rho_t, ..) - ind_fn(rho_s0, ..) of nearly equal numbers, and in fp32 they
    cancel.  Worst distance over a stand-in chain (tests/golden/make_golden_deis.py) from the same recurrence run in float64 on the
    same fp32 tables, max |x| 16-39:

      order  steps            reference (= "float32")            float64 coefficients, fp32 data
      1      4 / 10 / 20 / 999  2.1e-5 / 1.5e-5 / 9.2e-6 / 5.6e-5  4.2e-5 / 1.9e-5 / 8.9e-6 / 5.4e-5
      2      4 / 10 / 20        3.2e-5 / 1.9e-5 / 1.7e-5           2.3e-5 / 3.3e-5 / 7.9e-6
      2      999                5.3e-3                             5.3e-5
      3      10 / 20            9.7e-5 / 1.5e-4                    3.7e-5 / 1.3e-5
      3      999                4.04                               4.7e-5

    At the step counts DEIS is meant for the two agree; at 999 steps and order 3 the reference is off by a fifth of the signal, and
    "float64" is the way out of it."""
    order = 1
    _KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "solver_order", "prediction_type",
             "thresholding", "dynamic_thresholding_ratio", "sample_max_value", "algorithm_type", "solver_type", "lower_order_final",
             "coefficient_dtype")

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                 solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0,
                 algorithm_type="deis", solver_type="logrho", lower_order_final=True, coefficient_dtype="float32", **unused):
        if algorithm_type != "deis":                                                    # scheduling_deis_multistep.py:155-165
            if algorithm_type not in ("dpmsolver", "dpmsolver++"):
                raise NotImplementedError(f"{algorithm_type} does is not implemented for {self.__class__}")
            algorithm_type = "deis"
        if solver_type != "logrho":
            if solver_type not in ("midpoint", "heun", "bh1", "bh2"):
                raise NotImplementedError(f"solver type {solver_type} does is not implemented for {self.__class__}")
            solver_type = "logrho"
        if solver_order not in (1, 2, 3):
            raise ValueError(f"solver_order must be 1, 2 or 3, got {solver_order}")
        if coefficient_dtype not in ("float32", "float64"):
            raise ValueError(f"coefficient_dtype must be 'float32' (the reference's arithmetic) or 'float64', got {coefficient_dtype!r}")
        self._refuse_thresholding(thresholding, sample_max_value)
        self.config = FrozenConfig(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value, algorithm_type=algorithm_type,
            solver_type=solver_type, lower_order_final=lower_order_final, coefficient_dtype=coefficient_dtype)
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self._make_lambda_tables(num_train_timesteps)

    def _reset(self):
        self.lower_order_nums = 0
        self._ring = [None] * self.config.solver_order      # converted model outputs, oldest first; [-1] is the previous step's

    def _plan(self, step_index):
        """Host part of the step at `step_index` given the current `lower_order_nums`: (order_used, alpha_s, sigma_s, cx, c0, alpha_t,
        k0, k1, k2) for bd_deis_step's formula (include/bd_hip.h); the scalars of the branch not taken are 0.  No device access."""
        cfg = self.config
        key = (step_index, self.lower_order_nums, cfg.solver_order, cfg.lower_order_final, cfg.coefficient_dtype)
        return self._cached_plan(key, step_index)

    @staticmethod
    def _log(v):
        """numpy's log of a 0-dim tensor, in its dtype, as a tensor: what np.log(tensor) gives the reference"""
        return torch.as_tensor(np.log(v.numpy()))

    @classmethod
    def _ind2(cls, t, b, c):
        """the integral of (log t - log c) / (log b - log c) (:338-340), in the reference's order of operations"""
        lt, lb, lc = cls._log(t), cls._log(b), cls._log(c)
        return t * (-lc + lt - 1) / (lb - lc)

    @classmethod
    def _ind3(cls, t, b, c, d):
        """the integral of (log t - log c)(log t - log d) / ((log b - log c)(log b - log d)) (:384-395), likewise"""
        lt, lb, lc, ld = cls._log(t), cls._log(b), cls._log(c), cls._log(d)
        numerator = t * (lc * (ld - lt + 1) - ld * lt + ld + lt ** 2 - 2 * lt + 2)
        return numerator / ((lb - lc) * (lb - ld))

    def _plan_scalars(self, step_index):
        ts, n, cfg = self._ts, len(self._ts), self.config
        last = step_index == n - 1
        prev_t = 0 if last else int(ts[step_index + 1])
        final = last and cfg.lower_order_final and n < 15                                   # :442-447
        second = step_index == n - 2 and cfg.lower_order_final and n < 15
        if cfg.solver_order == 1 or self.lower_order_nums < 1 or final:
            order = 1
        elif cfg.solver_order == 2 or self.lower_order_nums < 2 or second:
            order = 2
        else:
            order = 3
        wide = cfg.coefficient_dtype == "float64"
        # fp32 0-dim tensors as the reference indexes them out of its tables, or the same table entries widened
        at = (lambda table, t: table[t].double()) if wide else (lambda table, t: table[t])
        s0 = int(ts[step_index])
        alpha_t, sigma_t = at(self.alpha_t, prev_t), at(self.sigma_t, prev_t)
        alpha_s0, sigma_s0 = at(self.alpha_t, s0), at(self.sigma_t, s0)
        zero = torch.zeros(())
        cx = c0 = k0 = k1 = k2 = zero
        if order == 1:
            h = at(self.lambda_t, prev_t) - at(self.lambda_t, s0)
            cx, c0 = alpha_t / alpha_s0, sigma_t * (torch.exp(h) - 1.0)
        else:
            older = [int(ts[step_index - j]) for j in range(1, order)]
            rho_t, rho_s0 = sigma_t / alpha_t, sigma_s0 / alpha_s0
            rho_s1 = at(self.sigma_t, older[0]) / at(self.alpha_t, older[0])
            if order == 2:
                k0 = self._ind2(rho_t, rho_s0, rho_s1) - self._ind2(rho_s0, rho_s0, rho_s1)
                k1 = self._ind2(rho_t, rho_s1, rho_s0) - self._ind2(rho_s0, rho_s1, rho_s0)
            else:
                rho_s2 = at(self.sigma_t, older[1]) / at(self.alpha_t, older[1])
                k0 = self._ind3(rho_t, rho_s0, rho_s1, rho_s2) - self._ind3(rho_s0, rho_s0, rho_s1, rho_s2)
                k1 = self._ind3(rho_t, rho_s1, rho_s2, rho_s0) - self._ind3(rho_s0, rho_s1, rho_s2, rho_s0)
                k2 = self._ind3(rho_t, rho_s2, rho_s0, rho_s1) - self._ind3(rho_s0, rho_s2, rho_s0, rho_s1)
        f32 = lambda v: float(torch.as_tensor(v).float())       # noqa: E731  (the one rounding of a float64 scalar; a fp32 one is exact)
        return (order, float(self.alpha_t[s0]), float(self.sigma_t[s0]), f32(cx), f32(c0), float(self.alpha_t[prev_t]) if order > 1 else 0.0,
                f32(k0), f32(k1), f32(k2))

    def step(self, model_output, timestep, sample, return_dict=True, clip=None):
        # scheduling_deis_multistep.py:407-473
        eps, x, restore = self._begin_step(model_output, sample)
        order, alpha_s, sigma_s, cx, c0, alpha_t, k0, k1, k2 = self._plan(self._step_index(timestep))
        m1, m2, oldest = self._history(order, x)
        prev = ops.deis_step(eps, x, alpha_s, sigma_s, cx=cx, c0=c0, m1=m1, alpha_t=alpha_t, k0=k0, k1=k1, m2=m2, k2=k2,
                             x0_clip=1.0 if self.config.thresholding else None, clip=clip, m0_out=oldest)
        self._advance(oldest)
        return self._output(prev, restore, return_dict)


class _SigmaScheduler(_Base):
    """What the sigma-space (k-diffusion) schedulers share -- the constructor, `set_timesteps`, the resolution of a timestep to its
    position, and for the four whose transition is a single launch the body of `step` (`_planned_step`): the sample
    lives in the variance-exploding coordinates x = x_vp * sqrt(sigma^2 + 1) with sigma = sqrt((1 - abar) / abar), the chain starts from noise * init_noise_sigma, the model sees
    scale_model_input(x) = x / sqrt(sigma^2 + 1) at a timestep of np.linspace(0, T - 1, N) -- fractional in general, which is why
    UNet2DModel takes float timesteps -- and every transition is ONE `bd_sigma_step` launch that also writes the next evaluation's
    model input (`step(..., scaled=True)` returns it as `.scaled_sample`).  Host tables: `timesteps` (float64 numpy), `sigmas` (fp32
    torch, trailing 0) and, per position, the fp32 divisor sqrt(sigma^2 + 1) computed with the reference's expression on 0-dim
    tensors.  `step(..., clip=r)` clamps the sample in the coordinates the model sees (the clipping defence of the other pipelines
    carried into sigma space; the reference has no clip here)."""
    order = 1
    _KEYS = ("num_train_timesteps", "beta_start", "beta_end", "beta_schedule", "trained_betas", "prediction_type")
    _BETAS = (0.0001, 0.02)         # the class's default (beta_start, beta_end), the reference's
    # a transition is two `step` calls: a first order stage that leaves something in `_stage`, then the stage that consumes it.
    # `timesteps` then lists a timestep twice (or two equal ones side by side): it resolves to its last position in the first order
    # state and to its first otherwise, and `_check_stage` holds the state against the position's parity
    _two_stage = False
    _second_stage = "a second"      # what the messages call the stage at an odd position

    def __init__(self, num_train_timesteps=1000, beta_start=None, beta_end=None, beta_schedule="linear", trained_betas=None,
                 prediction_type="epsilon", **unused):
        beta_start = self._BETAS[0] if beta_start is None else beta_start
        beta_end = self._BETAS[1] if beta_end is None else beta_end
        self.config = FrozenConfig(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                   beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type)
        self._make_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, trained_betas)
        self.num_inference_steps = None
        self._set_tables(num_train_timesteps)
        self._reset()

    def _reset(self):
        self._stage = None          # what a first order stage left for the stage that follows it

    def set_timesteps(self, num_inference_steps, device=None):
        # the tables stay on the host; the pipelines upload the timesteps once
        self._set_tables(num_inference_steps)
        self._reset()
        self.num_inference_steps = num_inference_steps

    def _set_tables(self, n):
        self._finish_tables(*self._interp(n))

    def _interp(self, n):
        """(timesteps float64 [n] descending, sigmas fp32 [n + 1] with the trailing 0): scheduling_lms_discrete.py:203-206"""
        timesteps = np.linspace(0, self.config.num_train_timesteps - 1, n, dtype=float)[::-1].copy()
        sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        return timesteps, np.concatenate([sigmas, [0.0]]).astype(np.float32)

    def _finish_tables(self, timesteps, sigmas):
        self.timesteps = timesteps                                   # float64 host array
        self.sigmas = torch.from_numpy(sigmas)                       # fp32, on the host: every scalar of a step is a host value
        self.init_noise_sigma = float(self.sigmas.max())
        self._in_div = [float((s ** 2 + 1) ** 0.5) for s in self.sigmas]      # (sigma**2 + 1) ** 0.5 on fp32 0-dim tensors
        # positions by value; a device tensor of fp32 timesteps (what the pipelines hand the UNet) is found by its rounded value
        self._index = {}
        for i, t in enumerate(timesteps):
            for key in {float(t), float(np.float32(t))}:
                self._index.setdefault(key, []).append(i)

    def _positions(self, timestep):
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        pos = self._index.get(float(timestep))
        if not pos:
            raise ValueError(f"{type(self).__name__}: timestep {float(timestep)!r} is not one of this schedule's")
        return pos

    @property
    def state_in_first_order(self):
        return self._stage is None

    def _step_index(self, timestep):
        pos = self._positions(timestep)
        return pos[-1] if self._two_stage and self.state_in_first_order else pos[0]

    def _check_stage(self, k):
        """the state against the parity of position k (before anything touches the GPU); True in a first order stage"""
        first = self.state_in_first_order
        if first != (k % 2 == 0):
            raise ValueError(f"{type(self).__name__}.step: position {k} of the schedule is "
                             f"{'a first order' if k % 2 == 0 else self._second_stage} stage, the scheduler is in the other state")
        return first

    def _kept_sample(self, first, x):
        """None in a first order stage, else the sample the transition started from, which must stand beside x in one launch"""
        if first:
            return None
        if not self._fits(self._stage, x):
            raise ValueError(f"{type(self).__name__}.step: the stored first stage does not have this sample's shape and layout "
                             "(one chain per set_timesteps)")
        return self._stage

    def _step_noise(self, noise, generator, model_output, used):
        """the tensor `bd_sigma_noise_step` reads, given or drawn (draw_step_noise), in the sample's layout; None when the step reads none"""
        if noise is None:
            noise = draw_step_noise(tuple(model_output.shape), generator, model_output.device, used)
        if not used:
            return None
        if noise.dtype != torch.float32 or not noise.is_cuda:
            raise TypeError(f"{type(self).__name__}.step: noise must be a float32 GPU tensor")
        if self._flat(model_output)[1] == "nhwc":          # _align's layout: the model output's
            q = noise.permute(0, 2, 3, 1)
            return q if q.is_contiguous() else q.contiguous()
        return noise.contiguous()

    def _planned_step(self, model_output, timestep, sample, generator, noise, return_dict, clip, scaled, *plan_args):
        """`step` of Euler, Euler-ancestral, KDPM2 and KDPM2-ancestral: one launch of what `_plan_scalars` says -- `bd_sigma_noise_step`
        where it names a churn or a sigma_up, `bd_sigma_step` otherwise, from the kept sample where it says base.  The noise is drawn
        as the reference draws it: with a CPU generator in every call, read or not (a deterministic class passes no generator)."""
        k = self._step_index(timestep)
        first = self._check_stage(k) if self._two_stage else True
        eps, x, restore = self._begin_step(model_output, sample)
        p = self._plan_scalars(k, *plan_args)
        noisy = p["churn"] is not None or p["sigma_up"] is not None
        z = self._step_noise(noise, generator, model_output, noisy)
        sc = torch.empty_like(x) if scaled else None
        base = self._kept_sample(first, x) if p["base"] else None
        if noisy:
            prev = ops.sigma_noise_step(eps, x, z, p["sigma_in"], p["dt"], p["in_div"], base=base, churn=p["churn"], sigma_up=p["sigma_up"],
                                        scaled_out=sc, clip=clip)
        else:
            prev = ops.sigma_step(eps, x, p["sigma_in"], p["dt"], p["in_div"], base=base, scaled_out=sc, clip=clip)
        if self._two_stage:
            self._stage = x if first else None
        return self._output(prev, restore, return_dict, scaled_sample=sc)

    def scale_model_input(self, sample, timestep):
        """sample / sqrt(sigma^2 + 1) at `timestep` (bd_scale_input): bit-equal to the `.scaled_sample` of the step that produced
        `sample` (without clip; with it the step scales before it clamps)."""
        if not sample.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.scale_model_input runs on the GPU only")
        x, tag = self._flat(sample)
        out = ops.scale_input(x, 1.0, self._in_div[self._step_index(timestep)])
        return out.permute(0, 3, 1, 2) if tag == "nhwc" else out


class HeunDiscreteScheduler(_SigmaScheduler):
    """Heun's second order sampler in sigma space (scheduling_heun_discrete.py:84-275, epsilon prediction).  A transition from
    sigma_i to sigma_{i+1} is two calls of `step`, each after one UNet evaluation: a first order (Euler) stage that stores its
    derivative, dt and the sample it started from, then the averaging stage from that sample.  The last transition (to sigma = 0) is a
    plain Euler stage, so N steps cost 2N - 1 evaluations; `timesteps` has those 2N - 1 entries (each after the first twice) and
    `sigmas` 2N.  The defaults are the reference's (beta_start=0.00085, beta_end=0.012)."""
    _BETAS = (0.00085, 0.012)
    _two_stage = True               # scheduling_heun_discrete.py:115-125
    _second_stage = "an averaging"

    def _set_tables(self, n):
        # scheduling_heun_discrete.py:146-187
        t, s = self._interp(n)
        self._finish_tables(np.concatenate([t[:1], np.repeat(t[1:], 2)]), np.concatenate([s[:1], np.repeat(s[1:-1], 2), s[-1:]]))

    def _reset(self):
        self._stage = None          # (derivative buffer, dt, sample) of a first order stage that waits for its averaging stage
        self._dbuf = None

    def _plan_scalars(self, k):
        """(sigma_in, dt or None, in_div) of the stage at position k: an even position is a first order stage sigmas[k] -> sigmas[k + 1],
        an odd one the averaging stage, whose model output was taken at sigmas[k] (the reference's sigma_next) and whose dt is the
        stored one"""
        s = self.sigmas
        return float(s[k]), (float(s[k + 1] - s[k]) if k % 2 == 0 else None), self._in_div[k + 1]

    def step(self, model_output, timestep, sample, return_dict=True, clip=None, scaled=False):
        # scheduling_heun_discrete.py:193-275
        k = self._step_index(timestep)
        eps, x, restore = self._begin_step(model_output, sample)
        first = self._check_stage(k)
        sigma_in, dt, in_div = self._plan_scalars(k)
        sc = torch.empty_like(x) if scaled else None
        if first:
            last = k == len(self.timesteps) - 1
            dbuf = None
            if not last:
                dbuf = self._dbuf if self._fits(self._dbuf, x) else torch.empty_like(x)
            prev = ops.sigma_step(eps, x, sigma_in, dt, in_div, d_out=dbuf, scaled_out=sc, clip=clip)
            if not last:
                self._stage, self._dbuf = (dbuf, dt, x), dbuf
        else:
            dbuf, dt, base = self._stage
            if not self._fits(dbuf, x) or not self._fits(base, x):
                raise ValueError("HeunDiscreteScheduler.step: the stored first stage does not have this sample's shape and layout "
                                 "(one chain per set_timesteps)")
            prev = ops.sigma_step(eps, x, sigma_in, dt, in_div, base=base, average=True, h1=dbuf, scaled_out=sc, clip=clip)
            self._stage = None
        return self._output(prev, restore, return_dict, scaled_sample=sc)


class LMSDiscreteScheduler(_SigmaScheduler):
    """Linear multistep sampler in sigma space (scheduling_lms_discrete.py:106-290, epsilon prediction): `step(..., order=4)` adds the
    derivatives of up to `order` steps with the integrals of their Lagrange basis polynomials over [sigma, sigma_next].  The
    coefficients are the reference's expression on the host -- fp32 0-dim tensors inside the integrand, scipy's quad at epsrel=1e-4 --
    computed once per (num_inference_steps, order) and kept, so a sampling loop makes no quad call.  The previous derivatives live in
    a ring of order - 1 device buffers (order <= 4: one launch carries three history terms); a step writes its own into the oldest.
    Order 1 is Euler."""
    MAX_ORDER = 4

    def __init__(self, *args, **kw):
        self._coeffs = {}           # (steps, order): coefficient table; tables are a function of the step count, so it outlives set_timesteps
        super().__init__(*args, **kw)

    def _reset(self):
        self._ring = []             # previous derivatives, oldest first

    def set_timesteps(self, num_inference_steps, device=None, order=None):
        # scheduling_lms_discrete.py:191-215; order: also prepare the coefficient table of that order
        super().set_timesteps(num_inference_steps)
        if order is not None:
            self.lms_coefficients(order)

    def get_lms_coefficient(self, order, t, current_order):
        # scheduling_lms_discrete.py:169-189
        from scipy import integrate
        sigmas = self.sigmas

        def lms_derivative(tau):
            prod = 1.0
            for k in range(order):
                if current_order == k:
                    continue
                prod *= (tau - sigmas[t - k]) / (sigmas[t - current_order] - sigmas[t - k])
            return prod

        return integrate.quad(lms_derivative, sigmas[t], sigmas[t + 1], epsrel=1e-4)[0]

    def lms_coefficients(self, order):
        """[step][j]: the coefficients of the step at each position for `step(..., order=order)`, as Python floats (the reference
        multiplies fp32 tensors by them: one rounding to fp32 at the launch)"""
        if not 1 <= order <= self.MAX_ORDER:
            raise ValueError(f"LMSDiscreteScheduler: order must be 1..{self.MAX_ORDER} on the HIP path, got {order}")
        key = (len(self.timesteps), order)
        if key not in self._coeffs:
            self._coeffs[key] = [[float(self.get_lms_coefficient(min(i + 1, order), i, j)) for j in range(min(i + 1, order))]
                                 for i in range(len(self.timesteps))]
        return self._coeffs[key]

    def _plan_scalars(self, k, order):
        """(sigma_in, coefficients newest first, in_div) of the step at position k"""
        return float(self.sigmas[k]), self.lms_coefficients(order)[k], self._in_div[k + 1]

    def step(self, model_output, timestep, sample, order=4, return_dict=True, clip=None, scaled=False):
        # scheduling_lms_discrete.py:217-285
        k = self._step_index(timestep)
        eps, x, restore = self._begin_step(model_output, sample)
        sigma_in, coeffs, in_div = self._plan_scalars(k, order)
        ring = self._ring[-(order - 1):] if order > 1 else []
        for h in ring:
            if not self._fits(h, x):
                raise ValueError("LMSDiscreteScheduler.step: the stored derivatives do not have this sample's shape and layout "
                                 "(one chain per set_timesteps)")
        # the reference zips the coefficients with the derivatives it has: a chain entered late uses fewer terms
        terms = min(len(coeffs), 1 + len(ring))
        hist = [ring[-1 - j] if j + 1 < terms else None for j in range(3)]
        c = [coeffs[j] if j < terms else 0.0 for j in range(4)]
        dbuf = None
        if order > 1:       # this step's derivative goes to the oldest buffer of a full ring (it may be the last term read)
            dbuf = ring.pop(0) if len(ring) == order - 1 else torch.empty_like(x)
        sc = torch.empty_like(x) if scaled else None
        prev = ops.sigma_step(eps, x, sigma_in, c[0], in_div, h1=hist[0], c1=c[1], h2=hist[1], c2=c[2], h3=hist[2], c3=c[3],
                              d_out=dbuf, scaled_out=sc, clip=clip)
        self._ring = ring + [dbuf] if order > 1 else []
        return self._output(prev, restore, return_dict, scaled_sample=sc)


def _host_stream(generator):
    """the generator is the reference's: one CPU stream that every `step` call draws from, used or not"""
    return isinstance(generator, ShardedGenerator) or (generator is not None and generator.device.type == "cpu")


def draw_step_noise(shape, generator, device, used):
    """The noise tensor of one `step` call of a stochastic sigma-space sampler, or None.  The reference draws in every call of Euler,
    Euler-ancestral and KDPM2-ancestral whether the step reads the noise or not, so with a CPU generator (or a ShardedGenerator) an
    unused tensor is drawn on the host and dropped -- the stream stays the reference's; with generator=None or a device generator
    only what is used is drawn, on the device."""
    if used:
        return randn_tensor(shape, generator=generator, device=device)
    if _host_stream(generator):
        randn_tensor(shape, generator=generator, device="cpu")
    return None


class EulerDiscreteScheduler(_SigmaScheduler):
    """Euler's method in sigma space with Karras et al.'s churn (scheduling_euler_discrete.py:60-354, epsilon prediction, linear sigma
    interpolation).  gamma = min(s_churn / N, sqrt(2) - 1) inside [s_tmin, s_tmax], else 0.  gamma == 0 is one `bd_sigma_step`
    launch; gamma > 0 one `bd_sigma_noise_step` launch that first raises the sample to sigma_hat = sigma (gamma + 1) with
    (noise s_noise) (sigma_hat^2 - sigma^2)^0.5 and then steps from sigma_hat.  As in the reference the model was evaluated at sigma,
    not at sigma_hat: parity with it is the contract here.  One noise tensor per `step` call on a CPU generator, used or not."""
    _KEYS = _SigmaScheduler._KEYS + ("interpolation_type", "use_karras_sigmas")

    def __init__(self, *args, interpolation_type="linear", use_karras_sigmas=False, **kw):
        if interpolation_type != "linear":
            raise NotImplementedError(f"EulerDiscreteScheduler: interpolation_type={interpolation_type!r} is not on the HIP path (linear only)")
        if use_karras_sigmas:
            raise NotImplementedError("EulerDiscreteScheduler: use_karras_sigmas is not on the HIP path")
        super().__init__(*args, **kw)
        self.config.interpolation_type = interpolation_type
        self.config.use_karras_sigmas = False

    def _plan_scalars(self, k, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0):
        """the scalars of the step at position k, the reference's expressions on fp32 0-dim tensors: sigma_in (= sigma_hat), dt,
        in_div, and churn = (s_noise, (sigma_hat^2 - sigma^2)^0.5) when gamma > 0, else None"""
        sigma = self.sigmas[k]
        gamma = min(s_churn / (len(self.sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sigma <= s_tmax else 0.0
        sigma_hat = sigma * (gamma + 1)
        churn = (float(s_noise), float((sigma_hat ** 2 - sigma ** 2) ** 0.5)) if gamma > 0 else None
        return dict(sigma_in=float(sigma_hat), dt=float(self.sigmas[k + 1] - sigma_hat), in_div=self._in_div[k + 1], churn=churn,
                    sigma_up=None, base=False)

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0, generator=None,
             return_dict=True, noise=None, clip=None, scaled=False):
        # scheduling_euler_discrete.py:257-354
        return self._planned_step(model_output, timestep, sample, generator, noise, return_dict, clip, scaled, s_churn, s_tmin, s_tmax, s_noise)


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """Ancestral sampling with Euler steps (scheduling_euler_ancestral_discrete.py:60-281, epsilon prediction): a deterministic Euler
    step from sigma down to sigma_down < sigma_next, then fresh noise of standard deviation sigma_up, so that the sample lands on
    sigma_next.  One `bd_sigma_noise_step` launch per step; sigma_up and sigma_down are the reference's expressions on fp32 0-dim
    tensors."""

    def _plan_scalars(self, k):
        """sigma_in, dt = sigma_down - sigma, in_div and sigma_up of the step at position k"""
        sigma_from, sigma_to = self.sigmas[k], self.sigmas[k + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        return dict(sigma_in=float(sigma_from), dt=float(sigma_down - sigma_from), in_div=self._in_div[k + 1], churn=None,
                    sigma_up=float(sigma_up), base=False)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None, clip=None, scaled=False):
        # scheduling_euler_ancestral_discrete.py:193-281
        return self._planned_step(model_output, timestep, sample, generator, noise, return_dict, clip, scaled)


class _KDPM2Base(_SigmaScheduler):
    """What KDPM2 and KDPM2-ancestral share (DPM-Solver-2 of Karras et al. in sigma space): a transition is two calls of `step`, a
    first order stage from sigma to an interpolated sigma_interpol, which keeps the sample it started from, and a second stage that
    takes the derivative there and steps from the kept sample over the whole interval.  `timesteps` has 2N - 1 entries -- the N
    of the schedule with the fractional sigma_to_t(sigma_interpol) between them -- and the last is a first order stage to
    sigma_interpol = 0, so a finished chain leaves its stage pending; set_timesteps resets it.  The flat tables `sigmas`,
    `sigmas_interpol` (and the ancestral ones) have the reference's layout: the first entry once, every later one twice, the last
    once more.  Entries of `timesteps` may be equal (KDPM2-ancestral's sigma_interpol is sigma_next to within rounding): a timestep
    resolves to its last position in the first order state and to its first otherwise, and `step` checks the state against the
    position's parity.  `_stage` is the sample a first order stage started from, waiting for its second stage.  The defaults are the
    reference's (beta_start=0.00085, beta_end=0.012)."""
    _BETAS = (0.00085, 0.012)
    _two_stage = True

    @staticmethod
    def _twice(v):
        return torch.cat([v[:1], v[1:].repeat_interleave(2), v[-1:]])

    def _sigma_to_t(self, sigma, log_sigmas):
        """the (fractional) training timestep whose sigma is `sigma`, by linear interpolation in log sigma over the training table;
        fp32 throughout, as the reference computes it"""
        log_sigma = sigma.log()
        below = (log_sigma - log_sigmas[:, None]).ge(0)
        low_idx = below.cumsum(dim=0).argmax(dim=0).clamp(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = ((low - log_sigma) / (low - high)).clamp(0, 1)
        return ((1 - w) * low_idx + w * high_idx).view(sigma.shape)

    def _base_tables(self, n):
        """(timesteps float64 tensor [n], sigmas fp32 tensor [n + 1], log of the training sigmas fp32)"""
        timesteps, sigmas = self._interp(n)
        train = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
        return torch.from_numpy(timesteps), torch.from_numpy(sigmas), torch.from_numpy(np.log(train))

    def _finish_kdpm2(self, timesteps, sigmas, sigmas_interpol, interpol_of_odd):
        """interpol_of_odd(k): the index into the flat sigmas_interpol of the sigma the second stage at odd position k is evaluated at"""
        self.sigmas_interpol = self._twice(sigmas_interpol)
        self._finish_tables(timesteps.numpy(), self._twice(sigmas).numpy())
        flat = self.sigmas_interpol
        # the divisor of the model input per position: sigma at a first order position, sigma_interpol at a second stage one; one
        # more entry for what follows the last position (sigma_interpol = 0 there)
        self._in_div = [float(((self.sigmas[k] if k % 2 == 0 else flat[interpol_of_odd(k)]) ** 2 + 1) ** 0.5)
                        for k in range(len(self.timesteps) + 1)]


class KDPM2DiscreteScheduler(_KDPM2Base):
    """KDPM2 (scheduling_k_dpm_2_discrete.py:60-310, epsilon prediction): deterministic, both stages on `bd_sigma_step`.
    sigma_interpol is the geometric mean of sigma and sigma_next (a log-lerp with the rolled sigmas).  N steps cost 2N - 1 UNet
    evaluations."""

    def _set_tables(self, n):
        # scheduling_k_dpm_2_discrete.py:152-203
        timesteps, sigmas, log_sigmas = self._base_tables(n)
        sigmas_interpol = sigmas.log().lerp(sigmas.roll(1).log(), 0.5).exp()       # [i]: between sigmas[i - 1] and sigmas[i]
        t_interpol = self._sigma_to_t(sigmas_interpol, log_sigmas).to(timesteps.dtype)
        pairs = torch.stack((t_interpol[1:-1, None], timesteps[1:, None]), dim=-1).flatten()
        self._finish_kdpm2(torch.cat([timesteps[:1], pairs]), sigmas, sigmas_interpol, lambda k: k)

    def _plan_scalars(self, k):
        """sigma_in, dt, in_div of the stage at position k, and whether it starts from the kept sample"""
        s, si = self.sigmas, self.sigmas_interpol
        if k % 2 == 0:      # sigmas[k] -> sigma_interpol
            return dict(sigma_in=float(s[k]), dt=float(si[k + 1] - s[k]), in_div=self._in_div[k + 1], churn=None, sigma_up=None, base=False)
        return dict(sigma_in=float(si[k]), dt=float(s[k] - s[k - 1]), in_div=self._in_div[k + 1], churn=None, sigma_up=None, base=True)

    def step(self, model_output, timestep, sample, return_dict=True, clip=None, scaled=False):
        # scheduling_k_dpm_2_discrete.py:232-310
        return self._planned_step(model_output, timestep, sample, None, None, return_dict, clip, scaled)


class KDPM2AncestralDiscreteScheduler(_KDPM2Base):
    """KDPM2 with ancestral sampling (scheduling_k_dpm_2_ancestral_discrete.py:60-329, epsilon prediction): the first stage runs on
    `bd_sigma_step` towards sigma_interpol, the geometric mean of sigma and sigma_down; the second on `bd_sigma_noise_step`, from
    the kept sample with dt = sigma_down - sigma and noise of standard deviation sigma_up.  The reference draws a noise tensor in
    both stages and uses the second's; with a CPU generator so does `step`.  The last entries of `sigmas_up` are NaN (0 * 0 / 0) in
    the reference and here, and are never read.  num_inference_steps < 3 is refused: at 2 the reference's schedule holds a NaN
    timestep and its chain fails."""

    def _set_tables(self, n):
        # scheduling_k_dpm_2_ancestral_discrete.py:153-214
        if n < 3:
            raise ValueError(f"KDPM2AncestralDiscreteScheduler: num_inference_steps={n} must be at least 3 (at 2 the schedule has a NaN "
                             "timestep, in the reference as well, and no chain runs)")
        timesteps, sigmas, log_sigmas = self._base_tables(n)
        sigmas_next = sigmas.roll(-1)
        sigmas_next[-1] = 0.0
        sigmas_up = (sigmas_next ** 2 * (sigmas ** 2 - sigmas_next ** 2) / sigmas ** 2) ** 0.5
        sigmas_down = (sigmas_next ** 2 - sigmas_up ** 2) ** 0.5
        sigmas_down[-1] = 0.0
        sigmas_interpol = sigmas.log().lerp(sigmas_down.log(), 0.5).exp()
        sigmas_interpol[-2:] = 0.0
        self.sigmas_up, self.sigmas_down = self._twice(sigmas_up), self._twice(sigmas_down)
        t_interpol = self._sigma_to_t(sigmas_interpol, log_sigmas).to(timesteps.dtype)
        pairs = torch.stack((t_interpol[:-2, None], timesteps[1:, None]), dim=-1).flatten()
        self._finish_kdpm2(torch.cat([timesteps[:1], pairs]), sigmas, sigmas_interpol, lambda k: k - 1)

    def _plan_scalars(self, k):
        """sigma_in, dt, in_div of the stage at position k; a second stage also has sigma_up and starts from the kept sample"""
        s, si = self.sigmas, self.sigmas_interpol
        if k % 2 == 0:      # sigmas[k] -> sigma_interpol
            return dict(sigma_in=float(s[k]), dt=float(si[k] - s[k]), in_div=self._in_div[k + 1], churn=None, sigma_up=None, base=False)
        return dict(sigma_in=float(si[k - 1]), dt=float(self.sigmas_down[k - 1] - s[k - 1]), in_div=self._in_div[k + 1], churn=None,
                    sigma_up=float(self.sigmas_up[k - 1]), base=True)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, noise=None, clip=None, scaled=False):
        # scheduling_k_dpm_2_ancestral_discrete.py:243-329
        return self._planned_step(model_output, timestep, sample, generator, noise, return_dict, clip, scaled)


class SchedulerConfigCarrier(DDPMScheduler):
    """What DiffuserModelSched returns as `noise_sched` for the `--sched` types the reference constructs but never steps
    (model.py:598-630: DPM-Solver(++), UniPC, DEIS, Heun, LMS): training only uses its betas (`add_noise`,
    `alphas_cumprod`, `config.num_train_timesteps`) and sampling goes through PNDMPipeline, which rebuilds a PNDMScheduler
    from this config.  `class_name` records which reference class the config stands for."""

    def __init__(self, class_name, **kw):
        super().__init__(**kw)
        self.class_name = class_name

    def step(self, *a, **k):
        raise NotImplementedError(f"{self.class_name}.step is never called by the reference either: PNDMPipeline converts the "
                                  "scheduler to PNDMScheduler (pipeline_pndm.py:46)")
