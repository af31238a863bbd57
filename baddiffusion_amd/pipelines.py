"""DDPMPipeline / DDIMPipeline -- drop-in for the two (locally modified) pipelines BadDiffusion samples with
(diffusers/src/diffusers/pipelines/ddpm/pipeline_ddpm.py:46-125, pipelines/ddim/pipeline_ddim.py:50-142 of the reference tree),
including the repo's additions `init=`, `save_every_step=`, `start_from=` and the `.movie` output -- and the pipelines of the other
samplers: PNDM, DPM-Solver(++), UniPC, DEIS (_MultistepPipeline), Heun, LMS, Euler, Euler-ancestral, KDPM2, KDPM2-ancestral
(_SigmaPipeline) and RePaint.

Loop body = one UNet forward (bd_unet_forward) + one fused scheduler step kernel; the image never leaves the
GPU until the final (x/2+0.5).clamp(0,1) -> NHWC conversion (bd_to_image).  With a CPU `generator` the
per-step noise is drawn on the CPU in the reference's order (seed parity, scheduling_ddpm.py:400-404);
with a CUDA generator or `generator=None` it is drawn on the device (throughput mode).
"""
import json
import os

import numpy as np
import torch

from . import ops
from .schedulers import (DDIMScheduler, PNDMScheduler, DDPMScheduler, DEISMultistepScheduler, DPMSolverMultistepScheduler,
                         EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, HeunDiscreteScheduler,
                         KDPM2AncestralDiscreteScheduler, KDPM2DiscreteScheduler, LMSDiscreteScheduler, RePaintScheduler,
                         UniPCMultistepScheduler, draw_step_noise, randn_tensor)


class ImagePipelineOutput:
    def __init__(self, images, movie=None):
        self.images = images
        self.movie = movie if movie is not None else []


def _static_weights(call):
    """The sampling loop evaluates the UNet num_inference_steps times over the same parameters: promise that to the plan so it
    prepares the weights (split-plane copy, upsample tap planes) once per loop instead of once per evaluation."""
    import functools

    @functools.wraps(call)
    def wrapped(self, *a, **kw):
        sw = getattr(self.unet, "static_weights", None)
        if sw is None:
            return call(self, *a, **kw)
        with sw():
            return call(self, *a, **kw)
    return wrapped


class _PipelineBase:
    supports_u8 = True      # output_type="u8" returns device uint8 images (batch_sampling_save's overlapped PNG path)

    def __init__(self, unet, scheduler):
        self.unet = unet
        self.scheduler = scheduler
        self._progress = {}

    @property
    def device(self):
        return self.unet.device

    def to(self, device):
        self.unet.to(device)
        return self

    def set_progress_bar_config(self, **kw):
        self._progress = kw

    def progress_bar(self, it):
        if self._progress.get("disable", True):
            return it
        try:
            from tqdm.auto import tqdm
            return tqdm(it, **{k: v for k, v in self._progress.items() if k != "disable"})
        except ImportError:
            return it

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image
        if images.ndim == 3:
            images = images[None, ...]
        images = (images * 255).round().astype("uint8")
        if images.shape[-1] == 1:
            return [Image.fromarray(image.squeeze(), mode="L") for image in images]
        return [Image.fromarray(image) for image in images]

    def _image_shape(self, batch_size):
        s = self.unet.config.sample_size
        return (batch_size, self.unet.config.in_channels, s, s)

    def _to_numpy(self, image_nhwc_storage, shape):
        """image: NHWC storage [B,H,W,C] -> float32 numpy [B,H,W,C] in [0,1] (pipeline_ddpm.py:115-116)."""
        return ops.to_image(image_nhwc_storage, True, shape).cpu().numpy()

    def _to_u8(self, image_nhwc_storage, shape):
        """device uint8 [B,H,W,C] = round(255 * (x/2+0.5).clamp(0,1)): what the PNG writer needs, without leaving the GPU
        and without a host synchronisation (output_type="u8"; model.py:496-502 quantises the same way on the host)."""
        return ops.to_image(image_nhwc_storage, True, shape, want_u8=True)[1]

    def _start(self, batch_size, generator, init):
        shape = self._image_shape(batch_size)
        if init is None:
            image = randn_tensor(shape, generator=generator, device=self.device)
        else:
            image = init.detach().clone().to(self.device)
            shape = tuple(image.shape)
        # keep the running sample in NHWC storage (what the UNet consumes and produces)
        return ops.nchw_to_nhwc(image.float()), shape

    def _finish(self, image, shape, mov, output_type, save_every_step, return_dict):
        """What every __call__ returns: the final sample (NHWC storage) as device uint8 ("u8"), PIL images ("pil", the movie's frames
        too) or float32 numpy (anything else), alone in a tuple or with the movie in an ImagePipelineOutput."""
        if output_type == "u8":
            images = self._to_u8(image, shape)
            return ImagePipelineOutput(images=images, movie=mov) if return_dict else (images,)
        images = self._to_numpy(image, shape)
        if output_type == "pil":
            images = self.numpy_to_pil(images)
            if save_every_step:
                mov = list(map(self.numpy_to_pil, mov))
        if not return_dict:
            return (images,)
        return ImagePipelineOutput(images=images, movie=mov)

    def noise_draws(self, num_inference_steps=None, start_from=0, eta=0.0, **kwargs):
        """How many chunk-shaped tensors ONE call draws from its generator after the initial sample: what a rank that owns no row of a chunk
        must draw and discard to keep a shared CPU stream in the unsharded order (model.batch_sampling_save(parity=True))."""
        return 0

    def advance_generator(self, batch_size, generator, init_given, **kwargs):
        """draw and discard everything __call__(batch_size, generator=generator, init=None / given, **kwargs) would draw"""
        shape = self._image_shape(batch_size)
        for _ in range((0 if init_given else 1) + self.noise_draws(**kwargs)):
            torch.randn(shape, generator=generator)

    # ---- diffusers-layout save (SURVEY f-2) ------------------------------------------------------------------
    def save_pretrained(self, save_directory):
        from .model import save_unet, save_scheduler
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "model_index.json"), "w") as f:
            json.dump({"_class_name": type(self).__name__, "_diffusers_version": "0.16.0.dev0",
                       "scheduler": ["diffusers", type(self.scheduler).__name__], "unet": ["diffusers", "UNet2DModel"]}, f, indent=2)
        save_unet(self.unet, os.path.join(save_directory, "unet"))
        save_scheduler(self.scheduler, os.path.join(save_directory, "scheduler"))


class DDPMPipeline(_PipelineBase):
    def noise_draws(self, num_inference_steps=1000, start_from=0, **kwargs):
        self.scheduler.set_timesteps(num_inference_steps)
        return sum(1 for t in self.scheduler.timesteps[start_from:] if int(t) > 0)      # scheduling_ddpm.py:400: `if t > 0`

    @_static_weights
    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, num_inference_steps=1000, start_from=0, output_type="pil", init=None,
                 save_every_step=False, return_dict=True, **kwargs):
        image, shape = self._start(batch_size, generator, init)
        self.scheduler.set_timesteps(num_inference_steps)
        mov = [self._to_numpy(image, shape)] if save_every_step else []
        ts_host = self.scheduler.timesteps[start_from:]
        ts_dev = torch.as_tensor(ts_host, dtype=torch.int64).to(self.device)    # one H2D copy for the whole chain
        for i, t in enumerate(self.progress_bar(ts_host)):
            t = int(t)
            eps = self.unet(image.permute(0, 3, 1, 2), ts_dev[i]).sample.permute(0, 2, 3, 1)        # NHWC storage
            noise = None
            if t > 0:   # same draw order / shape as randn_tensor(model_output.shape) in the reference
                noise = randn_tensor(shape, generator=generator, device=self.device)
                noise = ops.nchw_to_nhwc(noise)
            image = self.scheduler.step(eps.permute(0, 3, 1, 2), t, image.permute(0, 3, 1, 2),
                                        noise=noise.permute(0, 3, 1, 2) if noise is not None else None
                                        ).prev_sample.permute(0, 2, 3, 1)
            if save_every_step:
                mov.append(self._to_numpy(image, shape))
        return self._finish(image, shape, mov, output_type, save_every_step, return_dict)


class DDIMPipeline(_PipelineBase):
    def __init__(self, unet, scheduler):
        # pipeline_ddim.py:39-42: make sure the scheduler can always be converted to DDIM
        scheduler = DDIMScheduler.from_config(scheduler.config)
        super().__init__(unet, scheduler)

    def noise_draws(self, num_inference_steps=50, eta=0.0, **kwargs):
        self.scheduler.set_timesteps(num_inference_steps)
        return len(self.scheduler.timesteps) if eta > 0 else 0                           # scheduling_ddim.py:366: `if eta > 0`

    @_static_weights
    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, eta=0.0, num_inference_steps=50, use_clipped_model_output=None,
                 output_type="pil", init=None, save_every_step=False, return_dict=True, **kwargs):
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective "
                             f"batch size of {batch_size}.")
        image, shape = self._start(batch_size, generator, init)
        self.scheduler.set_timesteps(num_inference_steps)
        mov = [self._to_numpy(image, shape)] if save_every_step else []
        ts_dev = torch.as_tensor(self.scheduler.timesteps, dtype=torch.int64).to(self.device)   # one H2D copy for the whole chain
        for i, t in enumerate(self.progress_bar(self.scheduler.timesteps)):
            t = int(t)
            eps = self.unet(image.permute(0, 3, 1, 2), ts_dev[i]).sample
            image = self.scheduler.step(eps, t, image.permute(0, 3, 1, 2), eta=eta,
                                        use_clipped_model_output=bool(use_clipped_model_output),
                                        generator=generator).prev_sample.permute(0, 2, 3, 1)
            if save_every_step:
                mov.append(self._to_numpy(image, shape))
        return self._finish(image, shape, mov, output_type, save_every_step, return_dict)


class _MultistepPipeline(_PipelineBase):
    """The sampling loop of the deterministic samplers (PNDMPipeline, DPMSolverPipeline, UniPCPipeline, DEISPipeline; _SigmaPipeline has its own
    under the same call): the call surface of the reference's PNDM pipeline (`init`, `start_from`, `save_every_step`, output_type
    "pil" | "numpy" | "u8" | None), one UNet forward + one fused step launch per step, no noise drawn after the start.  `clip_sample`
    is the post-step clamp of the sample (pipeline_pndm.py:108-109), folded into the step launch (`scheduler.step(..., clip=)`).  A
    subclass names its scheduler class and `default_steps`, the num_inference_steps of a call that gives none; a scheduler of
    another class is converted from its config.  With start_from=k the scheduler's history is empty, so the first executed step is
    first order."""
    scheduler_class = None
    default_steps = None

    def __init__(self, unet, scheduler, clip_sample=False, clip_sample_range=1.0):
        if not isinstance(scheduler, self.scheduler_class):
            scheduler = self.scheduler_class.from_config(scheduler.config)
        super().__init__(unet, scheduler)
        self.clip_sample = clip_sample
        self.clip_sample_range = clip_sample_range

    @_static_weights
    @torch.no_grad()
    def __call__(self, batch_size=1, num_inference_steps=None, start_from=0, generator=None, output_type="pil", init=None,
                 save_every_step=False, return_dict=True, **kwargs):
        if num_inference_steps is None:
            num_inference_steps = self.default_steps
        return self._sample(batch_size, num_inference_steps, start_from, generator, output_type, init, save_every_step, return_dict)

    def _sample(self, batch_size, num_inference_steps, start_from, generator, output_type, init, save_every_step, return_dict):
        image, shape = self._start(batch_size, generator, init)
        mov = [self._to_numpy(image, shape)] if save_every_step else []
        self.scheduler.set_timesteps(num_inference_steps)
        ts_host = self.scheduler.timesteps[int(start_from):]
        ts_dev = torch.as_tensor(ts_host, dtype=torch.int64).to(self.device)
        clip = float(self.clip_sample_range) if self.clip_sample else None
        for i, t in enumerate(self.progress_bar(ts_host)):
            eps = self.unet(image.permute(0, 3, 1, 2), ts_dev[i]).sample
            image = self.scheduler.step(eps, int(t), image.permute(0, 3, 1, 2), clip=clip).prev_sample.permute(0, 2, 3, 1)
            if save_every_step:
                mov.append(self._to_numpy(image, shape))
        return self._finish(image, shape, mov, output_type, save_every_step, return_dict)


class PNDMPipeline(_MultistepPipeline):
    """pipelines/pndm/pipeline_pndm.py:39-122 (the reference's modified copy: `clip_sample` / `clip_sample_range`, `init`,
    `start_from`, `save_every_step`): _MultistepPipeline's loop.  Whatever scheduler it is given, a PNDMScheduler included, is
    rebuilt as a PNDMScheduler from its config (:46) -- which is how every `--sched` other than DDPM / DDIM samples in the
    reference."""
    scheduler_class = PNDMScheduler
    default_steps = 50

    def __init__(self, unet, scheduler, clip_sample=False, clip_sample_range=1.0):
        super().__init__(unet, PNDMScheduler.from_config(scheduler.config), clip_sample, clip_sample_range)

    def encode(self, image, *args, **kwargs):
        return image

    def decode(self, image, *args, **kwargs):
        return image


class DPMSolverPipeline(_MultistepPipeline):
    """Sampling with DPMSolverMultistepScheduler: _MultistepPipeline's loop, one UNet forward + one `bd_dpm_step` launch per step.
    The reference has no pipeline for this scheduler (its DPM-Solver `--sched` names sample through PNDMPipeline);
    num_inference_steps=20 is this project's default.  A scheduler that is not a DPMSolverMultistepScheduler is converted from its
    config."""
    scheduler_class = DPMSolverMultistepScheduler
    default_steps = 20


class UniPCPipeline(_MultistepPipeline):
    """Sampling with UniPCMultistepScheduler: _MultistepPipeline's loop, one UNet forward + one `bd_unipc_step` launch (corrector +
    predictor) per step.  The reference has no pipeline for this scheduler either; num_inference_steps=10 is this project's default,
    the regime UniPC is built for.  A scheduler that is not a UniPCMultistepScheduler is converted from its config.  With
    start_from=k there is no last sample, so the first executed step has no corrector and is first order."""
    scheduler_class = UniPCMultistepScheduler
    default_steps = 10


class DEISPipeline(_MultistepPipeline):
    """Sampling with DEISMultistepScheduler: _MultistepPipeline's loop, one UNet forward + one `bd_deis_step` launch per step.  The
    reference has no pipeline for this scheduler either (its DEIS-SCHED samples through PNDMPipeline); num_inference_steps=10 is this
    project's default, the regime DEIS is built for.  A scheduler that is not a DEISMultistepScheduler is converted from its config."""
    scheduler_class = DEISMultistepScheduler
    default_steps = 10


class _SigmaPipeline(_MultistepPipeline):
    """The sampling loop of the sigma-space samplers (HeunPipeline, LMSPipeline, EulerPipeline, EulerAncestralPipeline, KDPM2Pipeline,
    KDPM2AncestralPipeline), with _MultistepPipeline's call surface.  The raw
    state is init * init_noise_sigma -- `init` is what the sibling pipelines start from, so noise + trigger is scaled as a whole --
    and the model never sees it: every evaluation reads the scaled buffer x / sqrt(sigma^2 + 1), which `bd_scale_input` produces at
    the start and each `bd_sigma_step` launch afterwards, next to the raw sample.  One UNet forward at a float timestep (uploaded
    once, fp32) + one fused launch per evaluation; the deterministic samplers draw no noise after the start, the stochastic ones
    (`_noise_used`) one tensor per position where the reference draws one.  `clip_sample` clamps the scaled buffer (the
    sample in the coordinates the model sees) and rescales the raw sample to match.  `save_every_step` frames are the scaled
    buffers -- the only ones that are images; the last frame is the final sample, at sigma = 0 where both coincide.  With
    start_from=k the chain enters at position k of `scheduler.timesteps` with an empty history."""

    _odd_start = None        # samplers with two evaluations per transition: what an odd start_from is, for the refusal
    _stochastic = False      # the reference draws a noise tensor at every evaluation (`_noise_used` says which are read)

    def _step_kwargs(self):
        return {}

    def _set_kwargs(self):
        """what set_timesteps takes beside the step count: the step's own keywords, unless a subclass says otherwise"""
        return self._step_kwargs()

    def _check_start(self, start_from):
        if self._odd_start and start_from % 2:
            raise ValueError(f"{type(self).__name__}: start_from={start_from} is {self._odd_start}; start at an even position")

    def noise_draws(self, num_inference_steps=None, start_from=0, **kwargs):
        if not self._stochastic:
            return 0
        n = num_inference_steps or self.default_steps
        return (2 * n - 1 if self.scheduler_class._two_stage else n) - int(start_from)

    def _noise_used(self, position):
        """None: the sampler draws nothing at this position of `scheduler.timesteps`; True / False: the reference draws a tensor there
        and the step reads it / drops it"""
        return None

    def _step_noise(self, position, shape, generator):
        """{} or {"noise": tensor} for the step at `position`: drawn as the reference draws it (draw_step_noise) in NCHW order, then
        taken to the NHWC storage the sample lives in, as DDPMPipeline does"""
        used = self._noise_used(position)
        if used is None:
            return {}
        noise = draw_step_noise(shape, generator, self.device, used)
        return {} if noise is None else {"noise": ops.nchw_to_nhwc(noise).permute(0, 3, 1, 2)}

    def _sample(self, batch_size, num_inference_steps, start_from, generator, output_type, init, save_every_step, return_dict):
        start_from = int(start_from)
        self._check_start(start_from)
        sched = self.scheduler
        sched.set_timesteps(num_inference_steps, **self._set_kwargs())       # a refused step count: before anything is drawn
        image, shape = self._start(batch_size, generator, init)
        ts_host = [float(t) for t in sched.timesteps[start_from:]]
        ts_dev = torch.as_tensor(ts_host, dtype=torch.float64).to(torch.float32).to(self.device)    # one H2D copy for the whole chain
        clip = float(self.clip_sample_range) if self.clip_sample else None
        scaled = image
        if ts_host:
            # raw = init * init_noise_sigma; first model input = raw / sqrt(sigma_0^2 + 1), both roundings in one launch
            scaled = ops.scale_input(image, sched.init_noise_sigma, sched._in_div[start_from])
            image = ops.scale_input(image, sched.init_noise_sigma, 1.0, out=image)
        mov = [self._to_numpy(scaled, shape)] if save_every_step else []
        for i, t in enumerate(self.progress_bar(ts_host)):
            eps = self.unet(scaled.permute(0, 3, 1, 2), ts_dev[i]).sample
            out = sched.step(eps, t, image.permute(0, 3, 1, 2), clip=clip, scaled=True, **self._step_kwargs(),
                             **self._step_noise(start_from + i, shape, generator))
            image, scaled = out.prev_sample.permute(0, 2, 3, 1), out.scaled_sample.permute(0, 2, 3, 1)
            if save_every_step:
                mov.append(self._to_numpy(scaled, shape))
        # the last divisor is sqrt(0 + 1) = 1: the scaled buffer is the final sample (and carries the clamp when clip_sample is set)
        image = scaled
        return self._finish(image, shape, mov, output_type, save_every_step, return_dict)


class HeunPipeline(_SigmaPipeline):
    """Sampling with HeunDiscreteScheduler: _SigmaPipeline's loop.  The reference has no pipeline for this scheduler (its HEUN-SCHED
    samples through PNDMPipeline); num_inference_steps=10 is this project's default: 19 UNet evaluations, two per transition but
    the last.  start_from counts positions of `scheduler.timesteps` (evaluations); an odd one is the averaging stage of a
    transition whose first stage was not run, and is refused."""
    scheduler_class = HeunDiscreteScheduler
    default_steps = 10
    _odd_start = "the second entry of a timestep pair (the averaging stage of a transition whose first stage would be missing)"


class LMSPipeline(_SigmaPipeline):
    """Sampling with LMSDiscreteScheduler at `order` (1..4; 1 is Euler): _SigmaPipeline's loop.  The reference has no pipeline for
    this scheduler either; num_inference_steps=20 is this project's default."""
    scheduler_class = LMSDiscreteScheduler
    default_steps = 20

    def __init__(self, unet, scheduler, clip_sample=False, clip_sample_range=1.0, order=4):
        super().__init__(unet, scheduler, clip_sample=clip_sample, clip_sample_range=clip_sample_range)
        if not 1 <= int(order) <= LMSDiscreteScheduler.MAX_ORDER:
            raise ValueError(f"LMSPipeline: order must be 1..{LMSDiscreteScheduler.MAX_ORDER}, got {order}")
        self.order = int(order)

    def _step_kwargs(self):
        return {"order": self.order}


class EulerPipeline(_SigmaPipeline):
    """Sampling with EulerDiscreteScheduler: _SigmaPipeline's loop.  s_churn / s_noise are Karras et al.'s churn, handed to every
    `step`: with s_churn == 0 (the default) the chain is the deterministic Euler one, one `bd_sigma_step` per step; with
    s_churn > 0 every step is one `bd_sigma_noise_step` that first raises the sample to sigma_hat.  The reference draws a noise
    tensor in every step either way, so with a CPU generator one is drawn (and dropped when unused): the stream, and the next
    chunk's initial noise, stay the reference's.  num_inference_steps=20 is this project's default."""
    scheduler_class = EulerDiscreteScheduler
    default_steps = 20
    _stochastic = True

    def __init__(self, unet, scheduler, clip_sample=False, clip_sample_range=1.0, s_churn=0.0, s_noise=1.0):
        super().__init__(unet, scheduler, clip_sample=clip_sample, clip_sample_range=clip_sample_range)
        self.s_churn, self.s_noise = float(s_churn), float(s_noise)

    def _step_kwargs(self):
        return {"s_churn": self.s_churn, "s_noise": self.s_noise}

    def _set_kwargs(self):
        return {}

    def _noise_used(self, position):
        return self.scheduler._plan_scalars(position, s_churn=self.s_churn, s_noise=self.s_noise)["churn"] is not None


class EulerAncestralPipeline(_SigmaPipeline):
    """Sampling with EulerAncestralDiscreteScheduler: _SigmaPipeline's loop, one UNet forward + one `bd_sigma_noise_step` launch per
    step, one noise tensor per step.  num_inference_steps=20 is this project's default."""
    scheduler_class = EulerAncestralDiscreteScheduler
    default_steps = 20
    _stochastic = True

    def _noise_used(self, position):
        return True


class KDPM2Pipeline(_SigmaPipeline):
    """Sampling with KDPM2DiscreteScheduler: _SigmaPipeline's loop, deterministic.  num_inference_steps=10 is this project's
    default: 19 UNet evaluations, two per transition but the last.  start_from counts positions of `scheduler.timesteps`
    (evaluations); an odd one is the second stage of a transition whose first stage was not run, and is refused."""
    scheduler_class = KDPM2DiscreteScheduler
    default_steps = 10
    _odd_start = "the second stage of a transition whose first stage would be missing"


class KDPM2AncestralPipeline(KDPM2Pipeline):
    """Sampling with KDPM2AncestralDiscreteScheduler: KDPM2Pipeline's loop with a `bd_sigma_noise_step` second stage.  The
    reference draws a noise tensor at every position, 2N - 1 per chain, and reads the second stages'; with a CPU generator so does
    this pipeline."""
    scheduler_class = KDPM2AncestralDiscreteScheduler
    _stochastic = True

    def _noise_used(self, position):
        return position % 2 == 1


def with_default_steps(pipeline, num_inference_steps):
    """`pipeline` with its calls (and its noise_draws) defaulting to num_inference_steps: how a command-line --infer_steps reaches the
    helpers that call a pipeline without naming a step count (batch_sampling, batch_sampling_save)"""
    base = type(pipeline)

    class _Fixed(base):
        def __call__(self, *a, **kw):
            kw.setdefault("num_inference_steps", num_inference_steps)
            return super().__call__(*a, **kw)

        def noise_draws(self, **kw):
            kw.setdefault("num_inference_steps", num_inference_steps)
            return super().noise_draws(**kw)
    _Fixed.__name__, _Fixed.__qualname__ = base.__name__, base.__qualname__      # save_pretrained records the class by name
    pipeline.__class__ = _Fixed
    return pipeline


class RePaintPipeline(_PipelineBase):
    """pipelines/repaint/pipeline_repaint.py:73-171 for tensors: inpaint `image` where `mask_image` is 0 with an unconditional DDPM UNet.
    Whatever scheduler it is given is converted to a RePaintScheduler from its config.  Loop body = one UNet forward + one fused
    `bd_repaint_step` launch on the way down, one `bd_repaint_undo` call (num_train_timesteps // num_inference_steps noising sub-steps)
    on the way back up; the running sample stays in NHWC storage and the original image and the mask are read through their strides.
    Additions in the style of the sibling pipelines: `init=` (replaces the initial noise: how noise + trigger is fed in), `batch_size=`
    (chains per call when `image` is one shared [1,C,H,W] / [C,H,W] image), `known_shift=` (the schedulers' trigger-consistent variant),
    `save_every_step=` / `.movie`, output_type="u8".  The reference's PIL preprocessing is not ported: tensors only."""

    def __init__(self, unet, scheduler):
        super().__init__(unet, RePaintScheduler.from_config(scheduler.config))

    def _counts(self, num_inference_steps, jump_length, jump_n_sample):
        """(UNet evaluations, undo transitions) of one chain"""
        self.scheduler.set_timesteps(num_inference_steps, jump_length, jump_n_sample)
        ts = [int(t) for t in self.scheduler.timesteps]
        evals, undos, t_last = 0, 0, ts[0] + 1
        for t in ts:
            if t < t_last:
                evals += 1
            else:
                undos += 1
            t_last = t
        return evals, undos

    def noise_draws(self, num_inference_steps=250, jump_length=10, jump_n_sample=10, **kwargs):
        evals, undos = self._counts(num_inference_steps, jump_length, jump_n_sample)      # one draw per step, one per undo sub-step
        return evals + undos * (self.scheduler.config.num_train_timesteps // self.scheduler.num_inference_steps)

    @staticmethod
    def _tensor(x, name):
        if not torch.is_tensor(x):
            raise TypeError(f"RePaintPipeline: {name} must be a torch.Tensor in the model's range (PIL preprocessing is not ported), "
                            f"got {type(x).__name__}")
        return x

    @_static_weights
    @torch.no_grad()
    def __call__(self, image, mask_image, num_inference_steps=250, eta=0.0, jump_length=10, jump_n_sample=10, generator=None,
                 output_type="pil", return_dict=True, batch_size=None, init=None, known_shift=None, save_every_step=False, **kwargs):
        original = self._tensor(image, "image").detach().to(self.device, torch.float32)
        mask = self._tensor(mask_image, "mask_image").detach().to(self.device, torch.float32)
        if known_shift is not None:
            known_shift = self._tensor(known_shift, "known_shift").detach().to(self.device, torch.float32)
        if original.dim() == 3:
            original = original[None]
        if original.dim() != 4:
            raise ValueError(f"RePaintPipeline: image must be [B,C,H,W], [1,C,H,W] or [C,H,W], got {tuple(original.shape)}")
        if isinstance(generator, (list, tuple)):
            raise NotImplementedError("RePaintPipeline: per-sample generator lists are not supported")
        if init is not None:
            batch_size = init.shape[0]
        elif batch_size is None:
            batch_size = original.shape[0]
        if original.shape[0] not in (1, batch_size):
            raise ValueError(f"RePaintPipeline: image batch {original.shape[0]} does not match {batch_size} chains")
        shape = (batch_size,) + tuple(original.shape[1:])
        if init is None:
            x = randn_tensor(shape, generator=generator, device=self.device)
        else:
            x = init.detach().clone().to(self.device)
            if tuple(x.shape) != shape:
                raise ValueError(f"RePaintPipeline: init {tuple(x.shape)} does not match the image {shape}")
        x = ops.nchw_to_nhwc(x.float())                                   # NHWC storage, as the UNet consumes and produces it
        self.scheduler.set_timesteps(num_inference_steps, jump_length, jump_n_sample)
        self.scheduler.eta = eta
        mov = [self._to_numpy(x, shape)] if save_every_step else []
        ts_host = [int(t) for t in self.scheduler.timesteps]
        ts_dev = torch.as_tensor(ts_host, dtype=torch.int64).to(self.device)      # one H2D copy for the whole chain
        t_last = ts_host[0] + 1
        for i, t in enumerate(self.progress_bar(ts_host)):
            xl = x.permute(0, 3, 1, 2)
            if t < t_last:
                eps = self.unet(xl, ts_dev[i]).sample
                x = self.scheduler.step(eps, t, xl, original, mask, generator=generator, shift=known_shift).prev_sample.permute(0, 2, 3, 1)
            else:
                x = self.scheduler.undo_step(xl, t_last, generator=generator, shift=known_shift).permute(0, 2, 3, 1)
            t_last = t
            if save_every_step:
                mov.append(self._to_numpy(x, shape))
        return self._finish(x, shape, mov, output_type, save_every_step, return_dict)
