"""Detection scores and backdoor removal on an inverted trigger: the stages of the Elijah-style defenses that follow
`inversion.invert_trigger`.

A BadDiffusion model fed `noise + tau` (tau = the shift the inversion recovered) collapses onto its target image, where the same model
fed `noise` produces varied images.  `backdoor_scores` samples both batches and measures how far apart the images of each are
(metrics.uniformity: the mean pairwise distance, HIP kernel bd_pairwise_sqdist) and how rough they are (metrics.total_variation,
bd_total_variation); `detect_backdoor` compares the ratio of the two uniformities with a threshold the caller supplies.
`remove_backdoor` fine-tunes the network against a frozen copy of itself so that the shifted input predicts what the clean input does.
"""
import torch

from . import metrics


def _sample_u8(pipeline, init, max_batch_n, pipeline_kwargs):
    """images of `init` as float [n, C, H, W] in [0, 1] on the device: the pipeline's uint8 NHWC output / 255 (a view, NHWC storage)"""
    out = []
    for chunk in torch.split(init, int(max_batch_n)):
        res = pipeline(batch_size=chunk.shape[0], init=chunk, output_type="u8", **pipeline_kwargs)
        res = getattr(res, "images", res)
        out.append(res[0] if isinstance(res, (tuple, list)) else res)
    u8 = torch.cat(out, 0)
    if u8.dtype != torch.uint8 or u8.dim() != 4:
        raise TypeError(f"backdoor_scores: the pipeline must return uint8 [n,H,W,C] images for output_type='u8', got {u8.dtype} {tuple(u8.shape)}")
    return (u8.float() / 255).permute(0, 3, 1, 2)


def backdoor_scores(pipeline, tau, *, n, generator=None, init=None, max_batch_n=256, **pipeline_kwargs):
    """Sample n images from noise and n from noise + tau (noise = `init`, or randn(n, *tau.shape) from `generator`) through
    `pipeline(batch_size=, init=, output_type="u8", **pipeline_kwargs)` in chunks of max_batch_n, take the device uint8 images / 255 (the
    values measure() would write to PNG) and return
        {"uniformity_clean", "uniformity_trigger", "tv_clean", "tv_trigger", "uniformity_ratio" = uniformity_trigger / uniformity_clean}.
    Any pipeline object honouring that call works.  A backdoored model gives a ratio far below 1; what "far" means is the caller's call
    (`detect_backdoor`)."""
    if init is None:
        noise = torch.randn(int(n), *tau.shape, generator=generator, device=generator.device if generator is not None else tau.device)
    else:
        noise = init.detach()
    if noise.shape[0] != n or tuple(noise.shape[1:]) != tuple(tau.shape):
        raise ValueError(f"backdoor_scores: noise {tuple(noise.shape)} does not match n={n} and tau {tuple(tau.shape)}")
    noise = noise.to(tau.device, torch.float32)
    scores = {}
    for tag, x in (("clean", noise), ("trigger", noise + tau.detach().to(torch.float32))):
        images = _sample_u8(pipeline, x, max_batch_n, pipeline_kwargs)
        scores[f"uniformity_{tag}"] = metrics.uniformity(images)
        scores[f"tv_{tag}"] = metrics.total_variation(images)
    scores["uniformity_ratio"] = scores["uniformity_trigger"] / scores["uniformity_clean"]
    return scores


def detect_backdoor(scores, *, max_ratio):
    """True when the triggered batch is more than 1 / max_ratio times tighter than the clean one.  `max_ratio` has no default on purpose:
    Elijah fits its threshold on a zoo of clean and backdoored models, which this project does not have."""
    return scores["uniformity_ratio"] < max_ratio


def frozen_copy(model):
    """A second UNet2DModel of the same config, parameters and compute mode on the same device, for inference forwards only."""
    from .unet import UNet2DModel
    frozen = UNet2DModel(**dict(model.config), compute_mode=model.compute_mode, max_chunk=model.max_chunk).to(model.device)
    frozen.load_state_dict(model.state_dict())
    frozen.requires_grad_(False)
    return frozen


def remove_backdoor(model, noise_sched, tau, *, steps, batch, lr, timestep=None, noises=None, generator=None, max_grad_norm=1.0, engine=None):
    """Fine-tune `model` in place so that it no longer follows the shift tau.  With frozen = `frozen_copy(model)` (never updated) and
    T = timestep (default num_train_timesteps - 1), step k takes eps = noises[k] (if given) else randn(batch, C, S, S), target =
    frozen(eps, T) without grad, and one TrainEngine.step_from_noisy on inputs cat(eps + tau, eps), targets cat(target, target), all 2 * batch
    rows at T: the first half pulls the triggered prediction back onto the clean one, the second half keeps the clean prediction where it
    was.  The engine is built once (Adam, constant `lr`, `max_grad_norm`, l2 loss) unless the caller passes its own.
    Returns [{"loss", "grad_norm" (before clipping)} per step] as floats.
    Out of scope: a clean-data term (the denoising loss on real images Elijah adds) would need a dataset."""
    from . import ops
    from .trainer import TrainEngine
    dev = model.device
    C, S = model.config.in_channels, model.config.sample_size
    T = int(noise_sched.config.num_train_timesteps) - 1 if timestep is None else int(timestep)
    tau = tau.detach().to(dev, torch.float32)
    frozen = frozen_copy(model)
    if engine is None:
        engine = TrainEngine(model, noise_sched, lr=lr, max_grad_norm=max_grad_norm, num_training_steps=None, loss_type="l2", use_graph=False)
    history = []
    for k in range(steps if noises is None else min(steps, len(noises))):
        if noises is not None:
            eps = noises[k].to(dev, torch.float32)
        else:
            eps = torch.randn(batch, C, S, S, generator=generator, device=generator.device if generator is not None else dev).to(dev)
        t = torch.full((2 * eps.shape[0],), T, dtype=torch.int64, device=dev)
        with torch.no_grad():
            target = frozen(eps, t[: eps.shape[0]], return_dict=False)[0].permute(0, 2, 3, 1)       # NHWC storage
        xn = ops.nchw_to_nhwc(torch.cat((eps + tau, eps), 0))
        loss = engine.step_from_noisy(xn, torch.cat((target, target), 0).contiguous(), t)
        history.append((loss.detach().clone(), engine.grad_norm.detach().clone()))
    model._reset_static_cache()          # the parameters changed in place
    del frozen
    return [{"loss": float(l), "grad_norm": float(g)} for l, g in history]
