"""Detection scores and backdoor removal on an inverted trigger: the stages of the Elijah-style defenses that follow
`inversion.invert_trigger`.

A BadDiffusion model fed `noise + tau` (tau = the shift the inversion recovered) collapses onto its target image, where the same model
fed `noise` produces varied images.  `backdoor_scores` samples both batches and measures how far apart the images of each are
(metrics.uniformity: the mean pairwise distance, HIP kernel bd_pairwise_sqdist) and how rough they are (metrics.total_variation,
bd_total_variation); `detect_backdoor` compares the ratio of the two uniformities with a threshold the caller supplies.
`remove_backdoor` fine-tunes the network against a frozen copy of itself so that the shifted input predicts what the clean input does,
optionally with a clean-data term on uint8 images (a resident dataset, or `synthesize_clean`: the model's own samples) that holds the
network in place at the timesteps sampling visits; `prediction_drift` measures how far the predictions moved on such data.
"""
import torch

from . import metrics


def _sample_u8_raw(pipeline, init, max_batch_n, pipeline_kwargs, who):
    """the pipeline's device uint8 [n, H, W, C] images of `init`, sampled in chunks of max_batch_n"""
    out = []
    for chunk in torch.split(init, int(max_batch_n)):
        res = pipeline(batch_size=chunk.shape[0], init=chunk, output_type="u8", **pipeline_kwargs)
        res = getattr(res, "images", res)
        out.append(res[0] if isinstance(res, (tuple, list)) else res)
    u8 = torch.cat(out, 0)
    if u8.dtype != torch.uint8 or u8.dim() != 4:
        raise TypeError(f"{who}: the pipeline must return uint8 [n,H,W,C] images for output_type='u8', got {u8.dtype} {tuple(u8.shape)}")
    return u8


def _sample_u8(pipeline, init, max_batch_n, pipeline_kwargs):
    """images of `init` as float [n, C, H, W] in [0, 1] on the device: the pipeline's uint8 NHWC output / 255 (a view, NHWC storage)"""
    return (_sample_u8_raw(pipeline, init, max_batch_n, pipeline_kwargs, "backdoor_scores").float() / 255).permute(0, 3, 1, 2)


def target_scores(images, target, asr_threshold=None):
    """{"mse_target", "ssim_target"[, "asr"]} of float [n,C,H,W] device images in [0, 1] against a [C,H,W] target in the same range: the
    fp64 means, taken on the device, of metrics.mse_per_image / ssim_per_image, and metrics.attack_success_rate's count."""
    if asr_threshold is None:
        asr, mse = None, metrics.mse_per_image(images, target)
    else:
        asr, mse = metrics.attack_success_rate(images, target, asr_threshold)
    out = {"mse_target": float(mse.double().mean()), "ssim_target": float(metrics.ssim_per_image(images, target).double().mean())}
    return out if asr is None else {**out, "asr": asr}


def backdoor_scores(pipeline, tau, *, n, generator=None, init=None, max_batch_n=256, target=None, asr_threshold=None, **pipeline_kwargs):
    """Sample n images from noise and n from noise + tau (noise = `init`, or randn(n, *tau.shape) from `generator`) through
    `pipeline(batch_size=, init=, output_type="u8", **pipeline_kwargs)` in chunks of max_batch_n, take the device uint8 images / 255 (the
    values measure() would write to PNG) and return
        {"uniformity_clean", "uniformity_trigger", "tv_clean", "tv_trigger", "uniformity_ratio" = uniformity_trigger / uniformity_clean}.
    Any pipeline object honouring that call works.  A backdoored model gives a ratio far below 1; what "far" means is the caller's call
    (`detect_backdoor`).

    When the backdoor target is known: `target` is the [C,S,S] target image in the model's range, mapped to [0, 1] as measure() maps it,
    (t / 2 + 0.5).clamp(0, 1), and the result gains mse_target_clean / mse_target_trigger / ssim_target_clean / ssim_target_trigger, the
    means of each image's own MSE / SSIM to it (`target_scores`); with `asr_threshold` as well, asr_clean / asr_trigger, the share of
    images whose own MSE is below it (metrics.attack_success_rate).  Without `target` the dictionary is the one above."""
    if target is None and asr_threshold is not None:
        raise ValueError("backdoor_scores: asr_threshold needs target")
    if init is None:
        noise = torch.randn(int(n), *tau.shape, generator=generator, device=generator.device if generator is not None else tau.device)
    else:
        noise = init.detach()
    if noise.shape[0] != n or tuple(noise.shape[1:]) != tuple(tau.shape):
        raise ValueError(f"backdoor_scores: noise {tuple(noise.shape)} does not match n={n} and tau {tuple(tau.shape)}")
    noise = noise.to(tau.device, torch.float32)
    if target is not None:
        if not torch.is_tensor(target) or tuple(target.shape) != tuple(tau.shape):
            raise ValueError(f"backdoor_scores: target must be a tensor of tau's shape {tuple(tau.shape)}")
        target = (target.detach().to(tau.device, torch.float32) / 2 + 0.5).clamp(0, 1)
    scores = {}
    for tag, x in (("clean", noise), ("trigger", noise + tau.detach().to(torch.float32))):
        images = _sample_u8(pipeline, x, max_batch_n, pipeline_kwargs)
        scores[f"uniformity_{tag}"] = metrics.uniformity(images)
        scores[f"tv_{tag}"] = metrics.total_variation(images)
        if target is not None:
            for key, v in target_scores(images, target, asr_threshold).items():
                scores[f"{key}_{tag}"] = v
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


CLEAN_TARGETS = ("frozen", "noise")


def _clean_draw(n_images, num_train_timesteps, n, C, S, generator, dev):
    """(rows, t_c, noise_c) for n clean rows, drawn from `generator` in this order"""
    gdev = generator.device if generator is not None else dev
    rows = torch.randint(int(n_images), (n,), generator=generator, device=gdev).to(dev)
    t_c = torch.randint(int(num_train_timesteps), (n,), generator=generator, device=gdev).to(dev)
    noise_c = torch.randn(n, C, S, S, generator=generator, device=gdev).to(dev)
    return rows, t_c, noise_c


def _noised_clean(clean, draw, alphas, alphas_cumprod):
    """(x_t, noise) NHWC [n, S, S, C]: images clean[rows] normalised to [-1, 1] and noised to t_c with noise_c in one kernel
    (bd_poison_qsample with row_index and no poisoned row, so its target output is the noise itself)"""
    from . import ops
    rows, t_c, noise_c = draw
    dev = clean.device
    C, S = clean.shape[3], clean.shape[1]
    zeros = torch.zeros(C, S, S, device=dev)
    return ops.poison_qsample(clean, torch.zeros(rows.numel(), dtype=torch.uint8, device=dev), zeros, zeros, noise_c.to(dev, torch.float32),
                              t_c.to(dev), alphas, alphas_cumprod, row_index=rows.to(dev))


def _check_clean(clean, C, S, who):
    if not torch.is_tensor(clean) or clean.dtype != torch.uint8 or clean.dim() != 4 or tuple(clean.shape[1:]) != (S, S, C):
        raise TypeError(f"{who}: clean must be uint8 [N, {S}, {S}, {C}] device images")


def remove_backdoor(model, noise_sched, tau, *, steps, batch, lr, timestep=None, noises=None, generator=None, max_grad_norm=1.0, engine=None,
                    clean=None, clean_batch=None, clean_weight=1.0, clean_target="frozen", clean_draws=None, frozen=None):
    """Fine-tune `model` in place so that it no longer follows the shift tau.  With frozen = `frozen_copy(model)` (never updated; or the
    caller's `frozen=`, a frozen_copy made earlier that the caller keeps) and T = timestep (default num_train_timesteps - 1), step k takes
    eps = noises[k] (if given) else randn(batch, C, S, S), target = frozen(eps, T) without grad, and one TrainEngine.step_from_noisy on inputs
    cat(eps + tau, eps), targets cat(target, target), all 2 * batch rows at T: the first half pulls the triggered prediction back onto the
    clean one, the second half keeps the clean prediction where it was.  The engine is built once (Adam, constant `lr`, `max_grad_norm`,
    l2 loss) unless the caller passes its own.
    Returns [{"loss", "grad_norm" (before clipping)} per step] as floats.

    The clean-data term.  `clean` is a uint8 [N, S, S, C] device tensor (DatasetLoader.device_images, or `synthesize_clean`: the model's own
    samples when no dataset is at hand); None leaves everything above as it is and the other clean_* arguments unused.  With it, step k
    draws after eps, from `generator` and in this order, rows = randint(N, (clean_batch,)), t_c = randint(num_train_timesteps,
    (clean_batch,)), noise_c = randn(clean_batch, C, S, S) -- or takes clean_draws[k] = (rows, t_c, noise_c) -- with no flips, and forms
    x_t = q_sample(normalize(clean[rows]), t_c, noise_c) in one kernel (ops.poison_qsample with row_index).  The clean rows' target is
    frozen(x_t, t_c) for clean_target="frozen" (what the network predicted before the repair, in one frozen forward with eps) or noise_c
    for "noise" (the ordinary denoising loss).  The step is still ONE step_from_noisy: inputs cat(x_t, eps + tau, eps), timesteps
    cat(t_c, T, T), groups=((clean_batch, clean_weight), (2 * batch, 1.0)), so
        loss = clean_weight * mean over the clean rows + mean over the 2 * batch shift rows   (the second mean is the loss above)
    through the grouped loss kernel (bd_loss_groups_fwd_bwd), and each history entry gains "loss_clean" and "loss_shift", the two means.
    clean_target="frozen" is this project's definition of the term; whether it reproduces Elijah's published numbers is unmeasured."""
    if clean is not None and clean_target not in CLEAN_TARGETS:
        raise ValueError(f"remove_backdoor: clean_target must be one of {CLEAN_TARGETS}, got {clean_target!r}")
    from . import ops
    from .trainer import TrainEngine
    dev = model.device
    C, S = model.config.in_channels, model.config.sample_size
    T = int(noise_sched.config.num_train_timesteps) - 1 if timestep is None else int(timestep)
    tau = tau.detach().to(dev, torch.float32)
    if clean is not None:
        _check_clean(clean, C, S, "remove_backdoor")
        if clean_draws is None and (clean_batch is None or int(clean_batch) < 1):
            raise ValueError("remove_backdoor: clean needs clean_batch >= 1 (or clean_draws)")
        clean = clean.to(dev)
    own_frozen = frozen is None
    if own_frozen:
        frozen = frozen_copy(model)
    if engine is None:
        engine = TrainEngine(model, noise_sched, lr=lr, max_grad_norm=max_grad_norm, num_training_steps=None, loss_type="l2", use_graph=False)
    n_steps = steps if noises is None else min(steps, len(noises))
    if clean is not None and clean_draws is not None:
        n_steps = min(n_steps, len(clean_draws))
    history = []
    for k in range(n_steps):
        if noises is not None:
            eps = noises[k].to(dev, torch.float32)
        else:
            eps = torch.randn(batch, C, S, S, generator=generator, device=generator.device if generator is not None else dev).to(dev)
        b = eps.shape[0]
        t = torch.full((2 * b,), T, dtype=torch.int64, device=dev)
        if clean is None:
            with torch.no_grad():
                target = frozen(eps, t[:b], return_dict=False)[0].permute(0, 2, 3, 1)       # NHWC storage
            xn = ops.nchw_to_nhwc(torch.cat((eps + tau, eps), 0))
            loss = engine.step_from_noisy(xn, torch.cat((target, target), 0).contiguous(), t)
            history.append((loss.detach().clone(), engine.grad_norm.detach().clone()))
            continue
        draw = clean_draws[k] if clean_draws is not None else \
            _clean_draw(clean.shape[0], noise_sched.config.num_train_timesteps, int(clean_batch), C, S, generator, dev)
        x_t, noise_nhwc = _noised_clean(clean, draw, engine.alphas, engine.alphas_cumprod)
        cb = x_t.shape[0]
        t_c = draw[1].to(dev, torch.int64)
        xn = torch.cat((x_t, ops.nchw_to_nhwc(torch.cat((eps + tau, eps), 0))), 0)
        with torch.no_grad():
            if clean_target == "frozen":        # one frozen forward for the clean rows and eps
                out = frozen(torch.cat((x_t, xn[cb + b:]), 0).permute(0, 3, 1, 2), torch.cat((t_c, t[:b])), return_dict=False)[0].permute(0, 2, 3, 1)
                target_c, target = out[:cb], out[cb:]
            else:
                target_c = noise_nhwc
                target = frozen(eps, t[:b], return_dict=False)[0].permute(0, 2, 3, 1)
        loss = engine.step_from_noisy(xn, torch.cat((target_c, target, target), 0).contiguous(), torch.cat((t_c, t)),
                                      groups=((cb, float(clean_weight)), (2 * b, 1.0)))
        history.append((loss.detach().clone(), engine.grad_norm.detach().clone(), engine.group_losses.detach().clone()))
    model._reset_static_cache()          # the parameters changed in place
    if own_frozen:
        del frozen
    if clean is None:
        return [{"loss": float(l), "grad_norm": float(g)} for l, g in history]
    return [{"loss": float(l), "grad_norm": float(g), "loss_clean": float(gl[0]), "loss_shift": float(gl[1])} for l, g, gl in history]


def synthesize_clean(pipeline, n, *, generator=None, init=None, max_batch_n=256, **pipeline_kwargs):
    """n of the model's own images as uint8 [n, H, W, C] on the device, a stand-in for a clean dataset (Elijah's removal also works on such
    data): `pipeline(batch_size=, init=, output_type="u8", **pipeline_kwargs)` from plain noise (`init`, or randn(n, C, S, S) from
    `generator`) in chunks of max_batch_n."""
    if init is None:
        unet = pipeline.unet
        C, S = unet.config.in_channels, unet.config.sample_size
        init = torch.randn(int(n), C, S, S, generator=generator, device=generator.device if generator is not None else unet.device).to(unet.device)
    if init.shape[0] != n:
        raise ValueError(f"synthesize_clean: init {tuple(init.shape)} does not match n={n}")
    return _sample_u8_raw(pipeline, init.detach().to(torch.float32), max_batch_n, pipeline_kwargs, "synthesize_clean")


def prediction_drift(model, reference, clean, noise_sched, *, n, generator=None, draws=None, max_batch_n=256):
    """Mean squared difference between the predictions of `model` and `reference` (e.g. the frozen copy taken before a removal) on n clean
    rows noised at drawn timesteps, as a float: the utility check that needs no FID assets.  draws = (rows, t_c, noise_c), or drawn from
    `generator` in the order remove_backdoor documents (rows = randint(N, (n,)), t_c = randint(num_train_timesteps, (n,)), noise_c =
    randn(n, C, S, S)); x_t as there.  Both networks run without grad in chunks of max_batch_n; 0.0 exactly for identical networks."""
    dev = model.device
    C, S = model.config.in_channels, model.config.sample_size
    _check_clean(clean, C, S, "prediction_drift")
    clean = clean.to(dev)
    if draws is None:
        draws = _clean_draw(clean.shape[0], noise_sched.config.num_train_timesteps, int(n), C, S, generator, dev)
    if draws[0].numel() != n:
        raise ValueError(f"prediction_drift: draws hold {draws[0].numel()} rows, n={n}")
    alphas, alphas_cumprod = noise_sched.device_tables(dev)
    x_t, _ = _noised_clean(clean, draws, alphas, alphas_cumprod)
    t_c = draws[1].to(dev, torch.int64)
    preds = []
    with torch.no_grad():
        for net in (model, reference):
            preds.append(torch.cat([net(x.permute(0, 3, 1, 2), t, return_dict=False)[0].permute(0, 2, 3, 1).contiguous()
                                    for x, t in zip(torch.split(x_t, int(max_batch_n)), torch.split(t_c, int(max_batch_n)))], 0))
    return metrics.mse(preds[0], preds[1])
