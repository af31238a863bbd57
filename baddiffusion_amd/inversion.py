"""Trigger inversion: the inversion stage of the Elijah-style defenses against backdoored diffusion models.

A BadDiffusion backdoor makes the network's noise prediction follow a shift of the initial noise.  `invert_trigger` optimises such a
shift `tau` through the FROZEN network: it needs nothing but d loss / d x, which `UNet2DModel` provides with its data-gradient-only
backward (bd_unet_backward_input with grads == NULL: no weight gradient is computed in any of the passes).  Detection scores and
backdoor removal built on the inverted trigger are in defense.py; this module states the optimisation below and nothing more.
"""
import torch


def invert_trigger(model, *, steps=100, batch=64, lr=0.1, lam=0.5, timestep=999, tau0=None, noises=None, generator=None,
                   optimizer=None):
    """Per step k:  x = noises[k] (if given) else randn(batch, C, S, S);  eps = model(x + tau, T) with T = timestep for every sample;
    m = eps.mean(0);  loss = mean((m - lam * tau)^2);  tau <- optimizer([tau]) step  (a factory; default Adam(lr)).

    The model's parameters are frozen for the duration and their requires_grad flags restored afterwards (`flat.grad` is not
    touched), so every backward is the data-gradient-only schedule.  Returns (tau [C, S, S], [loss_k as floats])."""
    dev = model.device
    C, S = model.config.in_channels, model.config.sample_size
    tau = torch.zeros(C, S, S, device=dev) if tau0 is None else tau0.detach().to(dev, torch.float32).clone()
    tau.requires_grad_(True)
    opt = torch.optim.Adam([tau], lr=lr) if optimizer is None else optimizer([tau])
    flags = [(p, p.requires_grad) for p in model.parameters()]
    losses = []
    try:
        for p, _ in flags:
            p.requires_grad_(False)
        T = torch.full((batch if noises is None else noises[0].shape[0],), int(timestep), dtype=torch.int64, device=dev)
        for k in range(steps if noises is None else min(steps, len(noises))):
            if noises is not None:
                x = noises[k].to(dev, torch.float32)
            else:
                x = torch.randn(batch, C, S, S, generator=generator, device=generator.device if generator is not None else dev).to(dev)
            if T.numel() != x.shape[0]:
                T = torch.full((x.shape[0],), int(timestep), dtype=torch.int64, device=dev)
            eps = model(x + tau, T, return_dict=False)[0]
            loss = ((eps.mean(0) - lam * tau) ** 2).mean()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
    finally:
        for p, f in flags:
            p.requires_grad_(f)
    return tau.detach(), [float(v) for v in losses]
