"""How good is a checkpoint on clean data?  The variational bound in bits per dimension, term by term, on the MI355X path.

    python likelihood_eval.py --ckpt <checkpoint dir> [--dataset CIFAR10] [--dataset_path datasets] [--n 16] [--batch 256] [--t_stride 1]
                              [--variance_type fixed_small|fixed_large] [--no_clip] [--target NAME [--trigger BOX_14] [--backdoor]]
                              [--output_dir DIR] [--seed 0] [--gpu 0]

The sibling of inpaint_eval.py.  The first --n images of the dataset are scored by likelihood.bits_per_dim (baddiffusion_amd/likelihood.py:
formulas, noise order, and the caveat that the decoder term uses the exact normal CDF, so totals differ in the third decimal from papers
that use improved-DDPM's tanh approximation).  A full evaluation is T = num_train_timesteps UNet evaluations per image.
  --t_stride K      evaluates t = 0, the prior and every K-th of t = 1 ... T-1 only and reports
                    estimate_bpd = prior + L_0 + K * (sum of the evaluated KL terms), an ESTIMATE of the bound ("complete": false); K = 1 is
                    the bound itself
  --variance_type   the model variance of the bound; default: the checkpoint's scheduler's
  --no_clip         x0_hat is not clamped to [-1, 1]
  --target NAME     a Backdoor target (HAT, CAT, CORNER, TRIGGER, SHIFT; --trigger matters for the relative ones) quantised to uint8 and
                    scored as one more row: "target_bpd" -- does the model assign the backdoor target a better code length than the data?
  --backdoor        (needs --target) also scores the --n rows as TRIGGERED rows along the backdoored chain of BadDiffusion
                    (likelihood.bits_per_dim(backdoor=...): the images are the carriers of --trigger, x0 is the target, x_t is shifted by
                    rho_t r): how many bits the model charges for the target when the trigger is present, on the same noise.  A perfectly
                    implanted backdoor scores (close to) 0 in its KL rows under --no_clip and fixed_small; WITHOUT --no_clip the figure is
                    the bound of the clamped sampler, under which it does not.  No really backdoored checkpoint has been scored with it yet.
Outputs in <output_dir>/<name>: config.json, likelihood.json ({"complete", "t_stride", "timesteps", "n", "variance_type", "clip_denoised",
"mean_bpd" (complete only), "estimate_bpd", "per_image", "prior_bpd", "l0_bpd"[, "target_bpd"][, "backdoor_bpd": {"mean_bpd" (complete
only), "estimate_bpd", "per_image", "prior_bpd", "l0_bpd", "clip_denoised"}]}) and likelihood_terms.npz (terms [len(timesteps) + 1, rows]
float32 with the prior last and the target row last, timesteps[, backdoor_terms [len(timesteps) + 1, n]]).  Without --backdoor every file
is what it was before the flag existed.  `--ckpt` must be a local diffusers-layout directory.
"""
import argparse
import json
import os
from dataclasses import dataclass
from typing import Union

import numpy as np
import torch

from baddiffusion_amd import likelihood
from baddiffusion_amd.model import DiffuserModelSched


@dataclass
class Config:
    ckpt: Union[str, os.PathLike] = None
    dataset: str = "CIFAR10"
    dataset_path: Union[str, os.PathLike] = "datasets"
    n: int = 16
    batch: int = 256
    t_stride: int = 1
    variance_type: str = None
    clip: bool = True
    target: str = None
    trigger: str = "BOX_14"
    backdoor: bool = False
    output_dir: Union[str, os.PathLike] = ""
    score_file: Union[str, os.PathLike] = "likelihood.json"
    terms_file: Union[str, os.PathLike] = "likelihood_terms.npz"
    seed: int = 0
    gpu: str = "0"


def naming_fn(config):
    return f"res_likelihood_n{config.n}_k{config.t_stride}_{os.path.basename(str(config.ckpt).rstrip('/'))}"


def get_config(argv=None):
    config = Config()
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--ckpt", "-c", type=str, required=True)
    p.add_argument("--dataset", "-ds", type=str, default=config.dataset)
    p.add_argument("--dataset_path", "-dp", type=str, default=config.dataset_path)
    p.add_argument("--n", type=int, default=config.n)
    p.add_argument("--batch", "-b", type=int, default=config.batch)
    p.add_argument("--t_stride", type=int, default=config.t_stride)
    p.add_argument("--variance_type", type=str, choices=list(likelihood.VARIANCE_TYPES))
    p.add_argument("--no_clip", action="store_true", help="do not clamp the predicted x0 to [-1, 1]")
    p.add_argument("--target", type=str, help="name of a backdoor target (Backdoor.get_target): scored as one more row")
    p.add_argument("--trigger", type=str, default=config.trigger, help="trigger name; needed only for the targets defined relative to the trigger")
    p.add_argument("--backdoor", action="store_true",
                   help="with --target: also score the rows as triggered rows along the backdoored chain (bits/dim of the target when the "
                        "trigger is present); with the clamp on (no --no_clip) this is the bound of the clamped sampler, under which a "
                        "perfect implant does not score 0")
    p.add_argument("--output_dir", "-od", type=str)
    p.add_argument("--seed", type=int, default=config.seed)
    p.add_argument("--gpu", "-g", type=str, default=config.gpu)
    args = p.parse_args(argv)
    no_clip = args.__dict__.pop("no_clip")
    for k, v in vars(args).items():
        if v is not None:
            setattr(config, k, v)
    config.clip = not no_clip
    if config.n < 1 or config.batch < 1 or config.t_stride < 1:
        p.error("--n, --batch and --t_stride must be positive")
    if config.backdoor and config.target is None:
        p.error("--backdoor needs --target (the image the triggered chain ends in)")
    config.output_dir = os.path.join(config.output_dir or "", naming_fn(config))
    os.makedirs(config.output_dir, exist_ok=True)
    with open(os.path.join(config.output_dir, "config.json"), "w") as f:
        # (the backdoor field appears only with --backdoor: without the flag the file is what it was before the flag existed)
        json.dump({k: v for k, v in config.__dict__.items() if config.backdoor or k != "backdoor"}, f, indent=2, default=str)
    return config


def clean_images(config, model, log=print):
    """the first --n dataset images as the resident uint8 [n, S, S, C] device array"""
    from baddiffusion_amd.dataset import DatasetLoader
    root = config.dataset_path if config.dataset_path and os.path.isdir(str(config.dataset_path)) else None
    dsl = DatasetLoader(root=root, name=config.dataset, channel=model.in_channels, image_size=model.sample_size, seed=config.seed,
                        device=model.device, num_images=config.n)
    log(f"data: {dsl.source}")
    return dsl.device_images[: config.n]


def target_u8(config, model):
    """the backdoor target quantised to uint8 [1, S, S, C] on the device, or None without --target"""
    if config.target is None:
        return None
    from baddiffusion_amd.dataset import Backdoor
    bd = Backdoor(root=config.dataset_path)
    trigger = bd.get_trigger(type=config.trigger, channel=model.in_channels, image_size=model.sample_size)
    target = bd.get_target(type=config.target, trigger=trigger).to(torch.float32)
    return ((target / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0)[None].contiguous().to(model.device)


def backdoor_pair(config, model):
    """(trigger, target) float32 [C, S, S] of --trigger / --target, as ops.poison_qsample takes them"""
    from baddiffusion_amd.dataset import Backdoor
    bd = Backdoor(root=config.dataset_path)
    trigger = bd.get_trigger(type=config.trigger, channel=model.in_channels, image_size=model.sample_size)
    return trigger.to(torch.float32), bd.get_target(type=config.target, trigger=trigger).to(torch.float32)


def summarise_backdoor(config, res):
    """the "backdoor_bpd" block of a bits_per_dim(backdoor=...) result"""
    out = summarise(config, res, res["terms"].shape[1])
    out = {k: out[k] for k in ("mean_bpd", "estimate_bpd", "per_image", "prior_bpd", "l0_bpd") if k in out}
    out["clip_denoised"] = bool(config.clip)
    return out


def summarise(config, res, n_clean):
    """the JSON block of a bits_per_dim result whose last row (with --target) is the target's"""
    est = likelihood.estimate_bpd(res["terms"], config.t_stride)
    out = {"complete": bool(res["complete"]), "t_stride": config.t_stride, "timesteps": len(res["timesteps"]), "n": n_clean,
           "estimate_bpd": float(est[:n_clean].mean()), "per_image": [float(v) for v in est[:n_clean]],
           "prior_bpd": float(res["terms"][-1, :n_clean].double().mean()), "l0_bpd": float(res["terms"][0, :n_clean].double().mean())}
    if res["complete"]:
        out["mean_bpd"] = float(res["sum_bpd"][:n_clean].mean())
    if est.numel() > n_clean:
        out["target_bpd"] = float(est[n_clean])
    return out


def main(argv=None):
    config = get_config(argv)
    model, noise_sched, _ = DiffuserModelSched.get_pretrained(ckpt=config.ckpt, clip_sample=None)
    model = model.cuda()
    clean = clean_images(config, model)
    n_clean = clean.shape[0]
    target = target_u8(config, model)
    if target is not None:
        clean = torch.cat((clean, target), 0)
    T = int(noise_sched.config.num_train_timesteps)
    res = likelihood.bits_per_dim(model, noise_sched, clean, timesteps=likelihood.strided_timesteps(T, config.t_stride),
                                  generator=torch.manual_seed(config.seed), max_batch_n=config.batch, clip_denoised=config.clip,
                                  variance_type=config.variance_type)
    result = summarise(config, res, n_clean)
    result["variance_type"] = config.variance_type or noise_sched.config.variance_type
    result["clip_denoised"] = bool(config.clip)
    arrays = {"terms": res["terms"].numpy(), "timesteps": np.asarray(res["timesteps"], dtype=np.int64)}
    if config.backdoor:
        res_bd = likelihood.bits_per_dim(model, noise_sched, clean[:n_clean], timesteps=likelihood.strided_timesteps(T, config.t_stride),
                                         generator=torch.manual_seed(config.seed), max_batch_n=config.batch, clip_denoised=config.clip,
                                         variance_type=config.variance_type, backdoor=backdoor_pair(config, model))
        result["backdoor_bpd"] = summarise_backdoor(config, res_bd)
        arrays["backdoor_terms"] = res_bd["terms"].numpy()
    label = "bits/dim" if result["complete"] else f"bits/dim (ESTIMATE from every {config.t_stride}-th timestep)"
    print(f"{label}: {result['estimate_bpd']:.6g}  (prior {result['prior_bpd']:.3g}, L_0 {result['l0_bpd']:.6g})"
          + (f", target {config.target}: {result['target_bpd']:.6g}" if "target_bpd" in result else ""))
    if config.backdoor:
        b = result["backdoor_bpd"]
        print(f"{label} of target {config.target} along the chain triggered by {config.trigger}: {b['estimate_bpd']:.6g}  (prior "
              f"{b['prior_bpd']:.3g}, L_0 {b['l0_bpd']:.6g}; {'clamped sampler' if config.clip else 'unclamped'})")
    print(json.dumps({k: ({j: w for j, w in v.items() if j != "per_image"} if isinstance(v, dict) else v) for k, v in result.items()
                      if k != "per_image"}))
    with open(os.path.join(config.output_dir, config.score_file), "w") as f:
        json.dump(result, f, indent=2)
    np.savez(os.path.join(config.output_dir, config.terms_file), **arrays)
    return result


if __name__ == "__main__":
    main()
