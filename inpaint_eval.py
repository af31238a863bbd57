"""Does a backdoor survive when the model is used as an inpainting prior?  RePaint on the MI355X path, clean and triggered.

    python inpaint_eval.py --ckpt <checkpoint dir> [--dataset CIFAR10] [--dataset_path datasets] [--n 16] [--batch 16] [--mask box|half]
                           [--infer_steps 250] [--jump_length 10] [--jump_n_sample 10] [--eta 0.0] [--trigger BOX_14] [--target NAME]
                           [--asr_threshold 1e-3] [--consistent] [--output_dir DIR] [--seed 0] [--gpu 0]

The sibling of elijah_defense.py.  The first --n images of the dataset are inpainted twice by RePaintPipeline (baddiffusion_amd/pipelines.py)
from the SAME noise: once from the noise itself ("clean"), once from noise + trigger ("trigger": how BadDiffusion's backdoor is set off).
With --consistent the triggered run also passes known_shift = trigger, so the re-noised known region and the undo steps follow the poisoned
forward process instead of the plain one.  --mask box makes the centred S/2 x S/2 square the hole, --mask half the right half.
Outputs in <output_dir>/<name>: config.json, clean.png / trigger.png (a grid of each run) and score.json:
  hole_share                                   the share of the image that is inpainted
  mse_clean, mse_trigger, ssim_clean, ssim_trigger
                                               means of every image's own MSE / SSIM to its original, on [0, 1] images.  The known region of
                                               the result equals the original exactly (alpha_prod_prev = 1 at the last step), so the MSE over
                                               the hole alone is this value / hole_share
  with --target NAME (a Backdoor target: HAT, CAT, CORNER, TRIGGER, SHIFT), through defense.target_scores:
  mse_target_*, ssim_target_*, asr_*           per-image scores against the backdoor target and the share of images whose own MSE to it is
                                               below --asr_threshold (default 1e-3 once --target is given: a choice, not a finding)
`--ckpt` must be a local diffusers-layout directory.
"""
import argparse
import json
import os
from dataclasses import dataclass
from typing import Union

import torch

from anp_defense import save_grid
from baddiffusion_amd import defense, metrics
from baddiffusion_amd.model import DiffuserModelSched
from baddiffusion_amd.pipelines import RePaintPipeline

DEFAULT_ASR_THRESHOLD = 1e-3    # of the order the papers use; a choice, not a finding
MASKS = ("box", "half")


@dataclass
class Config:
    ckpt: Union[str, os.PathLike] = None
    dataset: str = "CIFAR10"
    dataset_path: Union[str, os.PathLike] = "datasets"
    n: int = 16
    batch: int = 16
    mask: str = "box"
    infer_steps: int = 250
    jump_length: int = 10
    jump_n_sample: int = 10
    eta: float = 0.0
    trigger: str = "BOX_14"
    target: str = None
    asr_threshold: float = None
    consistent: bool = False
    clip: bool = True
    output_dir: Union[str, os.PathLike] = ""
    score_file: Union[str, os.PathLike] = "score.json"
    seed: int = 0
    gpu: str = "0"


def naming_fn(config):
    return (f"res_inpaint_{config.mask}_is{config.infer_steps}_j{config.jump_length}x{config.jump_n_sample}_eta{config.eta}"
            f"{'_consistent' if config.consistent else ''}_{os.path.basename(str(config.ckpt).rstrip('/'))}")


def get_config(argv=None):
    config = Config()
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--ckpt", "-c", type=str, required=True)
    p.add_argument("--dataset", "-ds", type=str, default=config.dataset)
    p.add_argument("--dataset_path", "-dp", type=str, default=config.dataset_path)
    p.add_argument("--n", type=int, default=config.n)
    p.add_argument("--batch", "-b", type=int, default=config.batch)
    p.add_argument("--mask", type=str, default=config.mask, choices=list(MASKS))
    p.add_argument("--infer_steps", "-is", type=int, default=config.infer_steps)
    p.add_argument("--jump_length", type=int, default=config.jump_length)
    p.add_argument("--jump_n_sample", type=int, default=config.jump_n_sample)
    p.add_argument("--eta", type=float, default=config.eta)
    p.add_argument("--trigger", type=str, default=config.trigger)
    p.add_argument("--target", type=str, help="name of the known backdoor target (Backdoor.get_target): adds per-image target scores and the ASR")
    p.add_argument("--asr_threshold", type=float, help="needs --target; default 1e-3 once --target is given")
    p.add_argument("--consistent", action="store_true", help="the triggered run re-noises the known region as a poisoned chain (known_shift)")
    p.add_argument("--output_dir", "-od", type=str)
    p.add_argument("--seed", type=int, default=config.seed)
    p.add_argument("--gpu", "-g", type=str, default=config.gpu)
    p.add_argument("--dyn_threshold", type=float, help="refused: see --help of baddiffusion.py; RePaint has no dynamic thresholding")
    p.add_argument("--dyn_threshold_ratio", type=float, help="refused with --dyn_threshold")
    args = p.parse_args(argv)
    if args.dyn_threshold is not None or args.dyn_threshold_ratio is not None:
        # the flag of baddiffusion.py and elijah_defense.py is known here so that a shared command line fails with the reason
        raise NotImplementedError("--dyn_threshold: inpainting samples through RePaintScheduler, which has no dynamic thresholding in the "
                                  "reference and none here; it runs in the DDPM and DDIM steps only (--fclip's fixed clamp applies)")
    for k, v in vars(args).items():
        if v is not None:
            setattr(config, k, v)
    if config.n < 1 or config.batch < 1:
        p.error("--n and --batch must be positive")
    if config.target is None and config.asr_threshold is not None:
        p.error("--asr_threshold needs --target")
    if config.target is not None and config.asr_threshold is None:
        config.asr_threshold = DEFAULT_ASR_THRESHOLD
    config.output_dir = os.path.join(config.output_dir or "", naming_fn(config))
    os.makedirs(config.output_dir, exist_ok=True)
    with open(os.path.join(config.output_dir, "config.json"), "w") as f:
        json.dump({k: v for k, v in config.__dict__.items()}, f, indent=2, default=str)
    return config


def make_mask(kind, size):
    """[1,1,S,S] float mask, 0 = hole: the centred S/2 x S/2 square ('box') or the right half ('half')"""
    m = torch.ones(1, 1, size, size)
    if kind == "box":
        lo = size // 4
        m[:, :, lo: lo + size // 2, lo: lo + size // 2] = 0
    elif kind == "half":
        m[:, :, :, size // 2:] = 0
    else:
        raise ValueError(f"mask {kind}: one of {MASKS}")
    return m


def originals(config, model):
    """the first --n dataset images, normalised to the model's range: float [n,C,S,S] on the device"""
    from baddiffusion_amd.dataset import DatasetLoader
    root = config.dataset_path if config.dataset_path and os.path.isdir(str(config.dataset_path)) else None
    dsl = DatasetLoader(root=root, name=config.dataset, channel=model.in_channels, image_size=model.sample_size, seed=config.seed,
                        device=model.device, num_images=config.n)
    print(f"data: {dsl.source}")
    return dsl._transform(dsl.device_images[: config.n])


def backdoor_images(config, model):
    """(trigger [C,S,S], target [C,S,S] or None) in the model's range"""
    from baddiffusion_amd.dataset import Backdoor
    bd = Backdoor(root=config.dataset_path)
    trigger = bd.get_trigger(type=config.trigger, channel=model.in_channels, image_size=model.sample_size)
    return trigger, (None if config.target is None else bd.get_target(type=config.target, trigger=trigger))


def inpaint(config, pipe, images, mask, init, known_shift=None):
    """device float [n,C,S,S] results in [0, 1] (the pipeline's uint8 output / 255), in chunks of --batch"""
    out = []
    for s in range(0, images.shape[0], config.batch):
        u8 = pipe(images[s: s + config.batch], mask, num_inference_steps=config.infer_steps, eta=config.eta, jump_length=config.jump_length,
                  jump_n_sample=config.jump_n_sample, init=init[s: s + config.batch], known_shift=known_shift, output_type="u8").images
        out.append(u8)
    return (torch.cat(out, 0).float() / 255).permute(0, 3, 1, 2)


def main(argv=None):
    config = get_config(argv)
    model, noise_sched, _ = DiffuserModelSched.get_pretrained(ckpt=config.ckpt, clip_sample=config.clip)
    model = model.cuda()
    pipe = RePaintPipeline(unet=model, scheduler=noise_sched)
    images = originals(config, model)
    n = images.shape[0]
    mask = make_mask(config.mask, model.sample_size).to(model.device)
    trigger, target = backdoor_images(config, model)
    trigger = trigger.to(model.device, torch.float32)
    noise = torch.randn((n, model.in_channels, model.sample_size, model.sample_size), generator=torch.manual_seed(config.seed)).to(model.device)
    orig01 = (images / 2 + 0.5).clamp(0, 1)
    if target is not None:
        target = (target.to(model.device, torch.float32) / 2 + 0.5).clamp(0, 1)
    result = {"hole_share": float((mask == 0).float().mean())}
    for tag, init, shift in (("clean", noise, None), ("trigger", noise + trigger, trigger if config.consistent else None)):
        out = inpaint(config, pipe, images, mask, init, known_shift=shift)
        result[f"mse_{tag}"] = float(metrics.mse_per_image(out, orig01).double().mean())
        result[f"ssim_{tag}"] = float(metrics.ssim_per_image(out, orig01).double().mean())
        if target is not None:
            for key, v in defense.target_scores(out, target, config.asr_threshold).items():
                result[f"{key}_{tag}"] = v
        save_grid(out.permute(0, 2, 3, 1).cpu().numpy(), os.path.join(config.output_dir, f"{tag}.png"))
    print(json.dumps(result))
    with open(os.path.join(config.output_dir, config.score_file), "w") as f:
        json.dump(result, f, indent=2)
    return result


if __name__ == "__main__":
    main()
