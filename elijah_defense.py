"""Elijah-style defense on the MI355X path: invert the trigger, score the checkpoint, remove the backdoor, score it again.

    python elijah_defense.py --ckpt <checkpoint dir> [--inv_steps 100] [--inv_batch 64] [--inv_lr 0.1] [--lam 0.5]
                             [--detect_n 256] [--sched DDIM-SCHED|DDPM-SCHED|DPM_SOLVER_{PP_,}O{1,2,3}-SCHED|UNIPC_O{1,2,3}-SCHED|DEIS_O{1,2,3}-SCHED|HEUN_O2-SCHED|LMSD_O{1,2,3,4}-SCHED|EULER_{A_,}O1-SCHED|KDPM2_{A_,}O2-SCHED] [--infer_steps 50] [--max_ratio R]
                             [--remove_steps 200] [--batch 64] [--learning_rate 2e-5] [--output_dir DIR] [--tag T] [--seed 0] [--gpu 0]
                             [--clean_source none|synthetic|dataset] [--clean_n 256] [--clean_batch 64] [--clean_weight 1.0]
                             [--clean_target frozen|noise] [--dataset CIFAR10] [--dataset_path datasets]
                             [--target NAME] [--trigger BOX_14] [--asr_threshold 1e-3] [--dyn_threshold V [--dyn_threshold_ratio 0.995]]
                             [--bpd_images N [--bpd_t_stride K] [--bpd_backdoor]]
                             [--correction ode|sde|ddim|ddpm [--correction_zeta Z] [--correction_steps N --correction_eta E]]

The sibling of anp_defense.py.  Stages (baddiffusion_amd/inversion.py, baddiffusion_amd/defense.py):
  1. invert_trigger: the shift tau the frozen network follows;
  2. backdoor_scores of the checkpoint on noise / noise + tau, and -- only when --max_ratio is given -- the verdict;
  3. remove_backdoor (skipped with --remove_steps 0); with --clean_source synthetic (the checkpoint's own samples, synthesize_clean) or
     dataset (DatasetLoader's resident uint8 images) it adds the clean-data term, and prediction_drift of the repaired model against the
     frozen copy taken before the removal, on the same clean images, is written as score.json["drift"];
  4. backdoor_scores of the repaired model on the same noise.
When the backdoor target is known, --target NAME (a Backdoor target: HAT, CAT, CORNER, TRIGGER, SHIFT; --trigger NAME, default BOX_14, matters
only for the targets defined relative to the trigger) adds to both score blocks the mean per-image MSE / SSIM to the target and the attack
success rate -- the share of generated images whose own MSE to the target is below --asr_threshold -- and the log states "ASR before ->
after": the direct statement that the repair worked.  The default threshold, 1e-3, is this project's choice of a value of the order the
papers use, not a finding.
--bpd_images N adds the utility figure that stands on its own: the variational bound in bits per dimension (likelihood.bits_per_dim) of the
checkpoint on N clean rows -- the first N of the clean-data term's images, or of the dataset (--dataset, default CIFAR10) without one --
before and after the removal, on the same noise, printed beside the drift and written as score.json["bpd"].  --bpd_t_stride K evaluates every
K-th timestep only and reports likelihood.estimate_bpd, marked as an estimate.  Without the flag nothing changes.
--bpd_backdoor (needs --bpd_images and --target) adds the figure that needs no samples: bits per dimension of the target along the chain
triggered by --trigger (likelihood.bits_per_dim(backdoor=...), the same N rows as carriers, the clamped sampler's bound), before and after the
removal on the same noise, printed and written as score.json["bpd"]["backdoor_before" / "backdoor_after"].  One expects a removal to RAISE
it -- the repaired model should charge more bits for the target when the trigger is present -- but nothing here has measured that: no
really backdoored checkpoint has been scored with it yet.
--correction KIND names the correction table the checkpoint was trained with (baddiffusion.py --correction, baddiffusion_amd/correction.py): the
inversion models mean eps_hat = c_T-1 * tau, so --lam then defaults to that table's entry at the last timestep (0.99998 for ode; the
reference's rho_T-1 is 0.5025, which the standing default 0.5 approximates).  An explicit --lam wins; without --correction nothing changes.
Outputs in <output_dir>/<name>: config.json, score.json ({"before", "after", "detected", "removal"[, "drift"][, "bpd"]}), tau.pt and the repaired model in the
diffusers layout (unet/, scheduler/), which DiffuserModelSched.get_trained loads.  `--ckpt` must be a local diffusers-layout directory.
"""
import argparse
import json
import os
from dataclasses import dataclass
from typing import Union

import torch

from baddiffusion_amd import defense
from baddiffusion_amd.inversion import invert_trigger
from baddiffusion_amd.model import DiffuserModelSched, save_scheduler, save_unet
from baddiffusion_amd.sched_names import ELIJAH_CHOICES as SCHED_CHOICES, SCHEDS


@dataclass
class Config:
    project: str = "elijah_test"
    ckpt: Union[str, os.PathLike] = None
    inv_steps: int = 100
    inv_batch: int = 64
    inv_lr: float = 0.1
    lam: float = 0.5
    detect_n: int = 256
    sched: str = DiffuserModelSched.DDIM_SCHED
    infer_steps: int = 50
    max_ratio: float = None
    remove_steps: int = 200
    clip: bool = True
    batch: int = 64
    learning_rate: float = 2e-5
    eval_max_batch: int = 256
    gpu: str = "0"
    tag: str = None
    output_dir: Union[str, os.PathLike] = ""
    score_file: Union[str, os.PathLike] = "score.json"
    seed: int = 0
    clean_source: str = "none"
    clean_n: int = 256
    clean_batch: int = 64
    clean_weight: float = 1.0
    clean_target: str = "frozen"
    dataset: str = None
    dataset_path: Union[str, os.PathLike] = "datasets"
    target: str = None
    trigger: str = "BOX_14"
    asr_threshold: float = None
    dyn_threshold: float = None
    dyn_threshold_ratio: float = 0.995
    bpd_images: int = None
    bpd_t_stride: int = 1
    bpd_backdoor: bool = False


DEFAULT_ASR_THRESHOLD = 1e-3    # of the order the papers use; a choice, not a finding


def correction_lam(args):
    """--lam under --correction: the table's entry at the last timestep, on the tables of the checkpoint's own scheduler (a checkpoint
    named by its hub id has no scheduler folder to read here: the google/ddpm-* checkpoints this project knows all carry DDPMScheduler's
    default tables, which stand in)"""
    from baddiffusion_amd import correction
    from baddiffusion_amd.model import load_scheduler
    from baddiffusion_amd.schedulers import DDPMScheduler
    d = os.path.join(str(args.ckpt), "scheduler")
    sched = load_scheduler(d) if os.path.isdir(d) else DDPMScheduler()
    if args.correction == "ddpm":
        return float(correction.reference_rho(sched.alphas, sched.alphas_cumprod)[-1])
    return float(correction.table_values(args.correction, sched, zeta=args.correction_zeta, steps=args.correction_steps,
                                         eta=args.correction_eta)[-1])


def naming_fn(config):
    add_on = f"_{config.tag}" if config.tag is not None else ""
    return (f"res_elijah_inv{config.inv_steps}_lam{config.lam}_rm{config.remove_steps}_lr{config.learning_rate}{add_on}_"
            f"{os.path.basename(str(config.ckpt).rstrip('/'))}")


def get_config(argv=None):
    config = Config()
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--project", "-pj", type=str)
    p.add_argument("--ckpt", "-c", type=str, required=True)
    p.add_argument("--inv_steps", type=int, default=config.inv_steps)
    p.add_argument("--inv_batch", type=int, default=config.inv_batch)
    p.add_argument("--inv_lr", type=float, default=config.inv_lr)
    p.add_argument("--lam", type=float,
                   help=f"the inversion models mean eps_hat = lam * tau at the last timestep ({config.lam}: the reference's rho_T-1 = 0.5025, "
                        "rounded; with --correction: that table's entry at the last timestep)")
    p.add_argument("--detect_n", type=int, default=config.detect_n)
    p.add_argument("--sched", "-sc", type=str, default=config.sched, choices=SCHED_CHOICES,
                   help="sampling pipeline of the score passes; the DPM_SOLVER_* names run DPMSolverMultistepScheduler (always the native solver here), "
                        "the UNIPC_O* names UniPCMultistepScheduler, the DEIS_O* names DEISMultistepScheduler, HEUN_O2 / LMSD_O* the sigma-space samplers, "
                        "EULER_O1 / EULER_A_O1 / KDPM2_O2 / KDPM2_A_O2 Euler, Euler-ancestral, KDPM2 and KDPM2-ancestral")
    p.add_argument("--infer_steps", "-is", type=int, default=config.infer_steps)
    p.add_argument("--max_ratio", type=float)
    p.add_argument("--remove_steps", type=int, default=config.remove_steps)
    p.add_argument("--batch", "-b", type=int, default=config.batch)
    p.add_argument("--learning_rate", "-lr", type=float, default=config.learning_rate)
    p.add_argument("--output_dir", "-od", type=str)
    p.add_argument("--tag", "-t", type=str)
    p.add_argument("--seed", type=int, default=config.seed)
    p.add_argument("--gpu", "-g", type=str, default=config.gpu)
    p.add_argument("--clean_source", type=str, default=config.clean_source, choices=["none", "synthetic", "dataset"])
    p.add_argument("--clean_n", type=int, default=config.clean_n)
    p.add_argument("--clean_batch", type=int, default=config.clean_batch)
    p.add_argument("--clean_weight", type=float, default=config.clean_weight)
    p.add_argument("--clean_target", type=str, default=config.clean_target, choices=list(defense.CLEAN_TARGETS))
    p.add_argument("--dataset", "-ds", type=str)
    p.add_argument("--dataset_path", "-dp", type=str, default=config.dataset_path)
    p.add_argument("--target", type=str, help="name of the known backdoor target (Backdoor.get_target): adds per-image target scores and the ASR")
    p.add_argument("--trigger", type=str, default=config.trigger, help="trigger name; needed only for the targets defined relative to the trigger")
    p.add_argument("--asr_threshold", type=float,
                   help="an image counts as a hit when its own MSE to the target is below this (needs --target; default 1e-3 once --target is "
                        "given: this project's choice of a value of the order the papers use, not a finding)")
    p.add_argument("--dyn_threshold", type=float,
                   help="score passes with dynamic thresholding of the predicted x0 in place of the fixed clamp: the sample_max_value of the "
                        "sampling scheduler (DDIM-SCHED / DDPM-SCHED only)")
    p.add_argument("--dyn_threshold_ratio", type=float, help="the quantile of --dyn_threshold (0.995)")
    p.add_argument("--bpd_images", type=int, help="bits per dimension (variational bound) of this many clean rows, before -> after the removal")
    p.add_argument("--bpd_t_stride", type=int, help="with --bpd_images: evaluate every K-th timestep and report the estimate (default 1: the bound)")
    p.add_argument("--bpd_backdoor", action="store_true",
                   help="with --bpd_images and --target: bits per dimension of the target along the chain triggered by --trigger, before -> "
                        "after the removal (one expects it to rise; not measured on a really backdoored checkpoint yet)")
    p.add_argument("--correction", type=str, choices=["ode", "sde", "ddim", "ddpm"],
                   help="the correction table the checkpoint was trained with (baddiffusion.py --correction): --lam then defaults to its "
                        "entry at the last timestep, c_T-1 (0.99998 for ode), since a model trained against eps + c_t R answers a shifted "
                        "input with mean eps_hat = c_T-1 * tau.  An explicit --lam wins")
    p.add_argument("--correction_zeta", type=float, help="zeta of --correction sde")
    p.add_argument("--correction_steps", type=int, help="steps of --correction ddim")
    p.add_argument("--correction_eta", type=float, help="eta of --correction ddim (0)")
    args = p.parse_args(argv)
    if args.correction is None and any(v is not None for v in (args.correction_zeta, args.correction_steps, args.correction_eta)):
        p.error("--correction_zeta / --correction_steps / --correction_eta need --correction")
    if args.correction is not None and args.lam is None:
        args.lam = correction_lam(args)
    if args.bpd_t_stride is not None and args.bpd_images is None:
        p.error("--bpd_t_stride needs --bpd_images")
    if args.bpd_backdoor and (args.bpd_images is None or args.target is None):
        p.error("--bpd_backdoor needs --bpd_images (the carrier rows) and --target (the image the triggered chain ends in)")
    if (args.bpd_images is not None and args.bpd_images < 1) or (args.bpd_t_stride is not None and args.bpd_t_stride < 1):
        p.error("--bpd_images and --bpd_t_stride must be positive")
    if args.dyn_threshold_ratio is not None and args.dyn_threshold is None:
        p.error("--dyn_threshold_ratio needs --dyn_threshold")
    for k, v in vars(args).items():
        if v is not None:
            setattr(config, k, v)
    DiffuserModelSched._check_dyn_threshold(config.sched, config.dyn_threshold, config.dyn_threshold_ratio)
    if config.clean_source == "dataset" and config.dataset is None:
        p.error("--clean_source dataset needs --dataset")
    if config.target is None and config.asr_threshold is not None:
        p.error("--asr_threshold needs --target")
    if config.target is not None and config.asr_threshold is None:
        config.asr_threshold = DEFAULT_ASR_THRESHOLD
    config.output_dir = os.path.join(config.output_dir or "", naming_fn(config))
    os.makedirs(config.output_dir, exist_ok=True)
    with open(os.path.join(config.output_dir, "config.json"), "w") as f:
        # (the bpd fields appear only with --bpd_images: without the flag the file is what it was before the flag existed)
        # (and bpd_backdoor only with --bpd_backdoor)
        json.dump({k: v for k, v in config.__dict__.items()
                   if (config.bpd_images is not None or not k.startswith("bpd_")) and (config.bpd_backdoor or k != "bpd_backdoor")}, f, indent=2,
                  default=str)
    return config


def make_pipeline(config, model, noise_sched):
    """the sampling pipeline of config.sched over the checkpoint's scheduler config; always the native scheduler of a name that has one"""
    rec = SCHEDS[config.sched]
    if not rec.dyn_threshold:
        noise_sched = rec.scheduler.from_config({**noise_sched.config, **rec.sched_kw})
    elif config.dyn_threshold is not None:
        # DDPM-SCHED, DDIM-SCHED: the checkpoint's scheduler as it is, unless thresholding asks for a sampling scheduler of its own --
        # the checkpoint's, which is saved back with the repaired model, keeps its config
        noise_sched = rec.scheduler(**noise_sched.config)
        DiffuserModelSched._set_dyn_threshold(noise_sched, config.dyn_threshold, config.dyn_threshold_ratio)
    return rec.pipeline(unet=model, scheduler=noise_sched, **rec.pipe_kw)


def invert(config, model, noise_sched, log=print):
    g = torch.Generator(device=model.device); g.manual_seed(config.seed)
    tau, losses = invert_trigger(model, steps=config.inv_steps, batch=config.inv_batch, lr=config.inv_lr, lam=config.lam,
                                 timestep=noise_sched.num_train_timesteps - 1, generator=g)
    log(f"inversion: loss {losses[0]:.6g} -> {losses[-1]:.6g}, |tau| {float(tau.norm()):.6g}")
    torch.save(tau.cpu(), os.path.join(config.output_dir, "tau.pt"))
    return tau


def detection_noise(config, model):
    """the one noise batch both score passes start from"""
    s = model.sample_size
    return torch.randn((config.detect_n, model.in_channels, s, s), generator=torch.manual_seed(config.seed))


def target_image(config, model):
    """the [C,S,S] backdoor target in the model's range at the checkpoint's channel count and size, or None without --target"""
    if config.target is None:
        return None
    from baddiffusion_amd.dataset import Backdoor
    bd = Backdoor(root=config.dataset_path)
    trigger = bd.get_trigger(type=config.trigger, channel=model.in_channels, image_size=model.sample_size)
    return bd.get_target(type=config.target, trigger=trigger)


def score(config, model, noise_sched, tau, noise, log=print, tag="before", target=None):
    known = {} if target is None else {"target": target.to(model.device), "asr_threshold": config.asr_threshold}
    sc = defense.backdoor_scores(make_pipeline(config, model, noise_sched), tau, n=config.detect_n, init=noise.to(model.device),
                                 max_batch_n=config.eval_max_batch, num_inference_steps=config.infer_steps, **known)
    log(f"[{tag}] " + json.dumps(sc))
    return sc


def clean_images(config, model, noise_sched, log=print):
    """uint8 [N, H, W, C] device images for the clean-data term: the checkpoint's own samples, or the first --clean_n rows of the dataset"""
    if config.clean_source == "synthetic":
        g = torch.Generator(device=model.device); g.manual_seed(config.seed + 2)
        clean = defense.synthesize_clean(make_pipeline(config, model, noise_sched), config.clean_n, generator=g, max_batch_n=config.eval_max_batch,
                                         num_inference_steps=config.infer_steps)
    else:
        from baddiffusion_amd.dataset import DatasetLoader
        root = config.dataset_path if config.dataset_path and os.path.isdir(str(config.dataset_path)) else None
        dsl = DatasetLoader(root=root, name=config.dataset, channel=model.in_channels, image_size=model.sample_size, seed=config.seed,
                            device=model.device, num_images=config.clean_n)
        clean = dsl.device_images[: config.clean_n]
        log(f"clean data: {dsl.source}")
    log(f"clean data: {config.clean_source}, {tuple(clean.shape)}")
    return clean


def remove(config, model, noise_sched, tau, log=print, clean=None, frozen=None):
    g = torch.Generator(device=model.device); g.manual_seed(config.seed + 1)
    if clean is None:
        history = defense.remove_backdoor(model, noise_sched, tau, steps=config.remove_steps, batch=config.batch, lr=config.learning_rate, generator=g)
    else:
        history = defense.remove_backdoor(model, noise_sched, tau, steps=config.remove_steps, batch=config.batch, lr=config.learning_rate, generator=g,
                                          clean=clean, clean_batch=config.clean_batch, clean_weight=config.clean_weight,
                                          clean_target=config.clean_target, frozen=frozen)
    log(f"removal: loss {history[0]['loss']:.6g} -> {history[-1]['loss']:.6g}")
    return history


def drift(config, model, frozen, clean, noise_sched, log=print):
    g = torch.Generator(device=model.device); g.manual_seed(config.seed + 3)
    d = defense.prediction_drift(model, frozen, clean, noise_sched, n=clean.shape[0], generator=g, max_batch_n=config.eval_max_batch)
    log(f"prediction drift on the clean data: {d:.6g}")
    return d


def bpd_rows(config, model, clean, log=print):
    """the uint8 [N, H, W, C] device rows --bpd_images scores: the first N of the clean-data term's images, else of the dataset"""
    n = config.bpd_images
    if clean is None:
        from baddiffusion_amd.dataset import DatasetLoader
        root = config.dataset_path if config.dataset_path and os.path.isdir(str(config.dataset_path)) else None
        dsl = DatasetLoader(root=root, name=config.dataset or "CIFAR10", channel=model.in_channels, image_size=model.sample_size,
                            seed=config.seed, device=model.device, num_images=n)
        log(f"bits/dim data: {dsl.source}")
        clean = dsl.device_images
    if clean.shape[0] < n:
        raise ValueError(f"--bpd_images {n}: only {clean.shape[0]} clean images are at hand")
    return clean[:n]


def backdoor_pair(config, model):
    """(trigger, target) float32 [C, S, S] of --trigger / --target, as ops.poison_qsample takes them"""
    from baddiffusion_amd.dataset import Backdoor
    bd = Backdoor(root=config.dataset_path)
    trigger = bd.get_trigger(type=config.trigger, channel=model.in_channels, image_size=model.sample_size)
    return trigger.to(torch.float32), bd.get_target(type=config.target, trigger=trigger).to(torch.float32)


def bpd(config, model, noise_sched, rows, backdoor=None):
    """mean bits per dimension of `rows` (the estimate of likelihood.estimate_bpd with --bpd_t_stride > 1), always on the same noise;
    backdoor: the (trigger, target) pair -- the rows are then the carriers of the triggered chain"""
    from baddiffusion_amd import likelihood
    g = torch.Generator(device=model.device); g.manual_seed(config.seed + 4)
    res = likelihood.bits_per_dim(model, noise_sched, rows, generator=g, max_batch_n=config.eval_max_batch,
                                  timesteps=likelihood.strided_timesteps(noise_sched.config.num_train_timesteps, config.bpd_t_stride),
                                  **({} if backdoor is None else {"backdoor": backdoor}))
    return float(likelihood.estimate_bpd(res["terms"], config.bpd_t_stride).mean()), bool(res["complete"])


def save_model(config, model, noise_sched):
    save_unet(model, os.path.join(config.output_dir, "unet"))
    save_scheduler(noise_sched, os.path.join(config.output_dir, "scheduler"))


def main(argv=None):
    config = get_config(argv)
    # the checkpoint's own scheduler carries the training tables and is saved back; --sched only picks the sampling pipeline
    model, noise_sched, _ = DiffuserModelSched.get_pretrained(ckpt=config.ckpt, clip_sample=config.clip)
    model = model.cuda()
    tau = invert(config, model, noise_sched)
    noise = detection_noise(config, model)
    target = target_image(config, model)
    result = {"before": score(config, model, noise_sched, tau, noise, tag="before", target=target), "after": None, "detected": None, "removal": []}
    if config.max_ratio is not None:
        result["detected"] = bool(defense.detect_backdoor(result["before"], max_ratio=config.max_ratio))
        print(f"backdoor detected: {result['detected']} (uniformity_ratio {result['before']['uniformity_ratio']:.6g} vs {config.max_ratio})")
    clean = clean_images(config, model, noise_sched) if config.clean_source != "none" else None
    if config.bpd_images is not None:
        rows = bpd_rows(config, model, clean)
        result["bpd"] = {"n": config.bpd_images, "t_stride": config.bpd_t_stride}
        result["bpd"]["before"], result["bpd"]["complete"] = bpd(config, model, noise_sched, rows)
        if config.bpd_backdoor:
            pair = backdoor_pair(config, model)
            result["bpd"]["backdoor_before"] = bpd(config, model, noise_sched, rows, backdoor=pair)[0]
    if config.clean_source != "none":
        # one frozen copy serves the removal (its targets) and the drift (the predictions before the repair)
        frozen = defense.frozen_copy(model)
        if config.remove_steps > 0:
            result["removal"] = remove(config, model, noise_sched, tau, clean=clean, frozen=frozen)
        result["drift"] = drift(config, model, frozen, clean, noise_sched)
        del frozen
    elif config.remove_steps > 0:
        result["removal"] = remove(config, model, noise_sched, tau)
    if config.bpd_images is not None:
        result["bpd"]["after"] = bpd(config, model, noise_sched, rows)[0]
        print(f"bits/dim of {config.bpd_images} clean rows before -> after: {result['bpd']['before']:.6g} -> {result['bpd']['after']:.6g}"
              + ("" if result["bpd"]["complete"] else f" (ESTIMATE from every {config.bpd_t_stride}-th timestep)"))
        if config.bpd_backdoor:
            result["bpd"]["backdoor_after"] = bpd(config, model, noise_sched, rows, backdoor=pair)[0]
            print(f"bits/dim of target {config.target} along the chain triggered by {config.trigger} ({config.bpd_images} carrier rows) before -> "
                  f"after: {result['bpd']['backdoor_before']:.6g} -> {result['bpd']['backdoor_after']:.6g}"
                  + ("" if result["bpd"]["complete"] else f" (ESTIMATE from every {config.bpd_t_stride}-th timestep)"))
    result["after"] = score(config, model, noise_sched, tau, noise, tag="after", target=target)
    if target is not None:
        print(f"ASR (MSE to {config.target} < {config.asr_threshold:g}) before -> after: {result['before']['asr_trigger']:.4f} -> "
              f"{result['after']['asr_trigger']:.4f}")
    if config.dyn_threshold is not None:
        result["dyn_threshold"], result["dyn_threshold_ratio"] = float(config.dyn_threshold), float(config.dyn_threshold_ratio)
    with open(os.path.join(config.output_dir, config.score_file), "w") as f:
        json.dump(result, f, indent=2)
    save_model(config, model, noise_sched)
    return result


if __name__ == "__main__":
    main()
