"""GPU: baddiffusion.py's train loop with --use_ema on a small network -- the in-training samples come from the averaged weights and the
raw ones are back afterwards, the checkpoint holds both, log.jsonl carries ema_decay, and --mode sampling --use_ema loads unet_ema."""
import dataclasses
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


def test_train_loop_with_use_ema(gpu, tmp_path, monkeypatch):
    import baddiffusion as cli
    from baddiffusion_amd.dataset import DatasetLoader
    from baddiffusion_amd.model import load_unet
    from baddiffusion_amd.pipelines import DDIMPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler
    from baddiffusion_amd.unet import unet_from_config
    cfg_net = dataclasses.replace(C.SMALL_CFGS["small"], sample_size=32)
    model = unet_from_config(cfg_net).to(gpu)
    model.load_state_dict(U.gen_params(cfg_net, 7))
    dsl = DatasetLoader(root=None, name=DatasetLoader.CIFAR10, batch_size=4, seed=0, device=gpu, num_images=16)
    dsl.set_poison(trigger_type="BOX_14", target_type="CORNER", clean_rate=1.0, poison_rate=0.25).prepare_dataset(mode="FIXED")
    config = cli.TrainingConfig()
    config.mode, config.dataset, config.ckpt, config.sched = cli.MODE_TRAIN, "CIFAR10", "local", None
    config.output_dir = str(tmp_path / "run"); os.makedirs(config.output_dir)
    config.ckpt_path = os.path.join(config.output_dir, config.ckpt_dir)
    config.data_ckpt_path = os.path.join(config.output_dir, config.data_ckpt_dir)
    config.batch, config.epoch, config.gradient_accumulation_steps, config.learning_rate, config.lr_warmup_steps = 4, 1, 1, 1e-3, 2
    config.clip, config.sample_ep, config.eval_sample_n, config.eval_max_batch, config.seed = False, None, 4, 4, 0
    config.use_ema = True
    # what the sampling inside the loop sees: record the weights the pipeline runs on
    seen = []
    real_sampling = cli.sampling

    def spy(cfg, name, pipeline, d):
        seen.append(pipeline.unet.flat.detach().clone())
        return real_sampling(cfg, name, pipeline, d)
    monkeypatch.setattr(cli, "sampling", spy)
    torch.manual_seed(3)
    get_pipeline = lambda unet, scheduler: DDIMPipeline(unet, scheduler)         # 50 DDIM steps: the loop's sampling stays short
    cli.train_loop(config, model, DDPMScheduler(clip_sample=False), get_pipeline, dsl, gpu, 1, 0)
    raw = model.flat.detach().cpu()
    files = set(os.listdir(config.output_dir))
    assert {"unet", "unet_ema", "scheduler", "model_index.json", "log.jsonl", "samples", "backdoor_samples", "ckpt"} <= files, files
    assert os.path.exists(os.path.join(config.ckpt_path, "ema.bin")) and os.path.exists(os.path.join(config.ckpt_path, "optimizer.bin"))
    st = torch.load(os.path.join(config.ckpt_path, "ema.bin"), map_location="cpu")
    assert st["optimization_step"] == 4 and st["use_ema_warmup"] is True and st["power"] == 0.75 and st["decay"] == 0.9999
    shadow = st["shadow_params"]
    mask = torch.ones(model.num_flat, dtype=torch.bool)
    for lo, hi in model._pads:
        mask[lo:hi] = False
    # the loop sampled on the averaged weights and put the raw ones back
    assert len(seen) == 1 and torch.equal(seen[0].cpu(), shadow) and not torch.equal(shadow, raw)
    assert torch.equal(load_unet(os.path.join(config.output_dir, "unet")).flat.detach()[mask], raw[mask])
    assert torch.equal(load_unet(os.path.join(config.output_dir, "unet_ema")).flat.detach()[mask], shadow[mask])
    log = [json.loads(ln) for ln in open(os.path.join(config.output_dir, "log.jsonl"))]
    assert log and log[0]["ema_decay"] == 0.0 and log[0]["step"] == 1       # get_decay(1) = 0: the first update copies (up to rounding)
    # a later command: raw weights without the flag, the averaged ones with it
    config.mode = cli.MODE_SAMPLING
    for flag, want in ((False, raw), (True, shadow)):
        config.use_ema = flag
        m2, _, _ = cli.get_model_sched(config, gpu)
        assert torch.equal(m2.flat.detach().cpu()[mask], want[mask]), flag
    os.rename(os.path.join(config.output_dir, "unet_ema"), os.path.join(config.output_dir, "gone"))
    with pytest.raises(FileNotFoundError):
        cli.get_model_sched(config, gpu)
