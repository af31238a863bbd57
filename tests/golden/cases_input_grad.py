"""Seeds / shapes of the input-gradient fixtures (input_grad.npz), shared by make_golden_input_grad.py and the tests.
The training inputs and the 256 x 256 inputs are the ones of cases.py (train_inputs, celeba_full_inputs, celeba_b4_inputs)."""
import torch

from oracle import unet_ref as U
from tests.golden.cases import SMALL_CFGS

# tag -> (config, weight seed, batch): loss = mse(target, pred) on q_sample of train_inputs(cfg, B), dx = d loss / d x_noisy
TRAIN_CASES = {
    "small": (SMALL_CFGS["small"], 7, 2),
    "small_default": (SMALL_CFGS["small_default"], 7, 2),
    "cifar": (U.CIFAR10_32, 0, 2),
    "cifar128": (U.CIFAR10_32, 0, 128),          # rows FULL_ROWS + per-sample sum / sumsq only
}
# tag -> (weight seed, stride of the stored dx slice): upstream gradient dout straight into the network output
CELEBA_CASES = {"celeba256": (5, 4), "celeba256b4": (5, 8)}

# trigger inversion (inversion.invert_trigger's loop written out): small topology, seed-7 weights
INV_CFG = "small"
INV_SEED = 7
INV_BATCH = 4
INV_STEPS = 3
INV_LR = 50.0          # SGD; with lr = 0.1 |tau| stays at 2e-3 and steps 2, 3 would not depend on tau
INV_LAM = 0.5
INV_T = 999
INV_NOISE_SEED = 21


def inv_noises():
    cfg = SMALL_CFGS[INV_CFG]
    g = torch.Generator().manual_seed(INV_NOISE_SEED)
    return [torch.randn(INV_BATCH, cfg.in_channels, cfg.sample_size, cfg.sample_size, generator=g) for _ in range(INV_STEPS)]
