"""Shared seeds / shapes of the RePaint fixtures (tests/golden/repaint.npz): imported by make_golden_repaint.py (reference side, CPU) and by
tests/test_repaint*.py, so both sides build bit-identical inputs."""
import torch

# (num_inference_steps, jump_length, jump_n_sample)
TIMESTEP_CASES = ((250, 10, 10), (10, 2, 3), (6, 2, 2), (4, 1, 2), (3, 5, 5))
TS_4_1_2 = [750, 500, 750, 500, 250, 500, 250, 0, 250, 0]

STEP_INFER = 10
STEP_TS = (900, 500, 0)
STEP_ETAS = (0.0, 0.5, 1.0)
STEP_MASKS = ("one", "row", "frac")
STEP_NOISE_SEED = 95
UNDO_CASES = {"k4": (250, 400), "k100": (10, 500)}      # tag -> (num_inference_steps, timestep); k = 1000 // num_inference_steps
UNDO_NOISE_SEED = 96

CHAIN = (10, 2, 3)
CHAIN_SEED = 97
CHAIN_CASES = tuple((eta, clip) for eta in (0.0, 1.0) for clip in (True, False))

UNET_CFG, UNET_PARAM_SEED = "small", 7
UNET_CHAIN = (4, 1, 2)
UNET_ETAS = (0.0, 1.0)
UNET_SEED = 1234
UNET_HOLE = (slice(4, 12), slice(6, 14))


def _g(seed):
    return torch.Generator().manual_seed(seed)


def step_inputs():
    """(sample, model_output, original_image) [2,3,8,8]"""
    return (torch.randn(2, 3, 8, 8, generator=_g(91)), torch.randn(2, 3, 8, 8, generator=_g(92)),
            torch.rand(2, 3, 8, 8, generator=_g(93)) * 2 - 1)


def step_mask(kind):
    """'one': binary [1,1,8,8]; 'row': binary [2,1,8,8]; 'frac': fractional [2,3,8,8]"""
    g = _g(94)
    if kind == "one":
        return (torch.rand(1, 1, 8, 8, generator=g) < 0.5).float()
    if kind == "row":
        return (torch.rand(2, 1, 8, 8, generator=g) < 0.5).float()
    return torch.rand(2, 3, 8, 8, generator=g)


def shift_image():
    """a [3,8,8] trigger-like image for the shift variant: zero outside a bright corner box"""
    s = torch.zeros(3, 8, 8)
    s[:, 5:, 5:] = torch.rand(3, 3, 3, generator=_g(98)) + 0.5
    return s


def undo_sample():
    return torch.randn(2, 3, 8, 8, generator=_g(99))


def chain_inputs():
    """(initial sample, original_image, mask [1,1,8,8]) of the stand-in chain"""
    mask = torch.ones(1, 1, 8, 8)
    mask[:, :, 2:6, 3:7] = 0
    return torch.randn(2, 3, 8, 8, generator=_g(77)), torch.rand(2, 3, 8, 8, generator=_g(78)) * 2 - 1, mask


def unet_inputs():
    """(image [2,3,16,16] in [-1, 1], mask [1,1,16,16]: ones with a hole)"""
    image = torch.rand(2, 3, 16, 16, generator=_g(81)) * 2 - 1
    mask = torch.ones(1, 1, 16, 16)
    mask[(slice(None), slice(None)) + UNET_HOLE] = 0
    return image, mask
