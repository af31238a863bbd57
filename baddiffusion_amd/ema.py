"""Exponential moving average of the weights over ONE flat shadow buffer, with the interface of diffusers' EMAModel
(diffusers/src/diffusers/training_utils.py:46-322).

The reference keeps one shadow tensor per parameter and moves each by `one_minus_decay * (shadow - param)` (:200-202).  Here the
model's parameters are one flat fp32 buffer (`model.flat`), so the shadow is a clone of it -- alignment pads included, which then
stay equal -- and an update is one launch over it: `bd_ema_update` from `step()`, or, inside a training engine, the same three
fp32 roundings fused into the clip + Adam launch (`TrainEngine(..., ema=EMAModel(model))`).  Method names, the decay schedule, the
state-dict keys and the validation messages are the reference's (pinned by tests/golden/ema_decay.json); methods take the model
where the reference takes its parameters.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import ops

# state_dict() order; every key but the last is a host scalar kept as an attribute of the same name
_SCALARS = ("decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power")
_SHADOW_KEY = "shadow_params"
# load_state_dict(): (key, what a valid value satisfies, the reference's message), checked in this order
_CHECKS = (
    ("decay", lambda x: 0.0 <= x <= 1.0, "Decay must be between 0 and 1"),
    ("min_decay", lambda x: isinstance(x, float), "Invalid min_decay"),
    ("optimization_step", lambda x: isinstance(x, int), "Invalid optimization_step"),
    ("update_after_step", lambda x: isinstance(x, int), "Invalid update_after_step"),
    ("use_ema_warmup", lambda x: isinstance(x, bool), "Invalid use_ema_warmup"),
    ("inv_gamma", lambda x: isinstance(x, (float, int)), "Invalid inv_gamma"),
    ("power", lambda x: isinstance(x, (float, int)), "Invalid power"),
)
_NOTHING_STORED = "This ExponentialMovingAverage has no `store()`ed weights to `restore()`"


class EMAModel:
    def __init__(self, model, decay=0.9999, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
        self.shadow = model.flat.detach().clone()
        self.temp_stored_params = None        # store() ... restore()
        self.decay, self.min_decay, self.update_after_step = decay, min_decay, update_after_step
        self.use_ema_warmup, self.inv_gamma, self.power = use_ema_warmup, inv_gamma, power
        self.optimization_step = 0
        self.cur_decay_value = None           # the decay of the last step taken
        self.attached = False                 # a TrainEngine (and possibly a captured graph of its step) holds the shadow's address

    # ---- schedule: training_utils.py:157-174, in Python floats and in the reference's operation order, so the values are equal ----
    def get_decay(self, optimization_step):
        n = optimization_step - self.update_after_step - 1
        if n <= 0:
            return 0.0
        value = 1 - (1 + n / self.inv_gamma) ** -self.power if self.use_ema_warmup else (1 + n) / (10 + n)
        return max(min(value, self.decay), self.min_decay)

    def advance(self):
        """Count one optimization step and return its one_minus_decay as the kernels take it: the Python float 1 - decay rounded to
        fp32, which is what torch makes of that scalar when it multiplies an fp32 tensor.  step() and the training engine's fused
        update both come through here, so they cannot disagree on the schedule."""
        self.optimization_step += 1
        self.cur_decay_value = self.get_decay(self.optimization_step)
        return float(np.float32(1 - self.cur_decay_value))

    def _flat_of(self, model):
        flat = model.flat
        if flat.numel() != self.shadow.numel() or flat.device != self.shadow.device:
            raise ValueError(f"EMAModel: the model's flat parameter ({flat.numel()} floats on {flat.device}) does not match the shadow "
                             f"({self.shadow.numel()} floats on {self.shadow.device})")
        return flat

    @torch.no_grad()
    def step(self, model):
        """one update from the model's current weights (one bd_ema_update launch); a flat parameter that does not require grad is
        copied, as the reference copies such parameters"""
        flat = self._flat_of(model)
        omd = self.advance()
        if flat.requires_grad:
            ops.ema_update(self.shadow, flat.data, omd)
        else:
            self.shadow.copy_(flat.data)

    # ---- weights in and out of the model: device-to-device copies of the flat buffer --------------------------------------------
    def _write(self, model, src):
        # the weights change in place under a model whose pipelines run with static weights: drop the prepared weight planes
        self._flat_of(model).data.copy_(src)
        model._reset_static_cache()

    @torch.no_grad()
    def copy_to(self, model):
        self._write(model, self.shadow)

    @torch.no_grad()
    def store(self, model):
        """keep the model's current weights for restore(); the copy stays on the device"""
        self.temp_stored_params = self._flat_of(model).detach().clone()

    @torch.no_grad()
    def restore(self, model):
        if self.temp_stored_params is None:
            raise RuntimeError(_NOTHING_STORED)
        self._write(model, self.temp_stored_params)
        self.temp_stored_params = None

    def to(self, device=None, dtype=None):
        """Move the shadow (and a stored copy).  The kernels read fp32 only, so another dtype is refused; a move to the device the
        shadow is on already leaves the buffer where it is; once a training engine holds its address the shadow cannot move."""
        if dtype is not None and dtype != torch.float32:
            raise TypeError(f"EMAModel.to: the shadow is float32 (the update kernels read nothing else), got dtype {dtype}")
        if device is None or torch.empty(0, device=device).device == self.shadow.device:
            return
        if self.attached:
            raise RuntimeError("EMAModel.to: a TrainEngine holds this shadow's address; move the model and build the EMAModel before the engine")
        self.shadow = self.shadow.to(device=device)
        if self.temp_stored_params is not None:
            self.temp_stored_params = self.temp_stored_params.to(device=device)

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        sd = {key: getattr(self, key) for key in _SCALARS}
        sd[_SHADOW_KEY] = self.shadow
        return sd

    def load_state_dict(self, state_dict):
        for key, valid, message in _CHECKS:
            if key in state_dict:
                setattr(self, key, state_dict[key])
            if not valid(getattr(self, key)):
                raise ValueError(message)
        shadow = state_dict.get(_SHADOW_KEY)
        if shadow is None:
            return
        if not isinstance(shadow, torch.Tensor):
            raise ValueError(f"{_SHADOW_KEY} must be a Tensor")
        if shadow.dtype != torch.float32 or shadow.shape != self.shadow.shape:
            raise ValueError(f"{_SHADOW_KEY} must be float32 {tuple(self.shadow.shape)}, got {shadow.dtype} {tuple(shadow.shape)}")
        self.shadow.copy_(shadow)       # in place: a training engine, and a captured graph of its step, hold this buffer's address

    def averaged_state_dict(self, model):
        """the shadow under the model's state-dict keys and shapes (the offset table model.state_dict() goes through)"""
        return OrderedDict((key, model._logical_view(self.shadow, key).contiguous()) for key in model._table)
