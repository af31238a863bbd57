"""EMA fixtures -> tests/golden/ema_decay.json.

Everything is recorded from the imported reference EMAModel (diffusers, training_utils.py:46-322): get_decay(k) under five
settings (floats by repr, so the comparison is ==), the keys of state_dict(), and the messages load_state_dict raises for a bad
decay, min_decay, inv_gamma and power.  The import shim comes from make_golden.py (nothing is generated on import).

    python tests/golden/make_golden_ema.py
"""
import json
import os
import sys
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch

from tests.golden import make_golden as MG           # noqa: F401  -- the reference import shim
from diffusers.training_utils import EMAModel

STEPS = list(range(41)) + [1000, 31623, 10 ** 6]
SETTINGS = {
    "default": {},
    "warmup_p23": {"use_ema_warmup": True, "power": 2 / 3},
    "warmup_p34_g2": {"use_ema_warmup": True, "power": 3 / 4, "inv_gamma": 2},
    "after3": {"update_after_step": 3},
    "min05": {"min_decay": 0.5},
}
# the engine tests' schedule (EMAModel(model, use_ema_warmup=True, power=0.75)) is "warmup_p34" below
SETTINGS["warmup_p34"] = {"use_ema_warmup": True, "power": 0.75}
BAD = {"decay": 1.5, "min_decay": 1, "inv_gamma": "1", "power": "x"}


def main():
    params = [torch.nn.Parameter(torch.zeros(3))]
    out = {"steps": STEPS, "settings": {}, "decay": {}, "errors": {}}
    for name, kw in SETTINGS.items():
        e = EMAModel(params, **kw)
        out["settings"][name] = {k: repr(v) for k, v in kw.items()}
        out["decay"][name] = [repr(e.get_decay(k)) for k in STEPS]
    e = EMAModel(params)
    out["state_dict_keys"] = list(e.state_dict().keys())
    for key, bad in BAD.items():
        sd = {key: bad}
        try:
            EMAModel(params).load_state_dict(sd)
            raise SystemExit(f"the reference accepted {sd}")
        except ValueError as err:
            out["errors"][key] = {"state": {k: repr(v) for k, v in sd.items()}, "message": str(err)}
    try:
        EMAModel(params).restore(params)
    except RuntimeError as err:
        out["errors"]["restore"] = {"message": str(err)}
    path = os.path.join(HERE, "ema_decay.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
