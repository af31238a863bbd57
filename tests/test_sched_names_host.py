"""CPU: what every `--sched` name builds, pinned as typed-out data recorded from the code before the names moved into one table
(baddiffusion_amd/sched_names.py) -- not computed from that table.  DiffuserModelSched.get_pretrained + get_pipeline with and
without native_sched, elijah_defense.make_pipeline with and without --dyn_threshold, and both command lines' SCHED_CHOICES."""
import types

import pytest

NOT_IMPL = "NotImplementedError"
CARRIER, PNDM = "SchedulerConfigCarrier", "PNDMPipeline"
NO_NATIVE = "has no native scheduler (native_sched covers the DPM-Solver names; without it this name samples through PNDMPipeline)"
UNHANDLED = "not handled by the reference's model.py:577-643 either"

# get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, clip_sample=True, native_sched=...) then get_pipeline(model, noise_sched):
# (scheduler type, SchedulerConfigCarrier.class_name, config solver_order, config algorithm_type, config.clip_sample,
#  pipeline type, pipeline.clip_sample, pipeline.order) -- None where the object has no such attribute -- or (exception type, message)
# the names whose outcome does not depend on native_sched
MODEL_EITHER = {
    None: ("DDPMScheduler", None, None, None, True, "DDPMPipeline", None, None),
    "DDPM-SCHED": ("DDPMScheduler", None, None, None, True, "DDPMPipeline", None, None),
    "DDIM-SCHED": ("DDIMScheduler", None, None, None, True, "DDIMPipeline", None, None),
    "PNDM-SCHED": ("PNDMScheduler", None, None, None, True, PNDM, True, None),
    "UNIPC_O1-SCHED": ("UniPCMultistepScheduler", None, 1, None, True, "UniPCPipeline", True, None),
    "UNIPC_O2-SCHED": ("UniPCMultistepScheduler", None, 2, None, True, "UniPCPipeline", True, None),
    "UNIPC_O3-SCHED": ("UniPCMultistepScheduler", None, 3, None, True, "UniPCPipeline", True, None),
    "DEIS_O1-SCHED": ("DEISMultistepScheduler", None, 1, "deis", True, "DEISPipeline", True, None),
    "DEIS_O2-SCHED": ("DEISMultistepScheduler", None, 2, "deis", True, "DEISPipeline", True, None),
    "DEIS_O3-SCHED": ("DEISMultistepScheduler", None, 3, "deis", True, "DEISPipeline", True, None),
    "HEUN_O2-SCHED": ("HeunDiscreteScheduler", None, None, None, True, "HeunPipeline", True, None),
    "LMSD_O1-SCHED": ("LMSDiscreteScheduler", None, None, None, True, "LMSPipeline", True, 1),
    "LMSD_O2-SCHED": ("LMSDiscreteScheduler", None, None, None, True, "LMSPipeline", True, 2),
    "LMSD_O3-SCHED": ("LMSDiscreteScheduler", None, None, None, True, "LMSPipeline", True, 3),
    "LMSD_O4-SCHED": ("LMSDiscreteScheduler", None, None, None, True, "LMSPipeline", True, 4),
    "EULER_O1-SCHED": ("EulerDiscreteScheduler", None, None, None, True, "EulerPipeline", True, None),
    "EULER_A_O1-SCHED": ("EulerAncestralDiscreteScheduler", None, None, None, True, "EulerAncestralPipeline", True, None),
    "KDPM2_O2-SCHED": ("KDPM2DiscreteScheduler", None, None, None, True, "KDPM2Pipeline", True, None),
    "KDPM2_A_O2-SCHED": ("KDPM2AncestralDiscreteScheduler", None, None, None, True, "KDPM2AncestralPipeline", True, None),
    "LDM-SCHED": (NOT_IMPL, f"LDM-SCHED: {UNHANDLED}"),
    "SCORE-SDE-VE-SCHED": (NOT_IMPL, f"SCORE-SDE-VE-SCHED: {UNHANDLED}"),
    "EDM-VE-SCHED": (NOT_IMPL, f"EDM-VE-SCHED: {UNHANDLED}"),
    "EDM-VE-ODE-SCHED": (NOT_IMPL, f"EDM-VE-ODE-SCHED: {UNHANDLED}"),
    "EDM-VE-SDE-SCHED": (NOT_IMPL, f"EDM-VE-SDE-SCHED: {UNHANDLED}"),
    "NO-SUCH-SCHED": (NOT_IMPL, ""),
}
# name: (outcome with native_sched=False, outcome with native_sched=True)
MODEL_BY_NATIVE = {
    "DPM_SOLVER_PP_O1-SCHED": ((CARRIER, "DPMSolverMultistepScheduler", None, None, True, PNDM, True, None),
                               ("DPMSolverMultistepScheduler", None, 1, "dpmsolver++", True, "DPMSolverPipeline", True, None)),
    "DPM_SOLVER_O1-SCHED": ((CARRIER, "DPMSolverMultistepScheduler", None, None, True, PNDM, True, None),
                            ("DPMSolverMultistepScheduler", None, 1, "dpmsolver", True, "DPMSolverPipeline", True, None)),
    "DPM_SOLVER_PP_O2-SCHED": ((CARRIER, "DPMSolverMultistepScheduler", None, None, True, PNDM, True, None),
                               ("DPMSolverMultistepScheduler", None, 2, "dpmsolver++", True, "DPMSolverPipeline", True, None)),
    "DPM_SOLVER_O2-SCHED": ((CARRIER, "DPMSolverMultistepScheduler", None, None, True, PNDM, True, None),
                            ("DPMSolverMultistepScheduler", None, 2, "dpmsolver", True, "DPMSolverPipeline", True, None)),
    "DPM_SOLVER_PP_O3-SCHED": ((CARRIER, "DPMSolverMultistepScheduler", None, None, True, PNDM, True, None),
                               ("DPMSolverMultistepScheduler", None, 3, "dpmsolver++", True, "DPMSolverPipeline", True, None)),
    "DPM_SOLVER_O3-SCHED": ((CARRIER, "DPMSolverMultistepScheduler", None, None, True, PNDM, True, None),
                            ("DPMSolverMultistepScheduler", None, 3, "dpmsolver", True, "DPMSolverPipeline", True, None)),
    "UNIPC-SCHED": ((CARRIER, "UniPCMultistepScheduler", None, None, True, PNDM, True, None),
                    (NOT_IMPL, f"UNIPC-SCHED: UniPCMultistepScheduler {NO_NATIVE}")),
    "DEIS-SCHED": ((CARRIER, "DEISMultistepScheduler", None, None, True, PNDM, True, None),
                   (NOT_IMPL, f"DEIS-SCHED: DEISMultistepScheduler {NO_NATIVE}")),
    "HEUN-SCHED": ((CARRIER, "HeunDiscreteScheduler", None, None, True, PNDM, True, None),
                   (NOT_IMPL, f"HEUN-SCHED: HeunDiscreteScheduler {NO_NATIVE}")),
    "LMSD-SCHED": ((CARRIER, "LMSDiscreteScheduler", None, None, True, PNDM, True, None),
                   (NOT_IMPL, f"LMSD-SCHED: LMSDiscreteScheduler {NO_NATIVE}")),
}
MODEL_CASES = [(name, native, out) for name, out in MODEL_EITHER.items() for native in (False, True)] + \
    [(name, native, outs[native]) for name, outs in MODEL_BY_NATIVE.items() for native in (False, True)]

# elijah_defense.make_pipeline(config, unet, DDPMScheduler(num_train_timesteps=400)), keyed by (--sched, --dyn_threshold):
# (pipeline type, scheduler type, len(scheduler) == 400, config solver_order, config algorithm_type, pipeline.order,
#  pipeline.clip_sample, the scheduler is the checkpoint's own object, its config.sample_max_value)
ELIJAH = {
    ("DDIM-SCHED", None): ("DDIMPipeline", "DDIMScheduler", True, None, None, None, None, False, 1.0),
    ("DDIM-SCHED", 1.5): ("DDIMPipeline", "DDIMScheduler", True, None, None, None, None, False, 1.5),
    ("DDPM-SCHED", None): ("DDPMPipeline", "DDPMScheduler", True, None, None, None, None, True, 1.0),
    ("DDPM-SCHED", 1.5): ("DDPMPipeline", "DDPMScheduler", True, None, None, None, None, False, 1.5),
    ("DPM_SOLVER_O1-SCHED", None): ("DPMSolverPipeline", "DPMSolverMultistepScheduler", True, 1, "dpmsolver", None, False, False, 1.0),
    ("DPM_SOLVER_O2-SCHED", None): ("DPMSolverPipeline", "DPMSolverMultistepScheduler", True, 2, "dpmsolver", None, False, False, 1.0),
    ("DPM_SOLVER_O3-SCHED", None): ("DPMSolverPipeline", "DPMSolverMultistepScheduler", True, 3, "dpmsolver", None, False, False, 1.0),
    ("DPM_SOLVER_PP_O1-SCHED", None): ("DPMSolverPipeline", "DPMSolverMultistepScheduler", True, 1, "dpmsolver++", None, False, False, 1.0),
    ("DPM_SOLVER_PP_O2-SCHED", None): ("DPMSolverPipeline", "DPMSolverMultistepScheduler", True, 2, "dpmsolver++", None, False, False, 1.0),
    ("DPM_SOLVER_PP_O3-SCHED", None): ("DPMSolverPipeline", "DPMSolverMultistepScheduler", True, 3, "dpmsolver++", None, False, False, 1.0),
    ("UNIPC_O1-SCHED", None): ("UniPCPipeline", "UniPCMultistepScheduler", True, 1, None, None, False, False, 1.0),
    ("UNIPC_O2-SCHED", None): ("UniPCPipeline", "UniPCMultistepScheduler", True, 2, None, None, False, False, 1.0),
    ("UNIPC_O3-SCHED", None): ("UniPCPipeline", "UniPCMultistepScheduler", True, 3, None, None, False, False, 1.0),
    ("DEIS_O1-SCHED", None): ("DEISPipeline", "DEISMultistepScheduler", True, 1, "deis", None, False, False, 1.0),
    ("DEIS_O2-SCHED", None): ("DEISPipeline", "DEISMultistepScheduler", True, 2, "deis", None, False, False, 1.0),
    ("DEIS_O3-SCHED", None): ("DEISPipeline", "DEISMultistepScheduler", True, 3, "deis", None, False, False, 1.0),
    ("HEUN_O2-SCHED", None): ("HeunPipeline", "HeunDiscreteScheduler", True, None, None, None, False, False, None),
    ("LMSD_O1-SCHED", None): ("LMSPipeline", "LMSDiscreteScheduler", True, None, None, 1, False, False, None),
    ("LMSD_O2-SCHED", None): ("LMSPipeline", "LMSDiscreteScheduler", True, None, None, 2, False, False, None),
    ("LMSD_O3-SCHED", None): ("LMSPipeline", "LMSDiscreteScheduler", True, None, None, 3, False, False, None),
    ("LMSD_O4-SCHED", None): ("LMSPipeline", "LMSDiscreteScheduler", True, None, None, 4, False, False, None),
    ("EULER_A_O1-SCHED", None): ("EulerAncestralPipeline", "EulerAncestralDiscreteScheduler", True, None, None, None, False, False, None),
    ("EULER_O1-SCHED", None): ("EulerPipeline", "EulerDiscreteScheduler", True, None, None, None, False, False, None),
    ("KDPM2_A_O2-SCHED", None): ("KDPM2AncestralPipeline", "KDPM2AncestralDiscreteScheduler", True, None, None, None, False, False, None),
    ("KDPM2_O2-SCHED", None): ("KDPM2Pipeline", "KDPM2DiscreteScheduler", True, None, None, None, False, False, None),
}

TRAIN_CHOICES = {"DDPM-SCHED", "DDIM-SCHED", "DPM_SOLVER_PP_O1-SCHED", "DPM_SOLVER_O1-SCHED", "DPM_SOLVER_PP_O2-SCHED", "DPM_SOLVER_O2-SCHED",
                 "DPM_SOLVER_PP_O3-SCHED", "DPM_SOLVER_O3-SCHED", "UNIPC-SCHED", "PNDM-SCHED", "DEIS-SCHED", "HEUN-SCHED", "SCORE-SDE-VE-SCHED",
                 "UNIPC_O1-SCHED", "UNIPC_O2-SCHED", "UNIPC_O3-SCHED", "HEUN_O2-SCHED", "LMSD_O1-SCHED", "LMSD_O2-SCHED", "LMSD_O3-SCHED",
                 "LMSD_O4-SCHED", "DEIS_O1-SCHED", "DEIS_O2-SCHED", "DEIS_O3-SCHED", "EULER_O1-SCHED", "EULER_A_O1-SCHED", "KDPM2_O2-SCHED",
                 "KDPM2_A_O2-SCHED"}
ELIJAH_CHOICES = {"DDIM-SCHED", "DDPM-SCHED", "DPM_SOLVER_O1-SCHED", "DPM_SOLVER_O2-SCHED", "DPM_SOLVER_O3-SCHED", "DPM_SOLVER_PP_O1-SCHED",
                  "DPM_SOLVER_PP_O2-SCHED", "DPM_SOLVER_PP_O3-SCHED", "UNIPC_O1-SCHED", "UNIPC_O2-SCHED", "UNIPC_O3-SCHED", "DEIS_O1-SCHED",
                  "DEIS_O2-SCHED", "DEIS_O3-SCHED", "HEUN_O2-SCHED", "LMSD_O1-SCHED", "LMSD_O2-SCHED", "LMSD_O3-SCHED", "LMSD_O4-SCHED",
                  "EULER_A_O1-SCHED", "EULER_O1-SCHED", "KDPM2_A_O2-SCHED", "KDPM2_O2-SCHED"}
# the names dynamic thresholding goes with (and no scheduler name)
DYN_THRESHOLD_NAMES = {"DDPM-SCHED", "DDIM-SCHED"}


class _StubUNet:
    """stands in for UNet2DModel: the builders only hand the network to the pipeline"""

    def __init__(self, **kw):
        pass


@pytest.fixture
def stub_unet(monkeypatch):
    from baddiffusion_amd import model
    monkeypatch.setattr(model, "UNet2DModel", _StubUNet)


@pytest.mark.parametrize("name,native,expected", MODEL_CASES)
def test_model_builds_what_it_built(stub_unet, name, native, expected):
    from baddiffusion_amd.model import DiffuserModelSched
    try:
        m, s, get_pipeline = DiffuserModelSched.get_pretrained("DDPM-CIFAR10-32", noise_sched_type=name, allow_random_init=True,
                                                               clip_sample=True, native_sched=native)
        p = get_pipeline(m, s)
    except Exception as e:      # noqa: BLE001 -- the outcome is the exception
        assert (type(e).__name__, str(e)) == expected
        return
    assert p.unet is m
    assert (type(s).__name__, getattr(s, "class_name", None), s.config.get("solver_order"), s.config.get("algorithm_type"), s.config.clip_sample,
            type(p).__name__, getattr(p, "clip_sample", None), getattr(p, "order", None)) == expected
    # the reference's tables under every name, also where the class defaults differ (Heun, KDPM2)
    assert (s.config.num_train_timesteps, s.config.beta_start, s.config.beta_end) == (1000, 0.0001, 0.02)


def test_the_tables_cover_every_name():
    from baddiffusion_amd.sched_names import SCHEDS
    assert set(SCHEDS) == (set(MODEL_EITHER) | set(MODEL_BY_NATIVE)) - {None, "NO-SUCH-SCHED"}
    assert {name for name, _ in ELIJAH} == ELIJAH_CHOICES


@pytest.mark.parametrize("name,dyn", list(ELIJAH))
def test_elijah_builds_what_it_built(name, dyn, capsys):
    import elijah_defense as E
    from baddiffusion_amd.schedulers import DDPMScheduler
    ckpt_sched = DDPMScheduler(num_train_timesteps=400)
    unet = _StubUNet()
    p = E.make_pipeline(types.SimpleNamespace(sched=name, dyn_threshold=dyn, dyn_threshold_ratio=0.995), unet, ckpt_sched)
    s = p.scheduler
    assert p.unet is unet
    assert (type(p).__name__, type(s).__name__, len(s) == 400, s.config.get("solver_order"), s.config.get("algorithm_type"),
            getattr(p, "order", None), getattr(p, "clip_sample", None), s is ckpt_sched, s.config.get("sample_max_value")) == ELIJAH[name, dyn]
    assert bool(s.config.get("thresholding")) is (dyn is not None)
    assert ckpt_sched.config.thresholding is False          # the checkpoint's scheduler, which is saved back, keeps its config


def test_sched_choices_are_what_they_were():
    import baddiffusion as cli
    import elijah_defense as E
    for got, want in ((cli.SCHED_CHOICES, TRAIN_CHOICES), (E.SCHED_CHOICES, ELIJAH_CHOICES)):
        assert len(got) == len(set(got)) and set(got) == want


def test_dyn_threshold_goes_with_the_same_names():
    from baddiffusion_amd.model import DiffuserModelSched
    DiffuserModelSched._check_dyn_threshold(None, 1.5, 0.995)
    for name in (set(MODEL_EITHER) | set(MODEL_BY_NATIVE)) - {None}:
        if name in DYN_THRESHOLD_NAMES:
            DiffuserModelSched._check_dyn_threshold(name, 1.5, 0.995)
        else:
            with pytest.raises(NotImplementedError, match=f"dyn_threshold with {name}: dynamic thresholding runs in the DDPM and DDIM steps only"):
                DiffuserModelSched._check_dyn_threshold(name, 1.5, 0.995)
