"""The one table of `--sched` names: what each name builds, where it is offered and what it refuses.  DiffuserModelSched
(model.py), elijah_defense.make_pipeline and both command lines' SCHED_CHOICES read it; a new sampler is one more row here."""
from dataclasses import dataclass, field
from functools import partial

from .pipelines import (DDIMPipeline, DDPMPipeline, DEISPipeline, DPMSolverPipeline, EulerAncestralPipeline, EulerPipeline, HeunPipeline,
                        KDPM2AncestralPipeline, KDPM2Pipeline, LMSPipeline, PNDMPipeline, UniPCPipeline)
from .schedulers import (DDIMScheduler, DDPMScheduler, DEISMultistepScheduler, DPMSolverMultistepScheduler,
                         EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, HeunDiscreteScheduler, KDPM2AncestralDiscreteScheduler,
                         KDPM2DiscreteScheduler, LMSDiscreteScheduler, PNDMScheduler, SchedulerConfigCarrier, UniPCMultistepScheduler)

DDPM_SCHED = "DDPM-SCHED"
DDIM_SCHED = "DDIM-SCHED"


@dataclass(frozen=True)
class SchedName:
    name: str
    scheduler: type = None              # the native scheduler class, built with sched_kw over the builder's own keywords
    sched_kw: dict = field(default_factory=dict)
    pipeline: type = None               # the pipeline that steps it, with pipe_kw
    pipe_kw: dict = field(default_factory=dict)
    # model.py:598-630: the reference builds this class but samples through PNDMPipeline, which converts it to a PNDMScheduler
    # (pipeline_pndm.py:46); DiffuserModelSched then returns a SchedulerConfigCarrier that records the class name
    carrier: str = None
    refused: str = None                 # the name is known and builds nothing: why
    clip_in_sched: bool = False         # DiffuserModelSched hands clip_sample to the scheduler (DDPM, DDIM), not to the pipeline
    dyn_threshold: bool = False         # dynamic thresholding runs in this name's step
    in_train: bool = True               # offered by baddiffusion.py --sched
    in_elijah: bool = True              # offered by elijah_defense.py --sched

    @property
    def native_only(self):
        """the native scheduler and pipeline are used under native_sched=True only, the PNDM conversion otherwise"""
        return self.carrier is not None and self.scheduler is not None

    def resolve(self, native_sched):
        """(scheduler factory, its keywords, pipeline class, its keywords) this name samples with"""
        if self.refused is not None:
            raise NotImplementedError(f"{self.name}: {self.refused}")
        if self.carrier is None or (native_sched and self.scheduler is not None):
            return self.scheduler, self.sched_kw, self.pipeline, self.pipe_kw
        if native_sched:
            raise NotImplementedError(f"{self.name}: {self.carrier} has no native scheduler "
                                      "(native_sched covers the DPM-Solver names; without it this name samples through PNDMPipeline)")
        # SURVEY f-4: training uses only the betas of this object; sampling = PNDMPipeline with the post-step clip
        return partial(SchedulerConfigCarrier, self.carrier), {}, PNDMPipeline, {}


def _dpm(name, order, algorithm):
    # model.py:598-614; native_sched=True (and elijah_defense.py always) runs the solver the name says
    return SchedName(name, DPMSolverMultistepScheduler, dict(solver_order=order, algorithm_type=algorithm), DPMSolverPipeline,
                     carrier="DPMSolverMultistepScheduler")


def _reference_only(name, carrier, in_train=True):
    # elijah_defense.py offers no name that only samples through the PNDM conversion
    return SchedName(name, carrier=carrier, in_train=in_train, in_elijah=False)


def _unhandled(name, in_train=False):
    # named in model.py:556-563 but not handled by its __get_model_sched either (it raises NotImplementedError)
    return SchedName(name, refused="not handled by the reference's model.py:577-643 either", in_train=in_train, in_elijah=False)


_TABLE = (
    SchedName(DDPM_SCHED, DDPMScheduler, {}, DDPMPipeline, clip_in_sched=True, dyn_threshold=True),
    SchedName(DDIM_SCHED, DDIMScheduler, {}, DDIMPipeline, clip_in_sched=True, dyn_threshold=True),
    _dpm("DPM_SOLVER_PP_O1-SCHED", 1, "dpmsolver++"), _dpm("DPM_SOLVER_O1-SCHED", 1, "dpmsolver"),
    _dpm("DPM_SOLVER_PP_O2-SCHED", 2, "dpmsolver++"), _dpm("DPM_SOLVER_O2-SCHED", 2, "dpmsolver"),
    _dpm("DPM_SOLVER_PP_O3-SCHED", 3, "dpmsolver++"), _dpm("DPM_SOLVER_O3-SCHED", 3, "dpmsolver"),
    _reference_only("UNIPC-SCHED", "UniPCMultistepScheduler"),
    SchedName("PNDM-SCHED", PNDMScheduler, {}, PNDMPipeline, in_elijah=False),
    _reference_only("DEIS-SCHED", "DEISMultistepScheduler"),
    _reference_only("HEUN-SCHED", "HeunDiscreteScheduler"),
    # oddities kept as found: baddiffusion.py does not offer LMSD-SCHED, which builds like its three siblings above, nor LDM-SCHED and
    # the EDM names, but it does offer SCORE-SDE-VE-SCHED, which is refused like them
    _reference_only("LMSD-SCHED", "LMSDiscreteScheduler", in_train=False),
    _unhandled("LDM-SCHED"), _unhandled("SCORE-SDE-VE-SCHED", in_train=True), _unhandled("EDM-VE-SCHED"), _unhandled("EDM-VE-ODE-SCHED"),
    _unhandled("EDM-VE-SDE-SCHED"),
    # names of this project's own, with or without native_sched (the reference's UNIPC-SCHED, DEIS-SCHED, HEUN-SCHED and LMSD-SCHED keep
    # their PNDM conversion; it names no Euler or KDPM2).  UniPC's other options are the reference's defaults (bh2, predict_x0), DEIS
    # runs in the reference's coefficient arithmetic
    *(SchedName(f"UNIPC_O{o}-SCHED", UniPCMultistepScheduler, dict(solver_order=o), UniPCPipeline) for o in (1, 2, 3)),
    SchedName("HEUN_O2-SCHED", HeunDiscreteScheduler, {}, HeunPipeline),
    *(SchedName(f"LMSD_O{o}-SCHED", LMSDiscreteScheduler, {}, LMSPipeline, dict(order=o)) for o in (1, 2, 3, 4)),
    *(SchedName(f"DEIS_O{o}-SCHED", DEISMultistepScheduler, dict(solver_order=o), DEISPipeline) for o in (1, 2, 3)),
    SchedName("EULER_O1-SCHED", EulerDiscreteScheduler, {}, EulerPipeline),
    SchedName("EULER_A_O1-SCHED", EulerAncestralDiscreteScheduler, {}, EulerAncestralPipeline),
    SchedName("KDPM2_O2-SCHED", KDPM2DiscreteScheduler, {}, KDPM2Pipeline),
    SchedName("KDPM2_A_O2-SCHED", KDPM2AncestralDiscreteScheduler, {}, KDPM2AncestralPipeline),
)
SCHEDS = {r.name: r for r in _TABLE}
TRAIN_CHOICES = [r.name for r in _TABLE if r.in_train]
ELIJAH_CHOICES = [r.name for r in _TABLE if r.in_elijah]
