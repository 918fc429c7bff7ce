"""marbler_amd -- MI355X-native (gfx950) vectorised Robotarium-gym step engine.

The one hot path of GT-STAR-Lab/MARBLER (the multi-robot env step) as hand-written HIP
kernels behind the reference's reset()/step() surface.  See DESIGN.md and INTEGRATION.md.
There is no CPU fallback: the HIP library must be built (python -m marbler_amd.build) and a
GPU must be visible, or construction raises.
"""
from . import render  # noqa: F401
from .episodes import EpisodeBuffer  # noqa: F401
from ._lib import RobogymError  # noqa: F401
from .targets import TargetMixer, td_targets  # noqa: F401
from .returns import TargetCritic, nstep_returns  # noqa: F401
from .learn import GruScan, TrainableActor, gru_scan_backward, gru_scan_forward  # noqa: F401
from .mixers import MixerFn, TrainableMixer, mixer_backward, mixer_forward  # noqa: F401
from .params import load_config, make_params  # noqa: F401
from .vec_env import VecRobotariumEnv  # noqa: F401
from .wrapper import Wrapper, env_dict, register_gym_ids  # noqa: F401

__all__ = ["VecRobotariumEnv", "Wrapper", "env_dict", "register_gym_ids", "load_config", "make_params",
           "RobogymError", "render", "EpisodeBuffer", "TargetMixer", "td_targets", "TargetCritic",
           "nstep_returns", "TrainableActor", "GruScan", "gru_scan_forward", "gru_scan_backward",
           "TrainableMixer", "MixerFn", "mixer_forward", "mixer_backward"]
