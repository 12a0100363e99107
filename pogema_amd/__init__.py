"""pogema_amd -- MI355X-native vectorized POGEMA step engine (drop-in for the reference's
grid.py / envs.py reset()/step() hot path).  See DESIGN.md."""
from .grid_config import (GridConfig, Easy8x8, Normal8x8, Hard8x8, Easy16x16, Hard16x16, Easy32x32,
                          Hard32x32, Easy64x64, Hard64x64)

__version__ = "0.1.0"

from .semantics import Semantics
from ._lib import OUTCOMES, NUM_OUTCOMES  # the codes of move_outcomes(), index = code
from ._lib import TOKENS  # the vocabulary of agent_tokens() (docs/SPEC.md S21)
from ._lib import CONFLICT_KINDS  # the kind bits of path_conflicts(), name -> bit (docs/SPEC.md S26)
from .tokens import token_length

__all__ = ["GridConfig", "Semantics", "OUTCOMES", "NUM_OUTCOMES", "CONFLICT_KINDS", "TOKENS", "token_length", "TokenHistory", "release_cached_buffers", "VecPogema", "PipelinedVecPogema", "PibtPolicy", "Pogema", "pogema_v0", "Easy8x8", "Normal8x8", "Hard8x8", "Easy16x16",
           "Hard16x16", "Easy32x32", "Hard32x32", "Easy64x64", "Hard64x64"]


def release_cached_buffers() -> None:
    """Gives back the zone-spread observation buffers that closed environments left mapped for their successors
    (pogema_amd.buffers.ParkedBuffers: at most PGX_POOL_CACHE_MB, default 2.5 GiB) -- for callers who close an
    environment to make room for something else."""
    from .buffers import ParkedBuffers, WalkVerdicts
    ParkedBuffers.clear()
    WalkVerdicts.clear()  # ... and the next engine may walk the device again


def __getattr__(name):
    # engine classes import torch + the HIP library lazily so that `GridConfig` stays importable anywhere
    if name == "VecPogema":
        from .vec_env import VecPogema
        return VecPogema
    if name == "PipelinedVecPogema":
        from .pipeline import PipelinedVecPogema
        return PipelinedVecPogema
    if name == "PibtPolicy":
        from .pibt import PibtPolicy
        return PibtPolicy
    if name == "TokenHistory":
        from .tokens import TokenHistory
        return TokenHistory
    if name in ("Pogema", "pogema_v0", "PogemaParallel"):
        from . import envs
        return getattr(envs, name)
    raise AttributeError(name)
