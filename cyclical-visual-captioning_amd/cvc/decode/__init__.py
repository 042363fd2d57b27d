"""cvc.decode -- the inference side of the hot path (reference model/captioner.py:384-443): checkpoint packing (weights.py), the
engine (engine.py) and its per-path launch lists (path_packed.py, path_tile.py, path_ring.py; path_experimental.py for the schedules
of include/cvc_hip_experimental.h), and the ensemble engine (ensemble.py: several checkpoints behind one selection per step)."""
from .weights import *          # noqa: F401,F403
from .weights import _segs      # noqa: F401
from .engine import DecodeEngine  # noqa: F401
from .ensemble import EnsembleEngine, EnsembleOptions, interleave_members  # noqa: F401
