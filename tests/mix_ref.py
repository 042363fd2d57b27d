"""Host restatement of the mixed selection block's coin (csrc/mix.hip, cvc_mixed_select_parts) and the small shared pieces of the
scheduled-sampling tests: the coin is the counter-based hash of csrc/dropout_rng.h (cvc.synth.dropout_hash) at site CVC_MIX_SITE + t
with the row as counter, turned into a uniform the way the sampler's noise is."""
import numpy as np

from cvc import synth
import sample_oracle as S

MIX_SITE = 0x4D000000             # include/cvc_hip_blocks.h, CVC_MIX_SITE
T_MAX = 64                        # the steps the sites must stay disjoint for


def coin_uniform(seed: int, call: int, t: int, rows: int) -> np.ndarray:
    """u [rows] fp32 = ((h >> 9) + 0.5) * 2^-23 of h = hash(seed, call, MIX_SITE + t, r): exact in fp32, strictly inside (0, 1)"""
    lo, hi = S.seed_words(seed)
    h = synth.dropout_hash(lo, hi, call, MIX_SITE + t, np.arange(rows, dtype=np.uint32))
    return ((np.asarray(h, dtype=np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def took(seed: int, call: int, t: int, rows: int, p: float) -> np.ndarray:
    """took [rows] bool: the fp32 comparison u < p the kernel makes"""
    return coin_uniform(seed, call, t, rows) < np.float32(p)


def took_steps(seed: int, call: int, T: int, rows: int, p: float) -> np.ndarray:
    """[rows, T]: column t is step t's coin (it decides the input of step t + 1)"""
    return np.stack([took(seed, call, t, rows, p) for t in range(T)], 1)
