"""What a decode is asked to do, resolved from DecodeEngine's option arguments in one pure step: DecodeMode.resolve checks the
options against each other (every refusal that needs neither the batch nor the library), normalises them and derives the flags the
engine, its path mixins and the tests read.  No device, no library: the result is an immutable, hashable value.  What depends on the
batch's shape or on how the library was built (packed / tile, the embedding-gate schedule, gsk / lang_ksx, the fused tail, the bf16
row limit) is decided in DecodeEngine.__init__ once the features are read.  The options themselves are documented there."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

WEIGHTS_DTYPES = ("fp32", "bf16")
CONSTRAINT_T_MAX = 64            # history steps of cvc_constrained_select_parts (one lane per step)
CONSTRAINT_LIST_MAX = 256        # entries of its ban_words / bad_endings lists (one thread per entry)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_bool(v):
    return isinstance(v, (bool, np.bool_))


def _constraints(no_repeat_ngram, no_immediate_repeat, min_len, ban_words, bad_endings):
    """The five constraint arguments checked and normalised: (n, immediate, min_len, ban ids, bad-ending ids), the lists sorted and
    without duplicates.  Malformed values raise the engine's RuntimeError (ids are checked against V by the caller)."""
    for name, v, hi in (("no_repeat_ngram", no_repeat_ngram, CONSTRAINT_T_MAX), ("min_len", min_len, None)):
        if not _is_int(v) or v < 0 or (hi is not None and v > hi):
            raise RuntimeError(f"DecodeEngine: {name} must be an integer >= 0 (0 = off)" + (f" and <= {hi}" if hi else "") + f", got {v!r}")
    if not _is_bool(no_immediate_repeat) and no_immediate_repeat not in (0, 1):
        raise RuntimeError(f"DecodeEngine: no_immediate_repeat must be a bool, got {no_immediate_repeat!r}")
    lists = []
    for name, given in (("ban_words", ban_words), ("bad_endings", bad_endings)):
        ids = [] if given is None else list(given) if isinstance(given, (list, tuple, set, frozenset, np.ndarray)) else None
        if ids is None or not all(_is_int(v) and v >= 0 for v in ids):
            raise RuntimeError(f"DecodeEngine: {name} must be a list of word ids (integers >= 0), got {given!r}")
        ids = tuple(sorted({int(v) for v in ids}))
        if len(ids) > CONSTRAINT_LIST_MAX:
            raise RuntimeError(f"DecodeEngine: {name} takes at most {CONSTRAINT_LIST_MAX} ids, got {len(ids)}")
        lists.append(ids)
    return int(no_repeat_ngram), bool(no_immediate_repeat), int(min_len), lists[0], lists[1]


@dataclass(frozen=True)
class DecodeMode:
    """The normalised options and derived flags of one decode, under the names DecodeEngine carries them (ENGINE_FIELDS are copied
    onto the engine).  inv_tau is None where no selection block reads it (neither sampling nor constrained), stoch_inv_tau without
    stochastic=True.  gsk / gate_ksplit / lang_ksx are the schedule REQUESTS as the mode leaves them -- None = the engine's default,
    False where the mode excludes them; whether a request can be served is the engine's check."""
    T: int
    beam: int
    weights_dtype: str
    bf16w: bool
    forced: bool
    cons: Tuple
    constrained: bool
    mix: bool
    beam_hist: bool
    groups: int
    diversity: float
    length_penalty: float
    grouped: bool
    force_n: int
    forcing: bool
    ranked: bool                     # the decode ends with cvc_beam_rank (cvc_beam_rank_force) / cvc_beam_backtrack_from
    stoch: bool
    stoch_inv_tau: Optional[float]
    sampling: bool
    given: bool                      # the next step's word is read from words[t + 1]: the sampling launch lists
    top_k: int
    top_p: float
    trunc: bool
    inv_tau: Optional[float]         # 0.0: the constrained block's arg-max mode
    nq: int                          # queries per clip: beams, samples or given captions (attention passes, gate_fc rows)
    gsk: object
    gate_ksplit: object
    lang_ksx: object

    ENGINE_FIELDS = ("T", "beam", "weights_dtype", "bf16w", "forced", "cons", "constrained", "mix", "beam_hist", "groups", "diversity",
                     "length_penalty", "grouped", "force_n", "forcing", "ranked", "stoch", "stoch_inv_tau", "sampling", "given", "top_k",
                     "top_p", "trunc", "inv_tau", "nq")

    @property
    def flags(self):
        """What distinguishes the launch lists of two modes (with the engine's packed / tile / fused_tail: the key of the first,
        uncaptured decode in DecodeEngine.capture) -- flags only, no option values: a finer key would add warm-up decodes."""
        return (self.beam > 1, self.sampling, self.weights_dtype, self.trunc, self.forced, self.constrained, self.beam_hist, self.grouped,
                self.ranked, self.forcing, self.mix, self.stoch)

    @classmethod
    def resolve(cls, T, V, beam=1, path="auto", gate_ksplit=None, gsk=None, embgate=None, lang_ksx=None, sample_n=1, temperature=None,
                weights_dtype="fp32", top_k=0, top_p=1.0, forced_n=0, no_repeat_ngram=0, no_immediate_repeat=False, min_len=0,
                ban_words=None, bad_endings=None, beam_groups=1, diversity=0.0, length_penalty=0.0, force_n=0, mix=False,
                stochastic=False, stochastic_tau=1.0, beam_history=False) -> "DecodeMode":
        """DecodeEngine's options (its defaults), T and the vocabulary size V -> the mode, or the RuntimeError of the first check that
        fails; the order of the checks decides which refusal a call with several faults gets (tests/golden/decode_modes.json).  V
        may be None: it is read only when ban_words / bad_endings hold ids."""
        T, beam = int(T), int(beam)
        experimental = bool(gsk or gate_ksplit or lang_ksx)          # a schedule of include/cvc_hip_experimental.h was asked for
        default_schedules = "the default schedules only (no gsk / gate_ksplit / lang_ksx)"

        def refuse_experimental(who):
            if experimental:
                raise RuntimeError(f"DecodeEngine: {who} runs on {default_schedules}")
        if weights_dtype not in WEIGHTS_DTYPES:
            raise RuntimeError(f"DecodeEngine: weights_dtype must be one of {WEIGHTS_DTYPES}, got {weights_dtype!r}")
        bf16w = weights_dtype == "bf16"
        if not _is_int(forced_n) or forced_n < 0:
            raise RuntimeError(f"DecodeEngine: forced_n must be an integer >= 0 (0 = off), got {forced_n!r}")
        forced = int(forced_n) >= 1
        if forced:
            if beam != 1:
                raise RuntimeError("DecodeEngine: the forced mode (forced_n) and beam search (beam > 1) exclude each other")
            if temperature is not None:
                raise RuntimeError("DecodeEngine: the forced mode (forced_n) follows given words: it takes no sampling temperature")
            refuse_experimental("the forced mode")
        cons = _constraints(no_repeat_ngram, no_immediate_repeat, min_len, ban_words, bad_endings)
        constrained = any(cons)
        if not _is_bool(mix):
            raise RuntimeError(f"DecodeEngine: mix must be a bool, got {mix!r}")
        mix = bool(mix)
        if mix:
            why = None
            if temperature is None:
                why = "it draws from the sampling engine: it needs a temperature"
            elif beam != 1:
                why = "beam search (beam > 1) chooses its own words"
            elif forced:
                why = "the forced mode (forced_n) follows given words only"
            elif constrained:
                why = "constrained decoding is not part of it"
            elif (_is_int(top_k) and top_k != 0) or top_p != 1.0:
                why = "top_k / top_p truncation is not part of it"
            elif bf16w:
                why = 'weights_dtype="bf16" is not part of it'
            if why is not None:
                raise RuntimeError(f"DecodeEngine: the mixed mode (mix=True) is refused: {why}")
        if not _is_bool(beam_history):
            raise RuntimeError(f"DecodeEngine: beam_history must be a bool, got {beam_history!r}")
        beam_hist = bool(beam_history)
        if beam_hist:
            if beam == 1:
                raise RuntimeError("DecodeEngine: beam_history keeps the histories of beam search: it needs beam > 1")
            if T > CONSTRAINT_T_MAX:
                raise RuntimeError(f"DecodeEngine: beam_history covers T <= {CONSTRAINT_T_MAX} steps, got T = {T}")
            refuse_experimental("beam_history")
        if not _is_int(beam_groups) or beam_groups < 1:
            raise RuntimeError(f"DecodeEngine: beam_groups must be an integer >= 1 (1 = off), got {beam_groups!r}")
        if not (0.0 <= float(diversity) < float("inf")):
            raise RuntimeError(f"DecodeEngine: diversity must be a finite number >= 0 (negative values are refused), got {diversity!r}")
        if not (0.0 <= float(length_penalty) < float("inf")):
            raise RuntimeError(f"DecodeEngine: length_penalty must be a finite number >= 0, got {length_penalty!r}")
        groups, diversity, length_penalty = int(beam_groups), float(diversity), float(length_penalty)
        grouped = groups > 1
        if not _is_int(force_n) or not 0 <= force_n <= 3:
            raise RuntimeError(f"DecodeEngine: force_n must be an integer in 0 .. 3 (0 = off), got {force_n!r}")
        force_n = int(force_n)
        forcing = force_n >= 1
        if forcing:
            if beam == 1:
                raise RuntimeError("DecodeEngine: force_n is an option of beam search: it needs beam > 1")
            if not beam_hist:
                raise RuntimeError("DecodeEngine: force_n needs beam_history=True (the forced words a hypothesis has met are read from "
                                   "its own history)")
            if beam % (force_n + 1) != 0:
                raise RuntimeError(f"DecodeEngine: force_n = {force_n} needs beam % (force_n + 1) == 0 (one bank per number of "
                                   f"forced words met), got beam = {beam}")
            if grouped:
                raise RuntimeError("DecodeEngine: force_n and beam_groups > 1 exclude each other (banks and groups both divide the "
                                   "clip's slots)")
        ranked = grouped or length_penalty != 0.0 or forcing
        if ranked:
            what = "beam_groups > 1" if grouped else "length_penalty != 0"
            if beam == 1:
                raise RuntimeError(f"DecodeEngine: {what} is an option of beam search: it needs beam > 1")
            if not beam_hist:
                raise RuntimeError(f"DecodeEngine: {what} needs beam_history=True (the groups and the ranking read the hypotheses' "
                                   "own histories)")
            if beam % groups != 0:
                raise RuntimeError(f"DecodeEngine: beam_groups = {groups} must divide beam = {beam}")
        if diversity != 0.0 and not grouped:
            raise RuntimeError("DecodeEngine: diversity acts between groups: it needs beam_groups > 1")
        if not _is_bool(stochastic):
            raise RuntimeError(f"DecodeEngine: stochastic must be a bool, got {stochastic!r}")
        stoch, stoch_inv_tau = bool(stochastic), None
        if stoch:
            why = None
            if beam == 1 or not beam_hist:
                why = "it is a beam search over hypotheses that carry their histories: it needs beam > 1 and beam_history=True"
            elif grouped or diversity != 0.0:
                why = "beam_groups > 1 / diversity are not part of it (the slots are one sample in draw order)"
            elif length_penalty != 0.0:
                why = "length_penalty is not part of it (the slots are ranked by their perturbed keys)"
            elif forcing:
                why = "force_n is not part of it"
            elif temperature is not None:
                why = "it takes no sampling temperature (stochastic_tau is its own)"
            elif experimental:
                why = f"it runs on {default_schedules}"
            elif not (0.0 < float(stochastic_tau) < float("inf")):
                why = f"stochastic_tau must be a positive finite number, got {stochastic_tau!r}"
            if why is not None:
                raise RuntimeError(f"DecodeEngine: stochastic beam search (stochastic=True) is refused: {why}")
            stoch_inv_tau = 1.0 / float(stochastic_tau)
        if constrained:
            if beam != 1 and not beam_hist:
                raise RuntimeError("DecodeEngine: constrained decoding under beam search (beam > 1) needs beam_history=True (a "
                                   "hypothesis' history follows its parents: it has to travel with it)")
            if forced:
                raise RuntimeError("DecodeEngine: the forced mode (forced_n) follows given words: it takes no constraints")
            refuse_experimental("constrained decoding")
            if T > CONSTRAINT_T_MAX:
                raise RuntimeError(f"DecodeEngine: constrained decoding covers T <= {CONSTRAINT_T_MAX} steps, got T = {T}")
            bad = [v for v in cons[3] + cons[4] if v >= V]
            if bad:
                raise RuntimeError(f"DecodeEngine: ban_words / bad_endings ids outside [0, V = {V}): {bad}")
        if bf16w:
            why = None
            if beam != 1:
                why = f"beam search (beam = {beam}) runs on the tile path"
            elif int(sample_n) != 1:
                why = f"sample_n = {sample_n} > 1 runs on the tile path"
            elif int(forced_n) > 1:
                why = f"forced_n = {forced_n} > 1 runs on the tile path"
            elif path in ("tile", "ring"):
                why = f'path="{path}" was asked for'
            elif experimental:
                why = "gsk / gate_ksplit / lang_ksx are experimental schedules of the fp32 kernels"
            elif embgate is not None and not embgate:
                why = "embgate=False: the packed path without the embedding-gate schedule"
            if why is not None:
                raise RuntimeError(f'DecodeEngine: weights_dtype="bf16" covers the packed path with the embedding-gate schedule only '
                                   f"(beam = 1, one caption per clip, <= 64 rows); refused: {why}")
        sampling = temperature is not None
        # (constrained beam search chooses in the beam block and reorders by parent like every beam engine)
        given = sampling or forced or (constrained and beam == 1)
        if not _is_int(top_k) or top_k < 0:
            raise RuntimeError(f"DecodeEngine: top_k must be an integer >= 0 (0 = off), got {top_k!r}")
        if not (0.0 < float(top_p) <= 1.0):
            raise RuntimeError(f"DecodeEngine: top_p must lie in (0, 1] (1 = off), got {top_p!r}")
        top_k, top_p = int(top_k), float(top_p)
        trunc = top_k > 0 or top_p < 1.0
        if trunc and not sampling:
            raise RuntimeError("DecodeEngine: top_k / top_p truncate the sampled distribution: they need a sampling temperature")
        inv_tau = 0.0 if constrained else None
        if sampling:
            tau = float(temperature)
            if not (0.0 < tau < float("inf")):
                raise RuntimeError(f"DecodeEngine: the sampling temperature must be a positive finite number, got {temperature!r}")
            if beam != 1:
                raise RuntimeError("DecodeEngine: sampling (temperature) and beam search (beam > 1) exclude each other")
            refuse_experimental("sampling")
            if int(sample_n) < 1:
                raise RuntimeError(f"DecodeEngine: sample_n must be >= 1, got {sample_n}")
            inv_tau = 1.0 / tau
        elif int(sample_n) != 1:
            raise RuntimeError("DecodeEngine: sample_n > 1 needs a sampling temperature")
        # The modes that passed refuse_experimental (or bf16's check) carry the requests as "off": the engine then neither takes
        # its defaults (GATE_KSPLIT_DEFAULT, LANG_KSX_DEFAULT) nor asks the library for them.
        if forced or constrained or sampling:
            gate_ksplit, lang_ksx = False, False
        if bf16w:
            gsk, gate_ksplit, lang_ksx = False, False, False
        return cls(T=T, beam=beam, weights_dtype=weights_dtype, bf16w=bf16w, forced=forced, cons=cons, constrained=constrained, mix=mix,
                   beam_hist=beam_hist, groups=groups, diversity=diversity, length_penalty=length_penalty, grouped=grouped,
                   force_n=force_n, forcing=forcing, ranked=ranked, stoch=stoch, stoch_inv_tau=stoch_inv_tau, sampling=sampling,
                   given=given, top_k=top_k, top_p=top_p, trunc=trunc, inv_tau=inv_tau,
                   nq=int(sample_n) if sampling else (int(forced_n) if forced else beam), gsk=gsk, gate_ksplit=gate_ksplit,
                   lang_ksx=lang_ksx)
