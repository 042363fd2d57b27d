"""Ensemble decoding: M checkpoints decode in lock-step behind ONE word choice per step ("Ensemble decoding").
Every member is an ordinary DecodeEngine over its own weights and its own clip features that runs every launch of its step but the
selection; after all members' launches of step t one cvc_ensemble_logprobs launch (csrc/ensemble.hip) writes the combined rows
[rows, V] into an engine-owned buffer and the EXISTING selection block of the mode runs on that buffer (nparts = 1, bias = NULL).  The
selection writes words[t + 1] (a beam: parent[t], scores, done flags, histories, keys) into the primary member's buffers; the
secondary members are built against the primary's words / parent tensors, so every member reads the word and the parent from
there.  One stream, one launch list, one captured graph; a sampling ensemble has one generator, the primary's."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .. import hip
from .mode import DecodeMode
from .engine import DecodeEngine, _capture_mode

COMBINES = ("prob", "logprob")          # arithmetic mean of the probabilities / weighted mean of the log-probs (product of experts)
_MODE_OPTIONS = ("beam", "path", "gate_ksplit", "gsk", "embgate", "lang_ksx", "sample_n", "temperature", "weights_dtype", "top_k", "top_p",
                 "forced_n", "no_repeat_ngram", "no_immediate_repeat", "min_len", "ban_words", "bad_endings", "beam_groups", "diversity",
                 "length_penalty", "force_n", "mix", "stochastic", "stochastic_tau", "beam_history")
_ENGINE_OPTIONS = ("inv_temp", "own_features", "driver", "seed", "tail")      # DecodeEngine's other keywords


def interleave_members(lists: Sequence[Sequence[Tuple]], T: int, combine, select) -> List[Tuple]:
    """M members' launch lists [(name, fn, args), ...] -> the ensemble's.  Every list is cut at its "word_select" entries, of which
    it must hold exactly T, one per step, each behind at least one launch of its step; step t then runs all members' segments in
    member order, combine(t, [member 0's word_select entry, ...]) and select(t); the members' trailing segments follow at the end
    in member order.  Pure: no device, no library -- the entries are opaque."""
    segs = []
    for m, launches in enumerate(lists):
        cut, sel = [[]], []
        for e in launches:
            if e[0] == "word_select":
                if not cut[-1]:
                    raise RuntimeError(f"EnsembleEngine: member {m}'s launch list has two word_select entries with nothing between "
                                       f"them (step {len(sel)})")
                sel.append(e)
                cut.append([])
            else:
                cut[-1].append(e)
        if len(sel) != T:
            raise RuntimeError(f"EnsembleEngine: member {m}'s launch list has {len(sel)} word_select entries, expected one per step "
                               f"(T = {T})")
        segs.append((cut, sel))
    out = []
    for t in range(T):
        for cut, _ in segs:
            out += cut[t]
        out.append(combine(t, [sel[t] for _, sel in segs]))
        out.append(select(t))
    for cut, _ in segs:
        out += cut[T]
    return out


def check_members(shapes: Sequence[Dict]) -> None:
    """Members must agree on what the one selection and the shared words / parents fix: B, N and V (dicts with those keys, member
    order).  A mismatch is refused with the member and the quantity."""
    for m, s in enumerate(shapes[1:], 1):
        for k in ("B", "N", "V"):
            if s[k] != shapes[0][k]:
                raise RuntimeError(f"EnsembleEngine: member {m} has {k} = {s[k]}, member 0 has {k} = {shapes[0][k]}: the members must agree "
                                   "on B, N, the proposal mask, V, T and unk_idx")


@dataclass(frozen=True)
class EnsembleOptions:
    """What an ensemble decode is asked to do, resolved in one pure step (as DecodeMode.resolve: no device, no library): the
    ensemble's own refusals first, then the members' mode with that function's refusals."""
    M: int
    combine: str
    geometric: bool
    logw: Tuple[float, ...]             # fp32 values (hip.ensemble_log_weights)
    mode: DecodeMode
    engine_options: Tuple               # the keywords every member's DecodeEngine is built with, sorted (key, value) pairs
    keep_rows: bool = False             # forced mode: the combined rows of every step are kept ([T, rows, V]; a teacher's soft targets)

    @classmethod
    def resolve(cls, M, T, V, member_weights=None, combine="prob", keep_rows=False, **options) -> "EnsembleOptions":
        if isinstance(M, bool) or not isinstance(M, int) or not 1 <= M <= hip.ENSEMBLE_MAX:
            raise RuntimeError(f"EnsembleEngine: an ensemble has 1 .. {hip.ENSEMBLE_MAX} members, got {M!r}")
        if combine not in COMBINES:
            raise RuntimeError(f"EnsembleEngine: combine must be one of {COMBINES}, got {combine!r}")
        try:
            logw = hip.ensemble_log_weights(member_weights, M)
        except RuntimeError as e:
            raise RuntimeError(f"EnsembleEngine: member_weights: {e}") from None
        unknown = sorted(set(options) - set(_MODE_OPTIONS) - set(_ENGINE_OPTIONS))
        if unknown:
            raise RuntimeError(f"EnsembleEngine: unknown options {unknown}")
        if options.get("weights_dtype", "fp32") == "bf16":
            raise RuntimeError('EnsembleEngine: weights_dtype="bf16" is refused: members on bf16-stored weights are not part of '
                               "ensemble decoding (the bf16 packs serve the packed greedy path with its own selection)")
        if options.get("mix", False):
            raise RuntimeError("EnsembleEngine: mix=True is refused: scheduled-sampling rollouts are a training mode of one model")
        if options.get("gsk") or options.get("gate_ksplit") or options.get("lang_ksx"):
            raise RuntimeError("EnsembleEngine: gsk / gate_ksplit / lang_ksx are refused: the members run on the default schedules")
        if options.get("tail") == "fused":
            raise RuntimeError('EnsembleEngine: tail="fused" is refused: the fused tail selects inside the member\'s own head, an '
                               "ensemble selects once over the combined rows")
        mode = DecodeMode.resolve(T, V, **{k: v for k, v in options.items() if k in _MODE_OPTIONS})
        if not isinstance(keep_rows, bool):
            raise RuntimeError(f"EnsembleEngine: keep_rows must be a bool, got {keep_rows!r}")
        if keep_rows and not mode.forced:
            raise RuntimeError("EnsembleEngine: keep_rows=True is refused outside the forced mode (forced_n): the kept rows are a "
                               "teacher's distributions along GIVEN captions; a decode that chooses its own words keeps the last step's only")
        return cls(M=M, combine=combine, geometric=combine == "logprob", logw=tuple(float(v) for v in logw), mode=mode,
                   engine_options=tuple(sorted(options.items(), key=lambda kv: kv[0])), keep_rows=keep_rows)


class EnsembleEngine:
    """EnsembleEngine(members=[(DecodeWeights, feats), ...], T, unk_idx, member_weights=None, combine="prob", **DecodeEngine options).
    run() returns what the DecodeEngine of that mode returns: logprob is the ENSEMBLE's log-prob of the chosen / given word (forced
    mode: rank under the combined distribution), the region attention is sum_m w_m att_m (member order, fp32, on the device inside
    the decode: cvc_ensemble_mix into the primary's att_steps), a beam backtracks over that buffer.  hypotheses / candidates /
    consensus / set_diversity / seed / rng_state / load_force_words are the primary member's, over the buffers the ensemble's
    selection filled.  M = 1: the single model through the combine launch.
    keep_rows=True (forced mode only): `combined` is [T, rows, V] and step t's combine launch and selection use combined[t] -- the
    ensemble's next-word distribution at every position of the given captions, in the t-major row order of the training loops' head
    (word-level distillation); nothing else in the launch list changes, so log-probs, ranks and attention keep their bits."""
    _warm = set()

    def __init__(self, members, T: int, unk_idx: int, member_weights=None, combine: str = "prob", keep_rows: bool = False, **options):
        members = list(members)
        V = getattr(members[0][0], "V", None) if members else None
        o = self.options = EnsembleOptions.resolve(len(members), T, V, member_weights, combine, keep_rows=keep_rows, **options)
        self.keep_rows = o.keep_rows
        self.M, self.combine, self.mode = o.M, o.combine, o.mode
        self.logw = (C.c_float * o.M)(*o.logw)
        kw = dict(o.engine_options)
        feats0 = members[0][1]
        pool0 = feats0["pool_feats"]
        check_members([dict(B=f["pool_feats"].shape[0], N=f["pool_feats"].shape[1], V=w.V) for w, f in members])
        self.members: List[DecodeEngine] = []
        for m, (w, f) in enumerate(members):
            if m > 0 and not torch.equal(hip._mask(f["pnt_mask"]), hip._mask(feats0["pnt_mask"])):
                raise RuntimeError(f"EnsembleEngine: member {m}'s proposal mask (pnt_mask) differs from member 0's: the members must agree "
                                   "on B, N, the proposal mask, V, T and unk_idx")
            self.members.append(DecodeEngine._member(self.members[0] if m else None, w, f, T, unk_idx, **kw))
        p = self.primary = self.members[0]
        self.T, self.rows, self.V = p.T, p.rows, p.W.V
        # the rows the selection reads (keep_rows: one [rows, V] matrix per step)
        self.combined = torch.zeros(*((self.T,) if self.keep_rows else ()), self.rows, self.V, device=pool0.device, dtype=torch.float32)
        self.att_src = (C.c_void_p * o.M)(*(e.att_steps.data_ptr() for e in self.members))
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._keep: List = []
        self._launches = self._build_launches()

    def __getattr__(self, name):
        # what the ensemble's selection fills lives in the primary member: its buffers, flags and read-side methods
        if name in ("primary", "members"):
            raise AttributeError(name)
        return getattr(self.primary, name)

    # ------------------------------------------------------------------ launch list

    def _rows_ptr(self, t) -> int:
        return (self.combined[t] if self.keep_rows else self.combined).data_ptr()

    def _combine_entry(self, t, selects):
        src = (hip.EnsembleSrc * self.M)()
        for m, (_, fn, args) in enumerate(selects):
            if fn is not None or len(args) != 4:
                raise RuntimeError(f"EnsembleEngine: member {m}'s word_select entry of step {t} is not a member's placeholder")
            src[m] = hip.EnsembleSrc(*args)
        self._keep.append(src)
        return ("ensemble_combine", hip.lib().cvc_ensemble_logprobs, (src, self.M, self.logw, int(self.options.geometric), self.rows, self.V,
                                                                     self._rows_ptr(t), self.V))

    def _select_entry(self, t):
        p, comb = self.primary, self._rows_ptr(t)
        if p.beam > 1:
            return p._word_select_beam(t, comb, 1, 0, None, real=True)
        if p.sampling or p.forced or p.constrained:
            return p._word_select_sampled(t, comb, 1, 0, None, real=True)
        return ("word_select", hip.lib().cvc_top2_unk, (comb, self.rows, self.V, p.unk, p.words[t + 1].data_ptr(), 1,
                                                        p.logprob[t].data_ptr()))

    def _build_launches(self):
        self._keep = []
        out = interleave_members([e._python_launches() for e in self.members], self.T, self._combine_entry, self._select_entry)
        n = self.primary.att_steps.numel()
        # the region attention: sum_m w_m att_m into the primary's att_steps (element-wise in place over source 0)
        out.append(("ensemble_attention", hip.lib().cvc_ensemble_mix, (self.att_src, self.M, self.logw, n, self.primary.att_steps.data_ptr())))
        return out

    def _run_once(self):
        for e in self.members:
            e._reset()
        stream = torch.cuda.current_stream().cuda_stream
        for name, fn, args in self._launches:
            if fn == "copy":
                args[0].copy_(args[1])
            else:
                rc = fn(*args, stream)
                if rc != 0:
                    hip._check(rc, name)
        self.primary._finish_beam()

    # ------------------------------------------------------------------ the engine's surface

    def run(self):
        """One full T-step decode of all members -> the tuple DecodeEngine.run() returns in this mode (views of the primary's
        buffers; clone to keep across runs)."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._run_once()
        return self.primary._result()

    def capture(self):
        """The whole M-member decode as one HIP graph; DecodeEngine.capture's warm-up rule (the first capture of a path and mode in the
        process runs once outside the capture, without advancing the generator)."""
        p = self.primary
        key = tuple((e.packed, e.tile) for e in self.members) + (self.combine,) + self.mode.flags
        if key not in EnsembleEngine._warm:
            saved = p.rng.clone() if (p.sampling or p.stoch) else None
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._run_once()
            torch.cuda.current_stream().wait_stream(s)
            if saved is not None:
                p.rng.copy_(saved)
            EnsembleEngine._warm.add(key)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=_capture_mode()):
            self._run_once()
        self.graph = g
        return self

    def load_features(self, feats: Sequence[Dict[str, torch.Tensor]]):
        """The next batch of the same shapes, one feature dict per member in member order (own_features=True)."""
        feats = list(feats)
        if len(feats) != self.M:
            raise RuntimeError(f"EnsembleEngine.load_features: {self.M} members need {self.M} feature dicts, got {len(feats)}")
        for e, f in zip(self.members, feats):
            e.load_features(f)
        return self

    def load_captions(self, words: torch.Tensor, frame_mask: Optional[torch.Tensor] = None):
        """Forced mode: the captions to follow, into the words every member reads (DecodeEngine.load_captions).  A frame mask is
        refused: the frame-masked scores are one member's, the ensemble has no such output."""
        if frame_mask is not None:
            raise RuntimeError("EnsembleEngine.load_captions: a frame mask is refused (the frame-masked attention scores are a single "
                               "member's output)")
        self.primary.load_captions(words)
        return self

    def seed(self, s: int):
        self.primary.seed(s)
        return self

    def load_force_words(self, words):
        self.primary.load_force_words(words)
        return self

    def bind_features(self, feats):
        raise RuntimeError("EnsembleEngine.bind_features: an ensemble runs no C-driver plan; use own_features=True and load_features")

    def run_timed(self):
        raise RuntimeError("EnsembleEngine.run_timed: per-launch timing is a single engine's tool (tools/bench_ensemble.py measures "
                           "the ensemble)")

    def set_mix_prob(self, p):
        raise RuntimeError("EnsembleEngine.set_mix_prob: the mixed mode (mix=True) is not part of ensemble decoding")
