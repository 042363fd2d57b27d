"""The decode engine: binds a checkpoint (DecodeWeights) and one batch of clip features to a flat per-step launch list, runs it
through the C drivers (cvc_decode_greedy / cvc_decode_beam: one host call per decode) or eagerly, optionally as a HIP-graph replay.
The per-path buffers and launch lists live in path_packed / path_tile / path_ring (/ path_experimental)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from .. import hip
from .weights import *          # noqa: F401,F403  (packers, layouts, cache plan, switches)
from .weights import _segs
from .mode import DecodeMode
from .path_packed import PackedPath
from .path_tile import TilePath
from .path_ring import RingPath
from .path_experimental import ExperimentalPaths


def _capture_mode() -> str:
    """"global" (torch's default) unless a c10d "nccl" process group is up in this process: its watchdog thread polls the events of
    earlier collectives with hipEventQuery, which fails with hipErrorStreamCaptureUnsupported while ANOTHER thread captures in
    global mode -- the watchdog then dies with that exception and takes the rank down.  "thread_local" confines the capture's
    restrictions to the capturing thread; the decode graph contains no collective, so no event of that group is ever recorded in
    the capturing stream.  (The package's own runs -- bench.py, cvc.main -- keep torch.distributed on gloo and the exchange on
    cvc.comm.RcclComm: no such thread exists there.)"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl":
        return "thread_local"
    return "global"


class DecodeEngine(PackedPath, TilePath, RingPath, ExperimentalPaths):
    """Binds weights + one batch of clip features to preallocated state and a launch list."""
    _warm = set()
    _ensemble = None                 # an ensemble's member: True (the primary) or the primary engine (DecodeEngine._member)

    @classmethod
    def _member(cls, primary, *args, **options):
        """Internal (cvc/decode/ensemble.py): an engine built as a member of an EnsembleEngine -- primary = None for the primary member,
        else the primary engine whose words / parents this one reads.  What that changes is in __init__'s documentation."""
        self = cls.__new__(cls)
        self._ensemble = True if primary is None else primary
        self.__init__(*args, **options)
        return self

    def __init__(self, weights: DecodeWeights, feats: Dict[str, torch.Tensor], T: int, unk_idx: int, beam: int = 1,
                 inv_temp: float = 1.0, own_features: bool = False, path: str = "auto", gate_ksplit: Optional[bool] = None,
                 driver: bool = True, gsk: Optional[bool] = None, embgate: Optional[bool] = None, lang_ksx: Optional[bool] = None,
                 sample_n: int = 1, temperature: Optional[float] = None, seed: Optional[int] = None, weights_dtype: str = "fp32",
                 top_k: int = 0, top_p: float = 1.0, forced_n: int = 0, no_repeat_ngram: int = 0, no_immediate_repeat: bool = False,
                 min_len: int = 0, ban_words=None, bad_endings=None, beam_groups: int = 1, diversity: float = 0.0,
                 length_penalty: float = 0.0, force_n: int = 0, tail: Optional[str] = None, mix: bool = False,
                 stochastic: bool = False, stochastic_tau: float = 1.0, beam_history: bool = False):
        """driver: enqueue the decode through the C-ABI drivers cvc_decode_greedy / cvc_decode_beam (one host call per decode);
        False walks the launch list in Python (one ctypes call per kernel; tests compare the two).
        embgate: packed path only -- the embedding-gate schedule (the embedded word's share of the att-LSTM gates is a row of
        a per-checkpoint table: 34 MB less to stream per step at config 2, and the gate GEMM no longer waits for the word).  None = on when the table fits EMBGATE_MAX_BYTES; tests compare on / off.
        lang_ksx: packed path, R = 2048 -- the language cell on the K-split gate GEMM with the exchange finish
        (cvc_packed_lstm_ksx_fwd: activations read once per 256 gate rows instead of once per 32; the tile's 8 K slices
        exchange their partial tiles inside the launch).  None = off (measured no faster inside the decode graph; CVC_LANG_KSX=1:
        on); the exchange's error word is checked after the first decode and the engine re-binds without it if it is set.
        gsk: packed path only -- True selects the grouped stream-K schedule (csrc/gemm_gsk.hip; measured slower than the
        embedding-gate schedule, kept selectable and tested; needs R % 64 == 0, split-product arithmetic).
        path: "auto" picks packed (greedy, <= 64 rows) / tile (> 64 rows or beams) / ring (odd widths); "ring" forces the
        row-major fallback kernels, "tile" the tile path at any row count (tests compare the paths).
        own_features: keep private copies of the clip features, so that the bound launch list (and a captured HIP
        graph) can be reused for the next batch of the same shape through load_features().
        temperature: None = the arg-max word (greedy / beam, as always).  A value tau > 0 samples every word from softmax(logits /
        tau) without UNK (Gumbel-max, csrc/sample.hip), sample_n captions per clip (row b * sample_n + j is sample j of clip b),
        noise from the engine's own generator state {seed_lo, seed_hi, call, 0} (seed(); every decode first advances `call`).
        A sampling engine walks its launch list from Python (no C driver); beam > 1, gsk, gate_ksplit, lang_ksx and the packed
        path without the embedding-gate schedule are refused.
        top_k, top_p: truncation of the sampled distribution (both need a temperature): top_k = k > 0 keeps the k
        most likely words (and every word tied with the k-th), top_p = p < 1 then the smallest set of most likely words whose mass
        under softmax(z / tau) over the kept words reaches p (nucleus sampling).  The word is the one the untruncated sampler draws
        from the same state whenever that lies in the kept set; logprob stays the model's log-prob (full vocabulary -- not the
        truncated distribution's).  A truncating engine owns self.cutoff [T, rows] (the smallest kept logit) and self.kept
        [T, rows] (int32, the size of the kept set); 0 / 1.0 = off: the launch list of a temperature-only engine.
        weights_dtype: "fp32" (default) or "bf16" -- a precision setting, not a speed switch: the six weight matrices
        (BF16_ROUNDED_KEYS) are rounded to bf16 (nearest even) when the engine binds the checkpoint and stored as bf16 packs
        (the WB16 mode of csrc/gemm_packed.hip: half the weight bytes per step, three MFMAs per product instead of six); the decode computes
        what the fp32 engine computes on a checkpoint that holds the rounded values -- activations, state, accumulation, softmax
        and word selection stay fp32.  Packed path with the embedding-gate schedule only (greedy or sampling with sample_n = 1,
        <= 64 rows); the engine walks its launch list from Python (no C driver) and capture() turns it into a HIP graph.  Every
        other configuration is refused with a RuntimeError -- the mode never runs in fp32 instead.
        forced_n: 0 = off.  n >= 1: the teacher-forced mode -- the engine chooses no word, it follows n given
        captions per clip (load_captions(); row b * n + j is caption j of clip b) and the selection block cvc_forced_select_parts
        writes the given word's log-prob (self.logprob [T, rows]) and its rank among the logits (self.rank [T, rows] int32).  The
        launch lists are the sampling paths' with that block as word_select, on the same choice of paths with the same refusals
        (beam > 1, a temperature, gsk, gate_ksplit, lang_ksx, the packed path without the embedding-gate schedule); no C driver.
        With a frame mask bound (load_captions) the region attention also writes its frame-masked pre-softmax scores per step
        (self.fm_steps [T, rows, N]): the att2_weights of the training pass, what grounding on given sentences reads.
        no_repeat_ngram, no_immediate_repeat, min_len, ban_words, bad_endings: constrained decoding (the rule is
        the comment of cvc_constrained_select_parts in include/cvc_hip_blocks.h).  Step t never chooses UNK, a word of ban_words, a
        word that would complete an n-gram the row already holds (no_repeat_ngram = n), the previous word (no_immediate_repeat),
        word 0 before step min_len or right after a word of bad_endings.  All five off (the default): nothing changes.  Any of
        them on: the sampling paths' launch lists with that block as word_select, with or without a temperature (without: the
        arg-max over the allowed words), with sample_n and top_k / top_p; no C driver; capture() works (t and the rules are launch
        constants, the lists live in engine-owned device buffers).  The engine owns self.nbanned [T, rows] int32 (the size of the
        ban set) and run() returns the sampling engine's tuple in both modes.  Refused: beam > 1 without beam_history, forced_n,
        gsk / gate_ksplit / lang_ksx, the packed path without the embedding-gate schedule, T > 64, malformed values and ids outside
        [0, V).
        beam_history: beam search whose hypotheses carry their own histories on the device ("Constrained beam
        search"; needs beam > 1, T <= 64, no gsk / gate_ksplit / lang_ksx).  The engine owns self.bhist [2, T, rows] int64 and its
        word_select launch is cvc_beam_select_hist_parts with hist_in = bhist[t & 1] and hist_out = bhist[(t + 1) & 1], on the tile
        path (fused slabs or finished logits) and on the ring path; the launch list is walked from Python or captured (no C
        driver).  run() returns what a beam engine returns, with the plain beam engine's bits; hypotheses() returns all `beam`
        hypotheses of every clip in rank order (n-best).  With it the five constraints run under beam search: the rule is applied
        to every hypothesis' own history (a frozen hypothesis is left alone), scores stay sums of the model's log-probs, and
        self.nbanned [T, rows] is filled.
        beam_groups, diversity, length_penalty: diverse (group) beam search and a length penalty on the final ranking (DESIGN
        section 7, "Diverse beam search"; the rule is the comment of cvc_beam_select_groups_parts in include/cvc_hip_blocks.h).
        beam_groups = G > 1 splits a clip's beam = G * bd slots into G groups that are served in turn within a step, later groups
        paying diversity = lambda >= 0 per earlier live selection of the same word (Hamming diversity); the word_select launch is
        cvc_beam_select_groups_parts on the tile path (fused slabs or finished logits) and on the ring path, G, lambda and t are
        launch constants (capture() works), and it composes with the five constraints.  length_penalty = alpha > 0 ranks the final
        hypotheses by norm = score / len^alpha, len = the words up to and including the first 0.  With either on, the decode ends
        with cvc_beam_rank (self.order [B, beam] int64, self.norm, self.hyp_len) and cvc_beam_backtrack_from(order[:, 0]), both
        inside a captured graph: run() returns the best hypothesis by norm, its attention rows and the final scores, and
        hypotheses(ranked=True) returns (seq, score, norm, group) in that order.  Both need beam_history=True and beam > 1;
        beam % beam_groups != 0, a negative diversity and diversity != 0 with one group are refused.  1 / 0.0 / 0.0 (the default):
        nothing changes.
        force_n: 0 = off.  C in 1 .. 3: lexically constrained beam search ("Forced words"; the rule is the comment of
        cvc_beam_select_force_parts in include/cvc_hip_blocks.h) -- up to C words per clip that the caption should contain
        (load_force_words(); -1 = unused, so clips may have fewer).  A clip's beam = (C + 1) * bd slots are C + 1 banks by the number
        of forced words a hypothesis has met; a candidate goes to the bank of its row's count, one higher if its word is a forced
        word the row has not met, and every bank keeps its own bd best.  The word_select launch is cvc_beam_select_force_parts on
        the tile path (fused slabs or finished logits) and on the ring path, C and t are launch constants and the words live in an
        engine-owned device buffer (a captured graph serves new batches); it composes with the five constraints and with
        length_penalty.  The decode ends with cvc_beam_rank_force (self.order, self.norm, self.hyp_len, self.final_nmet
        [B, beam] int32) and cvc_beam_backtrack_from(order[:, 0]), both inside a captured graph: run() returns the best-normed
        hypothesis among those that met the most forced words, hypotheses(ranked=True) returns (seq, score, norm, nmet) in that
        order, and self.nmet [T, rows] int32 holds the count of every row entering step t.  Needs beam_history=True, beam > 1 and
        beam % (force_n + 1) == 0; refused with beam_groups > 1.
        tail: plain greedy decode on the packed embedding-gate schedule (beam = 1, <= 64 rows, fp32 weights, no sampling / forced /
        constrained mode, no gsk / gate_ksplit / lang_ksx, split-product arithmetic) -- "fused": the vocabulary head posts every
        block's best candidate as a 64-bit key (an integer max over the workgroups: csrc/sel_keys.h), the next step's attention cell
        decodes its word from the keys, and one launch after the loop writes words and log-probs: six launches per step instead of
        seven.  "launch": cvc_top2_final after every head, as every other mode runs.  None = TAIL_DEFAULT where the fused tail
        applies, "launch" elsewhere; an explicit "fused" where it does not apply is refused.
        mix: scheduled sampling -- a sampling engine (temperature, seed, sample_n) that also holds given words
        (load_captions(); self.given_words [T, rows]) and a probability in device memory (set_mix_prob(); self.mix_prob, one float,
        0 until set).  Step t's word_select is cvc_mixed_select_parts: it draws the sampler's word, flips a per-row coin and writes
        the drawn word (probability p) or the given word of that position as words[t + 1], the next step's input; the probability is
        read by the kernel, so a captured graph serves a changing one.  The sampling paths' launch lists (packed, tile, ring), no C
        driver, capture() works.  run() returns (inputs_next [rows, T] = the words that were fed on, att2_weights, logprob of the
        DRAWN words); self.drawn [T, rows] int64, self.took [T, rows] uint8 and self.given_logprob [T, rows] (the given word's
        log-prob, the forced block's bits) stay on the engine.  Refused: no temperature, beam > 1, forced_n, any constraint, top_k /
        top_p, weights_dtype="bf16".
        stochastic, stochastic_tau: stochastic beam search ("Stochastic beam search"; Kool, van Hoof and Welling
        2019; the rule is the comment of cvc_beam_select_stoch_parts in include/cvc_hip_blocks.h) -- a history beam whose ranking
        key is a Gumbel-perturbed sampling log-prob conditioned on the parent's key: a clip's `beam` slots are a sample WITHOUT
        replacement from q_tau = the sampling engine's distribution at temperature stochastic_tau (UNK and the ban set left out,
        renormalised per step), in draw order, pairwise distinct; slot 0 is an ordinary sample.  The word_select launch is
        cvc_beam_select_stoch_parts on the tile path (fused slabs or finished logits) and on the ring path; tau and t are launch
        constants and the noise comes from the engine's generator state (seed(); every decode and every replay of a captured graph
        first advances `call`), so capture() works and a replay draws afresh.  The engine owns self.logq / self.G [2, rows]
        (ping-pong like score); run() returns slot 0 (the beam engine's tuple, scores = sums of the model's log-probs in slot
        order), hypotheses() returns (seq, score, G, logq) in draw order, consensus() works as for any history beam (fillers are
        not live), and it composes with the five constraints.  Needs beam > 1 and beam_history=True; refused with beam_groups > 1,
        diversity, length_penalty, force_n, a temperature (stochastic_tau is its own) and gsk / gate_ksplit / lang_ksx.
        An engine built by DecodeEngine._member (cvc/decode/ensemble.py; internal) is a member of an EnsembleEngine: self._ensemble is True
        on the primary member and the primary engine on a secondary one, which reads words and parents from that primary's buffers.  A
        member runs every launch of its step but the selection: with beam = 1 its lists take the `given` form (finished logits or
        K-slice slabs, the next word read from words[t + 1]), its word_select entries are placeholders (fn = None, args = the logit
        source (parts, nparts, part_stride, bias)) that the ensemble replaces by one combine launch and one selection, no C-driver plan
        is bound and the fused tail is off; only the primary advances the generator.  Every other engine: _ensemble is None, nothing
        changes."""
        # every check that needs neither the batch nor the library, before a feature is read (cvc/decode/mode.py)
        m = self.mode = DecodeMode.resolve(
            T, getattr(weights, "V", None), beam=beam, path=path, gate_ksplit=gate_ksplit, gsk=gsk, embgate=embgate, lang_ksx=lang_ksx,
            sample_n=sample_n, temperature=temperature, weights_dtype=weights_dtype, top_k=top_k, top_p=top_p, forced_n=forced_n,
            no_repeat_ngram=no_repeat_ngram, no_immediate_repeat=no_immediate_repeat, min_len=min_len, ban_words=ban_words,
            bad_endings=bad_endings, beam_groups=beam_groups, diversity=diversity, length_penalty=length_penalty, force_n=force_n,
            mix=mix, stochastic=stochastic, stochastic_tau=stochastic_tau, beam_history=beam_history)
        for name in DecodeMode.ENGINE_FIELDS:            # the engine, its path mixins and the tests read them as self.<name>
            if getattr(m, name) is not None:             # (inv_tau / stoch_inv_tau exist only in the modes that read them)
                setattr(self, name, getattr(m, name))
        gsk, gate_ksplit, lang_ksx = m.gsk, m.gate_ksplit, m.lang_ksx     # the schedule requests as the mode leaves them
        _ensemble = self._ensemble                       # (set by _member before this runs; None on every other engine)
        if _ensemble is not None and self.beam == 1:
            self.given = True                            # a member's step ends with its logits; the word comes from words[t + 1]
        shared = _ensemble if isinstance(_ensemble, DecodeEngine) else None      # a secondary member: the primary's words / parents
        W = self.W = weights
        self.unk = int(unk_idx)
        fc, conv, pconv = feats["fc_feats"], feats["conv_feats"], feats["p_conv_feats"]
        pool, ppool = feats["pool_feats"], feats["p_pool_feats"]
        mask = feats["pnt_mask"][:, 1:] if feats["pnt_mask"].shape[1] == pool.shape[1] + 1 else feats["pnt_mask"]
        self.B, self.N, self.F = pool.shape[0], pool.shape[1], conv.shape[1]
        B, N, Fr, R, A, V = self.B, self.N, self.F, W.R, W.A, W.V
        dev = pool.device
        # the packed path: one query per clip, at most 64 rows, widths the fragment layouts take
        packed = self.nq == 1 and B * self.nq <= 64 and path != "tile" and R % 32 == 0 and W.E % 32 == 0 and A % 32 == 0
        if (self.forced or self.constrained) and packed and embgate is not None and not embgate:   # (before anything is copied or allocated)
            raise RuntimeError(f"DecodeEngine: {'the forced mode' if self.forced else 'constrained decoding'} on the packed path needs "
                               "the embedding-gate schedule (the attention cell reads the word from words[t])")
        if self.bf16w and (B * self.nq > 64 or R % 32 or W.E % 32 or A % 32):          # (before anything is copied or allocated)
            raise RuntimeError(f'DecodeEngine: weights_dtype="bf16" covers the packed path only: at most 64 rows and R, E, A '
                               f"multiples of 32 (got {B * self.nq} rows, R = {R}, E = {W.E}, A = {A})")
        for name, t, shape in (("fc_feats", fc, (B, R)), ("conv_feats", conv, (B, Fr, R)), ("p_conv_feats", pconv, (B, Fr, A)),
                               ("pool_feats", pool, (B, N, R)), ("p_pool_feats", ppool, (B, N, A))):
            if tuple(t.shape) != shape:
                raise RuntimeError(f"DecodeEngine: {name} has shape {tuple(t.shape)}, expected {shape}")
            hip._dev(t, name=name)
        self.mask = hip._mask(mask)
        if own_features:
            fc, conv, pconv, pool, ppool = (t.clone() for t in (fc, conv, pconv, pool, ppool))
            self.mask = self.mask.clone()
        self.own_features = own_features
        self.feats = (fc, conv, pconv, pool, ppool)
        rows = self.rows = B * self.nq
        # ---- the schedules: what depends on the batch and on the library (the order decides which refusal fires)
        self.packed = packed
        # packed path: K-split gate GEMMs (activations shared through LDS, csrc/gemm_packed_ks.hip) where the shape allows
        # (True: partial tiles + a finishing launch; "fused": the last-arriving K slice of a tile finishes it in the same launch)
        self.gate_ksplit = GATE_KSPLIT_DEFAULT if gate_ksplit is None else gate_ksplit
        self.gate_fused = self.gate_ksplit == "fused"
        self.gate_ksplit = bool(self.gate_ksplit)
        gsk_ok = self.packed and R % 64 == 0 and not self.gate_ksplit and hip.gemm_packed_split(-1) == 2
        if gsk and not gsk_ok:
            raise RuntimeError("DecodeEngine: the stream-K schedule needs the packed path, R % 64 == 0 and cvc_gemm_packed_split(2)")
        self.gsk = False if gsk is None else bool(gsk)
        # more than 64 live rows (beam search, big greedy batches): bf16-fragment tile GEMMs (csrc/gemm_tile.hip)
        self.tile = (not self.packed) and (self.nq > 1 or rows > 64 or path == "tile") and R % 16 == 0 and W.E % 16 == 0 and path != "ring"
        eg_ok = (self.packed and not self.gsk and not self.gate_ksplit) or self.tile
        if embgate and not eg_ok:
            raise RuntimeError("DecodeEngine: the embedding-gate schedule needs the packed path (without gsk / gate_ksplit) or the tile path")
        self.embgate = (eg_ok and 4 * V * 4 * R <= EMBGATE_MAX_BYTES) if embgate is None else bool(embgate)
        if self.given and self.packed and not self.embgate:
            raise RuntimeError(f"DecodeEngine: {'sampling' if self.sampling else 'the forced mode' if self.forced else 'constrained decoding'} on the packed path needs the "
                               "embedding-gate schedule (the attention cell reads the word from words[t])")
        if self.bf16w and not (self.packed and self.embgate):
            raise RuntimeError('DecodeEngine: weights_dtype="bf16" needs the embedding-gate schedule, and its table '
                               f"({4 * V * 4 * R} bytes) is over EMBGATE_MAX_BYTES")
        exp = hip.experimental_built()          # gsk / gate_ksplit / lang_ksx: forms of include/cvc_hip_experimental.h
        if not exp and (self.gsk or self.gate_ksplit or lang_ksx):
            raise RuntimeError("DecodeEngine: gsk / gate_ksplit / lang_ksx are experimental schedules (include/cvc_hip_experimental.h): "
                               "this libcvc_hip.so was built without CVC_EXPERIMENTAL=1")
        ksx_ok = (exp and self.packed and not self.gsk and not self.gate_ksplit and R == 2048 and self.T > 1 and
                  hip.gemm_packed_split(-1) == 2 and int(hip.lib().cvc_packed_lstm_ks_slices(3 * R, R)) == 8)
        if lang_ksx and not ksx_ok:
            raise RuntimeError("DecodeEngine: lang_ksx needs the packed path at R = 2048, T > 1, split-product arithmetic")
        self.lang_ksx = ksx_ok and not self.bf16w and (LANG_KSX_DEFAULT if lang_ksx is None else bool(lang_ksx))
        fused_ok = (self.packed and self.embgate and not self.given and not self.bf16w and not self.gsk and not self.gate_ksplit and
                    not self.lang_ksx and self.beam == 1 and self.unk >= 0 and hip.gemm_packed_split(-1) == 2)
        if tail is None:
            tail = TAIL_DEFAULT if fused_ok else "launch"
        if tail not in TAILS:
            raise RuntimeError(f"DecodeEngine: tail must be one of {TAILS} (or None), got {tail!r}")
        if tail == "fused" and not fused_ok:
            raise RuntimeError('DecodeEngine: tail="fused" covers plain greedy decode on the packed embedding-gate schedule only (beam = 1, '
                               "<= 64 rows, fp32 weights, no sampling / forced / constrained mode, no gsk / gate_ksplit / lang_ksx, "
                               "cvc_gemm_packed_split(2))")
        self.tail = tail
        self.fused_tail = tail == "fused"
        # ---- state and buffers
        nb = lambda t: t.numel() * t.element_size()
        f32 = dict(device=dev, dtype=torch.float32)
        z = lambda *s: torch.zeros(*s, **f32)
        # ping-pong recurrent state: index t & 1 is read, (t+1) & 1 is written
        self.h_att, self.c_att = [z(rows, R), z(rows, R)], [z(rows, R), z(rows, R)]
        self.h_lang, self.c_lang = [z(rows, R), z(rows, R)], [z(rows, R), z(rows, R)]
        self.q = z(rows, A)
        self.scores_r, self.scores_f = z(rows, N), z(rows, Fr)
        self.attn_f = z(rows, Fr)
        self.ctx_sum = z(rows, R)
        self.logits = z(rows, V)
        self.gate_fc = z(rows, 4 * R)      # step-invariant part of the att-LSTM gates: fc x W_ih[:, R:2R] + b_ih + b_hh
        self.QSPLIT = 8                    # h2attn runs split-K over the chip; attn_scores sums the slices
        self.q_parts = z(self.QSPLIT, rows, A)
        self.emb = z(rows, W.E)            # relu(Emb[word_t]), written by the word-selection kernel of step t-1
        self.top2_part = z((V + 31) // 32, 64, 6)
        self.att_steps = z(self.T, rows, N)                       # post-softmax region attention per step
        self.words = torch.zeros(self.T + 1, rows, dtype=torch.int64, device=dev) if shared is None else shared.words   # words[0] = BOS = 0
        self.logprob = z(self.T, rows)
        # fc is per clip; beams of a clip read the same row through a row-gather index
        self.fc = fc
        self.clip_of_row = torch.arange(rows, device=dev, dtype=torch.int64) // self.nq
        if self.sampling or self.stoch:
            self.rng = torch.zeros(4, device=dev, dtype=torch.int32)          # {seed_lo, seed_hi, call, 0} (uint32 bit patterns)
            self.seed(0 if seed is None else seed)
        if self.mix:
            self.given_words = torch.zeros(self.T, rows, dtype=torch.int64, device=dev)   # the given word of every position (load_captions)
            self.mix_prob = z(1)                                                          # P(the drawn word is fed on); set_mix_prob
            self.drawn = torch.zeros(self.T, rows, dtype=torch.int64, device=dev)
            self.took = torch.zeros(self.T, rows, dtype=torch.uint8, device=dev)
            self.given_logprob = z(self.T, rows)
        if self.forced:
            self.rank = torch.zeros(self.T, rows, dtype=torch.int32, device=dev)      # rank of the given word among the row's logits
            self.fmask = self.fm_steps = None                                          # bound by load_captions(frame_mask=...)
        if self.trunc:
            self.cutoff = z(self.T, rows)                                     # min over the kept set of z, per step and row
            self.kept = torch.zeros(self.T, rows, dtype=torch.int32, device=dev)
        if self.constrained:
            n_, imm_, len_, ban_, bad_ = self.cons
            i32 = lambda ids: torch.tensor(list(ids) or [0], dtype=torch.int32, device=dev)
            self.nbanned = torch.zeros(self.T, rows, dtype=torch.int32, device=dev)   # |Ban| per step and row, UNK included
            self.ban_ids, self.bad_ids = i32(ban_), i32(bad_)
            self._cons_desc = hip.Constraint(n_, int(imm_), len_, len(ban_), self.ban_ids.data_ptr(), self.bad_ids.data_ptr(), len(bad_))
        if self.beam > 1:
            self.score = z(2, rows)
            self.done = torch.zeros(2, rows, dtype=torch.uint8, device=dev)
            self.parent = torch.zeros(self.T, rows, dtype=torch.int64, device=dev) if shared is None else shared.parent
            self.bt_seq = torch.zeros(self.B, self.T, dtype=torch.int64, device=dev)      # the returned hypothesis (cvc_beam_backtrack: rank 0; ranked engines: the best by norm)
            self.bt_att = z(self.B, self.T, N)
            self.gather_tmp = [z(rows, R) for _ in range(4)]
            self.beam_ws = z((26 if self.stoch else 21 if self.forcing else 17) * rows)
            if self.stoch:                   # sampling log-prob and perturbed key of every slot, ping-pong like score
                self.logq, self.G = z(2, rows), z(2, rows)
            if self.beam_hist:               # the hypotheses' own histories, ping-pong: step t reads [t & 1], writes [(t + 1) & 1]
                self.bhist = torch.zeros(2, self.T, rows, dtype=torch.int64, device=dev)
            if self.ranked:                  # the final ranking (cvc_beam_rank): slots by norm, norm, len
                self.order = torch.zeros(self.B, self.beam, dtype=torch.int64, device=dev)
                self.norm = z(self.B, self.beam)
                self.hyp_len = torch.zeros(self.B, self.beam, dtype=torch.int32, device=dev)
            if self.forcing:                 # the forced words (load_force_words), n(r) of the rows entering each step, n of the final slots
                self.force_words = torch.full((self.B, self.force_n), -1, dtype=torch.int32, device=dev)
                self.nmet = torch.zeros(self.T, rows, dtype=torch.int32, device=dev)
                self.final_nmet = torch.zeros(self.B, self.beam, dtype=torch.int32, device=dev)
        self.inv_temp = float(inv_temp)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self._keep: List = []
        # what stays in the Infinity Cache between steps: small linear weights, then (embedding-gate schedule on the packed path) the
        # attention cell's gate matrix over K = 2R if it fits, then the largest subset of the feature tensors
        bpw = 2 if self.bf16w else 4                       # bytes per stored weight
        keep = cache_plan(bpw * (V * R + A * R), {"ppool": nb(ppool), "pconv": nb(pconv), "pool": nb(pool), "conv": nb(conv)},
                          gate_weight_bytes=bpw * 4 * R * 2 * R if (self.packed and self.embgate and (rows > 32 or self.bf16w)) else None,
                          lang_weight_bytes=bpw * 4 * R * 3 * R if self.bf16w else None)
        self.cache_keep = keep
        self.att_w_cached = bool(keep.get("att_w", False))
        self.lang_w_cached = bool(keep.get("lang_w", False))
        # cvc_attn_set.stream: bit 0 = proj read non-temporally, bit 1 = ctx
        self.stream_r = (0 if keep["ppool"] else 1) | (0 if keep["pool"] else 2)
        self.stream_f = (0 if keep["pconv"] else 1) | (0 if keep["conv"] else 2)
        self._plan = None
        self._driver = driver
        self._ksx_checked = False
        if self.lang_ksx:
            self.ksx_slab = torch.empty(8 * (R // 8) * 2048, device=dev, dtype=torch.float32)
            self.ksx_flags = torch.zeros(R // 8 + 1, device=dev, dtype=torch.int32)
        if self.packed:
            self._alloc_packed()
        elif self.tile:
            self._alloc_tile()
        if self.fused_tail:
            # [T][4][64] candidate keys, then [T][64] UNK keys (64-bit words; cleared at the start of every decode), and the
            # per-step (max, sum-exp) records of the head's blocks
            self.tail_keys = torch.zeros(self.T * 64 * 5, dtype=torch.int64, device=dev)
            self.tail_ms = z(self.T, (V + 31) // 32, 64, 2)
        self._launches = self._build_launches()
        if driver and _ensemble is None and not self.given and not self.bf16w and not self.beam_hist and (self.tile or (self.packed and not (self.ks_att or self.ks_lang))):
            self._bind_driver()

    # ------------------------------------------------------------------ C-ABI decode driver (csrc/decode_driver.hip)

    def _bind_driver(self):
        """Bind every buffer of this engine into a cvc_decode_desc and create the plan: run() / capture() then enqueue the
        whole decode with ONE call (cvc_decode_greedy / cvc_decode_beam) instead of walking the launch list in Python.  The
        Python launch list stays for run_timed() (per-launch HIP events) and as the reference the driver is tested against."""
        W, L = self.W, hip.lib()
        ptr = lambda t: None if t is None else t.data_ptr()
        d = hip.DecodeDesc()
        d.B, d.beam, d.T, d.N, d.F, d.R, d.A, d.E, d.V = self.B, self.beam, self.T, self.N, self.F, W.R, W.A, W.E, W.V
        d.unk_idx, d.attn_kind, d.inv_temp = self.unk, W.kind, self.inv_temp
        d.stream_r, d.stream_f = self.stream_r, self.stream_f
        for k in ("b_ih_att", "b_hh_att", "b_ih_lang", "b_hh_lang", "b_h", "w_a", "b_a", "b_o", "embed"):
            setattr(d, k, ptr(getattr(W, k)))
        fc, conv, pconv, pool, ppool = self.feats
        d.fc, d.conv, d.pconv, d.pool, d.ppool, d.mask = ptr(fc), ptr(conv), ptr(pconv), ptr(pool), ptr(ppool), ptr(self.mask)
        d.words, d.att_steps, d.logprob = ptr(self.words), ptr(self.att_steps), ptr(self.logprob)
        d.scores_r, d.scores_f, d.attn_f = ptr(self.scores_r), ptr(self.scores_f), ptr(self.attn_f)
        if self.packed:
            R = W.R
            d.path, d.qsplit = 0, self.QSPLIT
            d.w_att, d.w_lang, d.w_h, d.w_o = ptr(W.p_att2 if self.embgate else W.p_att), ptr(W.p_lang), ptr(W.p_h), ptr(W.p_o)
            w_fc = W.w_ih_att[:, R:2 * R]
            d.w_fc, d.ld_w_fc = w_fc.data_ptr(), w_fc.stride(0)
            d.gate_fc, d.q_parts, d.top2_part = ptr(self.gate_fc), ptr(self.q_parts), ptr(self.top2_part)
            for name, bufs in (("xa", self.XA), ("xl", self.XL), ("ca", self.cA), ("cl", self.cL)):
                arr = getattr(d, name)
                arr[0], arr[1] = ptr(bufs[0]), ptr(bufs[1])
            d.xa0_init = ptr(self.XA0_init)
            if self.embgate:
                d.w_att = ptr(W.p_att2)
                d.emb_gate, d.sel_counter = ptr(W.t_embgate), ptr(self.sel_counter)
                d.att_w_cached = int(self.att_w_cached)
            if self.lang_ksx:
                d.lang_ksx, d.ksx_slab, d.ksx_flags = 1, ptr(self.ksx_slab), ptr(self.ksx_flags)
            if self.fused_tail:
                d.tail, d.tail_keys, d.tail_ms = 1, ptr(self.tail_keys), ptr(self.tail_ms)
            if self.gsk:
                d.gsk_nwg = self.gsk_nwg
                d.slab_att, d.slab_lang, d.slab_q, d.slab_o = (ptr(self.slab_att), ptr(self.slab_lang), ptr(self.slab_q),
                                                              ptr(self.slab_o))
        else:
            d.path = 1
            d.ks_gate, d.ks_q, d.ks_o, d.ks_fc = self.ks_gate, self.ks_q, self.ks_o, self.ks_fc
            d.w_att, d.w_lang, d.w_h, d.w_o, d.w_fc_frag = ptr(W.t_att2 if self.embgate else W.t_att), ptr(W.t_lang), ptr(W.t_h), ptr(W.t_o), ptr(W.t_fc)
            if self.embgate:
                d.emb_gate = ptr(W.t_embgate)
            d.gate_fc, d.q, d.q_parts, d.logits = ptr(self.gate_fc_clip), ptr(self.q), ptr(self.parts_q), ptr(self.logits)
            for name, t in (("xaf", self.XAf), ("xlf", self.XLf), ("xhf", self.XHf), ("xff", self.XFf)):
                p_, s_ = hip._frag_ptr(t)
                setattr(d, name, p_)
                setattr(d, name + "_stride", s_)
            d.parts_gate, d.parts_o, d.parts_fc = ptr(self.parts_gate), ptr(self.parts_o), ptr(self.parts_fc)
            d.h_att, d.c_att, d.h_lang, d.c_lang = ptr(self.t_h_att), ptr(self.t_c_att), ptr(self.t_h_lang), ptr(self.t_c_lang)
            d.c_att_prev, d.c_lang_prev, d.zero_state = ptr(self.t_c_att_prev), ptr(self.t_c_lang_prev), ptr(self.t_zero)
            if self.beam > 1:
                d.score, d.done, d.parent, d.beam_ws = ptr(self.score), ptr(self.done), ptr(self.parent), ptr(self.beam_ws)
        plan = C.c_void_p()
        hip._check(L.cvc_decode_plan_create(C.byref(d), C.byref(plan)), "cvc_decode_plan_create")
        self._desc, self._plan = d, plan
        self._plan_call = L.cvc_decode_beam if self.beam > 1 else L.cvc_decode_greedy

    def __del__(self):
        plan = getattr(self, "_plan", None)
        if plan is not None and plan.value:
            try:
                hip.lib().cvc_decode_plan_destroy(plan)
            except Exception:
                pass
            self._plan = None

    def _run_driver(self):
        hip._check(self._plan_call(self._plan, torch.cuda.current_stream().cuda_stream), "cvc_decode_greedy/beam")

    # ------------------------------------------------------------------ packed path (greedy, rows <= 64)

    def _reset(self):
        if self.packed:
            self.XA[0].copy_(self.XA0_init)
            self.XL[0].zero_()
            self.cA[0].zero_()
            self.cL[0].zero_()
            self.words[0].zero_()
            if self.fused_tail:
                self.tail_keys.zero_()
            return
        if not self.tile:                    # (the tile path's first launch packs its state from t_zero)
            for bufs in (self.h_att, self.c_att, self.h_lang, self.c_lang):
                bufs[0].zero_()
        self.words[0].zero_()
        if self.beam > 1:
            self.score.zero_()
            self.done.zero_()
            if self.stoch:
                self.logq.zero_()
                self.G.zero_()

    def _run_launches(self, timers=None):
        """timers: optional dict name -> list of (start_event, end_event), filled per launch
        (HIP events on the launch stream; used by bench.py for per-kernel durations)."""
        stream = torch.cuda.current_stream().cuda_stream
        for name, fn, args in self._python_launches():
            if timers is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            if fn == "copy":
                args[0].copy_(args[1])
            else:
                rc = fn(*args, stream)
                if rc != 0:
                    hip._check(rc, name)
            if timers is not None:
                e1.record()
                timers.setdefault(name, []).append((e0, e1))

    def load_features(self, feats: Dict[str, torch.Tensor]):
        """Next batch of the same shape into the engine's own feature buffers (own_features=True): ~0.2 ms of device
        copies at cfg2 instead of a new binding and a new graph capture (~6 ms)."""
        if not self.own_features:
            raise RuntimeError("DecodeEngine.load_features needs own_features=True")
        pool = feats["pool_feats"]
        mask = feats["pnt_mask"][:, 1:] if feats["pnt_mask"].shape[1] == pool.shape[1] + 1 else feats["pnt_mask"]
        for dst, src in zip(self.feats, (feats["fc_feats"], feats["conv_feats"], feats["p_conv_feats"], pool, feats["p_pool_feats"])):
            if dst.shape != src.shape:
                raise RuntimeError(f"DecodeEngine.load_features: shape {tuple(src.shape)} != bound {tuple(dst.shape)}")
            dst.copy_(src)
        self.mask.copy_(hip._mask(mask))
        return self

    def load_captions(self, words: torch.Tensor, frame_mask: Optional[torch.Tensor] = None):
        """Forced mode: the captions to follow, words [B * n, T] int64 (row b * n + j = caption j of clip b), copied into the
        engine-owned words[1:] (words[0] stays BOS) -- a stream-ordered copy, so a captured graph is reused across batches as
        load_features() does it.  frame_mask [T, B * n, N] (uint8 / bool, non-zero = the proposal lies outside the word's frames):
        copied into the engine-owned mask; from the first such call on the region attention of step t also writes fm_steps[t], its
        pre-softmax scores with the fill value at the masked proposals.  The mask changes the launch list, so it has to be bound
        before capture(); None on an engine that has one clears it (fm_steps = the unmasked scores)."""
        if not self.forced and not self.mix:
            raise RuntimeError("DecodeEngine.load_captions: this engine is not in the forced mode (forced_n = 0)")
        if tuple(words.shape) != (self.rows, self.T) or words.dtype != torch.int64:
            raise RuntimeError(f"DecodeEngine.load_captions: words must be int64 [{self.rows}, {self.T}], got {words.dtype} "
                               f"{tuple(words.shape)}")
        if self.mix:                     # the mixed mode: the given word of every position, the same stream-ordered copy
            if frame_mask is not None:
                raise RuntimeError("DecodeEngine.load_captions: the mixed mode takes no frame mask")
            self.given_words.copy_(words.t())
            return self
        if frame_mask is not None:
            if tuple(frame_mask.shape) != (self.T, self.rows, self.N):
                raise RuntimeError(f"DecodeEngine.load_captions: frame_mask has shape {tuple(frame_mask.shape)}, expected "
                                   f"{(self.T, self.rows, self.N)}")
            if self.fmask is None:
                if self.graph is not None:
                    raise RuntimeError("DecodeEngine.load_captions: the captured graph has no frame-masked output; bind the first "
                                       "frame mask before capture()")
                dev = self.words.device
                self.fmask = torch.zeros(self.T, self.rows, self.N, dtype=torch.uint8, device=dev)
                self.fm_steps = torch.zeros(self.T, self.rows, self.N, dtype=torch.float32, device=dev)
                self._launches = None                   # rebuilt on demand with the mask in the region set
            self.fmask.copy_(hip._mask(frame_mask))
        elif self.fmask is not None:
            self.fmask.zero_()
        self.words[1:].copy_(words.t())
        return self

    def weights_refreshed(self):
        """After DecodeWeights.refresh(): the one engine-owned operand that was computed from a weight when the engine was bound --
        the embedded BOS word in the packed path's initial activations without the embedding-gate schedule -- is recomputed in
        place.  Everything else the launch list reads is the weights object's own storage."""
        if self.packed and not self.embgate:
            W = self.W
            bos = torch.relu(W.embed[0]).view(1, W.E).expand(self.rows, W.E).contiguous()
            self.XA0_init[W.R // 4:(W.R + W.E) // 4] = to_quad(bos)
        return self

    def set_mix_prob(self, p: float):
        """Mixed mode: the probability that a step feeds its DRAWN word on (0 = teacher forcing, 1 = the sampling engine), filled
        into the engine-owned device float (stream-ordered: a captured graph reads the new value at its next replay)."""
        if not self.mix:
            raise RuntimeError("DecodeEngine.set_mix_prob: this engine is not in the mixed mode (mix=False)")
        p = float(p)
        if not (0.0 <= p <= 1.0):
            raise RuntimeError(f"DecodeEngine.set_mix_prob: the probability must lie in [0, 1], got {p!r}")
        self.mix_prob.fill_(p)
        return self

    def load_force_words(self, words):
        """Lexically constrained beam search (force_n = C >= 1): the words the captions should contain, [B, C] integers, -1 (or any
        inactive entry: 0, UNK, a duplicate) = unused.  Copied into the engine-owned self.force_words (int32) -- a stream-ordered
        copy, so a captured graph serves new batches as load_features() does it.  Refused: another shape, an id >= V, a word that
        ban_words forbids."""
        if not self.forcing:
            raise RuntimeError("DecodeEngine.load_force_words: this engine forces no words (force_n = 0)")
        w = torch.as_tensor(np.asarray(words.cpu()) if isinstance(words, torch.Tensor) else np.asarray(words))
        if tuple(w.shape) != (self.B, self.force_n) or w.dtype.is_floating_point or w.dtype == torch.bool:
            raise RuntimeError(f"DecodeEngine.load_force_words: words must be integers [{self.B}, {self.force_n}], got {w.dtype} "
                               f"{tuple(w.shape)}")
        big = sorted({int(v) for v in w.reshape(-1).tolist() if v >= self.W.V})
        if big:
            raise RuntimeError(f"DecodeEngine.load_force_words: ids outside [0, V = {self.W.V}): {big}")
        both = sorted({int(v) for v in w.reshape(-1).tolist()} & set(self.cons[3]))
        if both:
            raise RuntimeError(f"DecodeEngine.load_force_words: words that ban_words forbids cannot be forced: {both}")
        self.force_words.copy_(w.to(torch.int32))
        return self

    def _region_set(self, t):
        """The region feature set of step t's attention passes; the forced mode with a frame mask bound adds the mask and the
        frame-masked output of that step."""
        fc, conv, pconv, pool, ppool = self.feats
        ptr = lambda x: None if x is None else x.data_ptr()
        fm_in = fm_out = None
        if self.forced and self.fmask is not None:
            fm_in, fm_out = ptr(self.fmask[t]), ptr(self.fm_steps[t])
        return hip.AttnSet(ptr(ppool), ptr(pool), ptr(self.mask), fm_in, ptr(self.scores_r), fm_out, ptr(self.att_steps[t]), None,
                           self.N, self.stream_r)

    def bind_features(self, feats: Dict[str, torch.Tensor]):
        """Next batch of the same shape WITHOUT copying it: the C-ABI plan (and this engine) is pointed at the caller's
        feature tensors.  Only for engines that run through the driver without a captured graph (a graph keeps the pointers it
        was captured with: use load_features there)."""
        if self._plan is None or self.graph is not None:
            raise RuntimeError("DecodeEngine.bind_features needs a driver-bound engine without a captured graph")
        pool = feats["pool_feats"]
        mask = feats["pnt_mask"][:, 1:] if feats["pnt_mask"].shape[1] == pool.shape[1] + 1 else feats["pnt_mask"]
        new = (feats["fc_feats"], feats["conv_feats"], feats["p_conv_feats"], pool, feats["p_pool_feats"])
        for dst, src, name in zip(self.feats, new, ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats")):
            if dst.shape != src.shape:
                raise RuntimeError(f"DecodeEngine.bind_features: shape {tuple(src.shape)} != bound {tuple(dst.shape)}")
            hip._dev(src, name=name)
        self.mask = hip._mask(mask)
        self.feats = new
        self.fc = new[0]
        hip._check(hip.lib().cvc_decode_plan_set_features(self._plan, *(t.data_ptr() for t in new), self.mask.data_ptr()),
                   "cvc_decode_plan_set_features")
        self._launches = None                       # the Python launch list holds the old pointers: rebuilt on demand
        return self

    def _build_launches(self):
        out = self._build_packed() if self.packed else (self._build_tile() if self.tile else self._build())
        if (self.sampling or self.stoch) and not isinstance(self._ensemble, DecodeEngine):
            # first entry: a fresh `call` for every decode (and every replay of a captured graph); an ensemble: the primary's only
            out.insert(0, ("sample_advance", hip.lib().cvc_sample_advance, (self.rng.data_ptr(),)))
        return out

    def _word_select_sampled(self, t, parts, nparts, part_stride, bias, real=False):
        """The sampling paths' word_select launch of step t over logits parts[0] + ... (+ bias): the plain block, or the
        truncating one (top_k / top_p are launch constants: they live in the captured graph); the forced mode: the block that
        scores the given word words[t + 1] and writes none.  An ensemble's member: the placeholder that names the logit source
        (real=True: the block itself, what the ensemble asks its primary for over the combined rows)."""
        if self._ensemble is not None and not real:
            return ("word_select", None, (parts, nparts, part_stride, bias))
        L, rows, V = hip.lib(), self.rows, self.W.V
        if self.forced:
            return ("word_select", L.cvc_forced_select_parts, (parts, nparts, part_stride, bias, rows, V, self.words[t + 1].data_ptr(), 1,
                                                               self.logprob[t].data_ptr(), self.rank[t].data_ptr()))
        head = (parts, nparts, part_stride, bias, rows, V, self.unk, self.inv_tau)
        if self.constrained:           # the history is words[1 .. t]: row r of step s at words[1] + s * rows + r
            opt = lambda buf: buf[t].data_ptr() if self.trunc else None
            return ("word_select", L.cvc_constrained_select_parts, head + (
                self.top_k, self.top_p, self.rng.data_ptr() if self.sampling else None, t, self.words[t + 1].data_ptr(), 1,
                self.logprob[t].data_ptr(), opt(getattr(self, "cutoff", None)), opt(getattr(self, "kept", None)),
                self.words[1].data_ptr(), rows, self._cons_desc, self.nbanned[t].data_ptr()))
        tail = (self.rng.data_ptr(), t, self.words[t + 1].data_ptr(), 1, self.logprob[t].data_ptr())
        if self.mix:
            return ("word_select", L.cvc_mixed_select_parts, head + tail + (
                self.given_words[t].data_ptr(), 1, self.mix_prob.data_ptr(), self.drawn[t].data_ptr(), self.took[t].data_ptr(),
                self.given_logprob[t].data_ptr()))
        if not self.trunc:
            return ("word_select", L.cvc_sample_select_parts, head + tail)
        return ("word_select", L.cvc_sample_select_trunc_parts, head + (self.top_k, self.top_p) + tail +
                (self.cutoff[t].data_ptr(), self.kept[t].data_ptr()))

    def _word_select_beam(self, t, parts, nparts, part_stride, bias, real=False):
        """A beam path's word_select launch of step t over logits parts[0] + ... (+ bias): the plain block, or with beam_history
        the block that carries the hypotheses' histories (and applies the constraints to them; t and the rules are launch
        constants).  An ensemble's member: the placeholder, as in _word_select_sampled."""
        if self._ensemble is not None and not real:
            return ("word_select", None, (parts, nparts, part_stride, bias))
        L, B, beam, V = hip.lib(), self.B, self.beam, self.W.V
        srd, swr = t & 1, (t + 1) & 1
        head = (parts, nparts, part_stride, bias, self.score[srd].data_ptr(), self.done[srd].data_ptr(), B, beam, V, self.unk)
        tail = (self.parent[t].data_ptr(), self.words[t + 1].data_ptr(), self.score[swr].data_ptr(), self.done[swr].data_ptr())
        ws = self.beam_ws.data_ptr()
        if not self.beam_hist:
            return ("word_select", L.cvc_beam_select_parts, head + (1 if t == 0 else 0,) + tail + (ws,))
        cons = (self._cons_desc, self.nbanned[t].data_ptr()) if self.constrained else (None, None)
        hist = (t, self.bhist[srd].data_ptr(), self.bhist[swr].data_ptr(), self.rows, cons[0])
        if self.stoch:
            return ("word_select", L.cvc_beam_select_stoch_parts, head + hist + (
                self.stoch_inv_tau, self.rng.data_ptr(), self.logq[srd].data_ptr(), self.G[srd].data_ptr()) + tail + (
                self.logq[swr].data_ptr(), self.G[swr].data_ptr(), cons[1], ws))
        if self.grouped:
            return ("word_select", L.cvc_beam_select_groups_parts, head + hist + (self.groups, self.diversity) + tail + (cons[1], ws))
        if self.forcing:
            return ("word_select", L.cvc_beam_select_force_parts, head + hist + (self.force_words.data_ptr(), self.force_n) + tail +
                    (cons[1], self.nmet[t].data_ptr(), ws))
        return ("word_select", L.cvc_beam_select_hist_parts, head + hist + tail + (cons[1], ws))

    def hypotheses(self, ranked: bool = False):
        """n-best: all `beam` hypotheses of every clip after run(), in slot order (one group: rank order by score) -- (seq
        [B, beam, T] int64, score [B, beam]), views of engine-owned buffers (beam_history=True: the histories the selection block
        carried, no backtracking); a stochastic beam: (seq, score, G [B, beam], logq [B, beam]) in draw order, G the perturbed keys
        (non-increasing over the slots) and logq the captions' log-probs under q_tau.  ranked=True (beam_groups > 1 or a length_penalty): (seq, score, norm, group [B, beam] int64) in
        the order of cvc_beam_rank -- norm descending, ties to the lowest slot -- as new tensors; with force_n the fourth is nmet
        [B, beam] int32, the forced words each hypothesis met, and the order is cvc_beam_rank_force's."""
        if not self.beam_hist:
            raise RuntimeError("DecodeEngine.hypotheses needs beam_history=True")
        B, beam, T = self.B, self.beam, self.T
        seq, score = self.bhist[T & 1].view(T, B, beam).permute(1, 2, 0), self.score[T & 1].view(B, beam)
        if self.stoch:                      # draw order is slot order; a filler holds -inf in all three
            if ranked:
                raise RuntimeError("DecodeEngine.hypotheses(ranked=True): a stochastic beam's slots are in draw order, there is no ranking")
            return seq, score, self.G[T & 1].view(B, beam), self.logq[T & 1].view(B, beam)
        if not ranked:
            return seq, score
        if not self.ranked:
            raise RuntimeError("DecodeEngine.hypotheses(ranked=True) needs beam_groups > 1, a length_penalty or force_n")
        o = self.order
        return (seq.gather(1, o.unsqueeze(2).expand(B, beam, T)), score.gather(1, o), self.norm.gather(1, o),
                self.final_nmet.gather(1, o) if self.forcing else o // (beam // self.groups))

    def consensus(self, table, utility=None, weights: str = "uniform", alpha: float = 1.0, want_pairs: bool = False):
        """Consensus (minimum-Bayes-risk) selection among the candidates of the last run() ("Consensus
        selection"): per clip the candidate with the highest mean CIDEr-D against the clip's other candidates as stand-in
        references, over `table` (a cvc.cider.CiderD; csrc/consensus.hip).  A sampling engine with sample_n > 1: the n samples of
        a clip.  A beam engine with beam_history=True: its hypotheses(), live where the score is finite.
        utility: None, or a mix {name: weight} over cvc.metrics.REWARD_NAMES -- the pair utility is then the weighted sum of CIDEr-D,
        BLEU-1..4 and ROUGE-L of the candidate against ONE other candidate.  weights: "uniform", or "model" -- every other candidate
        counts as a reference with weight exp(alpha * score), score the model's log-prob of the hypothesis (hypotheses()); a history
        beam only (diverse and forced beams included): the candidates of a sampling engine and of a stochastic beam are draws, their
        uniform mean is the expectation already, and both refuse "model".  alpha: finite, >= 0 (0: uniform again).
        With utility None or CIDEr-D alone at weight 1 AND uniform weights the launch is cvc_consensus_cider, as ever; anything else
        is one launch of cvc_consensus_mix (csrc/consensus_mix.hip; cvc.metrics.consensus), and self.consensus_logw keeps the
        log-weights it used (None: uniform); want_pairs=True forces that launch and keeps its raw pair metrics [B, n, n, 6] in
        self.consensus_pairs.
        -> (seq [B, T], att2_weights [B, T, N], logprob [B, T] or None for a beam, pick [B] int32 -- the index of the kept sample /
        the kept slot --, utility [B * n] fp32), new tensors, everything selected on the device with pick (a beam's attention rows
        by cvc_beam_backtrack_from the picked slot); no host read-back."""
        from .. import metrics
        if weights not in ("uniform", "model"):
            raise RuntimeError(f"DecodeEngine.consensus: weights must be 'uniform' or 'model', got {weights!r}")
        alpha = float(alpha)
        if not (alpha >= 0.0) or alpha == float("inf"):
            raise RuntimeError(f"DecodeEngine.consensus: alpha must be a finite number >= 0, got {alpha!r}")
        if weights == "model" and self.sampling:
            raise RuntimeError("DecodeEngine.consensus: weights='model' on a sampling engine -- its candidates are draws from the model, "
                               "the uniform mean over them is the expectation already; use weights='uniform'")
        if weights == "model" and self.stoch:
            raise RuntimeError("DecodeEngine.consensus: weights='model' on a stochastic beam -- its candidates are draws without "
                               "replacement (importance weights for them are not implemented); use weights='uniform'")
        mix = None if (weights == "uniform" and metrics.is_cider_only(utility) and not want_pairs) else metrics.utility_coefficients(
            utility or {"cider": 1.0}, "DecodeEngine.consensus")
        cand, n, live = self.candidates("consensus")
        self.consensus_live = live          # (the mask this selection used: None = every sample counts; model.last_consensus keeps it)
        self.consensus_logw = self.consensus_pairs = None
        if mix is not None:
            if weights == "model":
                self.consensus_logw = (self.hypotheses()[1].reshape(-1) * alpha).contiguous()
            mix = dict(zip(metrics.REWARD_NAMES, mix))

            def select(cand, n, live=None):
                out = metrics.consensus(cand, n, mix, table, self.consensus_logw, live, want_pairs=want_pairs)
                self.consensus_pairs = out.get("pairs")
                return out["utility"], out["pick"], out["best"]
        else:
            select = table.consensus
        B, T, N = self.B, self.T, self.N
        if self.sampling:
            utility, pick, best = select(cand, n)
            at = torch.arange(B, device=cand.device) * n + pick
            return (best, self.att_steps.permute(1, 0, 2).index_select(0, at), self.logprob.t().index_select(0, at), pick, utility)
        utility, pick, _ = select(cand, n, live=live)
        start = pick.to(torch.int64)
        bt_seq = torch.empty(B, T, dtype=torch.int64, device=start.device)
        bt_att = torch.empty(B, T, N, dtype=torch.float32, device=start.device)
        hip._check(hip.lib().cvc_beam_backtrack_from(self.words[1:].data_ptr(), self.parent.data_ptr(), self.att_steps.data_ptr(), B, n,
                                                     T, N, start.data_ptr(), 1, bt_seq.data_ptr(), bt_att.data_ptr(), hip._stream()),
                   "cvc_beam_backtrack_from")
        return bt_seq, bt_att, None, pick, utility

    def candidates(self, who: str = "candidates"):
        """The candidate set of the last run() as consensus() and set_diversity() take it: (cand [B * n, T] int64, n, live [B * n] bool or
        None).  A sampling engine with sample_n > 1: its rows, all live.  A beam engine with beam_history=True: its hypotheses(), live
        where the score is finite.  Refuses a forced engine, a mix engine, a beam without histories and one candidate per clip."""
        if self.forced:
            raise RuntimeError(f"DecodeEngine.{who}: a forced engine scores given words, it has no candidates to choose among")
        if self.mix:
            raise RuntimeError(f"DecodeEngine.{who}: a mix engine's rows follow given captions (scheduled sampling), they are no "
                               "candidates of one clip")
        if self.beam > 1 and not self.beam_hist:
            raise RuntimeError(f"DecodeEngine.{who}: a beam engine needs beam_history=True (the candidates are hypotheses())")
        if self.nq < 2:
            raise RuntimeError(f"DecodeEngine.{who}: one candidate per clip -- it needs sample_n > 1 or beam > 1")
        if self.sampling:
            return self.words[1:].t().contiguous(), self.nq, None
        seq, score = self.hypotheses()[:2]
        return seq.reshape(self.B * self.nq, self.T), self.nq, torch.isfinite(score).reshape(-1)

    def set_diversity(self):
        """Diversity of every clip's candidate set after run() ("Caption-set diversity"; csrc/diversity.hip):
        cvc.metrics.set_diversity on exactly the candidates and live mask consensus() uses, with the same refusals.  -> dict(stats
        [B, 12] int32, mbleu_stats [B * n, 10] int32, mbleu [B * n, 4], div [B, 2]), new tensors on the device; the engine's state
        and launch lists are not touched, no host read-back.  (Not `diversity`: that attribute is the diverse beam's lambda.)"""
        from .. import metrics
        cand, n, live = self.candidates("set_diversity")
        return metrics.set_diversity(cand, n, live)

    def set_spectrum(self, cider=None):
        """Spectral diversity of every clip's candidate set after run() ("Spectral set diversity";
        csrc/spectrum.hip): cvc.metrics.set_spectrum on exactly the candidates and live mask consensus() and set_diversity() use,
        with the same refusals.  cider: a cvc.cider.CiderD (Self-CIDEr over its table) or None (LSA).  -> dict(lam [B, 32] fp64,
        score [B, 2], info [B, 2] int32), new tensors on the device; the engine's state and launch lists are not touched, no host
        read-back."""
        from .. import metrics
        cand, n, live = self.candidates("set_spectrum")
        return metrics.set_spectrum(cand, n, live, cider=cider)

    def _python_launches(self):
        if self._launches is None:
            self._keep = []
            self._launches = self._build_launches()
        return self._launches

    def run_timed(self):
        """One eager decode with a HIP-event pair around every launch.  Returns name -> list of ms."""
        timers = {}
        self._reset()
        self._run_launches(timers)
        torch.cuda.synchronize()
        return {k: [a.elapsed_time(b) for a, b in v] for k, v in timers.items()}

    def _run_once(self):
        """One decode on the current stream: through the C-ABI driver when bound (it resets its state itself), else the
        Python launch list."""
        if self._plan is not None:
            self._run_driver()
        else:
            self._reset()
            self._run_launches()
        self._finish_beam()

    def _finish_beam(self):
        """What a beam decode enqueues behind its T steps: the returned hypothesis (and, on a ranked engine, the final ranking)."""
        if self.beam > 1 and self.ranked:                  # the final ranking, then the best hypothesis by norm: two launches
            L, T = hip.lib(), self.T
            if self.forcing:
                hip._check(L.cvc_beam_rank_force(self.bhist[T & 1].data_ptr(), self.rows, self.score[T & 1].data_ptr(),
                                                 self.force_words.data_ptr(), self.force_n, self.B, self.beam, T, self.W.V, self.unk,
                                                 self.length_penalty, self.order.data_ptr(), self.norm.data_ptr(),
                                                 self.hyp_len.data_ptr(), self.final_nmet.data_ptr(), hip._stream()), "cvc_beam_rank_force")
            else:
                hip._check(L.cvc_beam_rank(self.bhist[T & 1].data_ptr(), self.rows, self.score[T & 1].data_ptr(), self.B, self.beam, T,
                                           self.length_penalty, self.order.data_ptr(), self.norm.data_ptr(), self.hyp_len.data_ptr(),
                                           hip._stream()), "cvc_beam_rank")
            hip._check(L.cvc_beam_backtrack_from(self.words[1:].data_ptr(), self.parent.data_ptr(), self.att_steps.data_ptr(), self.B,
                                                 self.beam, T, self.N, self.order.data_ptr(), self.beam, self.bt_seq.data_ptr(),
                                                 self.bt_att.data_ptr(), hip._stream()), "cvc_beam_backtrack_from")
        elif self.beam > 1:                                # rank-0 hypothesis: one launch (was ~60 indexing launches per decode)
            hip._check(hip.lib().cvc_beam_backtrack(self.words[1:].data_ptr(), self.parent.data_ptr(), self.att_steps.data_ptr(),
                                                    self.B, self.beam, self.T, self.N, self.bt_seq.data_ptr(),
                                                    self.bt_att.data_ptr(), hip._stream()), "cvc_beam_backtrack")

    def capture(self):
        """Capture the T-step loop into a HIP graph (launch-bound inner loop -> one replay)."""
        if self.lang_ksx and not self._ksx_checked:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._run_once()
            torch.cuda.current_stream().wait_stream(s)
            self.check_ksx()
        key = (self.packed, self.tile, self.fused_tail) + self.mode.flags
        if key not in DecodeEngine._warm:                 # first capture of this path in the process: run once outside capture
            saved = self.rng.clone() if (self.sampling or self.stoch) else None     # (the warm-up decode must not advance the sampling state)
            s = torch.cuda.Stream()                       # (module load, lazy init); later engines skip the extra decode
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._run_once()
            torch.cuda.current_stream().wait_stream(s)
            if saved is not None:
                self.rng.copy_(saved)
            DecodeEngine._warm.add(key)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode=_capture_mode()):
            self._run_once()
        self.graph = g
        return self

    def seed(self, s: int):
        """Sampling: the generator state becomes {seed_lo, seed_hi, 0, 0} of the 64-bit seed s (a stream-ordered copy); the k-th
        decode after it draws its noise with call = k."""
        if not self.sampling and not self.stoch:
            raise RuntimeError("DecodeEngine.seed: this engine does not sample (temperature=None)")
        s = int(s) & 0xFFFFFFFFFFFFFFFF
        words = np.array([s & 0xFFFFFFFF, s >> 32, 0, 0], dtype=np.uint32).view(np.int32)
        self.rng.copy_(torch.from_numpy(words))
        return self

    @property
    def rng_state(self) -> torch.Tensor:
        """The generator words {seed_lo, seed_hi, call, 0} (int32 [4], device memory, the engine's own buffer): after run() `call` is
        the one that decode drew its noise with -- what cvc_scst_weights_wor hashes its per-clip root key from.  Read-only."""
        if not self.sampling and not self.stoch:
            raise RuntimeError("DecodeEngine.rng_state: this engine does not sample (temperature=None)")
        return self.rng

    def run(self):
        """One full T-step decode.  Returns (seq [B,T] int64, att2_weights [B,T,N]) -- views of
        engine-owned buffers (clone to keep across runs).  Sampling: (seq [B*n, T], att2_weights [B*n, T, N],
        logprob [B*n, T]), row b * n + j = sample j of clip b; a constrained engine with beam = 1 returns that tuple with or without a
        temperature (constrained beam search: what a beam engine returns, (seq, att2_weights, final beam scores [B, beam])).  A beam
        engine's seq is the rank-0 hypothesis; with beam_groups > 1 or a length_penalty it is the best hypothesis by norm = score /
        len^alpha (self.order[:, 0]), with its attention rows, and the scores stay in slot order.  Forced mode: (seq = the given words, att2_weights, logprob,
        rank [B*n, T] int32), row b * n + j = caption j of clip b.  Mixed mode: the sampling engine's tuple with seq = the words
        that were fed on (drawn or given) and logprob = the DRAWN words' (self.drawn)."""
        if self.graph is not None:
            self.graph.replay()
        else:
            self._run_once()
            if self.lang_ksx and not self._ksx_checked and self.check_ksx():
                self._run_once()                           # the fallback's results
        return self._result()

    def _result(self):
        """run()'s tuple: views of the engine-owned buffers the last decode filled."""
        if self.forced:
            return self.words[1:].t(), self.att_steps.permute(1, 0, 2), self.logprob.t(), self.rank.t()
        if self.sampling or (self.constrained and self.beam == 1):
            return self.words[1:].t(), self.att_steps.permute(1, 0, 2), self.logprob.t()
        if self.beam == 1:
            return self.words[1:].t(), self.att_steps.permute(1, 0, 2)
        return self._backtrack()

    def _backtrack(self):
        """The returned hypothesis of every clip and the final beam scores [B, beam] in slot order: rank 0 (cvc_beam_backtrack), or on
        an engine with beam_groups > 1 or a length_penalty the best hypothesis by norm (cvc_beam_rank, then cvc_beam_backtrack_from
        order[:, 0]); enqueued with the decode."""
        return self.bt_seq, self.bt_att, self.score[self.T & 1].view(self.B, self.beam)

    def _backtrack_host(self):
        """The same by indexing on the host side of torch (kept as the cross-check of the kernel in the tests)."""
        B, beam, T, N = self.B, self.beam, self.T, self.N
        words = self.words[1:].view(T, B, beam)
        parent = self.parent.view(T, B, beam)
        att = self.att_steps.view(T, B, beam, N)
        k = torch.zeros(B, dtype=torch.int64, device=words.device)
        ar = torch.arange(B, device=words.device)
        seq, atts = [], []
        for t in range(T - 1, -1, -1):
            seq.append(words[t, ar, k])
            k_parent = parent[t, ar, k]
            atts.append(att[t, ar, k_parent])     # attention was computed for the parent row at step t
            k = k_parent
        seq.reverse()
        atts.reverse()
        final_scores = self.score[self.T & 1].view(B, beam)
        return torch.stack(seq, 1), torch.stack(atts, 1), final_scores
