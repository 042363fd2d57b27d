"""CaptionEnsemble: several captioners behind the decode-side surface of one ("Ensemble decoding").  Each member
encodes the batch with its own encoder; the decode runs on ONE cached cvc.decode.EnsembleEngine, which chooses one word per step from
the combined distribution.  Not an nn.Module: it owns no parameters, training steps never see it."""
from __future__ import annotations

from typing import Optional

import torch

from .. import functional as F_
from ..decode.ensemble import EnsembleEngine, EnsembleOptions
from .captioner import DecodeAndGroundCaptionerGVDROI

_FEATS = ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats")


class CaptionEnsemble:
    """CaptionEnsemble(models, weights=None, combine="prob"): _sample(...) and score(...) are DecodeAndGroundCaptionerGVDROI's own methods run on
    this object -- same signatures, keywords, defaults (member 0's attributes) and results --, with two pieces replaced: the encoder
    (every member's, on the same batch) and the cached engine (an EnsembleEngine over every member's weights and features; the key is
    the members' weights objects, their feature shapes and every option, and the cache loads the next batch's features and captions
    as DecodeAndGroundCaptionerGVDROI._decode_engine does).  logprob is the ensemble's, rank the rank under the combined distribution, the
    attention sum_m w_m att_m.  Refused: decode_weights="bf16", score(grounding=True), encoded= (one encoder's outputs), and what
    EnsembleEngine refuses.  A one-model ensemble is allowed."""

    def __init__(self, models, weights=None, combine: str = "prob"):
        self.models = list(models)
        # (the refusals that need no decode: member count, combine, weights)
        EnsembleOptions.resolve(len(self.models), 1, None, weights, combine)
        for m, model in enumerate(self.models[1:], 1):
            for k in ("vocab_size", "seq_length", "unk_idx"):
                if getattr(model, k) != getattr(self.models[0], k):
                    raise RuntimeError(f"CaptionEnsemble: member {m} has {k} = {getattr(model, k)}, member 0 has {getattr(self.models[0], k)}")
        self.member_weights, self.combine = weights, combine
        self.last_consensus: Optional[dict] = None
        self.last_stochastic: Optional[dict] = None
        self.consensus_table = None
        self._engine_cache = self._score_cache = self._soft_cache = None
        self._encoded = None

    def __getattr__(self, name):
        # decode defaults (beam_size, sample_max, the constraints, consensus, ...), opts, seq_length, unk_idx: member 0's
        if name == "models":
            raise AttributeError(name)
        return getattr(self.models[0], name)

    def eval(self):
        for m in self.models:
            m.eval()
        return self

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("CaptionEnsemble.train: an ensemble decodes, training steps never see it")
        return self.eval()

    @property
    def training(self) -> bool:
        return False

    # ---- the two pieces DecodeAndGroundCaptionerGVDROI._sample / _score call on self

    def _member_feats(self, enc):
        fc, conv, pconv, pool, ppool, pnt = enc
        return dict(fc_feats=fc.contiguous(), conv_feats=conv.contiguous(), p_conv_feats=pconv.contiguous(), pool_feats=pool.contiguous(),
                    p_pool_feats=ppool.contiguous(), pnt_mask=pnt)

    def encode_clips(self, *batch):
        self._encoded = [self._member_feats(m.encode_clips(*batch)) for m in self.models]
        e = self._encoded[0]
        return tuple(e[k] for k in _FEATS) + (e["pnt_mask"],)

    def _encode(self, *batch):
        outs = [m._encode(*batch) for m in self.models]
        self._encoded = [self._member_feats(tuple(o[1][:5]) + (o[1][6],)) for o in outs]
        return outs[0]

    def _decode_engine(self, slot, feats, T, extra=(), unkeyed=(), may_bind=False, prepare=None, **options):
        all_feats, self._encoded = self._encoded, None
        if all_feats is None:
            raise RuntimeError("CaptionEnsemble: encoded= is one encoder's output; an ensemble encodes the batch with every member")
        temp = float(getattr(self.opts, "softmax_temp", 1.0))
        weights = [m.decode_weights() for m in self.models]
        hashable = lambda v: tuple(v) if isinstance(v, (list, tuple)) else v
        mw = None if self.member_weights is None else tuple(float(w) for w in self.member_weights)
        key = (tuple(id(w) for w in weights) + tuple(tuple(f[k].shape) for f in all_feats for k in ("fc_feats", "conv_feats", "pool_feats")) +
               (temp, T, self.use_hip_graph, tuple(extra), mw, self.combine) +
               tuple((k, hashable(v)) for k, v in sorted(options.items()) if k not in unkeyed))
        cached = getattr(self, slot, None)
        if cached is not None and cached[0] == key:
            engine = cached[1]
            engine.load_features(all_feats)
        else:
            engine = EnsembleEngine(list(zip(weights, all_feats)), T, self.unk_idx, member_weights=self.member_weights, combine=self.combine,
                                    inv_temp=1.0 / temp, own_features=True, **options)
        if prepare is not None:
            prepare(engine)
        if cached is None or cached[0] != key:
            if self.use_hip_graph:
                engine.capture()
            setattr(self, slot, (key, engine))
        return engine

    # ---- the surface

    _sample = DecodeAndGroundCaptionerGVDROI._sample

    @torch.no_grad()
    def soft_targets(self, segs_feat, input_seq, gt_caption, num, proposals, gt_boxes, mask_boxes, region_feats, frm_mask, sample_idx,
                     pnt_mask):
        """The ensemble as a TEACHER (word-level distillation; DESIGN section 7, "Distillation"): forward's 11 tensors -> (rows, logprob).
        The members follow the batch's ground-truth captions gt_caption[:, :seq_per_img] on a cached forced engine that keeps the
        combined row of every step (EnsembleEngine keep_rows=True): rows [T, B * seq_per_img, V] is the ensemble's log-scale next-word
        distribution at every position, in the t-major row order of the training loops' vocabulary head; logprob [B * seq_per_img, T]
        the given words' log-probs.  Both are VIEWS of the engine's buffers: valid until the next call.  eval() semantics, no
        autograd, no host read-back.  A one-member ensemble is a single-checkpoint teacher."""
        self.eval()
        T, n = self.seq_length, self.seq_per_img
        captions = gt_caption[:, :n, :T].reshape(-1, T).contiguous()
        if captions.dtype != torch.int64:
            raise RuntimeError(f"CaptionEnsemble.soft_targets: the captions must be int64, got {captions.dtype}")
        F_.new_step()
        self._encode(segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, frm_mask, sample_idx, pnt_mask)
        engine = self._decode_engine("_soft_cache", self._encoded[0], T, forced_n=n, weights_dtype="fp32", keep_rows=True,
                                     prepare=lambda e: e.load_captions(captions))
        _seq, _att, logprob, _rank = engine.run()
        return engine.combined, logprob

    def score(self, *batch, captions: Optional[torch.Tensor] = None, grounding: bool = False, decode_weights: Optional[str] = None):
        """DecodeAndGroundCaptionerGVDROI.score over the ensemble: logprob / seq_logprob are the ensemble's log-probs of the given words, rank the
        rank under the combined distribution, att the averaged attention.  grounding=True is refused (the frame-masked scores and
        the grounder are one member's)."""
        if grounding:
            raise RuntimeError("CaptionEnsemble.score: grounding=True is refused: the frame-masked attention scores and the grounder are "
                               "a single member's")
        self.eval()
        with torch.no_grad():
            return DecodeAndGroundCaptionerGVDROI._score(self, *batch, captions, False, decode_weights)
