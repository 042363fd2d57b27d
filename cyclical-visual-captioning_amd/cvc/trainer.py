"""Train / eval harness with the reference's hooks (trainer.py:26-373): the 12-tuple batch
contract, the per-batch trimming, the 11-tensor model call, the loss mix (ground_loss is returned
but never optimised), zero_grad -> backward -> [gradient all-reduce] -> clip_grad_norm_(0.1) ->
step.  Reference bugs are not copied: `next(it)` instead of `.next()`, the
reconstruction-loss meter is updated, grounding stats are only logged when they exist.

Caption / grounding scoring lives in external toolkits the reference vendors as (empty)
submodules; pass `scorer(predictions, grd_output, opts) -> dict` to get language stats, and / or
`device_metrics=True` for BLEU, ROUGE-L and CIDEr-D by word id on the device (cvc.metrics) -- and, with opts.eval_obj_grounding
beside it, the grounding F1 of the generated captions (cvc.metrics.GroundingScorer).
"""
from __future__ import annotations

import contextlib
import functools
import json
import os
import time
from collections import defaultdict

import numpy as np
import torch
import torch.nn as nn

from .distributed import GradReducer, gather_eval_outputs
from .prefetch import DevicePrefetcher
from .misc import utils
from .misc.utils import AverageMeter


def _trim(t, n, dim=1):
    return t.narrow(dim, 0, n)


SHAPE_BUCKETS = 4         # trimmed lengths are rounded up to one of this many sizes per axis (graphed training: one graph per shape)


def bucket_len(n: int, full: int, buckets: int = SHAPE_BUCKETS) -> int:
    """n rounded up to the next of `buckets` evenly spaced lengths <= full (the loader's padded length).  What lies between n and
    the bucket's length is the loader's OWN padding -- zero rows with their mask bit set (dataloader_anet.py:376-388), exactly what
    a shorter clip of the batch already carries up to the batch maximum (trainer.py:63-69) -- so the step computes the same
    function of the batch, only the set of distinct shapes becomes small enough to keep one captured graph per shape.
    ONE EXCEPTION, handled by the caller (Trainer._prepare): a clip whose proposals are ALL masked.  The reference's mask fill is the
    finite -1e8 (model/modules.py:122-129), so such a row's softmax is uniform over all N positions of the trimmed axis and its
    context the mean of N rows; a longer axis changes that N.  A batch that contains a clip with zero proposals is therefore
    trimmed exactly as the reference trims it, never bucketed."""
    if buckets <= 0 or n >= full:
        return min(n, full)
    step = -(-full // buckets)
    return min(full, -(-n // step) * step)


def ss_prob_at(epoch: int, start: int, increase_every: int = 5, increase_prob: float = 0.05, max_prob: float = 0.25) -> float:
    """The scheduled-sampling share of an epoch: 0 before epoch `start` (and always with start < 0), then
    min(max_prob, increase_prob * ((epoch - start) // increase_every)) -- a staircase that starts at 0 and is capped."""
    if start < 0 or epoch < start:
        return 0.0
    return float(min(max_prob, increase_prob * ((epoch - start) // max(int(increase_every), 1))))


def _shape_key(b) -> tuple:
    out = []
    for k in sorted(b):
        v = b[k]
        if isinstance(v, torch.Tensor):
            out.append((k, tuple(v.shape), str(v.dtype)))
        elif isinstance(v, dict):
            out.append((k, tuple((kk, tuple(vv.shape), str(vv.dtype)) for kk, vv in sorted(v.items()) if isinstance(vv, torch.Tensor))))
    return tuple(out)


def _copy_into(static, b):
    for k, v in b.items():
        if isinstance(v, torch.Tensor):
            static[k].copy_(v, non_blocking=True)
        elif isinstance(v, dict):
            for kk, vv in v.items():
                if isinstance(vv, torch.Tensor):
                    static[k][kk].copy_(vv, non_blocking=True)
        else:
            static[k] = v


def _averaged_by_default(fn):
    """eval / sample / score / ground_gt take `weights="ema" | "live"`: on the averaged weights (Trainer.averaged_weights) when the
    weight average is attached, unless told otherwise; without an average the method is what it was"""
    @functools.wraps(fn)
    def wrapper(self, *a, weights=None, **kw):
        if self._use_ema(weights):
            with self.averaged_weights():
                return fn(self, *a, **kw)
        return fn(self, *a, **kw)
    return wrapper


class Trainer:
    # a cvc.model.CaptionEnsemble over the model (member 0) and further checkpoints, set by whoever builds the trainer (cvc.main
    # --ensemble): eval(), sample() and score() then decode through it; training steps never see it.  None: every decode is the model's
    ensemble = None
    _averaged = 0                     # depth of averaged_weights(): non-zero while the parameters hold the weight averages

    def __init__(self, opts, dataset, model, optimizer, train_loader, val_loader, scorer=None, grad_reducer=None, device_metrics=False,
                 val_diversity=False, ema=None, val_self_cider=False):
        self.opts = opts
        self.dataset = dataset
        self.model = model
        self.optimizer = optimizer
        self.train_loader = train_loader
        self.val_loader = val_loader
        self.scorer = scorer
        self.grad_reducer = grad_reducer
        # eval(): BLEU-1..4, ROUGE-L and CIDEr-D of the decoded captions against the batches' own references, on the device
        # (cvc.metrics.DeviceScorer); off: eval is what it was
        self.device_metrics = bool(device_metrics)
        # eval(): the diversity of every clip's candidate set (cvc.metrics.DiversityScorer over model.last_consensus) next to the
        # device metrics; off: eval is what it was
        self.val_diversity = bool(val_diversity)
        # eval(): Self-CIDEr and LSA diversity of the same candidate sets (cvc.metrics.SpectrumScorer) next to the set diversity;
        # off: eval is what it was
        self.val_self_cider = bool(val_self_cider)
        if self.val_self_cider and not self.val_diversity:
            raise RuntimeError("Trainer: val_self_cider scores the candidate sets of val_diversity -- it needs val_diversity=True")
        self._val_cider = None        # cvc.cider.CiderD over the validation loader's captions, built at the first eval
        self._word_cls = None         # word id -> detection class (utils.word_class_table), built at the first eval that grounds
        self.device = next(model.parameters()).device
        self._graph = None            # HIP-graph state of train_step_graphed
        # ---- train(): one captured graph per (bucketed) batch shape
        # shape buckets exist for ONE purpose -- a small set of shapes to keep captured graphs for -- so they are active only while
        # train() replays graphs (decided at the start of every train(): graph_capable()); an eager run (raw features through an
        # encoder that cannot be captured, a c10d / gloo exchange, a non-capturable optimizer, the CPU) trims exactly as the
        # reference does (trainer.py:63-69) and pays for no padding
        self.shape_buckets = SHAPE_BUCKETS if bool(getattr(opts, "hip_graph", 0)) else 0
        self._active_buckets = 0
        # deferred error words (cvc.hip.defer_errors): the step's status word while train() runs a model whose persistent kernels
        # report time-outs (the once-per-clip encoder's GRU) as captured / replayed steps; None otherwise
        self._status = None
        self.deferred_stats = dict(void_steps=0, rerun_steps=0)
        self._graphs = {}             # shape key -> (graph, static inputs, static result)
        self._shape_seen = {}         # shape key -> eager steps taken at that shape
        self._eager_steps = 0
        self._graph_pool = None
        self._side = None
        self._graph_broken = False
        self.graph_stats = dict(eager=0, replayed=0, captured=0)
        # ---- self-critical training (scst_step): from epoch opts.scst_after on, -1 = never
        self.scst_after = int(getattr(opts, "scst_after", -1))
        self._cider = None            # cvc.cider.CiderD over the training captions, built at the first self-critical step
        self._scst_steps = 0
        self.last_scst = None
        # the reward mix {name: weight} (cvc.metrics.REWARD_NAMES; cvc.main --scst_reward); None or cider alone at 1: CIDEr-D as ever
        self.scst_reward_weights = getattr(opts, "scst_reward_weights", None)
        # rollouts without replacement (cvc.main --scst_wor): a stochastic beam of scst_samples + 1 slots, importance-weighted
        self.scst_wor = bool(getattr(opts, "scst_wor", False))
        if self.scst_wor:
            self._scst_wor_samples()
        self.reward_history = {}     # epoch -> the mean reward of every display interval
        # ---- scheduled sampling (train_step_prepared while model.ss_prob > 0): rollout temperature, seed of step k = ss_seed + k
        self.ss_temperature = float(getattr(opts, "ss_temperature", 1.0))
        self.ss_seed = int(getattr(opts, "ss_seed", 1))
        self._ss_steps = 0
        self.last_ss = None
        # ---- label smoothing of the cross-entropy steps (the model's criteria: cvc.main --label_smoothing): fixed when the trainer is
        # built -- a captured step holds it as a launch argument.  With eps > 0 every cross-entropy step's result carries one more
        # element at its END, loop A's unsmoothed mean NLL (model.last_nll), and train() logs it beside the smoothed LM loss
        self.label_smoothing = float(getattr(getattr(model, "module", model), "label_smoothing", 0.0))
        self.nll_history = {}         # epoch -> the mean unsmoothed NLL of every display interval (label_smoothing > 0)
        # ---- entropy regulariser (cvc.main --confidence_penalty / --scst_entropy / --log_entropy): the cross-entropy and
        # scheduled-sampling steps take opts.confidence_penalty (else the model's), the self-critical steps opts.scst_entropy; None =
        # off (the launches of a trainer without it), log_entropy turns a None into 0 = measured only.  Fixed when the trainer is built
        # -- a captured step holds beta as a launch argument.  With it not None every step's result carries one more element at its
        # very END (behind the NLL of label smoothing), the mean masked entropy of the word distribution, read back with the rest
        from . import hip as _hip
        core = getattr(model, "module", model)
        self.log_entropy = bool(getattr(opts, "log_entropy", False))
        beta = getattr(opts, "confidence_penalty", None)
        if beta is None:
            beta = getattr(core, "confidence_penalty", None)
        if beta is None and self.log_entropy:
            beta = 0.0
        self.confidence_penalty = None if beta is None else _hip.check_entropy_beta(beta, "confidence_penalty")
        if self.confidence_penalty is not None and getattr(core, "confidence_penalty", None) != self.confidence_penalty:
            core.confidence_penalty = self.confidence_penalty
        beta = getattr(opts, "scst_entropy", None)
        if beta is None and self.log_entropy:
            beta = 0.0
        self.scst_entropy = None if beta is None else _hip.check_entropy_beta(beta, "scst_entropy")
        self.entropy_history = {}     # epoch -> the mean entropy of every display interval (a coefficient that is not None)
        # ---- word-level distillation (model.distill = dict(teacher=CaptionEnsemble, alpha=, tau=); cvc.main --distill_from): the
        # cross-entropy steps run eagerly with the teacher's forced pass in front (_kd_step_prepared); their result carries two more
        # elements at its end, loop A's unmixed mean NLL and its unmixed mean tau^2 KL(teacher || student).  Self-critical steps are
        # not distilled
        self.kd_history = {}          # epoch -> the mean KD of every display interval (distilled steps)
        self.last_kd = None
        # ---- weight averaging (ema=(decay, warmup), or opts.ema_decay / opts.ema_warmup: cvc.main --ema_decay): an exponential moving
        # average of every stepped parameter, kept INSIDE the optimizer pass (cvc.optim._ClipStep.attach_ema) and therefore by every
        # step kind, captured or eager, and by no void step.  Attached here, before anything is captured: a captured step holds the
        # entry it launches.  eval / sample / score then run on the averaged weights (averaged_weights)
        if ema is None and getattr(opts, "ema_decay", 0):
            ema = (float(opts.ema_decay), bool(getattr(opts, "ema_warmup", False)))
        if ema:                       # (ema=False: none, whatever the options say)
            attach = getattr(optimizer, "attach_ema", None)
            if attach is None:
                raise RuntimeError("Trainer: the weight average is kept by the native optimizer step (cvc.optim.ClipAdam / ClipSGD / "
                                   "ClipAdamax); %s is a library optimizer (CVC_CLIP_ADAM=0, or parameters on the CPU) and gets "
                                   "none -- it is not emulated" % type(optimizer).__name__)
            attach(float(ema[0]), bool(ema[1]))

    # ------------------------------------------------------------------ batch plumbing
    def _prepare(self, batch, train: bool):
        seg_feat, iseq, gts_seq, num, proposals, bboxs, box_mask, seg_id, region_feat, frm_mask, sample_idx, ppl_mask = batch
        n_prop = max(int(num[:, 1].max()), 1)
        # a clip with zero proposals is a uniform softmax over the trimmed axis (bucket_len's exception): trim such a batch exactly
        buckets = self._active_buckets if (train and int(num[:, 1].min()) > 0) else 0
        if buckets:
            n_prop = bucket_len(n_prop, proposals.size(1), buckets)
        proposals, ppl_mask, region_feat = _trim(proposals, n_prop), _trim(ppl_mask, n_prop), _trim(region_feat, n_prop)
        if train:
            n_box = max(int(num[:, 2].max()), 1)
            if buckets:
                n_box = bucket_len(n_box, bboxs.size(1), buckets)
            bboxs, box_mask = _trim(bboxs, n_box), _trim(box_mask, n_box, 2)
            frm_mask = _trim(_trim(frm_mask, n_prop), n_box, 2)
        dev = self.device
        # async from pinned memory; a trimmed view that already lives on the device is made dense (the kernels take contiguous tensors)
        to = lambda x: x.to(dev, non_blocking=True).contiguous() if isinstance(x, torch.Tensor) else x
        if isinstance(seg_feat, dict):
            # pre-extracted features (cvc.model.captioner.PrecomputedRegionFeatures): their region axis is trimmed with the proposals
            reg = {"pool_feats": n_prop, "p_pool_feats": n_prop, "g_pool_feats": n_prop, "pnt_mask": n_prop + 1}
            seg = {k: to(_trim(v, reg[k]) if (k in reg and v.size(1) > reg[k]) else v) for k, v in seg_feat.items()}
        else:
            seg = to(seg_feat).float()
        mask_ppls = to(ppl_mask)
        pnt_mask = torch.cat((mask_ppls.new_zeros(mask_ppls.size(0), 1), mask_ppls), dim=1)
        return dict(segs_feat=seg, input_seqs=to(iseq), gt_seqs=to(gts_seq), num=to(num), ppls=to(proposals),
                    gt_bboxs=to(bboxs), mask_bboxs=to(box_mask), ppls_feat=to(region_feat), mask_frms=to(frm_mask),
                    sample_idx=to(sample_idx).type_as(to(iseq)), pnt_mask=pnt_mask, seg_id=seg_id)

    def _decoder(self):
        """who decodes in eval() / sample() / score(): the ensemble when one is set, else the model itself"""
        return self.ensemble if self.ensemble is not None else getattr(self.model, "module", self.model)

    def _call(self, b, lang_eval=False, **kw):
        if lang_eval and self.ensemble is not None and not kw.get("teacher_forcing", False):
            return self.ensemble._sample(b["segs_feat"], b["input_seqs"], b["ppls"], b["gt_seqs"], b["num"], b["mask_bboxs"], b["gt_bboxs"],
                                         b["ppls_feat"], b["mask_frms"], b["sample_idx"], b["pnt_mask"])
        return self.model(b["segs_feat"], b["input_seqs"], b["gt_seqs"], b["num"], b["ppls"], b["gt_bboxs"], b["mask_bboxs"],
                          b["ppls_feat"], b["mask_frms"], b["sample_idx"], b["pnt_mask"], lang_eval, **kw)

    def loss_mix(self, out):
        """trainer.py:92-109"""
        o = self.opts
        # the reference takes .mean() of every loss because DataParallel gathers one value per replica; one process per GPU holds
        # one value: the mean of a one-element tensor is that element (no reduction kernel, none in the backward)
        one = lambda x: x.reshape(()) if x.numel() == 1 else x.mean()
        lm_loss, att2_loss, _ground_loss, cls_loss = [one(x) for x in out[:4]]
        lm_recon = one(out[4]) if len(out) > 4 else torch.zeros((), device=lm_loss.device)
        # terms with a zero weight (w_att2 = w_cls = 0 by default, opts.py:72-75) add an exact zero and a zero gradient: left out
        terms = [(o.xe_loss_weight, lm_loss), (o.w_att2, att2_loss), (o.w_cls, cls_loss)]
        if len(out) > 4:
            terms.append((o.caption_consistency_loss_weight, lm_recon))
        loss = None
        for wgt, val in terms:
            if wgt != 0:
                loss = wgt * val if loss is None else loss + wgt * val
        if loss is None:
            loss = 0.0 * lm_loss
        return loss, lm_loss, att2_loss, cls_loss, lm_recon

    def _nll_tail(self):
        """(loop A's unsmoothed mean NLL of the pass that just ran,) with label smoothing on, else ()"""
        if not self.label_smoothing > 0:
            return ()
        model = getattr(self.model, "module", self.model)
        if float(model.label_smoothing) != self.label_smoothing:
            raise RuntimeError(f"Trainer: the model's label_smoothing is {model.label_smoothing}, the trainer was built with "
                               f"{self.label_smoothing} (captured steps hold it as a launch argument: build a new Trainer)")
        return (model.last_nll.detach().reshape(()),)

    def _ent_tail(self):
        """(loop A's mean masked entropy of the pass that just ran,) with a confidence penalty (0 included), else ()"""
        model = getattr(self.model, "module", self.model)
        beta = getattr(model, "confidence_penalty", None)
        if beta != self.confidence_penalty:
            raise RuntimeError(f"Trainer: the model's confidence_penalty is {beta}, the trainer was built with "
                               f"{self.confidence_penalty} (captured steps hold it as a launch argument: build a new Trainer)")
        if self.confidence_penalty is None:
            return ()
        return (model.last_entropy.detach().reshape(()),)

    def train_step(self, batch):
        return self.train_step_prepared(self._prepare(batch, True))

    def train_step_prepared(self, b):
        """One optimisation step on a batch that already is on the device (see cvc.prefetch.DevicePrefetcher)."""
        if self.opts.att_model != 'cyclical':
            raise ValueError('Unknown att_model: {}'.format(self.opts.att_model))
        if float(getattr(getattr(self.model, "module", self.model), "ss_prob", 0.0)) > 0:
            if self._distilling():
                raise RuntimeError("Trainer: model.distill together with scheduled sampling (model.ss_prob > 0) is refused: the student "
                                   "would be fed words the teacher never saw")
            return self._ss_step_prepared(b)
        if self._distilling():
            return self._kd_step_prepared(b)
        out = self._call(b)
        loss, lm, att2, cls, rec = self.loss_mix(out)
        self._backward_and_update(loss)
        self._weights_changed()
        return (loss.detach(), lm.detach(), att2.detach(), cls.detach(), rec.detach(), *self._nll_tail(), *self._ent_tail())

    def _distilling(self) -> bool:
        return getattr(getattr(self.model, "module", self.model), "distill", None) is not None

    def _kd_step_prepared(self, b):
        """The distillation step (Hinton et al. 2015; Kim & Rush 2016, word level; model.distill set): the teacher -- a CaptionEnsemble
        of frozen checkpoints -- follows the batch's ground-truth captions on its cached forced engine and leaves its next-word
        distribution of every position (teacher.soft_targets: eval mode, no autograd), then the ordinary cyclical pass with loop A's
        criterion (1 - alpha) NLL + alpha tau^2 KL(teacher || student) at temperature tau, and the update.  Runs eagerly; no host
        read-back between the teacher pass and optimizer.step().  -> (loss, lm, att2, cls, recon, loop A's unmixed mean NLL, its unmixed
        mean KD); self.last_kd keeps the teacher's log-probs of the given words and the step's KD (device tensors)."""
        model = getattr(self.model, "module", self.model)
        if self.label_smoothing > 0 or self.confidence_penalty is not None:
            raise ValueError("Trainer: model.distill cannot be combined with label_smoothing > 0 or a confidence penalty (the teacher's "
                             "row is the target distribution)")
        rows, t_logprob = model.distill["teacher"].soft_targets(
            b["segs_feat"], b["input_seqs"], b["gt_seqs"], b["num"], b["ppls"], b["gt_bboxs"], b["mask_bboxs"], b["ppls_feat"],
            b["mask_frms"], b["sample_idx"], b["pnt_mask"])
        out = self._call(b, soft_targets=rows)
        loss, lm, att2, cls, rec = self.loss_mix(out)
        nll, kd = model.last_nll.detach().reshape(()), model.last_kd.detach().reshape(())
        self._backward_and_update(loss)
        self._weights_changed()
        self.last_kd = dict(teacher_logprob=t_logprob, kd=kd, nll=nll)
        return (loss.detach(), lm.detach(), att2.detach(), cls.detach(), rec.detach(), nll, kd)

    def _ss_step_prepared(self, b):
        """The scheduled-sampling step (Bengio et al. 2015; model.ss_prob > 0): the encoder once in eval mode without autograd, one
        decode of the cached mixed engine over the ground-truth captions (model.ss_rollout, seed ss_seed + step: every position feeds
        on the model's own sample with probability ss_prob, else the ground truth's word), then the ordinary cyclical pass with those
        words as loop A's inputs, the update, and model.refresh_decode_weights() -- the engine and its graph survive the update.
        The rollout samples from the eval-mode policy without UNK, as the sampling engine does.  Runs eagerly; no host read-back
        between the rollout and optimizer.step().  self.last_ss keeps the step's inputs, took, given_logprob, seed and the share of
        sampled inputs (a device scalar)."""
        model = getattr(self.model, "module", self.model)
        seed = self.ss_seed + self._ss_steps
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                enc = model.encode_clips(b["segs_feat"], b["ppls"], b["num"], b["mask_bboxs"], b["ppls_feat"], b["gt_bboxs"], b["mask_frms"],
                                         b["sample_idx"], b["pnt_mask"])
                ss_inputs = model.ss_rollout(enc, b["gt_seqs"], float(model.ss_prob), self.ss_temperature, seed)
                eng = model.ss_engine()
                took = eng.took.t().clone()                               # [rows, T]; column t decided the input of step t + 1
                given_logprob = eng.given_logprob.t().clone()
        finally:
            model.train(was_training)
        out = self._call(b, ss_inputs=ss_inputs)
        loss, lm, att2, cls, rec = self.loss_mix(out)
        nll = self._nll_tail() + self._ent_tail()
        self._backward_and_update(loss)
        model.refresh_decode_weights()
        T = took.size(1)
        share = took[:, :T - 1].float().mean() if T > 1 else took.new_zeros((), dtype=torch.float32)
        self.last_ss = dict(inputs=ss_inputs, took=took, given_logprob=given_logprob, seed=seed, share=share,
                            prob=float(model.ss_prob))
        self._ss_steps += 1
        return (loss.detach(), lm.detach(), att2.detach(), cls.detach(), rec.detach(), *nll)

    def _backward_and_update(self, loss, set_to_none=True):
        """zero_grad -> backward -> [gradient exchange] -> clip_grad_norm_ -> step (trainer.py:116-122).  With a GradReducer
        the gradients live in flat arenas: one fill to zero them, the exchange in place, one multiply to clip (1/G folded in)."""
        if self._averaged:
            raise RuntimeError("Trainer: a training step inside averaged_weights() would update the averages in the parameters' place")
        red = self.grad_reducer
        fused = getattr(self.optimizer, "clip_and_step", None)     # cvc.optim.ClipAdam: norm + clip + Adam in three launches
        if red is None:
            # ClipAdam keys its device segment table on the gradients' addresses: keep them (zero in place) instead of fresh
            # tensors every step, which would rebuild and re-upload the table per step
            self.optimizer.zero_grad(set_to_none=set_to_none and fused is None)
            loss.backward()
            if fused is not None:
                fused(self.opts.grad_clip, 1.0, **({'skip': self._status} if self._status is not None else {}))
                return
            nn.utils.clip_grad_norm_(self.model.parameters(), self.opts.grad_clip)
        else:
            red.zero_grad()
            loss.backward()
            # the one exchange step of the path (+ the step's status word, so that every rank voids -- and later re-runs -- the
            # same steps: a void step's gradients have already been summed into every rank's arenas)
            red.finalize(average=False, status=self._status)
            if fused is not None:
                # (the arenas hold sums over ranks: 1 / G folded into the coefficient; the gradients are read here for the last
                # time, so the pass leaves them zero and the next step's zero_grad() has nothing to fill)
                fused(self.opts.grad_clip, 1.0 / red.world, zero_grad=True, **({'skip': self._status} if self._status is not None else {}))
                red.mark_zeroed()
                return
            red.clip_(self.opts.grad_clip, summed=True)
        self.optimizer.step()

    def _weights_changed(self):
        """The fused Adam kernel and HIP-graph replays update parameters without touching their version counters,
        which is what the captioner's cached decode binding watches: drop it explicitly."""
        inval = getattr(self.model, "invalidate_decode_cache", None)
        if inval is not None:
            inval()                               # (bumps the weights generation as well)
        else:
            from . import hip
            hip.bump_weights_generation()

    # ------------------------------------------------------------------ weight averaging
    @property
    def ema_active(self) -> bool:
        return bool(getattr(getattr(self, "optimizer", None), "ema_active", False))

    def _use_ema(self, weights) -> bool:
        if weights not in (None, "ema", "live"):
            raise ValueError("weights must be 'ema' or 'live', got %r" % (weights,))
        if weights == "ema" and not self.ema_active:
            raise RuntimeError("weights='ema': no weight average is attached (Trainer(ema=...), cvc.main --ema_decay)")
        return self.ema_active if weights is None else weights == "ema"

    @contextlib.contextmanager
    def averaged_weights(self):
        """The averaged weights in the parameters' OWN storage while the block runs (optimizer.averaged(): one exchange launch in,
        one out, the live values back bit for bit).  Everything keyed on the parameters' addresses -- the decode engine's packs,
        the encoder's operands, the optimizer's tables, captured graphs -- stays valid; what caches VALUES is told on the way in
        and out (_weights_changed).  Re-entrant: an inner block changes nothing.  No training step may run inside."""
        if self._averaged:
            self._averaged += 1
            try:
                yield
            finally:
                self._averaged -= 1
            return
        with self.optimizer.averaged():
            self._averaged = 1
            self._weights_changed()
            try:
                yield
            finally:
                self._averaged = 0
        self._weights_changed()

    # ------------------------------------------------------------------ self-critical training step
    def cider(self):
        """the CIDEr-D table of the training captions (cvc.cider.CiderD.from_dataset), built on first use"""
        if self._cider is None:
            from .cider import CiderD
            self._cider = CiderD.from_dataset(self.dataset, self.device)
        return self._cider

    def _consensus_table(self, model):
        """consensus selection (model._sample(consensus=...)) takes its utilities over the training captions' table: set on first use"""
        if model.consensus_table is None:
            model.consensus_table = self.cider()

    def scst_step(self, batch):
        return self.scst_step_prepared(self._prepare(batch, True))

    def _scst_wor_samples(self) -> int:
        """opts.scst_samples for a step without replacement, refused outside [2, 7]"""
        S = int(getattr(self.opts, "scst_samples", 5))
        if S < 2:
            raise RuntimeError(f"Trainer: scst_wor needs scst_samples >= 2, got {S} (the baseline of a without-replacement rollout is built "
                               f"from the clip's other rollouts: one rollout's own baseline cancels it)")
        if S > 7:
            raise RuntimeError(f"Trainer: scst_wor takes scst_samples <= 7, got {S} (the rollouts are a stochastic beam of scst_samples + 1 "
                               f"slots, and a beam holds at most 8)")
        return S

    def scst_step_prepared(self, b):
        """One self-critical optimisation step (SCST, Rennie et al. 2017) on a prepared batch: S = opts.scst_samples captions per clip
        sampled from the model at opts.scst_temperature (the cached decode binding, DecodeEngine's sampling mode), scored against the
        clip's ground-truth captions with CIDEr-D on the device (cvc.cider) -- or, with opts.scst_reward_weights, with the mix
        sum_k w_k metric_k of CIDEr-D, BLEU-1..4 and ROUGE-L (cvc.metrics.reward_mix: raw scales, CIDEr-D in [0, 10], the others in
        [0, 1]; fixed order, fp32 on the device; the greedy baseline is scored with the same mix) -- and the REINFORCE gradient of
        -sum adv * log p(sampled word) / sum(mask) through loop A and the vocabulary head (model.scst_loss).  Baseline: the mean
        reward of the clip's other samples (S > 1), or the reward of the greedy caption (S = 1).  The encoder runs once, without
        autograd and in eval mode; the decoder's parameters (decoder_core, embed, logit) are what the loss reaches.  Dropout is off in
        the gradient pass unless opts.scst_dropout.  No host read-back between the rollout and optimizer.step().
        The sampler leaves UNK out while log p is taken over the full vocabulary, as in the sampling engine.  Runs eagerly.
        opts.scst_wor (2 <= S <= 7): the rollouts are drawn WITHOUT replacement -- model._sample(beam_size=S + 1, stochastic_beam=True,
        stochastic_tau=scst_temperature), slots 0 .. S-1 -- so no two rollouts of a clip are the same sentence; rewards are taken on
        those B * S rows unchanged and model.scst_loss(wor=) weights them (cvc_scst_weights_wor: importance weights, per-row
        baseline; DESIGN section 7, "Self-critical training without replacement").  last_scst then also holds logq, G [B, S + 1],
        state, wgt [B * S], expected_reward [B] and distinct (the share of live rollouts: 1 whenever a clip has S captions to give);
        logprob is None, and the third scalar is the mean of expected_reward.
        -> (loss, mean reward, mean baseline, mean |advantage|) as device scalars; the step's samples, rewards and advantages stay
        in self.last_scst (with a mix also reward_parts: the metrics that were weighted, per row)."""
        from . import metrics
        model = getattr(self.model, "module", self.model)
        o = self.opts
        mix = None if metrics.is_cider_only(self.scst_reward_weights) else self.scst_reward_weights
        parts = None
        S, tau = int(getattr(o, "scst_samples", 5)), float(getattr(o, "scst_temperature", 1.0))
        wor = None
        if self.scst_wor:
            S = self._scst_wor_samples()
        seed = int(getattr(o, "scst_seed", 1)) + self._scst_steps          # a sampling engine is seeded when it is built: once per step
        cider = self.cider()
        T = model.seq_length
        plain = dict(beam_size=1, top_k=0, top_p=1.0, no_repeat_ngram=0, no_immediate_repeat=False, min_len=0, ban_words=(), bad_endings=(),
                     beam_groups=1, diversity_lambda=0.0, length_penalty=0.0, consensus=False)
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                enc = model.encode_clips(b["segs_feat"], b["ppls"], b["num"], b["mask_bboxs"], b["ppls_feat"], b["gt_bboxs"], b["mask_frms"],
                                         b["sample_idx"], b["pnt_mask"])
                args = (b["segs_feat"], b["input_seqs"], b["ppls"], b["gt_seqs"], b["num"], b["mask_bboxs"], b["gt_bboxs"], b["ppls_feat"],
                        b["mask_frms"], b["sample_idx"], b["pnt_mask"])
                if self.scst_wor:
                    # a stochastic beam of S + 1 slots: slots 0 .. S-1 are the clip's rollouts (pairwise distinct, in draw order), slot
                    # S gives the threshold key.  The model's five constraints compose, as they do in the stochastic engine
                    model._sample(*args, beam_size=S + 1, sample_max=1, stochastic_beam=True, stochastic_tau=tau, seed=seed, encoded=enc,
                                  consensus=False, beam_groups=1, diversity_lambda=0.0, length_penalty=0.0)
                    draws = model.last_stochastic
                    seq, logprob = draws["seq"][:, :S].reshape(-1, T), None
                    wor = dict(logq=draws["logq"], G=draws["G"], state=draws["state"], normalize=True)
                else:
                    seq, _, logprob = model._sample(*args, sample_max=0, temperature=tau, sample_n=S, seed=seed, encoded=enc, **plain)
                seq = seq.contiguous()
                refs = b["gt_seqs"][:, :, :T].contiguous()
                nref = b["num"][:, 0].to(torch.int32)
                if mix is None:
                    reward = cider.score(seq, refs, nref)
                else:
                    reward, parts = metrics.reward_mix(mix, cider, seq, refs, nref)
                base = greedy = None
                if S == 1:
                    greedy = model._sample(*args, sample_max=1, encoded=enc, **plain)[0].contiguous()
                    base = cider.score(greedy, refs, nref) if mix is None else metrics.reward_mix(mix, cider, greedy, refs, nref)[0]
            if bool(getattr(o, "scst_dropout", False)):
                model.train()
            ent = {} if self.scst_entropy is None else dict(entropy_beta=self.scst_entropy)       # (off: the call of a trainer without it)
            loss, adv = (model.scst_loss(enc, seq, reward, base, S, **ent) if wor is None else
                         model.scst_loss(enc, seq, reward, None, S, wor=wor, **ent))
        finally:
            model.train(was_training)
        self._backward_and_update(loss)
        self._weights_changed()
        self._scst_steps += 1
        self.last_scst = dict(seq=seq, logprob=logprob, reward=reward, base=base, greedy=greedy, adv=adv, seed=seed)
        if mix is not None:
            self.last_scst["reward_parts"] = parts
        if self.scst_entropy is not None:       # (the mean entropy of the word distribution over the rollouts' steps: a device scalar)
            self.last_scst["entropy"] = model.last_entropy
        if wor is not None:
            est = model.last_wor["est"]
            self.last_scst.update(logq=wor["logq"], G=wor["G"], state=wor["state"], wgt=model.last_wor["wgt"], expected_reward=est,
                                  distinct=torch.isfinite(wor["G"][:, :S]).to(torch.float32).mean())
            # the mean baseline: a row's baseline B_i / W_i estimates the clip's expected reward, which est is
            return loss.detach(), reward.mean(), est.mean(), adv.abs().mean()
        return loss.detach(), reward.mean(), (reward - adv).mean(), adv.abs().mean()

    # ------------------------------------------------------------------ HIP-graph training step
    def _core_step(self, b):
        out = self._call(b)
        loss, lm, att2, cls, rec = self.loss_mix(out)
        nll = self._nll_tail() + self._ent_tail()
        self._backward_and_update(loss, set_to_none=False)
        res = torch.stack([loss.detach().reshape(()), lm.detach().reshape(()), att2.detach().reshape(()),
                           cls.detach().reshape(()), rec.detach().reshape(())])
        st = self._status
        if st is not None:
            # deferred error words: a step some launch declared void contributes nothing to the loss sums and says so in a sixth
            # element; the word is cleared at the END of the step (whoever sets it before a step voids that step: tests do)
            void = st != 0
            res = torch.cat((torch.where(void, torch.zeros_like(res), res), void.to(res.dtype)))
            if nll:                       # (label smoothing: the unsmoothed NLL goes last, behind the layout everybody knows; the
                tail = torch.stack(nll)   # mean entropy of a confidence penalty behind that)
                res = torch.cat((res, torch.where(void, torch.zeros_like(tail), tail)))
            st.zero_()
        elif nll:
            res = torch.cat((res, torch.stack(nll)))
        return res

    def train_step_graphed(self, batch):
        """Same step as train_step, captured once into a HIP graph and replayed: the per-step Python / launch overhead
        disappears.  Requirements: constant batch shapes (inputs are copied into static buffers), an optimizer built with
        capturable=True (build_optimizer(..., capturable=True)).  The gradient exchange of a multi-rank GradReducer is part of
        the captured step when it runs on RCCL (backend "nccl": the collectives are issued on the communicator's stream behind
        events of the capturing stream, which stream capture records as graph dependencies); other backends (gloo) cannot be
        captured.  Returns a static tensor [loss, lm, att2, cls, recon] (clone to keep); with label smoothing one more element at
        the end, loop A's unsmoothed mean NLL; with a confidence penalty (0 included) one more behind that, loop A's mean entropy."""
        self._check_capturable()
        b = self._prepare(batch, True)
        if self._graph is None:
            static = {k: (v.clone() if isinstance(v, torch.Tensor) else ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v))
                      for k, v in b.items()}
            s = torch.cuda.Stream()
            if self.grad_reducer is not None:
                self.grad_reducer.bind_stream(s)                    # gradient accumulators on the stream of warm-up AND capture
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(3):                                  # warm-up on a side stream (allocator, lazy init, Adam state)
                    self._core_step(static)
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s, capture_error_mode=self._capture_mode()):
                res = self._core_step(static)
            self._graph = (g, static, res)
        g, static, res = self._graph
        _copy_into(static, b)
        sync = getattr(self.optimizer, "sync_hyperparameters", None)
        if sync is not None:
            sync()                                # a scheduler may have moved the learning rates since the capture
        g.replay()
        self._weights_changed()
        return res

    def _check_capturable(self):
        """The gradient exchange inside a captured step must be a pure stream operation: the package's own RCCL communicator
        (GradReducer(comm=...), backend "rccl").  torch.distributed's collectives are refused -- gloo is host-side, and c10d's
        "nccl" group keeps a watchdog thread whose event queries race with the capture (round-4 finding: it killed about one
        capture in five; there is no way to fence it off short of waiting it out, which this code no longer does)."""
        red = self.grad_reducer
        if red is not None and red.exchange and red.backend != "rccl":
            raise RuntimeError(f"train_step_graphed: the gradient exchange on torch.distributed backend {red.backend!r} cannot be captured "
                               "into a HIP graph; build the GradReducer with comm=cvc.distributed.exchange_comm() (cvc.comm.RcclComm), "
                               "or use train_step")

    @staticmethod
    def _capture_mode() -> str:
        """"thread_local" when somebody's c10d "nccl" group is up in this process (its watchdog polls events from another thread:
        under "global" capture mode those queries fail and the watchdog takes the process down); nothing of that group is part of
        the captured step, so there is nothing to wait for."""
        import torch.distributed as dist
        up = dist.is_available() and dist.is_initialized() and dist.get_backend() == "nccl"
        return "thread_local" if up else "global"

    def graph_capable(self) -> bool:
        """train() replays captured steps when: --hip_graph is on, the optimizer keeps its step state on the device (ClipAdam or a
        capturable torch optimizer), and the gradient exchange (if any) is a stream operation."""
        if not self.shape_buckets or self.device.type != "cuda":
            return False
        # the model's whole step must consist of stream operations: the decode / localize / reconstruct path on pre-extracted
        # features is; the once-per-clip encoder is not (its persistent GRU reports barrier time-outs through a host read, widths
        # outside the HIP forms run in the library) -- raw-feature runs through the encoder train with eager steps
        cap = getattr(self.model, "step_capturable", None)
        if cap is None or not cap(deferred_errors=self._can_defer()):
            return False
        if getattr(self.optimizer, "clip_and_step", None) is None and not all(g.get("capturable", False) for g in self.optimizer.param_groups):
            return False
        red = self.grad_reducer
        return red is None or not red.exchange or red.backend == "rccl"

    def _can_defer(self) -> bool:
        """deferred error words need an optimizer pass that honours the status word (cvc.optim.ClipAdam) and, with an exchange, a
        transport that can carry the word inside the step (the package's RCCL communicator)"""
        red = self.grad_reducer
        return getattr(self.optimizer, "clip_and_step", None) is not None and self.device.type == "cuda" and \
            (red is None or not red.exchange or red.backend == "rccl")

    def _needs_deferral(self) -> bool:
        need = getattr(self.model, "reports_error_words", None)
        return bool(need is not None and need())

    def deferred_errors(self):
        """Context manager: error words of the model's persistent kernels go to the device's status word instead of being read by
        the host (train() uses it whenever it replays graphs over a model that has such kernels; bench.py for the same step)."""
        import contextlib
        from . import hip

        @contextlib.contextmanager
        def cm():
            if not (self._needs_deferral() and self._can_defer()):
                yield False
                return
            self._status = hip.step_status(self.device)
            self._status.zero_()
            hip.defer_errors(self._status)
            try:
                yield True
            finally:
                hip.defer_errors(None)
                self._status = None
        return cm()

    def rerun_void_steps(self, batches):
        """The steps of `batches` (prepared, on the device) were void: some persistent launch reported a barrier time-out, the
        optimizer pass left the parameters alone.  They are taken again here, eagerly, on the per-step forms (which have no barrier)
        with host-checked error words.  Every rank of a multi-GPU run calls this with the same number of batches (the status word
        travels with the gradient exchange).  Returns the five loss values of each re-run step."""
        from . import gru, hip, lstm_seq
        hip.warn_once("trainer.void-steps", "a persistent recurrence kernel reported a barrier time-out inside a captured training step; "
                      "the step left the parameters untouched and is re-run on the per-step forms (reported once; counts in "
                      "Trainer.deferred_stats)")
        keep = (gru.PERSISTENT, gru.BWD_PERSISTENT, self._status)
        keep_lstm = lstm_seq.PERSISTENT
        hip.defer_errors(None)
        gru.PERSISTENT = gru.BWD_PERSISTENT = lstm_seq.PERSISTENT = False
        self._status = None
        out = []
        try:
            for b in batches:
                out.append(torch.stack([x.reshape(()) for x in self.train_step_prepared(b)]))
                self.deferred_stats["rerun_steps"] += 1
        finally:
            gru.PERSISTENT, gru.BWD_PERSISTENT, self._status = keep
            lstm_seq.PERSISTENT = keep_lstm
            if self._status is not None:
                hip.defer_errors(self._status)
        return out

    def train_step_bucketed(self, b):
        """One optimisation step on a prepared batch, replayed from the HIP graph of its shape when there is one.  A shape's first
        occurrence runs eagerly -- that IS the training step, and it is the warm-up the capture needs (allocator, lazy workspaces);
        the very first steps of a run are eager whatever their shape (the reducer learns and compacts its arenas on step one, the
        optimizer builds its segment table on step two).  From its second occurrence on a shape is captured once (capturing runs
        nothing) and replayed.  Eager and replayed steps are the same launches on the same buffers: bit-identical results.
        Returns [loss, lm, att2, cls, recon] on the device (static for replayed steps: read or clone before the next step)."""
        key = _shape_key(b)
        if self._side is None:
            # ONE stream for eager steps, captures and replays; the reducer's gradient accumulators are re-created under it (a node
            # made under another stream would fork every backward pass -- and every captured graph -- once per parameter)
            self._side = torch.cuda.Stream(self.device)
            if self.grad_reducer is not None:
                self.grad_reducer.bind_stream(self._side)
        ent = self._graphs.get(key)
        if ent is None and (self._graph_broken or self._eager_steps < 2 or self._shape_seen.get(key, 0) < 1):
            cur = torch.cuda.current_stream()
            self._side.wait_stream(cur)
            with torch.cuda.stream(self._side):
                res = self._core_step(b)
            cur.wait_stream(self._side)
            res.record_stream(cur)
            for v in b.values():                     # the batch's tensors were used on the side stream: allocator ownership
                for t_ in (v.values() if isinstance(v, dict) else (v,)):
                    if isinstance(t_, torch.Tensor) and t_.is_cuda:
                        t_.record_stream(self._side)
            self._eager_steps += 1
            self._shape_seen[key] = self._shape_seen.get(key, 0) + 1
            self.graph_stats["eager"] += 1
            self._weights_changed()
            return res
        if ent is None:
            self._check_capturable()
            static = {k: (v.clone() if isinstance(v, torch.Tensor) else ({kk: vv.clone() for kk, vv in v.items()} if isinstance(v, dict) else v))
                      for k, v in b.items()}
            torch.cuda.current_stream().synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                # (every shape's graph allocates from its OWN private pool: graphs replay in data-dependent order, and PyTorch only
                # guarantees a shared pool for graphs replayed in capture order -- a later graph's intermediates could alias an
                # earlier graph's static result.  288 GB of HBM pay for one live set per shape, at most 16 shapes)
                with torch.cuda.graph(g, stream=self._side, capture_error_mode=self._capture_mode()):
                    res = self._core_step(static)
            except Exception as ex:      # noqa: BLE001 -- a model whose step cannot be captured (a host read inside the forward, a
                # library fallback that allocates) trains eagerly from here on; said once, loudly
                from . import hip
                hip.warn_once("trainer.capture", f"the training step could not be captured into a HIP graph ({type(ex).__name__}: "
                              f"{str(ex)[:300]}); training continues with eager steps")
                self._graph_broken = True
                torch.cuda.synchronize()
                if self.grad_reducer is not None:
                    self.grad_reducer.zero_grad()
                else:
                    self.optimizer.zero_grad(set_to_none=False)
                return self.train_step_bucketed(b)
            ent = self._graphs[key] = (g, static, res)
            self.graph_stats["captured"] += 1
        g, static, res = ent
        _copy_into(static, b)
        sync = getattr(self.optimizer, "sync_hyperparameters", None)
        if sync is not None:
            sync()
        g.replay()
        self.graph_stats["replayed"] += 1
        self._weights_changed()
        return res

    # ------------------------------------------------------------------ epoch loops
    def train(self, epoch, tb_logger=None):
        meters = {k: AverageMeter() for k in ("batch", "data", "lm", "attn", "cls", "recon", "reward", "sampled", "nll", "entropy", "kd")}
        self.model.train()
        end = time.time()
        n_steps = len(self.train_loader) - 1                 # the reference drops the last batch (:55)
        scst = self.scst_after >= 0 and epoch >= self.scst_after     # self-critical epochs: eager steps (scst_step_prepared)
        # scheduled-sampling epochs (model.ss_prob > 0, set per epoch by cvc.main): eager steps with a rollout in front
        ss = not scst and float(getattr(getattr(self.model, "module", self.model), "ss_prob", 0.0)) > 0
        # distilled epochs (model.distill set; not the self-critical ones): eager steps with the teacher's pass in front, two more
        # elements at the end of every step's result: the unmixed NLL and the KD
        kd = not scst and self._distilling()
        graphed = self.graph_capable() and not scst and not ss and not kd
        smooth = (self.label_smoothing > 0 or kd) and not scst       # (a last element of every step's result: the unsmoothed NLL)
        ent = (self.scst_entropy if scst else self.confidence_penalty) is not None     # (the very last element: the mean entropy)
        i_nll = -2 if (ent or kd) else -1
        self._active_buckets = self.shape_buckets if graphed else 0       # (read by _prepare, which the prefetcher calls)
        # batch k+1 is staged into HBM on a side stream while step k runs
        batches = DevicePrefetcher(self.train_loader, lambda raw: self._prepare(raw, True), self.device, limit=n_steps)
        if self.opts.att_model != 'cyclical':
            raise ValueError('Unknown att_model: {}'.format(self.opts.att_model))
        n = self.opts.batch_size * self.opts.seq_per_img
        acc, pending, last = None, 0, None           # device-side sums of [loss, lm, att2, cls, recon (, void)] since the last read-back
        kept = []                                    # deferred error words: the interval's prepared batches (a void step is re-run)
        KEEP_MAX = 16                                # ... at most this many are held (377 MB each at config-2 size), then a read-back
        void_flags = None

        def flush():
            """ONE host read per display interval (the reference reads four scalars per step, trainer.py:124-135): the meters get
            the interval's means with the interval's weight, `.val` the latest step's values.  Deferred error words: the same read
            tells which steps of the interval were void; they are re-run now and their losses join the interval's sums."""
            nonlocal acc, pending
            if acc is None:
                return
            if deferred:
                width = last.numel()
                sums, cur, flags = torch.cat([acc, last, void_flags[:pending]]).split([width, width, pending])
                sums, cur, flags = sums.tolist(), cur.tolist(), flags.tolist()
                void = [i for i, f in enumerate(flags) if f != 0]
                if void:
                    self.deferred_stats["void_steps"] += len(void)
                    for r in self.rerun_void_steps([kept[i] for i in void]):
                        r = r.tolist()
                        sums[:5] = [a + b_ for a, b_ in zip(sums[:5], r[:5])]
                        if smooth:
                            sums[i_nll] += r[i_nll]
                        if ent:
                            sums[-1] += r[-1]
                        if void[-1] == pending - 1:
                            cur[:5] = r[:5]
                            if smooth:
                                cur[i_nll] = r[i_nll]
                            if ent:
                                cur[-1] = r[-1]
                kept.clear()
            else:
                sums, cur = torch.stack([acc, last]).tolist()
            if scst:                                  # (a sixth element: the step's mean reward)
                meters["reward"].update(sums[5] / pending, n * pending)
                meters["reward"].val = cur[5]
                self.reward_history.setdefault(epoch, []).append(sums[5] / pending)
            if ss:                                    # (a sixth element: the share of loop A's inputs that were sampled words)
                meters["sampled"].update(sums[5] / pending, n * pending)
                meters["sampled"].val = cur[5]
            if smooth:                                # (the last element: loop A's unsmoothed mean NLL beside the smoothed LM loss)
                meters["nll"].update(sums[i_nll] / pending, n * pending)
                meters["nll"].val = cur[i_nll]
                self.nll_history.setdefault(epoch, []).append(sums[i_nll] / pending)
            if ent:                                   # (the very last element: the mean entropy of the word distribution)
                meters["entropy"].update(sums[-1] / pending, n * pending)
                meters["entropy"].val = cur[-1]
                self.entropy_history.setdefault(epoch, []).append(sums[-1] / pending)
            if kd:                                    # (the very last element: loop A's mean tau^2 KL(teacher || student))
                meters["kd"].update(sums[-1] / pending, n * pending)
                meters["kd"].val = cur[-1]
                self.kd_history.setdefault(epoch, []).append(sums[-1] / pending)
            for name, i in (("lm", 1), ("attn", 2), ("cls", 3), ("recon", 4)):
                meters[name].update(sums[i] / pending, n * pending)
                meters[name].val = cur[i]
            acc, pending = None, 0

        step = -1
        import contextlib
        with (self.deferred_errors() if graphed else contextlib.nullcontext(False)) as deferred:
            if deferred:
                void_flags = torch.zeros(KEEP_MAX, device=self.device)
            for step, b in enumerate(batches):
                meters["data"].update(time.time() - end)
                if scst:
                    # the meters' "LM Loss" is the self-critical loss; the attention / class / reconstruction terms take no part
                    s_loss, s_reward, _s_base, _s_adv = self.scst_step_prepared(b)
                    zero = torch.zeros((), device=s_loss.device)
                    res = torch.stack([s_loss, s_loss, zero, zero, zero, s_reward.to(s_loss.dtype)] +
                                      ([self.last_scst["entropy"].to(s_loss.dtype).reshape(())] if ent else []))
                elif graphed:
                    res = self.train_step_bucketed(b)
                elif ss:                          # (a sixth element: the step's share of sampled inputs)
                    vals = [x.reshape(()) for x in self.train_step_prepared(b)]
                    res = torch.stack(vals[:5] + [self.last_ss["share"].to(torch.float32)] + vals[5:])
                else:
                    res = torch.stack([x.reshape(()) for x in self.train_step_prepared(b)])
                acc = res.clone() if acc is None else acc.add_(res)
                if deferred:
                    void_flags[pending:pending + 1].copy_(res[5:6])
                    kept.append(b)
                last, pending = res, pending + 1
                if step % self.opts.disp_interval == 0:
                    flush()
                    meters["batch"].update((time.time() - end))
                    print('Epoch: [{0}][{1}/{2}]\tTime {b.val:.3f} ({b.avg:.3f})\tData {d.val:.3f} ({d.avg:.3f})\t'
                          'LM Loss {l.val:.4f} ({l.avg:.4f})\tAttn Loss {a.val:.4f} ({a.avg:.4f})\t'
                          'Cls Loss {c.val:.4f} ({c.avg:.4f})\tRecon Loss {r.val:.4f} ({r.avg:.4f})'.format(
                              epoch, step, n_steps, b=meters["batch"], d=meters["data"], l=meters["lm"], a=meters["attn"],
                              c=meters["cls"], r=meters["recon"]) +
                          ('\tReward {r.val:.4f} ({r.avg:.4f})'.format(r=meters["reward"]) if scst else '') +
                          ('\tSampled {s.val:.3f} ({s.avg:.3f})'.format(s=meters["sampled"]) if ss else '') +
                          ('\tNLL {s.val:.4f} ({s.avg:.4f})'.format(s=meters["nll"]) if smooth else '') +
                          ('\tH {s.val:.4f} ({s.avg:.4f})'.format(s=meters["entropy"]) if ent else '') +
                          ('\tKD {s.val:.4f} ({s.avg:.4f})'.format(s=meters["kd"]) if kd else ''))
                else:
                    if deferred and pending >= KEEP_MAX:
                        flush()
                    meters["batch"].update(time.time() - end)      # (launch time of an asynchronous step; display steps include the wait)
                end = time.time()
            flush()
        if tb_logger:
            tb_logger.add_scalar('train/learning_rate', self.optimizer.param_groups[0]['lr'], epoch)
            tb_logger.add_scalar('train/lm_loss', meters["lm"].avg, epoch)
            tb_logger.add_scalar('train/attn_loss', meters["attn"].avg, epoch)
            tb_logger.add_scalar('train/cls_loss', meters["cls"].avg, epoch)
            tb_logger.add_scalar('train/lm_recon_loss', meters["recon"].avg, epoch)
            if scst:
                tb_logger.add_scalar('train/scst_reward', meters["reward"].avg, epoch)
            if smooth:
                tb_logger.add_scalar('train/lm_nll', meters["nll"].avg, epoch)
            if ent:
                tb_logger.add_scalar('train/entropy', meters["entropy"].avg, epoch)
            if kd:
                tb_logger.add_scalar('train/kd', meters["kd"].avg, epoch)

    def _segment_timestamps(self):
        """{video: {segment: [start, end]}} of the validation segments: the reference reads them from the ANet-Entities
        annotation file `opts.grd_reference` (trainer.py:162) as ['annotations'][vid]['segments'][seg]['timestamps']; a
        dataset object may carry the same structure as `dataset.grd_reference` (the synthetic stand-in does)."""
        if getattr(self, "_timestamps", None) is None:
            src = getattr(self.dataset, "grd_reference", None)
            if src is None:
                path = getattr(self.opts, "grd_reference", None)
                if not path or not os.path.isfile(path):
                    raise FileNotFoundError(
                        f"eval needs the segment timestamps (opts.grd_reference = {path!r}, reference trainer.py:162): the "
                        "densecap file the ANETcaptions evaluator reads carries a 'timestamp' per predicted segment")
                with open(path) as f:
                    src = json.load(f)
            self._timestamps = src['annotations']
        return self._timestamps

    @_averaged_by_default
    def eval(self, epoch, tb_logger=None):
        """Greedy (or beam) decode of the validation split -> predictions in the densecap JSON
        layout (trainer.py:254-286: {'sentence', 'timestamp': [start, end]} per segment) -> optional external scorer.
        With the model's consensus switch on (opts.consensus = samples / beam) every clip's caption is the consensus pick among its
        candidates (model._sample), with that candidate's attention rows: the densecap file, the device metrics and the grounding
        all see the picked caption."""
        self.model.eval()
        core = self._decoder()
        core.eval()
        if getattr(core, "consensus", "off") != "off":
            self._consensus_table(core)
        predictions = defaultdict(list)
        grd_output = defaultdict(dict)
        o = self.opts
        ds = self.dataset
        timestamps = self._segment_timestamps()
        dev_scorer = self._device_scorer() if (self.device_metrics and o.val_split != 'hidden_test') else None
        # the grounding scores of the generated captions (cvc.metrics.GroundingScorer): only with the device metrics AND
        # --eval_obj_grounding; the grounding file then is built from the kernel's picks
        grd_scorer = self._grounding_scorer() if (dev_scorer is not None and getattr(o, "eval_obj_grounding", False)) else None
        div_scorer = None
        if self.val_diversity:
            if dev_scorer is None or getattr(core, "consensus", "off") == "off":
                raise RuntimeError("Trainer.eval: val_diversity needs device_metrics=True and the model's consensus switch on (samples / "
                                   "beam): the candidates it scores are those of the consensus selection")
            from .metrics import DiversityScorer
            div_scorer = DiversityScorer()
        spec_scorer = None
        if div_scorer is not None and self.val_self_cider:
            from .metrics import SpectrumScorer
            spec_scorer = SpectrumScorer(self._val_cider)
        with torch.no_grad():
            for b in DevicePrefetcher(self.val_loader, lambda raw: self._prepare(raw, False), self.device):
                seq, att2_weights, _ = self._call(b, True)
                if dev_scorer is not None:                  # the references scst_step_prepared scores against; no host read
                    T = seq.size(1)
                    dev_scorer.add(seq.contiguous(), b["gt_seqs"][:, :, :T].contiguous(), b["num"][:, 0].to(torch.int32))
                    if div_scorer is not None:              # the candidates the consensus pick was chosen among; no host read
                        last = core.last_consensus
                        cand = last["candidates"]
                        per = cand.size(0) // seq.size(0) if cand.dim() == 2 else cand.size(1)
                        div_scorer.add(cand.reshape(-1, cand.size(-1)), per, None if last.get("live") is None else last["live"].reshape(-1),
                                       b["gt_seqs"][:, :, :T].contiguous(), b["num"][:, 0].to(torch.int32), self._val_cider)
                        if spec_scorer is not None:         # the same sets and live mask; no host read
                            spec_scorer.add(cand.reshape(-1, cand.size(-1)), per, None if last.get("live") is None else last["live"].reshape(-1))
                if getattr(o, "eval_obj_grounding", False):
                    assert o.beam_size == 1, 'only support beam_size is 1'
                    if grd_scorer is not None:
                        self._collect_grounding_device(b, seq, att2_weights, grd_scorer, grd_output)
                    else:
                        self._collect_grounding(b, seq, att2_weights, grd_output)
                sents = utils.decode_sequence(ds.itow, getattr(ds, "itod", None), getattr(ds, "ltow", None),
                                              getattr(ds, "itoc", None), getattr(ds, "wtod", None), seq.data, o.vocab_size, o)
                for k, sent in enumerate(sents):
                    vid_idx, entry = densecap_entry(sent, b["seg_id"][k], timestamps)
                    predictions[vid_idx].append(entry)
        # every rank decoded its shard of the clips; merge host-side, rank 0 writes the files and scores
        predictions, grd_output = gather_eval_outputs(predictions, grd_output)
        lang_stats = {}
        if dev_scorer is not None:                          # (every rank: its sums are merged like the predictions)
            lang_stats = self._merged_device_metrics(dev_scorer)
        if grd_scorer is not None:
            lang_stats = {**lang_stats, **self._merged_grounding(grd_scorer)}
        if div_scorer is not None:                          # ONE read per validation pass
            res = self._merged_diversity(div_scorer)
            lang_stats = {**lang_stats, **{k: res[k] for k in ("Div_1", "Div_2", "mBLEU_4", "Unique", "oracle_CIDEr") if k in res}}
        if spec_scorer is not None:                         # ONE read per validation pass
            res = self._merged_spectrum(spec_scorer)
            lang_stats = {**lang_stats, "Self_CIDEr": res["Self_CIDEr"], "LSA": res["LSA"]}
        if getattr(o, "eval_obj_grounding_gt", False):        # (every rank: its shards are merged like the predictions)
            self._eval_ground_gt(epoch, tb_logger)
        self.submission_file = self.attn_file = None
        self.predictions = predictions
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_rank() != 0:
            return lang_stats
        if getattr(o, "language_eval", False) and o.val_split != 'hidden_test':
            self.submission_file = write_densecap_json(predictions, o)
        if getattr(o, "eval_obj_grounding", False):
            self.attn_file = write_grounding_json(grd_output, o)
        if self.scorer is not None:
            lang_stats = {**lang_stats, **(self.scorer(predictions, grd_output, o) or {})}      # an external scorer's keys win
        if tb_logger:
            for k, v in lang_stats.items():
                tb_logger.add_scalar('eval/' + k, v, epoch)
        self.predictions = predictions
        return lang_stats

    def _device_scorer(self):
        """a fresh cvc.metrics.DeviceScorer over the CIDEr-D table of the validation loader's own captions (document frequencies
        over the evaluated split, as the toolkits take them); the table is built once, at the first eval"""
        from .cider import CiderD
        from .metrics import DeviceScorer
        if self._val_cider is None:
            self._val_cider = CiderD.from_dataset(self.val_loader.dataset, self.device)
        return DeviceScorer(self._val_cider)

    @staticmethod
    def _merged_device_metrics(dev_scorer):
        """one host read of this rank's sums; with several ranks the sums are exchanged host-side, next to gather_eval_outputs, and
        added in rank order on every rank (more than one rank: untested)"""
        import torch.distributed as dist
        from .metrics import result_from_sums
        mine = dev_scorer.sums()
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return result_from_sums(*mine)
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, mine)
        stats = [sum(p[0][i] for p in parts) for i in range(10)]
        return result_from_sums(stats, *(sum(p[j] for p in parts) for j in (1, 2, 3)))

    @staticmethod
    def _merged_diversity(div_scorer):
        """one host read of this rank's sums; with several ranks the sums are exchanged host-side and added on every rank, as
        _merged_device_metrics does (more than one rank: untested)"""
        import torch.distributed as dist
        from .metrics import diversity_from_sums
        mine = div_scorer.sums()
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return diversity_from_sums(*mine)
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, mine)
        return diversity_from_sums([sum(p[0][i] for p in parts) for i in range(13)], [sum(p[1][i] for p in parts) for i in range(7)])

    @staticmethod
    def _merged_spectrum(spec_scorer):
        """one host read of this rank's sums; with several ranks the sums are exchanged host-side and merged through add_sums on
        every rank, in rank order (more than one rank: untested)"""
        import torch.distributed as dist
        from .metrics import SpectrumScorer, spectrum_from_sums
        mine = spec_scorer.sums()
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return spectrum_from_sums(mine)
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, mine)
        merged = SpectrumScorer()
        for p in parts:
            merged.add_sums(p)
        return merged.result()

    def _grounding_scorer(self):
        """a fresh cvc.metrics.GroundingScorer; the word -> detection class table is built once, at the first eval"""
        from .metrics import GroundingScorer
        o = self.opts
        if self._word_cls is None:
            self._word_cls = utils.word_class_table(o).to(self.device)
        return GroundingScorer(self._word_cls, len(o.itod), o.num_sampled_frm, o.num_prop_per_frm)

    @staticmethod
    def _merged_grounding(grd_scorer):
        """one host read of this rank's per-class table; with several ranks the tables are exchanged host-side and added on every
        rank, as _merged_device_metrics does with its sums (more than one rank: untested)"""
        import torch.distributed as dist
        from .metrics import grounding_result
        mine = grd_scorer.sums()
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return grounding_result(mine)
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, mine)
        return grounding_result(sum(parts[1:], parts[0]))

    def _eval_ground_gt(self, epoch, tb_logger):
        """eval's --eval_obj_grounding_gt part: grounding on the GT sentences, kept as self.grounding_gt_stats and logged under
        grounding_gt/ -- never merged into eval's lang_stats (the LR schedule and the best-score logic read those)."""
        self.grounding_gt_stats = self.ground_gt()
        if tb_logger and self.grounding_gt_stats:
            for k, v in self.grounding_gt_stats.items():
                tb_logger.add_scalar('grounding_gt/' + k, v, epoch)

    def _val_batches(self):
        """the validation split's batches as eval prepares them, with the proposal axis of the frame mask trimmed like the proposals
        (what the label glue of a teacher-forced pass reads; _prepare trims it for training batches only)"""
        for b in DevicePrefetcher(self.val_loader, lambda raw: self._prepare(raw, False), self.device):
            n_prop = b["ppls"].size(1)
            if b["mask_frms"].size(1) != n_prop:
                b["mask_frms"] = b["mask_frms"][:, :n_prop].contiguous()
            yield b

    def _full_proposal_axis(self, ppls, weights):
        """an evaluation batch is trimmed to its largest proposal count (_prepare); the per-frame box gather wants all
        num_sampled_frm x num_prop_per_frm slots: the missing ones are zero boxes that no word attends to"""
        full = self.opts.num_sampled_frm * self.opts.num_prop_per_frm
        pad = full - ppls.size(1)
        if pad <= 0:
            return ppls, weights
        return (torch.nn.functional.pad(ppls, (0, 0, 0, pad)), torch.nn.functional.pad(weights, (0, pad), value=float("-inf")))

    def _score_call(self, model, b, **kw):
        return model.score(b["segs_feat"], b["input_seqs"], b["gt_seqs"], b["num"], b["ppls"], b["gt_bboxs"], b["mask_bboxs"],
                           b["ppls_feat"], b["mask_frms"], b["sample_idx"], b["pnt_mask"], **kw)

    @_averaged_by_default
    def score(self, stem: str = None):
        """Teacher-forced scoring of the validation split's GT captions (model.score: the decode engine's forced mode).
        Writes <results_dir>/<stem>_scores.json (rank 0, after the merge of the ranks' shards, as sample does; stem defaults to
        densecap-<val_split>-<id>):  {video: [{"segment", "timestamp", "logprob": sum of the caption's log-probs over its masked
        steps, "words": the number of those steps, "top1": how many of them have the given word as the model's arg-max}]}
        Returns {"ppl": exp(-sum logprob / sum words), "top1": sum top1 / sum words} over the first caption of every segment."""
        model = self._decoder()
        o = self.opts
        timestamps = self._segment_timestamps()
        scores = defaultdict(list)
        for b in self._val_batches():
            out = self._score_call(model, b)
            n = out["logprob"].size(0) // len(b["seg_id"])
            mask = out["mask"]
            lp, nw = out["seq_logprob"].tolist(), mask.sum(1).tolist()
            top1 = ((out["rank"] == 0) & mask).sum(1).tolist()
            for k, seg_id in enumerate(b["seg_id"]):
                vid_idx, entry = densecap_entry("", seg_id, timestamps)
                scores[vid_idx].append({"segment": entry["segment"], "timestamp": entry["timestamp"], "logprob": lp[k * n],
                                        "words": nw[k * n], "top1": top1[k * n]})
        scores, _ = gather_eval_outputs(scores, {})
        self.scores = scores
        tot = [sum(e[key] for segs in scores.values() for e in segs) for key in ("logprob", "words", "top1")]
        stats = {"ppl": float(np.exp(-tot[0] / max(tot[1], 1))), "top1": tot[2] / max(tot[1], 1)}
        if not (torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_rank() != 0):
            d = getattr(o, "results_dir", "results")
            os.makedirs(d, exist_ok=True)
            self.scores_file = os.path.join(d, (stem or "densecap-%s-%s" % (o.val_split, o.id)) + "_scores.json")
            with open(self.scores_file, "w") as f:
                json.dump(scores, f)
        return stats

    @_averaged_by_default
    def ground_gt(self, stem: str = None):
        """Grounding on the GT sentences (--eval_obj_grounding_gt; the reference parses the flag and raises NotImplementedError,
        trainer.py:352-353): model.score(grounding=True) over the validation split, then per annotated object word the proposal
        with the largest weight among those that are not frame-masked -- once by the decoder's frame-masked region attention
        (att2_weights -> box_accu_att), once by the grounder (ground_weights -> box_accu_grd); a hit is a proposal that overlaps one
        of the word's boxes (roi_labels).  Writes attn-gt-sent-results-<split>-<id>.json and grd-gt-sent-results-<split>-<id>.json
        (write_grounding_json's layout, 'eval_mode': 'GT'; a stem replaces the first part of both names) and returns the two
        accuracies, their per-class means and the number of annotated object words."""
        model = self._decoder()                     # (an ensemble refuses grounding=True: the frame-masked scores are one member's)
        o = self.opts
        records = defaultdict(list)
        grd_att, grd_grd = defaultdict(dict), defaultdict(dict)
        for b in self._val_batches():
            out = self._score_call(model, b, grounding=True)
            T = out["att2_weights"].size(1)
            cls = (b["input_seqs"][:, 0, 1:T + 1, 0] - o.vocab_size)
            annotated = (~b["mask_bboxs"][:, 0, :, 1:T + 1].bool()).any(1)                       # [B, T]
            counted = (cls >= 1) & annotated
            hits = [ground_picks(out[k], out["frm_mask_output"], out["roi_labels"])[1] for k in ("att2_weights", "ground_weights")]
            sel = counted.nonzero().tolist()
            cls_l, ha, hg = cls.tolist(), hits[0].tolist(), hits[1].tolist()
            records["words"].extend((cls_l[i][t], ha[i][t], hg[i][t]) for i, t in sel)
            gt_words = b["gt_seqs"][:, 0].tolist()
            obj = (cls >= 1).tolist()
            for key, dst in (("att2_weights", grd_att), ("ground_weights", grd_grd)):
                boxes_l = self._frame_boxes(*self._full_proposal_axis(b["ppls"], out[key]))[..., :4].tolist()
                for i, seg_id in enumerate(b["seg_id"]):
                    vid_id, seg_idx = seg_id.split('_segment_')
                    res = {'clss': [], 'idx_in_sent': [], 'bbox_for_all_frames': []}
                    for j, w in enumerate(gt_words[i][:T]):
                        if w == 0:
                            break
                        if obj[i][j]:
                            res['bbox_for_all_frames'].append(boxes_l[i][j])
                            res['clss'].append(o.itod[cls_l[i][j]])
                            res['idx_in_sent'].append(j)
                    dst[vid_id][str(int(seg_idx))] = res
        records, grd_att = gather_eval_outputs(records, grd_att)
        _, grd_grd = gather_eval_outputs({}, grd_grd)
        stats = ground_accuracy(records.get("words", []))
        self.grounding_gt = (grd_att, grd_grd)
        self.grounding_gt_files = None
        if not (torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_rank() != 0):
            self.grounding_gt_files = (write_grounding_json(grd_att, o, stem=(stem or 'attn') + '-gt-sent-results', eval_mode='GT'),
                                       write_grounding_json(grd_grd, o, stem=(stem or 'grd') + '-gt-sent-results', eval_mode='GT'))
        return stats

    @_averaged_by_default
    def sample(self, n: int, temperature: float, seed: int = 0, stem: str = None, top_k: int = 0, top_p: float = 1.0,
               constraints: dict = None, consensus: bool = False, without_replacement: bool = False, diversity: bool = False,
               self_cider: bool = False):
        """Sampled decode of the validation split: n captions per segment, every word drawn from softmax(logits / temperature)
        without UNK (DecodeEngine's sampling mode; the engine is seeded once with `seed`, later batches draw fresh noise);
        top_k / top_p truncate that distribution (0 / 1.0 = off; the log-probs stay the model's, over the full vocabulary).
        constraints: keyword arguments of model._sample's constrained decoding (no_repeat_ngram, no_immediate_repeat, min_len,
        ban_words, bad_endings); what is not given is the model's attribute, i.e. the run's options -- as in eval().
        Writes <results_dir>/<stem>_samples.json (rank 0, as eval does; stem defaults to densecap-<val_split>-<id>):
            {video: [{"segment": seg_idx, "timestamp": [start, end], "sentences": [n], "logprobs": [n]}]}
        logprobs[j]: the sum of the log-probs of sample j's words up to and including its first EOS (all T steps without one).
        consensus=True (n > 1): every entry also holds "consensus": the index of the consensus pick among its n sentences, and
        "utilities": [n], each sentence's CIDEr-D against the segment's other samples over the training captions' table
        (cvc.cider.CiderD.consensus); the last batch's device tensors stay in model.last_consensus.
        without_replacement=True (n > 1): the n captions of a segment are drawn WITHOUT replacement by stochastic beam search
        (model._sample(beam_size=n, stochastic_beam=True, stochastic_tau=temperature)): pairwise distinct, in draw order, the first
        an ordinary sample.  "logprobs" is then each caption's model log-prob as the beam carries it (the same sum), and every entry
        also holds "logq": [n], the captions' log-probs under the sampling distribution q_tau, and "G": [n], their perturbed keys
        (non-increasing).  top_k / top_p are refused with it; the constraints and consensus work.
        diversity=True (n > 1): every entry also holds "diversity": {"div1", "div2", "mbleu4", "unique"} of its n sentences
        (cvc.metrics.set_diversity: distinct 1- and 2-grams over the set's word count, the corpus BLEU-4 of each sentence against the
        others, the number of different sentences), and the file gains the top-level key "diversity": the split's summary
        (cvc.metrics.DiversityScorer.result(), with oracle_CIDEr and mean_CIDEr against the validation references), which is also
        logged and kept in self.sample_diversity.  Off: the file is what it was.
        self_cider=True (with diversity=True): every entry's "diversity" gains "selfcider" and "lsa" -- the set's Self-CIDEr over the
        validation captions' table and its LSA diversity (cvc.metrics.set_spectrum, score 0 in mode cider and score 1 in mode lsa) --
        and the summary gains Self_CIDEr and LSA (cvc.metrics.SpectrumScorer.result()).  Off: the file is what it was.
        Returns the path (None on the other ranks)."""
        model = self._decoder()
        n = int(n)
        if diversity and n < 2:
            raise RuntimeError(f"Trainer.sample: diversity is that of a set of n > 1 captions per segment, got n = {n}")
        if self_cider and not diversity:
            raise RuntimeError("Trainer.sample: self_cider adds to the diversity of every set -- it needs diversity=True")
        model.eval()
        o, ds = self.opts, self.dataset
        timestamps = self._segment_timestamps()
        samples = defaultdict(list)
        div_scorer = None
        if diversity:
            from .metrics import DiversityScorer, corpus_bleu
            div_scorer = DiversityScorer()
            self._device_scorer()                           # (builds the validation captions' CIDEr-D table once)
        spec_scorer = None
        if self_cider:
            from .metrics import SpectrumScorer
            spec_scorer = SpectrumScorer(self._val_cider)
        if without_replacement:
            if n < 2:
                raise RuntimeError(f"Trainer.sample: without_replacement draws n > 1 distinct captions per segment, got n = {n}")
            if top_k != 0 or top_p != 1.0:
                raise RuntimeError("Trainer.sample: without_replacement is refused with top_k / top_p (stochastic beam search samples "
                                   "the untruncated distribution)")
        if consensus:
            if n < 2:
                raise RuntimeError(f"Trainer.sample: consensus selection needs n > 1 samples per segment, got n = {n}")
            self._consensus_table(model)
        with torch.no_grad():
            for b in DevicePrefetcher(self.val_loader, lambda raw: self._prepare(raw, False), self.device):
                args = (b["segs_feat"], b["input_seqs"], b["ppls"], b["gt_seqs"], b["num"], b["mask_bboxs"], b["gt_bboxs"],
                        b["ppls_feat"], b["mask_frms"], b["sample_idx"], b["pnt_mask"])
                if without_replacement:
                    model._sample(*args, beam_size=n, sample_max=1, stochastic_beam=True, stochastic_tau=temperature, seed=seed,
                                  consensus=False, beam_groups=1, diversity_lambda=0.0, length_penalty=0.0, **(constraints or {}))
                    draws = model.last_stochastic
                    seq, logprob = draws["seq"].reshape(-1, draws["seq"].size(2)), None
                else:
                    seq, _, logprob = model._sample(*args, sample_max=0, temperature=temperature, sample_n=n, seed=seed, top_k=top_k,
                                                    top_p=top_p, consensus=False, **(constraints or {}))
                if consensus:
                    from . import metrics as cvc_metrics
                    mix = getattr(model, "consensus_utility", None)
                    if cvc_metrics.is_cider_only(mix):
                        utility, pick, _ = model.consensus_table.consensus(seq, n)
                    else:                                   # the model's utility mix (--consensus_utility), uniform over the draws
                        picked = cvc_metrics.consensus(seq, n, mix, model.consensus_table)
                        utility, pick = picked["utility"], picked["pick"]
                    model.last_consensus = dict(candidates=seq, pick=pick, utility=utility)
                    picks, utils_ = pick.tolist(), utility.view(-1, n).tolist()
                if diversity:                               # a stochastic beam's fillers (score -inf) are no captions
                    live = torch.isfinite(draws["score"]).reshape(-1) if without_replacement else None
                    T = seq.size(1)
                    dv = div_scorer.add(seq.contiguous(), n, live, b["gt_seqs"][:, :, :T].contiguous(), b["num"][:, 0].to(torch.int32),
                                        self._val_cider)
                    div_l = dv["div"].tolist()
                    set_l = dv["stats"].tolist()
                    mb_l = dv["mbleu_stats"].view(-1, n, 10).sum(1).tolist()
                    if spec_scorer is not None:
                        sp = spec_scorer.add(seq.contiguous(), n, live)
                        sc_l, lsa_l = sp["cider"]["score"][:, 0].tolist(), sp["lsa"]["score"][:, 1].tolist()
                sents = utils.decode_sequence(ds.itow, getattr(ds, "itod", None), getattr(ds, "ltow", None),
                                              getattr(ds, "itoc", None), getattr(ds, "wtod", None), seq.data, o.vocab_size, o)
                # sequence log-prob: the steps up to and including the first EOS (word 0)
                ended = torch.cumsum((seq == 0).to(torch.int32), 1) - (seq == 0).to(torch.int32)
                if without_replacement:
                    seq_lp, seq_lq, seq_G = (draws[k].reshape(-1).tolist() for k in ("score", "logq", "G"))
                else:
                    seq_lp = (logprob * (ended == 0).to(logprob.dtype)).sum(1).tolist()
                for k, seg_id in enumerate(b["seg_id"]):
                    vid_idx, entry = densecap_entry(sents[k * n], seg_id, timestamps)
                    samples[vid_idx].append({"segment": entry["segment"], "timestamp": entry["timestamp"],
                                             "sentences": sents[k * n:(k + 1) * n], "logprobs": seq_lp[k * n:(k + 1) * n]})
                    if without_replacement:
                        samples[vid_idx][-1].update(logq=seq_lq[k * n:(k + 1) * n], G=seq_G[k * n:(k + 1) * n])
                    if consensus:
                        samples[vid_idx][-1].update(consensus=picks[k], utilities=utils_[k])
                    if diversity:
                        samples[vid_idx][-1]["diversity"] = {"div1": div_l[k][0], "div2": div_l[k][1],
                                                             "mbleu4": float(corpus_bleu(mb_l[k])[3]), "unique": set_l[k][9]}
                        if spec_scorer is not None:
                            samples[vid_idx][-1]["diversity"].update(selfcider=sc_l[k], lsa=lsa_l[k])
        samples, _ = gather_eval_outputs(samples, {})
        self.samples = samples
        if diversity:
            self.sample_diversity = self._merged_diversity(div_scorer)
            if spec_scorer is not None:
                res = self._merged_spectrum(spec_scorer)
                self.sample_diversity = {**self.sample_diversity, "Self_CIDEr": res["Self_CIDEr"], "LSA": res["LSA"]}
            samples = dict(samples)
            samples["diversity"] = self.sample_diversity
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_rank() != 0:
            return None
        d = getattr(o, "results_dir", "results")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, (stem or "densecap-%s-%s" % (o.val_split, o.id)) + "_samples.json")
        with open(path, "w") as f:
            json.dump(samples, f)
        if diversity:
            print("diversity of %d captions per segment: %s" % (n, json.dumps(self.sample_diversity)), flush=True)
        return path

    def _frame_boxes(self, ppls, weights):
        """weights [B, T, N] over the proposals (N = num_sampled_frm x num_prop_per_frm, frame-major) -> per word the proposal
        with the largest weight in every sampled frame: boxes [B, T, num_sampled_frm, 7] (trainer.py:217-225)"""
        o = self.opts
        B = weights.size(0)
        ind = torch.max(weights.view(B, weights.size(1), o.num_sampled_frm, o.num_prop_per_frm), dim=-1)[1]
        return torch.gather(ppls.view(-1, o.num_sampled_frm, o.num_prop_per_frm, 7).permute(0, 2, 1, 3).contiguous(), 1,
                            ind.unsqueeze(-1).expand(B, ind.size(1), o.num_sampled_frm, ppls.size(-1)))

    def _collect_grounding(self, b, seq, att2_weights, grd_output):
        """Per generated word, the most attended proposal of every sampled frame (trainer.py:217-248)."""
        o = self.opts
        B = seq.size(0)
        boxes = self._frame_boxes(*self._full_proposal_axis(b["ppls"], att2_weights))
        lemma_det = {o.wtol[k]: i for k, i in o.wtod.items() if k in o.wtol}
        words = seq.tolist()                                   # one device -> host copy each, not one per word
        boxes_l = boxes[..., :4].tolist()
        for i in range(B):
            vid_id, seg_idx = b["seg_id"][i].split('_segment_')
            res = {'clss': [], 'idx_in_sent': [], 'bbox_for_all_frames': []}
            for j, w in enumerate(words[i]):
                if w == 0:
                    break
                lemma = o.wtol[o.itow[str(w)]]
                if lemma in lemma_det:
                    res['bbox_for_all_frames'].append(boxes_l[i][j])
                    res['clss'].append(o.itod[lemma_det[lemma]])
                    res['idx_in_sent'].append(j)
            grd_output[vid_id][str(int(seg_idx))] = res

    def _collect_grounding_device(self, b, seq, att2_weights, grd_scorer, grd_output):
        """_collect_grounding on the grounding kernel (eval with the device metrics): one launch scores the batch into the scorer's
        per-class table and returns every object word's proposal slot per sampled frame; the boxes of those words alone are
        gathered and read in ONE device -> host copy (position, class and 4 x frames coordinates per object word)."""
        o = self.opts
        ppls = b["ppls"]
        pick = grd_scorer.add(seq, att2_weights, ppls, b["gt_bboxs"], b["num"][:, 2])["pick"]          # [B, T, frames] int32
        at = (pick[:, :, 0] >= 0).nonzero()                                                       # the object words: (row, position)
        rows_i, pos = at[:, 0], at[:, 1]
        slots = pick[rows_i, pos].long()                                                          # [n, frames]
        clips = (rows_i // (seq.size(0) // ppls.size(0))).unsqueeze(1)
        given = (slots < ppls.size(1)).unsqueeze(2)                                               # a trimmed slot: a zero box
        boxes = torch.where(given, ppls[clips, slots.clamp(max=ppls.size(1) - 1), :4], ppls.new_zeros(()))
        cls = grd_scorer.word_cls[seq[rows_i, pos]]
        flat = torch.cat([torch.stack([rows_i, pos, cls.long()], 1).double(), boxes.double().flatten(1)], 1).tolist()
        res = []
        for seg_id in b["seg_id"]:
            vid_id, seg_idx = seg_id.split('_segment_')
            res.append({'clss': [], 'idx_in_sent': [], 'bbox_for_all_frames': []})
            grd_output[vid_id][str(int(seg_idx))] = res[-1]
        for rec in flat:
            r = res[int(rec[0])]
            r['bbox_for_all_frames'].append([rec[3 + 4 * f:7 + 4 * f] for f in range(pick.size(2))])
            r['clss'].append(o.itod[int(rec[2])])
            r['idx_in_sent'].append(int(rec[1]))


def ground_picks(weights, frm_mask_output, roi_labels):
    """weights [B, T, N] (attention or grounder scores of every word over the proposals), frm_mask_output [B, T, N + 1] bool (column 0:
    the sentinel), roi_labels [B, T, N] bool -> pick [B, T] int64: the arg-max over the proposals that are not frame-masked, lowest
    index on ties, -1 for a word without such a proposal; hit [B, T] bool: roi_labels at the pick (a word without one: a miss)."""
    free = ~frm_mask_output[:, :, 1:].bool()
    some = free.any(2)
    pick = weights.masked_fill(~free, float("-inf")).argmax(2)           # (the first of equal maxima)
    hit = roi_labels.bool().gather(2, pick.unsqueeze(2)).squeeze(2) & some
    return torch.where(some, pick, torch.full_like(pick, -1)), hit


def ground_accuracy(words):
    """words: (class index, hit by the attention, hit by the grounder) per annotated object word -> box_accu_att / box_accu_grd
    (hits over all such words), their per-class means box_accu_*_per_cls, and the number of words"""
    per = defaultdict(list)
    for cls, ha, hg in words:
        per[int(cls)].append((bool(ha), bool(hg)))
    n = sum(len(v) for v in per.values())
    stats = {"obj_words": n}
    for i, name in enumerate(("att", "grd")):
        stats["box_accu_" + name] = sum(h[i] for v in per.values() for h in v) / n if n else 0.0
        stats["box_accu_%s_per_cls" % name] = float(np.mean([np.mean([h[i] for h in v]) for v in per.values()])) if n else 0.0
    return stats


def densecap_entry(sentence, seg_id, timestamps):
    """One element of predictions[video] as the reference builds it (trainer.py:253-261): the sentence plus the segment's
    [start, end] from the annotation file, rounded to 2 decimals -- what the ANETcaptions evaluator matches on.
    `segment` (the segment index as a string) is an extra key for the multi-rank merge and debugging."""
    vid_idx, seg_idx = seg_id.split('_segment_')
    seg_idx = str(int(seg_idx))
    stamps = timestamps[vid_idx]['segments'][seg_idx]['timestamps']
    return vid_idx, {'sentence': sentence, 'timestamp': [round(ts, 2) for ts in stamps], 'segment': seg_idx}


def _results_path(o, stem):
    d = getattr(o, "results_dir", "results")
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, stem + '-' + o.val_split + '-' + o.id + '.json')


def write_densecap_json(predictions, o):
    """The ActivityNet dense-captioning submission file the external scorer reads (trainer.py:279-286)."""
    path = _results_path(o, 'densecap')
    with open(path, 'w') as f:
        json.dump({'version': 'VERSION 1.0', 'results': predictions,
                   'external_data': {'used': 'true', 'details': 'Visual Genome for Faster R-CNN pre-training'}}, f)
    return path


def write_grounding_json(grd_output, o, stem='attn-gen-sent-results', eval_mode='gen'):
    """Per-word grounding boxes of the generated sentences for the ANet-Entities scorer (trainer.py:318-329); with another stem and
    eval_mode 'GT': of the GT sentences (Trainer.ground_gt)."""
    path = _results_path(o, stem)
    with open(path, 'w') as f:
        json.dump({'results': grd_output, 'eval_mode': eval_mode,
                   'external_data': {'used': True,
                                     'details': 'Object detector pre-trained on Visual Genome on object detection task.'}}, f)
    return path


CLIP_ADAM = os.environ.get("CVC_CLIP_ADAM", "1") != "0"      # False: torch.optim.Adam (fused) / SGD / Adamax + the library's clip (A/B)


def build_optimizer(model, opt, capturable: bool = False):
    """One param group per tensor; 0.1x LR for ctx2pool_grd / vis_embed (reference main.py:171-191).
    capturable=True keeps Adam's step counters on the device (needed by Trainer.train_step_graphed)."""
    params = []
    for key, value in dict(model.named_parameters()).items():
        if not value.requires_grad:
            continue
        lr = opt.learning_rate * (0.1 if ('ctx2pool_grd' in key or 'vis_embed' in key) else 1.0)
        params.append({'params': [value], 'lr': lr, 'weight_decay': opt.weight_decay, 'betas': (opt.optim_alpha, opt.optim_beta)})
    # every parameter on the GPU and CVC_CLIP_ADAM != 0: clip_grad_norm_ + step in one pass (cvc.optim, csrc/optim.hip), for all
    # three of the reference's optimizers -- which is also what lets --hip_graph and deferred error words take the step
    clip_step = CLIP_ADAM and all(p['params'][0].is_cuda for p in params)
    if opt.optim == 'sgd':
        groups = [{k: v for k, v in p.items() if k != 'betas'} for p in params]
        if clip_step:
            from .optim import ClipSGD
            return ClipSGD(groups, lr=opt.learning_rate, momentum=0.9)
        return torch.optim.SGD(groups, lr=opt.learning_rate, momentum=0.9)
    if opt.optim == 'adam':
        # fused = one pass over (p, g, m, v) per tensor instead of the foreach path's ~9 passes (Adam was 8 % of the step)
        fused = all(p['params'][0].is_cuda for p in params)
        if fused and CLIP_ADAM:
            from .optim import ClipAdam                      # clip_grad_norm_ + step in one pass over p / g / m / v (csrc/optim.hip)
            return ClipAdam(params)
        return torch.optim.Adam(params, capturable=capturable, fused=fused)
    if opt.optim == 'adamax':
        if clip_step:
            from .optim import ClipAdamax
            return ClipAdamax(params)
        return torch.optim.Adamax(params, capturable=capturable)
    raise ValueError('Unknown optimizer: {}'.format(opt.optim))
