"""Decode-and-ground captioner -- drop-in for the reference's model/captioner.py
(`DecodeAndGroundCaptionerGVDROI`): same constructor, same 11-tensor forward, same
state_dict keys, same returns (a tuple of [1]-shaped losses in training, `(seq, att2_weights,
None)` in inference).  What differs is where the arithmetic runs:

* inference (`_sample`, reference :384-443) goes through cvc.decode.DecodeEngine: a flat list of
  HIP launches per step, no host round trips, optional HIP-graph replay; `beam_size > 1` (which
  the reference only asserts away, trainer.py:218) is implemented per SURVEY.md section 7;
* training (`_forward_3_loops`, reference :196-382) runs the same three loops through the
  autograd ops of cvc.functional, with the localizer loop (no recurrence) and both vocabulary
  projections batched over T.

The once-per-clip encoder (`roi_extractor`, reference model/backbone.py) is outside the hot path:
pass any module with the reference extractor's call/return contract (the reference class itself
works); `PrecomputedRegionFeatures` below feeds pre-extracted features.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import dropout
from .. import functional as F_
from .. import hip
from ..decode import DecodeEngine, DecodeWeights
from ..misc import utils
from .decoder_core import AttenedDecoderCore, TopDownDecoderCore
from .localizer_core import LocalizerNoLSTMCore


class PrecomputedRegionFeatures(nn.Module):
    """Stand-in for the once-per-clip encoder when features are pre-extracted / pre-projected
    (the benchmark's input contract).  Owns the two encoder tensors the captioner's grounder
    reads (`vis_embed.0.weight`, `vis_classifiers_bias`, reference backbone.py:55,140) and
    returns, in the order of backbone.py:350-351, the feature dict handed in as `segs_feat`."""

    KEYS = ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "g_pool_feats", "pnt_mask")

    def __init__(self, detect_size: int, vis_encoding_size: int, drop_prob: float = 0.5):
        super().__init__()
        self.vis_embed = nn.Sequential(nn.Embedding(detect_size + 1, vis_encoding_size), nn.ReLU(), nn.Dropout(drop_prob))
        self.vis_classifiers_bias = nn.Parameter(torch.zeros(detect_size + 1))

    def forward(self, segs_feat, proposals=None, num=None, mask_boxes=None, region_feats=None, gt_boxes=None,
                overlaps=None, sample_idx=None, eval_obj_ground=False, replicate_feat=True):
        if not isinstance(segs_feat, dict):
            raise TypeError("PrecomputedRegionFeatures expects the feature dict as the first model input")
        f = segs_feat
        cls_loss = f.get("cls_loss", f["fc_feats"].new_zeros(()))
        return (f["fc_feats"], f["conv_feats"], f["p_conv_feats"], f["pool_feats"], f["p_pool_feats"], f["g_pool_feats"],
                f["pnt_mask"], overlaps, None, cls_loss)


class DecodeAndGroundCaptionerGVDROI(nn.Module):
    """reference model/captioner.py:16-443"""

    def __init__(self, opts, pretrained_decoder=None, embed=None, logit=None, roi_extractor=None):
        super().__init__()
        self.opts = opts
        self.vocab_size = opts.vocab_size
        self.ix_to_word = getattr(opts, "itow", None)
        if roi_extractor is None:
            raise ValueError(
                "roi_extractor is required: the once-per-clip region/frame encoder (reference model/backbone.py) is "
                "outside the MI355X hot path.  Pass the reference's RegionalFeatureExtractorGVD, or "
                "cvc.model.captioner.PrecomputedRegionFeatures for pre-extracted features.")
        self.roi_feat_extractor = roi_extractor
        self.seq_length = opts.seq_length
        self.seq_per_img = opts.seq_per_img
        self.decoder_num_layers = 2
        self.localizer_num_layers = 1
        self.rnn_size = opts.rnn_size
        # scheduled sampling (Bengio et al. 2015): the share of loop A's inputs that are the model's own sampled words instead of the
        # ground truth; read by Trainer.train_step_prepared, set per epoch by cvc.main (cvc.trainer.ss_prob_at).  0 = teacher forcing
        self.ss_prob = 0.0
        self.iou_threshold = 0.5

        self.decoder_core = TopDownDecoderCore(opts) if pretrained_decoder is None else pretrained_decoder
        vocab_rows = opts.vocab_size + 1 if opts.embedding_vocab_plus_1 else opts.vocab_size
        if embed is None:
            embed = nn.Sequential(nn.Embedding(vocab_rows, opts.input_encoding_size), nn.ReLU(),
                                  nn.Dropout(opts.drop_prob_lm))
        self.embed = embed
        self.logit = nn.Linear(opts.rnn_size, vocab_rows) if logit is None else logit
        self.localizer_core = LocalizerNoLSTMCore(opts)
        # reconstructor shares the decoder's two LSTM cells (reference :86-87)
        self.attended_roi_decoder_core = AttenedDecoderCore(opts, self.decoder_core.att_lstm, self.decoder_core.lang_lstm)
        self.critLM = utils.LMCriterion(opts)
        self.unk_idx = int(opts.wtoi['UNK'])
        self.xe_criterion = utils.LanguageCriterion(opts)
        # label smoothing of the two language criteria of a training pass (loop A's decode loss, loop C's reconstruction loss): both
        # criteria read opts.label_smoothing; model.label_smoothing = eps changes both.  With eps > 0 a training pass leaves loop A's
        # UNSMOOTHED mean NLL here as a device scalar (no graph), else None.  The self-critical loss and every scoring / evaluation
        # path are not smoothed.
        self.last_nll = None
        # entropy regulariser: both criteria read opts.confidence_penalty (None = off); model.confidence_penalty = beta changes both.
        # With it not None a training pass leaves loop A's mean masked entropy of the word distribution here, and scst_loss with
        # entropy_beta not None the rollouts' (a device scalar, no graph), else None.  Evaluation passes carry no penalty.
        self.last_entropy = None
        # word-level distillation: dict(teacher=CaptionEnsemble, alpha=, tau=) or None.  forward(soft_targets=rows) then trains loop A
        # against the teacher's rows (teacher.soft_targets(batch)[0]) mixed with the one-hot loss; the pass leaves loop A's UNMIXED
        # mean NLL in last_nll and its unmixed mean tau^2 KL(teacher || student) in last_kd (device scalars, no graph), else None.
        # The reconstruction loss, loops B / C, the attention criteria, the self-critical loss and evaluation are not distilled.
        self.distill: Optional[dict] = None
        self.last_kd = None
        self._soft_targets = None
        self.beam_size = int(getattr(opts, "beam_size", 1))
        self.use_hip_graph = bool(getattr(opts, "hip_graph", False))
        # decoding rule of _sample: sample_max = 1 takes the arg-max word (greedy / beam); sample_max = 0 samples from
        # softmax(logits / sample_temperature) without UNK, sample_n captions per clip, noise seeded with sample_seed
        self.sample_max = int(getattr(opts, "sample_max", 1))
        self.sample_temperature = float(getattr(opts, "temperature", 1.0))
        self.sample_n = int(getattr(opts, "sample_n", 1))
        self.sample_seed = int(getattr(opts, "sample_seed", 0))
        # truncation of the sampled distribution (DecodeEngine top_k / top_p; 0 / 1.0 = off)
        self.sample_top_k = int(getattr(opts, "top_k", 0))
        self.sample_top_p = float(getattr(opts, "top_p", 1.0))
        # constrained decoding (DecodeEngine no_repeat_ngram / no_immediate_repeat / min_len / ban_words / bad_endings; all off =
        # the unconstrained engines); the two lists are word ids
        self.no_repeat_ngram = int(getattr(opts, "no_repeat_ngram", 0))
        self.no_immediate_repeat = bool(getattr(opts, "no_immediate_repeat", False))
        self.min_caption_len = int(getattr(opts, "min_caption_len", 0))
        self.ban_words = tuple(getattr(opts, "ban_word_ids", None) or ())
        self.bad_endings = tuple(getattr(opts, "bad_ending_ids", None) or ())
        # diverse (group) beam search and the final ranking's length penalty (DecodeEngine beam_groups / diversity / length_penalty)
        self.beam_groups = int(getattr(opts, "group_size", 1))
        self.diversity_lambda = float(getattr(opts, "diversity_lambda", 0.0))
        self.length_penalty = float(getattr(opts, "length_penalty", 0.0))
        # lexically constrained beam search (DecodeEngine force_n): word ids every caption should contain, or per clip the words of
        # its force_detected best-scored detection classes (cvc.misc.utils.detected_force_words)
        self.force_words = tuple(getattr(opts, "force_word_ids", None) or ())
        self.force_detected = int(getattr(opts, "force_detected", 0))
        # consensus (minimum-Bayes-risk) selection among a clip's candidates (DecodeEngine.consensus): "off", "samples" (every decode
        # of _sample draws consensus_samples captions per clip and keeps the consensus one) or "beam" (the hypotheses of beam search);
        # consensus_table is the cvc.cider.CiderD the utilities are taken over (Trainer sets the training captions' table)
        self.consensus = str(getattr(opts, "consensus", "off") or "off")
        # stochastic beam search (_sample(stochastic_beam=...); DecodeEngine stochastic): beam_size distinct sampled captions per clip
        self.stochastic_beam = bool(getattr(opts, "stochastic_beam", False))
        self.stochastic_tau = float(getattr(opts, "stochastic_tau", 1.0))
        self.consensus_samples = int(getattr(opts, "consensus_samples", 16))
        self.consensus_temperature = float(getattr(opts, "consensus_temperature", 1.0))
        self.consensus_seed = int(getattr(opts, "consensus_seed", 1))
        # the utility mix ({name: weight} over cvc.metrics.REWARD_NAMES, None: CIDEr-D alone), the candidates' weights as references
        # ("uniform" / "model": exp(consensus_alpha * the hypothesis' log-prob), beam candidates only), and whether last_consensus
        # keeps the raw pair metrics (DecodeEngine.consensus; csrc/consensus_mix.hip)
        self.consensus_utility = getattr(opts, "consensus_utility", None) or None
        self.consensus_weights = str(getattr(opts, "consensus_weights", None) or "uniform")
        self.consensus_alpha = 1.0 if getattr(opts, "consensus_alpha", None) is None else float(opts.consensus_alpha)
        self.consensus_pairs = False
        self.consensus_table = None
        self.last_consensus: Optional[dict] = None
        # decode precision: "fp32", or "bf16" = the six weight matrices of the decode stored as bf16 (DecodeEngine weights_dtype)
        self.decode_weights_dtype = getattr(opts, "decode_weights", "fp32")
        # test hook: set to a dict to receive the training pass's intermediate tensors (ground_weights, att2_weights,
        # output_seq) that the reference computes as locals of _forward_3_loops and never returns
        self.debug_collect: Optional[dict] = None

    # ------------------------------------------------------------------ small pieces
    @property
    def device(self):
        return self.logit.weight.device

    def step_capturable(self, deferred_errors: bool = False) -> bool:
        """True when a whole training step of this model can be captured into a HIP graph (cvc.trainer.Trainer.train): the hot
        path on pre-extracted features always; with the once-per-clip encoder in front (raw features, the reference's own flow:
        trainer.py:39-150 -> model/backbone.py:298-351) when the encoder says so -- its persistent recurrence kernels report barrier
        time-outs through error words, which a captured step can only carry in deferred mode (cvc.hip.defer_errors)."""
        ext = self.roi_feat_extractor
        if isinstance(ext, PrecomputedRegionFeatures):
            return True
        cap = getattr(ext, "step_capturable", None)
        return bool(cap is not None and cap(deferred_errors=deferred_errors))

    def reports_error_words(self) -> bool:
        """does a step of this model launch kernels that report through error words (the encoder's persistent GRU)?"""
        rep = getattr(self.roi_feat_extractor, "reports_error_words", None)
        return bool(rep is not None and rep())

    def init_hidden(self, batch_size, num_layers):
        """reference :96-101"""
        z = torch.zeros(num_layers, batch_size, self.rnn_size, device=self.device)
        return (z, z.clone())

    def _init_step_state(self, batch_size):
        """init_hidden() as the unstacked (h_att, c_att, h_lang, c_lang) the cores' step() takes"""
        z = torch.zeros(4, batch_size, self.rnn_size, device=self.device)
        return tuple(z.unbind(0))

    def _embed(self, word, site=None):
        """embed = Embedding -> ReLU -> Dropout (reference :53-68); lookup+ReLU(+mask) is one kernel.  site: the dropout site's
        name (cvc/dropout.py) so that a test can dictate the mask."""
        drop_p = self.embed[2].p if (self.training and len(self.embed) > 2) else 0.0
        table = self.embed[0].weight
        drop = None
        if 0 < drop_p < 1 and site is not None and dropout.in_kernel(table):
            return F_.embed_relu(table, word, rng=(dropout.rng_state(table.device), dropout.site_id(site), float(drop_p)))
        if drop_p > 0:
            drop = dropout.keep_mask(site or "emb", (word.numel(), table.shape[1]), drop_p, table.device)
        return F_.embed_relu(table, word, drop)

    def _logprobs(self, output):
        """F.log_softmax(self.logit(output), dim=1) (reference :266, :361, :437)"""
        return F_.log_softmax(self._logits(output))

    def _logits(self, output):
        """self.logit(output); the training pass hands these to the fused criteria, which never write log-probs"""
        return F_.linear(output, self.logit.weight, self.logit.bias)

    def _grounder(self, xt, att_feats, mask, bias=None, min_value=-1e8):
        """reference :132-173, dot-product branch (the captioner owns no alpha_net)."""
        assert xt.size(-1) == att_feats.size(-1)
        B, S, _ = xt.size()
        R = att_feats.size(1)
        if mask.dim() == 2:
            mask = mask.unsqueeze(1).expand(B, S, R)
        elif mask.dim() != 3:
            raise NotImplementedError
        if bias is not None:
            assert bias.numel() == B * S * R
        return F_.grounder(xt, att_feats, bias, mask)

    # ------------------------------------------------------------------ forward
    def forward(self, segs_feat, input_seq, gt_caption, num, proposals, gt_boxes, mask_boxes, region_feats, frm_mask,
                sample_idx, pnt_mask, lang_eval=False, teacher_forcing=False, ss_inputs=None, soft_targets=None):
        """reference :175-194.  ss_inputs [B * seq_per_img, T] int64 (column 0 = BOS; ss_rollout's result): loop A embeds these words
        instead of gt_caption[:, :T] -- scheduled sampling; targets, label glue, the grounder's class inputs and loops B / C are the
        ground truth's.  None: teacher forcing, as always.
        soft_targets [T, B * seq_per_img, V] fp32 (CaptionEnsemble.soft_targets' rows): loop A's criterion is distilled against them
        with self.distill's alpha and tau -- a training pass only, not with ss_inputs (the student would be fed words the teacher
        never saw), label smoothing or the confidence penalty.  None: today's launches."""
        if soft_targets is not None:
            if lang_eval or ss_inputs is not None:
                raise RuntimeError("forward: soft_targets are a teacher-forced training pass's (lang_eval=False, no ss_inputs)")
            if self.distill is None:
                raise RuntimeError("forward: soft_targets need model.distill = dict(teacher=, alpha=, tau=)")
            if self.label_smoothing > 0 or self.confidence_penalty is not None:
                raise ValueError("forward: soft_targets cannot be combined with label_smoothing > 0 or the confidence penalty")
            hip.check_distill_scalars(self.distill["alpha"], self.distill["tau"], "model.distill")
            self._soft_targets = soft_targets
            try:
                return self.forward(segs_feat, input_seq, gt_caption, num, proposals, gt_boxes, mask_boxes, region_feats, frm_mask,
                                    sample_idx, pnt_mask)
            finally:
                self._soft_targets = None
        F_.new_step()
        if lang_eval and teacher_forcing and (self.label_smoothing > 0 or self.confidence_penalty is not None):
            # an evaluation pass reports the model's true log-probs: label smoothing and the confidence penalty are the training
            # criterion's alone
            eps, self.label_smoothing = self.label_smoothing, 0.0
            beta, self.confidence_penalty = self.confidence_penalty, None
            try:
                return self._forward_3_loops(segs_feat, input_seq, proposals, gt_caption, num, mask_boxes, gt_boxes,
                                             region_feats, frm_mask, sample_idx, pnt_mask, ss_inputs)
            finally:
                self.label_smoothing = eps
                self.confidence_penalty = beta
        if lang_eval is False or teacher_forcing:
            return self._forward_3_loops(segs_feat, input_seq, proposals, gt_caption, num, mask_boxes, gt_boxes,
                                         region_feats, frm_mask, sample_idx, pnt_mask, ss_inputs)
        if ss_inputs is not None:
            raise RuntimeError("forward: ss_inputs are the training pass's (lang_eval=False)")
        return self._sample(segs_feat, input_seq, proposals, gt_caption, num, mask_boxes, gt_boxes, region_feats,
                            frm_mask, sample_idx, pnt_mask)

    def _encode(self, segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, frm_mask, sample_idx, pnt_mask):
        if proposals.is_cuda and proposals.dtype == torch.float32 and gt_boxes.dtype == torch.float32:
            overlaps = hip.bbox_overlaps(proposals.data, gt_boxes.data, frm_mask.data, pnt_mask[:, 1:].data)     # one launch, bit-exact
        else:
            overlaps = utils.bbox_overlaps(proposals.data, gt_boxes.data, (frm_mask | pnt_mask[:, 1:].unsqueeze(-1)).data)
        return overlaps, self.roi_feat_extractor(segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, overlaps,
                                                 sample_idx)

    def encode_clips(self, segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, frm_mask, sample_idx, pnt_mask):
        """what a decode reads of the once-per-clip encoder: (fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, pnt_mask)"""
        _ov, (fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, _g, pnt_mask, _o, _c, _l) = self._encode(
            segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, frm_mask, sample_idx, pnt_mask)
        return fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, pnt_mask

    def _forward_3_loops(self, segs_feat, input_seq, proposals, gt_caption, num, mask_boxes, gt_boxes, region_feats,
                         frm_mask, sample_idx, pnt_mask, ss_inputs=None):
        """reference :196-382"""
        batch_size = proposals.size(0)
        num_rois = proposals.size(1)
        T = self.seq_length
        gt_caption = gt_caption[:, :self.seq_per_img, :].clone().view(-1, gt_caption.size(2))
        gt_caption = torch.cat((gt_caption.new_zeros(gt_caption.size(0), 1), gt_caption), 1)     # BOS = 0
        input_seq = input_seq.view(-1, input_seq.size(2), input_seq.size(3))
        B = gt_caption.size(0)
        if self.training and dropout.in_kernel(self.logit.weight):
            dropout.advance(self.device)              # this pass's masks: step word of the in-kernel generator += 1, on the device

        overlaps, (fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, g_pool_feats, pnt_mask, _ov, _cls_pred,
                   cls_loss) = self._encode(segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, frm_mask,
                                            sample_idx, pnt_mask)
        region_mask = pnt_mask[:, 1:].contiguous()

        # ---- label glue for all T steps at once (reference :246-260 does it per step; none of it depends on
        # the recurrence): per-word proposal labels and the frame mask on proposals
        tgt_steps = slice(1, T + 1)
        if overlaps.is_cuda and overlaps.dtype == torch.float32:
            # one kernel for all T steps (csrc/label_glue.hip): bool results, bit-exact; the deprecated seq_update side effect of
            # bbox_target (a clone nobody reads, misc/utils.py:363-371) is not reproduced
            roi_labels, frm_mask_output, step_fmask = hip.label_glue(overlaps, mask_boxes[:, 0, :, tgt_steps], frm_mask, pnt_mask)
            return self._forward_after_glue(gt_caption, input_seq, fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats,
                                            g_pool_feats, region_mask, step_fmask, frm_mask_output, roi_labels, cls_loss, ss_inputs)
        bm = mask_boxes[:, :, :, tgt_steps]                                           # [B, seq_per_img, K, T]
        ov = overlaps.unsqueeze(1).masked_fill(bm[:, 0].permute(0, 2, 1).unsqueeze(2).expand(B, T, num_rois, -1), 0)
        roi_labels = ov.max(3)[0] > 0.5                                                # [B, T, N]   (utils.bbox_target)
        no_prop = (roi_labels.sum(2) > 0) != (input_seq[:, tgt_steps, 2] > 0)          # deprecated seq_update side effect
        upd = input_seq.data.clone()[:, tgt_steps]
        upd[..., 0] = torch.where(no_prop, upd[..., 3], upd[..., 0])
        upd[..., 1] = torch.where(no_prop, torch.zeros_like(upd[..., 1]), upd[..., 1])
        upd[..., 2] = torch.where(no_prop, torch.zeros_like(upd[..., 2]), upd[..., 2])
        box_mask_t = bm[:, 0].permute(0, 2, 1).unsqueeze(2)                            # [B, T, 1, K]
        frm_on_prop = torch.sum(~(box_mask_t | frm_mask.unsqueeze(1)), dim=3) <= 0     # [B, T, N]
        frm_mask_output = torch.cat((frm_on_prop.new_zeros(B, T, 1), frm_on_prop), dim=2) | pnt_mask.bool().unsqueeze(1)
        step_fmask = frm_mask_output[:, :, 1:].permute(1, 0, 2).contiguous()           # [T, B, N]
        return self._forward_after_glue(gt_caption, input_seq, fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats,
                                        g_pool_feats, region_mask, step_fmask, frm_mask_output, roi_labels, cls_loss, ss_inputs)

    def _forward_after_glue(self, gt_caption, input_seq, fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, g_pool_feats,
                            region_mask, step_fmask, frm_mask_output, roi_labels, cls_loss, ss_inputs=None):
        """_forward_3_loops from loop A on (reference :242-382).  ss_inputs: loop A's input words (scheduled sampling); loop C
        reconstructs from the ground truth's either way."""
        T = self.seq_length
        B = gt_caption.size(0)
        num_rois = pool_feats.size(1)
        if ss_inputs is not None and (tuple(ss_inputs.shape) != (B, T) or ss_inputs.dtype != torch.int64):
            raise RuntimeError(f"forward: ss_inputs must be int64 [B * seq_per_img, T] = [{B}, {T}], got {ss_inputs.dtype} "
                               f"{tuple(ss_inputs.shape)}")
        # ---- Loop A: teacher-forced decode (sequential: LSTM recurrence)            reference :242-270
        emb_all = self._embed(gt_caption[:, :T] if ss_inputs is None else ss_inputs, "emb_a")      # [B, T, E], one launch
        loops = self._loop_plan(B, fc_feats)
        if loops is not None:
            return self._forward_loops_driven(loops, emb_all, gt_caption, input_seq, fc_feats, conv_feats, p_conv_feats, pool_feats,
                                              p_pool_feats, g_pool_feats, region_mask, step_fmask, frm_mask_output, roi_labels, cls_loss,
                                              mixed=ss_inputs is not None)
        state = self._init_step_state(B)
        outputs, masked_attn = [], []
        # one unbind per tensor instead of T selects: a select's backward is a zero-filled [B, T, E] tensor plus an
        # accumulation per step, unbind's is a single stack
        emb_steps = emb_all.unbind(1)
        # the att-LSTM's inputs that do not depend on the recurrence (fc_feats, the teacher-forced embedded words) are multiplied
        # for all T steps in one dense product; the per-step launches stream only the recurrent columns (cvc.functional)
        R = self.rnn_size
        hoist = torch.is_grad_enabled() and fc_feats.is_cuda
        w_att = self.decoder_core.att_lstm.weight_ih
        att_segs = (lambda e: [(fc_feats, R), (e, 2 * R)]) if self.opts.global_img_in_attn_lstm else (lambda e: [(e, R)])
        g_att = F_.hoisted_gates(w_att, att_segs(emb_all), T, B) if hoist else None
        for t in range(T):
            output, state, _roi_attn, frame_masked_attn, _wp = self.decoder_core.step(
                emb_steps[t], fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, region_mask, state,
                proposal_frame_mask=step_fmask[t], drop_site="out_a.%d" % t, gate_pre_att=None if g_att is None else g_att[t])
            outputs.append(output)
            masked_attn.append(frame_masked_attn)
        att2_weights = torch.stack(masked_attn, dim=1)                               # pre-softmax (:273)
        lang_logits = self._logits(torch.stack(outputs, 1).view(B * T, -1))          # all T at once, [B*T, V]

        # ---- grounder over all T                                                      reference :282-294
        xt_clamp = torch.clamp(input_seq[:, 1:T + 1, 0].clone() - self.vocab_size, min=0)
        xt_all = self._vis_embed(xt_clamp)
        if hasattr(self.roi_feat_extractor, 'vis_classifiers_bias'):
            bias = self.roi_feat_extractor.vis_classifiers_bias[xt_clamp].type(xt_all.type()).unsqueeze(2).expand(
                B, T, num_rois)
        else:
            bias = 0
        ground_weights = self._grounder(xt_all, g_pool_feats, frm_mask_output[:, :, 1:], bias + att2_weights)

        if self.debug_collect is not None:
            self.debug_collect.update(ground_weights=ground_weights, att2_weights=att2_weights, roi_labels=roi_labels,
                                      frm_mask_output=frm_mask_output)
        target = gt_caption[:, 1:T + 1].clone()
        # criteria fused with log_softmax and the argmax cut of :313 (one pass over the logits, no [B,T,V] log-probs)
        lm_loss, att2_loss, ground_loss, output_seq = self.critLM.from_logits(
            lang_logits, att2_weights, ground_weights, target, roi_labels[:, :T, :].clone(), input_seq[:, 1:T + 1, 0].clone(),
            **({} if self._soft_targets is None else dict(distill=self._kd())))
        self.last_nll = self.critLM.last_nll
        self.last_entropy = self.critLM.last_entropy
        self.last_kd = self.critLM.last_kd
        if self.opts.train_decoder_only:                                              # reference :297-307
            return lm_loss.reshape(1), att2_loss.reshape(1), ground_loss.reshape(1), cls_loss.reshape(1)

        # ---- argmax cut, Loop B: localize (no recurrence -> all T in one attention call)  :313-338
        loc_emb = self._embed(output_seq, "emb_b")                                   # [B, T, E]
        loc_pool, loc_conv, _prob = self.localizer_core.forward_all_steps(loc_emb, conv_feats, p_conv_feats, pool_feats,
                                                                           p_pool_feats, region_mask)

        # ---- Loop C: reconstruct from the localized regions (sequential)             reference :348-362
        state = self._init_step_state(B)
        # fresh dropout mask in training; with scheduled-sampling inputs emb_all is not the ground truth's
        emb_all_c = self._embed(gt_caption[:, :T], "emb_c") if (self.training or ss_inputs is not None) else emb_all
        rec_outputs = []
        emb_steps_c, pool_steps, conv_steps = emb_all_c.unbind(1), loc_pool.unbind(1), loc_conv.unbind(1)
        # loop C knows even more of its inputs beforehand: the localized context of every step (loop B's output)
        g_att_c = F_.hoisted_gates(w_att, att_segs(emb_all_c), T, B) if hoist else None
        ctx_all = (loc_pool + loc_conv) if hoist else None                                  # [B, T, R], one add instead of T
        g_lang_c = F_.hoisted_gates(self.attended_roi_decoder_core.lang_lstm.weight_ih, [(ctx_all, 0)], T, B) if hoist else None
        ctx_steps = ctx_all.unbind(1) if g_lang_c is not None else None
        for t in range(T):
            output, state = self.attended_roi_decoder_core.step(
                emb_steps_c[t], fc_feats, pool_steps[t], conv_steps[t], state, drop_site="out_c.%d" % t,
                gate_pre_att=None if g_att_c is None else g_att_c[t], gate_pre_lang=None if g_lang_c is None else g_lang_c[t],
                ctx_sum=None if ctx_steps is None else ctx_steps[t])
            rec_outputs.append(output)
        lm_recon_loss = self.xe_criterion.from_logits(self._logits(torch.stack(rec_outputs, 1).view(B * T, -1)), target)
        return (lm_loss.reshape(1), att2_loss.reshape(1), ground_loss.reshape(1), cls_loss.reshape(1),
                lm_recon_loss.reshape(1))

    def _kd(self):
        """loop A's distill= of this pass: (teacher rows, alpha, tau), or None"""
        if self._soft_targets is None:
            return None
        return self._soft_targets, self.distill["alpha"], self.distill["tau"]

    @property
    def label_smoothing(self) -> float:
        return self.critLM.label_smoothing

    @label_smoothing.setter
    def label_smoothing(self, eps):
        eps = hip.check_label_smoothing(eps)
        self.critLM.label_smoothing = self.xe_criterion.label_smoothing = eps

    @property
    def confidence_penalty(self):
        return self.critLM.confidence_penalty

    @confidence_penalty.setter
    def confidence_penalty(self, beta):
        beta = None if beta is None else hip.check_entropy_beta(beta, "confidence_penalty")
        self.critLM.confidence_penalty = self.xe_criterion.confidence_penalty = beta

    # ------------------------------------------------------------------ training pass on the C-driven loops
    def _loop_plan(self, B, like):
        """(attention kind, 1 / temperature, dropout spec of loop A, of loop C) when the two recurrent loops of this pass can run
        as one C-driven autograd node each (cvc/train_loops.py), else None (per-step path: dictated dropout masks, library
        dropout, widths the packed kernels do not take).  More than 64 clips: groups of <= 64 (cvc.train_loops.clip_groups)."""
        from .. import train_loops
        from .modules import AdditiveSoftAttention
        dc, rc = self.decoder_core, self.attended_roi_decoder_core
        sa = dc.soft_attn
        R, E, A = self.rnn_size, self.embed[0].weight.shape[1], sa.h2attn.weight.shape[0]
        if not train_loops.eligible(B, R, E, A, like, self.seq_length) or dropout.active():
            return None
        if not (dc.att_lstm.weight_ih.is_contiguous() and dc.lang_lstm.weight_ih.is_contiguous() and sa.h2attn.weight.is_contiguous()):
            return None
        specs = []
        for mod, site in ((dc.dropout, "out_a.0"), (rc.dropout, "out_c.0")):
            if mod.training and mod.p > 0:
                if not (mod.p < 1 and dropout.in_kernel(like)):
                    return None
                specs.append((dropout.rng_state(like.device), dropout.site_id(site), float(mod.p)))
            else:
                specs.append(None)
        additive = isinstance(sa, AdditiveSoftAttention)
        return (hip.ATTN_ADDITIVE if additive else hip.ATTN_DOT, 1.0 if additive else 1.0 / float(sa.temp), specs[0], specs[1])

    def _forward_loops_driven(self, plan, emb_all, gt_caption, input_seq, fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats,
                              g_pool_feats, region_mask, step_fmask, frm_mask_output, roi_labels, cls_loss, mixed=False):
        """_forward_3_loops from loop A on (reference :242-382) with loops A and C as one autograd node each; rows of the loops'
        outputs are t-major (t * B + b), so the vocabulary head and its criterion run on t-major rows too.  mixed: emb_all embeds
        scheduled-sampling inputs, so loop C embeds the ground truth itself."""
        emb_gt = None if mixed else emb_all
        from .. import train_loops
        attn_kind, inv_temp, drop_a, drop_c = plan
        B, T, R = emb_all.shape[0], self.seq_length, self.rnn_size
        num_rois = pool_feats.shape[1]
        dc = self.decoder_core
        fc_in = fc_feats if self.opts.global_img_in_attn_lstm else None
        # the loops take 64 clips: a larger batch runs them once per group of clips (clips are independent through both loops), each
        # group with its own arena; what is batch-wide below (head, criteria, grounder, localizer, embeddings) is one call over all B
        groups = train_loops.clip_groups(B)
        nslots = 1 if self.opts.train_decoder_only else 2
        arenas = [train_loops.LoopArena(nslots, T, b1 - b0, R, emb_all.shape[2], emb_all.device) for b0, b1 in groups]
        feats = (pool_feats, p_pool_feats, conv_feats, p_conv_feats)
        cut = (lambda x, b0, b1: x) if len(groups) == 1 else (lambda x, b0, b1: None if x is None else x[b0:b1])
        cut_t = (lambda x, b0, b1: x) if len(groups) == 1 else (lambda x, b0, b1: None if x is None else x[:, b0:b1].contiguous())
        join_t = (lambda xs: xs[0]) if len(groups) == 1 else (lambda xs: None if xs[0] is None else torch.cat(xs, 1))      # [T, b, .] -> [T, B, .]
        for a_ in arenas:
            a_.sole = len(groups) == 1           # several groups: a weight's gradient has several producers (see LoopArena.sole)

        def grp_drop(spec, g):
            """a group's own dropout sites (site0 + 64 g + t): without it clip i of every group would draw clip i's mask of group 0"""
            return None if spec is None else (spec[0], spec[1] + 64 * g, spec[2])

        parts = [train_loops.decode_loop(arenas[g], cut(emb_all, b0, b1), cut(fc_in, b0, b1), tuple(cut(f, b0, b1) for f in feats),
                                         cut(region_mask, b0, b1), cut_t(step_fmask, b0, b1), dc.att_lstm, dc.lang_lstm, dc.soft_attn,
                                         attn_kind, inv_temp, grp_drop(drop_a, g)) for g, (b0, b1) in enumerate(groups)]
        out_a = join_t([p_[0] for p_ in parts])
        fm = join_t([p_[1] for p_ in parts])
        target = gt_caption[:, 1:T + 1].clone()
        out_c, done = None, None
        kd = {} if self._soft_targets is None else dict(distill=self._kd())
        head = self.critLM.head_words(out_a.view(T * B, R), self.logit, target, t_major=True, **kd) if all(a.joint_ok() for a in arenas) else None
        if head is not None:
            # A group's two loops fit the joint back-propagation (64 + 64 rows: config 3; 32 + 32: the shares of the 8-GPU job): loops B
            # and C come FIRST, fed the argmax words of the head's arithmetic, and loop A's outputs pass through loop C's graph node
            # -- its backward then holds both loops' output gradients and runs their back-propagation as one pass (cvc.train_loops._Loop).
            done, output_seq = head
            out_c, out_a, fm = self._loops_b_c(arenas, groups, output_seq, gt_caption, emb_gt, fc_in, conv_feats, p_conv_feats, pool_feats,
                                               p_pool_feats, region_mask, attn_kind, drop_c, joint=[(p_[0], p_[1]) for p_ in parts])
        att2_weights = fm.transpose(0, 1)                                             # [B, T, N] pre-softmax (:273)

        # ---- grounder over all T                                                      reference :282-294
        xt_clamp = torch.clamp(input_seq[:, 1:T + 1, 0].clone() - self.vocab_size, min=0)
        xt_all = self._vis_embed(xt_clamp)
        if hasattr(self.roi_feat_extractor, 'vis_classifiers_bias'):
            bias = self.roi_feat_extractor.vis_classifiers_bias[xt_clamp].type(xt_all.type()).unsqueeze(2).expand(B, T, num_rois)
        else:
            bias = 0
        ground_weights = self._grounder(xt_all, g_pool_feats, frm_mask_output[:, :, 1:], bias + att2_weights)
        if self.debug_collect is not None:
            self.debug_collect.update(ground_weights=ground_weights, att2_weights=att2_weights, roi_labels=roi_labels,
                                      frm_mask_output=frm_mask_output)
        # vocabulary head + criterion + the argmax cut of :313 as one op on the t-major rows (no logits tensor)
        lm_loss, att2_loss, ground_loss, output_seq = self.critLM.from_head(
            out_a.view(T * B, R), self.logit, att2_weights, ground_weights, target, roi_labels[:, :T, :], input_seq[:, 1:T + 1, 0],
            t_major=True, done=done, **kd)
        self.last_nll = self.critLM.last_nll
        self.last_entropy = self.critLM.last_entropy
        self.last_kd = self.critLM.last_kd
        if self.opts.train_decoder_only:                                              # reference :297-307
            return lm_loss.reshape(1), att2_loss.reshape(1), ground_loss.reshape(1), cls_loss.reshape(1)
        if out_c is None:
            out_c = self._loops_b_c(arenas, groups, output_seq, gt_caption, emb_gt, fc_in, conv_feats, p_conv_feats, pool_feats, p_pool_feats,
                                    region_mask, attn_kind, drop_c)
        lm_recon_loss = self.xe_criterion.from_head(out_c.view(T * B, R), self.logit, target, t_major=True)
        return (lm_loss.reshape(1), att2_loss.reshape(1), ground_loss.reshape(1), cls_loss.reshape(1), lm_recon_loss.reshape(1))

    def _loops_b_c(self, arenas, groups, output_seq, gt_caption, emb_all, fc_in, conv_feats, p_conv_feats, pool_feats, p_pool_feats,
                   region_mask, attn_kind, drop_c, joint=None):
        """the argmax cut, loop B (localize, all T in one attention call; reference :313-338) and loop C (reconstruct from the
        localized regions; reference :348-362).  Loop B and the embeddings are one call over the whole batch; loop C runs once per
        group of <= 64 clips (cvc.train_loops.clip_groups).  -> out_c [T, B, R], or (out_c, loop A's out, loop A's fm) with `joint`
        (per group: loop A's (out, fm) of that group).  emb_all: the embedded ground-truth inputs, reused in eval mode; None =
        embed them here (loop A ran on other inputs)"""
        from .. import train_loops
        dc, T = self.decoder_core, self.seq_length
        loc_emb = self._embed(output_seq, "emb_b")                                   # [B, T, E]
        ctx_all = self.localizer_core.forward_all_steps_sum(loc_emb, conv_feats, p_conv_feats, pool_feats, p_pool_feats, region_mask)
        emb_all_c = self._embed(gt_caption[:, :T], "emb_c") if (self.training or emb_all is None) else emb_all   # fresh dropout mask in training
        one = len(groups) == 1
        outs = []
        for g, (b0, b1) in enumerate(groups):
            sl = (lambda x: x) if one else (lambda x: None if x is None else x[b0:b1])
            drop = None if drop_c is None else (drop_c[0], drop_c[1] + 64 * g, drop_c[2])
            outs.append(train_loops.recon_loop(arenas[g], sl(emb_all_c), sl(fc_in), sl(ctx_all), dc.att_lstm, dc.lang_lstm, dc.soft_attn,
                                               attn_kind, drop, joint=None if joint is None else joint[g]))
        if one:
            return outs[0]
        if joint is None:
            return torch.cat(outs, 1)
        fms = [o[2] for o in outs]
        return (torch.cat([o[0] for o in outs], 1), torch.cat([o[1] for o in outs], 1),
                None if fms[0] is None else torch.cat(fms, 1))

    # ------------------------------------------------------------------ self-critical training: the gradient pass
    def scst_loss(self, encoded, words, reward, base=None, per_clip: int = 1, wor=None, entropy_beta=None):
        """The self-critical loss of sampled captions: loop A (reference :242-270) teacher-forced on the SAMPLED words, the vocabulary
        head and its criterion with the advantage as row weight:  -sum_{r,t} w[r, t] log p(words[r, t]) / sum(mask),
        w = advantage x mask (cvc_scst_weights; mask = LMCriterion's: the steps up to and including the first 0).
        encoded: the once-per-clip encoder's (fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, pnt_mask) of the B clips
        (constants here: the decoder's parameters -- decoder_core, embed, logit -- are what this loss reaches);
        words [B * per_clip, T] int64, row b * per_clip + j = sample j of clip b; reward [B * per_clip]; base [B] (per_clip == 1:
        the greedy caption's reward) or None (per_clip > 1: leave-one-out mean of the clip's other samples).
        Dropout follows the module's mode: eval() = the policy that was sampled.  More than 64 rows run loop A as groups of <= 64.
        wor = dict(logq=, G=, state=, normalize=True): the rows are a stochastic beam's first per_clip slots, a sample WITHOUT
        replacement (logq, G [B, per_clip + 1] with the threshold slot, state the engine's generator words: model.last_stochastic);
        w comes from cvc_scst_weights_wor -- importance weights and a per-row baseline ("Self-critical training
        without replacement") --, base must be None, and self.last_wor = dict(wgt [B * per_clip], est [B]) keeps the weights and the
        clip's estimated expected reward.  None: cvc_scst_weights, the launches and the bits of a step without it.
        entropy_beta = beta (finite): the entropy bonus, -beta x the mean entropy of the word distribution over the steps that count
        (the mask of w) added to the loss; the entropy is the model's full-vocabulary one at temperature 1, not the sampler's (which
        leaves UNK out and may be tempered or truncated), as log p above.  self.last_entropy keeps that mean (no graph).  0: the
        entropy is measured, loss and gradient keep their bits.  None: the launches and the bits of a step without it.
        -> (loss (), adv [B * per_clip])"""
        from .. import train_loops
        fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, pnt_mask = encoded
        T, R, S = self.seq_length, self.rnn_size, int(per_clip)
        rows = words.size(0)
        if words.dim() != 2 or words.size(1) != T or words.dtype != torch.int64 or rows != fc_feats.size(0) * S:
            raise RuntimeError(f"scst_loss: words must be int64 [B * per_clip, T] = [{fc_feats.size(0)} * {S}, {T}], got {words.dtype} "
                               f"{tuple(words.shape)}")
        F_.new_step()
        if self.training and dropout.in_kernel(self.logit.weight):
            dropout.advance(self.device)
        rep = (lambda x: x.detach().contiguous()) if S == 1 else (lambda x: x.detach().repeat_interleave(S, 0))
        fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats = (rep(x) for x in (fc_feats, conv_feats, p_conv_feats, pool_feats,
                                                                                           p_pool_feats))
        region_mask = rep(pnt_mask[:, 1:])
        words = words.contiguous()
        # a rollout goes on sampling behind its end mark (no early exit, reference :384-443): in the TARGET those words are zeroed, so
        # that LMCriterion's mask of it (and its count) is "the steps up to and including the first 0", the mask of w; the inputs stay
        # the rollout's own words, so every step's log-probs are the engine's (the recurrence is causal: no step that counts sees them)
        target = words.masked_fill((words == 0).cumsum(1) > 0, 0)
        inputs = torch.cat((words.new_zeros(rows, 1), words[:, :T - 1]), 1)                 # BOS = 0, then the sampled words
        emb_all = self._embed(inputs, "emb_a")                                             # [rows, T, E]
        dc = self.decoder_core
        fc_in = fc_feats if self.opts.global_img_in_attn_lstm else None
        plan = self._loop_plan(min(rows, 64), fc_feats)
        if plan is not None:
            attn_kind, inv_temp, drop_a, _ = plan
            groups = train_loops.clip_groups(rows)
            cut = lambda x, b0, b1: None if x is None else (x if len(groups) == 1 else x[b0:b1])
            outs = []
            for g, (b0, b1) in enumerate(groups):
                arena = train_loops.LoopArena(1, T, b1 - b0, R, emb_all.shape[2], emb_all.device)
                arena.sole = len(groups) == 1
                drop = None if drop_a is None else (drop_a[0], drop_a[1] + 64 * g, drop_a[2])
                outs.append(train_loops.decode_loop(arena, cut(emb_all, b0, b1), cut(fc_in, b0, b1),
                                                    tuple(cut(f, b0, b1) for f in (pool_feats, p_pool_feats, conv_feats, p_conv_feats)),
                                                    cut(region_mask, b0, b1), None, dc.att_lstm, dc.lang_lstm, dc.soft_attn, attn_kind,
                                                    inv_temp, drop)[0])
            out = (outs[0] if len(outs) == 1 else torch.cat(outs, 1)).view(T * rows, R)      # t-major rows
            t_major = True
        else:
            state = self._init_step_state(rows)
            steps = []
            for t, emb in enumerate(emb_all.unbind(1)):
                output, state, _roi, _fm, _wp = dc.step(emb, fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, region_mask,
                                                        state, drop_site="out_a.%d" % t)
                steps.append(output)
            out = torch.stack(steps, 1).view(rows * T, R)
            t_major = False
        if wor is None:
            adv, w = hip.scst_weights(reward, base, S, words, t_major=t_major)
        else:
            if base is not None:
                raise RuntimeError("scst_loss: wor carries its own per-row baseline, base must be None")
            adv, wgt, est, w = hip.scst_weights_wor(reward, wor["logq"], wor["G"], wor["state"], S, words, t_major=t_major,
                                                    normalize=bool(wor.get("normalize", True)))
            self.last_wor = dict(wgt=wgt, est=est)
        if self.debug_collect is not None:
            self.debug_collect.update(scst_out=out, scst_t_major=t_major, scst_w=w)
        loss = self.xe_criterion.from_head(out, self.logit, target, t_major=t_major, row_weight=w, entropy_beta=entropy_beta)
        self.last_entropy = self.xe_criterion.last_entropy
        return loss.reshape(()), adv

    def _vis_embed(self, xt_clamp):
        """roi_feat_extractor.vis_embed (Embedding -> ReLU -> Dropout, backbone.py:55-57) on the grounder's class indices"""
        ve = self.roi_feat_extractor.vis_embed
        ve_seq = self.training and isinstance(ve, nn.Sequential) and len(ve) == 3 and isinstance(ve[2], nn.Dropout)
        if ve_seq and 0 < ve[2].p < 1 and dropout.in_kernel(ve[0].weight) and isinstance(ve[0], nn.Embedding) and ve[0].weight.shape[1] % 4 == 0:
            # lookup + ReLU + dropout in the embedding kernel, mask generated there
            return F_.embed_relu(ve[0].weight, xt_clamp, rng=(dropout.rng_state(xt_clamp.device), dropout.site_id("vis_embed"), float(ve[2].p)))
        if dropout.active() and ve_seq:
            return dropout.apply(ve[2], ve[1](ve[0](xt_clamp)), "vis_embed")         # dictated mask (train-mode parity tests)
        return ve(xt_clamp)

    # ------------------------------------------------------------------ inference
    def decode_weights(self) -> DecodeWeights:
        """Flat (and, on first use by the packed decode path, fragment-packed) views of the hot-path parameters.
        Cached until any parameter is modified in place (optimizer step, load_state_dict), detected through the
        tensors' version counters, so an evaluation loop binds / packs the checkpoint once."""
        params = [p for _, p in sorted(self.state_dict(keep_vars=True).items())]
        key = tuple((p.data_ptr(), p._version) for p in params)
        cached = getattr(self, "_decode_cache", None)
        if cached is None or cached[0] != key:
            sd = {k: v for k, v in self.state_dict().items()}
            cached = (key, DecodeWeights(sd, getattr(self.opts, "softattn_type", "additive")))
            self._decode_cache = cached
        return cached[1]

    def invalidate_decode_cache(self):
        """Drop the cached decode binding.  Needed after parameter updates that bypass the tensors' version counters:
        a HIP-graph replay of the training step, or a fused optimizer kernel (Trainer calls this after every step)."""
        self._decode_cache = None
        self._engine_cache = None
        self._score_cache = None
        self._ss_cache = None
        hip.bump_weights_generation()            # the encoder's packed GRU / dense operands are keyed on it (cvc/gru.py, cvc/dense.py)

    def refresh_decode_weights(self):
        """After a parameter update IN PLACE (an optimizer step, a replayed training graph): keep the cached decode binding and the
        cached engines -- launch lists, captured graphs -- and recompute the binding's derived operands into their storage
        (DecodeWeights.refresh()) instead of dropping everything as invalidate_decode_cache() does.  A parameter whose storage moved
        (load_state_dict into new tensors, .to()) cannot be refreshed: that falls back to invalidation.  Used by the
        scheduled-sampling step, which decodes on every step; the encoder's packed operands follow the weights generation as ever."""
        cached = getattr(self, "_decode_cache", None)
        if cached is None:
            return self.invalidate_decode_cache()
        params = [p for _, p in sorted(self.state_dict(keep_vars=True).items())]
        if tuple(p.data_ptr() for p in params) != tuple(k[0] for k in cached[0]):
            return self.invalidate_decode_cache()
        cached[1].refresh()
        self._decode_cache = (tuple((p.data_ptr(), p._version) for p in params), cached[1])
        for slot in ("_engine_cache", "_score_cache", "_ss_cache"):
            ent = getattr(self, slot, None)
            if ent is not None:
                ent[1].weights_refreshed()
        hip.bump_weights_generation()

    # ------------------------------------------------------------------ the cached decode engines
    def _decode_engine(self, slot, feats, T, extra=(), unkeyed=(), may_bind=False, prepare=None, **options):
        """The engine of `slot` (_engine_cache / _score_cache / _ss_cache, each one (key, engine)) with this batch's features in it:
        the cached one when its key matches -- the batch is copied into the engine's own buffers (0.2 ms at cfg2; a captured graph
        keeps the pointers it was captured with), or with may_bind the C-ABI plan of a driver-bound engine without a graph is
        pointed at the new tensors -- else a new DecodeEngine(**options), captured when the model uses HIP graphs, which replaces
        the slot's.  The key is made of what the engine is built from: the weights object, the feature shapes, softmax_temp, T,
        use_hip_graph and every option passed on (lists as tuples), so no option reaches the engine without being in the key;
        `unkeyed` names options that do not distinguish engines (a seed that is set again on every call), `extra` adds what
        distinguishes them without being an option.  prepare(engine): what has to be bound before capture on a new engine, and
        after the features on a cached one (the forced mode's captions and frame mask)."""
        temp = float(getattr(self.opts, "softmax_temp", 1.0))
        weights = self.decode_weights()
        hashable = lambda v: tuple(v) if isinstance(v, (list, tuple)) else v
        key = ((id(weights),) + tuple(tuple(feats[k].shape) for k in ("fc_feats", "conv_feats", "pool_feats")) +
               (temp, T, self.use_hip_graph, tuple(extra)) + tuple((k, hashable(v)) for k, v in sorted(options.items()) if k not in unkeyed))
        cached = getattr(self, slot, None)
        if cached is not None and cached[0] == key:
            engine = cached[1]
            if may_bind and engine._plan is not None and engine.graph is None:
                engine.bind_features(feats)
            else:
                engine.load_features(feats)
            if prepare is not None:
                prepare(engine)
            return engine
        engine = DecodeEngine(weights, feats, T, self.unk_idx, inv_temp=1.0 / temp, own_features=True, **options)
        if prepare is not None:
            prepare(engine)
        if self.use_hip_graph:
            engine.capture()
        setattr(self, slot, (key, engine))
        return engine

    # ------------------------------------------------------------------ scheduled sampling: the rollout
    @torch.no_grad()
    def ss_rollout(self, encoded, gt_caption, prob: float, temperature: float = 1.0, seed: int = 0):
        """Loop A's inputs of a scheduled-sampling step: one decode of the cached MIXED engine (DecodeEngine mix=True, sample_n =
        seq_per_img) over the batch's ground-truth captions -- at every position the word fed on is the model's own sample (drawn
        from softmax(logits / temperature) without UNK, as the sampling engine draws) with probability `prob`, else the ground
        truth's.  No autograd, eval() semantics (dropout off), no host read-back; the engine is re-seeded with `seed` (its first
        decode after that draws with call = 1).
        encoded: encode_clips()'s result; gt_caption: the batch's [B, n, >= T] (or [B * seq_per_img, T]) int64 captions.
        -> ss_inputs [B * seq_per_img, T] int64 = cat(BOS, inputs_next[:, :T - 1]); the engine (ss_engine()) keeps took, drawn,
        given_logprob of the decode."""
        T, S = self.seq_length, self.seq_per_img
        fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, pnt_mask = encoded
        if gt_caption.dim() == 3:
            gt_caption = gt_caption[:, :S, :T].reshape(-1, T)
        given = gt_caption[:, :T].contiguous()
        was_training = self.training
        self.eval()
        try:
            feats = dict(fc_feats=fc_feats.contiguous(), conv_feats=conv_feats.contiguous(), p_conv_feats=p_conv_feats.contiguous(),
                         pool_feats=pool_feats.contiguous(), p_pool_feats=p_pool_feats.contiguous(), pnt_mask=pnt_mask)
            # (the seed is no part of the key: the engine is re-seeded on every call)
            engine = self._decode_engine("_ss_cache", feats, T, unkeyed=("seed",), sample_n=S, temperature=float(temperature), seed=seed,
                                         mix=True)
            engine.load_captions(given)
            engine.set_mix_prob(prob)
            engine.seed(seed)
            inputs_next = engine.run()[0]
            return torch.cat((inputs_next.new_zeros(inputs_next.size(0), 1), inputs_next[:, :T - 1]), 1)
        finally:
            self.train(was_training)

    def ss_engine(self):
        """the cached mixed engine of the last ss_rollout (None before the first, and after invalidate_decode_cache())"""
        ent = getattr(self, "_ss_cache", None)
        return None if ent is None else ent[1]

    @torch.no_grad()
    def _sample(self, segs_feat, seq, proposals, gt_caption, num, mask_boxes, gt_boxes, region_feats, frm_mask, sample_idx,
                pnt_mask, beam_size: Optional[int] = None, sample_max: Optional[int] = None, temperature: Optional[float] = None,
                sample_n: Optional[int] = None, seed: Optional[int] = None, decode_weights: Optional[str] = None,
                top_k: Optional[int] = None, top_p: Optional[float] = None, no_repeat_ngram: Optional[int] = None,
                no_immediate_repeat: Optional[bool] = None, min_len: Optional[int] = None, ban_words=None, bad_endings=None,
                beam_groups: Optional[int] = None, diversity_lambda: Optional[float] = None, length_penalty: Optional[float] = None,
                force_words=None, encoded=None, consensus=None, stochastic_beam: Optional[bool] = None,
                stochastic_tau: Optional[float] = None, consensus_utility=None, consensus_weights: Optional[str] = None,
                consensus_alpha: Optional[float] = None):
        """reference :384-443: exactly seq_length decoder steps from BOS, no EOS early exit, UNK
        suppressed; returns (seq [B,T], att2_weights [B,T,N] post-softmax, None).
        sample_max = 0 (argument, else the model's attribute): every word is sampled from softmax(logits / temperature) without
        UNK, sample_n captions per clip -> (seq [B*n, T], att2_weights [B*n, T, N], logprob [B*n, T]), row b * n + j = sample j of
        clip b.  The sampling engine is seeded once, when it is created (seed); later batches draw fresh noise.
        top_k / top_p (arguments, else the model's sample_top_k / sample_top_p): top-k / nucleus truncation of the sampled
        distribution (DecodeEngine); logprob stays the model's log-prob over the full vocabulary.
        decode_weights: "fp32" / "bf16" (argument, else the model's opts.decode_weights): DecodeEngine's weights_dtype; what the
        bf16 mode does not cover (beam search, sample_n > 1, more than 64 rows) raises, it never decodes in fp32 instead.
        no_repeat_ngram / no_immediate_repeat / min_len / ban_words / bad_endings (arguments, else the model's attributes, read from
        opts): DecodeEngine's constrained decoding.  With any of them on the third result is the log-prob [B*n, T] in the arg-max
        mode too.  With beam_size > 1 the engine is built with beam_history=True (constrained beam search: the rule applies to every
        hypothesis' own history) and the result is a beam decode's (seq, att2_weights, None).
        beam_groups / diversity_lambda / length_penalty (arguments, else the model's attributes, read from opts.group_size /
        diversity_lambda / length_penalty): DecodeEngine's diverse beam search and length-normalised final ranking; with
        beam_size > 1 and any of them on the engine is built with beam_history=True and seq is the best hypothesis by norm (all of
        them: engine.hypotheses(ranked=True)).  With beam_size == 1 the engine refuses them.
        force_words (argument, else the model's attributes, read from opts.force_word_ids / opts.force_detected): words the captions
        should contain, DecodeEngine's force_n -- a [B, C] integer tensor (-1 = unused) or a list of C ids applied to every clip,
        C <= 3; the engine is built with beam_history=True and force_n = C, the words are loaded into it for every batch, and seq is
        the best-normed hypothesis among those that met the most forced words.
        encoded: encode_clips()'s result for this batch -- the encoder is then not run again (Trainer.scst_step: its rollouts, its
        greedy baseline and its gradient pass read the same encoder outputs).
        consensus (argument, else the model's attribute, read from opts.consensus; off by default): consensus (minimum-Bayes-risk)
        selection among the clip's candidates under CIDEr-D over self.consensus_table (DecodeEngine.consensus; without a table the
        call raises).  True: the candidates are what this call decodes -- with sample_max = 0 and sample_n > 1 the n samples of a
        clip, the result is the picked sample per clip (seq [B, T], att2_weights [B, T, N], logprob [B, T]); with beam_size > 1 the
        hypotheses of the beam (the engine is built with beam_history=True), the result is (seq, att2_weights, None) of the picked
        one.  "samples": sampling whatever sample_max says, with the model's consensus_samples / consensus_temperature /
        consensus_seed where sample_n / temperature / seed are not given, beam_size 1.  "beam": as True, beam_size > 1 required.
        The candidates are exactly what the same call returns with consensus=False and the same seed; self.last_consensus =
        dict(candidates, pick, utility, live) keeps them (seq [B * n, T] / hypotheses [B, beam, T]) with the picks [B], the utilities
        [B * n] and the live mask the selection used (None: every sample counts / [B, beam] bool: the score is finite), device tensors.
        consensus_utility / consensus_weights / consensus_alpha (arguments, else the model's attributes, read from opts; CIDEr-D
        alone, "uniform", 1.0 by default): DecodeEngine.consensus's utility mix ({name: weight} over cvc.metrics.REWARD_NAMES), the
        candidates' weights as references ("model": exp(alpha * the hypothesis' log-prob); beam candidates only, a sampling call and
        a stochastic beam raise) and alpha.  At their defaults the selection is the launch it has always been; otherwise it is one
        launch of cvc_consensus_mix.  last_consensus also holds weights (the log-weights used [B * n], None: uniform) and, with
        self.consensus_pairs = True, pairs [B, n, n, 6] (the raw pair metrics).
        stochastic_beam / stochastic_tau (arguments, else the model's attributes, read from opts; off by default): stochastic beam
        search with beam_size > 1 -- the engine is built with beam_history=True and stochastic=True, seeded once with seed (else the
        model's sample_seed); the result is a beam decode's (seq, att2_weights, None) of slot 0, an ordinary sample of q_tau, and
        self.last_stochastic = dict(seq [B, beam, T], score, G, logq [B, beam]) keeps the clip's beam_size distinct captions in
        draw order with their model log-probs, perturbed keys and sampling log-probs, and state, the generator words the decode drew
        its noise with (clones).  It composes with the five
        constraints and with consensus "beam" / True (the candidates are the distinct samples); what the engine refuses raises."""
        mode = self.consensus if consensus is None else consensus
        mode = "on" if mode is True else (None if (not mode or mode == "off") else mode)
        if mode not in (None, "on", "samples", "beam"):
            raise RuntimeError(f"_sample: consensus must be a bool, 'off', 'samples' or 'beam', got {mode!r}")
        if mode is not None and self.consensus_table is None:
            raise RuntimeError("_sample: consensus selection needs model.consensus_table, a cvc.cider.CiderD (Trainer sets the "
                               "training captions' table); there is none")
        c_util = self.consensus_utility if consensus_utility is None else consensus_utility
        c_weights = self.consensus_weights if consensus_weights is None else consensus_weights
        c_alpha = self.consensus_alpha if consensus_alpha is None else float(consensus_alpha)
        if mode is not None:
            if c_weights not in ("uniform", "model"):
                raise RuntimeError(f"_sample: consensus_weights must be 'uniform' or 'model', got {c_weights!r}")
            if not (c_alpha >= 0.0) or c_alpha == float("inf"):
                raise RuntimeError(f"_sample: consensus_alpha must be a finite number >= 0, got {c_alpha!r}")
            if c_util is not None:
                from .. import metrics
                metrics.utility_coefficients(c_util, "_sample: consensus_utility")
        if encoded is not None:
            fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, pnt_mask = encoded
        else:
            fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, pnt_mask = self.encode_clips(
                segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, frm_mask, sample_idx, pnt_mask)
        feats = dict(fc_feats=fc_feats.contiguous(), conv_feats=conv_feats.contiguous(), p_conv_feats=p_conv_feats.contiguous(),
                     pool_feats=pool_feats.contiguous(), p_pool_feats=p_pool_feats.contiguous(), pnt_mask=pnt_mask)
        beam = self.beam_size if beam_size is None else int(beam_size)
        sampling = mode == "samples" or (self.sample_max if sample_max is None else int(sample_max)) == 0
        d_tau, d_n, d_seed = ((self.consensus_temperature, self.consensus_samples, self.consensus_seed) if mode == "samples" else
                              (self.sample_temperature, self.sample_n, self.sample_seed))
        tau = (d_tau if temperature is None else float(temperature)) if sampling else None
        n = (d_n if sample_n is None else int(sample_n)) if sampling else 1
        s_seed = (d_seed if seed is None else int(seed)) if sampling else None
        if mode == "samples":
            beam = 1
        # (the model's attribute is the default of a beam decode only: a sampling call that does not ask for it is left as it was)
        stoch = (self.stochastic_beam and not sampling) if stochastic_beam is None else bool(stochastic_beam)
        stau = self.stochastic_tau if stochastic_tau is None else float(stochastic_tau)
        if stoch and not sampling:
            s_seed = self.sample_seed if seed is None else int(seed)
        if mode is not None and c_weights == "model" and (sampling or stoch):
            raise RuntimeError("_sample: consensus_weights = 'model' weights the hypotheses of a beam by the model's probability; the "
                               "candidates of a sampling decode and of a stochastic beam are draws, whose uniform mean is the "
                               "expectation already -- use consensus_weights = 'uniform' there")
        if mode is not None and not (n > 1 if (sampling and mode != "beam") else (not sampling and beam > 1)):
            raise RuntimeError(f"_sample: consensus selection needs several candidates per clip -- sample_max = 0 with sample_n > 1, or "
                               f"beam_size > 1 without sampling (got consensus = {mode!r}, sampling = {sampling}, sample_n = {n}, "
                               f"beam_size = {beam})")
        k = (self.sample_top_k if top_k is None else int(top_k)) if sampling else 0
        p = (self.sample_top_p if top_p is None else float(top_p)) if sampling else 1.0
        wdtype = self.decode_weights_dtype if decode_weights is None else decode_weights
        cons = dict(no_repeat_ngram=self.no_repeat_ngram if no_repeat_ngram is None else no_repeat_ngram,
                    no_immediate_repeat=self.no_immediate_repeat if no_immediate_repeat is None else no_immediate_repeat,
                    min_len=self.min_caption_len if min_len is None else min_len,
                    ban_words=tuple(self.ban_words if ban_words is None else ban_words),
                    bad_endings=tuple(self.bad_endings if bad_endings is None else bad_endings))
        groups = self.beam_groups if beam_groups is None else int(beam_groups)
        lam = self.diversity_lambda if diversity_lambda is None else float(diversity_lambda)
        alpha = self.length_penalty if length_penalty is None else float(length_penalty)
        if force_words is None:
            if self.force_detected > 0:
                force_words = utils.detected_force_words(proposals, num, self.force_detected, self.opts.itod, self.opts.wtoi, self.unk_idx)
            elif self.force_words:
                force_words = self.force_words
        if force_words is not None and not isinstance(force_words, torch.Tensor):        # ids applied to every clip
            force_words = torch.tensor([int(w) for w in force_words], dtype=torch.int64).view(1, -1).expand(fc_feats.shape[0], -1)
        force_n = 0 if force_words is None else int(force_words.shape[-1])
        # "consensus on" is part of the key although it changes no argument of a sampling engine: a consensus call must not take
        # over the generator state of the previous call's engine (its candidates are what the same call draws without consensus)
        engine = self._decode_engine(
            "_engine_cache", feats, self.seq_length, extra=(mode is not None,) + ((
                tuple(sorted(c_util.items())) if c_util is not None else None, c_weights, c_alpha) if mode is not None else ()),
            may_bind=True, beam=beam, sample_n=n, temperature=tau,
            seed=s_seed, weights_dtype=wdtype, top_k=k, top_p=p,
            beam_history=beam > 1 and (any(cons.values()) or groups > 1 or lam != 0.0 or alpha != 0.0 or force_n > 0)
            or (beam > 1 and mode is not None) or stoch,      # (consensus chooses among hypotheses())
            beam_groups=groups, diversity=lam, length_penalty=alpha, force_n=force_n,
            **(dict(stochastic=True, stochastic_tau=stau) if stoch else {}), **cons)
        if force_n > 0:
            engine.load_force_words(force_words)
        res = engine.run()
        if stoch:
            self.last_stochastic = dict(zip(("seq", "score", "G", "logq"), (x.clone() for x in engine.hypotheses())))
            self.last_stochastic["state"] = engine.rng_state.clone()     # the generator words this decode drew with (scst_loss(wor=))
        if mode is not None:
            seq_c, att_c, logprob_c, pick, utility = engine.consensus(self.consensus_table, c_util, c_weights, c_alpha,
                                                                      want_pairs=bool(self.consensus_pairs))
            self.last_consensus = dict(candidates=(res[0] if sampling else engine.hypotheses()[0]).clone(), pick=pick, utility=utility,
                                       live=None if sampling else engine.consensus_live.view(engine.B, -1),
                                       weights=engine.consensus_logw)
            if self.consensus_pairs:
                self.last_consensus["pairs"] = engine.consensus_pairs
            return seq_c, att_c, logprob_c
        if sampling or (engine.constrained and beam == 1):
            return res[0].clone(), res[1].clone(), res[2].clone()
        return res[0].clone(), res[1].clone(), None

    # ------------------------------------------------------------------ teacher-forced decode (scoring, grounding on GT sentences)
    @torch.no_grad()
    def score(self, segs_feat, input_seq, gt_caption, num, proposals, gt_boxes, mask_boxes, region_feats, frm_mask, sample_idx,
              pnt_mask, captions: Optional[torch.Tensor] = None, grounding: bool = False, decode_weights: Optional[str] = None):
        """The decoder run over GIVEN words on the decode engine's forced mode (DecodeEngine forced_n; no autograd pass, eval()
        semantics): forward's 11 tensors, plus
        captions: [B, n, T] or [B * n, T] int64, n captions per clip (row b * n + j = caption j of clip b); None = the batch's
        ground-truth captions gt_caption[:, :seq_per_img].
        -> dict of clones: logprob [B * n, T] (the model's log-prob of every given word, full vocabulary), rank [B * n, T] int32
        (its rank among the logits, 0 = arg-max), mask [B * n, T] bool (the steps up to and including the first 0, as LMCriterion
        masks them), seq_logprob [B * n] (the masked sum), att [B * n, T, N] (post-softmax region attention).
        grounding=True (ground-truth captions only, n = seq_per_img = 1): the frame mask of every word's boxes is bound to the
        engine, and the dict also holds att2_weights [B, T, N] (frame-masked pre-softmax attention), ground_weights [B, T, N],
        roi_labels [B, T, N] and frm_mask_output [B, T, N + 1] -- the tensors debug_collect shows for the eval-mode training pass.
        decode_weights: "fp32" / "bf16" (argument, else opts.decode_weights), DecodeEngine's weights_dtype."""
        was_training = self.training
        self.eval()
        try:
            return self._score(segs_feat, input_seq, gt_caption, num, proposals, gt_boxes, mask_boxes, region_feats, frm_mask,
                               sample_idx, pnt_mask, captions, grounding, decode_weights)
        finally:
            self.train(was_training)

    def _score(self, segs_feat, input_seq, gt_caption, num, proposals, gt_boxes, mask_boxes, region_feats, frm_mask, sample_idx,
               pnt_mask, captions, grounding, decode_weights):
        T = self.seq_length
        B = proposals.size(0)
        if grounding and (captions is not None or self.seq_per_img != 1):
            raise RuntimeError("score(grounding=True) grounds the batch's ground-truth captions, one per clip: captions must be None "
                               f"and seq_per_img 1 (got seq_per_img = {self.seq_per_img})")
        if captions is None:
            captions = gt_caption[:, :self.seq_per_img, :]
        if captions.dim() == 3:
            if captions.size(0) != B:
                raise RuntimeError(f"score: captions [B, n, T] has {captions.size(0)} clips, the batch {B}")
            captions = captions.reshape(-1, captions.size(2))
        if captions.dim() != 2 or captions.size(1) != T or captions.size(0) % B or captions.dtype != torch.int64:
            raise RuntimeError(f"score: captions must be int64 [B, n, T] or [B * n, T] with B = {B}, T = {T}; got {captions.dtype} "
                               f"{tuple(captions.shape)}")
        n = captions.size(0) // B
        F_.new_step()
        overlaps, (fc_feats, conv_feats, p_conv_feats, pool_feats, p_pool_feats, g_pool_feats, pnt_mask, _o, _c, _l) = self._encode(
            segs_feat, proposals, num, mask_boxes, region_feats, gt_boxes, frm_mask, sample_idx, pnt_mask)
        feats = dict(fc_feats=fc_feats.contiguous(), conv_feats=conv_feats.contiguous(), p_conv_feats=p_conv_feats.contiguous(),
                     pool_feats=pool_feats.contiguous(), p_pool_feats=p_pool_feats.contiguous(), pnt_mask=pnt_mask)
        step_fmask = None
        if grounding:
            # label glue exactly as _forward_3_loops does it: per-word proposal labels and the frame mask on proposals
            roi_labels, frm_mask_output, step_fmask = hip.label_glue(overlaps, mask_boxes[:, 0, :, 1:T + 1], frm_mask, pnt_mask)
        wdtype = self.decode_weights_dtype if decode_weights is None else decode_weights
        captions = captions.contiguous()
        # one forced engine per batch shape, in a slot of its own: a score call between two _sample calls evicts nothing there
        # (the frame mask is part of the launch list: it is bound before capture, and grounding is part of the key)
        engine = self._decode_engine("_score_cache", feats, T, extra=(bool(grounding),), forced_n=n, weights_dtype=wdtype,
                                     prepare=lambda e: e.load_captions(captions, step_fmask))
        _seq, att, logprob, rank = engine.run()
        first0 = (captions == 0).long().cumsum(1)
        mask = (first0 == 0) | ((first0 == 1) & (captions == 0))           # steps up to and including the first 0 (LMCriterion)
        logprob = logprob.clone()
        out = dict(logprob=logprob, rank=rank.clone(), mask=mask, seq_logprob=logprob.masked_fill(~mask, 0.0).sum(1), att=att.clone())
        if grounding:
            att2_weights = engine.fm_steps.transpose(0, 1).clone()                    # [B, T, N] pre-softmax, frame-masked
            xt_clamp = torch.clamp(input_seq.view(-1, input_seq.size(2), input_seq.size(3))[:, 1:T + 1, 0].clone() - self.vocab_size, min=0)
            xt_all = self._vis_embed(xt_clamp)
            if hasattr(self.roi_feat_extractor, 'vis_classifiers_bias'):
                bias = self.roi_feat_extractor.vis_classifiers_bias[xt_clamp].type(xt_all.type()).unsqueeze(2).expand(
                    B, T, pool_feats.size(1))
            else:
                bias = 0
            ground_weights = self._grounder(xt_all, g_pool_feats, frm_mask_output[:, :, 1:], bias + att2_weights)
            out.update(att2_weights=att2_weights, ground_weights=ground_weights.clone(), roi_labels=roi_labels.clone(),
                       frm_mask_output=frm_mask_output.clone())
        return out
