"""Criteria, label glue and small helpers -- the parts of the reference's misc/utils.py the
caption hot path touches: LMCriterion / LanguageCriterion
(misc/utils.py:127-192), bbox_overlaps / bbox_target (:335-373), update_values (:58-63),
decode_sequence (:100-116), AverageMeter (:501-517).  The dead NBT image utilities are not
reproduced.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import functional as F_


def update_values(dict_from, dict_to):
    """YAML overlay: non-None values of dict_from win, recursively (reference :58-63)."""
    for key, value in dict_from.items():
        if isinstance(value, dict):
            update_values(dict_from[key], dict_to[key])
        elif value is not None:
            dict_to[key] = dict_from[key]


def decode_sequence(itow, itod, ltow, itoc, wtod, seq, vocab_size, opt):
    """Word indices -> sentences, stopping at the first 0 (reference :100-116; the unused
    detection-vocabulary arguments are kept for signature compatibility)."""
    out = []
    for row in seq.tolist():
        words = []
        for ix in row:
            if ix == 0:
                break
            words.append(itow[str(ix)])
        # the reference emits a separating blank before it sees the terminating 0
        txt = ' '.join(words)
        if len(words) < len(row) and len(words) > 0:
            txt += ' '
        out.append(txt)
    return out


def detected_force_words(proposals, num, C, itod, wtoi, unk_idx):
    """The words to force per clip from its detections (DecodeEngine.load_force_words): proposals [B, P, 7] with the columns the
    data loader documents (class at 5, score at 6), num [B, 7] with the count of valid proposals at 1.  Of the clip's valid proposals'
    classes whose itod name is a single word of the vocabulary wtoi other than UNK and word 0, the C distinct ones with the
    highest proposal score, ties to the lower class index.  -> [B, C] int64 on the host, missing entries -1."""
    props, num = torch.as_tensor(proposals).detach().cpu(), torch.as_tensor(num).detach().cpu()
    out = torch.full((props.shape[0], int(C)), -1, dtype=torch.int64)
    for b in range(props.shape[0]):
        best = {}
        for p in props[b, :max(0, min(int(num[b, 1]), props.shape[1]))].tolist():
            cls = int(p[5])
            name = itod.get(str(cls), itod.get(cls))
            if name is None or name not in wtoi or int(wtoi[name]) in (0, int(unk_idx)):
                continue
            best[cls] = max(best.get(cls, float("-inf")), float(p[6]))
        for j, cls in enumerate(sorted(best, key=lambda c: (-best[c], c))[:int(C)]):
            out[b, j] = int(wtoi[itod.get(str(cls), itod.get(cls))])
    return out


def word_class_table(opts):
    """[vocab_size] int32 on the host: word id -> the detection class (an index of itod, >= 1) a generated word is grounded as, 0 for
    every other id -- the rule Trainer._collect_grounding applies word by word: the word's lemma (wtol) is the lemma of a detection
    class name (wtod).  Built once per trainer; the grounding kernel (cvc.metrics.grounding) reads it on the device."""
    lemma_det = {opts.wtol[k]: i for k, i in opts.wtod.items() if k in opts.wtol}
    table = torch.zeros(int(opts.vocab_size), dtype=torch.int32)
    for ix, word in opts.itow.items():
        ix = int(ix)
        lemma = opts.wtol.get(word)
        if 0 < ix < table.numel() and lemma in lemma_det:
            table[ix] = int(lemma_det[lemma])
    return table


def _text_mask(target):
    m = target.gt(0)
    return torch.cat([torch.ones_like(m[:, :1]), m[:, :-1]], 1)   # includes the first EOS (:135-137)


def _masked_nll_mean(txt_input, target, label_smoothing=0.0):
    mask = _text_mask(target)
    w = mask.reshape(-1).to(torch.float32)
    total = F_.masked_nll_sum(txt_input, target.reshape(-1), w, label_smoothing=label_smoothing)
    count = w.sum()
    return (total / count).reshape(())


def _distill_rows(distill, target, t_major, row_weight):
    """a criterion's distill=(teacher_rows [T, B, V], alpha, tau) as cvc.functional takes it for rows in the criterion's order: the
    teacher's rows are t-major (row t * B + b, the order the forced decode engine writes them in), so a b-major criterion gets the
    int32 row map b * T + t -> t * B + b"""
    if row_weight is not None:
        raise ValueError("distill cannot be combined with row_weight: a self-critical step is not distilled")
    if not isinstance(distill, (tuple, list)) or len(distill) != 3:
        raise ValueError(f"distill: expected (teacher_rows, alpha, tau), got {type(distill).__name__}")
    rows, alpha, tau = distill
    B, T = target.shape
    if not isinstance(rows, torch.Tensor) or rows.dim() != 3 or tuple(rows.shape[:2]) != (T, B):
        raise ValueError(f"distill: teacher_rows must be [T = {T}, B = {B}, V], got "
                         f"{tuple(rows.shape) if isinstance(rows, torch.Tensor) else type(rows).__name__}")
    if t_major:
        return rows, alpha, tau
    row_map = torch.arange(B * T, device=target.device, dtype=torch.int32).view(T, B).t().reshape(-1)
    return rows, alpha, tau, row_map


def _masked_nll_mean_from_logits(logits, target, t_major=False, row_weight=None, label_smoothing=0.0, want_nll=False,
                                 entropy_beta=None, want_entropy=False, distill=None):
    """Same value as _masked_nll_mean(log_softmax(logits), target), plus the per-row argmax, from one fused pass.
    t_major: the rows of `logits` are ordered t * B + b (the C-driven training loops' outputs) instead of b * T + t.
    row_weight, label_smoothing, want_nll, entropy_beta, want_entropy, distill: see _masked_nll_mean_from_head."""
    w = _text_mask(target).to(torch.float32)
    count = w.sum()
    ent = ()
    if distill is not None:
        kd = _distill_rows(distill, target, t_major, row_weight)
        tf, wf = (target.t().reshape(-1), w.t().reshape(-1)) if t_major else (target.reshape(-1), w.reshape(-1))
        total, argmax, nll, k = F_.vocab_nll(logits, tf, wf, label_smoothing=label_smoothing, return_nll=True, entropy_beta=entropy_beta,
                                             return_entropy=want_entropy, distill=kd, return_kd=True)
        ent = ((k / count).reshape(()),)
    elif entropy_beta is not None or want_entropy:
        tf, wf = (target.t().reshape(-1), w.t().reshape(-1)) if t_major else (target.reshape(-1), w.reshape(-1))
        total, argmax, nll, h = F_.vocab_nll(logits, tf, wf if row_weight is None else row_weight.reshape(-1),
                                             label_smoothing=0.0 if row_weight is not None else label_smoothing, return_nll=True,
                                             entropy_beta=entropy_beta, entropy_weight=wf, return_entropy=True)
        ent = ((h / count).reshape(()),) if want_entropy else ()
    elif row_weight is not None:
        total, argmax = F_.vocab_nll(logits, (target.t() if t_major else target).reshape(-1), row_weight.reshape(-1))
        nll = total.detach()
    elif t_major:
        total, argmax, nll = F_.vocab_nll(logits, target.t().reshape(-1), w.t().reshape(-1), label_smoothing=label_smoothing,
                                          return_nll=True)
    else:
        total, argmax, nll = F_.vocab_nll(logits, target.reshape(-1), w.reshape(-1), label_smoothing=label_smoothing, return_nll=True)
    res = ((total / count).reshape(()), argmax.view(target.shape[1], target.shape[0]).t() if t_major else argmax.view(target.shape))
    return (*res, *(((nll / count).reshape(()),) if want_nll else ()), *ent)


def _masked_nll_mean_from_head(x, weight, bias, target, t_major=False, done=None, compute_only=False, row_weight=None,
                               label_smoothing=0.0, want_nll=False, entropy_beta=None, want_entropy=False, distill=None):
    """_masked_nll_mean_from_logits(x W^T + b, target) with the criterion folded into the vocabulary head's GEMM finish: the logits
    are never materialised (cvc.functional.vocab_head_nll); falls back to the two-step form for shapes that kernel does not take.
    row_weight: a real weight per row of x (in x's row order, any sign, 0 where the loss mask is 0) in place of the 0 / 1 loss mask:
    -sum_r row_weight[r] log p(target[r]) / sum(mask) -- the self-critical loss, row_weight = advantage x mask.  None: the mask.
    label_smoothing: eps in [0, 1), the target distribution (1 - eps) onehot + eps / V (cvc.functional.vocab_head_nll).  The
    self-critical loss IGNORES it: with row_weight the criterion is the one-hot one whatever eps is, because REINFORCE's gradient
    is advantage x grad log p(sampled word) -- it needs the log-prob itself, not a regularised target.
    want_nll: a further result, the UNSMOOTHED mean as a scalar without a graph (the figure to log beside a smoothed loss).
    entropy_beta: beta (finite, any sign) adds -beta sum_r mask[r] H[r] / sum(mask) to the loss, H the entropy of the row's softmax
    (the model's full-vocabulary distribution at temperature 1, not a sampler's tempered, truncated or UNK-free one): an entropy
    bonus with row_weight, a confidence penalty without.  The entropy weight is always the loss mask of `target`, in x's row
    order; it applies with row_weight too (label smoothing does not).  None: today's launches; 0: the entropy is computed and
    nothing else changes.
    want_entropy: a last result, the mean entropy sum_r mask[r] H[r] / sum(mask) as a scalar without a graph.
    distill = (teacher_rows [T, B, V] fp32 log-scale scores in the forced decode engine's t-major order, alpha, tau): word-level
    distillation, the loss (1 - alpha) x the mean NLL + alpha tau^2 x the mean masked KL(teacher || student) at temperature tau
    (cvc.functional.vocab_head_nll); refused with row_weight, label_smoothing > 0 or entropy_beta (ValueError).  With it want_nll is the
    UNMIXED mean NLL and the last result is the unmixed mean tau^2 KL, a scalar without a graph.  None: today's launches."""
    if distill is not None:
        distill = (*_distill_rows(distill, target, True, row_weight)[:3],)       # (checked once; the row map is made where it is needed)
    if row_weight is not None:
        label_smoothing = 0.0
    if not F_.vocab_head_nll_ok(x, weight):
        return _masked_nll_mean_from_logits(F_.linear(x, weight, bias), target, t_major, row_weight=row_weight,
                                            label_smoothing=label_smoothing, want_nll=want_nll, entropy_beta=entropy_beta,
                                            want_entropy=want_entropy, distill=distill)
    # the loss mask, its count and the t-major copies depend on the target alone: both heads of a cyclical pass (decode,
    # reconstruction) score against the same target tensor, so they are formed once and kept on it
    pre = getattr(target, "_cvc_nll_pre", None)
    if pre is None or pre[0] != (target._version, t_major):
        w = _text_mask(target).to(torch.float32)
        tf, wf = (target.t().reshape(-1), w.t().reshape(-1)) if t_major else (target.reshape(-1), w.reshape(-1))
        pre = ((target._version, t_major), tf.contiguous(), wf.contiguous(), w.sum())
        target._cvc_nll_pre = pre
    _, tf, wf, count = pre
    ent = dict(entropy_beta=entropy_beta, entropy_weight=wf, return_entropy=True) if entropy_beta is not None or want_entropy else {}
    if distill is not None:
        ent = dict(ent, entropy_beta=entropy_beta, return_entropy=want_entropy, distill=_distill_rows(distill, target, t_major, None))
        want_entropy = True                      # (the last result below: the KD mean in the entropy's place -- never both)
    if row_weight is not None:
        wf = row_weight.reshape(-1).contiguous()
    if compute_only:       # -> (opaque result for a later call with done=, the argmax words)
        done = F_.vocab_head_nll_compute(x, weight, bias, tf, wf, label_smoothing=label_smoothing, **ent)
        argmax = done[1]
        return done, (argmax.view(target.shape[1], target.shape[0]).t() if t_major else argmax.view(target.shape))
    if distill is not None:
        ent["return_kd"] = True
    total, argmax, nll, *h = F_.vocab_head_nll(x, weight, bias, tf, wf, done, label_smoothing=label_smoothing, return_nll=True, **ent)
    res = ((total / count).reshape(()), argmax.view(target.shape[1], target.shape[0]).t() if t_major else argmax.view(target.shape))
    return (*res, *(((nll / count).reshape(()),) if want_nll else ()), *(((h[0] / count).reshape(()),) if want_entropy else ()))


def _opt_label_smoothing(opt, label_smoothing):
    """the criteria's eps: the constructor argument, else opt.label_smoothing, else 0; validated (ValueError outside [0, 1))"""
    from .. import hip
    if label_smoothing is None:
        label_smoothing = getattr(opt, "label_smoothing", 0.0) if opt is not None else 0.0
    return hip.check_label_smoothing(0.0 if label_smoothing is None else label_smoothing)


def _opt_confidence_penalty(opt, confidence_penalty):
    """the criteria's entropy coefficient: the constructor argument, else opt.confidence_penalty, else None (off: today's launches);
    validated (ValueError unless finite)"""
    from .. import hip
    if confidence_penalty is None:
        confidence_penalty = getattr(opt, "confidence_penalty", None) if opt is not None else None
    return None if confidence_penalty is None else hip.check_entropy_beta(confidence_penalty, "confidence_penalty")


class LMCriterion(nn.Module):
    """reference misc/utils.py:127-172.  label_smoothing (argument, else opt.label_smoothing, else 0): the language loss is the
    smoothed cross entropy of torch.nn.functional.cross_entropy(label_smoothing=); after a from_logits / from_head call with it > 0
    last_nll is the UNSMOOTHED mean NLL of that call (a device scalar without a graph), else None.
    confidence_penalty (argument, else opt.confidence_penalty, else None): beta adds -beta x the mean masked entropy of the word
    distribution to the language loss (Pereyra et al. 2017; beta > 0 penalises confident distributions); after a from_logits /
    from_head call with it not None (0: only measured) last_entropy is that mean entropy (a device scalar without a graph), else
    None.  The log-prob form forward() has no entropy term."""

    def __init__(self, opt, label_smoothing=None, confidence_penalty=None):
        super().__init__()
        self.vocab_size = opt.vocab_size
        self.label_smoothing = _opt_label_smoothing(opt, label_smoothing)
        self.confidence_penalty = _opt_confidence_penalty(opt, confidence_penalty)
        self.last_nll = None
        self.last_entropy = None
        self.last_kd = None

    def _keep(self, res, distill=None):
        """(loss, argmax[, unsmoothed / unmixed mean -- asked for when smoothing is on or a teacher is given][, mean entropy -- when the
        penalty is not None][, mean KD -- when a teacher is given]) -> (loss, argmax); the others stay on the module"""
        rest = list(res[2:])
        self.last_nll = rest.pop(0) if self.label_smoothing > 0 or distill is not None else None
        self.last_entropy = rest.pop(0) if self.confidence_penalty is not None and distill is None else None
        self.last_kd = rest.pop(0) if distill is not None else None
        return res[0], res[1]

    def _ent(self):
        return dict(entropy_beta=self.confidence_penalty, want_entropy=self.confidence_penalty is not None)

    def forward(self, txt_input, att2_weights, ground_weights, target, att2_target, input_seq):
        if not torch.cuda.is_current_stream_capturing():
            assert torch.sum(target >= self.vocab_size) == 0                  # reference :134 (host check; skipped under capture)
        loss = _masked_nll_mean(txt_input, target, self.label_smoothing)
        return (loss, *self.attention_losses(att2_weights, ground_weights, att2_target))

    def from_logits(self, logits, att2_weights, ground_weights, target, att2_target, input_seq, t_major=False, distill=None):
        """forward() fed raw logits instead of log-probs: -> (lm_loss, att2_loss, ground_loss, argmax [B, T]).
        SURVEY section 8(f) rank 2: the criterion folded into the vocabulary head's epilogue pass.
        distill = (teacher_rows [T, B, V], alpha, tau): see from_head."""
        if not torch.cuda.is_current_stream_capturing():
            assert torch.sum(target >= self.vocab_size) == 0
        loss, argmax = self._keep(_masked_nll_mean_from_logits(logits, target, t_major, label_smoothing=self.label_smoothing,
                                                               want_nll=self.label_smoothing > 0 or distill is not None, distill=distill,
                                                               **self._ent()), distill)
        return (loss, *self.attention_losses(att2_weights, ground_weights, att2_target), argmax)

    def from_head(self, x, head, att2_weights, ground_weights, target, att2_target, input_seq, t_major=False, done=None, row_weight=None,
                  distill=None):
        """from_logits() fed the vocabulary head's INPUT x [rows, R] and the head module (nn.Linear): the head's GEMM and the
        criterion run as one op, no logits tensor.  done: head_words()'s first result for the same x (the arithmetic then is not
        repeated).  row_weight: the self-critical loss, which ignores label smoothing (_masked_nll_mean_from_head).
        distill = (teacher_rows [T, B, V], alpha, tau): word-level distillation (_masked_nll_mean_from_head); last_nll and last_kd then
        are the unmixed mean NLL and the unmixed mean tau^2 KL of the call.  Refused with row_weight, label smoothing or the confidence
        penalty (ValueError)."""
        if not torch.cuda.is_current_stream_capturing():
            assert torch.sum(target >= self.vocab_size) == 0
        loss, argmax = self._keep(_masked_nll_mean_from_head(x, head.weight, head.bias, target, t_major, done=done, row_weight=row_weight,
                                                             label_smoothing=self.label_smoothing,
                                                             want_nll=self.label_smoothing > 0 or distill is not None, distill=distill,
                                                             **self._ent()), distill)
        return (loss, *self.attention_losses(att2_weights, ground_weights, att2_target), argmax)

    def head_words(self, x, head, target, t_major=False, distill=None):
        """the head + criterion arithmetic of from_head() ahead of its graph node: -> (done, argmax words [B, T]), or None for
        shapes the fused head does not take.  distill: as from_head (the `done` carries its alpha and tau)"""
        if not F_.vocab_head_nll_ok(x, head.weight):
            return None
        return _masked_nll_mean_from_head(x, head.weight, head.bias, target, t_major, compute_only=True,
                                          label_smoothing=self.label_smoothing, entropy_beta=self.confidence_penalty, distill=distill)

    @staticmethod
    def attention_losses(att2_weights, ground_weights, att2_target):
        # supervised attention / grounding losses (w_att2 = 0 by default).  The reference
        # branches on `att2_target.sum() != 0` and uses masked_select (:150-162); the same value without a host round
        # trip or a data-dependent shape: -sum(log_softmax * target) / max(count, 1), which is 0 when nothing is labelled.
        if att2_weights.is_cuda and att2_weights.dtype == torch.float32 and ground_weights.dtype == torch.float32 \
                and att2_weights.dim() == 3 and att2_weights.stride(2) == 1 and ground_weights.stride(2) == 1:
            # both criteria of all T steps from one kernel pair (csrc/label_glue.hip), no library log_softmax / masked sums
            return F_.attn_nll(att2_weights, ground_weights, att2_target)
        tgt = att2_target.to(att2_weights.dtype)
        count = tgt.sum().clamp(min=1.0)
        att2_loss = (-(F.log_softmax(att2_weights, dim=2) * tgt).sum() / count).reshape(1)
        ground_loss = (-(F.log_softmax(ground_weights, dim=2) * tgt).sum() / count).reshape(1)
        return att2_loss, ground_loss


class LanguageCriterion(nn.Module):
    """reference misc/utils.py:175-192.  label_smoothing (argument, else opt.label_smoothing, else 0): as LMCriterion; a call with
    row_weight (the self-critical loss) ignores it.  confidence_penalty (argument, else opt.confidence_penalty, else None): as
    LMCriterion, for the calls without row_weight; a call with row_weight takes its own entropy_beta (the self-critical loss's entropy
    bonus) instead.  last_entropy: the mean masked entropy of the last from_logits / from_head call whose coefficient was not None
    (a device scalar without a graph), else None."""

    def __init__(self, opt=None, label_smoothing=None, confidence_penalty=None):
        super().__init__()
        self.label_smoothing = _opt_label_smoothing(opt, label_smoothing)
        self.confidence_penalty = _opt_confidence_penalty(opt, confidence_penalty)
        self.last_entropy = None

    def forward(self, txt_input, target):
        return _masked_nll_mean(txt_input, target, self.label_smoothing)

    def _keep(self, res, beta):
        self.last_entropy = res[2] if beta is not None else None
        return res[0]

    def from_logits(self, logits, target, t_major=False):
        beta = self.confidence_penalty
        return self._keep(_masked_nll_mean_from_logits(logits, target, t_major, label_smoothing=self.label_smoothing, entropy_beta=beta,
                                                       want_entropy=beta is not None), beta)

    def from_head(self, x, head, target, t_major=False, row_weight=None, entropy_beta=None):
        beta = self.confidence_penalty if row_weight is None else entropy_beta
        if beta is not None and row_weight is not None:
            from .. import hip
            beta = hip.check_entropy_beta(beta)
        return self._keep(_masked_nll_mean_from_head(x, head.weight, head.bias, target, t_major, row_weight=row_weight,
                                                     label_smoothing=self.label_smoothing, entropy_beta=beta,
                                                     want_entropy=beta is not None), beta)


def bbox_overlaps(rois, gt_box, frm_mask):
    """IoU of proposals [B,N,>=5] vs GT boxes [B,K,>=5] (reference :335-338 ->
    misc/bbox_transform.py:224-272): +1-pixel convention, zero where frm_mask, 0 for degenerate GT
    boxes, -1 for degenerate proposals."""
    a, g = rois[:, :, :4], gt_box[:, :, :4]
    gx, gy = g[:, :, 2] - g[:, :, 0] + 1, g[:, :, 3] - g[:, :, 1] + 1
    ax, ay = a[:, :, 2] - a[:, :, 0] + 1, a[:, :, 3] - a[:, :, 1] + 1
    iw = (torch.min(a[:, :, None, 2], g[:, None, :, 2]) - torch.max(a[:, :, None, 0], g[:, None, :, 0]) + 1).clamp(min=0)
    ih = (torch.min(a[:, :, None, 3], g[:, None, :, 3]) - torch.max(a[:, :, None, 1], g[:, None, :, 1]) + 1).clamp(min=0)
    inter = iw * ih
    ov = inter / ((ax * ay).unsqueeze(2) + (gx * gy).unsqueeze(1) - inter)
    ov = ov * (~frm_mask).to(ov.dtype)
    ov = ov.masked_fill(((gx == 1) & (gy == 1)).unsqueeze(1).expand_as(ov), 0)
    ov = ov.masked_fill(((ax == 1) & (ay == 1)).unsqueeze(2).expand_as(ov), -1)
    return ov


def bbox_target(mask, overlaps, seq, seq_update, vocab_size):
    """Per-word proposal labels (reference :351-373): proposal n is positive for the word if it
    overlaps (IoU > 0.5) a GT box that grounds the word.  Also reproduces the (deprecated)
    seq_update side effect."""
    B = overlaps.size(0)
    ov = overlaps.masked_fill(mask.reshape(B, 1, -1).expand_as(overlaps), 0)
    labels = ov.max(2)[0] > 0.5
    no_proposal_idx = (labels.sum(1) > 0) != (seq[:, 2] > 0)
    # same writes as the reference's guarded block, expressed without a host-side `if .sum() > 0` (a
    # device->host sync per decode step that would keep the launch queue from running ahead)
    seq_update[:, 0] = torch.where(no_proposal_idx, seq_update[:, 3], seq_update[:, 0])
    seq_update[:, 1] = torch.where(no_proposal_idx, torch.zeros_like(seq_update[:, 1]), seq_update[:, 1])
    seq_update[:, 2] = torch.where(no_proposal_idx, torch.zeros_like(seq_update[:, 2]), seq_update[:, 2])
    return labels


class AverageMeter(object):
    """reference :501-517"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def set_tb_logger(log_dir, exp_name, resume):
    """TensorBoard writer if tensorboardX / torch.utils.tensorboard is importable, else None
    (the reference hard-requires tensorboardX, cycle_utils.py:14-23)."""
    import os
    import shutil
    path = log_dir + '/' + exp_name
    if not resume and os.path.exists(path):
        shutil.rmtree(path, ignore_errors=True)
    try:
        from tensorboardX import SummaryWriter
    except ImportError:
        try:
            from torch.utils.tensorboard import SummaryWriter
        except ImportError:
            return None
    return SummaryWriter(log_dir=path)
