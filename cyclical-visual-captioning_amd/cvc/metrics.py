"""Caption metrics from token overlap alone, on the device: BLEU-1..4 and ROUGE-L (csrc/overlap.hip) next to CIDEr-D (cvc.cider), for
validation loops that have none of the external toolkits (Trainer(device_metrics=True), cvc.main --val_metrics device) and for reward
mixes of self-critical training (cvc.main --scst_reward).

Definitions (what csrc/overlap.hip computes and tests/overlap_ref.py restates):

* a caption is a row of T <= 63 word ids in [0, 65534]; for BLEU and ROUGE-L its words are the ids BEFORE its first 0 -- the end mark
  is no word, what stands behind it is ignored, without a 0 all T ids count; L = 0 is possible.  (CIDEr-D here counts the end mark.)
* BLEU statistics (exact integers), n = 1..4: guess_n = max(0, Lc - n + 1); correct_n = sum over the candidate's distinct n-grams of
  min(count_c, max_r count_r); cand_len = Lc; ref_len = the counted reference length closest to Lc, the shorter on a tie, 0 without
  a reference.
* sentence BLEU_k (fp32, device) = bp * exp((sum_{n<=k} log p_n) / k), p_n = (correct_n + 1e-15) / (guess_n + 1e-9), bp = 1 if
  Lc >= ref_len else exp(1 - ref_len / Lc); 0 when Lc = 0 or the clip has no reference.
* corpus BLEU_k: the same formula on the column sums of the statistics over all captions, in fp64 on the host (corpus_bleu).
* ROUGE-L, beta = 1.2: p = max_r lcs_r / Lc, q = max_r lcs_r / Lr (Lr = 0: 0), (1 + beta^2) p q / (q + beta^2 p); 0 when Lc = 0,
  no reference, or p q = 0.  Corpus value: the mean over the captions.

These are NOT the toolkit's numbers: no PTB tokenizer is applied (the ids are the dataset's tokens, UNK is a word like any other),
CIDEr-D counts the end mark, METEOR and SPICE are not attempted.

Further down: the grounding scores of the generated captions (csrc/grounding.hip; grounding, grounding_result, GroundingScorer) --
F1_all / F1_loc in the manner of ActivityNet-Entities, for Trainer.eval with the device metrics and --eval_obj_grounding both on.
At the end: the diversity of a clip's caption SET (csrc/diversity.hip; set_diversity, DiversityScorer) -- Div-1, Div-2, mBLEU, distinct
captions, next to the set's oracle and mean CIDEr-D -- and the set's spectral diversity (csrc/spectrum.hip; set_spectrum,
SpectrumScorer): Self-CIDEr and LSA-based diversity from the eigenvalues of the captions' similarity matrix.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

TINY, SMALL = 1e-15, 1e-9
REWARD_NAMES = ("cider", "bleu1", "bleu2", "bleu3", "bleu4", "rougel")       # the fixed order in which a reward mix is added
KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")         # the toolkits' names


def overlap(cand: torch.Tensor, refs: torch.Tensor, nref: torch.Tensor, per_clip: Optional[int] = None, want_lcs: bool = False) -> dict:
    """cand [rows, T] int64 on the device; refs [clips, Rmax, T] int64 (per_clip = rows / clips consecutive candidates per clip); nref
    [clips]: how many of a clip's Rmax reference rows count.  -> dict(stats [rows, 10] int32: correct_1..4, guess_1..4, cand_len,
    ref_len; bleu [rows, 4] fp32; rouge [rows] fp32 (; lcs [rows, Rmax] int32, -1 in slots >= nref)), all on the device."""
    from . import hip
    from .cider import MAX_T
    if cand.shape[1] > MAX_T:
        raise RuntimeError(f"metrics.overlap: T = {cand.shape[1]}; the kernel takes at most T = {MAX_T} (one lane per position)")
    stats, lcs, bleu, rouge = hip.caption_overlap(cand.contiguous(), refs.contiguous(), nref.to(torch.int32).contiguous(), per_clip,
                                                  want_lcs)
    out = dict(stats=stats, bleu=bleu, rouge=rouge)
    if want_lcs:
        out["lcs"] = lcs
    return out


def corpus_bleu(stats_sum) -> np.ndarray:
    """the ten summed statistics (correct_1..4, guess_1..4, cand_len, ref_len) -> corpus BLEU_1..4, fp64 on the host; zeros when no
    candidate word was counted"""
    s = np.asarray(stats_sum.detach().cpu().numpy() if isinstance(stats_sum, torch.Tensor) else stats_sum, dtype=np.float64).reshape(10)
    out = np.zeros(4, dtype=np.float64)
    cand_len, ref_len = s[8], s[9]
    if cand_len <= 0:
        return out
    bp = 1.0 if cand_len >= ref_len else math.exp(1.0 - ref_len / cand_len)
    logs = 0.0
    for n in range(4):
        logs += math.log((s[n] + TINY) / (s[4 + n] + SMALL))
        out[n] = bp * math.exp(logs / (n + 1))
    return out


def parse_reward_weights(spec: str, flag: str = "--scst_reward") -> dict:
    """"cider:1,bleu4:0.5,rougel:0.5" -> {name: weight} in the fixed order of REWARD_NAMES (names that are not given: absent).  An
    unknown name, a repeated name, a weight that is no number or negative, or an empty mix is a SystemExit that says so, naming
    `flag`, the switch the spec came from (--consensus_utility is parsed here too)."""
    got = {}
    for item in (x.strip() for x in (spec or "").split(",")):
        if not item:
            continue
        name, sep, val = item.partition(":")
        name = name.strip().lower()
        if name not in REWARD_NAMES:
            raise SystemExit(flag + ": unknown metric %r (known: %s)" % (name, ", ".join(REWARD_NAMES)))
        if name in got:
            raise SystemExit(flag + ": %r is given twice" % name)
        try:
            w = float(val) if sep else 1.0
        except ValueError:
            raise SystemExit(flag + ": the weight of %r, %r, is not a number" % (name, val))
        if not (w >= 0.0) or math.isinf(w):
            raise SystemExit(flag + ": the weight of %r must be a finite number >= 0, got %r" % (name, val))
        got[name] = w
    if not got:
        raise SystemExit(flag + ": no metric given")
    return {k: got[k] for k in REWARD_NAMES if k in got}


def is_cider_only(weights: Optional[dict]) -> bool:
    """True for the reward self-critical training has had all along: CIDEr-D with weight 1 and nothing else weighted"""
    if not weights:
        return True
    return float(weights.get("cider", 0.0)) == 1.0 and all(float(w) == 0.0 for k, w in weights.items() if k != "cider")


def reward_mix(weights: dict, table, seq: torch.Tensor, refs: torch.Tensor, nref: torch.Tensor):
    """reward = sum_k w_k * metric_k over the names with a non-zero weight, added in the order of REWARD_NAMES, fp32 torch ops on the
    device; the weights apply to the raw scales (CIDEr-D in [0, 10], the others in [0, 1]).  -> (reward [rows], {name: metric [rows]})"""
    parts = {}
    ov = None
    for name in REWARD_NAMES:
        if float(weights.get(name, 0.0)) == 0.0:
            continue
        if name == "cider":
            parts[name] = table.score(seq, refs, nref)
            continue
        if ov is None:
            ov = overlap(seq, refs, nref)
        parts[name] = ov["rouge"] if name == "rougel" else ov["bleu"][:, int(name[4]) - 1].contiguous()
    reward = None
    for name, m in parts.items():
        term = m * float(weights[name])
        reward = term if reward is None else reward + term
    if reward is None:
        reward = torch.zeros(seq.shape[0], device=seq.device, dtype=torch.float32)
    return reward, parts


def utility_coefficients(utility: dict, who: str = "metrics.consensus") -> list:
    """a utility mix in parse_reward_weights' form -> its six coefficients in the order of REWARD_NAMES; an unknown name, a weight that
    is negative or not finite, or a mix without a positive weight raises RuntimeError"""
    unknown = [k for k in (utility or {}) if k not in REWARD_NAMES]
    if unknown:
        raise RuntimeError(f"{who}: utility names unknown metrics {unknown} (known: {', '.join(REWARD_NAMES)})")
    coef = [float((utility or {}).get(k, 0.0)) for k in REWARD_NAMES]
    if any(not (c >= 0.0) or math.isinf(c) for c in coef):
        raise RuntimeError(f"{who}: utility weights must be finite numbers >= 0, got {dict(utility)}")
    if not any(c > 0.0 for c in coef):
        raise RuntimeError(f"{who}: utility weights nothing -- give at least one of {', '.join(REWARD_NAMES)} a weight > 0")
    return coef


def consensus(cand: torch.Tensor, per_clip: int, utility: dict, table=None, log_weights: Optional[torch.Tensor] = None,
              live: Optional[torch.Tensor] = None, want_pairs: bool = False) -> dict:
    """Consensus (minimum-Bayes-risk) selection under a mix of utilities and weighted candidates (csrc/consensus_mix.hip; DESIGN
    section 7, "Weighted candidates and utility mixes").  cand [rows, T] int64 on the device, per_clip consecutive candidates per clip;
    utility: {name: weight} over REWARD_NAMES (parse_reward_weights' form); table: a cvc.cider.CiderD, needed when cider is weighted;
    log_weights [rows] (None: uniform): the candidates' log-weights as references, e.g. alpha * the model's log-prob of the caption;
    live [rows] (None: every row counts).
      u(i, j) = sum_k weight_k * metric_k(row i as the candidate, row j as its only reference), added in the order of REWARD_NAMES
      utility[i] = sum_j w_j u(i, j) / sum_j w_j over the clip's other live rows, w_j = exp(logw_j - max logw)
    -> dict(utility [rows] fp32, pick [clips] int32 (the first live row with the largest utility), best [clips, T] int64 (, pairs
    [clips, per_clip, per_clip, 6] fp32: the raw pair metrics)), all on the device: one launch, no host read."""
    from . import hip
    from .cider import MAX_T, MAX_PER_CLIP
    coef = utility_coefficients(utility)
    if cand.dim() != 2 or cand.shape[1] > MAX_T:
        raise RuntimeError(f"metrics.consensus: cand {tuple(cand.shape)}; the kernel takes rows of at most T = {MAX_T} words")
    if int(per_clip) > MAX_PER_CLIP:
        raise RuntimeError(f"metrics.consensus: {int(per_clip)} candidates per clip; the kernel takes at most per_clip = {MAX_PER_CLIP}")
    keys = idf = None
    idf_unseen, sigma = 0.0, 6.0
    if coef[0] > 0.0:
        if table is None:
            raise RuntimeError("metrics.consensus: utility weights cider, which needs table, a cvc.cider.CiderD (the idf table); there "
                               "is none")
        if table.keys is None or table.keys.device != cand.device:
            table.to(cand.device)
        keys, idf, idf_unseen, sigma = table.keys, table.idf, table.idf_unseen, table.sigma
    u, pick, best, pairs = hip.consensus_mix(cand.contiguous(), int(per_clip), coef, keys, idf, idf_unseen, sigma,
                                             live=None if live is None else live.to(torch.int32).contiguous(),
                                             logw=None if log_weights is None else log_weights.to(torch.float32).reshape(-1).contiguous(),
                                             want_pairs=want_pairs)
    out = dict(utility=u, pick=pick, best=best)
    if want_pairs:
        out["pairs"] = pairs
    return out


class DeviceScorer:
    """Corpus scores of a validation pass without a host read per batch: add() scores a batch on the device and adds to the int64 sum of
    the BLEU statistics, the fp64 sums of ROUGE-L and CIDEr-D, and the caption count; result() reads them once."""

    def __init__(self, cider_table):
        self.table = cider_table
        self.stats_sum = None          # [10] int64
        self.float_sums = None         # [3] fp64: sum ROUGE-L, sum CIDEr-D, captions

    def _ensure(self, device):
        if self.stats_sum is None:
            self.stats_sum = torch.zeros(10, dtype=torch.int64, device=device)
            self.float_sums = torch.zeros(3, dtype=torch.float64, device=device)

    def add(self, seq: torch.Tensor, refs: torch.Tensor, nref: torch.Tensor):
        """seq [rows, T] int64, refs [clips, Rmax, T], nref [clips], on the device; no host read"""
        self._ensure(seq.device)
        seq, refs, nref = seq.contiguous(), refs.contiguous(), nref.to(torch.int32).contiguous()
        ov = overlap(seq, refs, nref)
        cider = self.table.score(seq, refs, nref)
        self.stats_sum += ov["stats"].sum(0, dtype=torch.int64)
        self.float_sums += torch.stack([ov["rouge"].sum(dtype=torch.float64), cider.sum(dtype=torch.float64),
                                        torch.full((), float(seq.shape[0]), dtype=torch.float64, device=seq.device)])

    def add_sums(self, stats_sum, rouge_sum, cider_sum, count):
        """precomputed sums (another rank's, or a test's): stats_sum [10] integers, the rest numbers or one-element tensors"""
        stats_sum = torch.as_tensor(stats_sum)
        self._ensure(stats_sum.device)
        dev = self.stats_sum.device
        self.stats_sum += stats_sum.reshape(10).to(dev, torch.int64)
        self.float_sums += torch.stack([torch.as_tensor(x, dtype=torch.float64).reshape(()).to(dev) for x in (rouge_sum, cider_sum, count)])

    def sums(self):
        """-> (stats_sum: list of 10 ints, rouge_sum, cider_sum, count) on the host: ONE read"""
        if self.stats_sum is None:
            return [0] * 10, 0.0, 0.0, 0.0
        flat = torch.cat([self.stats_sum.to(torch.float64), self.float_sums]).tolist()       # (sums below 2^53 are exact in fp64)
        return [int(x) for x in flat[:10]], flat[10], flat[11], flat[12]

    def result(self) -> dict:
        stats_sum, rouge_sum, cider_sum, count = self.sums()
        return result_from_sums(stats_sum, rouge_sum, cider_sum, count)


def result_from_sums(stats_sum, rouge_sum, cider_sum, count) -> dict:
    bleu = corpus_bleu(stats_sum)
    n = max(float(count), 1.0)
    return {"Bleu_1": float(bleu[0]), "Bleu_2": float(bleu[1]), "Bleu_3": float(bleu[2]), "Bleu_4": float(bleu[3]),
            "ROUGE_L": float(rouge_sum) / n, "CIDEr": float(cider_sum) / n}


# --------------------------------------------------------------------------- grounding F1 of generated captions (csrc/grounding.hip)
# Definitions (what the kernel computes and tests/grounding_ref.py restates):
# * an object word is a position before the caption's first 0 whose word id maps to a detection class >= 1 (word_cls); the row's
#   predicted classes are the distinct such classes, each represented by its first object word.
# * pick[r, t, f]: for an object word and a sampled frame the proposal slot f * Np + j with the largest attention weight, the lowest j
#   among equal maxima (j = 0 for a frame without a weight > -inf); -1 elsewhere.  A trimmed proposal axis is padded with weight -inf
#   and zero boxes.
# * a class's box in frame f is the proposal its representative picks there; it hits an annotated box when the intersection has
#   positive width and height and 2 * inter > union (IoU > 1/2, no +1 pixel, fp32).
# * per class c, over the clip's annotated boxes of class c: gt, gt_pred (c is predicted), gt_hit (and the box's frame is a sampled
#   frame whose box hits it); over the rows that predict c: pred, pred_in_gt (the clip has a box of c), pred_hit (one of them is hit).
# * scores (grounding_result), over the classes S with gt > 0: Prec_all = mean pred_hit / pred (0 where pred = 0), Recall_all = mean
#   gt_hit / gt, Prec_loc = mean over pred_in_gt > 0 of pred_hit / pred_in_gt, Recall_loc = mean over gt_pred > 0 of gt_hit / gt_pred
#   (an empty mean: 0), F1 = 2 P R / (P + R) (0 when P + R = 0); the _micro scores: the same ratios on the column sums over all classes.
# These follow ActivityNet-Entities' F1_all / F1_loc but are NOT the toolkit's numbers: the toolkit is not pinned against, a word's
# class comes from the dataset's lemma table alone, and the boxes are the dataset's padded annotation rows.
GROUNDING_COLUMNS = ("gt", "gt_pred", "gt_hit", "pred", "pred_in_gt", "pred_hit")
GROUNDING_KEYS = ("F1_all", "F1_loc", "Prec_all", "Recall_all", "Prec_loc", "Recall_loc", "F1_all_micro", "F1_loc_micro")


def grounding(seq: torch.Tensor, att: torch.Tensor, ppls: torch.Tensor, gt_bboxs: torch.Tensor, nbox: torch.Tensor, word_cls: torch.Tensor,
              frames: int, per_clip: Optional[int] = None, table: Optional[torch.Tensor] = None,
              props_per_frame: Optional[int] = None) -> dict:
    """seq [rows, T] int64; att [rows, T, P] fp32; ppls [clips, P, 7]; gt_bboxs [clips, K, 6] (x1, y1, x2, y2, frame, class); nbox
    [clips]: how many of a clip's K boxes count; word_cls [V] int32: word id -> detection class or 0; frames: sampled frames per clip
    (P = frames * props_per_frame slots, frame-major; a trimmed axis, P smaller than that, needs props_per_frame); table [C + 1, 6]
    int32 is added to (None: a fresh one sized by word_cls' largest class -- one host read; pass a table to have none).
    -> dict(pick [rows, T, frames] int32, counts [rows, 6] int32, f1 [rows] fp32, table), all on the device."""
    from . import hip
    from .cider import MAX_T
    if seq.dim() != 2 or seq.shape[1] > MAX_T:
        raise RuntimeError(f"metrics.grounding: seq {tuple(seq.shape)}; the kernel takes rows of at most T = {MAX_T} words")
    if table is None:
        table = torch.zeros(max(int(word_cls.max()), 1) + 1, 6, dtype=torch.int32, device=seq.device)
    elif table.dim() != 2 or table.shape[0] < 2 or table.shape[1] != 6 or table.dtype != torch.int32:
        raise RuntimeError(f"metrics.grounding: the table must be [classes + 1, 6] int32, got {tuple(table.shape)} {table.dtype}")
    pick, counts, f1 = hip.grounding_f1(seq.contiguous(), att.contiguous(), ppls.contiguous(), gt_bboxs.contiguous(),
                                        nbox.to(torch.int32).contiguous(), word_cls.contiguous(), frames, table, per_clip, props_per_frame)
    return dict(pick=pick, counts=counts, f1=f1, table=table)


def grounding_result(table) -> dict:
    """the per-class counters [C + 1, 6] (GROUNDING_COLUMNS) -> the scores of GROUNDING_KEYS, fp64 on the host"""
    t = np.asarray(table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table, dtype=np.float64).reshape(-1, 6)
    gt, gt_pred, gt_hit, pred, pred_in_gt, pred_hit = (t[:, i] for i in range(6))

    def mean(num, den, keep):
        return float(np.mean(num[keep] / den[keep])) if keep.any() else 0.0

    def f1(p, r):
        return 2.0 * p * r / (p + r) if p + r > 0 else 0.0

    def ratio(num, den):
        return float(num / den) if den > 0 else 0.0
    S = gt > 0
    ratio_or_0 = np.divide(pred_hit, pred, out=np.zeros_like(pred), where=pred > 0)
    prec_all = float(np.mean(ratio_or_0[S])) if S.any() else 0.0
    rec_all = mean(gt_hit, gt, S)
    prec_loc = mean(pred_hit, pred_in_gt, S & (pred_in_gt > 0))
    rec_loc = mean(gt_hit, gt_pred, S & (gt_pred > 0))
    s = t.sum(0)
    return {"F1_all": f1(prec_all, rec_all), "F1_loc": f1(prec_loc, rec_loc), "Prec_all": prec_all, "Recall_all": rec_all,
            "Prec_loc": prec_loc, "Recall_loc": rec_loc, "F1_all_micro": f1(ratio(s[5], s[3]), ratio(s[2], s[0])),
            "F1_loc_micro": f1(ratio(s[5], s[4]), ratio(s[2], s[1]))}


class GroundingScorer:
    """Grounding scores of a validation pass without a host read per batch: add() runs the kernel on a batch, which adds to the
    per-class int32 table on the device; sums() reads it once; add_sums() takes another rank's table; result() -> grounding_result."""

    def __init__(self, word_cls: torch.Tensor, n_classes: int, frames: int, props_per_frame: Optional[int] = None):
        self.word_cls = word_cls.to(torch.int32).contiguous()
        self.n_classes, self.frames = int(n_classes), int(frames)
        self.props_per_frame = None if props_per_frame is None else int(props_per_frame)
        self.table = None              # [n_classes + 1, 6] int32 on the device
        self.extra = np.zeros((self.n_classes + 1, 6), dtype=np.int64)         # other ranks' tables, on the host

    def add(self, seq, att, ppls, gt_bboxs, nbox, per_clip: Optional[int] = None) -> dict:
        """one launch, no host read -> grounding()'s dict (pick, counts, f1 of this batch; table: the running one)"""
        if self.table is None:
            self.table = torch.zeros(self.n_classes + 1, 6, dtype=torch.int32, device=seq.device)
            self.word_cls = self.word_cls.to(seq.device)
        return grounding(seq, att, ppls, gt_bboxs, nbox, self.word_cls, self.frames, per_clip, self.table, self.props_per_frame)

    def add_sums(self, table):
        """a precomputed table (another rank's, or a test's): [n_classes + 1, 6] integers"""
        t = np.asarray(table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else table, dtype=np.int64)
        self.extra += t.reshape(self.n_classes + 1, 6)

    def sums(self) -> np.ndarray:
        """-> the table [n_classes + 1, 6] int64 on the host: ONE read"""
        mine = self.table.cpu().numpy().astype(np.int64) if self.table is not None else 0
        return self.extra + mine

    def result(self) -> dict:
        return grounding_result(self.sums())


# --------------------------------------------------------------------------- caption-set diversity (csrc/diversity.hip)
# Definitions (what the kernel computes and tests/diversity_ref.py restates), for the n candidate captions of one clip -- n samples,
# the n-best of a beam, the groups of a diverse beam, the draws of a stochastic beam -- of which the LIVE rows count:
# * a caption's words are the ids before its first 0, as for BLEU above (L = 0 is possible, UNK is a word like any other).
# * distinct_n, n = 1..4: the number of different n-grams of order n in the union of the live rows; total_n = sum over the live rows of
#   max(0, L - n + 1); unique: the live rows whose word sequence equals that of no earlier live row; scored: live if live >= 2 else 0.
# * Div_n of a clip = distinct_n / total_1 -- the set's WORD count is the denominator for every n, as in Shetty et al. 2017, Aneja et
#   al. 2019 and Wang & Chan 2019; Div_1, Div_2 of a corpus: the mean over the clips with total_1 > 0.  Higher is more diverse.
# * mBLEU: every live row as the candidate against the clip's other live rows as its references (ascending row order), the BLEU
#   statistics and sentence BLEU above; mBLEU_k of a corpus = corpus_bleu of the statistics summed over all scored rows.  LOWER is more
#   diverse.  A dead row and a row without another live row score nothing (all zeros).
# * Unique = sum unique / sum live;  Sets: the clips counted.
# * with the ground truth at hand: oracle_CIDEr = the mean over the clips with a live row of the best live row's CIDEr-D, mean_CIDEr =
#   the mean over the live rows -- accuracy and diversity trade against each other, so they are reported side by side.
# These are scores by word id over the dataset's tokens, NOT a toolkit's numbers: no tokenizer is applied, and mBLEU here is the
# corpus-level BLEU of the summed statistics, where some papers average sentence BLEU instead.
DIVERSITY_KEYS = ("Div_1", "Div_2", "mBLEU_1", "mBLEU_2", "mBLEU_3", "mBLEU_4", "Unique", "Sets")
SET_STATS_COLUMNS = ("distinct_1", "distinct_2", "distinct_3", "distinct_4", "total_1", "total_2", "total_3", "total_4", "live", "unique",
                     "scored", "reserved")


def set_diversity(cand: torch.Tensor, per_clip: int, live: Optional[torch.Tensor] = None) -> dict:
    """cand [rows, T] int64 on the device, per_clip consecutive candidates per clip; live [rows] (None: every row counts).
    -> dict(stats [clips, 12] int32 (SET_STATS_COLUMNS), mbleu_stats [rows, 10] int32, mbleu [rows, 4] fp32, div [clips, 2] fp32 =
    distinct_1 / total_1, distinct_2 / total_1, 0 where total_1 = 0), all on the device: one launch and a division, no host read."""
    from . import hip
    from .cider import MAX_T, MAX_PER_CLIP
    if cand.dim() != 2 or cand.shape[1] > MAX_T:
        raise RuntimeError(f"metrics.set_diversity: cand {tuple(cand.shape)}; the kernel takes rows of at most T = {MAX_T} words")
    if int(per_clip) > MAX_PER_CLIP:
        raise RuntimeError(f"metrics.set_diversity: {int(per_clip)} candidates per clip; the kernel takes at most per_clip = {MAX_PER_CLIP}")
    stats, mbleu_stats, mbleu = hip.caption_set_stats(cand.contiguous(), int(per_clip),
                                                      None if live is None else live.to(torch.int32).contiguous())
    total = stats[:, 4:5].to(torch.float32)                                 # (counts below 2^24: exact in fp32)
    div = torch.where(total > 0, stats[:, 0:2].to(torch.float32) / total, 0.0)          # (0 / 0 is not selected)
    return dict(stats=stats, mbleu_stats=mbleu_stats, mbleu=mbleu, div=div)


class DiversityScorer:
    """Set-diversity scores of a pass over the data without a host read per batch: add() runs the kernel on a batch's candidate sets and
    adds to the int64 sums (the mBLEU statistics; unique, live, clips) and the fp64 sums (Div_1, Div_2 and the clips they are over; with
    references the oracle and mean CIDEr-D sums and their counts) on the device; sums() reads them once; result() is fp64 on the host."""

    def __init__(self):
        self.int_sums = None           # [13] int64: the ten mBLEU statistics over the scored rows, sum unique, sum live, clips
        self.float_sums = None         # [7] fp64: sum Div_1, sum Div_2, clips with words, sum best CIDEr-D, clips with a live row,
        #                                sum CIDEr-D over the live rows, live rows scored against references

    def _ensure(self, device):
        if self.int_sums is None:
            self.int_sums = torch.zeros(13, dtype=torch.int64, device=device)
            self.float_sums = torch.zeros(7, dtype=torch.float64, device=device)

    def add(self, seq: torch.Tensor, per_clip: int, live: Optional[torch.Tensor] = None, refs: Optional[torch.Tensor] = None,
            nref: Optional[torch.Tensor] = None, cider=None) -> dict:
        """seq [rows, T] int64 on the device, per_clip consecutive candidates per clip, live [rows] or None; refs [clips, Rmax, T], nref
        [clips] and cider (a cvc.cider.CiderD), all three or none: the ground truth for oracle_CIDEr / mean_CIDEr.  No host read.
        -> set_diversity()'s dict of this batch (with "cider" [rows] fp32 when references are given)"""
        given = [x is not None for x in (refs, nref, cider)]
        if any(given) and not all(given):
            raise RuntimeError("DiversityScorer.add: refs, nref and cider go together (the oracle needs all three)")
        self._ensure(seq.device)
        per_clip = int(per_clip)
        out = set_diversity(seq, per_clip, live)
        st = out["stats"].to(torch.int64)
        clips = st.shape[0]
        self.int_sums += torch.cat([out["mbleu_stats"].sum(0, dtype=torch.int64), st[:, 9].sum().reshape(1), st[:, 8].sum().reshape(1),
                                    torch.full((1,), clips, dtype=torch.int64, device=seq.device)])
        worded = st[:, 4] > 0
        ratio = torch.where(worded.unsqueeze(1), st[:, 0:2].to(torch.float64) / st[:, 4:5].clamp(min=1).to(torch.float64),
                            torch.zeros((), dtype=torch.float64, device=seq.device))
        fl = [ratio[:, 0].sum(), ratio[:, 1].sum(), worded.sum().to(torch.float64)]
        zero = torch.zeros((), dtype=torch.float64, device=seq.device)
        if all(given):
            score = cider.score(seq.contiguous(), refs.contiguous(), nref)
            out["cider"] = score
            on = torch.ones(clips, per_clip, dtype=torch.bool, device=seq.device) if live is None else (live.reshape(clips, per_clip) != 0)
            s = score.to(torch.float64).view(clips, per_clip)
            any_live = on.any(1)
            best = torch.where(on, s, torch.full((), float("-inf"), dtype=torch.float64, device=seq.device)).max(1)[0]
            fl += [torch.where(any_live, best, zero).sum(), any_live.sum().to(torch.float64), torch.where(on, s, zero).sum(),
                   on.sum().to(torch.float64)]
        else:
            fl += [zero] * 4
        self.float_sums += torch.stack(fl)
        return out

    def add_sums(self, int_sums, float_sums):
        """precomputed sums (another rank's, or a test's), as sums() returns them"""
        int_sums = torch.as_tensor(int_sums)
        self._ensure(int_sums.device)
        dev = self.int_sums.device
        self.int_sums += int_sums.reshape(13).to(dev, torch.int64)
        self.float_sums += torch.as_tensor(float_sums, dtype=torch.float64).reshape(7).to(dev)

    def sums(self):
        """-> (int_sums: list of 13 ints, float_sums: list of 7 floats) on the host: ONE read"""
        if self.int_sums is None:
            return [0] * 13, [0.0] * 7
        flat = torch.cat([self.int_sums.to(torch.float64), self.float_sums]).tolist()        # (sums below 2^53 are exact in fp64)
        return [int(x) for x in flat[:13]], flat[13:]

    def result(self) -> dict:
        return diversity_from_sums(*self.sums())


def diversity_from_sums(int_sums, float_sums) -> dict:
    """DiversityScorer.sums() -> the scores of DIVERSITY_KEYS (and oracle_CIDEr, mean_CIDEr when rows were scored against references),
    fp64 on the host; empty sums give zeros"""
    i, f = [int(x) for x in int_sums], [float(x) for x in float_sums]
    bleu = corpus_bleu(np.asarray(i[:10], dtype=np.float64))
    out = {"Div_1": f[0] / f[2] if f[2] > 0 else 0.0, "Div_2": f[1] / f[2] if f[2] > 0 else 0.0,
           "mBLEU_1": float(bleu[0]), "mBLEU_2": float(bleu[1]), "mBLEU_3": float(bleu[2]), "mBLEU_4": float(bleu[3]),
           "Unique": i[10] / i[11] if i[11] > 0 else 0.0, "Sets": i[12]}
    if f[6] > 0:
        out["oracle_CIDEr"] = f[3] / f[4] if f[4] > 0 else 0.0
        out["mean_CIDEr"] = f[5] / f[6]
    return out


# --------------------------------------------------------------------------- spectral caption-set diversity (csrc/spectrum.hip)
# Definitions (what the kernel computes and tests/spectrum_ref.py restates; DESIGN section 7, "Spectral set diversity"):
# * sets, words and live rows as above; m = the clip's live rows, indexed 0 .. m - 1 in ascending row order.
# * mode cider -- plain CIDEr similarity, NOT CIDEr-D: v_n^a[g] = count_a(g) * idf(g), n = 1..4, idf from a CiderD's table (idf_unseen
#   for an absent key); s_n(a, b) = <v_n^a, v_n^b> / (|v_n^a| |v_n^b|), 0 when a norm is 0; K[a, b] = 1/4 sum_n s_n.  No clipping, no
#   length Gaussian, no factor 10: every s_n is a cosine kernel, K is positive semi-definite, K[a, a] = min(L, 4) / 4.
# * mode lsa: K[a, b] = sum_w count_a(w) count_b(w) over unigrams -- the Gram matrix of the bag-of-words matrix, lambda_i = sigma_i^2.
# * lam: the eigenvalues of the m x m matrix, descending, zeros behind them (fp64 Jacobi on the device).  With tr = sum_a K[a, a]:
#     score[:, 0] = -log(min(lam_1 / tr, 1)) / log(m);  score[:, 1] = -log(sqrt(lam_1) / sum_i sqrt(max(lam_i, 0))) / log(m);
#   both 0 where m < 2 or tr = 0.  0: every caption says the same; 1: no two captions share anything.  Higher is more diverse.
# * Self_CIDEr = the mean of score[:, 0] in mode cider, LSA = the mean of score[:, 1] in mode lsa, both over the clips with m >= 2 and
#   tr > 0;  Spectrum_sets: the clips with m >= 2.
# These two forms are this project's definitions, scores by word id over the dataset's tokens and NOT a toolkit's numbers: neither
# the paper's code nor its tokenizer is pinned against.  lam is returned so that any other form can be computed from it.
SPECTRUM_KEYS = ("Self_CIDEr", "LSA", "Spectrum_sets")


def set_spectrum(cand: torch.Tensor, per_clip: int, live: Optional[torch.Tensor] = None, cider=None, want_gram: bool = False) -> dict:
    """cand [rows, T] int64 on the device, per_clip consecutive candidates per clip; live [rows] (None: every row counts); cider: a
    cvc.cider.CiderD (mode cider over its idf table) or None (mode lsa).
    -> dict(lam [clips, 32] fp64, score [clips, 2] fp32, info [clips, 2] int32 (m, sweeps) (, gram [clips, 32, 32] fp32)), all on the
    device: one launch, no host read."""
    from . import hip
    from .cider import MAX_T, MAX_PER_CLIP
    if cand.dim() != 2 or cand.shape[1] > MAX_T:
        raise RuntimeError(f"metrics.set_spectrum: cand {tuple(cand.shape)}; the kernel takes rows of at most T = {MAX_T} words")
    if int(per_clip) > MAX_PER_CLIP:
        raise RuntimeError(f"metrics.set_spectrum: {int(per_clip)} candidates per clip; the kernel takes at most per_clip = {MAX_PER_CLIP}")
    live = None if live is None else live.to(torch.int32).contiguous()
    if cider is None:
        gram, lam, score, info = hip.caption_set_spectrum(cand.contiguous(), int(per_clip), "lsa", live=live, want_gram=want_gram)
    else:
        if cider.keys is None or cider.keys.device != cand.device:
            cider.to(cand.device)
        gram, lam, score, info = hip.caption_set_spectrum(cand.contiguous(), int(per_clip), "cider", cider.keys, cider.idf,
                                                          cider.idf_unseen, live=live, want_gram=want_gram)
    out = dict(lam=lam, score=score, info=info)
    if want_gram:
        out["gram"] = gram
    return out


class SpectrumScorer:
    """Self-CIDEr and LSA diversity of a pass over the data without a host read per batch: add() runs the kernel on a batch's candidate
    sets in mode cider (with a table), mode lsa, or both, and adds to five fp64 sums on the device; sums() reads them once; result()
    is fp64 on the host.  A scorer of its own: DiversityScorer's sums are not touched."""

    def __init__(self, cider=None, lsa: bool = True):
        if cider is None and not lsa:
            raise RuntimeError("SpectrumScorer: nothing to score -- give a CiderD table (Self_CIDEr), lsa=True (LSA), or both")
        self.table = cider
        self.lsa = bool(lsa)
        self.float_sums = None         # [5] fp64: sum score_0 (cider), its clips, sum score_1 (lsa), its clips, clips with m >= 2

    def _ensure(self, device):
        if self.float_sums is None:
            self.float_sums = torch.zeros(5, dtype=torch.float64, device=device)

    @staticmethod
    def _part(out, col):
        counted = (out["info"][:, 0] >= 2) & (out["lam"][:, 0] > 0)          # (K is positive semi-definite: tr > 0 iff lam_1 > 0)
        s = out["score"][:, col].to(torch.float64)
        return [torch.where(counted, s, torch.zeros((), dtype=torch.float64, device=s.device)).sum(), counted.sum().to(torch.float64)]

    def add(self, seq: torch.Tensor, per_clip: int, live: Optional[torch.Tensor] = None) -> dict:
        """seq [rows, T] int64 on the device, per_clip consecutive candidates per clip, live [rows] or None.  No host read.
        -> dict(cider=set_spectrum()'s dict in mode cider, lsa=... in mode lsa), the modes this scorer runs"""
        self._ensure(seq.device)
        zero = torch.zeros((), dtype=torch.float64, device=seq.device)
        outs, fl, info = {}, [], None
        if self.table is not None:
            outs["cider"] = set_spectrum(seq, per_clip, live, cider=self.table)
            fl += self._part(outs["cider"], 0)
            info = outs["cider"]["info"]
        else:
            fl += [zero, zero]
        if self.lsa:
            outs["lsa"] = set_spectrum(seq, per_clip, live)
            fl += self._part(outs["lsa"], 1)
            info = outs["lsa"]["info"]
        else:
            fl += [zero, zero]
        fl.append((info[:, 0] >= 2).sum().to(torch.float64))
        self.float_sums += torch.stack(fl)
        return outs

    def add_sums(self, float_sums):
        """precomputed sums (another rank's, or a test's), as sums() returns them"""
        float_sums = torch.as_tensor(float_sums, dtype=torch.float64)
        self._ensure(float_sums.device)
        self.float_sums += float_sums.reshape(5).to(self.float_sums.device)

    def sums(self):
        """-> list of 5 floats on the host: ONE read"""
        if self.float_sums is None:
            return [0.0] * 5
        return self.float_sums.tolist()

    def result(self) -> dict:
        return spectrum_from_sums(self.sums())


def spectrum_from_sums(float_sums) -> dict:
    """SpectrumScorer.sums() -> the scores of SPECTRUM_KEYS, fp64 on the host; empty sums (or a mode that never ran) give zeros"""
    f = [float(x) for x in float_sums]
    return {"Self_CIDEr": f[0] / f[1] if f[1] > 0 else 0.0, "LSA": f[2] / f[3] if f[3] > 0 else 0.0, "Spectrum_sets": int(f[4])}
