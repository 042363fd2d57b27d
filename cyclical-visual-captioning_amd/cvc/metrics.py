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


def parse_reward_weights(spec: str) -> dict:
    """"cider:1,bleu4:0.5,rougel:0.5" -> {name: weight} in the fixed order of REWARD_NAMES (names that are not given: absent).  An
    unknown name, a repeated name, a weight that is no number or negative, or an empty mix is a SystemExit that says so."""
    got = {}
    for item in (x.strip() for x in (spec or "").split(",")):
        if not item:
            continue
        name, sep, val = item.partition(":")
        name = name.strip().lower()
        if name not in REWARD_NAMES:
            raise SystemExit("--scst_reward: unknown metric %r (known: %s)" % (name, ", ".join(REWARD_NAMES)))
        if name in got:
            raise SystemExit("--scst_reward: %r is given twice" % name)
        try:
            w = float(val) if sep else 1.0
        except ValueError:
            raise SystemExit("--scst_reward: the weight of %r, %r, is not a number" % (name, val))
        if not (w >= 0.0) or math.isinf(w):
            raise SystemExit("--scst_reward: the weight of %r must be a finite number >= 0, got %r" % (name, val))
        got[name] = w
    if not got:
        raise SystemExit("--scst_reward: no metric given")
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
