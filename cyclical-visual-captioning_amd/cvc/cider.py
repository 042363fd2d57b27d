"""CIDEr-D (Vedantam et al. 2015, "CIDEr: Consensus-based Image Description Evaluation"; the -D variant with count clipping and the
Gaussian length term, document frequencies taken from a fixed corpus) scored on the device: the reward of self-critical training
(cvc.trainer.Trainer.scst_step) and a caption score for validation loops that needs none of the external toolkits.

Definition (what csrc/cider.hip computes in fp32 and tests/cider_ref.py restates in fp64):

* a caption's words are its ids up to and including the first 0 (the end mark counts as a word, so a caption that never ends is
  penalised through the length term and its missing end n-grams); without a 0 all T words count.  L = that length.
* for n = 1..4 and an n-gram g that occurs c times in the caption: v_n[g] = c * idf[g], idf[g] = ln N_doc - ln max(1, df[g]) with
  df[g] the number of corpus captions that contain g and N_doc the number of corpus captions (an n-gram the corpus never saw:
  idf = ln N_doc).
* s_n(c, r) = sum_g min(v_n^c[g], v_n^r[g]) v_n^r[g] / (|v_n^c| |v_n^r|) (0 if a norm is 0), times exp(-(L_c - L_r)^2 / (2 sigma^2)),
  sigma = 6;  score = 10 * mean over the references of the mean over n.  No reference: 0.

The table (built once, on the host): an n-gram is an exact 64-bit key, 16 bits per word holding id + 1, the first word in the
highest bits, unused positions 0 -- the order n is part of the key, nothing is hashed.  Keys are stored sorted as unsigned values
(in an int64 tensor: torch has no unsigned 64-bit arithmetic, the kernel reads the bits), idf is computed in fp64 and stored fp32.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import numpy as np
import torch

MAX_ID = 65534          # ids are stored as id + 1 in 16 bits
MAX_T = 63              # one wave per caption, lane p owns the n-grams starting at p
MAX_PER_CLIP = 32       # consensus selection: a clip's candidates share one workgroup's LDS
SIGMA = 6.0


def caption_words(ids) -> np.ndarray:
    """the ids up to and including the first 0 (all of them without one), as int64"""
    a = np.asarray(ids, dtype=np.int64).reshape(-1)
    z = np.flatnonzero(a == 0)
    return a[:int(z[0]) + 1] if z.size else a


def ngram_keys(words: np.ndarray, n: int) -> np.ndarray:
    """the keys (uint64) of the n-grams of `words` in order of their start position"""
    m = len(words) - n + 1
    if m <= 0:
        return np.zeros(0, dtype=np.uint64)
    w = words.astype(np.uint64) + np.uint64(1)
    k = np.zeros(m, dtype=np.uint64)
    for i in range(n):
        k |= w[i:i + m] << np.uint64(48 - 16 * i)
    return k


class CiderD:
    """The document-frequency table of a caption corpus on the device, and the scorer over it."""

    def __init__(self, keys: np.ndarray, idf: np.ndarray, n_doc: int, device=None, sigma: float = SIGMA):
        self.n_doc = int(n_doc)
        self.idf_unseen = float(math.log(self.n_doc)) if self.n_doc > 0 else 0.0
        self.sigma = float(sigma)
        self.keys_host = np.ascontiguousarray(keys, dtype=np.uint64)
        self.idf_host = np.ascontiguousarray(idf, dtype=np.float32)
        self.device = torch.device(device) if device is not None else None
        self.keys = self.idf = None
        if self.device is not None:
            self.to(self.device)

    def to(self, device):
        self.device = torch.device(device)
        self.keys = torch.from_numpy(self.keys_host.view(np.int64).copy()).to(self.device)
        self.idf = torch.from_numpy(self.idf_host.copy()).to(self.device)
        return self

    def __len__(self):
        return int(self.keys_host.size)

    @classmethod
    def from_captions(cls, captions: Iterable, device=None, sigma: float = SIGMA) -> "CiderD":
        """captions: 1-D arrays (or tensors) of word ids, one per corpus caption, 0-terminated or full length"""
        per_doc = []
        n_doc = 0
        for cap in captions:
            a = cap.detach().cpu().numpy() if isinstance(cap, torch.Tensor) else np.asarray(cap)
            a = a.astype(np.int64).reshape(-1)
            if a.size < 1:
                continue
            if a.size > MAX_T:
                raise RuntimeError(f"CiderD: a caption of {a.size} steps; the scorer takes at most T = {MAX_T} (one lane per position)")
            if a.min() < 0 or a.max() > MAX_ID:
                raise RuntimeError(f"CiderD: word id {int(a.max() if a.max() > MAX_ID else a.min())} outside [0, {MAX_ID}]: n-gram keys "
                                   f"hold id + 1 in 16 bits, the vocabulary must stay below {MAX_ID + 1} ids")
            w = caption_words(a)
            n_doc += 1
            per_doc.append(np.unique(np.concatenate([ngram_keys(w, n) for n in range(1, 5)])))
        if n_doc == 0:
            return cls(np.zeros(0, np.uint64), np.zeros(0, np.float32), 0, device, sigma)
        keys, df = np.unique(np.concatenate(per_doc), return_counts=True)        # ascending as unsigned values
        idf = math.log(n_doc) - np.log(np.maximum(1.0, df.astype(np.float64)))
        return cls(keys, idf.astype(np.float32), n_doc, device, sigma)

    @classmethod
    def from_dataset(cls, dataset, device=None, sigma: float = SIGMA) -> "CiderD":
        """the captions of a training split: `dataset.caption_ids()` when the dataset has one; the ActivityNet-Entities loader's
        caption file (tokens through its vocabulary, cut at seq_length -- the rows its items carry as gt_seq); otherwise the items
        themselves (position 2: gt_seq [*, T], position 3: num, whose first entry counts the captions)"""
        hook = getattr(dataset, "caption_ids", None)
        if callable(hook):
            return cls.from_captions(hook(), device, sigma)
        if hasattr(dataset, "caption_file") and hasattr(dataset, "split_ix") and hasattr(dataset, "info"):
            def rows():
                T = int(dataset.seq_length)
                for ix in dataset.split_ix:
                    vid, seg_no = dataset.info['videos'][ix]['id'].split('_segment_')
                    words = dataset.caption_file[vid]['segments'][str(int(seg_no))]['caption'][:T]
                    row = np.zeros(T, dtype=np.int64)
                    row[:len(words)] = [int(dataset.wtoi[w]) for w in words]
                    yield row
            return cls.from_captions(rows(), device, sigma)

        def items():
            for i in range(len(dataset)):
                it = dataset[i]
                gt, ncap = torch.as_tensor(it[2]), int(torch.as_tensor(it[3]).reshape(-1)[0])
                for r in range(max(0, min(ncap, gt.shape[0]))):
                    yield gt[r]
        return cls.from_captions(items(), device, sigma)

    def score(self, cand: torch.Tensor, refs: torch.Tensor, nref: torch.Tensor, per_order: bool = False):
        """cand [rows, T] int64 on the device; refs [clips, Rmax, T] int64 (rows / clips consecutive candidates per clip); nref [clips]:
        how many of a clip's Rmax reference rows count.  -> CIDEr-D [rows] fp32 (, its four per-order parts [rows, 4])."""
        from . import hip
        if self.keys is None or self.keys.device != cand.device:
            self.to(cand.device)
        if cand.shape[1] > MAX_T:
            raise RuntimeError(f"CiderD.score: T = {cand.shape[1]}; the scorer takes at most T = {MAX_T}")
        return hip.cider_d(cand.contiguous(), refs.contiguous(), nref.to(torch.int32).contiguous(), self.keys, self.idf, self.idf_unseen,
                           self.sigma, want_orders=per_order)

    def consensus(self, cand: torch.Tensor, per_clip: int, live: Optional[torch.Tensor] = None):
        """Consensus (minimum-Bayes-risk) selection under CIDEr-D.  cand [rows, T] int64 on the device, per_clip consecutive candidates
        per clip; live [rows] (nullable: every row counts): rows that are neither candidates nor references.
        -> utility [rows] fp32: the CIDEr-D of a row against the clip's other live rows as its references, with uniform weights;
        pick [clips] int32: the first live row with the largest utility; best [clips, T] int64: that row."""
        from . import hip
        if self.keys is None or self.keys.device != cand.device:
            self.to(cand.device)
        if cand.shape[1] > MAX_T:
            raise RuntimeError(f"CiderD.consensus: T = {cand.shape[1]}; the scorer takes at most T = {MAX_T}")
        if int(per_clip) > MAX_PER_CLIP:
            raise RuntimeError(f"CiderD.consensus: {int(per_clip)} candidates per clip; the selection takes at most per_clip = {MAX_PER_CLIP}")
        return hip.consensus_cider(cand.contiguous(), int(per_clip), self.keys, self.idf, self.idf_unseen, self.sigma,
                                   live=None if live is None else live.to(torch.int32).contiguous())

    def self_cider(self, cand: torch.Tensor, per_clip: int, live: Optional[torch.Tensor] = None) -> dict:
        """Self-CIDEr diversity of every clip's candidate set over this table (cvc.metrics.set_spectrum in mode cider: plain CIDEr
        similarity -- no clipping, no length term, the end mark is no word).  -> dict(lam [clips, 32] fp64, score [clips, 2] fp32,
        info [clips, 2] int32); score[:, 0] is the clip's Self-CIDEr."""
        from . import metrics
        return metrics.set_spectrum(cand, per_clip, live, cider=self)
