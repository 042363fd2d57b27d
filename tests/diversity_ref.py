"""Caption-set diversity restated from its definitions in plain Python: n-grams as tuples of ids in sets and Counters, the mBLEU rows
through the overlap restatement (tests/overlap_ref.py), the corpus scores in fp64 -- nothing shared with cvc/metrics.py or
csrc/diversity.hip.  Not collected.

  words(caption): the ids BEFORE the first 0; L = 0 is possible.  "Live rows": the clip's rows with live != 0 (None: all).
  set_stats [clips, 12]: distinct_n = |union over the live rows of their n-grams of order n|, n = 1..4;  total_n = sum over the live
    rows of max(0, L - n + 1);  live;  unique = the live rows whose words equal those of no earlier live row;  scored = live if
    live >= 2 else 0;  0.
  mbleu_stats [rows, 10] / mbleu [rows, 4]: the row against the clip's other live rows in ascending order (overlap_ref.bleu_stats /
    bleu_from_stats); zeros for a dead row and for a row without another live row.
  result(): Div_n = mean over the clips with total_1 > 0 of distinct_n / total_1;  mBLEU_k = corpus BLEU of the summed mbleu_stats;
    Unique = sum unique / sum live;  Sets = clips.
"""
import math

import numpy as np

import overlap_ref as O


def _live(live, rows):
    return np.ones(rows, bool) if live is None else np.asarray(live).reshape(rows) != 0


def set_stats(cand, per_clip, live=None):
    cand = np.asarray(cand)
    rows = cand.shape[0]
    on = _live(live, rows)
    out = np.zeros((rows // per_clip, 12), np.int64)
    for c in range(rows // per_clip):
        ws = [O.words(cand[r]) for r in range(c * per_clip, (c + 1) * per_clip) if on[r]]
        for n in range(1, 5):
            grams = set()
            for w in ws:
                grams |= set(O.ngram_counts(w, n))
            out[c, n - 1] = len(grams)
            out[c, 3 + n] = sum(max(0, len(w) - n + 1) for w in ws)
        out[c, 8] = len(ws)
        out[c, 9] = sum(1 for i, w in enumerate(ws) if w not in ws[:i])
        out[c, 10] = len(ws) if len(ws) >= 2 else 0
    return out


def gathered(cand, per_clip, live=None):
    """the route through what existed: every row's references gathered -- refs [rows, max(per_clip - 1, 1), T] (the clip's other live
    rows in ascending order, zero-padded), nref [rows] (0 for a dead row)"""
    cand = np.asarray(cand)
    rows, T = cand.shape
    on = _live(live, rows)
    refs = np.zeros((rows, max(per_clip - 1, 1), T), np.int64)
    nref = np.zeros(rows, np.int64)
    for r in range(rows):
        if not on[r]:
            continue
        c = r // per_clip
        others = [j for j in range(c * per_clip, (c + 1) * per_clip) if j != r and on[j]]
        for k, j in enumerate(others):
            refs[r, k] = cand[j]
        nref[r] = len(others)
    return refs, nref


def mbleu(cand, per_clip, live=None, dt=np.float64):
    """-> (mbleu_stats [rows, 10] int64, mbleu [rows, 4] float64 array of `dt` values)"""
    cand = np.asarray(cand)
    rows = cand.shape[0]
    refs, nref = gathered(cand, per_clip, live)
    stats, bleu = np.zeros((rows, 10), np.int64), np.zeros((rows, 4))
    for r in range(rows):
        if nref[r] == 0:
            continue
        st = O.bleu_stats(cand[r], [refs[r, k] for k in range(nref[r])])
        stats[r] = st
        bleu[r] = [float(x) for x in O.bleu_from_stats(st, True, dt)]
    return stats, bleu


def div(stats):
    """[clips, 2] fp64: distinct_1 / total_1, distinct_2 / total_1 (0 where total_1 = 0)"""
    stats = np.asarray(stats, np.float64)
    out = np.zeros((stats.shape[0], 2))
    ok = stats[:, 4] > 0
    out[ok] = stats[ok, 0:2] / stats[ok, 4:5]
    return out


def result(stats, mbleu_stats):
    """the corpus scores in fp64 from set_stats [clips, 12] and mbleu_stats [rows, 10] (several batches: concatenated)"""
    stats, mb = np.asarray(stats, np.int64).reshape(-1, 12), np.asarray(mbleu_stats, np.int64).reshape(-1, 10)
    d = [row for row in div(stats)[stats[:, 4] > 0]] if len(stats) else []
    bleu = O.corpus(mb.sum(0)) if int(mb[:, 8].sum()) > 0 else np.zeros(4)
    live = int(stats[:, 8].sum())
    return {"Div_1": math.fsum(x[0] for x in d) / len(d) if d else 0.0, "Div_2": math.fsum(x[1] for x in d) / len(d) if d else 0.0,
            "mBLEU_1": float(bleu[0]), "mBLEU_2": float(bleu[1]), "mBLEU_3": float(bleu[2]), "mBLEU_4": float(bleu[3]),
            "Unique": int(stats[:, 9].sum()) / live if live else 0.0, "Sets": int(stats.shape[0])}


def oracle(cider, per_clip, live=None):
    """cider [rows]: the rows' CIDEr-D against the ground truth -> (oracle_CIDEr: the mean over the clips with a live row of the best live
    row's, mean_CIDEr: the mean over the live rows), fp64, dead rows left out"""
    cider = np.asarray(cider, np.float64)
    on = _live(live, len(cider))
    best = [max(cider[r] for r in range(c, c + per_clip) if on[r]) for c in range(0, len(cider), per_clip) if on[c:c + per_clip].any()]
    return (math.fsum(best) / len(best) if best else 0.0), (math.fsum(cider[on]) / int(on.sum()) if on.any() else 0.0)


# ---- cases
KINDS = ("near", "wide", "mixed")


def clip_rows(rng, per_clip, T, kind):
    """one clip's rows [per_clip, T]: near-duplicates over a tiny vocabulary (V = 5: many equal n-grams across rows), a wide vocabulary
    (ids up to 65 000), or a mix; among them rows with L = 0, rows without a 0 (L = T), identical rows, garbage after the first 0"""
    hi = 6 if kind == "near" else 65001
    out = np.zeros((per_clip, T), np.int64)
    base = rng.integers(1, hi, T)
    for j in range(per_clip):
        what = j % 6 if kind != "wide" else (j % 6) + 1
        if what == 0 or j == 0:
            row = base.copy()                                   # (row 0: the base, no 0 at all: L = T)
        elif what == 1:
            row = base.copy()
            row[rng.integers(0, T)] = rng.integers(1, hi)       # one word changed
        elif what == 2:
            row = rng.integers(1, min(hi, 6) if kind == "mixed" else hi, T)
        elif what == 3:
            row = out[rng.integers(0, j)].copy()                # an earlier row again
        elif what == 4:
            row = np.roll(base, 1)                              # the same n-grams at other positions
        else:
            row = np.zeros(T, np.int64)                         # L = 0
        L = int(rng.integers(0, T + 1))
        if what not in (0, 3) and j != 0 and L < T:             # the end mark, garbage behind it
            row[L] = 0
            row[L + 1:] = rng.integers(0, hi, T - L - 1)
        out[j] = row
    return out


def case(seed, clips, per_clip, T):
    """-> (cand [clips * per_clip, T] int64, live [rows] int32): clip c is of kind KINDS[c % 3]; live masks at random, clip 1 (if any)
    without a live row, clip 2 with one, clip 0 of several clips all live (a single clip keeps its random mask)"""
    rng = np.random.default_rng(seed)
    cand = np.concatenate([clip_rows(rng, per_clip, T, KINDS[c % 3]) for c in range(clips)])
    live = (rng.random(clips * per_clip) < 0.7).astype(np.int32).reshape(clips, per_clip)
    if clips > 1:
        live[0] = 1
        live[1] = 0
    if clips > 2:
        live[2] = 0
        live[2, rng.integers(0, per_clip)] = 1
    return cand, live.reshape(-1)
