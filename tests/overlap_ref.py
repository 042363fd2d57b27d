"""BLEU statistics, sentence / corpus BLEU and ROUGE-L restated from their definitions, n-grams as Python tuples in Counters and the
longest common subsequence as the quadratic DP -- nothing shared with cvc/metrics.py or csrc/overlap.hip.  `dt` is the float type of ALL
arithmetic of the scores: np.float64 is the reference, np.float32 the yardstick the kernel's error is measured against.

  words(caption): the ids BEFORE the first 0 (the end mark is no word); all of them without a 0.  L = 0 is possible.
  guess_n = max(0, Lc - n + 1);  correct_n = sum over distinct candidate n-grams g of min(count_c(g), max_r count_r(g))
  ref_len = the reference length closest to Lc, the shorter on a tie, 0 without a reference
  p_n = (correct_n + 1e-15) / (guess_n + 1e-9);  BLEU_k = bp exp((sum_{n<=k} log p_n) / k), logs added in ascending n,
  bp = 1 if Lc >= ref_len else exp(1 - ref_len / Lc);  BLEU_k = 0 when Lc = 0 or there is no reference
  ROUGE_L = (1 + b^2) p q / (q + b^2 p), b = 1.2, p = max_r lcs_r / Lc, q = max_r lcs_r / Lr (Lr = 0: 0); 0 when Lc = 0, no
  reference, or p q = 0
"""
from collections import Counter

import numpy as np

TINY, SMALL, BETA = 1e-15, 1e-9, 1.2


def words(caption):
    out = []
    for w in caption:
        if int(w) == 0:
            break
        out.append(int(w))
    return out


def ngram_counts(w, n):
    return Counter(tuple(w[i:i + n]) for i in range(len(w) - n + 1))


def lcs(a, b):
    """length of the longest common subsequence, the quadratic DP"""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def bleu_stats(cand, refs):
    """one candidate against its list of references -> [correct_1..4, guess_1..4, cand_len, ref_len] (ints)"""
    wc = words(cand)
    wrs = [words(r) for r in refs]
    correct, guess = [], []
    for n in range(1, 5):
        cc = ngram_counts(wc, n)
        rcs = [ngram_counts(wr, n) for wr in wrs]
        correct.append(sum(min(c, max((rc.get(g, 0) for rc in rcs), default=0)) for g, c in cc.items()))
        guess.append(max(0, len(wc) - n + 1))
    ref_len = 0
    if wrs:
        ref_len = min((abs(len(wr) - len(wc)), len(wr)) for wr in wrs)[1]
    return correct + guess + [len(wc), ref_len]


def clipping_bites(cand, refs):
    """some candidate n-gram (n = 1..4) occurs more often than in any reference, and in some reference at least once"""
    wc = words(cand)
    wrs = [words(r) for r in refs]
    for n in range(1, 5):
        rcs = [ngram_counts(wr, n) for wr in wrs]
        for g, c in ngram_counts(wc, n).items():
            m = max((rc.get(g, 0) for rc in rcs), default=0)
            if c > m > 0:
                return True
    return False


def bleu_from_stats(stats, has_ref=True, dt=np.float64):
    """the ten statistics -> [BLEU_1..4] in `dt`"""
    correct, guess, cand_len, ref_len = stats[0:4], stats[4:8], int(stats[8]), int(stats[9])
    if cand_len == 0 or not has_ref:
        return [dt(0)] * 4
    bp = dt(1) if cand_len >= ref_len else dt(np.exp(dt(dt(1) - dt(dt(ref_len) / dt(cand_len)))))
    out, logs = [], dt(0)
    for n in range(4):
        p = dt(dt(dt(correct[n]) + dt(TINY)) / dt(dt(guess[n]) + dt(SMALL)))
        logs = dt(logs + dt(np.log(p)))
        out.append(dt(bp * dt(np.exp(dt(logs / dt(n + 1))))))
    return out


def rouge_l(cand, refs, dt=np.float64):
    """-> (ROUGE-L in `dt`, [lcs_r])"""
    wc = words(cand)
    ls = [lcs(wc, words(r)) for r in refs]
    if len(wc) == 0 or not refs or max(ls) == 0:
        return dt(0), ls
    p = dt(dt(max(ls)) / dt(len(wc)))
    q = dt(0)
    for l, r in zip(ls, refs):
        lr = len(words(r))
        if lr > 0:
            q = max(q, dt(dt(l) / dt(lr)))
    b2 = dt(dt(BETA) * dt(BETA))
    return dt(dt(dt(dt(dt(1) + b2) * p) * q) / dt(q + dt(b2 * p))), ls


def score_batch(cand, refs, nref, dt=np.float64):
    """cand [rows, T], refs [clips, Rmax, T], nref [clips] (clamped to [0, Rmax]) -> dict(stats [rows, 10] int64, lcs [rows, Rmax] int64
    with -1 in slots >= nref, bleu [rows, 4] and rouge [rows] as float64 arrays, clip [rows] bool: clipping bites)"""
    cand, refs, nref = np.asarray(cand), np.asarray(refs), np.asarray(nref)
    rows, Rmax = cand.shape[0], refs.shape[1]
    per = rows // refs.shape[0]
    out = dict(stats=np.zeros((rows, 10), np.int64), lcs=np.full((rows, Rmax), -1, np.int64), bleu=np.zeros((rows, 4)),
               rouge=np.zeros(rows), clip=np.zeros(rows, bool))
    for r in range(rows):
        c = r // per
        rs = [refs[c, j] for j in range(max(0, min(int(nref[c]), Rmax)))]
        st = bleu_stats(cand[r], rs)
        out["stats"][r] = st
        out["bleu"][r] = [float(x) for x in bleu_from_stats(st, bool(rs), dt)]
        rl, ls = rouge_l(cand[r], rs, dt)
        out["rouge"][r] = float(rl)
        out["lcs"][r, :len(ls)] = ls
        out["clip"][r] = clipping_bites(cand[r], rs)
    return out


def corpus(stats_sum):
    """corpus BLEU_1..4 in fp64 from the ten summed statistics"""
    return np.array([float(x) for x in bleu_from_stats(list(stats_sum), True, np.float64)])
