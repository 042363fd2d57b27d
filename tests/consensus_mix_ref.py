"""Consensus selection under a weighted mix of utilities restated on tests/cider_ref.py and tests/overlap_ref.py (imported, nothing
shared with cvc/metrics.py or csrc/consensus_mix.hip), and the inputs of its tests.

  metric_k(i; j), k in (cider, bleu1..4, rougel): row i as the candidate against row j as its ONLY reference -- cider_ref.score and
      overlap_ref.bleu_from_stats / rouge_l with one reference
  u(i, j)    = sum_k coef_k metric_k(i; j) over the coefficients > 0, added in that order
  w_j        = exp(logw_j - max over the clip's live rows of logw): 1 at the maximum, 0 for -inf or NaN; without logw: 1
  utility[i] = (sum_j w_j u(i, j)) / (sum_j w_j) over the live j != i of the clip in ascending order, both sums rounded term by term;
               0 for a dead row, a row without another live row, and a zero denominator
  pick[c]    = the first live row of clip c with the largest utility, 0 for a clip without a live row (consensus_ref.picks)

`dt` is the float type of all arithmetic, as in cider_ref: np.float64 is the reference, np.float32 the yardstick.
"""
import numpy as np

import cider_ref as R
import overlap_ref as OV
from consensus_ref import picks, _zipf          # noqa: F401  (picks: the same rule)

NAMES = ("cider", "bleu1", "bleu2", "bleu3", "bleu4", "rougel")
CASES = [(1, 2, 1, 5), (3, 2, 4, 7), (4, 5, 20, 23), (2, 16, 63, 23), (3, 32, 20, 23)]       # (clips, n, T, V)
COEFS = [{"cider": 1.0}, {"bleu4": 1.0}, {"rougel": 1.0}, {"cider": 1.0, "bleu4": 0.5, "rougel": 0.5}]
MIXED = COEFS[3]
LOGW_KINDS = ("uniform", "finite", "inf")
BLEU4_NONZERO = 1e-3          # a BLEU-4 without a common 4-gram is (1e-15 / guess)^(1/4) x ... < 2e-4: "zero" for what a test can show
_CACHE = {}


def coefficients(utility):
    """{name: weight} -> the six coefficients as the kernel gets them (fp32 values)"""
    return [float(np.float32(utility.get(k, 0.0))) for k in NAMES]


def pair_metrics(cand, per_clip, live, df, n_doc, dt=np.float64, sigma=6.0):
    """-> float64 array [rows, per_clip, 6] of values computed in `dt`: [i, j] = the six metrics of row i against row c0 + j alone;
    zeros on the diagonal and where either row is dead"""
    cand = np.asarray(cand)
    rows = cand.shape[0]
    live = np.ones(rows, dtype=bool) if live is None else np.asarray(live).astype(bool)
    out = np.zeros((rows, per_clip, 6))
    for i in range(rows):
        c0 = i // per_clip * per_clip
        for j in range(per_clip):
            r = c0 + j
            if r == i or not (live[i] and live[r]):
                continue
            out[i, j, 0] = float(R.score(cand[i], [cand[r]], df, n_doc, sigma, dt)[0])
            out[i, j, 1:5] = [float(x) for x in OV.bleu_from_stats(OV.bleu_stats(cand[i], [cand[r]]), True, dt)]
            out[i, j, 5] = float(OV.rouge_l(cand[i], [cand[r]], dt)[0])
    return out


def weights(logw, live, per_clip, dt=np.float64):
    """logw [rows] float32 or None -> float64 array [rows] of the weights computed in `dt` (0 for a dead row)"""
    live = np.asarray(live).astype(bool)
    rows = live.shape[0]
    if logw is None:
        return live.astype(np.float64)
    lw = np.asarray(logw, dtype=np.float32).astype(np.float64)
    lw = np.where(np.isnan(lw), -np.inf, lw)
    out = np.zeros(rows)
    for c0 in range(0, rows, per_clip):
        on = [r for r in range(c0, c0 + per_clip) if live[r]]
        if not on:
            continue
        top = max(lw[r] for r in on)
        for r in on:
            if lw[r] == -np.inf:
                out[r] = 0.0
            elif lw[r] == top:
                out[r] = 1.0
            else:
                out[r] = float(np.exp(dt(dt(lw[r]) - dt(top))))
    return out


def utilities(pairs, w, live, per_clip, utility, dt=np.float64):
    """pairs [rows, per_clip, 6] and w [rows] as computed in `dt` -> float64 array [rows] of the utilities computed in `dt`"""
    live = np.asarray(live).astype(bool)
    rows = live.shape[0]
    coef = coefficients(utility)
    out = np.zeros(rows)
    for i in range(rows):
        if not live[i]:
            continue
        c0 = i // per_clip * per_clip
        num, den = dt(0), dt(0)
        for j in range(per_clip):
            r = c0 + j
            if r == i or not live[r]:
                continue
            u = dt(0)
            for k in range(6):
                if coef[k] > 0:
                    u = dt(u + dt(dt(coef[k]) * dt(pairs[i, j, k])))
            num = dt(num + dt(dt(w[r]) * u))
            den = dt(den + dt(w[r]))
        out[i] = float(dt(num / den)) if den > 0 else 0.0
    return out


# ---- inputs
def near_duplicates(rng, n, T, V, resample=2, cut=0.3):
    """[n, T]: one base caption of L words (L uniform in [ceil(T / 2), T]; L = T: no end mark) and n candidates that each redraw up
    to `resample` of its positions and, with probability `cut`, end early (a 0 somewhere in the second half); behind a 0 stand zeros
    or, by a coin, random words.  Near-duplicates by construction: cvc_caption_overlap's BLEU is unsmoothed, and unrelated captions
    share no 4-gram -- a test on them would compare zeros."""
    L = int(rng.integers((T + 1) // 2, T + 1))
    base = _zipf(rng, L, V)
    out = np.zeros((n, T), dtype=np.int64)
    for j in range(n):
        w = base.copy()
        for _ in range(int(rng.integers(0, resample + 1))):
            w[int(rng.integers(0, L))] = _zipf(rng, 1, V)[0]
        if L > 1 and rng.random() < cut:
            w = w[:int(rng.integers((L + 1) // 2, L))]
        row = _zipf(rng, T, V) if rng.integers(0, 2) else np.zeros(T, dtype=np.int64)
        row[:len(w)] = w
        if len(w) < T:
            row[len(w)] = 0
        out[j] = row
    return out


def make_inputs(clips, n, T, V, seed=None):
    """-> (cand [clips * n, T], live [rows] bool, train): `clips` sets of near-duplicates; for n >= 5 about 15 % of the rows are dead,
    clip 0's row 1 is empty (a leading 0, words behind it) and its row 2 has no 0 at all; with clips >= 3 the last clip has no live row
    and the one before it exactly one"""
    rng = np.random.default_rng(clips * 1000 + n * 100 + T if seed is None else seed)
    train = [near_duplicates(rng, 1, T, V, cut=0.5)[0] for _ in range(200)]
    cand = np.concatenate([near_duplicates(rng, n, T, V) for _ in range(clips)])
    live = rng.random(clips * n) >= 0.15 if n >= 5 else np.ones(clips * n, dtype=bool)
    if n >= 5:
        cand[1] = _zipf(rng, T, V)
        cand[1, 0] = 0
        tail = _zipf(rng, T, V)
        z = np.flatnonzero(cand[2] == 0)
        if z.size:
            cand[2, int(z[0]):] = tail[int(z[0]):]
        live[1] = live[2] = True
    if clips >= 3:
        live[(clips - 1) * n:] = False
        live[(clips - 2) * n:(clips - 1) * n] = False
        live[(clips - 2) * n + n // 2] = True
    return cand, live, train


def logw_of(kind, rng, rows):
    """the three kinds of log-weights the tests run: None, finite fp32 numbers a few nats apart, and the same with about a quarter at
    -inf and one NaN"""
    if kind == "uniform":
        return None
    lw = (rng.standard_normal(rows) * 3.0 - 8.0).astype(np.float32)
    if kind == "inf":
        lw[rng.random(rows) < 0.25] = -np.inf
        lw[int(rng.integers(0, rows))] = np.nan
    return lw


def case(clips, n, T, V):
    """-> dict(cand, live, train, df, n_doc, p64, p32 (pair metrics in fp64 / fp32), logw {kind: array or None}): built once per
    session, shared and left unchanged"""
    key = (clips, n, T, V)
    if key not in _CACHE:
        cand, live, train = make_inputs(clips, n, T, V)
        df, n_doc = R.doc_freq(train)
        rng = np.random.default_rng(7 + clips + n + T)
        _CACHE[key] = dict(cand=cand, live=live, train=train, df=df, n_doc=n_doc,
                           p64=pair_metrics(cand, n, live, df, n_doc), p32=pair_metrics(cand, n, live, df, n_doc, dt=np.float32),
                           logw={k: logw_of(k, rng, clips * n) for k in LOGW_KINDS})
    return _CACHE[key]


def expected(c, n, utility, kind):
    """a case -> (u64, u32) for one utility mix and one kind of log-weights"""
    lw = c["logw"][kind]
    return (utilities(c["p64"], weights(lw, c["live"], n), c["live"], n, utility),
            utilities(c["p32"], weights(lw, c["live"], n, np.float32), c["live"], n, utility, np.float32))
