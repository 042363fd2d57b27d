"""Consensus (minimum-Bayes-risk) caption selection restated on tests/cider_ref.py (imported, nothing shared with cvc/cider.py or
csrc/consensus.hip), and the inputs of its tests.

  utility[i] = cider_ref.score(row i, the clip's other live rows in ascending order), 0 for a dead row or without another live row
  pick[c]    = the first live row of clip c with the largest utility, 0 for a clip without a live row

`dt` is the float type of all arithmetic, as in cider_ref: np.float64 is the reference, np.float32 the yardstick.
"""
import numpy as np

import cider_ref as R

CASES = [(1, 2, 1, 5), (3, 2, 4, 7), (4, 5, 20, 23), (2, 16, 63, 23), (3, 32, 20, 23), (64, 20, 20, 997)]       # (clips, n, T, V)
_CACHE = {}


def utilities(cand, per_clip, live, df, n_doc, dt=np.float64, sigma=6.0):
    """cand [rows, T], live [rows] (None: all) -> float64 array [rows] of values computed in `dt`"""
    cand = np.asarray(cand)
    rows = cand.shape[0]
    live = np.ones(rows, dtype=bool) if live is None else np.asarray(live).astype(bool)
    out = np.zeros(rows)
    for i in range(rows):
        if not live[i]:
            continue
        c0 = i // per_clip * per_clip
        refs = [cand[r] for r in range(c0, c0 + per_clip) if r != i and live[r]]
        out[i] = float(R.score(cand[i], refs, df, n_doc, sigma, dt)[0])
    return out


def picks(utilities, live, per_clip):
    """-> int array [clips]: the first live arg-max of every clip, 0 without a live row"""
    u = np.asarray(utilities).reshape(-1, per_clip)
    live = np.ones(u.shape, dtype=bool) if live is None else np.asarray(live).astype(bool).reshape(-1, per_clip)
    out = np.zeros(u.shape[0], dtype=np.int64)
    for c in range(u.shape[0]):
        best = -1
        for j in range(per_clip):
            if live[c, j] and (best < 0 or u[c, j] > u[c, best]):
                best = j
        out[c] = max(best, 0)
    return out


def _zipf(rng, size, V):
    """`size` words drawn from a Zipf-like law over 1 .. V - 1 (tests/test_gpu_cider.py: _caption)"""
    p = 1.0 / np.arange(1, V, dtype=np.float64)
    return rng.choice(np.arange(1, V), size=size, p=p / p.sum()).astype(np.int64)


def _row(rng, words, T, V, garbage):
    """the words, the end mark if there is room, and behind it zeros or (garbage; None: a coin decides) random words"""
    if garbage is None:
        garbage = bool(rng.integers(0, 2))
    row = _zipf(rng, T, V) if garbage else np.zeros(T, dtype=np.int64)
    L = len(words)
    row[:L] = words
    if L < T:
        row[L] = 0
    return row


def clip_candidates(rng, n, T, V, garbage=None):
    """[n, T]: one base caption of L words (L uniform in [1, T); 0 for T = 1) and its variants by j % 6 -- 0: the base; 1, 2: one or
    two of its words redrawn; 3: cut to ceil(L / 2) words; 4: one word appended, if it fits; 5: an unrelated caption of 0 .. T words"""
    L = int(rng.integers(1, T)) if T > 1 else 0
    base = _zipf(rng, L, V)
    out = np.zeros((n, T), dtype=np.int64)
    for j in range(n):
        kind = j % 6
        w = base.copy()
        if kind in (1, 2) and L > 0:
            for _ in range(kind):
                w[int(rng.integers(0, L))] = _zipf(rng, 1, V)[0]
        elif kind == 3:
            w = w[:(L + 1) // 2]
        elif kind == 4 and L + 1 <= T:
            w = np.concatenate([w, _zipf(rng, 1, V)])
        elif kind == 5:
            w = _zipf(rng, int(rng.integers(0, T + 1)), V)
        out[j] = _row(rng, w, T, V, garbage)
    return out


def case(clips, n, T, V):
    """-> dict(cand [clips * n, T], live [rows] bool or None, train, df, n_doc, u64, u32): built once per session, shared and left
    unchanged (the largest case is ~13 s of pure Python)"""
    key = (clips, n, T, V)
    if key not in _CACHE:
        rng = np.random.default_rng(clips * 1000 + n * 100 + T)
        train = [clip_candidates(rng, 1, T, V, garbage=False)[0] for _ in range(200 if V < 100 else 2000)]
        cand = np.concatenate([clip_candidates(rng, n, T, V) for _ in range(clips)])
        live = rng.random(clips * n) >= 0.15 if n >= 5 else None            # about 15 % of the rows are dead
        df, n_doc = R.doc_freq(train)
        _CACHE[key] = dict(cand=cand, live=live, train=train, df=df, n_doc=n_doc, u64=utilities(cand, n, live, df, n_doc),
                           u32=utilities(cand, n, live, df, n_doc, dt=np.float32))
    return _CACHE[key]
