"""Spectral caption-set diversity restated from its definitions in numpy: n-grams as tuples of ids in Counters, the similarity matrix
K in fp64 (and in float32 in the kernel's order of operations), the spectrum through numpy.linalg.eigvalsh, the two scores in fp64, and
a plain cyclic Jacobi with the kernel's skip rule -- nothing shared with cvc/metrics.py or csrc/spectrum.hip.  Not collected.

  words(caption): the ids BEFORE the first 0; L = 0 is possible.  "Live rows": the clip's rows with live != 0 (None: all); m of them,
    indexed 0 .. m - 1 in ascending row order.
  mode cider: v_n^a[g] = count_a(g) * idf(g), n = 1..4 (table: {key: idf}, `unseen` for an absent key); s_n = <v_n^a, v_n^b> /
    (|v_n^a| |v_n^b|), 0 when a norm is 0; K = 1/4 sum_n s_n.   mode lsa: K[a, b] = sum_w count_a(w) count_b(w).
  scores(lam, tr, m): -log(min(lam_1 / tr, 1)) / log m,  -log(sqrt(lam_1) / sum_i sqrt(max(lam_i, 0))) / log m; 0, 0 where m < 2 or tr = 0.
"""
import math
from collections import Counter

import numpy as np

import diversity_ref as D

SLOTS = 32
U = 2.0 ** -53


def words(row):
    row = [int(x) for x in np.asarray(row).reshape(-1)]
    return tuple(row[:row.index(0)]) if 0 in row else tuple(row)


def ngrams(w, n):
    return Counter(tuple(w[i:i + n]) for i in range(len(w) - n + 1))


def key_of(g):
    """the 64-bit key of an n-gram: id + 1 in 16 bits per word, the first word in the highest bits"""
    k = 0
    for i, w in enumerate(g):
        k |= ((w + 1) & 0xffff) << (48 - 16 * i)
    return k


def table_of(cider):
    """a cvc.cider.CiderD's host arrays -> ({key: float32 idf}, float32 idf_unseen)"""
    return {int(k): np.float32(v) for k, v in zip(cider.keys_host.tolist(), cider.idf_host.tolist())}, np.float32(cider.idf_unseen)


def live_rows(cand, per_clip, live, clip):
    cand = np.asarray(cand)
    on = np.ones(cand.shape[0], bool) if live is None else np.asarray(live).reshape(-1) != 0
    return [words(cand[r]) for r in range(clip * per_clip, (clip + 1) * per_clip) if on[r]]


def _vectors(w, n, table, unseen, dt):
    """{n-gram: count * idf} in `dt` (the idf are float32 values either way)"""
    return {g: dt(c) * dt(table.get(key_of(g), unseen)) for g, c in ngrams(w, n).items()}


def gram64(ws, mode, table=None, unseen=0.0):
    """one clip's K [m, m] in fp64 from its live rows' words"""
    m = len(ws)
    K = np.zeros((m, m))
    if mode == "lsa":
        cs = [ngrams(w, 1) for w in ws]
        for a in range(m):
            for b in range(m):
                K[a, b] = sum(c * cs[b][g] for g, c in cs[a].items())
        return K
    for n in range(1, 5):
        vs = [_vectors(w, n, table, unseen, np.float64) for w in ws]
        norms = [math.sqrt(math.fsum(x * x for x in v.values())) for v in vs]
        for a in range(m):
            for b in range(m):
                if norms[a] > 0 and norms[b] > 0:
                    K[a, b] += 0.25 * math.fsum(x * vs[b][g] for g, x in vs[a].items() if g in vs[b]) / (norms[a] * norms[b])
    return K


def _tree(x):
    """the wave sum: 64 float32 lanes added pairwise -- neighbours, quads, eights, sixteens, then the four rows (the DPP steps)"""
    x = np.asarray(x, np.float32)
    while x.size > 1:
        x = x[0::2] + x[1::2]
    return x[0]


def gram32(ws, mode, table=None, unseen=0.0):
    """K [m, m] in float32 the way the kernel forms it: a row's value of an n-gram sits at the lane of its first occurrence, squared
    norms and dot products are wave sums over the 64 lanes, s_n = dot / sqrt(|a|^2 |b|^2), K = 0.25 (((s_1 + s_2) + s_3) + s_4);
    the upper triangle is computed and mirrored"""
    f = np.float32
    m = len(ws)
    K = np.zeros((m, m), np.float32)
    lanes, sq = [], []
    for w in ws:
        per_n, sq_n = [], []
        for n in range(1, 5):
            if mode == "lsa" and n > 1:
                per_n.append({}), sq_n.append(f(0))
                continue
            first, vals = {}, np.zeros(64, np.float32)
            cnt = ngrams(w, n)
            for p in range(len(w) - n + 1):
                first.setdefault(tuple(w[p:p + n]), p)
            for g, p in first.items():
                vals[p] = f(cnt[g]) * (f(1) if mode == "lsa" else f(table.get(key_of(g), unseen)))
            per_n.append((first, vals))
            sq_n.append(_tree(vals * vals))
        lanes.append(per_n), sq.append(sq_n)
    for a in range(m):
        for b in range(a, m):
            s = []
            for n in range(4):
                if mode == "lsa" and n > 0:
                    break
                (fa, va), (fb, vb) = lanes[a][n], lanes[b][n]
                acc = np.zeros(64, np.float32)
                for g, p in fa.items():
                    if g in fb:
                        acc[p] = va[p] * vb[fb[g]]
                dot = _tree(acc)
                if mode == "lsa":
                    s.append(dot)
                else:
                    qa, qb = sq[a][n], sq[b][n]
                    s.append(dot / np.sqrt(qa * qb, dtype=np.float32) if qa > 0 and qb > 0 else f(0))
            K[a, b] = K[b, a] = s[0] if mode == "lsa" else f(0.25) * (((s[0] + s[1]) + s[2]) + s[3])
    return K


def padded(K, dt=np.float64):
    out = np.zeros((SLOTS, SLOTS), dt)
    out[:K.shape[0], :K.shape[1]] = K
    return out


def spectrum(K):
    """eigenvalues of the symmetric K in descending order (numpy.linalg.eigvalsh), padded with zeros to 32"""
    out = np.zeros(SLOTS)
    if K.shape[0]:
        out[:K.shape[0]] = np.linalg.eigvalsh(np.asarray(K, np.float64))[::-1]
    return out


def scores(lam, tr, m):
    """the two scores in fp64 from the (descending) eigenvalues, the trace and m"""
    if m < 2 or not tr > 0:
        return 0.0, 0.0
    lam = np.asarray(lam, np.float64)[:m]
    roots = math.fsum(math.sqrt(max(float(x), 0.0)) for x in lam)
    s0 = -math.log(min(float(lam[0]) / tr, 1.0)) / math.log(m)
    s1 = -math.log(math.sqrt(float(lam[0])) / roots) / math.log(m) if lam[0] > 0 else 0.0
    return s0 + 0.0, s1 + 0.0


def jacobi(K, max_sweeps=16):
    """plain cyclic Jacobi in fp64 with the kernel's rules: a rotation is skipped when |K_pq| <= 4 * 2^-53 * trace, a sweep without a
    rotation ends the solve, at most 16 sweeps -> (eigenvalues descending, sweeps run or -1 if the last one still rotated)"""
    A = np.array(K, np.float64)
    m = A.shape[0]
    thr = 4.0 * U * float(np.trace(A)) if m else 0.0
    sweeps = 0
    while sweeps < max_sweeps:
        rotated = False
        for p in range(m - 1):
            for q in range(p + 1, m):
                apq = A[p, q]
                if abs(apq) <= thr:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                t = -t if theta < 0 else t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                J = np.eye(m)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                A = J.T @ A @ J
                A[p, q] = A[q, p] = 0.0
                A = (A + A.T) / 2
                rotated = True
        sweeps += 1
        if not rotated:
            return np.sort(np.diag(A))[::-1], sweeps
    return np.sort(np.diag(A))[::-1], -1


def headline(score_col, m, counted):
    """the mean of a score column over the counted clips (fp64; none: 0)"""
    xs = [float(s) for s, k, c in zip(score_col, m, counted) if k >= 2 and c]
    return math.fsum(xs) / len(xs) if xs else 0.0


# ---- cases
def case(seed, clips, per_clip, T):
    """diversity_ref.case (near-duplicates over five words, ids up to 65 000, L = 0, rows without a 0, garbage behind the end mark,
    random live masks, clip 1 without a live row, clip 2 with one) and, among several clips: clip 3's rows all the same caption (a
    rank-1 K) and clip 4's rows repeating pairwise (rank m / 2), both all live -> (cand [rows, T] int64, live [rows] int32)"""
    cand, live = D.case(seed, clips, per_clip, T)
    cand, live = cand.copy(), live.copy().reshape(clips, per_clip)
    rng = np.random.default_rng(seed + 7)
    if clips > 3:
        row = rng.integers(1, 6, T)
        cand[3 * per_clip:4 * per_clip] = row
        live[3] = 1
    if clips > 4:
        for j in range(per_clip):
            if j % 2 == 0:
                cand[4 * per_clip + j] = rng.integers(1, 65001, T)
            else:
                cand[4 * per_clip + j] = cand[4 * per_clip + j - 1]
        live[4] = 1
    return cand, live.reshape(-1)
