"""CIDEr-D restated from its definition (Vedantam et al. 2015; the -D variant: counts clipped against the reference, Gaussian length
term, document frequencies from a fixed corpus), n-grams as Python tuples in dictionaries -- nothing shared with cvc/cider.py or
csrc/cider.hip.  `dt` is the float type of ALL arithmetic: np.float64 is the reference, np.float32 the yardstick the kernel's error is
measured against (idf is formed in fp64 and then rounded to `dt`, as the table stores it).

  words(caption): the ids up to and including the first 0; all of them without a 0.
  v_n[g] = count(g) * idf[g],  idf[g] = ln N_doc - ln max(1, df[g])  (df = 0 for an n-gram the corpus never saw)
  s_n(c, r) = sum_g min(v_n^c[g], v_n^r[g]) * v_n^r[g] / (|v_n^c| |v_n^r|), 0 if a norm is 0, times exp(-(L_c - L_r)^2 / (2 sigma^2))
  score = 10 * mean_r mean_n s_n;  no reference: 0
"""
import math
from collections import Counter

import numpy as np


def words(caption):
    out = []
    for w in caption:
        out.append(int(w))
        if int(w) == 0:
            break
    return out


def ngrams(w, n):
    return [tuple(w[i:i + n]) for i in range(len(w) - n + 1)]


def doc_freq(captions):
    """-> ({n-gram tuple: number of captions that contain it}, number of captions)"""
    df = Counter()
    n_doc = 0
    for cap in captions:
        w = words(cap)
        n_doc += 1
        seen = set()
        for n in range(1, 5):
            seen.update(ngrams(w, n))
        df.update(seen)
    return dict(df), n_doc


def idf64(df, n_doc, g):
    return math.log(n_doc) - math.log(max(1, df.get(g, 0)))


def key(g):
    """the 64-bit key of the table: 16 bits per word holding id + 1, first word highest, unused positions 0"""
    k = 0
    for i, w in enumerate(g):
        k |= (int(w) + 1) << (48 - 16 * i)
    return k


def _vec(w, n, df, n_doc, dt):
    return {g: dt(c) * dt(idf64(df, n_doc, g)) for g, c in Counter(ngrams(w, n)).items()}


def _norm(v, dt):
    s = dt(0)
    for x in v.values():
        s = dt(s + dt(x * x))
    return dt(np.sqrt(s))


def score(cand, refs, df, n_doc, sigma=6.0, dt=np.float64):
    """one candidate against its list of references -> (score, [four per-order parts, each 10 * mean_r s_n])"""
    if len(refs) == 0:
        return dt(0), [dt(0)] * 4
    wc = words(cand)
    acc = [dt(0)] * 4
    for ref in refs:
        wr = words(ref)
        d = dt(len(wc) - len(wr))
        gauss = dt(np.exp(dt(-(d * d)) / dt(dt(2) * dt(sigma) * dt(sigma))))
        for n in range(1, 5):
            vc, vr = _vec(wc, n, df, n_doc, dt), _vec(wr, n, df, n_doc, dt)
            nc, nr = _norm(vc, dt), _norm(vr, dt)
            dot = dt(0)
            for g, x in vr.items():
                dot = dt(dot + dt(min(vc.get(g, dt(0)), x) * x))
            if nc > 0 and nr > 0:
                acc[n - 1] = dt(acc[n - 1] + dt(dt(dot / dt(nc * nr)) * gauss))
    parts = [dt(dt(10) * a / dt(len(refs))) for a in acc]
    return dt(sum(parts, dt(0)) / dt(4)), parts


def score_batch(cand, refs, nref, df, n_doc, sigma=6.0, dt=np.float64):
    """cand [rows, T], refs [clips, Rmax, T], nref [clips] -> (scores [rows], parts [rows, 4]) as float64 arrays"""
    cand, refs, nref = np.asarray(cand), np.asarray(refs), np.asarray(nref)
    per = cand.shape[0] // refs.shape[0]
    out, parts = np.zeros(cand.shape[0]), np.zeros((cand.shape[0], 4))
    for r in range(cand.shape[0]):
        c = r // per
        s, p = score(cand[r], [refs[c, j] for j in range(int(nref[c]))], df, n_doc, sigma, dt)
        out[r], parts[r] = float(s), [float(x) for x in p]
    return out, parts


def text_mask(cand):
    """[rows, T] bool: the steps up to and including the first 0"""
    cand = np.asarray(cand)
    m = np.ones(cand.shape, dtype=bool)
    m[:, 1:] = np.cumprod(cand[:, :-1] != 0, axis=1).astype(bool)
    return m


def advantages(reward, per_clip, base=None):
    """fp64: leave-one-out baseline over the clip's own samples (per_clip > 1), or reward - base[clip] -> (adv [rows], sum_k |r_k| of the row's clip)"""
    r = np.asarray(reward, dtype=np.float64).reshape(-1, per_clip)
    mag = np.repeat(np.abs(r).sum(1), per_clip)
    if per_clip > 1:
        adv = r - (r.sum(1, keepdims=True) - r) / (per_clip - 1)
    else:
        adv = r - np.asarray(base, dtype=np.float64).reshape(-1, 1)
        mag = mag + np.abs(np.asarray(base, dtype=np.float64)).reshape(-1)
    return adv.reshape(-1), mag
