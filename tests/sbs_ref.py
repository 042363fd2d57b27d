"""fp64 host restatement of stochastic beam search (cvc_beam_select_stoch_parts, DESIGN section 7 "Stochastic beam search"; Kool,
van Hoof and Welling 2019): one selection step over hypotheses that carry their own histories, the toy the statistics are checked
on, and the T-step reference decoder on the CPU oracle's decoder step.  Builds on tests/constrain_ref.py (the ban set) and
tests/sample_oracle.py (the hash noise, the chi-square helpers) without changing them.

Row r = b * beam + k enters step t with its history, score[r] (the sum of the model's log-probs), logq[r] (its sampling log-prob)
and G[r] (its perturbed key); at t = 0 only slot 0 of a clip is live, with logq = G = 0.  A live row's candidates are the words
outside Ban(t, r); lseq = log-sum-exp of z / tau over the candidates only; phi = logq + (z / tau - lseq); g = phi + gumbel(hash(seed,
call, SBS_SITE + t, r * V + v)); Z = max_v g; the key is gt = -log(exp(-G) - exp(-Z) + exp(-g)) in its stable form.  A frozen row
offers (k, 0) at G with logq and score carried; a row at G = -inf or with every word banned offers -inf.  The `beam` largest gt of a
clip, ties to the lowest flat (k, v), slot i = the i-th; score_out = score + (z - lse) with the full-row lse."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

from cvc import synth
import constrain_ref as CR
import sample_oracle as SO

SBS_SITE = 0x42000000             # include/cvc_hip_blocks.h, CVC_SBS_SITE
LN2 = math.log(2.0)


def noise(seed: int, call: int, t: int, rows: int, V: int) -> np.ndarray:
    """[rows, V] fp64 Gumbel noise of step t: element (r, v) at hash counter (r * V + v) mod 2^32, site SBS_SITE + t"""
    lo, hi = SO.seed_words(seed)
    idx = (np.arange(rows * V, dtype=np.uint64) & 0xFFFFFFFF).astype(np.uint32)
    return SO.gumbel_from_hash(synth.dropout_hash(lo, hi, call, SBS_SITE + t, idx)).reshape(rows, V)


def condition(G, Z, g):
    """gt = -log(exp(-G) - exp(-Z) + exp(-g)) for g <= Z, in the stable form of the header; -inf where g or G is -inf.  No NaN."""
    G, Z, g = np.broadcast_arrays(np.asarray(G, np.float64), np.asarray(Z, np.float64), np.asarray(g, np.float64))
    out = np.full(g.shape, -np.inf)
    ok = np.isfinite(g) & np.isfinite(G) & np.isfinite(Z)
    d = np.minimum(g[ok] - Z[ok], 0.0)
    with np.errstate(divide="ignore"):
        l = np.where(d > -LN2, np.log(-np.expm1(d)), np.log1p(-np.exp(d)))            # d == 0: -inf
    u = (G[ok] - g[ok]) + l
    out[ok] = G[ok] - np.maximum(u, 0.0) - np.log1p(np.exp(-np.abs(u)))
    return out


def _lse(x, axis):
    m = x.max(axis, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide="ignore"):
        return (ms + np.log(np.exp(x - ms).sum(axis, keepdims=True))).squeeze(axis)


def step(z, score, logq, G, done, hist, t, B, beam, unk, tau, gum, ban=None, **rules):
    """One step, vectorised over the clips.  z [rows, V] logits (any float type), score / logq / G [rows], done [rows] bool, hist
    [rows, >= t], gum [rows, V] = noise(...).  ban: bool [rows, V] to use instead of the rules (UNK included).
    -> dict(parent, word [B, beam] int64; score, logq, G [B, beam] fp64; done [B, beam] bool; live; hist [rows, t + 1]; nbanned
    [rows]; sorted [B, beam + 1] the best beam + 1 keys; margin [B])"""
    z = np.asarray(z, dtype=np.float64)
    rows, V = z.shape
    score, logq, G = (np.asarray(a, dtype=np.float64).reshape(rows).copy() for a in (score, logq, G))
    done = np.asarray(done).astype(bool).reshape(rows)
    hist = np.asarray(hist).reshape(rows, -1)
    if ban is None:
        ban = CR.banned(hist, t, V, unk, **rules)
    ban = np.asarray(ban, dtype=bool)
    if t == 0:
        G.reshape(B, beam)[:, 1:] = -np.inf
    zt = np.where(ban, -np.inf, z / tau)
    lseq = _lse(zt, 1)
    lse = _lse(z, 1)
    with np.errstate(invalid="ignore"):
        phi = logq[:, None] + (zt - lseq[:, None])
    phi[ban | ~np.isfinite(lseq)[:, None]] = -np.inf
    g = np.where(np.isfinite(phi) & np.isfinite(G)[:, None], phi + gum, -np.inf)
    Z = g.max(1)
    key = condition(G[:, None], Z[:, None], g)
    sc = np.where(np.isfinite(key), score[:, None] + (z - lse[:, None]), -np.inf)
    # frozen rows: (k, 0) at the carried key, logq and score
    fr = done
    key[fr] = -np.inf
    key[fr, 0] = G[fr]
    phi[fr] = -np.inf
    phi[fr, 0] = np.where(np.isfinite(G[fr]), logq[fr], -np.inf)
    sc[fr] = -np.inf
    sc[fr, 0] = np.where(np.isfinite(G[fr]), score[fr], -np.inf)
    key = key.reshape(B, beam * V)
    order = np.argsort(-key, axis=1, kind="stable")[:, :beam + 1]           # ties -> lowest flat (k, v)
    srt = np.take_along_axis(key, order, 1)
    top = order[:, :beam]
    parent, word = top // V, top % V
    take = lambda a: np.take_along_axis(a.reshape(B, beam * V), top, 1)
    src = (parent + np.arange(B)[:, None] * beam).reshape(-1)
    hist_out = np.concatenate([hist[src, :t], word.reshape(-1, 1)], 1)
    done_out = done[src].reshape(B, beam) | (word == 0)
    with np.errstate(invalid="ignore"):
        gaps = srt[:, :-1] - srt[:, 1:]                                      # inf - ... handled below
    gaps = np.where(np.isfinite(srt[:, :-1]) & np.isfinite(srt[:, 1:]), gaps, np.inf)
    return dict(parent=parent, word=word, score=take(sc), logq=take(phi), G=srt[:, :beam], done=done_out,
                live=np.isfinite(srt[:, :beam]), hist=hist_out, nbanned=ban.sum(1).astype(np.int64), sorted=srt,
                margin=gaps.min(1))


# ------------------------------------------------------------------ the toy
def toy_table(V: int, T: int, seed: int) -> np.ndarray:
    """[T, V + 1, V] logits of step t after last word w (row w + 1; row 0: BOS), N(0, 1.5)"""
    return np.random.default_rng(seed).normal(0.0, 1.5, size=(T, V + 1, V))


def toy_run(table, trials, beam, tau, seed, call=1, unk=-1):
    """`trials` independent clips through T steps of step(); word 0 ends a caption.  -> hist [trials, beam, T], live [trials, beam],
    G, logq, score [trials, beam]"""
    T, _, V = table.shape
    rows = trials * beam
    score, logq, G = np.zeros(rows), np.zeros(rows), np.zeros(rows)
    done = np.zeros(rows, dtype=bool)
    hist = np.zeros((rows, 0), dtype=np.int64)
    ban = np.zeros((rows, V), dtype=bool)
    if unk >= 0:
        ban[:, unk] = True
    for t in range(T):
        last = hist[:, -1] + 1 if t else np.zeros(rows, dtype=np.int64)
        r = step(table[t][last], score, logq, G, done, hist, t, trials, beam, unk, tau, noise(seed, call, t, rows, V), ban=ban)
        score, logq, G, done, hist = [r[k].reshape(-1) for k in ("score", "logq", "G", "done")] + [r["hist"]]
    return hist.reshape(trials, beam, T), np.isfinite(G).reshape(trials, beam), G.reshape(trials, beam), logq.reshape(trials, beam), \
        score.reshape(trials, beam)


def toy_sequences(table, tau, unk=-1):
    """every caption of the toy (0s after the first 0) with its probability under the per-step renormalised q_tau: (list of tuples,
    fp64 array)"""
    T, _, V = table.shape
    seqs, probs = [], []
    for s in itertools.product(range(V), repeat=T):
        if unk in s or any(a == 0 and b != 0 for a, b in zip(s, s[1:])):
            continue
        p, last, ended = 1.0, 0, False
        for t, w in enumerate(s):
            if ended:
                continue
            zt = table[t][last] / tau
            keep = np.arange(V) != unk
            p *= math.exp(zt[w] - _lse(zt[keep], 0))
            last, ended = w + 1, w == 0
        seqs.append(s)
        probs.append(p)
    return seqs, np.array(probs)


def toy_chi_squares(hist, seqs, probs):
    """hist [trials, >= 2, T] -> ((statistic, df) of slot 0 against p(a), (statistic, df) of the ordered pair (slot 0, slot 1) against
    p(a) p(b) / (1 - p(a)))"""
    index = {s: i for i, s in enumerate(seqs)}
    n = len(seqs)
    a = np.array([index[tuple(int(w) for w in h)] for h in hist[:, 0]])
    b = np.array([index[tuple(int(w) for w in h)] for h in hist[:, 1]])
    first = np.bincount(a, minlength=n)
    pair = np.bincount(a * n + b, minlength=n * n)
    pp = probs[:, None] * probs[None, :] / (1.0 - probs[:, None])
    off = ~np.eye(n, dtype=bool)
    assert pair.reshape(n, n)[~off].sum() == 0, "slot 0 and slot 1 hold the same caption"
    return SO.chi_square(first, probs), SO.chi_square(pair.reshape(n, n)[off], pp[off])


# ------------------------------------------------------------------ the T-step reference decoder
def decode(P, feats, T, unk, beam, tau, seed, call, softattn_type="additive", **rules):
    """shaped like beam_constrain_ref.decode: the model's step in fp32 on the CPU oracle, the selection in fp64.
    -> dict(seq [B, beam, T], score, logq, G [B, beam], live, margin [B, T], parent / word [T, B, beam], nbanned [T, rows])"""
    from oracle import ref_cpu as O
    B, R = feats["fc_feats"].shape
    rep = lambda x: x.repeat_interleave(beam, 0)
    fc, conv, pconv, pool, ppool = [rep(feats[k]) for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats")]
    m = rep(feats["pnt_mask"][:, 1:])
    rows = B * beam
    state = O.init_hidden(rows, R)
    words = torch.zeros(rows, dtype=torch.long)
    score, logq, G = np.zeros(rows), np.zeros(rows), np.zeros(rows)
    done = np.zeros(rows, dtype=bool)
    hist = np.zeros((rows, 0), dtype=np.int64)
    margin, parents, wordss, nb = [], [], [], []
    for t in range(T):
        e = O.embed(P, words)
        out, state, _, _, _ = O.decoder_step(P, e, fc, conv, pconv, pool, ppool, m, state, None, softattn_type=softattn_type)
        z = F.linear(out, P["logit.weight"], P["logit.bias"])
        r = step(z.numpy(), score, logq, G, done, hist, t, B, beam, unk, tau, noise(seed, call, t, rows, z.shape[1]), **rules)
        margin.append(r["margin"])
        parents.append(r["parent"])
        wordss.append(r["word"])
        nb.append(r["nbanned"])
        gidx = torch.from_numpy((r["parent"] + np.arange(B)[:, None] * beam).reshape(-1))
        state = (state[0][:, gidx], state[1][:, gidx])
        score, logq, G, done, hist = [r[k].reshape(-1) for k in ("score", "logq", "G", "done")] + [r["hist"]]
        words = torch.from_numpy(r["word"].reshape(-1))
    return dict(seq=hist.reshape(B, beam, T), score=score.reshape(B, beam), logq=logq.reshape(B, beam), G=G.reshape(B, beam),
                live=np.isfinite(G).reshape(B, beam), margin=np.stack(margin, 1), parent=np.stack(parents, 0),
                word=np.stack(wordss, 0), nbanned=np.stack(nb, 0))
