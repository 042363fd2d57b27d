"""fp64 host restatement of constrained beam search (cvc_beam_select_hist_parts, DESIGN section 7 "Constrained beam search"): one
selection step over hypotheses that carry their own histories, and the T-step reference decoder on the CPU oracle's decoder step.
Builds on tests/constrain_ref.py (the ban set, by brute force from the rule) without changing it.

Hypothesis row r = b * beam + k enters step t with history y_0 .. y_{t-1} (its own path from the root; BOS is not history).
A live row's candidate (k, v) is score[k] + z[k, v] - lse[k], the log-sum-exp over the full row; -inf for v in Ban(t, r).  A frozen
row offers (k, 0) at its carried score and the ban is not applied to it.  Step 0: only row 0 of a clip is live.  The `beam` best of a
clip, ties to the lowest flat (k, v); the histories are gathered with the parents and the word is appended."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
import constrain_ref as CR


def row_lse(x):
    m = x.max(1, keepdim=True).values
    return (m + torch.log(torch.exp(x - m).sum(1, keepdim=True))).view(-1)


def candidates(z, score, done, ban, B, beam, first):
    """[B, beam * V] fp64 candidate values of one step (ban: bool [rows, V], UNK included)"""
    x = z.double()
    V = x.shape[1]
    sc = score.double().view(-1, 1)
    cand = sc + (x - row_lse(x).view(-1, 1))
    cand[torch.from_numpy(np.asarray(ban))] = -math.inf
    frozen = torch.full_like(cand, -math.inf)
    frozen[:, 0] = sc[:, 0]
    cand = torch.where(done.bool().view(-1, 1), frozen, cand).view(B, beam, V).clone()
    if first:
        cand[:, 1:] = -math.inf
    return cand.view(B, beam * V)


def select(cand, beam, V):
    """stable sort over the flat (k, v) index -> sorted values, parent, word, score of the `beam` best"""
    v, i = torch.sort(cand, dim=1, descending=True, stable=True)
    return v, i[:, :beam] // V, i[:, :beam] % V, v[:, :beam]


def step(z, score, done, hist, t, B, beam, unk, **rules):
    """One step.  z [rows, V] fp32 logits, score [rows], done [rows], hist [rows, >= t] (column s = y_s of the row).
    -> dict(parent, word, score [B, beam] fp64, done [B, beam] bool, live, hist [rows, t + 1], nbanned [rows], sorted [B, beam * V])"""
    rows, V = z.shape
    hist = np.asarray(hist).reshape(rows, -1)
    ban = CR.banned(hist, t, V, unk, **rules)
    cand = candidates(z, score, done, ban, B, beam, t == 0)
    srt, parent, word, val = select(cand, beam, V)
    src = (parent + torch.arange(B).view(-1, 1) * beam).view(-1).numpy()
    hist_out = np.concatenate([hist[src, :t], word.view(-1, 1).numpy()], 1)
    done_out = done.bool().view(B, beam).gather(1, parent) | (word == 0)
    return dict(parent=parent, word=word, score=val, done=done_out, live=torch.isfinite(val), hist=hist_out,
                nbanned=ban.sum(1).astype(np.int64), sorted=srt)


def margin_of(srt, beam):
    """[B]: the smallest gap between neighbours among the best beam + 1 finite candidates (inf with fewer than two)"""
    out = np.full(srt.shape[0], np.inf)
    for b in range(srt.shape[0]):
        v = srt[b, :beam + 1]
        v = v[torch.isfinite(v)]
        if len(v) >= 2:
            out[b] = float((v[:-1] - v[1:]).min())
    return out


def decode(P, feats, T, unk, beam, softattn_type="additive", **rules):
    """The T-step reference decoder, shaped like oracle.ref_cpu.beam_search (the model's step in fp32, the selection in fp64).
    -> dict(seq [B, beam, T] all hypotheses in rank order, score [B, beam] fp64, nbanned [T, rows], fired [B, T] (the step's
    selection differs from the one with UNK alone banned), margin [B, T], parent / word [T, B, beam])"""
    B, R = feats["fc_feats"].shape
    rep = lambda x: x.repeat_interleave(beam, 0)
    fc, conv, pconv, pool, ppool = [rep(feats[k]) for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats")]
    m = rep(feats["pnt_mask"][:, 1:])
    rows = B * beam
    state = O.init_hidden(rows, R)
    words = torch.zeros(rows, dtype=torch.long)
    score = torch.zeros(rows, dtype=torch.float64)
    done = torch.zeros(rows, dtype=torch.bool)
    hist = np.zeros((rows, 0), dtype=np.int64)
    nb, fired, margin, parents, wordss = [], [], [], [], []
    for t in range(T):
        e = O.embed(P, words)
        out, state, _, _, _ = O.decoder_step(P, e, fc, conv, pconv, pool, ppool, m, state, None, softattn_type=softattn_type)
        z = F.linear(out, P["logit.weight"], P["logit.bias"])
        r = step(z, score, done, hist, t, B, beam, unk, **rules)
        free = step(z, score, done, hist, t, B, beam, unk)
        fired.append(((r["parent"] != free["parent"]) | (r["word"] != free["word"])).any(1).numpy())
        margin.append(margin_of(r["sorted"], beam))
        nb.append(r["nbanned"])
        parents.append(r["parent"])
        wordss.append(r["word"])
        gidx = (r["parent"] + torch.arange(B).view(-1, 1) * beam).view(-1)
        state = (state[0][:, gidx], state[1][:, gidx])
        score, done, hist, words = r["score"].reshape(-1), r["done"].reshape(-1), r["hist"], r["word"].reshape(-1)
    return dict(seq=torch.from_numpy(hist).view(B, beam, T), score=score.view(B, beam), nbanned=np.stack(nb, 0),
                fired=np.stack(fired, 1), margin=np.stack(margin, 1), parent=torch.stack(parents, 0), word=torch.stack(wordss, 0))


def cut(row):
    """a hypothesis up to (not including) its first 0: frozen rows emit 0s after they end"""
    row = [int(w) for w in row]
    return row[:row.index(0)] if 0 in row else row


def repeats_ngram(row, n):
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(set(grams)) < len(grams)


def backtrack_all(words, parent):
    """words / parent [T, B, beam] -> [B, beam, T]: every final rank walked back through the parents (the n-best form of the
    engine's _backtrack_host)"""
    T, B, beam = words.shape
    k = torch.arange(beam).view(1, beam).expand(B, beam).clone()
    seq = []
    for t in range(T - 1, -1, -1):
        seq.append(words[t].gather(1, k))
        k = parent[t].gather(1, k)
    seq.reverse()
    return torch.stack(seq, 2)


# the cases of the issue's table: (checkpoint, seed, beam, rules) with clips fired and margins measured on this reference
ENGINE_CASES = [("tiny", 4321, 2, dict(no_repeat_ngram=1)), ("tiny", 4321, 2, dict(no_repeat_ngram=2)),
                ("tiny", 4321, 2, dict(no_repeat_ngram=3)), ("cfg1", 4321, 2, dict(no_repeat_ngram=2)),
                ("cfg1", 4321, 3, dict(no_repeat_ngram=2)), ("cfg1", 1, 3, dict(no_repeat_ngram=2)),
                ("cfg1", 5, 5, dict(no_repeat_ngram=3))]
MARGIN_MIN = 2e-4               # the score tolerance of test_beam5_cfg1_vs_oracle / test_cfg5_dims_beam_and_greedy_vs_oracle
_DECODES = {}


def shared_decode(i):
    """case i of ENGINE_CASES decoded once per process and left unchanged -> (d, P, feats, result)"""
    from cvc import synth
    if i not in _DECODES:
        name, seed, beam, rules = ENGINE_CASES[i]
        d = synth.CONFIGS[name]
        P, f = O.to_torch(synth.hot_path_state_dict(d, seed)), O.to_torch(synth.clip_features(d, seed))
        with torch.no_grad():
            _DECODES[i] = (d, P, f, decode(P, f, d.T, synth.UNK_IDX, beam, **rules))
    return _DECODES[i]
