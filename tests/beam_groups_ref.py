"""fp64 host restatement of diverse (group) beam search and the length-normalised final ranking (cvc_beam_select_groups_parts,
cvc_beam_rank; DESIGN section 7 "Diverse beam search"): one selection step, the T-step reference decoder on the CPU oracle's decoder
step, and the ranking.  Builds on tests/beam_constrain_ref.py (the candidates, the ban set) without changing it.

beam = G * bd, slot k of a clip belongs to group g = k / bd.  The base candidate c(k, v) is beam_constrain_ref's: score[k] + z[k, v] -
lse[k] over the full row, -inf in the row's ban set, a frozen row offers only (k, 0) at its carried score.  Step 0: only the first
slot of each group is live.  Groups are served in order; pen(v) = the number of slots selected at this step by groups < g whose
parent row was live, whose value was finite (a filler at -inf is no hypothesis) and whose word is v; aug = c - fp32(lambda * pen).
Group g takes the bd best of its bd * V candidates by aug, ties to the lowest flat (k, v), k the clip-wide slot; the j-th best goes to
slot g * bd + j and carries the UNAUGMENTED c.  len(r) = position of the first 0 of r's history + 1, or T; norm = score / len^alpha
(alpha = 0: the score itself); order = the clip's slots by norm descending, ties to the lowest slot, NaN last."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
import constrain_ref as CR
import beam_constrain_ref as BR


def base_candidates(z, score, done, ban, B, beam, groups, first):
    """[B, beam, V] fp64: beam_constrain_ref's candidates; first: only slots k % bd == 0 are live"""
    V = z.shape[1]
    cand = BR.candidates(z, score, done, ban, B, beam, False).view(B, beam, V).clone()
    if first:
        bd = beam // groups
        cand[:, [k for k in range(beam) if k % bd != 0]] = -math.inf
    return cand


def step(z, score, done, hist, t, B, beam, unk, groups=1, lam=0.0, **rules):
    """One step.  z [rows, V] fp32 logits, score [rows], done [rows], hist [rows, >= t] (column s = y_s of the row).
    -> dict(parent, word [B, beam] (parent clip-wide), score [B, beam] fp64 unaugmented, aug [B, beam], done, live, hist
    [rows, t + 1], nbanned [rows], margin [B] (the smallest gap between the bd-th and the (bd + 1)-th augmented candidate of any
    group, and between neighbours among a group's selected ones), augmented: the list over groups of the [B, bd * V] augmented
    values)"""
    rows, V = z.shape
    bd = beam // groups
    assert bd * groups == beam
    hist = np.asarray(hist).reshape(rows, -1)
    ban = CR.banned(hist, t, V, unk, **rules)
    cand = base_candidates(z, score, done, ban, B, beam, groups, t == 0)
    frozen = done.bool().view(B, beam)
    parent = torch.zeros(B, beam, dtype=torch.int64)
    word = torch.zeros(B, beam, dtype=torch.int64)
    val = torch.zeros(B, beam, dtype=torch.float64)
    augv = torch.zeros(B, beam, dtype=torch.float64)
    margin = np.full(B, np.inf)
    pen = torch.zeros(B, V, dtype=torch.float64)                       # counts, per clip and word
    augmented = []
    for g in range(groups):
        ks = slice(g * bd, (g + 1) * bd)
        lp = torch.from_numpy((np.float32(lam) * pen.numpy().astype(np.float32)).astype(np.float64))    # one rounded fp32 multiply
        aug = cand[:, ks] - torch.where(frozen[:, ks].unsqueeze(2), torch.zeros(B, 1, V, dtype=torch.float64), lp.view(B, 1, V))
        aug = aug.reshape(B, bd * V)
        augmented.append(aug)
        v, i = torch.sort(aug, dim=1, descending=True, stable=True)
        kk, vv = g * bd + i[:, :bd] // V, i[:, :bd] % V
        parent[:, ks], word[:, ks], augv[:, ks] = kk, vv, v[:, :bd]
        val[:, ks] = cand.view(B, beam * V).gather(1, kk * V + vv)
        for b in range(B):
            top = v[b, :bd + 1]
            top = top[torch.isfinite(top)]
            if len(top) >= 2:
                margin[b] = min(margin[b], float((top[:-1] - top[1:]).min()))
            for j in range(bd):
                if not bool(frozen[b, kk[b, j]]) and math.isfinite(float(v[b, j])):
                    pen[b, vv[b, j]] += 1
    src = (parent + torch.arange(B).view(-1, 1) * beam).view(-1).numpy()
    hist_out = np.concatenate([hist[src, :t], word.view(-1, 1).numpy()], 1)
    done_out = frozen.gather(1, parent) | (word == 0)
    return dict(parent=parent, word=word, score=val, aug=augv, done=done_out, live=torch.isfinite(augv), hist=hist_out,
                nbanned=ban.sum(1).astype(np.int64), margin=margin, augmented=augmented)


def lengths(seq):
    """seq [..., T] -> position of the first 0 + 1, or T"""
    seq = np.asarray(seq)
    T = seq.shape[-1]
    zero = seq == 0
    return np.where(zero.any(-1), zero.argmax(-1) + 1, T).astype(np.int64)


def rank(seq, score, alpha):
    """seq [B, beam, T], score [B, beam] -> dict(len [B, beam], norm [B, beam] fp64, order [B, beam], margin: the smallest gap
    between neighbours of the finite part of the norm order)"""
    ln = lengths(seq)
    sc = np.asarray(score, dtype=np.float64)
    norm = sc if alpha == 0 else sc / np.power(ln.astype(np.float64), np.float64(alpha))
    key = np.where(np.isnan(norm), -np.inf, norm)
    B, beam = norm.shape
    order = np.zeros((B, beam), dtype=np.int64)
    margin = np.inf
    for b in range(B):
        order[b] = sorted(range(beam), key=lambda k: (bool(np.isnan(norm[b, k])), -key[b, k], k))
        v = norm[b, order[b]]
        v = v[np.isfinite(v)]
        if len(v) >= 2:
            margin = min(margin, float((v[:-1] - v[1:]).min()))
    return dict(len=ln, norm=norm, order=order, margin=margin)


def decode(P, feats, T, unk, beam, groups=1, lam=0.0, alpha=0.0, softattn_type="additive", **rules):
    """The T-step reference decoder, shaped like beam_constrain_ref.decode.  -> dict(seq [B, beam, T] all hypotheses in slot order,
    score [B, beam] fp64, nbanned [T, rows], margin [B, T] (selection), parent / word [T, B, beam], len, norm, order, rank_margin,
    group [beam])"""
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
    nb, margin, parents, wordss = [], [], [], []
    for t in range(T):
        e = O.embed(P, words)
        out, state, _, _, _ = O.decoder_step(P, e, fc, conv, pconv, pool, ppool, m, state, None, softattn_type=softattn_type)
        z = F.linear(out, P["logit.weight"], P["logit.bias"])
        r = step(z, score, done, hist, t, B, beam, unk, groups, lam, **rules)
        margin.append(r["margin"])
        nb.append(r["nbanned"])
        parents.append(r["parent"])
        wordss.append(r["word"])
        gidx = (r["parent"] + torch.arange(B).view(-1, 1) * beam).view(-1)
        state = (state[0][:, gidx], state[1][:, gidx])
        score, done, hist, words = r["score"].reshape(-1), r["done"].reshape(-1), r["hist"], r["word"].reshape(-1)
    seq = torch.from_numpy(hist).view(B, beam, T)
    rk = rank(seq.numpy(), score.view(B, beam).numpy(), alpha)
    return dict(seq=seq, score=score.view(B, beam), nbanned=np.stack(nb, 0), margin=np.stack(margin, 1), parent=torch.stack(parents, 0),
                word=torch.stack(wordss, 0), len=rk["len"], norm=rk["norm"], order=rk["order"], rank_margin=rk["margin"],
                group=np.arange(beam) // (beam // groups))


def aug_gap_violations(r, gap):
    """pairs of augmented candidates of one group and clip that are neither exactly tied nor at least `gap` apart (finite values)"""
    bad = []
    for g, aug in enumerate(r["augmented"]):
        for b in range(aug.shape[0]):
            u = torch.unique(aug[b][torch.isfinite(aug[b])])
            d = u[1:] - u[:-1]
            if bool(((d > 0) & (d < gap)).any()):
                bad.append((g, b, float(d[d > 0].min())))
    return bad


# (checkpoint, seed, beam, groups, lambda, alpha, eos, rules): chosen on this reference so that its smallest margins exceed
# MARGIN_MIN.  eos is added to word 0's logit bias: the synthetic checkpoints never stop on their own, and a length penalty has
# nothing to rank unless hypotheses end at different lengths.
ENGINE_CASES = [("tiny", 4321, 6, 3, 0.5, 0.0, 0.0, {}), ("tiny", 1, 6, 3, 0.25, 0.7, 0.6, dict(no_repeat_ngram=3, min_len=2)),
                ("tiny", 4321, 6, 6, 1.0, 0.7, 0.6, {}), ("tiny", 7, 6, 2, 0.5, 1.0, 0.9, dict(no_repeat_ngram=2)),
                ("cfg1", 1, 4, 2, 0.5, 1.0, 0.9, dict(no_repeat_ngram=2)), ("cfg1", 1, 4, 4, 1.0, 0.7, 0.6, {}),
                ("cfg1", 1, 3, 1, 0.0, 1.0, 0.9, dict(no_repeat_ngram=2)), ("cfg1", 5, 6, 6, 0.5, 0.0, 0.0, {})]
MARGIN_MIN = BR.MARGIN_MIN      # the project's beam score tolerance
_DECODES = {}


def case_inputs(i):
    """-> (d, state dict (numpy, word 0's logit bias raised by the case's eos), clip features (numpy))"""
    from cvc import synth
    name, seed, beam, groups, lam, alpha, eos, rules = ENGINE_CASES[i]
    d = synth.CONFIGS[name]
    sd = dict(synth.hot_path_state_dict(d, seed))
    sd["logit.bias"] = np.array(sd["logit.bias"], copy=True)
    sd["logit.bias"][0] += np.float32(eos)
    return d, sd, synth.clip_features(d, seed)


def shared_decode(i):
    """case i of ENGINE_CASES decoded once per process and left unchanged -> (d, P, feats, result)"""
    from cvc import synth
    if i not in _DECODES:
        name, seed, beam, groups, lam, alpha, eos, rules = ENGINE_CASES[i]
        d, sd, f_np = case_inputs(i)
        P, f = O.to_torch(sd), O.to_torch(f_np)
        with torch.no_grad():
            _DECODES[i] = (d, P, f, decode(P, f, d.T, synth.UNK_IDX, beam, groups, lam, alpha, **rules))
    return _DECODES[i]
