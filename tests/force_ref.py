"""fp64 host restatement of lexically constrained beam search (cvc_beam_select_force_parts, cvc_beam_rank_force; DESIGN section 7
"Forced words"): one selection step as a full scan over all beam * V candidates with their target banks, the T-step reference
decoder on the CPU oracle's decoder step, the final ranking, and the engine cases.  Builds on tests/beam_constrain_ref.py (the
candidates, the ban set) and tests/beam_groups_ref.py (len, norm) without changing them.

force [B, C] int, C in {1, 2, 3}.  Entry j of clip b is ACTIVE iff 0 < w < V, w != unk and no entry j' < j of the clip holds the same
w; anything else is unused.  beam = (C + 1) * bd, slots [j * bd, (j + 1) * bd) of a clip are bank j.  For row r = (b, k) entering
step t with history y_0 .. y_{t-1}: met(r) = the active entries of clip b whose word occurs in the history, n(r) = |met(r)|.  The base
candidate c(k, v) is beam_constrain_ref's (score[k] + z[k, v] - lse[k] over the full row, -inf in the row's ban set, a frozen row
offers only (k, 0) at its carried score; step 0: only slot 0 is live).  The target bank of (k, v) is n(r) + 1 if r is live and v is an
active forced word of the clip that is not in met(r), else n(r).  Bank j takes the bd best candidates whose target is j over all rows
of the clip, ties to the lowest flat (k, v); the i-th best goes to slot j * bd + i; fewer than bd finite candidates: fillers at -inf
(what else a filler holds is not part of the rule).  Final order of a clip's slots: norm is NaN last, then norm == -inf, then nmet
(counted over the T-step history) descending, norm descending, lowest slot."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
import constrain_ref as CR
import beam_constrain_ref as BR
import beam_groups_ref as GR


def active(words, V, unk):
    """words [C] -> list of bool: the entry is an active forced word"""
    words = [int(w) for w in words]
    return [0 < w < V and w != unk and w not in words[:j] for j, w in enumerate(words)]


def met_sets(force, hist, t, beam, V, unk):
    """force [B, C], hist [rows, >= t] -> list over rows of (the set of active forced words in y_0 .. y_{t-1}, the unmet ones)"""
    out = []
    for r in range(len(hist)):
        f = force[r // beam]
        act = {int(w) for w, a in zip(f, active(f, V, unk)) if a}
        have = act & {int(w) for w in hist[r, :t]}
        out.append((have, act - have))
    return out


def nmet_of(force, hist, t, beam, V, unk):
    return np.array([len(m) for m, _ in met_sets(force, hist, t, beam, V, unk)], dtype=np.int64)


def step(z, score, done, hist, t, B, beam, unk, force, **rules):
    """One step.  z [rows, V] fp32 logits, score [rows], done [rows], hist [rows, >= t] (column s = y_s of the row), force [B, C].
    -> dict(parent, word [B, beam], score [B, beam] fp64, done, live (finite score: not a filler), hist [rows, t + 1], nbanned
    [rows], nmet [rows] (of the INPUT rows), margin [B] (the smallest gap among a bank's best bd + 1 finite candidates), banked:
    the list over banks of the [B, beam * V] candidate values with the other banks' at -inf)"""
    rows, V = z.shape
    force = np.asarray(force).reshape(B, -1)
    C = force.shape[1]
    bd = beam // (C + 1)
    assert bd * (C + 1) == beam and 1 <= C <= 3
    hist = np.asarray(hist).reshape(rows, -1)
    ban = CR.banned(hist, t, V, unk, **rules)
    cand = BR.candidates(z, score, done, ban, B, beam, t == 0).view(B, beam, V)
    sets = met_sets(force, hist, t, beam, V, unk)
    target = torch.zeros(B, beam, V, dtype=torch.int64)
    for r, (have, unmet) in enumerate(sets):
        target[r // beam, r % beam] = len(have)
        if not bool(done[r]):
            for w in unmet:
                target[r // beam, r % beam, w] += 1
    parent = torch.zeros(B, beam, dtype=torch.int64)
    word = torch.zeros(B, beam, dtype=torch.int64)
    val = torch.zeros(B, beam, dtype=torch.float64)
    margin = np.full(B, np.inf)
    banked = []
    for j in range(C + 1):
        ks = slice(j * bd, (j + 1) * bd)
        mine = torch.where(target == j, cand, torch.full_like(cand, -math.inf)).view(B, beam * V)
        banked.append(mine)
        v, i = torch.sort(mine, dim=1, descending=True, stable=True)
        parent[:, ks], word[:, ks], val[:, ks] = i[:, :bd] // V, i[:, :bd] % V, v[:, :bd]
        margin = np.minimum(margin, BR.margin_of(v, bd))
    src = (parent + torch.arange(B).view(-1, 1) * beam).view(-1).numpy()
    hist_out = np.concatenate([hist[src, :t], word.view(-1, 1).numpy()], 1)
    done_out = done.bool().view(B, beam).gather(1, parent) | (word == 0)
    return dict(parent=parent, word=word, score=val, done=done_out, live=torch.isfinite(val), hist=hist_out,
                nbanned=ban.sum(1).astype(np.int64), nmet=np.array([len(m) for m, _ in sets], dtype=np.int64), margin=margin,
                banked=banked)


def invariant_violations(r, force, beam, V, unk):
    """slots of a step's (or a decode's) output with a finite score whose history does not hold exactly `bank` active forced words"""
    hist, score = r["hist"], r["score"].reshape(-1)
    C = np.asarray(force).shape[1]
    bd = beam // (C + 1)
    n = nmet_of(force, hist, hist.shape[1], beam, V, unk)
    return [(row, int(n[row])) for row in range(len(hist)) if math.isfinite(float(score[row])) and n[row] != (row % beam) // bd]


def rank(seq, score, alpha, force, V, unk):
    """seq [B, beam, T], score [B, beam], force [B, C] -> dict(len, norm fp64, nmet [B, beam], order [B, beam], margin: the smallest
    norm gap between neighbours of the order that are finite and have met equally many forced words)"""
    seq = np.asarray(seq)
    B, beam, T = seq.shape
    g = GR.rank(seq, score, alpha)
    ln, norm = g["len"], g["norm"]
    nmet = nmet_of(force, seq.reshape(B * beam, T), T, beam, V, unk).reshape(B, beam)
    order = np.zeros((B, beam), dtype=np.int64)
    margin = np.inf
    for b in range(B):
        nan, ninf = np.isnan(norm[b]), norm[b] == -np.inf
        order[b] = sorted(range(beam), key=lambda k: (bool(nan[k]), bool(ninf[k]), -int(nmet[b, k]),
                                                     0.0 if nan[k] or ninf[k] else -norm[b, k], k))
        for a, c in zip(order[b, :-1], order[b, 1:]):
            if np.isfinite(norm[b, a]) and np.isfinite(norm[b, c]) and nmet[b, a] == nmet[b, c]:
                margin = min(margin, float(norm[b, a] - norm[b, c]))
    return dict(len=ln, norm=norm, nmet=nmet, order=order, margin=margin)


def decode(P, feats, T, unk, beam, force, alpha=0.0, softattn_type="additive", **rules):
    """The T-step reference decoder, shaped like beam_groups_ref.decode.  -> dict(seq [B, beam, T] all hypotheses in slot order, score
    [B, beam] fp64, nbanned / nmet [T, rows] (of the rows entering each step), live [T, B, beam] (the step's non-filler slots), margin
    [B, T] (selection), parent / word [T, B, beam], len, norm, final_nmet, order, rank_margin, bank [beam])"""
    B, R = feats["fc_feats"].shape
    V = P["logit.weight"].shape[0]
    force = np.asarray(force).reshape(B, -1)
    rep = lambda x: x.repeat_interleave(beam, 0)
    fc, conv, pconv, pool, ppool = [rep(feats[k]) for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats")]
    m = rep(feats["pnt_mask"][:, 1:])
    rows = B * beam
    state = O.init_hidden(rows, R)
    words = torch.zeros(rows, dtype=torch.long)
    score = torch.zeros(rows, dtype=torch.float64)
    done = torch.zeros(rows, dtype=torch.bool)
    hist = np.zeros((rows, 0), dtype=np.int64)
    nb, nm, live, margin, parents, wordss = [], [], [], [], [], []
    for t in range(T):
        e = O.embed(P, words)
        out, state, _, _, _ = O.decoder_step(P, e, fc, conv, pconv, pool, ppool, m, state, None, softattn_type=softattn_type)
        z = F.linear(out, P["logit.weight"], P["logit.bias"])
        r = step(z, score, done, hist, t, B, beam, unk, force, **rules)
        assert not invariant_violations(r, force, beam, V, unk)
        margin.append(r["margin"])
        nb.append(r["nbanned"])
        nm.append(r["nmet"])
        live.append(r["live"])
        parents.append(r["parent"])
        wordss.append(r["word"])
        gidx = (r["parent"] + torch.arange(B).view(-1, 1) * beam).view(-1)
        state = (state[0][:, gidx], state[1][:, gidx])
        score, done, hist, words = r["score"].reshape(-1), r["done"].reshape(-1), r["hist"], r["word"].reshape(-1)
    seq = torch.from_numpy(hist).view(B, beam, T)
    rk = rank(seq.numpy(), score.view(B, beam).numpy(), alpha, force, V, unk)
    return dict(seq=seq, score=score.view(B, beam), nbanned=np.stack(nb, 0), nmet=np.stack(nm, 0), live=torch.stack(live, 0),
                margin=np.stack(margin, 1), parent=torch.stack(parents, 0), word=torch.stack(wordss, 0), len=rk["len"], norm=rk["norm"],
                final_nmet=rk["nmet"], order=rk["order"], rank_margin=rk["margin"], bank=np.arange(beam) // (beam // (force.shape[1] + 1)))


def gap_violations(r, gap):
    """pairs of candidates of one bank and clip that are neither exactly tied nor at least `gap` apart (finite values)"""
    bad = []
    for j, vals in enumerate(r["banked"]):
        for b in range(vals.shape[0]):
            u = torch.unique(vals[b][torch.isfinite(vals[b])])
            d = u[1:] - u[:-1]
            if bool(((d > 0) & (d < gap)).any()):
                bad.append((j, b, float(d[d > 0].min())))
    return bad


# (checkpoint, seed, beam, C, alpha, eos, rules): chosen on this reference so that the smallest selection margin and the smallest
# gap of the final norm order exceed MARGIN_MIN.  eos is added to word 0's logit bias (the synthetic checkpoints never stop on their
# own).  The forced words of a case: force_words() below.
ENGINE_CASES = [("tiny", 4321, 4, 1, 0.0, 0.0, {}), ("tiny", 1, 6, 2, 0.7, 0.6, dict(no_repeat_ngram=2)),
                ("tiny", 7, 4, 3, 0.0, 0.0, {}), ("tiny", 11, 8, 3, 0.0, 0.0, {}), ("tiny", 3, 8, 1, 0.7, 0.6, {}),
                ("cfg1", 1, 6, 2, 0.5, 0.9, dict(no_repeat_ngram=2)), ("cfg1", 4321, 3, 2, 0.7, 0.6, {}),
                ("cfg1", 2, 8, 3, 0.7, 0.6, dict(no_repeat_ngram=2))]
MARGIN_MIN = BR.MARGIN_MIN      # the project's beam score tolerance
_DECODES = {}


def force_words(B, C, V, unk, seed):
    """[B, C] int32: per clip C distinct words of [1, V) without UNK from numpy's default_rng(seed); clips with b % 3 == 0 lose their
    last entry (-1)"""
    rng = np.random.default_rng(seed)
    pool = np.array([w for w in range(1, V) if w != unk])
    out = np.stack([rng.choice(pool, size=C, replace=False) for _ in range(B)]).astype(np.int32)
    out[::3, C - 1] = -1
    return out


def case_inputs(i):
    """-> (d, state dict (numpy, word 0's logit bias raised by the case's eos), clip features (numpy), force [B, C] int32)"""
    from cvc import synth
    name, seed, beam, C, alpha, eos, rules = ENGINE_CASES[i]
    d = synth.CONFIGS[name]
    sd = dict(synth.hot_path_state_dict(d, seed))
    sd["logit.bias"] = np.array(sd["logit.bias"], copy=True)
    sd["logit.bias"][0] += np.float32(eos)
    return d, sd, synth.clip_features(d, seed), force_words(d.B, C, d.V, synth.UNK_IDX, seed)


def shared_decode(i):
    """case i of ENGINE_CASES decoded once per process and left unchanged -> (d, P, feats, force, result)"""
    from cvc import synth
    if i not in _DECODES:
        name, seed, beam, C, alpha, eos, rules = ENGINE_CASES[i]
        d, sd, f_np, force = case_inputs(i)
        P, f = O.to_torch(sd), O.to_torch(f_np)
        with torch.no_grad():
            _DECODES[i] = (d, P, f, force, decode(P, f, d.T, synth.UNK_IDX, beam, force, alpha, **rules))
    return _DECODES[i]
