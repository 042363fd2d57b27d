"""fp64 host restatement of constrained decoding (cvc_constrained_select_parts): the ban set straight from the rule
by brute force, the selection over the allowed words, and the T-step reference decoder that applies both per step.  Builds on
tests/sample_oracle.py (noise, decoder step) and tests/sample_trunc_ref.py (the candidate sets of top-k / top-p) without changing
them.

Step t chooses y_t for a row with history y_0 .. y_{t-1} (BOS is not history).  Ban(t, row) is the union of {unk}, ban_words,
every v for which some j, n-1 <= j <= t-1, has y_j = v and y_{j-n+1 .. j-1} = y_{t-n+1 .. t-1} (no_repeat_ngram = n >= 1),
y_{t-1} (no_immediate_repeat, t >= 1), word 0 while t < min_len, word 0 when t >= 1 and y_{t-1} is in bad_endings."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
import sample_oracle as S
import sample_trunc_ref as R


def banned(hist, t: int, V: int, unk: int, no_repeat_ngram: int = 0, no_immediate_repeat: bool = False, min_len: int = 0,
           ban_words=(), bad_endings=()) -> np.ndarray:
    """hist [rows, >= t] word ids (column s = y_s; columns from t on are ignored) -> bool [rows, V].  Ids outside [0, V) ban
    nothing."""
    hist = np.asarray(hist).reshape(len(hist), -1)
    rows, n = hist.shape[0], int(no_repeat_ngram)
    out = np.zeros((rows, V), dtype=bool)

    def ban(r, v):
        if 0 <= v < V:
            out[r, int(v)] = True

    for r in range(rows):
        y = [int(w) for w in hist[r, :t]]
        ban(r, unk)
        for v in ban_words:
            ban(r, v)
        if n >= 1:
            for j in range(n - 1, t):                            # n-1 <= j <= t-1
                if y[j - n + 1:j] == y[t - n + 1:t]:             # the n - 1 words before y_j against the last n - 1 words
                    ban(r, y[j])
        if no_immediate_repeat and t >= 1:
            ban(r, y[t - 1])
        if t < min_len:
            ban(r, 0)
        if t >= 1 and y[t - 1] in set(int(v) for v in bad_endings):
            ban(r, 0)
    return out


def select(z, ban: np.ndarray, noise, inv_tau: float, top_k: int = 0, top_p: float = 1.0, tol: float = R.MASS_TOL, ztol: float = 0.0):
    """z [rows, V] fp32 logits, ban bool [rows, V].  noise None: the arg-max mode (inv_tau, top_k, top_p unused) -- s = z; else
    s = z * inv_tau + noise.  The word is the arg-max of s over the allowed words (lower index on ties), with top_k / top_p over
    the C2 of tests/sample_trunc_ref.py computed on the allowed words only (the j_lo end of its band).  Returns words, the fp64
    scores (-inf outside the candidates), the fp64 log-prob of each word over the full row, and info: j_lo, j_hi, unambiguous
    (False where the two ends of the band pick different words), empty (no allowed word: word 0, log-prob -inf)."""
    zd = z.double().numpy() if isinstance(z, torch.Tensor) else np.asarray(z, dtype=np.float64)
    zt = torch.from_numpy(np.asarray(zd, dtype=np.float32))
    rows, V = zd.shape
    s = zd.copy() if noise is None else zd * float(inv_tau) + noise
    trunc = noise is not None and (top_k > 0 or top_p < 1.0)
    out = np.full_like(s, -np.inf)
    word, w_hi = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    j_lo, j_hi = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    for r in range(rows):
        allowed = np.flatnonzero(~ban[r])
        if len(allowed) == 0:
            continue
        lo = hi = allowed
        if trunc:                                                # sample_trunc_ref's sets on the row without its banned columns
            tau = 1.0 / float(inv_tau)
            assert float(np.float32(1.0 / tau)) == float(inv_tau)
            orders, a, b = R.truncate(zt[r:r + 1, allowed], tau, -1, top_k, top_p, tol, ztol)
            lo, hi = allowed[orders[0][:a[0]]], allowed[orders[0][:b[0]]]
        j_lo[r], j_hi[r] = len(lo), len(hi)
        out[r, lo] = s[r, lo]
        word[r] = int(np.argmax(out[r]))
        sh = np.full(V, -np.inf)
        sh[hi] = s[r, hi]
        w_hi[r] = int(np.argmax(sh))
    m = zd.max(1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        lse = m[:, 0] + np.log(np.exp(zd - m).sum(1))
    empty = ~(~ban).any(1)
    lp = zd[np.arange(rows), word] - lse
    lp[empty] = -np.inf
    return word, out, lp, dict(j_lo=j_lo, j_hi=j_hi, unambiguous=word == w_hi, empty=empty)


def decode(P, feats, T: int, unk_idx: int, n: int = 1, tau=None, seed: int = 0, call: int = 1, top_k: int = 0, top_p: float = 1.0,
           tol: float = R.MASS_TOL, ztol: float = 0.0, softattn_type: str = "additive", temp: float = 1.0, **rules):
    """sample_oracle.sample with the rule applied per step (rules: the keyword arguments of banned()).  tau None: the arg-max
    mode (no noise, n = 1).  Returns seq [B*n, T], att2, logprob (fp32, the model's), the fp64 scores [rows, T, V] (-inf outside the
    candidates) and info: nbanned [rows, T], fired [rows, T] (the word the same step would choose with UNK alone banned lies in the
    ban set), unambiguous [rows, T]."""
    rep = lambda x: x.repeat_interleave(n, 0)
    fc, conv, pconv, pool, ppool = (rep(feats[k]) for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats"))
    mask = rep(feats["pnt_mask"][:, 1:])
    rows = fc.shape[0]
    state = O.init_hidden(rows, fc.shape[1])
    word = torch.zeros(rows, dtype=torch.long)
    inv_tau = 0.0 if tau is None else float(np.float32(1.0 / tau))
    hist = np.zeros((rows, T), dtype=np.int64)
    seq, atts, lps, scores, nb, fired, oks = [], [], [], [], [], [], []
    for t in range(T):
        e = O.embed(P, word)
        out, state, a_r, _, _ = O.decoder_step(P, e, fc, conv, pconv, pool, ppool, mask, state, None,
                                               softattn_type=softattn_type, temp=temp)
        z = F.linear(out, P["logit.weight"], P["logit.bias"])
        V = z.shape[1]
        noise = None if tau is None else S.gumbel_noise(seed, call, t, rows, V)
        ban = banned(hist, t, V, unk_idx, **rules)
        w, s, _, info = select(z, ban, noise, inv_tau, top_k, top_p, tol, ztol)
        only_unk = banned(hist, t, V, unk_idx)
        w0, _, _, _ = select(z, only_unk, noise, inv_tau, top_k, top_p, tol, ztol)
        hist[:, t] = w
        word = torch.from_numpy(w)
        logp = F.log_softmax(z, dim=1)
        seq.append(word)
        atts.append(a_r)
        lps.append(logp[torch.arange(rows), word])
        scores.append(s)
        nb.append(ban.sum(1))
        fired.append(ban[np.arange(rows), w0])
        oks.append(info["unambiguous"])
    info = dict(nbanned=np.stack(nb, 1), fired=np.stack(fired, 1), unambiguous=np.stack(oks, 1))
    return torch.stack(seq, 1), torch.stack(atts, 1), torch.stack(lps, 1), np.stack(scores, 1), info


def repeats_ngram(seq, n: int) -> np.ndarray:
    """bool [rows]: the row holds some n-gram twice (windows over the whole row; BOS not included)"""
    seq = np.asarray(seq)
    out = np.zeros(len(seq), dtype=bool)
    for r, row in enumerate(seq):
        grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
        out[r] = len(set(grams)) < len(grams)
    return out
