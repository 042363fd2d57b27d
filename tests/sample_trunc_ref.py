"""fp64 reference of top-k / nucleus (top-p) truncated sampling (cvc_sample_select_trunc_parts): the candidate
sets of the contract computed on the fp32 logits in fp64, and the T-step reference sampler with truncation.  Builds on
tests/sample_oracle.py (noise, decoder step) without changing it.

The top-k set is exact (it depends on fp32 values only).  The top-p cutoff compares an fp32 sum with p * total, so the reference
gives a BAND of prefix lengths [j_lo, j_hi] of the value-sorted candidates: j_lo is the first prefix whose fp64 mass reaches
(p - tol) * total, j_hi the first that reaches (p + tol) * total, both extended over ties.  MASS_TOL = 2e-5 relative is derived,
not measured: the fp32 mass is at most 32 sequential adds and 8 reduction levels (about 40 * 2^-24 = 2.4e-6), the exponent's
argument (z - m) * inv_tau carries two roundings at |arg| <~ 30 (2 * 30 * 2^-24 = 3.6e-6 relative on e), expf adds a few ulp:
about 6e-6 in all, and the tolerance leaves a factor 3."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
import sample_oracle as S

MASS_TOL = 2e-5


def _extend(vals: np.ndarray, j: int) -> int:
    """prefix length j extended over the words tied with its last value"""
    return int(np.searchsorted(-vals, -vals[j - 1], side="right"))


def truncate(z, tau: float, unk: int, top_k: int = 0, top_p: float = 1.0, tol: float = MASS_TOL, ztol: float = 0.0):
    """z [rows, V] fp32 logits.  Per row: order (the words of C0 by falling logit, ties by rising index), j_lo, j_hi.
    C2 is order[:j] for a j in [j_lo, j_hi]; top-k only (top_p = 1): j_lo = j_hi = |C1|.  ztol > 0 (logits known only up to
    +-ztol, as an engine's against the CPU oracle's) also widens the top-k end of the band."""
    zd = (z.double().numpy() if isinstance(z, torch.Tensor) else np.asarray(z, dtype=np.float64))
    inv_tau = float(np.float32(1.0 / tau))                      # what the block is handed
    rows, V = zd.shape
    orders, j_lo, j_hi = [], np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    cand = np.delete(np.arange(V), unk) if 0 <= unk < V else np.arange(V)
    for r in range(rows):
        zr = zd[r, cand]
        o = np.argsort(-zr, kind="stable")
        order, vals = cand[o], zr[o]
        n_in = n_out = len(vals)
        if 0 < top_k < len(vals):
            th = vals[top_k - 1]
            if ztol > 0:        # two logits move against each other by at most 2 ztol: surely inside = above the (k+1)-th by more
                n_in = max(1, int((vals > vals[top_k] + 2.0 * ztol).sum()))
                n_out = int((vals >= th - 2.0 * ztol).sum())
            else:
                n_in = n_out = int((vals >= th).sum())
        lo, hi = n_in, n_out
        if top_p < 1.0:
            e = np.exp((vals[:n_out] - vals[0]) * inv_tau)
            cum = np.cumsum(e)
            first = lambda target: int(np.searchsorted(cum, target, side="left")) + 1       # first prefix with cum >= target
            lo = min(n_in, _extend(vals, max(1, first((top_p - tol) * cum[n_in - 1]))))
            need = (top_p + tol) * cum[-1]
            hi = n_out if need > cum[-1] else min(n_out, _extend(vals, first(need)))
        orders.append(order)
        j_lo[r], j_hi[r] = lo, max(lo, hi)
    return orders, j_lo, j_hi


def select(z: torch.Tensor, noise: np.ndarray, tau: float, unk: int, orders, j):
    """Gumbel-max over the prefix order[:j[r]] of every row: words, fp64 perturbed scores (-inf outside the prefix)"""
    s = z.double().numpy() * float(np.float32(1.0 / tau)) + noise
    out = np.full_like(s, -np.inf)
    for r, (o, jr) in enumerate(zip(orders, j)):
        out[r, o[:jr]] = s[r, o[:jr]]
    return np.argmax(out, axis=1), out


def sample(P, feats, T: int, unk_idx: int, n: int, tau: float, seed: int, call: int, top_k: int = 0, top_p: float = 1.0,
           tol: float = MASS_TOL, ztol: float = 0.0, softattn_type: str = "additive", temp: float = 1.0):
    """S.sample with truncation.  The reference follows the word of the j_lo prefix.  Returns seq, att2, logprob, the fp64
    perturbed scores [rows, T, V] (-inf outside the j_lo prefix) and info: j_lo, j_hi [rows, T] and `unambiguous` [rows, T] --
    False where the band is wider than one point AND its two ends pick different words."""
    rep = lambda x: x.repeat_interleave(n, 0)
    fc, conv, pconv, pool, ppool = (rep(feats[k]) for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats"))
    mask = rep(feats["pnt_mask"][:, 1:])
    rows = fc.shape[0]
    state = O.init_hidden(rows, fc.shape[1])
    word = torch.zeros(rows, dtype=torch.long)
    seq, atts, lps, scores, los, his, oks = [], [], [], [], [], [], []
    for t in range(T):
        e = O.embed(P, word)
        out, state, a_r, _, _ = O.decoder_step(P, e, fc, conv, pconv, pool, ppool, mask, state, None,
                                               softattn_type=softattn_type, temp=temp)
        z = F.linear(out, P["logit.weight"], P["logit.bias"])
        noise = S.gumbel_noise(seed, call, t, rows, z.shape[1])
        orders, j_lo, j_hi = truncate(z, tau, unk_idx, top_k, top_p, tol, ztol)
        w, s = select(z, noise, tau, unk_idx, orders, j_lo)
        w_hi, _ = select(z, noise, tau, unk_idx, orders, j_hi)
        word = torch.from_numpy(w)
        logp = F.log_softmax(z, dim=1)
        seq.append(word)
        atts.append(a_r)
        lps.append(logp[torch.arange(rows), word])
        scores.append(s)
        los.append(j_lo)
        his.append(j_hi)
        oks.append(w == w_hi)
    info = dict(j_lo=np.stack(los, 1), j_hi=np.stack(his, 1), unambiguous=np.stack(oks, 1))
    return torch.stack(seq, 1), torch.stack(atts, 1), torch.stack(lps, 1), np.stack(scores, 1), info
