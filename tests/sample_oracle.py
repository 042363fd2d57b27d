"""CPU reference of sampled decoding (DecodeEngine(..., sample_n, temperature), csrc/sample.hip): the oracle's decoder step, embedding
and vocabulary head, and Gumbel-max noise computed in fp64 from the same counter-based hash (cvc.synth.dropout_hash restates
csrc/dropout_rng.h::cvc_drop_hash)."""
import numpy as np
import torch
import torch.nn.functional as F

from cvc import synth
from oracle import ref_cpu as O

SAMPLE_SITE = 0x53000000          # include/cvc_hip_blocks.h, CVC_SAMPLE_SITE


def seed_words(seed: int):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def uniform_from_hash(h: np.ndarray) -> np.ndarray:
    """u = ((h >> 9) + 0.5) * 2^-23: exactly representable in fp32, strictly inside (0, 1)"""
    return ((np.asarray(h, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_from_hash(h: np.ndarray) -> np.ndarray:
    return -np.log(-np.log(uniform_from_hash(h)))


def gumbel_noise(seed: int, call: int, t: int, rows: int, V: int, row0: int = 0) -> np.ndarray:
    """[rows, V] fp64 noise of decode step t for rows row0 .. row0 + rows - 1 (element (r, v) at hash counter r * V + v)"""
    lo, hi = seed_words(seed)
    idx = (np.arange(row0 * V, (row0 + rows) * V, dtype=np.uint64) & 0xFFFFFFFF).astype(np.uint32)
    h = synth.dropout_hash(lo, hi, call, SAMPLE_SITE + t, idx)
    return gumbel_from_hash(h).reshape(rows, V)


def select(z: torch.Tensor, noise: np.ndarray, tau: float, unk_idx: int):
    """words, fp64 perturbed scores (UNK at -inf) and the log-prob of each word, for logits z [rows, V]"""
    s = z.double().numpy() / tau + noise
    s[:, unk_idx] = -np.inf
    word = np.argmax(s, axis=1)                                  # first maximum: ties -> lower index
    logp = F.log_softmax(z, dim=1)
    lp = logp[torch.arange(z.shape[0]), torch.from_numpy(word)]
    return word, s, lp


def sample(P, feats, T: int, unk_idx: int, n: int, tau: float, seed: int, call: int, softattn_type: str = "additive",
           temp: float = 1.0):
    """Exactly T steps from BOS, n samples per clip (row b * n + j is sample j of clip b).  Returns seq [B*n, T],
    att2 [B*n, T, N], logprob [B*n, T] and the fp64 perturbed scores [B*n, T, V] (what the tie-aware comparison needs)."""
    rep = lambda x: x.repeat_interleave(n, 0)
    fc, conv, pconv, pool, ppool = (rep(feats[k]) for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats"))
    mask = rep(feats["pnt_mask"][:, 1:])
    rows = fc.shape[0]
    state = O.init_hidden(rows, fc.shape[1])
    word = torch.zeros(rows, dtype=torch.long)
    seq, atts, lps, scores = [], [], [], []
    for t in range(T):
        e = O.embed(P, word)
        out, state, a_r, _, _ = O.decoder_step(P, e, fc, conv, pconv, pool, ppool, mask, state, None,
                                               softattn_type=softattn_type, temp=temp)
        z = F.linear(out, P["logit.weight"], P["logit.bias"])
        w, s, lp = select(z, gumbel_noise(seed, call, t, rows, z.shape[1]), tau, unk_idx)
        word = torch.from_numpy(w)
        seq.append(word)
        atts.append(a_r)
        lps.append(lp)
        scores.append(s)
    return torch.stack(seq, 1), torch.stack(atts, 1), torch.stack(lps, 1), np.stack(scores, 1)


def score_gaps(scores: np.ndarray) -> np.ndarray:
    """[rows, T] margin by which the oracle's word wins: best minus second-best perturbed score (UNK is already -inf)"""
    top = -np.partition(-scores, 1, axis=-1)[..., :2]
    return top[..., 0] - top[..., 1]


def chi_square(counts: np.ndarray, probs: np.ndarray, min_expected: float = 5.0):
    """Pearson's statistic of `counts` against `probs`, categories with an expectation below min_expected pooled into one.
    Returns (statistic, degrees of freedom)."""
    counts = np.asarray(counts, dtype=np.float64)
    exp = np.asarray(probs, dtype=np.float64) * counts.sum()
    big = exp >= min_expected
    c = np.concatenate([counts[big], [counts[~big].sum()]]) if (~big).any() else counts[big]
    e = np.concatenate([exp[big], [exp[~big].sum()]]) if (~big).any() else exp[big]
    keep = e > 0
    return float(((c[keep] - e[keep]) ** 2 / e[keep]).sum()), int(keep.sum()) - 1


def chi_square_critical(df: int, z: float = 3.719) -> float:
    """Upper quantile of chi-square(df) by the Wilson-Hilferty approximation (z = 3.719: p = 1e-4)"""
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + z * np.sqrt(a)) ** 3
