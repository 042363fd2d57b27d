"""fp64 host restatement of cvc_scst_weights_wor (csrc/scst_wor.hip; the rule: include/cvc_hip_blocks.h; DESIGN section 7,
"Self-critical training without replacement"): importance weights, per-row baselines and per-token weights of a clip's S rollouts
drawn without replacement by stochastic beam search with beam = S + 1 (Kool, van Hoof and Welling 2019).  Builds on
tests/sbs_ref.py (the toy) and tests/sample_oracle.py (the seed words) without changing them.

Per clip b: reward f [S], logq / G [S + 1] (slot S: the threshold), a = -log u of the counter hash at site WOR_SITE, counter b.
  lambda = -G_S + log1p((a - 1) exp(G_S)), +inf when slot S is dead; corrected=False: lambda = -G_S, the threshold as the engine
  leaves it (conditioned on a root key of 0) -- the wrong rule the statistics must reject.
  d = logq + lambda, x = exp(d), log q_i = log(-expm1(-x)) (x < 1: d + log(-expm1(-x) / x), ratio 1 at x = 0; 0 at x = inf)
  l_i = logq_i - log q_i (live), -inf (dead);  W, W_i, B_i, wgt, adv, est as the header defines them."""
import numpy as np

from cvc import synth
import sample_oracle as SO

WOR_SITE = 0x57000000             # include/cvc_hip_blocks.h, CVC_WOR_SITE
MAX_S = 7


def root_hash(seed_lo: int, seed_hi: int, call: int, clips: int) -> np.ndarray:
    """h [clips] uint32: the counter hash of clip b at site WOR_SITE"""
    return synth.dropout_hash(seed_lo, seed_hi, call, WOR_SITE, np.arange(clips, dtype=np.uint32))


def root_exponential(h: np.ndarray, dt=np.float64) -> np.ndarray:
    """a = -log u, u = ((h >> 9) + 0.5) * 2^-23 (exact in fp32, strictly inside (0, 1)); dt = np.float32: the kernel's own arithmetic"""
    u = ((h >> np.uint32(9)).astype(dt) + dt(0.5)) * dt(2.0 ** -23)
    return -np.log(u)


def root_from_seed(seed: int, call: int, clips: int) -> np.ndarray:
    lo, hi = SO.seed_words(seed)
    return root_exponential(root_hash(lo, hi, call, clips))


def threshold(kt, a, corrected: bool = True) -> np.ndarray:
    """lambda [clips] = -kappa; +inf where slot S is not live"""
    kt, a = np.asarray(kt, np.float64), np.asarray(a, np.float64)
    ok = np.isfinite(kt)
    k = np.where(ok, kt, 0.0)
    lam = -k + (np.log1p((a - 1.0) * np.exp(k)) if corrected else 0.0)
    return np.where(ok, lam, np.inf)


def log_inclusion(d) -> np.ndarray:
    """log(1 - exp(-exp(d))), by the rule's three branches"""
    d = np.asarray(d, np.float64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        x = np.exp(d)
        small = x < 1.0
        xs = np.where(small & (x > 0), x, 1.0)
        ratio = np.where(small & (x > 0), -np.expm1(-xs) / xs, 1.0)
        big = np.log(-np.expm1(-np.where(small | np.isinf(x), 1.0, x)))
        out = np.where(small, d + np.log(ratio), big)
    return np.where(np.isinf(x), 0.0, out)


def _shifted(L, F):
    """sum_j exp(L_j) and sum_j exp(L_j) F_j over the finite L_j of every row, shifted by the row's largest exponent:
    (m, sum exp(L - m), sum exp(L - m) F); a row without a finite L: (-inf, 0, 0)"""
    m = L.max(1)
    ms = np.where(np.isfinite(m), m, 0.0)
    e = np.where(np.isfinite(L), np.exp(L - ms[:, None]), 0.0)
    return m, e.sum(1), (e * F).sum(1)


def weights(reward, logq, G, a, normalize: bool = True, corrected: bool = True) -> dict:
    """reward [B, S] (or [B * S]), logq / G [B, S + 1], a [B] -> dict of fp64 arrays:
    adv, wgt [B, S]; est [B]; n_live [B]; lam [B]; l [B, S]; adv_scale [B, S], est_scale [B]: the magnitudes of the terms the
    outputs are sums of (what a relative error is relative to: adv is a difference that may cancel)."""
    logq, G = np.asarray(logq, np.float64), np.asarray(G, np.float64)
    B, S1 = G.shape
    S = S1 - 1
    f = np.asarray(reward, np.float64).reshape(B, S)
    live = np.isfinite(G[:, :S])
    phi = logq[:, :S]
    lam = threshold(G[:, S], a, corrected)
    with np.errstate(invalid="ignore"):
        l = np.where(live, phi - log_inclusion(np.where(live, phi, 0.0) + lam[:, None]), -np.inf)
    fz = np.where(live, f, 0.0)
    n_live = live.sum(1)
    m, W, E = _shifted(l, fz)
    _, _, Eabs = _shifted(l, np.abs(fz))
    adv, wgt, adv_scale = np.zeros((B, S)), np.zeros((B, S)), np.zeros((B, S))
    some = n_live > 0
    Ws = np.where(some, W, 1.0)
    ms = np.where(some, m, 0.0)
    if normalize:
        est, est_scale = np.where(some, E / Ws, 0.0), np.where(some, Eabs / Ws, 0.0)
    else:
        est, est_scale = np.where(some, np.exp(ms) * E, 0.0), np.where(some, np.exp(ms) * Eabs, 0.0)
    for i in range(S):
        Li = l.copy()
        Li[:, i] = np.where(live[:, i], phi[:, i], -np.inf)        # row i enters its own sums with p_i instead of w_i
        mi, Wi, Bi = _shifted(Li, fz)
        _, _, Bia = _shifted(Li, np.abs(fz))
        on = live[:, i]
        Wi_s, mi_s = np.where(on, Wi, 1.0), np.where(on, mi, 0.0)
        li = np.where(on, l[:, i], 0.0)
        if normalize:
            w_i = np.exp(li - ms) / Ws
            a_i = n_live * w_i * (f[:, i] - Bi / Wi_s)
            s_i = n_live * w_i * (np.abs(f[:, i]) + Bia / Wi_s)
        else:
            w_i = np.exp(li)
            a_i = w_i * (f[:, i] - np.exp(mi_s) * Bi)
            s_i = w_i * (np.abs(f[:, i]) + np.exp(mi_s) * Bia)
        wgt[:, i], adv[:, i], adv_scale[:, i] = np.where(on, w_i, 0.0), np.where(on, a_i, 0.0), np.where(on, s_i, 0.0)
    return dict(adv=adv, wgt=wgt, est=est, n_live=n_live, lam=lam, l=l, adv_scale=adv_scale, est_scale=est_scale)


def text_mask(cand: np.ndarray) -> np.ndarray:
    """[rows, T] bool: the steps up to and including the first 0 (all T without one)"""
    zero = np.asarray(cand) == 0
    return (np.cumsum(zero, 1) - zero) == 0


def token_weights(adv, cand, t_major: bool = False) -> np.ndarray:
    """w [rows, T] (t_major: [T, rows]) = adv on the mask, 0 off it, in adv's dtype"""
    adv = np.asarray(adv).reshape(-1)
    w = np.where(text_mask(cand), adv[:, None], adv.dtype.type(0))
    return np.ascontiguousarray(w.T) if t_major else w


def leave_one_out(reward) -> np.ndarray:
    """cvc_scst_weights' advantage: f_i minus the mean of the clip's others; reward [B, S]"""
    f = np.asarray(reward, np.float64)
    S = f.shape[1]
    return f - (f.sum(1, keepdims=True) - f) / (S - 1)


# ------------------------------------------------------------------ the toy: statistics of the estimator
def toy_statistics(hist, logq, G, a, seqs, f, h, corrected: bool = True, weights_fn=None):
    """hist [trials, S + 1, T], logq / G [trials, S + 1] of sbs_ref.toy_run with beam = S + 1; seqs: sbs_ref.toy_sequences' captions; f, h
    [len(seqs)] the caption's reward and its stand-in for grad log p.  -> per trial (sum_i wgt_i f_i, sum_i adv_i h_i) of the
    UNNORMALISED form.  weights_fn(reward, logq, G): another producer of (adv, wgt, est) [trials, S] (the device block)."""
    index = {s: i for i, s in enumerate(seqs)}
    trials, S1, _ = hist.shape
    S = S1 - 1
    idx = np.array([[index.get(tuple(int(w) for w in hist[n, i]), 0) for i in range(S)] for n in range(trials)])
    fr, hr = np.asarray(f)[idx], np.asarray(h)[idx]
    if weights_fn is None:
        r = weights(fr, logq, G, a, normalize=False, corrected=corrected)
        adv, est = r["adv"], r["est"]
    else:
        adv, _wgt, est = weights_fn(fr, logq, G)
    return est, (adv * hr).sum(1)


TOY_TABLE_SEED, TOY_SEED, TOY_CALL, TOY_TRIALS = 4, 12, 1, 50000
# (tau, unk) of the two statistical cases.  The table of seed 4 is flat enough (largest caption probability 0.28 / 0.55) for the
# root-key correction to matter: on a peaked table (one caption at 0.9) the threshold is far below every phi, every inclusion
# probability is 1 whatever the threshold, and the uncorrected rule cannot be told from the right one.
TOY_CASES = {"tau1": (1.0, -1), "tau0.7_unk": (0.7, 1)}
_toy_cache = {}


def toy_case(name: str, V: int = 4, T: int = 3, beam: int = 4, trials: int = TOY_TRIALS) -> dict:
    """the toy of the statistical checks, computed once per process: sbs_ref.toy_run with beam = S + 1, every caption's
    probability, a fixed reward f in [0, 10) and a fixed positive h per caption, the per-clip a, and the exact values"""
    import sbs_ref
    key = (name, V, T, beam, trials)
    if key not in _toy_cache:
        tau, unk = TOY_CASES[name]
        table = sbs_ref.toy_table(V, T, TOY_TABLE_SEED)
        hist, live, G, logq, _score = sbs_ref.toy_run(table, trials, beam, tau, TOY_SEED, call=TOY_CALL, unk=unk)
        seqs, probs = sbs_ref.toy_sequences(table, tau, unk)
        rng = np.random.default_rng(TOY_TABLE_SEED + 100)
        f, h = rng.random(len(seqs)) * 10, rng.random(len(seqs)) + 0.5
        Ef, cov = exact_values(probs, f, h)
        _toy_cache[key] = dict(hist=hist, live=live, G=G, logq=logq, seqs=seqs, probs=probs, f=f, h=h, Ef=Ef, cov=cov,
                               a=root_from_seed(TOY_SEED, TOY_CALL, trials), seed=TOY_SEED, call=TOY_CALL)
    return _toy_cache[key]


def exact_values(probs, f, h):
    """(E f, sum p f h - (sum p f)(sum p h)): what the two statistics estimate"""
    p, f, h = (np.asarray(x, np.float64) for x in (probs, f, h))
    return float((p * f).sum()), float((p * f * h).sum() - (p * f).sum() * (p * h).sum())


def z_score(x, want) -> float:
    """(mean - want) in standard errors of the mean"""
    x = np.asarray(x, np.float64)
    return float((x.mean() - want) / (x.std(ddof=1) / np.sqrt(len(x))))
