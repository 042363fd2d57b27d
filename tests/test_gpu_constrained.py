"""Constrained decoding on the GPU (pytest -m gpu): the selection block cvc_constrained_select_parts (csrc/constrain.hip) against the
fp64 reference (tests/constrain_ref.py) on every row, the block with nothing banned against the blocks it extends, the engine's
three paths against the reference decoder and against the unconstrained engines, graph replay, bf16-stored weights, and the model
/ trainer / CLI plumbing.

The two lists hold at most 256 ids and a history at most 64 words, so "all but one word banned" and "everything banned" can be
stated at V <= 256 only: those two planted cases run at the V = 50 / 52 shapes."""
import functools

import numpy as np
import pytest
import torch

from cvc import synth
import sample_oracle as S
import sample_trunc_ref as R
import constrain_ref as CR
import test_gpu_sampling as TS               # its inputs, its tie-aware comparison and its tolerances
import test_gpu_sampling_trunc as TT         # the truncating block's launcher, finished()

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def cons_block(parts, bias, V, unk, inv_tau, top_k, top_p, state, t, hist, rules, trunc_out=True):
    """-> word, logprob, cutoff, kept, nbanned of cvc_constrained_select_parts (outputs pre-filled with values no launch writes).
    hist [>= t, M] int64 on the device; rules: the keyword arguments of constrain_ref.banned()."""
    from cvc import hip
    dev = parts.device
    nparts, M = parts.shape[0], parts.shape[1]
    word = torch.full((M,), -7, dtype=torch.int64, device=dev)
    lp = torch.full((M,), float("nan"), device=dev)
    cutoff = torch.full((M,), float("nan"), device=dev) if trunc_out else None
    kept = torch.full((M,), -7, dtype=torch.int32, device=dev) if trunc_out else None
    nb = torch.full((M,), -7, dtype=torch.int32, device=dev)
    i32 = lambda ids: torch.tensor(list(ids) or [0], dtype=torch.int32, device=dev)
    ban, bad = list(rules.get("ban_words", ())), list(rules.get("bad_endings", ()))
    ban_d, bad_d = i32(ban), i32(bad)
    c = hip.Constraint(int(rules.get("no_repeat_ngram", 0)), int(bool(rules.get("no_immediate_repeat", False))),
                       int(rules.get("min_len", 0)), len(ban), ban_d.data_ptr(), bad_d.data_ptr(), len(bad))
    ptr = lambda x: None if x is None else x.data_ptr()
    rc = hip.lib().cvc_constrained_select_parts(parts.data_ptr(), nparts, M * V, ptr(bias), M, V, unk, inv_tau, top_k, top_p, ptr(state), t,
                                                word.data_ptr(), 1, lp.data_ptr(), ptr(cutoff), ptr(kept), hist.data_ptr(), hist.shape[1],
                                                c, nb.data_ptr(), hip._stream())
    hip._check(rc, "cvc_constrained_select_parts")
    torch.cuda.synchronize()
    return word, lp, cutoff, kept, nb


# ------------------------------------------------------------------ 1. the block against the reference, every row
SHAPES = [(1, 50, 1, False), (64, 52, 4, True), (320, 50, 8, True), (64, 4999, 1, False), (64, 5000, 6, True), (33, 8192, 2, True)]
MODES = [("argmax", 0, 1.0), ("sample", 0, 1.0), ("sample", 40, 0.9)]
TAU = 0.7
T_HIST = 64


@functools.lru_cache(maxsize=None)
def base_case(M, V, nparts, with_bias):
    """slabs, bias and their finished logits of one shape, shared by its cases (never modified: the cases clone)"""
    g = torch.Generator().manual_seed(M * 131 + V + nparts + 7)
    parts = torch.randn(nparts, M, V, generator=g) * (1.5 / np.sqrt(nparts))
    bias = torch.randn(V, generator=g) * 0.3 if with_bias else None
    return parts, bias


def winners(z, noise, inv_tau, k, p, count):
    """the `count` words the unconstrained step would choose first, second, ...: [rows, count] (each found with the ones before it
    banned -- what a ban of the winner promotes)"""
    rows, V = z.shape
    ban = np.zeros((rows, V), bool)
    ban[:, UNK] = True
    out = np.zeros((rows, count), np.int64)
    for i in range(count):
        w, _, _, _ = CR.select(z, ban, noise, inv_tau, k, p)
        out[:, i] = w
        ban[np.arange(rows), w] = True
    return out


def check(dev, pd_, bd, z, V, mode, k, p, state, seed_call, t, hist, rules, label):
    """one launch (twice: bitwise equal) against the reference on every row.  -> words, the reference's ban matrix"""
    M = z.shape[0]
    sampling = mode == "sample"
    inv_tau = float(np.float32(1.0 / TAU)) if sampling else 0.0
    noise = S.gumbel_noise(seed_call[0], seed_call[1], t, M, V) if sampling else None
    trunc = sampling and (k > 0 or p < 1.0)
    ban = CR.banned(hist.T, t, V, UNK, **rules)
    w_ref, s, lp_ref, info = CR.select(z, ban, noise, inv_tau, k, p)
    hist_d = torch.from_numpy(np.ascontiguousarray(hist)).to(dev)
    out = cons_block(pd_, bd, V, UNK, inv_tau, k if sampling else 0, p if sampling else 1.0, state if sampling else None, t, hist_d, rules)
    again = cons_block(pd_, bd, V, UNK, inv_tau, k if sampling else 0, p if sampling else 1.0, state if sampling else None, t, hist_d, rules)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out, again)), label
    if not trunc:                                               # without cutoff / kept outputs: the kernel form without the search
        lean = cons_block(pd_, bd, V, UNK, inv_tau, 0, 1.0, state if sampling else None, t, hist_d, rules, trunc_out=False)
        assert all(torch.equal(bits(out[i]), bits(lean[i])) for i in (0, 1, 4)), label
    w, lp, cut, kept, nb = (x.cpu().numpy() for x in out)
    assert np.array_equal(nb, ban.sum(1)), (label, nb[:8], ban.sum(1)[:8])
    zd = z.double().numpy()
    sfull = zd if noise is None else zd * inv_tau + noise
    finite = s[np.isfinite(s)]
    TOL = 0.0 if not sampling else 1e-5 * (1.0 + (np.abs(finite).max() if finite.size else 0.0))    # arg-max mode: the same fp32 logits
    n_clear = 0
    for r in range(M):
        allowed = np.flatnonzero(~ban[r])
        if len(allowed) == 0:
            assert w[r] == 0 and np.isneginf(lp[r]) and kept[r] == 0 and cut[r] == np.inf, (label, r, w[r], lp[r], kept[r], cut[r])
            n_clear += 1
            continue
        c2 = allowed
        if trunc:
            assert info["j_lo"][r] <= kept[r] <= info["j_hi"][r], (label, r, kept[r], info["j_lo"][r], info["j_hi"][r])
        c2 = allowed[z[r, torch.from_numpy(allowed)].numpy() >= cut[r]]                  # the kept set the kernel reports
        assert len(c2) == kept[r] and cut[r] == z[r, torch.from_numpy(c2)].numpy().min(), (label, r, kept[r], len(c2), cut[r])
        if not trunc:
            assert kept[r] == len(allowed), (label, r)
        assert w[r] in c2, (label, r, w[r])
        sc = sfull[r, c2]
        assert sc.max() - sfull[r, w[r]] <= TOL, (label, r, sc.max() - sfull[r, w[r]])
        top2 = np.sort(sc)[-2:]
        if len(c2) == 1 or top2[1] - top2[0] > TOL:                                       # a clear margin: the arg-max itself
            assert w[r] == c2[np.argmax(sc)], (label, r)
            n_clear += 1
        elif not sampling:
            assert w[r] == c2[np.argmax(sc)], (label, r)                                  # exact ties: the lower index
        if info["unambiguous"][r] and info["j_lo"][r] == info["j_hi"][r] and (len(c2) == 1 or top2[1] - top2[0] > TOL):
            assert w[r] == w_ref[r], (label, r, w[r], w_ref[r])
    assert n_clear >= M - (M + 2) // 3, (label, n_clear)
    ok = ~info["empty"]
    lse = zd.max(1) + np.log(np.exp(zd - zd.max(1, keepdims=True)).sum(1))
    np.testing.assert_allclose(lp[ok].astype(np.float64), (zd[np.arange(M), w] - lse)[ok], rtol=0, atol=2e-6, err_msg=label)
    return w, ban


@pytest.mark.parametrize("mode,k,p", MODES)
@pytest.mark.parametrize("M,V,nparts,with_bias", SHAPES)
def test_block_vs_reference_on_every_row(dev, M, V, nparts, with_bias, mode, k, p):
    parts, bias = base_case(M, V, nparts, with_bias)
    parts = parts.clone()
    parts[0, 1::2, 0] += 12.0                                   # odd rows want to stop: word 0 leads (min_len / bad_endings act on it)
    z = TT.finished(parts, bias)
    pd_, bd = parts.contiguous().to(dev), None if bias is None else bias.to(dev)
    seed, call = 999 + M + V, 2
    state = TS.state_words(seed, call).to(dev)
    sampling = mode == "sample"
    inv_tau = float(np.float32(1.0 / TAU)) if sampling else 0.0
    rng = np.random.RandomState(M + V + nparts)
    rows = np.arange(M)
    run = lambda t, hist, rules, what: check(dev, pd_, bd, z, V, mode, k, p, state, (seed, call), t, hist, rules,
                                             f"M={M} V={V} nparts={nparts} {mode} k={k} p={p} t={t} {what}")

    def win(t, count=3):
        noise = S.gumbel_noise(seed, call, t, M, V) if sampling else None
        return winners(z, noise, inv_tau, k, p, count)

    def background(t):
        """a history over a small alphabet (so that n-grams recur by themselves too), rows of steps t .. 63 never read: out of range"""
        h = rng.choice(np.array([2, 31, 32, V - 1, 5]), size=(T_HIST, M))
        h[t:] = V + 99
        return h

    # --- the t sweep of no_repeat_ngram = 3: t = 0, 1, n-2, n-1, n, 63; even rows: the trigram (a, b, winner) is in the history and
    # the history ends on (a, b); at t = 63 three matches ban the winner (twice) and the runner-up
    n = 3
    for t in (0, 1, n - 2, n - 1, n, 63):
        w0 = win(t)
        h = background(t)
        if t == n:                                               # three words of history: only (c, c, c) holds its last two twice
            h[0, ::2] = h[1, ::2] = h[2, ::2] = w0[::2, 0]
        elif t == 63:
            a, b = 7, 9
            h[t - 2, ::2], h[t - 1, ::2] = a, b
            h[0, ::2], h[1, ::2], h[2, ::2] = a, b, w0[::2, 0]
            h[10, ::2], h[11, ::2], h[12, ::2] = a, b, w0[::2, 1]
            h[20, ::2], h[21, ::2], h[22, ::2] = a, b, w0[::2, 0]
        w, ban = run(t, h, dict(no_repeat_ngram=n), "ngram3")
        if t >= n:
            assert ban[rows[::2], w0[::2, 0]].all() and not (w[::2] == w0[::2, 0]).any()              # the would-be winner is banned
            assert (ban.sum(1)[::2] >= (3 if t == 63 else 2)).all()
        else:
            assert (ban.sum(1) == 1).all() and np.array_equal(w, w0[:, 0])                           # nothing but UNK while t < n
    # --- n = 1 at t = 63: every earlier word; n = 2 with the immediate rule
    t = 63
    w0 = win(t)
    h = background(t)
    h[40, ::2] = w0[::2, 0]
    w, ban = run(t, h, dict(no_repeat_ngram=1), "ngram1")
    assert ban[rows[::2], w0[::2, 0]].all() and (ban.sum(1) <= 7).all()
    t = 6
    w0 = win(t)
    h = background(t)
    h[t - 1] = w0[:, 0]                                          # the previous word is the winner: immediate repeat
    h[2, ::2], h[3, ::2] = w0[::2, 0], w0[::2, 1]                # (winner, runner-up) seen: the bigram rule bans the runner-up too
    w, ban = run(t, h, dict(no_repeat_ngram=2, no_immediate_repeat=True), "ngram2+immediate")
    assert ban[rows, w0[:, 0]].all() and ban[rows[::2], w0[::2, 1]].all()
    # --- the list: ids at 0, 31, 32, V - 1, UNK, a duplicate, ids outside [0, V), the winner
    t = 4
    w0 = win(t)
    lst = [0, 31, 32, V - 1, UNK, 31, V, V + 5, -3, 1 << 20, int(w0[0, 0])]
    w, ban = run(t, background(t), dict(ban_words=lst), "list")
    assert (ban.sum(1) == len({0, 31, 32, V - 1, UNK, int(w0[0, 0])})).all() and w[0] != w0[0, 0]
    # --- min_len on both sides of t (odd rows want word 0)
    for L in (t, t + 1):
        w0 = win(t)
        assert M == 1 or (w0[1::2, 0] == 0).mean() >= 0.5
        w, ban = run(t, background(t), dict(min_len=L), f"min_len={L}")
        assert ban[:, 0].all() == (t < L) and ((w == 0).any() == (t >= L) or M == 1)
    # --- a bad ending at y_{t-1} (rows 1, 5, 9, ...: word 0 is banned) and at y_{t-2} only (rows 3, 7, ...: it is not)
    h = background(t)
    h[t - 1, 1::4], h[t - 2, 1::4] = 11, 5
    h[t - 1, 3::4], h[t - 2, 3::4] = 5, 11
    w, ban = run(t, h, dict(bad_endings=[11, 13, V + 1]), "bad_endings")
    assert ban[1::4, 0].all() and not ban[3::4, 0].any() and not ban[0::2, 0].any()
    assert not (w[1::4] == 0).any() and np.array_equal(w[3::4] == 0, w0[3::4, 0] == 0)
    # --- all but one word banned; everything banned (V <= 256: the list holds at most 256 ids)
    if V <= 256:
        keep = 17
        w, ban = run(t, background(t), dict(ban_words=[v for v in range(V) if v != keep]), "all-but-one")
        assert (w == keep).all() and (ban.sum(1) == V - 1).all()
        w, ban = run(t, background(t), dict(ban_words=list(range(V))), "everything")
        assert (w == 0).all() and (ban.sum(1) == V).all()


def test_truncation_with_the_arg_max_mode_is_refused(dev):
    from cvc import hip
    z = torch.zeros(1, 4, 50, device=dev)
    hist = torch.zeros(4, 4, dtype=torch.int64, device=dev)
    for k, p in ((5, 1.0), (0, 0.9)):
        with pytest.raises(RuntimeError):
            cons_block(z, None, 50, UNK, 0.0, k, p, None, 2, hist, {})


# ------------------------------------------------------------------ 2. nothing banned
@pytest.mark.parametrize("M,V,nparts,with_bias", [(64, 52, 4, True), (64, 4999, 1, False), (64, 5000, 6, True), (33, 8192, 2, True)])
def test_with_nothing_banned_the_block_is_the_blocks_it_extends(dev, M, V, nparts, with_bias):
    from cvc import hip
    parts, bias = base_case(M, V, nparts, with_bias)
    pd_, bd = parts.contiguous().to(dev), None if bias is None else bias.to(dev)
    seed, call, t = 5, 3, 5
    state = TS.state_words(seed, call).to(dev)
    inv_tau = float(np.float32(1.0 / TAU))
    hist = torch.randint(0, V, (T_HIST, M), dtype=torch.int64, device=dev)
    hist[t - 1] = hist[t - 2]                                    # a repeat is there; n = 64 cannot see it at t = 5
    rules = dict(no_repeat_ngram=64)
    w0, lp0 = TS.select_block(pd_, bd, V, UNK, inv_tau, state, t)
    w, lp, cut, kept, nb = cons_block(pd_, bd, V, UNK, inv_tau, 0, 1.0, state, t, hist, rules, trunc_out=False)
    assert torch.equal(w, w0) and torch.equal(bits(lp), bits(lp0)) and (nb == 1).all()
    for k, p in ((40, 0.9), (0, 0.5), (7, 1.0), (0, 1.0)):
        a = TT.trunc_block(pd_, bd, V, UNK, inv_tau, k, p, state, t)
        b = cons_block(pd_, bd, V, UNK, inv_tau, k, p, state, t, hist, rules)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b[:4])), (k, p)
    # arg-max mode: the word of cvc_top2_unk on the same (finished) logits
    zf = TT.finished(parts, bias).contiguous().to(dev)
    wg = torch.full((M,), -7, dtype=torch.int64, device=dev)
    lg = torch.full((M,), float("nan"), device=dev)
    hip._check(hip.lib().cvc_top2_unk(zf.data_ptr(), M, V, UNK, wg.data_ptr(), 1, lg.data_ptr(), hip._stream()), "cvc_top2_unk")
    wa, lpa, _, _, _ = cons_block(pd_, bd, V, UNK, 0.0, 0, 1.0, None, t, hist, rules, trunc_out=False)
    assert torch.equal(wa, wg)
    np.testing.assert_allclose(lpa.cpu().numpy(), lg.cpu().numpy(), rtol=0, atol=2e-6)


# ------------------------------------------------------------------ 3. the engine
def _properties(seq, rules, T):
    n, L = rules.get("no_repeat_ngram", 0), rules.get("min_len", 0)
    ban, bad = list(rules.get("ban_words", ())), list(rules.get("bad_endings", ()))
    assert not np.isin(seq, ban + [UNK]).any()
    if n:
        assert not CR.repeats_ngram(seq, n).any()
    if rules.get("no_immediate_repeat"):
        assert not (seq[:, 1:] == seq[:, :-1]).any()
    assert not (seq[:, :min(L, T)] == 0).any()
    if bad:
        assert not (seq[:, 1:][np.isin(seq[:, :-1], bad)] == 0).any()


ARGMAX_CASES = [(name, path, n) for name, path in (("tiny", "ring"), ("tiny", "tile"), ("cfg1", "packed")) for n in (1, 2, 3)]


@pytest.mark.parametrize("name,path,n", ARGMAX_CASES)
def test_engine_arg_max_mode_vs_reference_decoder(dev, name, path, n):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs(name)
    rules = dict(no_repeat_ngram=n)
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, path="tile" if path == "tile" else "auto", **rules)
    assert (eng.packed, eng.tile) == (path == "packed", path == "tile") and eng._plan is None and eng.constrained and not eng.sampling
    assert eng.nbanned.shape == (d.T, d.B) and eng.nbanned.dtype == torch.int32
    seq, att, lp = eng.run()
    with torch.no_grad():
        ref = CR.decode(P, f, d.T, UNK, **rules)
    info = ref[4]
    assert info["fired"].any(1).mean() >= 0.5                    # the rule decides: a would-be winner is banned in these rows
    _properties(seq.cpu().numpy(), rules, d.T)
    TS._compare(seq, att, lp, ref[:4], f"constrained arg-max {name} {path} n={n}")
    same = np.cumprod(seq.cpu().numpy() == ref[0].numpy(), axis=1).astype(bool)
    ok_t = np.concatenate([np.ones((d.B, 1), bool), same[:, :-1]], 1)
    assert np.array_equal(eng.nbanned.t().cpu().numpy()[ok_t], info["nbanned"][ok_t])


# seeds picked on the CPU with the reference: at each, both calls ban a would-be winner in at least half of the rows and the
# reference's smallest deciding margin is above 10 x SCORE_TIE_TOL
@pytest.mark.parametrize("name,n,path,seed,trunc", [("tiny", 1, "ring", 2, False), ("tiny", 3, "tile", 3, False),
                                                   ("cfg1", 1, "packed", 4, False), ("cfg1", 1, "packed", 4, True)])
def test_engine_sampled_vs_reference_decoder(dev, name, n, path, seed, trunc):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs(name)
    tau = 0.05
    rules = dict(no_repeat_ngram=2, no_immediate_repeat=True)
    tk = dict(top_k=10, top_p=0.9) if trunc else {}
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, sample_n=n, temperature=tau, seed=seed, **tk, **rules)
    assert (eng.packed, eng.tile) == (path == "packed", path == "tile") and eng._plan is None and eng.constrained and eng.sampling
    for call in (1, 2):
        seq, att, lp = eng.run()
        assert seq.shape == (d.B * n, d.T) and int(eng.rng[2]) == call
        with torch.no_grad():
            if trunc:
                ref = CR.decode(P, f, d.T, UNK, n, tau, seed, call, tol=TT.engine_mass_tol(tau), ztol=TT.ENGINE_ZTOL, **tk, **rules)
            else:
                ref = CR.decode(P, f, d.T, UNK, n, tau, seed, call, **rules)
        info = ref[4]
        assert info["fired"].any(1).mean() >= 0.5, (call, info["fired"].any(1))
        _properties(seq.cpu().numpy(), rules, d.T)
        scores = ref[3]
        if trunc:                                               # a cutoff band whose ends pick different words: not comparable
            scores = scores.copy()
            amb = ~info["unambiguous"]
            scores[amb] = np.where(np.isfinite(scores[amb]), 0.0, scores[amb])
        TS._compare(seq, att, lp, (ref[0], ref[1], ref[2], scores), f"constrained sampled {name} n={n} {path} call {call} trunc={trunc}")
        if trunc:
            assert int(eng.kept.max()) <= 11 and int(eng.kept.min()) >= 1


@pytest.mark.parametrize("name,path", [("tiny", "ring"), ("tiny", "tile"), ("cfg1", "packed")])
def test_constraints_that_never_fire_change_nothing(dev, name, path):
    from helpers import to_dev
    from cvc import hip
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs(name)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    kw = dict(path="tile" if path == "tile" else "auto")
    never = dict(no_repeat_ngram=64)                             # T <= 10: no earlier window
    grab = lambda e: [x.clone() for x in e.run()]
    # sampling: the unconstrained sampling engine's words and log-probs, bit for bit
    a = grab(DecodeEngine(W, fd, d.T, UNK, temperature=0.9, seed=7, **kw))
    eb = DecodeEngine(W, fd, d.T, UNK, temperature=0.9, seed=7, **never, **kw)
    b = grab(eb)
    assert eb.constrained and (eb.nbanned == 1).all()
    assert torch.equal(a[0], b[0]) and torch.equal(bits(a[2]), bits(b[2])) and torch.equal(bits(a[1]), bits(b[1]))
    sel = [fn for nm, fn, _ in eb._python_launches() if nm == "word_select"]
    assert len(sel) == d.T and all(fn is hip.lib().cvc_constrained_select_parts for fn in sel)
    # arg-max mode: the greedy engine's words (its driver, its launch list: untouched), log-probs within the stated tolerance
    g = DecodeEngine(W, fd, d.T, UNK, **kw)
    assert not g.constrained and not g.given and (g._plan is not None) == (path != "ring")
    gs = [x.clone() for x in g.run()]
    glp = g.logprob.t().clone()
    c = grab(DecodeEngine(W, fd, d.T, UNK, **never, **kw))
    assert torch.equal(gs[0], c[0])
    np.testing.assert_allclose(c[2].cpu().numpy(), glp.cpu().numpy(), rtol=0, atol=TS.LOGPROB_TOL)
    np.testing.assert_allclose(c[1].cpu().numpy(), gs[1].cpu().numpy(), **TS.SEQ_TOL)


@pytest.mark.parametrize("name,n,tau", [("tiny", 3, 0.05), ("cfg1", 1, None), ("tiny", 1, None)])
def test_eager_equals_a_captured_graph_across_two_batches(dev, name, n, tau):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, _, _ = TS._inputs(name)
    f2 = to_dev(synth.clip_features(d, 777), dev)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    ban, bad = ([20], [23]) if name == "tiny" else ([3560], [2904])       # words their greedy decodes like
    kw = dict(no_repeat_ngram=2, min_len=2, ban_words=ban, bad_endings=bad, own_features=True)
    if tau is not None:
        kw.update(sample_n=n, temperature=tau, seed=11)
    e, g = DecodeEngine(W, fd, d.T, UNK, **kw), DecodeEngine(W, fd, d.T, UNK, **kw).capture()
    assert g.graph is not None and (tau is None or int(g.rng[2]) == 0)
    grab = lambda x: [bits(y.clone()) for y in x.run()] + [x.nbanned.clone()]
    first = None
    for feats in (fd, f2, fd):
        e.load_features(feats)
        g.load_features(feats)
        re_, rg = grab(e), grab(g)
        assert all(torch.equal(a, b) for a, b in zip(re_, rg))
        _properties(rg[0].cpu().numpy(), kw, d.T)
        if first is None:
            first = rg
    assert tau is None or (int(g.rng[2]) == 3 and int(e.rng[2]) == 3)   # (sampling: every replay advanced the generator)
    g.load_features(f2)
    assert not torch.equal(first[1], grab(g)[1])                    # another batch: other attention maps


def test_bf16_weights_with_constraints_match_the_fp32_engine_on_the_rounded_checkpoint(dev):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights, BF16_ROUNDED_KEYS, bf16_round
    d, sd, f_np, _, _ = TS._inputs("cfg1")
    sd_r = dict(sd)
    for key in BF16_ROUNDED_KEYS:
        sd_r[key] = bf16_round(torch.from_numpy(np.ascontiguousarray(sd[key]))).numpy()
    fd = to_dev(f_np, dev)
    for kw in (dict(no_repeat_ngram=2), dict(no_repeat_ngram=2, no_immediate_repeat=True, temperature=0.05, seed=4, top_p=0.9)):
        a = DecodeEngine(DecodeWeights(to_dev(sd, dev)), fd, d.T, UNK, weights_dtype="bf16", **kw)
        b = DecodeEngine(DecodeWeights(to_dev(sd_r, dev)), fd, d.T, UNK, **kw)
        assert a.bf16w and a.packed and a.constrained and b.packed and not b.bf16w
        ra, rb = [x.clone() for x in a.run()], [x.clone() for x in b.run()]
        assert torch.equal(ra[0], rb[0]) and torch.equal(bits(ra[2]), bits(rb[2])) and torch.equal(a.nbanned, b.nbanned)
        _properties(ra[0].cpu().numpy(), kw, d.T)
        assert int(a.nbanned.max()) >= 2                         # the rule had something to ban


# ------------------------------------------------------------------ 4. model, trainer, CLI
def test_model_sample_rebinds_when_a_constraint_changes(dev):
    from helpers import build_model, to_dev, model_call
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=True)
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, 99), dev)
    assert (model.no_repeat_ngram, model.no_immediate_repeat, model.min_caption_len, model.ban_words, model.bad_endings) == (0, False, 0, (), ())
    seq0, att0, none = model_call(model, f, b, True)
    e0 = model._engine_cache[1]
    assert none is None and not e0.constrained
    s1 = TS._model_sample(model, f, b, no_repeat_ngram=1)
    e1 = model._engine_cache[1]
    assert e1 is not e0 and e1.constrained and e1.cons[0] == 1 and e1.graph is not None
    assert s1[2] is not None and s1[2].shape == (d.B, d.T) and not CR.repeats_ngram(s1[0].cpu().numpy(), 1).any()
    assert CR.repeats_ngram(seq0.cpu().numpy(), 1).any()         # the unconstrained decode of this model repeats
    TS._model_sample(model, f, b, no_repeat_ngram=1)
    assert model._engine_cache[1] is e1                          # same rules: the cached engine
    s2 = TS._model_sample(model, f, b, no_repeat_ngram=1, ban_words=[int(s1[0][0, 0])])
    e2 = model._engine_cache[1]
    assert e2 is not e1 and e2.cons[3] == (int(s1[0][0, 0]),) and not (s2[0] == int(s1[0][0, 0])).any()
    model.no_repeat_ngram = 1                                    # the model's attributes are the defaults
    s3 = model_call(model, f, b, True)
    assert model._engine_cache[1].cons[0] == 1 and torch.equal(s3[0], s1[0]) and torch.equal(bits(s3[2]), bits(s1[2]))
    model.no_repeat_ngram = 0
    seq4, att4, none4 = model_call(model, f, b, True)           # and off is the greedy decode it was
    assert none4 is None and torch.equal(seq4, seq0) and torch.equal(bits(att4), bits(att0))


def test_cli_flags_reach_the_engine(dev, tmp_path):
    import json
    from cvc import main as cvc_main
    from cvc import sample as cvc_sample
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16",
              "--seq_length", "4", "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100",
              "--exp_name", "s", "--learning_rate", "0.001", "--results_dir", str(tmp_path / "results"),
              "--checkpoint_path", str(tmp_path) + "/", "--id", "s1"]
    flags = ["--no_repeat_ngram", "2", "--no_immediate_repeat", "--min_caption_len", "3", "--ban_words", "5,UNK,7", "--bad_endings", "9"]
    assert cvc_main.main(common + flags) == 0                  # one epoch, then the evaluation decodes under the rules
    tr = cvc_main.LAST_TRAINER
    e = getattr(tr.model, "module", tr.model)._engine_cache[1]
    assert e.constrained and e.cons == (2, True, 3, (UNK, 5, 7), (9,))
    seq = e.words[1:].t().cpu().numpy()
    _properties(seq, dict(no_repeat_ngram=2, no_immediate_repeat=True, min_len=3, ban_words=[5, 7], bad_endings=[9]), 4)
    assert cvc_sample.main(common + flags + ["--resume", "True", "--temperature", "0.8", "--sample_n", "2", "--sample_seed", "4"]) == 0
    e = getattr(cvc_main.LAST_TRAINER.model, "module", cvc_main.LAST_TRAINER.model)._engine_cache[1]
    assert e.constrained and e.sampling and e.nq == 2 and e.cons == (2, True, 3, (UNK, 5, 7), (9,))
    out = json.load(open(cvc_main.LAST_TRAINER.sample(2, 0.8, seed=4, constraints=dict(min_len=4))))
    assert len(out) == 8 and getattr(cvc_main.LAST_TRAINER.model, "module", cvc_main.LAST_TRAINER.model)._engine_cache[1].cons[2] == 4
    with pytest.raises(SystemExit, match="zebra"):
        cvc_main.main(common + ["--ban_words", "zebra"])
