"""Top-k / nucleus (top-p) truncated sampling on the GPU (pytest -m gpu): the truncating selection block
(cvc_sample_select_trunc_parts, csrc/sample.hip) against the fp64 reference (tests/sample_trunc_ref.py) on every row, truncation
switched off, the engine's three paths against the reference sampler, graph replay and seeding, the sampled distribution, and the
model / trainer / CLI plumbing.  The block test prints per case how many rows have a one-point band and where `kept` fell."""
import functools

import numpy as np
import pytest
import torch

from cvc import synth
import sample_oracle as S
import sample_trunc_ref as R
import test_gpu_sampling as TS               # its inputs, its tie-aware comparison and its tolerances

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
# An engine's logits against the CPU oracle's: the stated fp32 tolerance of a log-prob after T recurrent steps (TS.LOGPROB_TOL).
# A logit off by d moves its e = exp(z / tau) by d / tau relative, a ratio of two masses by at most 2 d / tau.
ENGINE_ZTOL = TS.LOGPROB_TOL
engine_mass_tol = lambda tau: R.MASS_TOL + 2.0 * ENGINE_ZTOL / tau


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def trunc_block(parts, bias, V, unk, inv_tau, top_k, top_p, state, t):
    """-> word, logprob, cutoff, kept of cvc_sample_select_trunc_parts (outputs pre-filled with values no launch writes)"""
    from cvc import hip
    nparts, M = parts.shape[0], parts.shape[1]
    word = torch.full((M,), -7, dtype=torch.int64, device=parts.device)
    lp = torch.full((M,), float("nan"), device=parts.device)
    cutoff = torch.full((M,), float("nan"), device=parts.device)
    kept = torch.full((M,), -7, dtype=torch.int32, device=parts.device)
    rc = hip.lib().cvc_sample_select_trunc_parts(parts.data_ptr(), nparts, M * V, None if bias is None else bias.data_ptr(), M, V, unk,
                                                 inv_tau, top_k, top_p, state.data_ptr(), t, word.data_ptr(), 1, lp.data_ptr(),
                                                 cutoff.data_ptr(), kept.data_ptr(), hip._stream())
    hip._check(rc, "cvc_sample_select_trunc_parts")
    return word, lp, cutoff, kept


def plain_block(parts, bias, V, unk, inv_tau, state, t):
    return TS.select_block(parts, bias, V, unk, inv_tau, state, t)


def finished(parts, bias):
    """the finishing pass's order: slab 0 + slab 1 + ... + bias, fp32"""
    z = parts[0].clone()
    for k in range(1, parts.shape[0]):
        z = z + parts[k]
    return z + bias if bias is not None else z


@functools.lru_cache(maxsize=None)
def base_case(M, V, nparts, with_bias):
    """slabs, bias and noise of one shape, shared by its (tau, k, p) cases (never modified: the cases clone)"""
    seed, call, t = 12345 + M + V, 3, 5
    g = torch.Generator().manual_seed(M * 131 + V + nparts)
    parts = torch.randn(nparts, M, V, generator=g) * (1.5 / np.sqrt(nparts))
    bias = torch.randn(V, generator=g) * 0.3 if with_bias else None
    return parts, bias, S.gumbel_noise(seed, call, t, M, V), (seed, call, t)


def set_logit(parts, bias, r, v, target):
    """make the finished logit of (r, v) exactly `target` (fp32): slab 0 searched over a few neighbours of target - bias, the other
    slabs zero.  Changes nothing and returns False if no neighbour sums to the value."""
    b = np.float32(0.0 if bias is None else float(bias[v]))
    t32 = np.float32(target)
    up = dn = np.float32(t32 - b)
    cands = [up]
    for _ in range(3):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        cands += [up, dn]
    for c in cands:
        if np.float32(c + b) == t32:                       # slab 0 + 0 + ... + 0 is exact; the bias is the one rounding
            parts[1:, r, v] = 0.0
            parts[0, r, v] = float(c)
            return True
    return False


def plant(parts, bias, tau, k, p, unk):
    """every third row each: UNK holds the largest logit; an exact duplicate of the k-th value just outside the first k (k > 0); one
    word alone carries more than p of the mass (p < 1).  -> rows of the second and third kind that were planted"""
    M, V = parts.shape[1], parts.shape[2]
    z = finished(parts, bias)
    dup_rows, heavy_rows = [], []
    for r in range(0, M, 3):
        parts[0, r, unk] += float(z[r].max() - z[r, unk]) + 2.0
    if 0 < k < V - 1:
        for r in range(1, M, 3):
            zr = z[r].double().numpy().copy()
            zr[unk] = -np.inf
            order = np.argsort(-zr, kind="stable")
            target = float(z[r, order[k - 1]])
            for v2 in order[k:k + 8]:                        # the first word outside the first k whose slab sum can hit the value
                if zr[v2] < target and set_logit(parts, bias, r, int(v2), target):
                    dup_rows.append(r)
                    break
    if p < 1.0:
        f = 0.5 * (1.0 + p)                                  # the planted word's share of the mass: midway between p and 1
        for r in range(2, M, 3):
            zr = z[r].double().numpy().copy()
            zr[unk] = -np.inf
            top = int(np.argmax(zr))
            rest = np.exp((np.delete(zr, [top, unk]) - zr[top]) / tau).sum()
            new = zr[top] + max(0.0, tau * np.log(rest * f / (1.0 - f))) + 0.25
            parts[0, r, top] += float(new - zr[top])
            heavy_rows.append(r)
    return dup_rows, heavy_rows


SHAPES = [(1, 50, 1, False), (64, 50, 4, True), (64, 52, 2, True), (64, 4999, 1, False), (320, 5000, 8, True), (64, 5000, 6, True),
          (64, 8192, 1, False), (64, 5000, 3, True)]
CASES = [(0.7, 0, 0.9), (0.7, 40, 1.0), (0.7, 40, 0.9), (0.25, 0, 0.9), (0.25, 0, 0.5), (1.0, 1, 1.0), (1.0, 2, 1e-6)]


# ------------------------------------------------------------------ 1. the block against fp64, no row left out
@pytest.mark.parametrize("tau,k,p", CASES)
@pytest.mark.parametrize("M,V,nparts,with_bias", SHAPES)
def test_trunc_block_vs_fp64_on_every_row(dev, M, V, nparts, with_bias, tau, k, p):
    unk = UNK
    parts0, bias, noise, (seed, call, t) = base_case(M, V, nparts, with_bias)
    parts = parts0.clone()
    inv_tau = float(np.float32(1.0 / tau))
    dup_rows, heavy_rows = plant(parts, bias, tau, k, p, unk)
    z = finished(parts, bias)
    zd = z.double().numpy()
    assert (zd[0::3, unk] > np.delete(zd[0::3], unk, axis=1).max(1)).all()           # the planted UNK leads the row
    orders, j_lo, j_hi = R.truncate(z, tau, unk, k, p)
    s = zd * inv_tau + noise
    s[:, unk] = -np.inf
    lse = zd.max(1) + np.log(np.exp(zd - zd.max(1, keepdims=True)).sum(1))

    pd_, bd = parts.contiguous().to(dev), None if bias is None else bias.to(dev)
    state = TS.state_words(seed, call).to(dev)
    word, lp, cutoff, kept = trunc_block(pd_, bd, V, unk, inv_tau, k, p, state, t)
    w_plain, _ = plain_block(pd_, bd, V, unk, inv_tau, state, t)
    w, kept_, cut, w_plain = word.cpu().numpy(), kept.cpu().numpy(), cutoff.cpu().numpy(), w_plain.cpu().numpy()
    print(f"[trunc block] M={M} V={V} nparts={nparts} tau={tau} k={k} p={p}: one-point bands {int((j_lo == j_hi).sum())}/{M}, "
          f"kept min/median/max {kept_.min()}/{int(np.median(kept_))}/{kept_.max()}, at j_lo {int((kept_ == j_lo).sum())}, "
          f"plain word kept {int(sum(w_plain[r] in orders[r][:kept_[r]] for r in range(M)))}/{M}")
    assert ((w >= 0) & (w < V)).all() and not (w == unk).any()
    TOL = 1e-5 * (1.0 + np.abs(s[np.isfinite(s)]).max())
    n_clear = 0
    for r in range(M):
        order, j = orders[r], int(kept_[r])
        assert j_lo[r] <= j <= j_hi[r], (r, j, j_lo[r], j_hi[r])
        vals = z[r, torch.from_numpy(order)].numpy()                                 # fp32 logits by falling value
        assert cut[r] == vals[j - 1] and int((vals >= cut[r]).sum()) == j, (r, j, cut[r], vals[j - 1])   # exactly that prefix
        if p == 1.0:
            assert j == j_lo[r] == j_hi[r], (r, j, j_lo[r], j_hi[r])                 # top-k only: exact
        c2 = order[:j]
        assert w[r] in c2, (r, w[r])
        best = s[r, c2].max()
        assert best - s[r, w[r]] <= TOL, (r, best - s[r, w[r]])
        top2 = np.sort(s[r, c2])[-2:]
        if j == 1 or top2[1] - top2[0] > TOL:                                        # a clear margin: the arg-max itself
            assert w[r] == c2[np.argmax(s[r, c2])], r
            n_clear += 1
        if w_plain[r] in c2:                                                         # the untruncated sampler's word survives
            assert w[r] == w_plain[r], (r, w[r], w_plain[r])
    assert n_clear >= M - (M + 2) // 3
    np.testing.assert_allclose(lp.cpu().double().numpy(), zd[np.arange(M), w] - lse, rtol=0, atol=2e-6)
    if p == 1.0 and 0 < k < V - 1:
        assert len(dup_rows) >= len(range(1, M, 3)) - 1                              # (a row may have no representable duplicate)
        assert (kept_[dup_rows] == k + 1).all(), kept_[dup_rows]
    if p < 1.0:
        assert (kept_[heavy_rows] == 1).all(), kept_[heavy_rows]
    if tau == 0.25:                                         # a condition of the test, not a measurement: sharp rows pin the cutoff
        assert (j_lo == j_hi).sum() >= 0.9 * M, int((j_lo == j_hi).sum())


# ------------------------------------------------------------------ 2. off means off
@pytest.mark.parametrize("M,V,nparts,with_bias", [(64, 50, 4, True), (64, 5000, 6, True), (64, 4999, 1, False)])
def test_truncation_off_is_the_plain_block_and_runs_are_bitwise_repeatable(dev, M, V, nparts, with_bias):
    parts, bias, _, (seed, call, t) = base_case(M, V, nparts, with_bias)
    z = finished(parts, bias)
    pd_, bd = parts.contiguous().to(dev), None if bias is None else bias.to(dev)
    state = TS.state_words(seed, call).to(dev)
    inv_tau = float(np.float32(1.0 / 0.7))
    w0, lp0 = plain_block(pd_, bd, V, UNK, inv_tau, state, t)
    zmin = np.delete(z.numpy(), UNK, axis=1).min(1)
    bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x
    for k in (0, V - 1, V + 7):
        w, lp, cut, kept = trunc_block(pd_, bd, V, UNK, inv_tau, k, 1.0, state, t)
        assert torch.equal(w, w0) and torch.equal(bits(lp), bits(lp0)), k
        assert (kept.cpu().numpy() == V - 1).all() and np.array_equal(cut.cpu().numpy(), zmin), k
        again = trunc_block(pd_, bd, V, UNK, inv_tau, k, 1.0, state, t)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip((w, lp, cut, kept), again)), k
    for k, p in ((40, 0.9), (0, 0.5), (7, 1.0)):
        a = trunc_block(pd_, bd, V, UNK, inv_tau, k, p, state, t)
        b = trunc_block(pd_, bd, V, UNK, inv_tau, k, p, state, t)
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b)), (k, p)


# ------------------------------------------------------------------ 3. the engine against the reference sampler
def _compare_trunc(eng, seq, att, lp, ref, label):
    """TS._compare's rule, and: a row stops being comparable at a step whose cutoff band is wider than one point and whose two ends
    pick different words (its deciding margin counts as 0); engine.kept inside the band while the row follows the reference."""
    seq_o, att_o, lp_o, scores, info = ref
    gaps = S.score_gaps(scores)
    gaps[~info["unambiguous"]] = 0.0
    from helpers import tie_aware_seq_equal
    sq, at, lpn = seq.cpu().numpy(), att.cpu().numpy(), lp.cpu().numpy()
    stats = {}
    n_exact = tie_aware_seq_equal(sq, seq_o.numpy(), None, tol=TS.SCORE_TIE_TOL, clear_gap=TS.SCORE_TIE_TOL, gaps=gaps, stats=stats)
    rows, T = sq.shape
    assert n_exact >= 0.9 * rows * T, (label, n_exact, stats)
    same = np.cumprod(sq == seq_o.numpy(), axis=1).astype(bool)
    ok_t = np.concatenate([np.ones((rows, 1), bool), same[:, :-1]], 1)                # step t depends on the words before it
    assert np.abs(lpn[same] - lp_o.numpy()[same]).max() <= TS.LOGPROB_TOL, label
    np.testing.assert_allclose(at[ok_t], att_o.numpy()[ok_t], **TS.SEQ_TOL)
    kept = eng.kept.t().cpu().numpy()
    assert ((kept >= info["j_lo"]) & (kept <= info["j_hi"]))[ok_t].all(), (label, kept[ok_t], info["j_lo"][ok_t], info["j_hi"][ok_t])
    assert not (sq == UNK).any()
    print(f"[trunc sampling] {label}: {stats}, ambiguous steps {int((~info['unambiguous']).sum())}, "
          f"one-point bands {int((info['j_lo'] == info['j_hi']).sum())}/{rows * T}")


# seeds: at tiny (12 / 36 row-steps) one row lost to a near tie already breaks the 90 % cap, so the seeds are ones at which the
# REFERENCE's smallest deciding margin over both calls is above 10 x SCORE_TIE_TOL (0.118 / 0.052); cfg1 takes what comes
@pytest.mark.parametrize("name,n,path,seed", [("tiny", 1, "ring", 92), ("tiny", 3, "tile", 101), ("cfg1", 1, "packed", 92),
                                              ("cfg1", 5, "tile", 96)])
def test_trunc_engine_vs_reference_sampler(dev, name, n, path, seed):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs(name)
    tau, k, p = 0.8, 10, 0.9
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, sample_n=n, temperature=tau, seed=seed,
                       top_k=k, top_p=p)
    assert (eng.packed, eng.tile) == (path == "packed", path == "tile") and eng._plan is None and eng.trunc
    assert eng.kept.shape == (d.T, d.B * n) and eng.kept.dtype == torch.int32 and eng.cutoff.shape == (d.T, d.B * n)
    for call in (1, 2):
        seq, att, lp = eng.run()
        assert seq.shape == (d.B * n, d.T) and int(eng.rng[2]) == call
        with torch.no_grad():
            ref = R.sample(P, f, d.T, UNK, n, tau, seed, call, top_k=k, top_p=p, tol=engine_mass_tol(tau), ztol=ENGINE_ZTOL)
        _compare_trunc(eng, seq, att, lp, ref, f"{name} n={n} {path} call {call}")
        assert int(eng.kept.max()) <= k + 1 and int(eng.kept.min()) >= 1


@pytest.mark.parametrize("name,path", [("tiny", "ring"), ("cfg1", "packed")])
def test_top_k_1_is_the_greedy_decode(dev, name, path):
    from helpers import to_dev, tie_aware_seq_equal
    from oracle import ref_cpu as O
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs(name)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    seq_g = DecodeEngine(W, fd, d.T, UNK).run()[0].clone().cpu().numpy()
    eng = DecodeEngine(W, fd, d.T, UNK, temperature=0.8, seed=3, top_k=1)
    seq = eng.run()[0].clone().cpu().numpy()
    with torch.no_grad():
        logp_o = O.greedy_sample(P, f, d.T, UNK, return_logprobs=True)[3]
    # equal wherever the fp64 top-2 margin of the oracle's greedy decode is clear (helpers' rule for two greedy decodes)
    n_exact = tie_aware_seq_equal(seq, seq_g, logp_o)
    assert n_exact >= 0.9 * d.B * d.T and int(eng.kept.max()) <= 2


# ------------------------------------------------------------------ 4. graph and seed
@pytest.mark.parametrize("name,n", [("tiny", 3), ("cfg1", 1)])
def test_trunc_graph_replay_draws_fresh_noise_and_seed_reproduces(dev, name, n):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, _, _ = TS._inputs(name)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x
    grab = lambda e: [x.clone() for x in e.run()] + ([e.cutoff.clone(), e.kept.clone()] if e.trunc else [])
    kw = dict(sample_n=n, temperature=1.5)
    plain_before = grab(DecodeEngine(W, fd, d.T, UNK, seed=21, **kw))
    g = DecodeEngine(W, fd, d.T, UNK, seed=9, top_k=10, top_p=0.9, **kw).capture()
    assert int(g.rng[2]) == 0                              # capture (and its warm-up decode) leaves `call` alone
    r1, r2 = grab(g), grab(g)
    assert int(g.rng[2]) == 2 and not torch.equal(r1[0], r2[0])
    k = 3
    g.seed(21)
    for _ in range(k):
        rg = grab(g)
    e = DecodeEngine(W, fd, d.T, UNK, seed=21, top_k=10, top_p=0.9, **kw)
    for _ in range(k):
        re_ = grab(e)
    assert int(g.rng[2]) == k and int(e.rng[2]) == k
    for a, b in zip(rg, re_):
        assert torch.equal(bits(a), bits(b))
    # a temperature-only engine is what it was: the same bits before and after truncating engines ran (and were captured)
    plain_after = grab(DecodeEngine(W, fd, d.T, UNK, seed=21, **kw))
    for a, b in zip(plain_before, plain_after):
        assert torch.equal(bits(a), bits(b))
    off = DecodeEngine(W, fd, d.T, UNK, seed=21, top_k=0, top_p=1.0, **kw)
    assert not off.trunc and not hasattr(off, "kept") and len(off._python_launches()) == len(e._python_launches())
    from cvc import hip
    sel = lambda eng: [fn for nm, fn, _ in eng._python_launches() if nm == "word_select"]
    assert len(sel(off)) == d.T and all(fn is hip.lib().cvc_sample_select_parts for fn in sel(off))
    assert len(sel(e)) == d.T and all(fn is hip.lib().cvc_sample_select_trunc_parts for fn in sel(e))


# ------------------------------------------------------------------ 5. the sampled distribution
def test_trunc_one_step_distribution_on_the_gpu(dev):
    """Step 0 of the tile path at tiny: 64 samples per clip per decode, 50 replays -> 3 200 draws per clip against softmax(z / tau)
    renormalised over the reference's nucleus; nothing outside it (fixed seed: deterministic)."""
    from helpers import to_dev
    from oracle import ref_cpu as O
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs("tiny")
    n, runs, tau, p = 64, 50, 1.3, 0.8
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, sample_n=n, temperature=tau, seed=2, top_p=p)
    eng.capture()
    first = torch.stack([eng.run()[0][:, 0].clone() for _ in range(runs)]).cpu().numpy()      # [runs, B*n]
    with torch.no_grad():
        out, _, _, _, _ = O.decoder_step(P, O.embed(P, torch.zeros(d.B, dtype=torch.long)), f["fc_feats"], f["conv_feats"],
                                         f["p_conv_feats"], f["pool_feats"], f["p_pool_feats"], f["pnt_mask"][:, 1:],
                                         O.init_hidden(d.B, d.R))
        z = torch.nn.functional.linear(out, P["logit.weight"], P["logit.bias"])
    orders, j_lo, j_hi = R.truncate(z, tau, UNK, 0, p, tol=engine_mass_tol(tau), ztol=ENGINE_ZTOL)
    kept0 = eng.kept[0].cpu().numpy().reshape(d.B, n)
    for b in range(d.B):
        counts = np.bincount(first[:, b * n:(b + 1) * n].ravel(), minlength=d.V)
        assert counts[UNK] == 0 and counts[np.setdiff1d(np.arange(d.V), orders[b][:j_hi[b]])].sum() == 0, b
        assert (kept0[b] == kept0[b, 0]).all() and j_lo[b] <= kept0[b, 0] <= j_hi[b] and kept0[b, 0] < d.V - 1
        c2 = orders[b][:kept0[b, 0]]
        prob = np.zeros(d.V)
        prob[c2] = torch.softmax(z[b, torch.from_numpy(c2)].double() / tau, 0).numpy()
        stat, df = S.chi_square(counts, prob)
        assert stat < S.chi_square_critical(df), (b, stat, df)


# ------------------------------------------------------------------ 6. model, trainer, CLI, bf16-stored weights
def test_model_sample_truncates_and_rebinds_when_p_changes(dev):
    from helpers import build_model, to_dev
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=True)
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, 99), dev)
    assert model.sample_top_k == 0 and model.sample_top_p == 1.0
    kw = dict(sample_max=0, temperature=0.9, sample_n=4, seed=3)
    s0 = TS._model_sample(model, f, b, **kw)
    e0 = model._engine_cache[1]
    assert not e0.trunc
    s1 = TS._model_sample(model, f, b, top_k=5, top_p=0.9, **kw)
    e1 = model._engine_cache[1]
    assert e1 is not e0 and e1.trunc and (e1.top_k, e1.top_p) == (5, 0.9)
    assert s1[0].shape == (d.B * 4, d.T) and not (s1[0] == UNK).any() and int(e1.kept.max()) <= 6 and int(e1.kept.min()) >= 1
    TS._model_sample(model, f, b, top_k=5, top_p=0.9, **kw)
    assert model._engine_cache[1] is e1                                             # same options: the cached engine
    TS._model_sample(model, f, b, top_k=5, top_p=0.5, **kw)
    e2 = model._engine_cache[1]
    assert e2 is not e1 and e2.top_p == 0.5
    model.sample_max, model.sample_temperature, model.sample_n, model.sample_seed = 0, 0.9, 4, 3
    model.sample_top_k, model.sample_top_p = 5, 0.9                                 # the model's attributes are the defaults
    from helpers import model_call
    s3 = model_call(model, f, b, True)
    assert model._engine_cache[1].top_k == 5 and torch.equal(s3[0], s1[0]) and torch.equal(s3[2], s1[2])
    assert s0[0].shape == s1[0].shape


def test_trainer_and_cli_sample_with_truncation(dev, tmp_path):
    import json
    from cvc import main as cvc_main
    from cvc import sample as cvc_sample
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16",
              "--seq_length", "4", "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100",
              "--exp_name", "s", "--learning_rate", "0.001", "--results_dir", str(tmp_path / "results"),
              "--checkpoint_path", str(tmp_path) + "/", "--id", "s1"]
    assert cvc_main.main(common) == 0                                              # one epoch -> a checkpoint
    tr = cvc_main.LAST_TRAINER
    path = tr.sample(3, 0.8, seed=4, top_k=5)
    out = json.load(open(path))
    model = getattr(tr.model, "module", tr.model)
    assert model._engine_cache[1].top_k == 5 and model._engine_cache[1].top_p == 1.0
    assert len(out) == 8 and all(len(e["sentences"]) == 3 and len(e["logprobs"]) == 3 and set(e) == {"segment", "timestamp", "sentences",
                                                                                                    "logprobs"}
                                 for segs in out.values() for e in segs)
    assert cvc_sample.main(common + ["--resume", "True", "--temperature", "0.8", "--sample_n", "2", "--sample_seed", "4",
                                     "--top_k", "5", "--top_p", "0.9"]) == 0
    out2 = json.load(open(path))
    assert len(out2) == 8 and all(len(e["sentences"]) == 2 for segs in out2.values() for e in segs)
    e = getattr(cvc_main.LAST_TRAINER.model, "module", cvc_main.LAST_TRAINER.model)._engine_cache[1]
    assert (e.top_k, e.top_p) == (5, 0.9)


def test_bf16_weights_with_top_p_match_the_fp32_engine_on_the_rounded_checkpoint(dev):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights, BF16_ROUNDED_KEYS, bf16_round
    d, sd, f_np, _, _ = TS._inputs("cfg1")
    sd_r = dict(sd)
    for key in BF16_ROUNDED_KEYS:
        sd_r[key] = bf16_round(torch.from_numpy(np.ascontiguousarray(sd[key]))).numpy()
    fd = to_dev(f_np, dev)
    kw = dict(sample_n=1, temperature=0.8, seed=5, top_p=0.9)
    a = DecodeEngine(DecodeWeights(to_dev(sd, dev)), fd, d.T, UNK, weights_dtype="bf16", **kw)
    b = DecodeEngine(DecodeWeights(to_dev(sd_r, dev)), fd, d.T, UNK, **kw)
    assert a.bf16w and a.packed and a.trunc and b.packed and not b.bf16w
    ra, rb = [x.clone() for x in a.run()], [x.clone() for x in b.run()]
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[2].view(torch.int32), rb[2].view(torch.int32))
    assert torch.equal(a.kept, b.kept) and torch.equal(a.cutoff.view(torch.int32), b.cutoff.view(torch.int32))
    assert int(a.kept.max()) < d.V - 1 and not (ra[0] == UNK).any()
