"""Ensemble decoding on the GPU (pytest -m gpu): the combine kernel (csrc/ensemble.hip) against fp64, an ensemble of identical members
against the single engine, two different checkpoints against the joint CPU decoder (tests/ensemble_oracle.py) and against the
members' own forced engines, graph replay and generator state, and the model / command-line plumbing."""
import ctypes as C
import dataclasses
import functools
import json

import numpy as np
import pytest
import torch

from cvc import synth
import ensemble_oracle as EO

pytestmark = pytest.mark.gpu

SEQ_TOL = dict(rtol=1e-4, atol=1e-4)      # attention maps after T recurrent steps (the greedy tests' tolerance)
LOGPROB_TOL = 1e-4
SCORE_TIE_TOL = 2e-3                      # margins below this may flip between two fp32 evaluations of the same decode
UNK = synth.UNK_IDX
SEEDS, WEIGHTS = (4321, 977), (0.4, 0.6)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def _bits(x):
    return x.view(torch.int32) if x.is_floating_point() else x


# ------------------------------------------------------------------ 1. the kernel against fp64
NPARTS = ((1, False), (4, True), (8, True))          # member m: NPARTS[m % 3] -- slab counts and biases differ within one call


def _kernel_inputs(rows, V, M, seed):
    g = np.random.default_rng(seed)
    members, logw_w = [], g.uniform(0.5, 2.0, M)
    for m in range(M):
        nparts, with_bias = NPARTS[m % 3]
        parts = (g.standard_normal((nparts, rows, V)) * (2.0 / np.sqrt(nparts))).astype(np.float32)
        bias = (g.standard_normal(V) * 0.3).astype(np.float32) if with_bias else None
        z = EO.finished(parts, bias)
        far = V // 2 + 3
        parts[0, 0, far] += np.float32((z[0].max() - 120.0) - z[0, far])          # row 0: a word > 110 nats below the top in EVERY member
        if rows > 1 and m == M - 1:
            parts[0, 1, 7] += np.float32(60.0)                                     # row 1: one member near one-hot
        if rows > 2:
            parts[0, 2, UNK] += np.float32(z[2].max() - z[2, UNK] + 5.0)           # row 2: the UNK column largest
        members.append((parts, bias))
    return members, logw_w


def _call_kernel(dev, members, logw, geometric, rows, V, ld_out=None, out=None):
    from cvc import hip
    M = len(members)
    ld_out = V if ld_out is None else ld_out
    keep, src = [], (hip.EnsembleSrc * M)()
    for m, (parts, bias) in enumerate(members):
        p = torch.from_numpy(parts).to(dev).contiguous()
        b = None if bias is None else torch.from_numpy(bias).to(dev)
        keep += [p, b]
        src[m] = hip.EnsembleSrc(p.data_ptr(), parts.shape[0], rows * V, None if b is None else b.data_ptr())
    if out is None:
        out = torch.full((rows, ld_out), float("nan"), device=dev)
    rc = hip.lib().cvc_ensemble_logprobs(src, M, (C.c_float * M)(*logw), geometric, rows, V, out.data_ptr(), ld_out, hip._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("combine", ["prob", "logprob"])
@pytest.mark.parametrize("M", [1, 2, 3, 8])
@pytest.mark.parametrize("rows,V", [(1, 50), (64, 50), (320, 50), (64, 5000), (320, 5000)])
def test_combine_kernel_vs_fp64(dev, rows, V, M, combine):
    from cvc import hip
    members, w = _kernel_inputs(rows, V, M, seed=rows * 7 + V + M)
    logw = hip.ensemble_log_weights(w, M)                        # unequal weights
    geometric = int(combine == "logprob")
    xs = [EO.finished(p, b) for p, b in members]
    ref64 = EO.combine64(xs, logw, geometric)
    err32 = np.abs(EO.combine32(xs, logw, geometric).astype(np.float64) - ref64).max()
    rc, out = _call_kernel(dev, members, logw, geometric, rows, V)
    assert rc == 0
    got = out.cpu().numpy()
    assert np.isfinite(got).all()                                # the word 120 nats below every member's top included
    err = np.abs(got.astype(np.float64) - ref64).max()
    print(f"[ensemble kernel] rows={rows} V={V} M={M} {combine}: kernel {err:.3e}  fp32 numpy {err32:.3e}  ratio {err / err32:.2f}")
    # another expf / logf and another reduction tree than numpy's: the margin the label-smoothing kernels were given
    assert err <= 4.0 * err32, (err, err32)
    assert all(x[0].max() - x[0, V // 2 + 3] > 110.0 for x in xs)       # (the planted word, in every member)
    if rows > 2:
        assert got[2].argmax() == UNK
    # bitwise deterministic
    rc2, out2 = _call_kernel(dev, members, logw, geometric, rows, V)
    assert rc2 == 0 and torch.equal(_bits(out), _bits(out2))
    if combine == "prob":                                        # log sum_m w_m p_m is normalised
        assert np.abs(np.exp(got.astype(np.float64)).sum(1) - 1.0).max() <= 1e-5
    if M == 1:                                                   # logw = {0}: the row log-softmax
        rc1, one = _call_kernel(dev, members, [0.0], geometric, rows, V)
        z = torch.from_numpy(xs[0]).to(dev).contiguous()
        ref = hip.log_softmax_fwd(z)
        d = (one.double() - ref.double()).abs().max().item()
        print(f"[ensemble kernel] rows={rows} V={V} M=1 vs cvc_log_softmax_fwd: {d:.3e}")
        assert rc1 == 0 and d <= 4.0 * err32
    # columns >= V are not written; a row stride that is no multiple of 4 takes the scalar form (another column-to-thread map, so
    # another order of the row sums: the same bound, not the same bits)
    rc3, wide = _call_kernel(dev, members, logw, geometric, rows, V, ld_out=V + 3)
    assert rc3 == 0 and torch.isnan(wide[:, V:]).all()
    assert np.abs(wide[:, :V].cpu().numpy().astype(np.float64) - ref64).max() <= 4.0 * err32


def test_combine_kernel_refusals(dev):
    from cvc import hip
    L, BAD, BIG = hip.lib(), -1, -2
    rows, V = 4, 52
    members, _ = _kernel_inputs(rows, V, 2, seed=1)
    p = [torch.from_numpy(m[0]).to(dev).contiguous() for m in members]
    out = torch.zeros(rows, V, device=dev)

    def call(src=None, M=2, logw=(-0.7, -0.7), rows_=rows, V_=V, out_=out, ld=V, nparts=(1, 4), stride=rows * V, null_parts=False):
        s = (hip.EnsembleSrc * 8)()
        for m in range(min(max(M, 0), 2)):
            s[m] = hip.EnsembleSrc(None if null_parts else p[m].data_ptr(), nparts[m], stride, None)
        lw = None if logw is None else (C.c_float * 8)(*logw)
        return L.cvc_ensemble_logprobs(None if src == "null" else s, M, lw, 0, rows_, V_, None if out_ is None else out_.data_ptr(), ld,
                                       hip._stream())
    assert call() == 0
    assert call(src="null") == BAD and call(logw=None) == BAD and call(out_=None) == BAD and call(null_parts=True) == BAD
    assert call(M=0) == BAD and call(M=9) == BAD
    assert call(ld=V - 1) == BAD
    assert call(logw=(float("nan"), -0.7)) == BAD and call(logw=(-0.7, float("-inf"))) == BAD and call(logw=(float("inf"), 0.0)) == BAD
    assert call(nparts=(1, 0)) == BAD and call(stride=rows * V - 1) == BAD and call(rows_=0) == BAD and call(V_=1, ld=V) == BAD
    assert call(V_=8193, ld=8193) == BIG                              # as select_row_check: more than 32 columns per thread
    assert call(rows_=1 << 20, V_=8192, ld=8192, stride=(1 << 20) * 8192) == BIG     # rows * V >= 2^32
    torch.cuda.synchronize()


# ------------------------------------------------------------------ inputs of the engine tests
@functools.lru_cache(maxsize=None)
def _member_np(name, seed, B=None):
    d = synth.CONFIGS[name]
    if B is not None:
        d = dataclasses.replace(d, B=B)
    sd, f = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed)
    f["pnt_mask"] = synth.clip_features(d, SEEDS[0])["pnt_mask"]          # every encoder sees the same proposals: one proposal mask
    return d, sd, f


def _members(name, dev, seeds=SEEDS, feat_seeds=None):
    """[(DecodeWeights, feats on the device)], and the same on the CPU for the oracle: each checkpoint with its own features"""
    from helpers import to_dev
    from oracle import ref_cpu as O
    from cvc.decode import DecodeWeights
    gpu, cpu = [], []
    for s, fs in zip(seeds, feat_seeds or seeds):
        d, sd, _ = _member_np(name, s)
        f = _member_np(name, fs)[2]
        gpu.append((DecodeWeights(to_dev(sd, dev)), to_dev(f, dev)))
        cpu.append((O.to_torch(sd), O.to_torch(f)))
    return d, gpu, cpu


def _cut_compare(a, b, may_cut, label):
    """Tie-aware: rows of a and b agree up to the first step at which they differ, where may_cut(r, t) must hold (a margin below
    SCORE_TIE_TOL); the rest of such a row is not compared.  -> the mask of compared positions, at least 90 % of all."""
    a, b = np.asarray(a), np.asarray(b)
    same = np.cumprod(a == b, axis=1).astype(bool)
    for r in np.nonzero(~same.all(1))[0]:
        t = int(np.argmin(same[r]))
        assert may_cut(r, t), f"{label}: row {r} differs at step {t} with a clear margin: {a[r]} vs {b[r]}"
    share = same.mean()
    print(f"[ensemble] {label}: {same.sum()} of {same.size} positions compared")
    assert share >= 0.9, (label, share)
    return same


def _att_mask(same):
    return np.concatenate([np.ones((same.shape[0], 1), bool), same[:, :-1]], 1)       # attention of step t depends on words < t


# ------------------------------------------------------------------ 2. identical members = the single engine
@pytest.mark.parametrize("combine", ["prob", "logprob"])
@pytest.mark.parametrize("name,kw", [
    ("tiny", dict(path="ring")), ("tiny", dict(path="tile")), ("cfg1", dict()),
    ("tiny", dict(beam=3)), ("cfg1", dict(beam=3)),
    ("tiny", dict(beam=3, beam_history=True, no_repeat_ngram=2)),
    ("tiny", dict(sample_n=3, temperature=0.7, seed=11)),
])
def test_identical_members_equal_the_single_engine(dev, name, kw, combine):
    from cvc.decode import DecodeEngine, EnsembleEngine
    d, gpu, _ = _members(name, dev, seeds=(SEEDS[0],))
    W, f = gpu[0]
    single = DecodeEngine(W, f, d.T, UNK, **kw)
    ens = EnsembleEngine([(W, f), (W, f)], d.T, UNK, member_weights=(0.3, 0.7), combine=combine, **kw)
    path = kw.get("path", "packed" if name == "cfg1" and "beam" not in kw else None)
    if path is not None:
        for e in ens.members:
            assert (e.packed, e.tile) == (path == "packed", path == "tile")
    assert all(e._plan is None for e in ens.members) and ens.members[1].words is ens.members[0].words
    rs = [x.clone() for x in single.run()]
    re_ = [x.clone() for x in ens.run()]
    label = f"identical {name} {kw} {combine}"
    assert not (re_[0] == UNK).any()
    if kw.get("beam", 1) > 1:
        ss, se = rs[2].cpu().numpy(), re_[2].cpu().numpy()
        # a returned hypothesis may differ only where the two best final scores are a tie
        same = _cut_compare(re_[0].cpu(), rs[0].cpu(), lambda r, t: abs(ss[r, 0] - se[r, 0]) < SCORE_TIE_TOL, label)
        whole = same.all(1)
        np.testing.assert_allclose(se[whole], ss[whole], rtol=0, atol=LOGPROB_TOL * d.T)           # LOGPROB_TOL per step
        if kw.get("beam_history"):
            hs, he = single.hypotheses(), ens.hypotheses()
            assert torch.equal(hs[0][torch.from_numpy(whole)], he[0][torch.from_numpy(whole)])
            rows_ok = torch.from_numpy(np.repeat(whole, 3))
            assert torch.equal(single.nbanned.cpu()[:, rows_ok], ens.nbanned.cpu()[:, rows_ok])
    elif "temperature" in kw:
        import sample_oracle as S
        from oracle import ref_cpu as O
        _, sd, fn = _member_np(name, SEEDS[0])
        with torch.no_grad():
            gaps = S.score_gaps(S.sample(O.to_torch(sd), O.to_torch(fn), d.T, UNK, 3, 0.7, 11, 1)[3])
        same = _cut_compare(re_[0].cpu(), rs[0].cpu(), lambda r, t: gaps[r, t] < SCORE_TIE_TOL, label)
        assert np.abs(re_[2].cpu().numpy()[same] - rs[2].cpu().numpy()[same]).max() <= LOGPROB_TOL
        assert torch.equal(ens.rng_state, single.rng_state)                 # one generator, advanced once
    else:
        lps, lpe = single.logprob.t().cpu().numpy(), ens.logprob.t().cpu().numpy()
        # two arg-max words of (nearly) one distribution: the margin is the difference of their log-probs
        same = _cut_compare(re_[0].cpu(), rs[0].cpu(), lambda r, t: abs(lps[r, t] - lpe[r, t]) < SCORE_TIE_TOL, label)
        assert np.abs(lpe[same] - lps[same]).max() <= LOGPROB_TOL
    ok = _att_mask(same)
    if kw.get("beam", 1) > 1:
        ok = ok & same.all(1, keepdims=True)            # a backtracked row follows ONE hypothesis: compared where it is the same one
    np.testing.assert_allclose(re_[1].cpu().numpy()[ok], rs[1].cpu().numpy()[ok], **SEQ_TOL)


# ------------------------------------------------------------------ 3. two different checkpoints
def _mixture_of_members(dev, d, gpu, words, nq):
    """log sum_m w_m exp(logprob_m[t]) of `words` [rows, T] from each member's OWN forced engine"""
    from cvc.decode import DecodeEngine
    w = np.asarray(WEIGHTS) / np.sum(WEIGHTS)
    lps = []
    for W, f in gpu:
        e = DecodeEngine(W, f, d.T, UNK, forced_n=nq).load_captions(words.contiguous())
        lps.append(e.run()[2].double().cpu().numpy())
    a = np.stack(lps) + np.log(w).reshape(-1, 1, 1)
    return a.max(0) + np.log(np.exp(a - a.max(0)).sum(0))


@pytest.mark.parametrize("combine", ["prob", "logprob"])
@pytest.mark.parametrize("name", ["tiny", "cfg1"])
def test_two_checkpoints_greedy_vs_joint_cpu_decoder(dev, name, combine):
    from helpers import tie_aware_seq_equal
    from cvc.decode import EnsembleEngine
    d, gpu, cpu = _members(name, dev)
    assert not np.array_equal(_member_np(name, SEEDS[0])[2]["pool_feats"], _member_np(name, SEEDS[1])[2]["pool_feats"])
    ens = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, combine=combine)
    seq, att = (x.clone() for x in ens.run())
    lp = ens.logprob.t().cpu().numpy()
    seq_o, att_o, lp_o, mix, _ = EO.joint_greedy([c[0] for c in cpu], [c[1] for c in cpu], d.T, UNK, WEIGHTS, combine)
    stats = {}
    n_exact = tie_aware_seq_equal(seq.cpu().numpy(), seq_o, mix, tol=SCORE_TIE_TOL, clear_gap=SCORE_TIE_TOL, stats=stats)
    print(f"[ensemble] two checkpoints {name} {combine}: {stats}")
    assert n_exact >= 0.9 * d.B * d.T, (n_exact, stats)
    assert not (seq == UNK).any()
    same = np.cumprod(seq.cpu().numpy() == seq_o, axis=1).astype(bool)
    assert np.abs(lp[same] - lp_o[same]).max() <= 2 * LOGPROB_TOL
    ok = _att_mask(same)
    np.testing.assert_allclose(att.cpu().numpy()[ok], (0.4 * att_o[0] + 0.6 * att_o[1])[ok], **SEQ_TOL)
    # the members are really different models: each one alone decodes something else somewhere, or scores it differently
    if combine == "prob":
        np.testing.assert_allclose(lp, _mixture_of_members(dev, d, gpu, seq, 1), rtol=0, atol=2 * LOGPROB_TOL)


@pytest.mark.parametrize("combine", ["prob", "logprob"])
@pytest.mark.parametrize("kw", [dict(), dict(beam=3), dict(sample_n=3, temperature=0.9, seed=5)])
def test_two_checkpoints_consistent_with_the_members_forced_engines(dev, kw, combine):
    from cvc.decode import EnsembleEngine
    name = "tiny"
    d, gpu, cpu = _members(name, dev)
    ens = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, combine=combine, **kw)
    res = [x.clone() for x in ens.run()]
    seq = res[0]
    assert not (seq == UNK).any()
    nq = kw.get("sample_n", 1)
    if combine == "prob":
        ref = _mixture_of_members(dev, d, gpu, seq, nq)
    else:       # the normalised geometric mixture of the joint CPU decoder over the same words
        rep = lambda f: {k: v.repeat_interleave(nq, 0) for k, v in f.items()}
        ref = EO.joint_greedy([c[0] for c in cpu], [rep(c[1]) for c in cpu], d.T, UNK, WEIGHTS, combine, given=seq.cpu().numpy())[2]
    if "beam" in kw:            # the final score of the returned hypothesis: the sum over its steps up to and including the first 0
        s = seq.cpu().numpy()
        ended = np.cumsum(s == 0, 1) - (s == 0)
        total = (ref * (ended == 0)).sum(1)
        np.testing.assert_allclose(res[2][:, 0].cpu().numpy(), total, rtol=0, atol=2 * LOGPROB_TOL * d.T)
    else:
        lp = ens.logprob.t().cpu().numpy()
        np.testing.assert_allclose(lp, ref, rtol=0, atol=2 * LOGPROB_TOL)


@pytest.mark.parametrize("combine", ["prob", "logprob"])
def test_forced_ensemble_scores_given_words_and_ranks_them(dev, combine):
    from cvc.decode import EnsembleEngine
    d, gpu, cpu = _members("tiny", dev)
    n = 2
    g = torch.Generator().manual_seed(3)
    words = torch.randint(0, d.V, (d.B * n, d.T), generator=g)           # arbitrary words: far down the ranking included
    ens = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, combine=combine, forced_n=n)
    ens.load_captions(words.to(dev))
    seq, att, lp, rank = (x.clone() for x in ens.run())
    assert torch.equal(seq.cpu(), words)
    rep = lambda f: {k: v.repeat_interleave(n, 0) for k, v in f.items()}
    _, att_o, lp_o, mix, _ = EO.joint_greedy([c[0] for c in cpu], [rep(c[1]) for c in cpu], d.T, UNK, WEIGHTS, combine, given=words.numpy())
    np.testing.assert_allclose(lp.cpu().numpy(), lp_o, rtol=0, atol=2 * LOGPROB_TOL)
    if combine == "prob":
        np.testing.assert_allclose(lp.cpu().numpy(), _mixture_of_members(dev, d, gpu, words.to(dev), n), rtol=0, atol=2 * LOGPROB_TOL)
    np.testing.assert_allclose(att.cpu().numpy(), 0.4 * att_o[0] + 0.6 * att_o[1], **SEQ_TOL)
    # the rank under the mixture, wherever the given word's fp64 margin to its neighbours is clear
    zw = np.take_along_axis(mix, words.numpy()[:, :, None], 2)
    rank_o = (mix > zw).sum(2)
    other = np.abs(mix - zw)
    np.put_along_axis(other, words.numpy()[:, :, None], np.inf, 2)
    clear = other.min(2) > SCORE_TIE_TOL
    assert clear.mean() > 0.5 and rank_o.max() > d.V // 2
    assert np.array_equal(rank.cpu().numpy()[clear], rank_o[clear])


# ------------------------------------------------------------------ 4. graph and state
@pytest.mark.parametrize("kw", [dict(), dict(beam=3)])
def test_captured_ensemble_replays_the_eager_bits(dev, kw):
    from cvc.decode import EnsembleEngine
    d, gpu, _ = _members("tiny", dev)
    eager = [x.clone() for x in EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, **kw).run()]
    g = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, **kw).capture()
    for _ in range(2):
        for a, b in zip(eager, g.run()):
            assert torch.equal(_bits(a), _bits(b))


def test_sampling_ensemble_draws_afresh_and_seed_repeats(dev):
    from cvc.decode import DecodeEngine, EnsembleEngine
    d, gpu, _ = _members("tiny", dev)
    kw = dict(sample_n=3, temperature=1.5)
    g = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, seed=9, **kw).capture()
    assert [e[0] for e in g._launches].count("sample_advance") == 1 and int(g.rng_state[2]) == 0
    r1 = [x.clone() for x in g.run()]
    r2 = [x.clone() for x in g.run()]
    assert int(g.rng_state[2]) == 2 and not torch.equal(r1[0], r2[0])
    g.seed(21)
    e = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, seed=21, **kw)
    s = DecodeEngine(gpu[0][0], gpu[0][1], d.T, UNK, seed=21, **kw)
    for _ in range(3):
        rg, re_ = [x.clone() for x in g.run()], [x.clone() for x in e.run()]
        s.run()
    for a, b in zip(rg, re_):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(g.rng_state, s.rng_state) and torch.equal(e.rng_state, s.rng_state)     # as the single engine leaves it


def test_load_features_equals_a_fresh_engine(dev):
    from cvc.decode import EnsembleEngine
    d, gpu, _ = _members("tiny", dev)
    _, gpu2, _ = _members("tiny", dev, feat_seeds=(55, 66))
    e = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, own_features=True).capture()
    e.run()
    got = [x.clone() for x in e.load_features([f for _, f in gpu2]).run()] + [e.logprob.clone()]
    fresh = EnsembleEngine(gpu2, d.T, UNK, member_weights=WEIGHTS)
    want = [x.clone() for x in fresh.run()] + [fresh.logprob.clone()]
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(RuntimeError, match="2 members need 2 feature dicts"):
        e.load_features([gpu2[0][1]])


@pytest.mark.parametrize("kw", [dict(), dict(beam=3)])
def test_members_swapped_give_the_same_words(dev, kw):
    """member buffers other than the shared words / parents are not aliased: the decode does not depend on who is primary"""
    from cvc.decode import EnsembleEngine
    d, gpu, _ = _members("tiny", dev)
    a = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, **kw)
    b = EnsembleEngine(gpu[::-1], d.T, UNK, member_weights=WEIGHTS[::-1], **kw)
    ra, rb = [x.clone() for x in a.run()], [x.clone() for x in b.run()]
    own = ("logits", "att_steps", "logprob", "scores_r", "gate_fc", "emb")
    assert all(getattr(a.members[0], k).data_ptr() != getattr(a.members[1], k).data_ptr() for k in own)
    assert a.members[0].words.data_ptr() == a.members[1].words.data_ptr()
    if "beam" in kw:
        sa, sb = ra[2].cpu().numpy(), rb[2].cpu().numpy()
        same = _cut_compare(ra[0].cpu(), rb[0].cpu(), lambda r, t: abs(sa[r, 0] - sb[r, 0]) < SCORE_TIE_TOL, f"swapped {kw}")
    else:
        la, lb = a.logprob.t().cpu().numpy(), b.logprob.t().cpu().numpy()
        same = _cut_compare(ra[0].cpu(), rb[0].cpu(), lambda r, t: abs(la[r, t] - lb[r, t]) < SCORE_TIE_TOL, f"swapped {kw}")
        assert np.abs(la[same] - lb[same]).max() <= LOGPROB_TOL
    ok = _att_mask(same) & (same.all(1, keepdims=True) if "beam" in kw else True)
    np.testing.assert_allclose(ra[1].cpu().numpy()[ok], rb[1].cpu().numpy()[ok], **SEQ_TOL)


def test_engine_surface_and_member_mismatch(dev):
    from helpers import to_dev
    from cvc.decode import DecodeWeights, EnsembleEngine
    d, gpu, _ = _members("tiny", dev)
    e = EnsembleEngine(gpu[:1], d.T, UNK)                       # M = 1: the single model through the combine launch
    assert e.run()[0].shape == (d.B, d.T)
    for call in (lambda: e.bind_features(gpu[0][1]), e.run_timed, lambda: e.set_mix_prob(0.5), lambda: e.seed(1),
                 lambda: e.load_captions(e.words[1:].t().contiguous())):
        with pytest.raises(RuntimeError):
            call()
    d2 = dataclasses.replace(d, N=d.N + 1)
    other = (DecodeWeights(to_dev(synth.hot_path_state_dict(d2, 5), dev)), to_dev(synth.clip_features(d2, 5), dev))
    with pytest.raises(RuntimeError, match=r"member 1 has N = 8, member 0 has N = 7"):
        EnsembleEngine([gpu[0], other], d.T, UNK)
    f_bad = dict(gpu[1][1])
    f_bad["pnt_mask"] = ~f_bad["pnt_mask"] if f_bad["pnt_mask"].dtype == torch.bool else 1 - f_bad["pnt_mask"]
    with pytest.raises(RuntimeError, match="member 1's proposal mask"):
        EnsembleEngine([gpu[0], (gpu[1][0], f_bad)], d.T, UNK)
    # n-best, consensus candidates and set diversity read the buffers the ensemble's selection filled
    h = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, beam=3, beam_history=True)
    seq, att, score = h.run()
    hyp, hs = h.hypotheses()
    assert hyp.shape == (d.B, 3, d.T) and torch.equal(hs, score)
    cand, n, live = h.candidates()
    assert cand.shape == (d.B * 3, d.T) and n == 3 and live.shape == (d.B * 3,)
    assert h.set_diversity()["div"].shape == (d.B, 2)


# ------------------------------------------------------------------ 5. model level
def _batch(d, dev, seed=99):
    from helpers import to_dev
    return to_dev(synth.clip_features(d, seed, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, seed), dev)


def _sample(model, f, b, **kw):
    dummy = torch.zeros(f["fc_feats"].shape[0], 1, 1, device=f["fc_feats"].device)
    return model._sample(f, b["input_seq"], b["proposals"], b["gt_seq"], b["num"], b["box_mask"], b["gt_bboxs"], dummy, b["frm_mask"],
                         b["sample_idx"], f["pnt_mask"], **kw)


def _score(model, f, b, **kw):
    dummy = torch.zeros(f["fc_feats"].shape[0], 1, 1, device=f["fc_feats"].device)
    return model.score(f, b["input_seq"], b["gt_seq"], b["num"], b["proposals"], b["gt_bboxs"], b["box_mask"], dummy, b["frm_mask"],
                       b["sample_idx"], f["pnt_mask"], **kw)


@pytest.mark.parametrize("graph", [False, True])
def test_caption_ensemble_of_one_model_twice_equals_the_model(dev, graph):
    from helpers import build_model
    from cvc.model.ensemble import CaptionEnsemble
    d = synth.CONFIGS["tiny"]
    m = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=graph)
    f, b = _batch(d, dev)
    ens = CaptionEnsemble([m, m], weights=(0.3, 0.7))
    assert ens.eval() is ens and ens.seq_length == d.T
    for kw in (dict(), dict(beam_size=3)):
        s_m, s_e = _sample(m, f, b, **kw), _sample(ens, f, b, **kw)
        assert s_e[2] is None and s_m[2] is None
        em, ee = m._engine_cache[1], ens._engine_cache[1]
        if kw:      # the returned hypotheses may differ where the two best final scores tie
            sm, se = (e.score[d.T & 1].view(d.B, 3).cpu().numpy() for e in (em, ee))
            same = _cut_compare(s_e[0].cpu(), s_m[0].cpu(), lambda r, t: abs(sm[r, 0] - se[r, 0]) < SCORE_TIE_TOL, f"model {kw}")
            ok = _att_mask(same) & same.all(1, keepdims=True)
            np.testing.assert_allclose(se[same.all(1)], sm[same.all(1)], rtol=0, atol=LOGPROB_TOL * d.T)
        else:
            lm, le = em.logprob.t().cpu().numpy(), ee.logprob.t().cpu().numpy()
            same = _cut_compare(s_e[0].cpu(), s_m[0].cpu(), lambda r, t: abs(lm[r, t] - le[r, t]) < SCORE_TIE_TOL, f"model {kw}")
            ok = _att_mask(same)
            assert np.abs(le[same] - lm[same]).max() <= LOGPROB_TOL
        np.testing.assert_allclose(s_e[1].cpu().numpy()[ok], s_m[1].cpu().numpy()[ok], **SEQ_TOL)
    # the cache: a second batch of the same shape reuses the engine
    eng = ens._engine_cache[1]
    f2, b2 = _batch(d, dev, seed=7)
    assert _sample(ens, f2, b2, beam_size=3)[0].shape == (d.B, d.T) and ens._engine_cache[1] is eng
    with pytest.raises(RuntimeError, match='weights_dtype="bf16" is refused'):
        _sample(ens, f, b, decode_weights="bf16")
    with pytest.raises(RuntimeError, match="grounding=True is refused"):
        _score(ens, f, b, grounding=True)


def test_caption_ensemble_score_is_the_mixture_of_the_members_scores(dev):
    from helpers import build_model
    from cvc.model.ensemble import CaptionEnsemble
    d = synth.CONFIGS["tiny"]
    m0, m1 = (build_model(d, synth.hot_path_state_dict(d, s), dev) for s in SEEDS)
    f, b = _batch(d, dev)
    out = _score(CaptionEnsemble([m0, m1], weights=WEIGHTS), f, b)
    o0, o1 = _score(m0, f, b), _score(m1, f, b)
    a = np.stack([o0["logprob"].double().cpu().numpy() + np.log(0.4), o1["logprob"].double().cpu().numpy() + np.log(0.6)])
    ref = a.max(0) + np.log(np.exp(a - a.max(0)).sum(0))
    np.testing.assert_allclose(out["logprob"].cpu().numpy(), ref, rtol=0, atol=2 * LOGPROB_TOL)
    assert torch.equal(out["mask"], o0["mask"]) and out["rank"].shape == o0["rank"].shape
    np.testing.assert_allclose(out["att"].cpu().numpy(), (0.4 * o0["att"] + 0.6 * o1["att"]).cpu().numpy(), **SEQ_TOL)
    one = _score(CaptionEnsemble([m0]), f, b)                 # a one-model ensemble is allowed
    np.testing.assert_allclose(one["logprob"].cpu().numpy(), o0["logprob"].cpu().numpy(), rtol=0, atol=LOGPROB_TOL)


def test_main_inference_with_ensemble_writes_the_ensembles_sentences(dev, tmp_path):
    from cvc import main as cvc_main
    from cvc.misc import utils
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16",
              "--seq_length", "4", "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100",
              "--learning_rate", "0.01", "--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/",
              "--language_eval"]
    assert cvc_main.main(common + ["--exp_name", "b", "--id", "b1", "--seed", "7"]) == 0          # a second checkpoint ...
    assert cvc_main.main(common + ["--exp_name", "a", "--id", "a1"]) == 0                         # ... and the one that is resumed
    other = str(tmp_path / "b" / "model.pth")
    assert cvc_main.main(common + ["--exp_name", "a", "--id", "a1", "--resume", "True", "--inference_only", "--ensemble", other,
                                   "--ensemble_weights", "1,2"]) == 0
    tr = cvc_main.LAST_TRAINER
    assert tr.ensemble is not None and len(tr.ensemble.models) == 2 and tr.ensemble.models[0] is getattr(tr.model, "module", tr.model)
    written = json.load(open(tr.submission_file))["results"]
    assert len(written) == 8
    o, ds, n = tr.opts, tr.dataset, 0
    with torch.no_grad():
        for bt in tr._val_batches():
            seq = tr.ensemble._sample(bt["segs_feat"], bt["input_seqs"], bt["ppls"], bt["gt_seqs"], bt["num"], bt["mask_bboxs"],
                                      bt["gt_bboxs"], bt["ppls_feat"], bt["mask_frms"], bt["sample_idx"], bt["pnt_mask"])[0]
            sents = utils.decode_sequence(ds.itow, getattr(ds, "itod", None), getattr(ds, "ltow", None), getattr(ds, "itoc", None),
                                          getattr(ds, "wtod", None), seq.data, o.vocab_size, o)
            for k, sent in enumerate(sents):
                vid, seg = bt["seg_id"][k].split("_segment_")
                assert [e["sentence"] for e in written[vid] if e["segment"] == str(int(seg))] == [sent]
                n += 1
    assert n == 8
    with pytest.raises(SystemExit, match="--ensemble needs --resume True"):
        cvc_main.main(common + ["--exp_name", "a", "--id", "a1", "--ensemble", other])
