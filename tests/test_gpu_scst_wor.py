"""GPU tests (pytest -m gpu) of self-critical training on captions sampled without replacement: the block cvc_scst_weights_wor
(csrc/scst_wor.hip) against the fp64 restatement tests/wor_ref.py, its statistics on the stochastic-beam toy, and the route from the
stochastic engine through model.scst_loss(wor=) to Trainer.scst_step with opts.scst_wor.  Figures: profiles/scst_wor.md.

Tolerances.  An output is compared with the fp64 reference relative to its SCALE: |wgt| for a weight, and for est and adv -- sums and
differences that may cancel -- the same expression over |f| (wor_ref.weights' est_scale / adv_scale); a scale below 1e-30 counts as
1e-30 (the absolute floor: fp32 has no relative precision to give down there).  REL_BOUND is the largest such relative error MEASURED
on the device over the block cases of this file (printed by every run); the tests assert 4 x REL_BOUND.  It is the inputs', not the
sums': logq down to -150 and a threshold down to -120 carry an absolute rounding error of about 150 * 2^-24 = 9e-6 into an exponent,
and 1 + (a - 1) exp(kt) cancels when a is small and kt is near 0."""
import functools

import numpy as np
import pytest
import torch

from cvc import synth
import sample_oracle as SO
import wor_ref as W

pytestmark = pytest.mark.gpu

BADARG = -1
REL_BOUND = 7.46e-6                           # measured (B = 70, S = 7, T = 9, unnormalised wgt): profiles/scst_wor.md
REL_TOL = 4 * REL_BOUND
FLOOR = 1e-30
Z_OK = 4.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def state_words(seed, call):
    lo, hi = SO.seed_words(seed)
    return torch.from_numpy(np.array([lo, hi, call, 0], dtype=np.uint32).view(np.int32))


# ------------------------------------------------------------------ 1. the block against the reference
@functools.lru_cache(maxsize=None)
def block_case(B, S, T):
    """fp32 inputs that meet every branch of the rule (asserted on the union of the cases by test_inputs_meet_every_branch)"""
    rng = np.random.default_rng(10000 * B + 100 * S + T)
    mag = lambda lo, hi, n: np.exp(rng.uniform(np.log(lo), np.log(hi), n))         # log-uniform magnitudes
    base = -mag(0.01, 150.0, B)
    logq = np.clip(base[:, None] + rng.normal(0, 3.0, (B, S + 1)) * (rng.random((B, 1)) < 0.7), -150.0, -0.01)
    # the threshold: near the clip's log-probs (x on both sides of 1), or anywhere in [-120, -1e-3]
    near = rng.random(B) < 0.5
    kt = np.where(near, logq[:, :S].mean(1) + rng.normal(0, 2.0, B), -mag(1e-3, 120.0, B))
    kt = np.clip(kt, -120.0, -1e-3)
    G = logq + rng.gumbel(size=(B, S + 1))
    G[:, S] = kt
    dead_thr = rng.random(B) < 0.2
    G[dead_thr, S] = -np.inf
    dead = rng.random((B, S)) < 0.15                             # dead rollouts, in the middle of a clip too: fillers hold -inf in both
    if B > 1:
        dead[0] = False
        dead[1, :] = True                                        # a clip without a live rollout ...
        dead[B - 1, 1:] = True                                   # ... and one with a single live row
        dead[B - 1, 0] = False
    G[:, :S][dead] = -np.inf
    logq[:, :S][dead] = -np.inf
    reward = rng.random(B * S) * 10
    V = 23
    cand = rng.integers(1, V, (B * S, T)).astype(np.int64)
    for r in range(B * S):                                       # an end mark anywhere (words behind it stay), or none
        L = int(rng.integers(1, T + 2))
        if L <= T:
            cand[r, L - 1] = 0
    seed, call = int(rng.integers(1, 2 ** 40)), int(rng.integers(1, 1000))
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return dict(B=B, S=S, T=T, reward=f32(reward), logq=f32(logq), G=f32(G), cand=cand, seed=seed, call=call)


def reference(c, normalize, call=None):
    lo, hi = SO.seed_words(c["seed"])
    a = W.root_exponential(W.root_hash(lo, hi, c["call"] if call is None else call, c["B"]))
    return W.weights(c["reward"].astype(np.float64), c["logq"].astype(np.float64), c["G"].astype(np.float64), a, normalize=normalize)


def launch(c, dev, t_major, normalize, call=None):
    from cvc import hip
    t = lambda x: torch.from_numpy(x).to(dev)
    return hip.scst_weights_wor(t(c["reward"]), t(c["logq"]), t(c["G"]), state_words(c["seed"], c["call"] if call is None else call).to(dev),
                                c["S"], t(c["cand"]), t_major=t_major, normalize=normalize)


def rel_errors(got, ref):
    """the largest |got - ref| / max(scale, FLOOR) of wgt, adv and est"""
    adv, wgt, est = (x.cpu().double().numpy() for x in got[:3])
    B, S = ref["wgt"].shape
    e = lambda g, r, s: float((np.abs(g - r) / np.maximum(s, FLOOR)).max())
    return dict(wgt=e(wgt.reshape(B, S), ref["wgt"], np.abs(ref["wgt"])), adv=e(adv.reshape(B, S), ref["adv"], ref["adv_scale"]),
                est=e(est, ref["est"], ref["est_scale"]))


CASES = [(B, S, T) for B in (1, 5, 70) for S in (2, 5, 7) for T in (1, 9, 20)]


def test_inputs_meet_every_branch():
    seen = dict(x_lt_1=0, x_ge_1=0, x_zero=0, x_inf=0, dead_thr=0, dead_mid=0, no_live=0, one_live=0, no_end=0, end=0, far=0, near=0,
                kt_near_0=0, kt_far=0)
    for B, S, T in CASES:
        c = block_case(B, S, T)
        r = reference(c, True)
        G, logq = c["G"].astype(np.float64), c["logq"].astype(np.float64)
        live = np.isfinite(G[:, :S])
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.exp(np.float32(logq[:, :S] + r["lam"][:, None]))[live & np.isfinite(r["lam"])[:, None]]
        seen["x_lt_1"] += int(((x < 1) & (x > 0)).sum()); seen["x_ge_1"] += int(((x >= 1) & np.isfinite(x)).sum())
        seen["x_zero"] += int((x == 0).sum()); seen["x_inf"] += int((np.isinf(r["lam"])[:, None] & live).sum())
        seen["dead_thr"] += int(np.isinf(G[:, S]).sum())
        seen["dead_mid"] += int((~live[:, 1:-1] & live[:, 2:] & live[:, :-2]).sum()) if S > 2 else 0
        seen["no_live"] += int((r["n_live"] == 0).sum()); seen["one_live"] += int((r["n_live"] == 1).sum())
        seen["no_end"] += int((c["cand"] != 0).all(1).sum()); seen["end"] += int((c["cand"] == 0).any(1).sum())
        lq = logq[:, :S][live]
        seen["far"] += int((lq < -88).sum()); seen["near"] += int((lq > -1).sum())
        kt = G[:, S][np.isfinite(G[:, S])]
        seen["kt_near_0"] += int((kt > -0.1).sum()); seen["kt_far"] += int((kt < -88).sum())
        assert logq[:, :S][live].min() >= -150 and lq.max() <= np.float32(-0.01) and (kt.size == 0 or (kt.min() >= -120 and kt.max() <= np.float32(-1e-3)))
    print("[wor inputs]", seen)
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("B,S,T", CASES)
def test_block_against_the_reference(dev, B, S, T):
    c = block_case(B, S, T)
    worst = {}
    for normalize in (True, False):
        ref = reference(c, normalize)
        outs = {}
        for t_major in (False, True):
            got = launch(c, dev, t_major, normalize)
            adv, wgt, est, w = got
            assert adv.shape == (B * S,) and wgt.shape == (B * S,) and est.shape == (B,) and w.shape == ((T, B * S) if t_major else (B * S, T))
            # w is exactly adv on the mask and 0 off it
            assert np.array_equal(w.cpu().numpy().view(np.int32), W.token_weights(adv.cpu().numpy(), c["cand"], t_major).view(np.int32))
            dead = ~np.isfinite(c["G"][:, :S]).reshape(-1)
            assert not adv.cpu().numpy()[dead].any() and not wgt.cpu().numpy()[dead].any()
            for x in (adv, wgt, est):
                assert bool(torch.isfinite(x).all())
            outs[t_major] = got
            for k, v in rel_errors(got, ref).items():
                worst[(k, normalize)] = max(worst.get((k, normalize), 0.0), v)
        for a_, b_ in zip(outs[False][:3], outs[True][:3]):           # the layout changes where w goes and nothing else
            assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
        if normalize:
            live_clips = ref["n_live"] > 0
            s = outs[False][1].cpu().double().numpy().reshape(B, S).sum(1)
            assert np.abs(s[live_clips] - 1).max(initial=0) <= 2e-6 and not s[~live_clips].any()
    print(f"[wor block] B={B} S={S} T={T}: max relative error " +
          ", ".join(f"{k} {'norm' if n else 'raw'} {v:.3e}" for (k, n), v in sorted(worst.items())) + f"  (bound {REL_TOL:.2e})")
    assert max(worst.values()) <= REL_TOL, worst


def test_root_key_is_the_host_hash_s(dev):
    """The block has no output for a; it shows through the weights.  kt = 0 gives lambda = log a, and with logq = -60 (x tiny) the
    unnormalised weight is exp(-lambda) = 1 / a.  Over 70 clips, for state words with a non-zero high seed word and a large call,
    wgt * a_host = 1 within the rounding of that chain: a - 1 rounds to 2^-25 max(a, 1) (absolute), which log1p(a - 1) = log a turns
    into 2^-25 max(a, 1) / a; phi + lambda with |phi| = 60 rounds to 60 * 2^-24 = 3.6e-6, twice; log1pf and expf add 2^-22 (|log a| + 1)."""
    from cvc import hip
    B, S, T = 70, 2, 1
    for seed, call in ((3, 1), ((0x9E3779B9 << 32) | 0x7F4A7C15, 123456789)):
        lo, hi = SO.seed_words(seed)
        h = W.root_hash(lo, hi, call, B)
        a = W.root_exponential(h)
        assert len(set(h.tolist())) == B
        logq = torch.full((B, S + 1), -60.0)
        G = torch.full((B, S + 1), -1.0)
        G[:, S] = 0.0
        adv, wgt, est, w = hip.scst_weights_wor(torch.ones(B * S).to(dev), logq.to(dev), G.to(dev), state_words(seed, call).to(dev), S,
                                                torch.zeros(B * S, T, dtype=torch.int64, device=dev), normalize=False)
        got = wgt.cpu().double().numpy().reshape(B, S)
        tol = 2.0 ** -25 * np.maximum(a, 1) / a + 2 * 60 * 2.0 ** -24 + 2.0 ** -22 * (np.abs(np.log(a)) + 1)
        err = np.abs(got * a[:, None] - 1)
        print(f"[wor a] seed {seed:#x} call {call}: a in [{a.min():.3e}, {a.max():.3f}], max |wgt a - 1| / tol = {(err / tol[:, None]).max():.3f}")
        assert (err <= tol[:, None]).all()
        # another call, another site or another counter would give other weights: the neighbours are far outside the tolerance
        other = W.root_exponential(W.root_hash(lo, hi, call + 1, B))
        assert (np.abs(got[:, 0] * other - 1) > tol).mean() > 0.9


def test_two_launches_agree_and_a_clip_does_not_see_the_others(dev):
    c = block_case(5, 5, 9)
    for normalize in (True, False):
        first, second = launch(c, dev, False, normalize), launch(c, dev, False, normalize)
        for a_, b_ in zip(first, second):
            assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
        o = block_case(5, 5, 20)                                   # other clips around clip 2 (same index: a is hashed from it)
        mixed = {k: c[k].copy() if isinstance(c[k], np.ndarray) else c[k] for k in c}
        for k in ("reward", "logq", "G"):
            keep = mixed[k].reshape(5, -1)[2].copy()
            mixed[k] = o[k].copy()
            mixed[k].reshape(5, -1)[2] = keep
        mixed["cand"] = np.ascontiguousarray(o["cand"][:, :9])
        mixed["cand"][10:15] = c["cand"][10:15]
        third = launch(mixed, dev, False, normalize)
        for a_, b_ in zip(first, third):
            a_, b_ = a_.view(torch.int32), b_.view(torch.int32)
            if a_.numel() == 5:
                assert torch.equal(a_[2], b_[2])
            else:
                assert torch.equal(a_[10:15], b_[10:15])
        assert not torch.equal(first[0], third[0])


def test_refusals_leave_the_outputs_untouched(dev):
    from cvc import hip
    from attn_step_cases import nan_buf, all_nan
    B, S, T = 2, 3, 4
    reward, logq, G = torch.zeros(B * S, device=dev), torch.zeros(B, S + 1, device=dev), torch.zeros(B, S + 1, device=dev)
    state, cand = state_words(1, 1).to(dev), torch.zeros(B * S, T, dtype=torch.int64, device=dev)
    outs = [nan_buf(64, dev=dev) for _ in range(4)]
    p = lambda x: None if x is None else x.data_ptr()

    def call(reward=reward, logq=logq, G=G, state=state, rows=B * S, per=S, cand=cand, T=T, outs=outs):
        return hip.lib().cvc_scst_weights_wor(p(reward), p(logq), p(G), p(state), rows, per, p(cand), T, 0, 1, *(p(o) for o in outs),
                                              torch.cuda.current_stream().cuda_stream)
    for name in ("reward", "logq", "G", "state", "cand"):
        assert call(**{name: None}) == BADARG, name
    for k in range(4):
        assert call(outs=[None if j == k else o for j, o in enumerate(outs)]) == BADARG
    assert call(per=1) == BADARG and call(per=8, rows=16) == BADARG and call(rows=7) == BADARG and call(rows=0) == BADARG and call(T=0) == BADARG
    torch.cuda.synchronize()
    assert all(all_nan(o) for o in outs)
    with pytest.raises(RuntimeError, match="cvc_scst_weights_wor failed: bad argument"):
        hip.scst_weights_wor(torch.zeros(16, device=dev), torch.zeros(2, 9, device=dev), torch.zeros(2, 9, device=dev), state, 8,
                             torch.zeros(16, T, dtype=torch.int64, device=dev))
    assert call() == 0                                              # the same buffers are fine for the call that is not refused
    torch.cuda.synchronize()
    assert not torch.isnan(outs[0][:B * S]).any() and bool(torch.isnan(outs[0][B * S:]).all())


def test_replays_from_a_graph_and_follows_the_generator_state(dev):
    from cvc import hip
    c = block_case(5, 7, 9)
    t = lambda x: torch.from_numpy(x).to(dev)
    reward, logq, G, cand = t(c["reward"]), t(c["logq"]), t(c["G"]), t(c["cand"])
    state = state_words(c["seed"], c["call"]).to(dev)
    run = lambda: hip.scst_weights_wor(reward, logq, G, state, c["S"], cand, t_major=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                          # one kernel node: no parallel branches
        out = run()
    g.replay()
    eager = run()
    for a_, b_ in zip(out, eager):
        assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
    before = [x.clone() for x in out]
    hip._check(hip.lib().cvc_sample_advance(state.data_ptr(), hip._stream()), "cvc_sample_advance")
    g.replay()
    want = launch(c, dev, True, True, call=c["call"] + 1)            # a fresh launch on fresh state words with the next call
    for a_, b_ in zip(out, want):
        assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
    assert not torch.equal(out[1], before[1])
    assert max(rel_errors(out, reference(c, True, call=c["call"] + 1)).values()) <= REL_TOL


# ------------------------------------------------------------------ 2. the toy through the block
@pytest.mark.parametrize("name", list(W.TOY_CASES))
def test_toy_statistics_through_the_block(dev, name):
    """the reference's 50 000 toy clips (logq, G in fp32, rewards) through the device block, unnormalised: the two 4.5-standard-error
    checks of tests/test_scst_wor_cpu.py"""
    from cvc import hip
    c = W.toy_case(name)
    trials, S = c["hist"].shape[0], c["hist"].shape[1] - 1
    state = state_words(c["seed"], c["call"]).to(dev)
    cand = torch.zeros(trials * S, 1, dtype=torch.int64, device=dev)

    def on_device(fr, logq, G):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        adv, wgt, est, _w = hip.scst_weights_wor(t(fr).view(-1), t(logq), t(G), state, S, cand, normalize=False)
        return tuple(x.cpu().double().numpy().reshape(trials, -1) if x.numel() > trials else x.cpu().double().numpy() for x in (adv, wgt, est))
    est, gh = W.toy_statistics(c["hist"], c["logq"], c["G"], c["a"], c["seqs"], c["f"], c["h"], weights_fn=on_device)
    z = W.z_score(est, c["Ef"]), W.z_score(gh, c["cov"])
    print(f"[wor toy, device] {name}: sum wgt f {z[0]:+.2f}, sum adv h {z[1]:+.2f} standard errors off")
    assert abs(z[0]) <= Z_OK and abs(z[1]) <= Z_OK


# ------------------------------------------------------------------ 3. engine -> model -> trainer
def _wor_trainer(dev, S=3, lr=1e-4, seed=5, tau=1.0):
    import test_gpu_scst as TS
    d = TS._dims()
    o, model, tr = TS._trainer(dev, d, seed=seed, S=S, lr=lr)
    o.scst_wor = tr.scst_wor = True
    o.scst_temperature = tau
    f, b, batch = TS._batch(dev, d, seed)
    return d, o, model, tr, f, b, batch


def test_whole_step_without_replacement(dev):
    # (on this model every logq is near -25, far below the threshold -- at tau = 0.3 too --, so the weights come out equal and the
    # advantage is the leave-one-out one; weights that differ are the block tests' ground)
    d, o, model, tr, f, b, batch = _wor_trainer(dev, lr=1e-3)
    S = 3
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    res = tr.scst_step(batch)
    assert len(res) == 4 and all(x.is_cuda and x.dim() == 0 and bool(torch.isfinite(x)) for x in res) and model.training
    last = tr.last_scst
    seq, logq, G = last["seq"], last["logq"], last["G"]
    assert seq.shape == (d.B * S, d.T) and logq.shape == G.shape == (d.B, S + 1) and last["logprob"] is None
    assert not (seq == synth.UNK_IDX).any()
    # the rollouts of a clip are pairwise distinct, and they are the engine's slots 0 .. S-1 with the engine's logq, G and state
    for clip in seq.view(d.B, S, d.T).tolist():
        assert len({tuple(r) for r in clip}) == S
    draws = model.last_stochastic
    assert torch.equal(draws["seq"][:, :S].reshape(-1, d.T), seq) and draws["seq"].shape == (d.B, S + 1, d.T)
    for k in ("logq", "G", "state"):
        assert torch.equal(draws[k].view(torch.int32), last[k].view(torch.int32)), k
    assert bool((G[:, 1:] <= G[:, :-1]).all()) and bool((logq <= 0).all()) and bool(torch.isfinite(G).all())
    lo, hi = SO.seed_words(last["seed"])
    assert last["state"].cpu().numpy().view(np.uint32).tolist() == [lo, hi, 1, 0]
    assert float(last["distinct"]) == 1.0
    # the weights are the rule's, from what the step left behind
    a = W.root_exponential(W.root_hash(lo, hi, 1, d.B))
    ref = W.weights(last["reward"].cpu().double().numpy(), logq.cpu().double().numpy(), G.cpu().double().numpy(), a, normalize=True)
    err = rel_errors((last["adv"], last["wgt"], last["expected_reward"]), ref)
    print(f"[wor step] relative errors {err}, weights of clip 0 {last['wgt'][:S].tolist()}, logq of clip 0 {logq[0].tolist()}, largest "
          f"weight per clip {last['wgt'].view(d.B, S).max(1).values.tolist()}, loss {float(res[0]):.5f}")
    assert max(err.values()) <= REL_TOL
    assert float(res[1]) == float(last["reward"].mean()) and float(res[2]) == float(last["expected_reward"].mean())
    assert float(res[3]) == float(last["adv"].abs().mean()) and int((last["adv"] != 0).sum()) >= 5
    moved = sum(int(not torch.equal(v, sd0[k])) for k, v in model.state_dict().items()
                if k.startswith(("decoder_core.att_lstm", "decoder_core.lang_lstm", "embed", "logit")))
    assert moved >= 8, moved
    for k, v in model.state_dict().items():
        if k.startswith(("roi_feat_extractor", "localizer_core")):
            assert torch.equal(v, sd0[k]), k
    res2 = tr.scst_step(batch)                                      # the next step: another seed, other draws
    assert tr.last_scst["seed"] == last["seed"] + 1 and not torch.equal(tr.last_scst["G"], G) and bool(torch.isfinite(res2[0]))


def test_gradient_of_the_step_s_loss_vs_cpu_autograd(dev):
    """the gradient scst_step hands to the optimizer against CPU autograd of -sum w log p / sum mask over the oracle's decoder, w =
    last_scst's advantages on the mask; the tolerance of tests/test_gpu_scst.py's gradient comparison"""
    import test_gpu_scst as TS
    d, o, model, tr, f, b, batch = _wor_trainer(dev)
    kept = {}
    orig = model.scst_loss

    def tap(enc, *a_, **k):
        kept["enc"] = enc
        return orig(enc, *a_, **k)
    model.scst_loss = tap
    tr._backward_and_update = lambda loss: (tr.optimizer.zero_grad(set_to_none=True), loss.backward(), kept.update(loss=loss.detach()))
    tr.scst_step(batch)
    last = tr.last_scst
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    f_np = {k: v.detach().cpu().numpy() for k, v in zip(("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "pnt_mask"),
                                                          kept["enc"])}
    P, loss_ref, _ = TS._oracle_grads(sd, f_np, last["seq"].cpu().numpy(), last["adv"].cpu().double().numpy(), d.T)
    assert float(kept["loss"]) == pytest.approx(loss_ref, rel=2e-5, abs=2e-6)
    checked = 0
    for n, p in model.named_parameters():
        if n.startswith(("roi_feat_extractor", "localizer_core")):
            assert p.grad is None or not p.grad.any(), n
            continue
        if n not in P or P[n].grad is None:
            assert p.grad is None or not p.grad.any(), n
            continue
        want = P[n].grad.double()
        err = float((p.grad.cpu().double() - want).norm())
        print(f"[wor grad] {n}: |err| {err:.3e}, |want| {float(want.norm()):.3e}")
        assert err <= 5e-4 * float(want.norm()) + 1e-6, (n, err, float(want.norm()))
        checked += 1
    assert checked >= 12, checked


def test_one_step_lowers_the_surrogate(dev):
    import test_gpu_scst as TS
    d, o, model, tr, f, b, batch = _wor_trainer(dev, lr=1e-4)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    tr.scst_step(batch)
    seq, adv = tr.last_scst["seq"], tr.last_scst["adv"]
    assert int((adv != 0).sum()) >= 5, adv
    after = TS._surrogate(model, f, b, seq, adv)
    model.load_state_dict(sd0)
    model.invalidate_decode_cache()
    before = TS._surrogate(model, f, b, seq, adv)
    print(f"[wor direction] surrogate before {before:.6f}, after {after:.6f}")
    assert after < before


def test_switched_off_the_step_is_the_one_it_was(dev, monkeypatch):
    """opts without scst_wor, and with scst_wor = False: the same step bit for bit, the with-replacement launches (cvc_scst_weights;
    the new block is never reached) and last_scst with the keys it had"""
    import test_gpu_scst as TS
    from cvc import hip
    d = TS._dims()

    def boom(*a_, **k):
        raise AssertionError("cvc_scst_weights_wor reached with scst_wor off")
    monkeypatch.setattr(hip, "scst_weights_wor", boom)
    runs = []
    for flag in (None, False):
        o, model, tr = TS._trainer(dev, d, seed=5, S=3, lr=1e-3)
        assert not hasattr(o, "scst_wor") and tr.scst_wor is False           # (the flag is cvc.main's: cvc.opts does not know it)
        if flag is not None:
            from cvc.trainer import Trainer
            o.scst_wor = flag
            cider = tr._cider
            tr = Trainer(o, None, model, tr.optimizer, None, None)
            tr._cider = cider
            assert tr.scst_wor is False
        _f, _b, batch = TS._batch(dev, d, 5)
        res = tr.scst_step(batch)
        runs.append((res, tr.last_scst, {k: v.clone() for k, v in model.state_dict().items()}))
        assert set(tr.last_scst) == {"seq", "logprob", "reward", "base", "greedy", "adv", "seed"}
        last = tr.last_scst
        assert last["seq"].shape == (d.B * 3, d.T) and last["logprob"].shape == (d.B * 3, d.T)
        adv, _w = hip.scst_weights(last["reward"], None, 3, last["seq"])
        assert torch.equal(adv.view(torch.int32), last["adv"].view(torch.int32))
        assert not hasattr(model, "last_wor")
    (r0, l0, s0), (r1, l1, s1) = runs
    for x, y in zip(r0, r1):
        assert torch.equal(x, y)
    for k in ("seq", "logprob", "reward", "adv"):
        assert torch.equal(l0[k], l1[k]), k
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def test_main_entry_point_takes_self_critical_epochs_without_replacement(tmp_path):
    from cvc import main as cvc_main
    rc = cvc_main.main(["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "12", "--num_prop_per_frm", "7",
                        "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "4",
                        "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "1", "--exp_name", "s", "--learning_rate", "0.001",
                        "--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/", "--id", "s1",
                        "--scst_after", "0", "--scst_wor", "--scst_samples", "3", "--scst_temperature", "1.0", "--scst_seed", "2"])
    assert rc == 0
    tr = cvc_main.LAST_TRAINER
    assert tr.scst_wor and tr._scst_steps == 2                              # 12 clips / 4 per batch, the last batch dropped
    last = tr.last_scst
    assert last["seq"].shape == (12, 4) and last["G"].shape == (4, 4) and last["wgt"].shape == (12,) and last["expected_reward"].shape == (4,)
    assert list(tr.reward_history) == [0] and all(np.isfinite(r) and r >= 0 for r in tr.reward_history[0])
    live = torch.isfinite(last["G"][:, :3])
    for clip, lv in zip(last["seq"].view(4, 3, 4).tolist(), live.tolist()):
        rows = [tuple(r) for r, l in zip(clip, lv) if l]
        assert len(set(rows)) == len(rows)
    with pytest.raises(SystemExit):
        cvc_main.main(["--no_cfg", "--scst_after", "0", "--scst_wor", "--scst_samples", "1"])
