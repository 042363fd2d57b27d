"""Scheduled sampling on the GPU (pytest -m gpu): the mixed selection block (csrc/mix.hip) against the sampler, the forced block and
the host coin (tests/mix_ref.py); the engine's mixed mode against the sampling and the forced engines, eagerly and as a graph;
DecodeWeights.refresh() against a fresh binding; the training forward on mixed inputs against CPU autograd; the trainer's step and the
command line.  Equalities are bit for bit unless a tolerance is named.  Tiny config of tests/test_gpu_scst.py: B = 5, R = 64, A = 32,
E = 32, V = 97, T = 6."""
import dataclasses
import os
import pickle

import numpy as np
import pytest
import torch

from cvc import synth
import mix_ref as MR
import sample_oracle as S

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
GRAD_TOL = (5e-4, 1e-6)       # tests/test_gpu_train.py, the gradient comparison: |err| <= 5e-4 |want| + 1e-6 (norms, fp64)
LOSS_TOL = dict(rel=2e-5, abs=2e-6)   # ... and its loss comparison
ENC = ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "pnt_mask")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def bits(x):
    return x.view(torch.int32) if x.is_floating_point() else x


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a.contiguous()), bits(b.contiguous()))


def state_words(seed, call):
    lo, hi = S.seed_words(seed)
    return torch.from_numpy(np.array([lo, hi, call, 0], dtype=np.uint32).view(np.int32))


# ------------------------------------------------------------------ the block against the sampler, the forced block and the host coin
def _sample_block(parts, bias, V, inv_tau, state, t):
    from cvc import hip
    nparts, M = parts.shape[0], parts.shape[1]
    word = torch.full((M,), -7, dtype=torch.int64, device=parts.device)
    lp = torch.full((M,), float("nan"), device=parts.device)
    hip._check(hip.lib().cvc_sample_select_parts(parts.data_ptr(), nparts, M * V, None if bias is None else bias.data_ptr(), M, V, UNK,
                                                 inv_tau, state.data_ptr(), t, word.data_ptr(), 1, lp.data_ptr(), hip._stream()),
               "cvc_sample_select_parts")
    return word, lp


def _forced_block(parts, bias, V, words):
    from cvc import hip
    nparts, M = parts.shape[0], parts.shape[1]
    lp = torch.full((M,), 123.0, device=parts.device)
    hip._check(hip.lib().cvc_forced_select_parts(parts.data_ptr(), nparts, M * V, None if bias is None else bias.data_ptr(), M, V,
                                                 words.data_ptr(), 1, lp.data_ptr(), None, hip._stream()), "cvc_forced_select_parts")
    return lp


def _mixed_block(parts, bias, V, inv_tau, state, t, given, p):
    """-> word, logprob, drawn, took, given_logprob (outputs pre-filled with values no launch writes)"""
    from cvc import hip
    nparts, M = parts.shape[0], parts.shape[1]
    dev = parts.device
    word = torch.full((M,), -7, dtype=torch.int64, device=dev)
    drawn = torch.full((M,), -7, dtype=torch.int64, device=dev)
    took = torch.full((M,), 9, dtype=torch.uint8, device=dev)
    lp, glp = torch.full((M,), 123.0, device=dev), torch.full((M,), 123.0, device=dev)
    prob = torch.tensor([p], dtype=torch.float32, device=dev)
    rc = hip.lib().cvc_mixed_select_parts(parts.data_ptr(), nparts, M * V, None if bias is None else bias.data_ptr(), M, V, UNK, inv_tau,
                                          state.data_ptr(), t, word.data_ptr(), 1, lp.data_ptr(), given.data_ptr(), 1, prob.data_ptr(),
                                          drawn.data_ptr(), took.data_ptr(), glp.data_ptr(), hip._stream())
    hip._check(rc, "cvc_mixed_select_parts")
    return word, lp, drawn, took, glp


# (3, 5, 1), (4, 97, 2), (3, 1028, 3) and one V per remaining loader form of select_dispatch (csrc/select_row.h).  float4 groups
# (V % 4 == 0): NG 1 / 2 / 4 / 5 / 8 at V <= 1024 / 2048 / 4096 / 5120 / 8192, with the unrolled slab counts 1, 2, 4, 6, 8 and the
# run-time one (3); scalar: NC 1 / 2 / 4 / 8 / 16 / 20 / 32 at V <= 256 / 512 / 1024 / 2048 / 4096 / 5120 / 8192
BLOCK_CASES = [(3, 5, 1), (4, 97, 2), (3, 1028, 3),
               (5, 100, 1), (4, 2052, 2), (4, 4100, 4), (4, 5124, 6), (4, 8192, 8),
               (4, 257, 1), (4, 513, 2), (4, 1025, 3), (4, 2049, 1), (4, 4097, 2), (4, 5121, 1), (4, 8191, 1)]


@pytest.mark.parametrize("M,V,nparts", BLOCK_CASES)
def test_block_vs_sampler_forced_block_and_host_coin(dev, M, V, nparts):
    seed, call, t, tau = 1000 + V, 2, 3, 0.8
    inv_tau = float(np.float32(1.0 / tau))
    g = torch.Generator().manual_seed(V * 7 + M)
    parts = (torch.randn(nparts, M, V, generator=g) * (1.5 / np.sqrt(nparts))).to(dev)
    bias = (torch.randn(V, generator=g) * 0.3).to(dev) if nparts > 1 else None
    state = state_words(seed, call).to(dev)
    w_s, lp_s = _sample_block(parts, bias, V, inv_tau, state, t)
    special = [0, UNK, V - 1, V + 3, -2]                     # given words: 0, UNK, the last id, one id >= V (and a negative one)
    for k, p in enumerate((0.0, 0.5, 1.0)):
        # every p sees the special values at other rows (M = 3: over the three p, each value at least once)
        given_l = [special[(r + 2 * k) % 4] for r in range(M)]
        if M >= 5:
            given_l[4] = special[4]
        given = torch.tensor(given_l, dtype=torch.int64, device=dev)
        in_range = (given >= 0) & (given < V)
        g0 = torch.where(in_range, given, torch.zeros_like(given))
        word, lp, drawn, took, glp = _mixed_block(parts, bias, V, inv_tau, state, t, given, p)
        assert same(drawn, w_s) and same(lp, lp_s), (p, drawn, w_s)
        want_took = torch.from_numpy(MR.took(seed, call, t, M, p)).to(dev)
        assert torch.equal(took.bool(), want_took) and int(took.max()) <= 1, (p, took)
        assert torch.equal(word, torch.where(want_took, drawn, g0)), (p, word)
        lp_f = _forced_block(parts, bias, V, g0)
        assert same(glp[in_range], lp_f[in_range]), (p, glp, lp_f)
        assert bool(torch.isnan(glp[~in_range]).all())
    covered = {special[(r + 2 * k) % 4] for r in range(M) for k in range(3)}
    assert covered == set(special[:4])
    # nullable outputs: the word alone
    from cvc import hip
    word2 = torch.full((M,), -7, dtype=torch.int64, device=dev)
    prob = torch.tensor([0.5], device=dev)
    hip._check(hip.lib().cvc_mixed_select_parts(parts.data_ptr(), nparts, M * V, None if bias is None else bias.data_ptr(), M, V, UNK,
                                                inv_tau, state.data_ptr(), t, word2.data_ptr(), 1, None, given.data_ptr(), 1,
                                                prob.data_ptr(), None, None, None, hip._stream()), "cvc_mixed_select_parts")
    want = torch.where(torch.from_numpy(MR.took(seed, call, t, M, 0.5)).to(dev), w_s, g0)
    assert torch.equal(word2, want)


def test_block_refuses_bad_arguments_without_a_launch(dev):
    import ctypes
    from cvc import hip
    fn = hip.lib().cvc_mixed_select_parts
    fake = ctypes.c_void_p(16)
    ok = dict(parts=fake, nparts=1, stride=0, M=4, V=50, inv_tau=1.0, state=fake, t=0, word=fake, wstride=1, given=fake, gstride=1,
              prob=fake)

    def call(**kw):
        a = {**ok, **kw}
        return fn(a["parts"], a["nparts"], a["stride"], None, a["M"], a["V"], UNK, a["inv_tau"], a["state"], a["t"], a["word"],
                  a["wstride"], None, a["given"], a["gstride"], a["prob"], None, None, None, None)

    for kw in (dict(parts=None), dict(state=None), dict(word=None), dict(t=-1), dict(inv_tau=0.0), dict(inv_tau=float("inf")),
               dict(nparts=0), dict(M=0), dict(V=1), dict(wstride=0), dict(nparts=2, stride=10), dict(given=None), dict(gstride=0),
               dict(prob=None)):
        assert call(**kw) == -1, kw                          # CVC_E_BADARG
    assert call(V=9000) == -2                                # CVC_E_TOOBIG
    torch.cuda.synchronize()                                 # nothing was launched on the fake pointers: the device is still fine


# ------------------------------------------------------------------ the engine
def _dims(**over):
    return dataclasses.replace(synth.CONFIGS["tiny"], **{**dict(B=5, R=64, A=32, E=32, V=97, T=6), **over})


_SHARED = {}


def _bound(dev, B):
    """weights and features of the tiny config at B clips, built once and left unchanged"""
    from helpers import to_dev
    from cvc.decode import DecodeWeights
    if B not in _SHARED:
        d = _dims(B=B)
        _SHARED[B] = (d, DecodeWeights(to_dev(synth.hot_path_state_dict(d, 31), dev)), to_dev(synth.clip_features(d, 31), dev))
    return _SHARED[B]


def _captions(d, n, seed, dev):
    """[B * n, T] given words in [0, V): 0, UNK and V - 1 among them"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(0, d.V, (d.B * n, d.T), generator=g)
    w[0, 0], w[1, 1], w[2, 2] = 0, UNK, d.V - 1
    return w.to(dev)


ENGINE_CASES = [(5, 1, "packed"), (33, 2, "tile")]           # 5 rows on the packed path; 66 rows = 33 clips x 2 on the tile path


@pytest.mark.parametrize("B,n,path", ENGINE_CASES)
def test_engine_p1_is_the_sampling_engine_eagerly_and_replayed(dev, B, n, path):
    from cvc.decode import DecodeEngine
    d, W, f = _bound(dev, B)
    tau, seed = 0.9, 17
    ref = DecodeEngine(W, f, d.T, UNK, sample_n=n, temperature=tau, seed=seed)
    mix = DecodeEngine(W, f, d.T, UNK, sample_n=n, temperature=tau, seed=seed, mix=True)
    assert (mix.packed, mix.tile) == (path == "packed", path == "tile") and mix._plan is None and mix.rows == B * n
    mix.load_captions(_captions(d, n, 3, dev)).set_mix_prob(1.0)
    want = [[x.clone() for x in ref.run()] for _ in range(3)]
    got = [[x.clone() for x in mix.run()]]                                      # eager: call = 1
    mix.capture()
    got += [[x.clone() for x in mix.run()] for _ in range(2)]                   # two replays: call = 2, 3
    assert int(mix.rng[2]) == 3
    for k in range(3):
        for a, b in zip(got[k], want[k]):
            assert same(a, b), (k, path)
    assert bool(mix.took.bool().all()) and same(mix.drawn.t(), got[2][0])
    assert not same(got[0][0], got[1][0])


@pytest.mark.parametrize("B,n,path", ENGINE_CASES)
def test_engine_p0_is_the_forced_engine(dev, B, n, path):
    from cvc.decode import DecodeEngine
    d, W, f = _bound(dev, B)
    cap = _captions(d, n, 4, dev)
    mix = DecodeEngine(W, f, d.T, UNK, sample_n=n, temperature=1.0, seed=5, mix=True).load_captions(cap)
    assert float(mix.mix_prob) == 0.0                                           # 0 until set
    forced = DecodeEngine(W, f, d.T, UNK, forced_n=n).load_captions(cap)
    assert (forced.packed, forced.tile) == (mix.packed, mix.tile)
    inputs_next, att, _lp = mix.run()
    _seq, att_f, lp_f, _rank = forced.run()
    assert same(inputs_next, cap) and not bool(mix.took.any())
    assert same(att, att_f) and same(mix.given_logprob.t(), lp_f)


@pytest.mark.parametrize("B,n,path", ENGINE_CASES)
def test_engine_p_half_mixes_and_the_forced_engine_reproduces_it(dev, B, n, path):
    from cvc.decode import DecodeEngine
    d, W, f = _bound(dev, B)
    cap = _captions(d, n, 6, dev)
    seed = 23
    mix = DecodeEngine(W, f, d.T, UNK, sample_n=n, temperature=1.0, seed=seed, mix=True).load_captions(cap).set_mix_prob(0.5)
    inputs_next, att, lp = (x.clone() for x in mix.run())
    took = mix.took.t().bool()
    assert torch.equal(took, torch.from_numpy(MR.took_steps(seed, 1, d.T, B * n, 0.5)).to(dev))
    assert bool(took.any()) and not bool(took.all())
    assert torch.equal(inputs_next, torch.where(took, mix.drawn.t(), cap))
    forced = DecodeEngine(W, f, d.T, UNK, forced_n=n).load_captions(inputs_next.contiguous())
    _seq, att_f, lp_f, _rank = forced.run()
    assert same(att, att_f)
    assert same(lp[took], lp_f[took])
    assert same(mix.given_logprob.t()[~took], lp_f[~took])                       # ... and the given words' at the others


def test_engine_probability_changes_between_replays_of_one_graph(dev):
    from cvc.decode import DecodeEngine
    d, W, f = _bound(dev, 5)
    seed = 41
    mix = DecodeEngine(W, f, d.T, UNK, temperature=1.0, seed=seed, mix=True).load_captions(_captions(d, 1, 8, dev)).capture()
    for call, p in enumerate((0.0, 1.0, 0.5, 0.125), start=1):
        mix.set_mix_prob(p)
        mix.run()
        assert int(mix.rng[2]) == call
        assert torch.equal(mix.took.t().bool(), torch.from_numpy(MR.took_steps(seed, call, d.T, 5, p)).to(dev)), p
    for p in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="0, 1"):
            mix.set_mix_prob(p)


def test_engine_refuses_every_excluded_combination(dev):
    from cvc.decode import DecodeEngine
    d, W, f = _bound(dev, 5)
    new = lambda **kw: DecodeEngine(W, f, d.T, UNK, mix=True, **kw)
    for kw in (dict(), dict(temperature=1.0, beam=3), dict(temperature=1.0, forced_n=1), dict(temperature=1.0, no_repeat_ngram=2),
               dict(temperature=1.0, no_immediate_repeat=True), dict(temperature=1.0, min_len=2), dict(temperature=1.0, ban_words=[3]),
               dict(temperature=1.0, bad_endings=[3]), dict(temperature=1.0, top_k=5), dict(temperature=1.0, top_p=0.9),
               dict(temperature=1.0, weights_dtype="bf16")):
        with pytest.raises(RuntimeError):
            new(**kw)
    plain = DecodeEngine(W, f, d.T, UNK, temperature=1.0)
    with pytest.raises(RuntimeError):
        plain.set_mix_prob(0.5)
    with pytest.raises(RuntimeError):
        plain.load_captions(_captions(d, 1, 1, dev))
    with pytest.raises(RuntimeError):
        new(temperature=1.0).load_captions(_captions(d, 1, 1, dev)[:, :3])


# ------------------------------------------------------------------ DecodeWeights.refresh()
@pytest.mark.parametrize("path,mixed", [("packed", False), ("tile", False), ("packed", True), ("tile", True)])
def test_refresh_serves_an_old_graph_after_an_in_place_update(dev, path, mixed):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d = _dims()
    sd = to_dev(synth.hot_path_state_dict(d, 12), dev)
    f = to_dev(synth.clip_features(d, 12), dev)
    kw = dict(temperature=1.0, seed=3, mix=True) if mixed else {}
    if path == "tile":
        kw["path"] = "tile"
    cap = _captions(d, 1, 2, dev)

    def ready(e):
        return e.load_captions(cap).set_mix_prob(0.5) if mixed else e

    W = DecodeWeights(sd)
    old = ready(DecodeEngine(W, f, d.T, UNK, **kw)).capture()
    assert (old.packed, old.tile) == (path == "packed", path == "tile")
    before = [x.clone() for x in old.run()]
    g = torch.Generator(device=dev).manual_seed(5)
    for k, v in sd.items():                                  # every parameter, in place
        if v.is_floating_point():
            v.add_(0.05 * torch.randn(v.shape, generator=g, device=dev) * (v.abs().mean() + 0.01))
    assert W.refresh() is W
    old.weights_refreshed()
    if mixed:
        old.seed(3)
    got = [x.clone() for x in old.run()]
    fresh = ready(DecodeEngine(DecodeWeights(sd), f, d.T, UNK, **kw))
    want = fresh.run()
    for a, b in zip(got, want):
        assert same(a, b), path
    assert not same(got[1], before[1])                       # the update was seen


# ------------------------------------------------------------------ the model: the training forward on mixed inputs
def _setup_model(dev, d, seed, end_marks=(), **over):
    """end_marks: (row, length) pairs -- that row's ground-truth caption ends after `length` words (zeros from there on)"""
    from helpers import build_model, to_dev
    sd = synth.hot_path_state_dict(d, seed)
    f_np, b_np = synth.clip_features(d, seed), synth.label_glue_batch(d, seed)
    for r, n in end_marks:
        b_np["gt_seq"][r, :, n:] = 0
    return sd, f_np, b_np, build_model(d, sd, dev, **over), to_dev(f_np, dev), to_dev(b_np, dev)


def _call(model, f, b, **kw):
    dummy = torch.zeros(f["fc_feats"].shape[0], 1, 1, device=f["fc_feats"].device)
    return model(f, b["input_seq"], b["gt_seq"], b["num"], b["proposals"], b["gt_bboxs"], b["box_mask"], dummy, b["frm_mask"],
                 b["sample_idx"], f["pnt_mask"], False, **kw)


def _gt_inputs(b, T):
    gt = b["gt_seq"][:, 0, :T]
    return torch.cat((gt.new_zeros(gt.size(0), 1), gt[:, :T - 1]), 1).contiguous()


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("decoder_only", [True, False])
def test_forward_on_the_gt_inputs_is_the_teacher_forced_forward(dev, decoder_only):
    """ss_inputs = the ground truth's inputs: the losses of forward() without the keyword, bit for bit, and the same gradients.
    train_decoder_only (the pass that returns exactly four losses; no loop C): every gradient bit for bit.  The cyclical pass (five
    losses): bit for bit too, except the embedding table -- without the keyword the eval-mode pass embeds the ground truth ONCE for
    loops A and C (autograd sums the two loops' gradients, then one scatter), with it loop C embeds on its own (two scatters, then
    the sum): the same terms added in another order, so that one tensor is held to the gradient tolerance of
    tests/test_gpu_train.py instead."""
    d = _dims()
    _sd, _f, _b, model, f, b = _setup_model(dev, d, 21, train_decoder_only=decoder_only)
    out0 = _call(model, f, b)
    sum(x.sum() for x in out0).backward()
    g0 = _grads(model)
    model.zero_grad(set_to_none=True)
    out1 = _call(model, f, b, ss_inputs=_gt_inputs(b, d.T))
    sum(x.sum() for x in out1).backward()
    g1 = _grads(model)
    assert len(out0) == len(out1) == (4 if decoder_only else 5)
    for a, c in zip(out0, out1):
        assert same(a.detach(), c.detach())
    assert set(g0) == set(g1) and len(g0) >= 12
    for n in g0:
        if n == "embed.0.weight" and not decoder_only:
            err, ref = float((g1[n].double() - g0[n].double()).norm()), float(g0[n].double().norm())
            print(f"[ss gt-inputs] {n}: |diff| {err:.3e}, |grad| {ref:.3e}")
            assert err <= GRAD_TOL[0] * ref + GRAD_TOL[1]
        else:
            assert same(g0[n], g1[n]), n


def _ss_words(d, b_np, seed):
    """random mixed inputs [B, T]: row 0 all sampled, row 1 the ground truth's untouched, the others mixed position by position;
    sampled words behind a row's end mark included (column 0 stays BOS)"""
    rng = np.random.default_rng(seed)
    gt = b_np["gt_seq"][:, 0, :d.T]
    base = np.concatenate([np.zeros((d.B, 1), np.int64), gt[:, :d.T - 1]], 1)
    rnd = rng.integers(0, d.V, (d.B, d.T)).astype(np.int64)
    take = rng.random((d.B, d.T)) < 0.5
    take[0], take[1] = True, False
    take[2, 1:] = True                                       # (all sampled again, a row whose caption ends early among them)
    take[:, 0] = False
    out = np.where(take, rnd, base)
    ended = np.cumsum(gt == 0, 1) > 0                        # positions at or behind the end mark of the ground truth
    assert (take[:, 1:] & ended[:, :-1]).any(), "the inputs must hold sampled words behind an end mark"
    return out


def _oracle_lm(sd, f_np, b_np, inputs, d):
    """CPU autograd of the teacher-forced decoder step (oracle.ref_cpu) on `inputs`, scored against the ground truth's targets"""
    from oracle import ref_cpu as O
    P = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in O.to_torch(sd).items()}
    f = O.to_torch(f_np)
    target = torch.from_numpy(b_np["gt_seq"][:, 0, :d.T])
    words = torch.from_numpy(inputs)
    state = O.init_hidden(d.B, d.R)
    logps = []
    for t in range(d.T):
        out, state, _a, _fm, _c = O.decoder_step(P, O.embed(P, words[:, t]), f["fc_feats"], f["conv_feats"], f["p_conv_feats"],
                                                 f["pool_feats"], f["p_pool_feats"], f["pnt_mask"][:, 1:], state, None)
        logps.append(O.logits_logsoftmax(P, out))
    loss = O.language_criterion(torch.stack(logps, 1).view(d.B * d.T, -1), target)
    loss.backward()
    return P, float(loss.detach())


@pytest.mark.parametrize("branch", ["loops", "steps"])
def test_forward_on_mixed_inputs_vs_cpu_autograd(dev, branch):
    """lm_loss and the decoder's gradients of forward(ss_inputs = random mixed words) against CPU autograd of the oracle's
    teacher-forced step on those inputs with the ground truth's targets; tolerance: tests/test_gpu_train.py's gradient comparison.
    `loops`: the C-driven branch; `steps`: the per-step branch (what a pass with dictated dropout masks takes; eval mode uses none)."""
    import contextlib
    from cvc import dropout
    d = _dims()
    sd, f_np, b_np, model, f, b = _setup_model(dev, d, 33, end_marks=((2, 2), (3, 3), (4, 0)))
    inputs = _ss_words(d, b_np, 9)
    P, loss_ref = _oracle_lm(sd, f_np, b_np, inputs, d)
    assert model._loop_plan(d.B, f["fc_feats"]) is not None                     # the shape takes the C-driven loops ...
    ctx = dropout.injected(lambda site, shape: torch.ones(shape)) if branch == "steps" else contextlib.nullcontext()
    with ctx:
        assert (model._loop_plan(d.B, f["fc_feats"]) is None) == (branch == "steps")      # ... unless masks are dictated
        out = _call(model, f, b, ss_inputs=torch.from_numpy(inputs).to(dev))
        out[0].sum().backward()
    print(f"[ss mixed {branch}] lm_loss {float(out[0].detach()):.6f}, oracle {loss_ref:.6f}")
    assert float(out[0].detach()) == pytest.approx(loss_ref, **LOSS_TOL)
    checked = 0
    for n, p in model.named_parameters():
        if not n.startswith(("decoder_core.", "embed.", "logit.")):
            continue
        if n not in P or P[n].grad is None:                  # a parameter the language loss does not reach
            assert p.grad is None or not bool(p.grad.any()), n
            continue
        want = P[n].grad.double()
        err = float((p.grad.cpu().double() - want).norm())
        print(f"[ss mixed {branch}] {n}: |err| {err:.3e}, |want| {float(want.norm()):.3e}")
        assert err <= GRAD_TOL[0] * float(want.norm()) + GRAD_TOL[1], (n, err, float(want.norm()))
        checked += 1
    assert checked >= 12, checked
    # targets, grounder and loops B / C are the ground truth's: the other losses of the pass do not depend on loop A's inputs
    # beyond loop A itself (att2 / ground read its attention; the reconstruction reads its arg-max words)
    with torch.no_grad():
        bad = torch.from_numpy(inputs).to(dev)[:, :3]
        with pytest.raises(RuntimeError):
            _call(model, f, b, ss_inputs=bad)


# ------------------------------------------------------------------ the trainer
def _batch(dev, d, seed):
    from helpers import to_dev
    f = to_dev(synth.clip_features(d, seed), dev)
    b = to_dev(synth.label_glue_batch(d, seed), dev)
    batch = (f, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
             ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], f["pnt_mask"][:, 1:])
    return f, b, batch


def _trainer(dev, d, seed=5, lr=1e-3, ss_seed=7):
    from helpers import make_opts
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    from cvc import opts as cvc_opts
    o = cvc_opts.parse_opt([])
    for k, v in vars(make_opts(d)).items():
        setattr(o, k, v)
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, lr, d.B
    o.ss_temperature, o.ss_seed = 1.0, ss_seed
    model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed).items()}, strict=False)
    model = model.to(dev).train()
    return o, model, Trainer(o, None, model, build_optimizer(model, o), None, None)


def _reseed(n=3):
    from cvc import dropout
    dropout.seed(n)
    torch.manual_seed(n)


def test_trainer_without_scheduled_sampling_takes_the_old_step(dev):
    """ss_prob = 0: train_step is the parent's sequence -- forward, loss mix, update, invalidation -- with its five losses"""
    d = _dims()
    _o, model, tr = _trainer(dev, d)
    _f, _b, batch = _batch(dev, d, 5)
    model.ss_prob = 0.0
    _reseed()
    got = [x.clone() for x in tr.train_step(batch)]
    assert tr.last_ss is None and tr._ss_steps == 0 and model.ss_engine() is None
    _o2, model2, tr2 = _trainer(dev, d)
    _reseed()
    out = tr2._call(tr2._prepare(batch, True))
    want = tr2.loss_mix(out)
    tr2._backward_and_update(want[0])
    tr2._weights_changed()
    assert len(got) == 5
    for a, c in zip(got, want):
        assert same(a, c.detach()), (got, want)
    for (k, v), (k2, v2) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k


def test_trainer_scheduled_sampling_steps(dev):
    from cvc.decode import DecodeEngine, DecodeWeights
    d = _dims()
    ss_seed, p = 7, 0.25
    _o, model, tr = _trainer(dev, d, ss_seed=ss_seed)
    f, b, batch = _batch(dev, d, 5)
    model.ss_prob = p
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    _reseed()
    l1 = [x.clone() for x in tr.train_step(batch)]
    assert len(l1) == 5 and all(x.is_cuda and bool(torch.isfinite(x).all()) for x in l1)
    assert model.training and tr._ss_steps == 1
    moved = sum(int(not torch.equal(v, sd0[k])) for k, v in model.state_dict().items() if k.startswith(("decoder_core", "embed", "logit")))
    assert moved >= 8, moved
    last = tr.last_ss
    rows = d.B
    assert last["seed"] == ss_seed and last["took"].shape == (rows, d.T) and last["given_logprob"].shape == (rows, d.T)
    assert torch.equal(last["took"].bool(), torch.from_numpy(MR.took_steps(ss_seed, 1, d.T, rows, p)).to(dev))
    gt_in = _gt_inputs(b, d.T)
    took_in = torch.cat((torch.zeros(rows, 1, dtype=torch.bool, device=dev), last["took"].bool()[:, :d.T - 1]), 1)
    assert torch.equal(last["inputs"][~took_in], gt_in[~took_in]) and bool((last["inputs"][:, 0] == 0).all())
    assert float(last["share"]) == float(last["took"][:, :d.T - 1].float().mean())
    # ---- the engine survived the update: the second step's rollout is a rollout of a FRESH engine bound after the first update
    eng = model.ss_engine()
    assert eng is not None and model.decode_weights() is eng.W                   # the cached binding was kept, not rebuilt
    model.eval()
    with torch.no_grad():
        pb = tr._prepare(batch, True)                                            # (the batch as the step sees it: trimmed axes)
        enc = model.encode_clips(pb["segs_feat"], pb["ppls"], pb["num"], pb["mask_bboxs"], pb["ppls_feat"], pb["gt_bboxs"],
                                 pb["mask_frms"], pb["sample_idx"], pb["pnt_mask"])
        feats = {k: v.contiguous() for k, v in zip(ENC, enc)}
        fresh = DecodeEngine(DecodeWeights({k: v.clone() for k, v in model.state_dict().items()}), feats, d.T, UNK, temperature=1.0,
                             seed=ss_seed + 1, mix=True)
        fresh.load_captions(pb["gt_seqs"][:, 0, :d.T].contiguous()).set_mix_prob(p)
        nxt = fresh.run()[0]
        want_inputs = torch.cat((nxt.new_zeros(rows, 1), nxt[:, :d.T - 1]), 1)
        want_glp = fresh.given_logprob.t().clone()
    model.train()
    l2 = [x.clone() for x in tr.train_step(batch)]
    assert model.ss_engine() is eng and tr.last_ss["seed"] == ss_seed + 1
    assert torch.equal(tr.last_ss["inputs"], want_inputs) and same(tr.last_ss["given_logprob"], want_glp)
    assert torch.equal(tr.last_ss["took"].bool(), torch.from_numpy(MR.took_steps(ss_seed + 1, 1, d.T, rows, p)).to(dev))
    # ---- two trainers with equal seeds: equal losses over two steps
    _o2, model2, tr2 = _trainer(dev, d, ss_seed=ss_seed)
    model2.ss_prob = p
    _reseed()
    m1 = [x.clone() for x in tr2.train_step(batch)]
    m2 = [x.clone() for x in tr2.train_step(batch)]
    for a, c in zip(l1 + l2, m1 + m2):
        assert same(a, c), (l1, l2, m1, m2)


MAIN_ARGS = ["--no_cfg", "--batch_size", "4", "--synthetic_clips", "16", "--num_prop_per_frm", "7", "--t_attn_size", "5", "--rnn_size",
             "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "4", "--vis_encoding_size", "24",
             "--tensorboard", "0", "--disp_interval", "1", "--exp_name", "s", "--learning_rate", "0.001", "--id", "s1",
             "--scheduled_sampling_start", "0", "--scheduled_sampling_increase_prob", "0.25", "--scheduled_sampling_max_prob", "0.25"]


@pytest.mark.parametrize("extra,want", [(["--max_epochs", "1"], {0: 0.0}),
                                        (["--max_epochs", "2", "--scheduled_sampling_increase_every", "1"], {0: 0.0, 1: 0.25})])
def test_main_entry_point_runs_the_schedule(dev, tmp_path, capsys, extra, want):
    from cvc import main as cvc_main
    rc = cvc_main.main(MAIN_ARGS + ["--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/"] + extra)
    assert rc == 0
    hist = pickle.load(open(os.path.join(tmp_path, "s", "histories_s1.pkl"), "rb"))
    assert hist["ss_prob_history"] == want
    tr = cvc_main.LAST_TRAINER
    log = capsys.readouterr().out
    if 1 in want:
        assert tr._ss_steps == 3 and tr.last_ss["prob"] == 0.25                  # 16 clips / 4 per batch, the last batch dropped
        assert "Sampled" in log
    else:
        assert tr._ss_steps == 0 and tr.last_ss is None and "Sampled" not in log
