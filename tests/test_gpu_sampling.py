"""Sampled decoding on the GPU (pytest -m gpu): the selection block (csrc/sample.hip) against fp64, the engine's three paths against
the CPU reference sampler (tests/sample_oracle.py), graph replay and seeding, the sampled distribution, and the model / trainer
plumbing."""
import dataclasses

import numpy as np
import pytest
import torch

from cvc import synth
import sample_oracle as S

pytestmark = pytest.mark.gpu

SEQ_TOL = dict(rtol=1e-4, atol=1e-4)      # attention maps after T recurrent steps (the greedy tests' tolerance)
LOGPROB_TOL = 1e-4
SCORE_TIE_TOL = 2e-3                      # perturbed-score margins below this may flip between the GPU and the fp32 oracle


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def select_block(parts, bias, V, unk, inv_tau, state, t, logprob=True):
    from cvc import hip
    nparts, M = parts.shape[0], parts.shape[1]
    word = torch.full((M,), -7, dtype=torch.int64, device=parts.device)
    lp = torch.full((M,), float("nan"), device=parts.device) if logprob else None
    rc = hip.lib().cvc_sample_select_parts(parts.data_ptr(), nparts, M * V, None if bias is None else bias.data_ptr(), M, V, unk,
                                           inv_tau, state.data_ptr(), t, word.data_ptr(), 1, None if lp is None else lp.data_ptr(),
                                           hip._stream())
    hip._check(rc, "cvc_sample_select_parts")
    return word, lp


def state_words(seed, call):
    lo, hi = S.seed_words(seed)
    return torch.from_numpy(np.array([lo, hi, call, 0], dtype=np.uint32).view(np.int32))


# ------------------------------------------------------------------ the selection block against fp64
@pytest.mark.parametrize("M,V,nparts,with_bias", [(1, 50, 1, False), (64, 50, 4, True), (320, 50, 8, True), (1, 5000, 8, True),
                                                  (64, 5000, 1, False), (64, 5000, 4, True), (320, 5000, 8, True),
                                                  (320, 5000, 1, True), (64, 5000, 6, True)])
def test_sample_block_vs_fp64(dev, M, V, nparts, with_bias):
    unk, tau, seed, call, t = synth.UNK_IDX, 0.7, 12345 + M + V, 3, 5
    g = torch.Generator().manual_seed(M * 131 + V + nparts)
    parts = torch.randn(nparts, M, V, generator=g) * (1.5 / np.sqrt(nparts))
    bias = torch.randn(V, generator=g) * 0.3 if with_bias else None
    noise = S.gumbel_noise(seed, call, t, M, V)
    inv_tau = float(np.float32(1.0 / tau))

    def finished(p):                                    # the finishing pass's order: slab 0 + slab 1 + ... + bias, fp32
        z = p[0].clone()
        for k in range(1, nparts):
            z = z + p[k]
        return z + bias if bias is not None else z

    z = finished(parts)
    s = z.double().numpy() * inv_tau + noise
    s[:, unk] = -np.inf
    best = s.argmax(1)
    # planted cases: rows whose UNK has the best perturbed score; rows with a second word tied to the best in fp64 up to fp32 rounding
    for r in range(0, M, 3):
        parts[0, r, unk] += float((s[r].max() - noise[r, unk]) / inv_tau - z[r, unk]) + 2.0
    for r in range(1, M, 3):
        v2 = (int(best[r]) + 7) % V
        v2 = v2 if v2 != unk else (v2 + 1) % V
        parts[0, r, v2] += float((s[r, best[r]] - noise[r, v2]) / inv_tau - z[r, v2])
    z = finished(parts)
    s = z.double().numpy() * inv_tau + noise
    assert (s[0::3, unk] > np.delete(s[0::3], unk, axis=1).max(1)).all()        # the planted UNK leads ...
    s[:, unk] = -np.inf                                                             # ... and may never be chosen
    top2 = -np.partition(-s, 1, axis=1)[:, :2]
    gap = top2[:, 0] - top2[:, 1]
    zd = z.double().numpy()
    lse = zd.max(1) + np.log(np.exp(zd - zd.max(1, keepdims=True)).sum(1))

    pd_, bd = parts.contiguous().to(dev), None if bias is None else bias.to(dev)
    state = state_words(seed, call).to(dev)
    word, lp = select_block(pd_, bd, V, unk, inv_tau, state, t)
    w = word.cpu().numpy()
    assert ((w >= 0) & (w < V)).all() and not (w == unk).any()
    # the chosen word's fp64 perturbed score is within the stated tolerance of the maximum; clear rows agree exactly
    TOL = 1e-5 * (1.0 + np.abs(s[np.isfinite(s)]).max())
    assert (top2[:, 0] - s[np.arange(M), w] <= TOL).all(), np.max(top2[:, 0] - s[np.arange(M), w])
    clear = gap > TOL
    assert np.array_equal(w[clear], s.argmax(1)[clear])
    assert clear.sum() >= M - (M + 2) // 3
    np.testing.assert_allclose(lp.cpu().double().numpy(), zd[np.arange(M), w] - lse, rtol=0, atol=2e-6)
    # bitwise deterministic run to run; the finished-matrix form (nparts = 1, no bias) gives the same bits
    word2, lp2 = select_block(pd_, bd, V, unk, inv_tau, state, t)
    assert torch.equal(word, word2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))
    word3, lp3 = select_block(z.to(dev).unsqueeze(0).contiguous(), None, V, unk, inv_tau, state, t)
    assert torch.equal(word, word3) and torch.equal(lp.view(torch.int32), lp3.view(torch.int32))
    # the advance block moves `call` by one: other noise, other words
    from cvc import hip
    hip._check(hip.lib().cvc_sample_advance(state.data_ptr(), hip._stream()), "cvc_sample_advance")
    assert state.cpu().tolist()[2] == call + 1
    if M >= 64:
        word4, _ = select_block(pd_, bd, V, unk, inv_tau, state, t)
        assert not torch.equal(word, word4)


# ------------------------------------------------------------------ the engine against the reference sampler
def _inputs(name, B=None, seed=4321):
    from helpers import to_dev
    from oracle import ref_cpu as O
    d = synth.CONFIGS[name]
    if B is not None:
        d = dataclasses.replace(d, B=B)
    sd, f_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed)
    return d, sd, f_np, O.to_torch(sd), O.to_torch(f_np)


def _compare(seq, att, lp, ref, label):
    """Tie-aware: a row's words equal the oracle's until a step whose fp64 perturbed-score margin is below SCORE_TIE_TOL (then the
    rest of that row is not comparable); log-probs and attention compared over the comparable steps."""
    from helpers import tie_aware_seq_equal
    seq_o, att_o, lp_o, scores = ref
    seq, att, lp = seq.cpu().numpy(), att.cpu().numpy(), lp.cpu().numpy()
    stats = {}
    n_exact = tie_aware_seq_equal(seq, seq_o.numpy(), None, tol=SCORE_TIE_TOL, clear_gap=SCORE_TIE_TOL, gaps=S.score_gaps(scores),
                                  stats=stats)
    rows, T = seq.shape
    assert n_exact >= 0.9 * rows * T, (label, n_exact, stats)
    same = np.cumprod(seq == seq_o.numpy(), axis=1).astype(bool)                   # steps whose words (and all before) agree
    att_ok = np.concatenate([np.ones((rows, 1), bool), same[:, :-1]], 1)            # attention of step t depends on words < t
    assert np.abs(lp[same] - lp_o.numpy()[same]).max() <= LOGPROB_TOL, label
    np.testing.assert_allclose(att[att_ok], att_o.numpy()[att_ok], **SEQ_TOL)
    assert not (seq == synth.UNK_IDX).any()
    print(f"[sampling] {label}: {stats}")


@pytest.mark.parametrize("name,B,n,path", [("tiny", None, 1, "ring"), ("tiny", None, 3, "tile"), ("cfg1", None, 1, "packed"),
                                           ("cfg1", None, 5, "tile"), ("cfg2", None, 1, "packed"), ("cfg2", 16, 5, "tile")])
def test_engine_vs_oracle_sampler(dev, name, B, n, path):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = _inputs(name, B)
    tau, seed = 0.8, 77 + n
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, synth.UNK_IDX, sample_n=n, temperature=tau, seed=seed)
    assert (eng.packed, eng.tile) == (path == "packed", path == "tile") and eng._plan is None
    assert not hasattr(eng, "score") and not hasattr(eng, "parent")               # no beam buffers
    for call in (1, 2):                                                             # the k-th run after seed() draws with call = k
        seq, att, lp = eng.run()
        assert seq.shape == (d.B * n, d.T) and att.shape == (d.B * n, d.T, d.N) and lp.shape == (d.B * n, d.T)
        assert int(eng.rng[2]) == call
        with torch.no_grad():
            ref = S.sample(P, f, d.T, synth.UNK_IDX, n, tau, seed, call)
        _compare(seq, att, lp, ref, f"{name} n={n} {path} call {call}")
        if name != "tiny":
            break


def test_packed_and_tile_paths_agree(dev):
    from helpers import to_dev, tie_aware_seq_equal
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = _inputs("cfg1")
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    e_p = DecodeEngine(W, fd, d.T, synth.UNK_IDX, temperature=1.0, seed=5)
    e_t = DecodeEngine(W, fd, d.T, synth.UNK_IDX, temperature=1.0, seed=5, path="tile")
    assert e_p.packed and e_t.tile
    sp, ap, lpp = (x.clone() for x in e_p.run())
    st, at, lpt = (x.clone() for x in e_t.run())
    with torch.no_grad():
        ref = S.sample(P, f, d.T, synth.UNK_IDX, 1, 1.0, 5, 1)
    gaps = S.score_gaps(ref[3])
    assert tie_aware_seq_equal(sp.cpu().numpy(), st.cpu().numpy(), None, tol=SCORE_TIE_TOL, clear_gap=SCORE_TIE_TOL, gaps=gaps) == d.B * d.T
    np.testing.assert_allclose(lpp.cpu().numpy(), lpt.cpu().numpy(), rtol=0, atol=LOGPROB_TOL)
    np.testing.assert_allclose(ap.cpu().numpy(), at.cpu().numpy(), **SEQ_TOL)


@pytest.mark.parametrize("name,n", [("tiny", 3), ("cfg1", 1)])
def test_graph_replay_draws_fresh_noise_and_seed_reproduces(dev, name, n):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, _, _ = _inputs(name)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    g = DecodeEngine(W, fd, d.T, synth.UNK_IDX, sample_n=n, temperature=1.5, seed=9).capture()
    assert int(g.rng[2]) == 0                              # capture (and its warm-up decode) leaves `call` alone
    r1 = [x.clone() for x in g.run()]
    r2 = [x.clone() for x in g.run()]
    assert int(g.rng[2]) == 2 and not torch.equal(r1[0], r2[0])
    k = 3
    g.seed(21)
    for _ in range(k):
        rg = [x.clone() for x in g.run()]
    e = DecodeEngine(W, fd, d.T, synth.UNK_IDX, sample_n=n, temperature=1.5, seed=21)
    for _ in range(k):
        re_ = [x.clone() for x in e.run()]
    assert int(g.rng[2]) == k and int(e.rng[2]) == k
    for a, b in zip(rg, re_):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)


def test_one_step_distribution_on_the_gpu(dev):
    """Step 0 of the tile path at tiny: 64 samples per clip per decode, 50 decodes -> 3 200 draws per clip against
    softmax(z / tau) without UNK (fixed seed: deterministic)."""
    from helpers import to_dev
    from oracle import ref_cpu as O
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = _inputs("tiny")
    n, runs, tau = 64, 50, 1.3
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, synth.UNK_IDX, sample_n=n, temperature=tau, seed=2)
    eng.capture()
    first = torch.stack([eng.run()[0][:, 0].clone() for _ in range(runs)]).cpu().numpy()      # [runs, B*n]
    with torch.no_grad():
        out, _, _, _, _ = O.decoder_step(P, O.embed(P, torch.zeros(d.B, dtype=torch.long)), f["fc_feats"], f["conv_feats"],
                                         f["p_conv_feats"], f["pool_feats"], f["p_pool_feats"], f["pnt_mask"][:, 1:],
                                         O.init_hidden(d.B, d.R))
        z = torch.nn.functional.linear(out, P["logit.weight"], P["logit.bias"]).double()
    for b in range(d.B):
        counts = np.bincount(first[:, b * n:(b + 1) * n].ravel(), minlength=d.V)
        assert counts[synth.UNK_IDX] == 0
        p = torch.softmax(z[b] / tau, 0).numpy()
        p[synth.UNK_IDX] = 0.0
        p /= p.sum()
        stat, df = S.chi_square(counts, p)
        assert stat < S.chi_square_critical(df), (b, stat, df)


# ------------------------------------------------------------------ model and trainer
def _model_sample(model, feats, batch, **kw):
    B = feats["fc_feats"].shape[0]
    dummy = torch.zeros(B, 1, 1, device=feats["fc_feats"].device)
    return model._sample(feats, batch["input_seq"], batch["proposals"], batch["gt_seq"], batch["num"], batch["box_mask"],
                         batch["gt_bboxs"], dummy, batch["frm_mask"], batch["sample_idx"], feats["pnt_mask"], **kw)


@pytest.mark.parametrize("graph", [False, True])
def test_greedy_is_unchanged_by_a_sampling_engine(dev, graph):
    from helpers import build_model, to_dev, model_call
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=graph)
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, 99), dev)
    seq, att, none = model_call(model, f, b, True)
    assert none is None
    s1 = _model_sample(model, f, b, sample_max=0, temperature=0.9, sample_n=4, seed=3)
    assert s1[0].shape == (d.B * 4, d.T) and s1[2].shape == (d.B * 4, d.T) and not (s1[0] == synth.UNK_IDX).any()
    s2 = _model_sample(model, f, b, sample_max=0, temperature=0.9, sample_n=4, seed=3)      # cached engine: fresh noise
    assert not torch.equal(s1[0], s2[0])
    seq2, att2, none2 = model_call(model, f, b, True)
    assert none2 is None and torch.equal(seq, seq2) and torch.equal(att.view(torch.int32), att2.view(torch.int32))
    # the model's attributes are the defaults of _sample
    model.sample_max, model.sample_temperature, model.sample_n, model.sample_seed = 0, 0.9, 4, 3
    s3 = model_call(model, f, b, True)
    assert torch.equal(s3[0], s1[0]) and torch.equal(s3[2], s1[2])


def test_trainer_sample_writes_n_sentences_per_segment(dev, tmp_path):
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
    path = tr.sample(3, 0.8, seed=4)
    out = json.load(open(path))
    assert path.endswith("densecap-validation-s1_samples.json") and len(out) == 8
    for vid, segs in out.items():
        i = int(vid[len("v_synth"):])
        for e in segs:
            assert len(e["sentences"]) == 3 and len(e["logprobs"]) == 3 and all(lp <= 0 for lp in e["logprobs"])
            assert e["timestamp"] == [round(1.5 * i, 2), round(1.5 * i + 7.25, 2)]
    # the CLI: its own flags, the rest to cvc.main with the checkpoint loading of an inference-only run
    assert cvc_sample.main(common + ["--resume", "True", "--temperature", "0.8", "--sample_n", "2", "--sample_seed", "4"]) == 0
    out2 = json.load(open(path))
    assert len(out2) == 8 and all(len(e["sentences"]) == 2 for segs in out2.values() for e in segs)
