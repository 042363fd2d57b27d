"""Self-critical training step (Trainer.scst_step, model.scst_loss) on the tiny synthetic config of the bf16 tests
(B = 5, R = 64, A = 32, E = 32, V = 97, T = 6): the gradient pass against CPU autograd, its log-probs against the sampling engine's,
the step's direction, and what a whole step returns and leaves behind."""
import dataclasses

import numpy as np
import pytest
import torch

from cvc import synth
import cider_ref as R

pytestmark = pytest.mark.gpu

LOGPROB_TOL = 1e-4            # tests/test_gpu_forced.py: the forced decode's log-probs against the training pass's
FLOOR = 2.0 ** -20            # tests/test_gpu_cider.py


def _dims(**over):
    return dataclasses.replace(synth.CONFIGS["tiny"], **{**dict(B=5, R=64, A=32, E=32, V=97, T=6), **over})


def _batch(dev, d, seed):
    from helpers import to_dev
    f = to_dev(synth.clip_features(d, seed), dev)
    b = to_dev(synth.label_glue_batch(d, seed), dev)
    batch = (f, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
             ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], f["pnt_mask"][:, 1:])
    return f, b, batch


def _corpus(d, seed):
    """the batch's ground-truth captions plus other captions of the same law: the CIDEr-D table's training captions"""
    extra = dataclasses.replace(d, B=60)
    return list(synth.captions(d, seed)) + list(synth.captions(extra, seed + 1))


def _trainer(dev, d, seed=5, S=5, lr=1e-4, **over):
    from helpers import make_opts
    from cvc.cider import CiderD
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    from cvc import opts as cvc_opts
    o = cvc_opts.parse_opt([])
    for k, v in vars(make_opts(d, **over)).items():
        setattr(o, k, v)
    o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, lr, d.B
    o.scst_samples, o.scst_temperature, o.scst_seed, o.scst_dropout = S, 1.0, 1, False
    model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed).items()}, strict=False)
    model = model.to(dev).train()
    tr = Trainer(o, None, model, build_optimizer(model, o), None, None)
    tr._cider = CiderD.from_captions(_corpus(d, seed), dev)
    return o, model, tr


def _words(rng, rows, T, V):
    w = rng.integers(1, V, (rows, T)).astype(np.int64)
    for r in range(rows):
        L = int(rng.integers(1, T + 2))
        if L <= T:
            w[r, L - 1] = 0                      # the end mark; what follows it stays random and must not count
    w[0, 0] = 0
    return w


def _oracle_grads(sd, f_np, words, adv, T):
    """CPU autograd of -sum w log p / sum mask over oracle.ref_cpu's teacher-forced decoder step, dropout off"""
    from oracle import ref_cpu as O
    P = {k: v.clone().requires_grad_(v.dtype.is_floating_point) for k, v in O.to_torch(sd).items()}
    S = words.shape[0] // f_np["fc_feats"].shape[0]
    f = {k: v.repeat_interleave(S, 0) for k, v in O.to_torch(f_np).items()}
    rows = words.shape[0]
    wt = torch.from_numpy(words)
    state = O.init_hidden(rows, f["fc_feats"].size(1))
    word = torch.zeros(rows, dtype=torch.long)
    logps = []
    for t in range(T):
        out, state, _a, _fm, _c = O.decoder_step(P, O.embed(P, word), f["fc_feats"], f["conv_feats"], f["p_conv_feats"], f["pool_feats"],
                                                 f["p_pool_feats"], f["pnt_mask"][:, 1:], state, None)
        logps.append(O.logits_logsoftmax(P, out).gather(1, wt[:, t:t + 1])[:, 0])
        word = wt[:, t]
    logp = torch.stack(logps, 1)                                             # [rows, T]
    # the steps up to and including the first 0 (LMCriterion's mask of a caption that is 0 behind its end mark; the random words
    # behind the end mark here, like a rollout's, must not count -- and, the recurrence being causal, cannot reach the steps that do)
    mask = torch.from_numpy(R.text_mask(words)).to(logp.dtype)
    w = torch.from_numpy(adv).to(logp.dtype)[:, None] * mask
    loss = -(w * logp).sum() / mask.sum()
    loss.backward()
    return P, float(loss.detach()), logp.detach()


@pytest.mark.parametrize("B,V,S", [(5, 97, 5), (5, 97, 1), (14, 100, 5)])
def test_gradient_pass_vs_cpu_autograd(B, V, S):
    """fixed sampled words and fixed rewards (negative advantages and an all-zero clip among them) -> the decoder's gradients against
    CPU autograd, with the tolerance of tests/test_gpu_train.py's gradient comparison; (14, 100, 5): 70 rows = two groups of the
    C-driven loop and a vocabulary the fused head takes."""
    from helpers import build_model, to_dev
    dev = torch.device("cuda:0")
    d = _dims(B=B, V=V)
    seed = 40 + B + S
    sd, f_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed)
    rng = np.random.default_rng(seed)
    rows = B * S
    words = _words(rng, rows, d.T, V)
    reward = (rng.random(rows) * 10).astype(np.float32)
    base = None
    if S > 1:
        reward[S:2 * S] = 3.25                      # a clip whose samples all score alike: its advantages are exactly 0
    else:
        base = (rng.random(B) * 10).astype(np.float32)
        base[1] = reward[1]
    adv64, _ = R.advantages(reward, S, base)
    assert (adv64 < 0).any() and (adv64 > 0).any() and (adv64[S:2 * S] == 0).all()
    P, loss_ref, _ = _oracle_grads(sd, f_np, words, adv64, d.T)
    model = build_model(d, sd, dev)                  # eval(): dropout off
    f = to_dev(f_np, dev)
    enc = tuple(f[k] for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "pnt_mask"))
    loss, adv = model.scst_loss(enc, torch.from_numpy(words).to(dev), torch.from_numpy(reward).to(dev),
                                None if base is None else torch.from_numpy(base).to(dev), S)
    assert float(loss.detach()) == pytest.approx(loss_ref, rel=2e-5, abs=2e-6)
    np.testing.assert_allclose(adv.cpu().numpy(), adv64, rtol=0, atol=(S + 2) * 2.0 ** -24 * 10 * max(S, 2))
    loss.backward()
    checked = 0
    for n, p in model.named_parameters():
        if n.startswith(("roi_feat_extractor", "localizer_core")):
            assert p.grad is None, n                 # encoder, localizer: no gradient (the reconstructor shares the decoder's cells)
            continue
        if n not in P or P[n].grad is None:
            assert p.grad is None or not p.grad.any(), n
            continue
        want = P[n].grad.double()
        err = float((p.grad.cpu().double() - want).norm())
        print(f"[scst grad] {n}: |err| {err:.3e}, |want| {float(want.norm()):.3e}")
        assert err <= 5e-4 * float(want.norm()) + 1e-6, (n, err, float(want.norm()))
        checked += 1
    assert checked >= 12, checked


def _sample_args(f, b):
    B = f["fc_feats"].shape[0]
    dummy = torch.zeros(B, 1, 1, device=f["fc_feats"].device)
    return (f, b["input_seq"], b["proposals"], b["gt_seq"], b["num"], b["box_mask"], b["gt_bboxs"], dummy, b["frm_mask"], b["sample_idx"],
            f["pnt_mask"])


def test_gradient_pass_scores_the_policy_that_was_sampled():
    """the per-token log-probs of the gradient pass (vocabulary head on loop A's outputs) equal the sampling engine's logprob"""
    from helpers import build_model
    from cvc import functional as F_
    dev = torch.device("cuda:0")
    d, S = _dims(), 5
    model = build_model(d, synth.hot_path_state_dict(d, 8), dev)
    f, b, _ = _batch(dev, d, 8)
    seq, _att, logprob = model._sample(*_sample_args(f, b), sample_max=0, temperature=1.0, sample_n=S, seed=3)
    enc = tuple(f[k] for k in ("fc_feats", "conv_feats", "p_conv_feats", "pool_feats", "p_pool_feats", "pnt_mask"))
    model.debug_collect = {}
    with torch.no_grad():
        model.scst_loss(enc, seq, torch.ones(d.B * S, device=dev), None, S)
    c = model.debug_collect
    out = c["scst_out"].view(d.T, d.B * S, -1).transpose(0, 1) if c["scst_t_major"] else c["scst_out"].view(d.B * S, d.T, -1)
    logp = torch.log_softmax(F_.linear(out.reshape(d.B * S * d.T, -1).contiguous(), model.logit.weight, model.logit.bias).double(), 1)
    got = logp.view(d.B * S, d.T, -1).gather(2, seq.unsqueeze(2))[:, :, 0]
    err = float((got - logprob.double()).abs().max())
    print(f"[scst policy] max |log p (gradient pass) - logprob (engine)| = {err:.3e}")
    assert err <= LOGPROB_TOL


def _surrogate(model, f, b, seq, adv):
    B = f["fc_feats"].shape[0]
    dummy = torch.zeros(B, 1, 1, device=seq.device)
    out = model.score(f, b["input_seq"], b["gt_seq"], b["num"], b["proposals"], b["gt_bboxs"], b["box_mask"], dummy, b["frm_mask"],
                      b["sample_idx"], f["pnt_mask"], captions=seq)
    return float(-(adv.double()[:, None] * out["mask"].double() * out["logprob"].double()).sum())


def test_one_step_lowers_the_surrogate():
    """fresh Adam moments, lr = 1e-4, S = 5: the first Adam step moves every parameter against its gradient's sign, so to first order
    the surrogate -sum w log p of the step's own samples and advantages drops by lr times a positive sum"""
    dev = torch.device("cuda:0")
    d = _dims()
    _o, model, tr = _trainer(dev, d, seed=5, S=5, lr=1e-4)
    f, b, batch = _batch(dev, d, 5)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    tr.scst_step(batch)
    seq, adv = tr.last_scst["seq"], tr.last_scst["adv"]
    assert int((adv != 0).sum()) >= 5, adv
    after = _surrogate(model, f, b, seq, adv)
    model.load_state_dict(sd0)
    model.invalidate_decode_cache()
    before = _surrogate(model, f, b, seq, adv)
    print(f"[scst direction] surrogate before {before:.6f}, after {after:.6f}")
    assert after < before


@pytest.mark.parametrize("S", [5, 1])
def test_whole_step(S):
    from cvc import dropout
    from cvc.decode import DecodeEngine, DecodeWeights
    dev = torch.device("cuda:0")
    d = _dims()
    seed = 5
    _o, model, tr = _trainer(dev, d, seed=seed, S=S, lr=1e-3)
    f, b, batch = _batch(dev, d, seed)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    model.eval()
    att_before = model._sample(*_sample_args(f, b))[1]
    model.train()
    res = tr.scst_step(batch)
    assert len(res) == 4 and all(x.is_cuda and x.dim() == 0 and bool(torch.isfinite(x)) for x in res)
    assert model.training                                   # the step leaves the module's mode as it found it
    last = tr.last_scst
    seq = last["seq"]
    assert seq.shape == (d.B * S, d.T) and not (seq == synth.UNK_IDX).any()
    # ---- the returned reward is the CIDEr-D of the returned samples
    df, n_doc = R.doc_freq(_corpus(d, seed))
    refs, nref = b["gt_seq"].cpu().numpy(), b["num"][:, 0].cpu().numpy().astype(np.int32)
    ref64 = R.score_batch(seq.cpu().numpy(), refs, nref, df, n_doc)[0]
    ref32 = R.score_batch(seq.cpu().numpy(), refs, nref, df, n_doc, dt=np.float32)[0]
    bound = max(4.0 * float(np.abs(ref32 - ref64).max()), FLOOR)
    err = float(np.abs(last["reward"].cpu().double().numpy() - ref64).max())
    print(f"[scst step] S={S}: reward max |err| {err:.3e} (bound {bound:.3e}), mean reward {ref64.mean():.4f}, non-zero advantages "
          f"{int((last['adv'] != 0).sum())}/{d.B * S}, loss {float(res[0]):.5f}")
    assert err <= bound
    assert float(res[1]) == float(last["reward"].mean()) and float(res[3]) == float(last["adv"].abs().mean())
    if S == 1:
        greedy = last["greedy"].cpu().numpy()
        base64, base32 = R.score_batch(greedy, refs, nref, df, n_doc)[0], R.score_batch(greedy, refs, nref, df, n_doc, dt=np.float32)[0]
        assert float(np.abs(last["base"].cpu().double().numpy() - base64).max()) <= max(4.0 * float(np.abs(base32 - base64).max()), FLOOR)
        assert torch.equal(last["adv"], last["reward"] - last["base"])
    assert int((last["adv"] != 0).sum()) >= 1
    # ---- only the decoder's parameters moved
    moved = 0
    for k, v in model.state_dict().items():
        if k.startswith(("roi_feat_extractor", "localizer_core")):
            assert torch.equal(v, sd0[k]), k
        elif k.startswith(("decoder_core.att_lstm", "decoder_core.lang_lstm", "embed", "logit")):
            moved += int(not torch.equal(v, sd0[k]))
    assert moved >= 8, moved
    # ---- a following decode sees the new weights
    model.eval()
    att_after = model._sample(*_sample_args(f, b))[1]
    fresh = DecodeEngine(DecodeWeights({k: v for k, v in model.state_dict().items()}), f, d.T, synth.UNK_IDX).run()[1]
    assert not torch.equal(att_after, att_before)
    np.testing.assert_allclose(att_after.cpu().numpy(), fresh.cpu().numpy(), rtol=0, atol=1e-6)
    # ---- a cross-entropy step afterwards, from the same state, is the step of a run that never took a self-critical step
    _o2, model2, tr2 = _trainer(dev, d, seed=seed, S=S, lr=1e-3)
    dropout.seed(3)
    torch.manual_seed(3)
    want = [x.clone() for x in tr2.train_step(batch)]
    model.load_state_dict(sd0)
    model.invalidate_decode_cache()
    model.train()
    from cvc.trainer import Trainer, build_optimizer
    tr3 = Trainer(tr.opts, None, model, build_optimizer(model, tr.opts), None, None)
    dropout.seed(3)
    torch.manual_seed(3)
    got = tr3.train_step(batch)
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_), (got, want)
    for (k, v), (k2, v2) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k


def test_main_entry_point_takes_self_critical_epochs(tmp_path):
    """python -m cvc.main --scst_after 1: a cross-entropy epoch, then a self-critical one (table from the dataset's captions); the log
    and the histories carry the mean reward per display interval"""
    import os
    import pickle
    from cvc import main as cvc_main
    rc = cvc_main.main(["--no_cfg", "--max_epochs", "2", "--batch_size", "4", "--synthetic_clips", "12", "--num_prop_per_frm", "7",
                        "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "4",
                        "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "1", "--exp_name", "s", "--learning_rate", "0.001",
                        "--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/", "--id", "s1",
                        "--scst_after", "1", "--scst_samples", "3", "--scst_temperature", "1.0", "--scst_seed", "2"])
    assert rc == 0
    tr = cvc_main.LAST_TRAINER
    assert tr._scst_steps == 2 and tr.cider().n_doc == 12                    # 12 clips / 4 per batch, the last batch dropped
    assert list(tr.reward_history) == [1] and len(tr.reward_history[1]) == 2 and all(np.isfinite(r) and r >= 0 for r in tr.reward_history[1])
    assert tr.last_scst["seq"].shape == (12, 4)
    hist = pickle.load(open(os.path.join(tmp_path, "s", "histories_s1.pkl"), "rb"))
    assert hist["reward_history"] == tr.reward_history
