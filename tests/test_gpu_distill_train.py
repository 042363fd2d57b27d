"""Word-level distillation above the kernels, on the GPU: the teacher's rows kept per step by the forced ensemble engine
(EnsembleEngine keep_rows=True, CaptionEnsemble.soft_targets), the student's distilled loss and gradients against torch autograd in
fp64, a short training run and the command line.  The kernels themselves: tests/test_gpu_distill.py."""
import dataclasses
import math
import os
import pickle

import numpy as np
import pytest
import torch

from cvc import synth
import distill_ref as R

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
SEEDS, WEIGHTS = (5, 11), (0.4, 0.6)
LOGPROB_TOL = 1e-4          # tests/test_gpu_ensemble.py: the forced ensemble against its oracle is held to 2 x this


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x


# ------------------------------------------------------------------------------------------------ teacher rows kept per step
def _members(dev, feat_seeds=None):
    """[(DecodeWeights, feats on the device)] of two checkpoints, each with its own features and one proposal mask"""
    from helpers import to_dev
    from cvc.decode import DecodeWeights
    d = synth.CONFIGS["tiny"]
    mask = synth.clip_features(d, SEEDS[0])["pnt_mask"]
    out = []
    for s, fs in zip(SEEDS, feat_seeds or SEEDS):
        f = synth.clip_features(d, fs)
        f["pnt_mask"] = mask
        out.append((DecodeWeights(to_dev(synth.hot_path_state_dict(d, s), dev)), to_dev(f, dev)))
    return d, out


def _words(d, n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, d.V, (d.B * n, d.T), generator=g).to(dev)      # arbitrary words: far down the ranking included


@pytest.mark.parametrize("combine", ["prob", "logprob"])
def test_keep_rows_keeps_every_steps_row_and_changes_nothing_else(dev, combine):
    """EnsembleEngine(forced_n=2, keep_rows=True): logprob, rank and att have the bits of the engine without it, the last kept row the
    bits of that engine's `combined`; at every step the fp64 log-softmax of the kept row at the given word meets the engine's logprob
    within 2 x LOGPROB_TOL (the bound tests/test_gpu_ensemble.py holds the forced mode to against its oracle); the launch lists differ
    in nothing but the rows' addresses"""
    from cvc.decode import EnsembleEngine
    d, gpu = _members(dev)
    n = 2
    words = _words(d, n, 3, dev)
    base = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, combine=combine, forced_n=n).load_captions(words)
    kept = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, combine=combine, forced_n=n, keep_rows=True).load_captions(words)
    rb, rk = [x.clone() for x in base.run()], [x.clone() for x in kept.run()]
    for a, b in zip(rb, rk):
        assert torch.equal(_bits(a), _bits(b))
    assert kept.combined.shape == (d.T, d.B * n, d.V) and base.combined.shape == (d.B * n, d.V)
    assert torch.equal(_bits(kept.combined[-1]), _bits(base.combined))
    assert [e[0] for e in base._launches] == [e[0] for e in kept._launches]
    lp = torch.log_softmax(kept.combined.double(), 2).gather(2, words.t()[:, :, None]).squeeze(2).t()        # [rows, T]
    err = float((lp - rk[2].double()).abs().max())
    print(f"[distill] kept rows ({combine}): max |fp64 log-softmax at the given word - engine logprob| {err:.3e} (bound {2 * LOGPROB_TOL:.1e})")
    assert err <= 2 * LOGPROB_TOL
    if combine == "prob":                       # the mixture of probabilities is normalised as it stands
        assert float(torch.logsumexp(kept.combined.double(), 2).abs().max()) <= 2 * LOGPROB_TOL
    with pytest.raises(RuntimeError, match="keep_rows"):
        EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, keep_rows=True)


def test_a_second_batch_through_the_captured_teacher_graph_equals_a_fresh_engine(dev):
    from cvc.decode import EnsembleEngine
    d, gpu = _members(dev)
    _, gpu2 = _members(dev, feat_seeds=(55, 66))
    n = 2
    w1, w2 = _words(d, n, 3, dev), _words(d, n, 4, dev)
    e = EnsembleEngine(gpu, d.T, UNK, member_weights=WEIGHTS, forced_n=n, keep_rows=True, own_features=True).load_captions(w1).capture()
    e.run()
    first = e.combined.clone()
    got = [x.clone() for x in e.load_features([f for _, f in gpu2]).load_captions(w2).run()] + [e.combined.clone()]
    fresh = EnsembleEngine(gpu2, d.T, UNK, member_weights=WEIGHTS, forced_n=n, keep_rows=True).load_captions(w2)
    want = [x.clone() for x in fresh.run()] + [fresh.combined.clone()]
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(first, got[-1])


# ------------------------------------------------------------------------------------------------ the student
def _dims(V):
    return dataclasses.replace(synth.CONFIGS["tiny"], B=12, R=64, A=32, E=32, V=V, T=6)


def _model(dev, d, seed=5, **over):
    from helpers import build_model
    return build_model(d, synth.hot_path_state_dict(d, seed), dev, **over)


def _batch(dev, d, seed=5):
    from helpers import to_dev
    return to_dev(synth.clip_features(d, seed), dev), to_dev(synth.label_glue_batch(d, seed), dev)


def _eleven(f, b):
    dummy = torch.zeros(f["fc_feats"].shape[0], 1, 1, device=f["fc_feats"].device)
    return (f, b["input_seq"], b["gt_seq"], b["num"], b["proposals"], b["gt_bboxs"], b["box_mask"], dummy, b["frm_mask"], b["sample_idx"],
            f["pnt_mask"])


def _pass(model, f, b, seed=31, **kw):
    """one training pass on the dropout masks of `seed`, backward of 0.5 lm + 0.5 recon -> (losses, {name: gradient})"""
    from cvc import dropout
    dropout.seed(seed)
    model.zero_grad(set_to_none=True)
    out = model(*_eleven(f, b), **kw)
    (0.5 * out[0].mean() + 0.5 * out[4].mean()).backward()
    return [x.detach().clone() for x in out], {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _restated(logits, rows_bm, target, alpha, tau, dtype):
    """the mixed loss on materialised b-major logits in `dtype`, differentiable: (1 - alpha) mean NLL + alpha tau^2 mean KL over the
    text mask -> (loss, nll, kd)"""
    import label_smoothing_ref as LS
    z = logits.to(dtype)
    tf = target.reshape(-1)
    m = LS.text_mask(target).reshape(-1).to(dtype)
    q = torch.softmax(rows_bm.to(dtype) / tau, 1)
    kl = (q * (torch.log_softmax(rows_bm.to(dtype) / tau, 1) - torch.log_softmax(z / tau, 1))).sum(1)
    nll = -torch.log_softmax(z, 1).gather(1, tf[:, None]).squeeze(1)
    n = m.sum()
    return ((m * ((1 - alpha) * nll + alpha * tau * tau * kl)).sum() / n, (m * nll).sum() / n, (m * tau * tau * kl).sum() / n)


@pytest.mark.parametrize("members", [2, 1])
@pytest.mark.parametrize("V", [100, 97])
def test_distilled_loss_and_gradients_vs_fp64_autograd(dev, V, members):
    """A small synthetic model in training mode (dropout on, in-kernel masks of a fixed seed) at a width the fused head takes (V = 100,
    72 rows) and at one it refuses (V = 97), a teacher of two checkpoints and of one (then on a captured forced engine), alpha 0.3,
    tau 2.
    Truth: the unfused path's own pass with its criterion replaced by torch autograd in fp64 over the logits it materialised (the
    mixed loss restated); yardstick: the same with the restatement in fp32.  The distilled pass of the unfused path (the two-step
    kernels, on those same logits) meets the truth in the LM loss and in every parameter's gradient within 4 x the yardstick's error,
    floor 2^-20.  The default pass (C-driven loops, fused head where it is taken) meets the truth's LM loss under the same bound; its
    gradients run through other kernels than the truth's graph, so they are held to the bound tests/test_gpu_train.py holds the two
    routes to against each other, 5e-4 of the norm.  last_nll / last_kd are the unmixed means."""
    from cvc import train_loops
    from cvc.model.ensemble import CaptionEnsemble
    alpha, tau = 0.3, 2.0
    d = _dims(V)
    model = _model(dev, d).train()
    f, b = _batch(dev, d)
    teachers = [_model(dev, d, seed=s, hip_graph=members == 1) for s in (11, 23)[:members]]
    teacher = CaptionEnsemble(teachers, weights=None if members == 1 else WEIGHTS)
    rows, t_lp = teacher.soft_targets(*_eleven(f, b))
    assert rows.shape == (d.T, d.B, V) and t_lp.shape == (d.B, d.T) and not rows.requires_grad
    rows = rows.clone()
    rows_bm = rows.permute(1, 0, 2).reshape(d.B * d.T, V)
    model.distill = dict(teacher=teacher, alpha=alpha, tau=tau)

    res = {}
    train_loops.ENABLED = False
    try:
        for dtype in (torch.float64, torch.float32):
            seen = {}

            def fake(logits, att2_weights, ground_weights, target, att2_target, input_seq, t_major=False, distill=None, _dt=dtype):
                assert not t_major and distill is None
                loss, nll, kd = _restated(logits, rows_bm, target, alpha, tau, _dt)
                seen.update(loss=loss.detach(), nll=nll.detach(), kd=kd.detach())
                amax = logits.argmax(1).view(target.shape)
                return (loss.float(), *model.critLM.attention_losses(att2_weights, ground_weights, att2_target), amax)
            model.critLM.from_logits = fake
            try:
                out, grads = _pass(model, f, b)
            finally:
                del model.critLM.from_logits
            res[dtype] = (seen, out, grads)
        out_e, grads_e = _pass(model, f, b, soft_targets=rows)
        nll_e, kd_e = model.last_nll.clone(), model.last_kd.clone()
    finally:
        train_loops.ENABLED = True
    (t64, out64, g64), (t32, _o32, g32) = res[torch.float64], res[torch.float32]
    tag = f"V {V} M {members}"
    for name, got, want, yard32 in (("lm_loss", out_e[0], t64["loss"], t32["loss"]), ("last_nll", nll_e, t64["nll"], t32["nll"]),
                                    ("last_kd", kd_e, t64["kd"], t32["kd"])):
        err, yard = abs(float(got.double().cpu()) - float(want)), abs(float(yard32) - float(want))
        bound = max(4.0 * yard, R.FLOOR)
        print(f"[distill] model {tag} unfused {name}: {float(got):.6f} vs {float(want):.6f}, |err| {err:.3e} (yardstick {yard:.3e}, bound {bound:.3e})")
        assert err <= bound, (name, err, bound)
    assert float(kd_e) > 0 and nll_e.dim() == 0 and not kd_e.requires_grad
    assert set(grads_e) == set(g64) and "logit.weight" in g64 and "decoder_core.att_lstm.weight_ih" in g64
    for n in sorted(g64):
        err = float((grads_e[n].double() - g64[n].double()).abs().max())
        yard = float((g32[n].double() - g64[n].double()).abs().max())
        bound = max(4.0 * yard, R.FLOOR)
        print(f"[distill] model {tag} unfused d {n}: max |err| {err:.3e} (yardstick {yard:.3e}, bound {bound:.3e})")
        assert err <= bound, (n, err, bound)
    # the default pass: C-driven loops, the fused head at V = 100
    calls = []
    orig = model.critLM.from_head
    model.critLM.from_head = lambda *a, **k: (calls.append(k), orig(*a, **k))[1]
    try:
        out_c, grads_c = _pass(model, f, b, soft_targets=rows)
    finally:
        del model.critLM.from_head
    assert len(calls) == 1 and calls[0]["distill"][1:] == (alpha, tau) and calls[0]["t_major"]
    err, yard = abs(float(out_c[0].double().cpu()) - float(t64["loss"])), abs(float(t32["loss"]) - float(t64["loss"]))
    bound = max(4.0 * yard, 4.0 * float(t64["loss"]) * 2.0 ** -23, R.FLOOR)
    print(f"[distill] model {tag} default lm_loss: |err| {err:.3e} (yardstick {yard:.3e}, bound {bound:.3e})")
    assert err <= bound
    for n in sorted(g64):
        if float(g64[n].abs().max()) <= R.FLOOR:
            # (a gradient that is zero in exact arithmetic -- alpha_net's bias under the softmax's shift invariance -- is rounding
            # noise in both passes: nothing to take a ratio of; it stays below the floor)
            assert float(grads_c[n].abs().max()) <= R.FLOOR, n
            continue
        rel = float((grads_c[n].double() - g64[n].double()).norm() / g64[n].double().norm())
        print(f"[distill] model {tag} default d {n}: relative error {rel:.3e}")
        assert rel <= 5e-4, (n, rel)
    # the reconstruction loss is not distilled: it is the plain pass's, bit for bit
    model.distill = None
    out_p, _ = _pass(model, f, b)
    assert torch.equal(out_p[4], out_c[4]) and model.last_kd is None and model.last_nll is None
    assert float(out_p[0]) != float(out_c[0])


def test_refusals_of_the_model_and_the_criteria(dev):
    from cvc.model.ensemble import CaptionEnsemble
    d = _dims(100)
    model = _model(dev, d).train()
    f, b = _batch(dev, d)
    teacher = CaptionEnsemble([_model(dev, d, seed=11)])
    rows = teacher.soft_targets(*_eleven(f, b))[0]
    with pytest.raises(RuntimeError, match="model.distill"):
        model(*_eleven(f, b), soft_targets=rows)
    model.distill = dict(teacher=teacher, alpha=0.5, tau=1.0)
    with pytest.raises(RuntimeError, match="soft_targets"):
        model(*_eleven(f, b), soft_targets=rows, ss_inputs=torch.zeros(d.B, d.T, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="soft_targets"):
        model(*_eleven(f, b), True, soft_targets=rows)
    model.label_smoothing = 0.1
    with pytest.raises(ValueError, match="label_smoothing"):
        model(*_eleven(f, b), soft_targets=rows)
    model.label_smoothing = 0.0
    model.confidence_penalty = 0.05
    with pytest.raises(ValueError, match="confidence penalty"):
        model(*_eleven(f, b), soft_targets=rows)
    model.confidence_penalty = None
    with pytest.raises(ValueError, match="teacher_rows"):
        model(*_eleven(f, b), soft_targets=rows[:-1])
    model.distill = dict(teacher=teacher, alpha=1.5, tau=1.0)
    with pytest.raises(ValueError, match="alpha"):
        model(*_eleven(f, b), soft_targets=rows)


def test_without_distillation_nothing_changes(dev):
    """two models built alike: one never hears of distillation, the other carries model.distill (set, and a pass without
    soft_targets; then unset) -- losses and every gradient bit-equal, the same criterion calls"""
    from cvc.model.ensemble import CaptionEnsemble
    d = _dims(100)
    f, b = _batch(dev, d)
    plain, other = _model(dev, d).train(), _model(dev, d).train()
    out_p, grads_p = _pass(plain, f, b)
    other.distill = dict(teacher=CaptionEnsemble([_model(dev, d, seed=11)]), alpha=0.5, tau=2.0)
    calls = []
    orig = other.critLM.from_head
    other.critLM.from_head = lambda *a, **k: (calls.append(k), orig(*a, **k))[1]
    try:
        out_s, grads_s = _pass(other, f, b)
    finally:
        del other.critLM.from_head
    assert len(calls) == 1 and "distill" not in calls[0]
    other.distill = None
    out_u, grads_u = _pass(other, f, b)
    for out, grads in ((out_s, grads_s), (out_u, grads_u)):
        assert all(torch.equal(x, y) for x, y in zip(out_p, out))
        assert set(grads) == set(grads_p) and all(torch.equal(grads[n], grads_p[n]) for n in grads_p)
    assert other.last_kd is None and other.last_nll is None


# ------------------------------------------------------------------------------------------------ training
def test_thirty_distilled_trainer_steps_bring_the_kd_down(dev, capsys):
    """thirty eager Trainer steps on one batch with alpha = 1, tau = 1 and a differently seeded teacher: every loss finite, kd_history
    filled (one display interval per step), the mean KD of the last three steps below that of the first three; the display line shows
    NLL and KD; no step was captured.  The steps train the decoder on loop A's loss alone (train_decoder_only): the reconstruction
    loss is not distilled and shares every weight with loop A -- at equal weight it pulls the student towards the one-hot captions
    and away from a randomly initialised teacher, whose distributions are nearly uniform (measured: the KD then rises from 0.096 to
    0.22 over the thirty steps while NLL and reconstruction loss fall)."""
    from helpers import make_opts
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.model.ensemble import CaptionEnsemble
    from cvc.trainer import Trainer, build_optimizer
    from cvc import opts as cvc_opts
    d, seed = _dims(100), 5
    o = cvc_opts.parse_opt([])
    for k, v in vars(make_opts(d, train_decoder_only=True)).items():
        setattr(o, k, v)
    o.xe_loss_weight, o.learning_rate, o.batch_size, o.disp_interval = 1.0, 2e-3, d.B, 1
    model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed).items()}, strict=False)
    model = model.to(dev)
    teacher = CaptionEnsemble([_model(dev, d, seed=11)])
    model.distill = dict(teacher=teacher, alpha=1.0, tau=1.0)
    f, b = _batch(dev, d, seed)
    batch = (f, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
             ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], f["pnt_mask"][:, 1:])
    tr = Trainer(o, None, model, build_optimizer(model, o), [batch] * 31, None)          # (train() drops the last batch)
    steps = []
    orig = tr.train_step_prepared
    tr.train_step_prepared = lambda bb: (steps.append([x.clone() for x in orig(bb)]), steps[-1])[1]
    before = {n: p.detach().clone() for n, p in teacher.models[0].named_parameters()}
    tr.train(0)
    torch.cuda.synchronize()
    assert len(steps) == 30 and all(len(s) == 7 for s in steps)
    vals = torch.stack([torch.stack([x.reshape(()) for x in s]) for s in steps]).cpu()
    assert bool(torch.isfinite(vals).all())
    kd = tr.kd_history[0]
    assert len(kd) == 30 and all(math.isfinite(x) and x > 0 for x in kd) and len(tr.nll_history[0]) == 30
    np.testing.assert_allclose(kd, vals[:, 6].numpy(), rtol=1e-6)
    first, last = sum(kd[:3]) / 3, sum(kd[-3:]) / 3
    print(f"[distill] thirty steps: mean KD of the first three {first:.5f}, of the last three {last:.5f}")
    assert last < first
    np.testing.assert_allclose(vals[:, 1].numpy(), vals[:, 6].numpy(), rtol=1e-5)       # alpha = 1: the LM loss is the KD
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Epoch: [")]
    assert len(lines) == 30 and all("\tKD " in l and "\tNLL " in l for l in lines)
    assert tr.graph_stats["captured"] == 0 and tr.graph_stats["replayed"] == 0
    assert tr.last_kd["teacher_logprob"].shape == (d.B, d.T)
    assert all(torch.equal(p.detach(), before[n]) for n, p in teacher.models[0].named_parameters())      # the teacher is frozen
    # a self-critical or scheduled-sampling step is not distilled
    model.ss_prob = 0.25
    with pytest.raises(RuntimeError, match="scheduled sampling"):
        orig(tr._prepare(batch, True))


def test_main_entry_point_distils_from_a_checkpoint(tmp_path, capsys):
    """python -m cvc.main --distill_from teacher.pth --max_epochs 1 on synthetic clips finishes, shows KD and writes kd_history; a run
    without the flags has no such key"""
    from cvc import main as cvc_main
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "12", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "4",
              "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "1", "--learning_rate", "0.001",
              "--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/"]
    assert cvc_main.main(common + ["--exp_name", "t", "--id", "t1", "--seed", "7"]) == 0           # the teacher's checkpoint
    hist = pickle.load(open(os.path.join(tmp_path, "t", "histories_t1.pkl"), "rb"))
    assert "kd_history" not in hist and cvc_main.LAST_TRAINER.kd_history == {}
    capsys.readouterr()
    teacher = str(tmp_path / "t" / "model.pth")
    rc = cvc_main.main(common + ["--exp_name", "s", "--id", "s1", "--distill_from", teacher, "--distill_alpha", "0.7",
                                 "--distill_temperature", "2"])
    assert rc == 0
    tr = cvc_main.LAST_TRAINER
    model = getattr(tr.model, "module", tr.model)
    assert model.distill["alpha"] == pytest.approx(0.7) and model.distill["tau"] == pytest.approx(2.0)
    assert len(model.distill["teacher"].models) == 1 and not any(p.requires_grad for p in model.distill["teacher"].models[0].parameters())
    assert sorted(tr.kd_history) == [0] and len(tr.kd_history[0]) == 2                  # 12 clips / 4 per batch, the last dropped
    assert all(math.isfinite(x) and x > 0 for x in tr.kd_history[0])
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Epoch: [")]
    assert len(lines) == 2 and all("\tKD " in l for l in lines) and "distilling from 1 checkpoints" in out
    hist = pickle.load(open(os.path.join(tmp_path, "s", "histories_s1.pkl"), "rb"))
    assert hist["kd_history"] == tr.kd_history
