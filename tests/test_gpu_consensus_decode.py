"""Consensus selection on the decode side: DecodeEngine.consensus over samples and over beam hypotheses, model._sample(consensus=...),
Trainer.eval / Trainer.sample and the command line -- tiny models, sample_n = 4, beam = 4, T <= 8.  The kernel itself is pinned in
tests/test_gpu_consensus.py; here the candidates must be exactly what the decode returns without the switch, and everything that
is returned must be the picked candidate's."""
import json

import numpy as np
import pytest
import torch

from cvc import synth
import consensus_ref as C
import test_gpu_sampling as TS               # the tiny models' inputs and the _sample launcher

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
N = 4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _table(d, dev):
    from cvc.cider import CiderD
    rng = np.random.default_rng(17)
    return CiderD.from_captions([C.clip_candidates(rng, 1, d.T, d.V, garbage=False)[0] for _ in range(200)], dev)


def _model(dev, graph=False, **over):
    from helpers import build_model, to_dev
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=graph, **over)
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, 99), dev)
    return d, model, f, b


@pytest.mark.parametrize("graph", [False, True])
def test_sample_returns_the_picked_sample_of_the_plain_call_s_candidates(dev, graph):
    d, model, f, b = _model(dev, graph)
    table = model.consensus_table = _table(d, dev)
    kw = dict(sample_max=0, temperature=0.9, sample_n=N, seed=3)
    seq, att, lp = TS._model_sample(model, f, b, consensus=True, **kw)
    last = model.last_consensus
    pick, util, cand = last["pick"], last["utility"], last["candidates"]
    assert seq.shape == (d.B, d.T) and att.shape == (d.B, d.T, d.N) and lp.shape == (d.B, d.T)
    assert pick.shape == (d.B,) and pick.dtype == torch.int32 and util.shape == (d.B * N,) and cand.shape == (d.B * N, d.T)
    p_seq, p_att, p_lp = TS._model_sample(model, f, b, consensus=False, **kw)          # another cache key: a new engine, the same seed
    assert torch.equal(cand, p_seq)
    at = torch.arange(d.B, device=dev) * N + pick
    assert torch.equal(seq, p_seq[at]) and torch.equal(att.view(torch.int32), p_att[at].view(torch.int32))
    assert torch.equal(lp.view(torch.int32), p_lp[at].view(torch.int32))
    u2, p2, best2 = table.consensus(p_seq.contiguous(), N)
    assert torch.equal(util, u2) and torch.equal(pick, p2) and torch.equal(seq, best2)
    assert float(util.max()) > 0
    # the model's attribute is the default of the argument; "samples" brings its own n, temperature and seed
    model.consensus, model.consensus_samples, model.consensus_temperature, model.consensus_seed = "samples", N, 0.9, 3
    model._engine_cache = None
    s3 = TS._model_sample(model, f, b)
    assert torch.equal(s3[0], seq) and torch.equal(s3[2].view(torch.int32), lp.view(torch.int32))


def test_consensus_off_is_the_call_without_the_keyword(dev):
    d, model, f, b = _model(dev)
    model.consensus_table = _table(d, dev)
    for kw in (dict(), dict(sample_max=0, temperature=0.9, sample_n=N, seed=3), dict(beam_size=N)):
        model._engine_cache = None
        a = TS._model_sample(model, f, b, **kw)
        model._engine_cache = None
        c = TS._model_sample(model, f, b, consensus=False, **kw)
        for x, y in zip(a, c):
            assert (x is None and y is None) or torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                            y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert model.last_consensus is None


def test_sample_refuses_a_single_candidate(dev):
    d, model, f, b = _model(dev)
    model.consensus_table = _table(d, dev)
    for kw in (dict(), dict(sample_max=0, sample_n=1), dict(consensus_mode="beam", beam_size=1)):
        mode = kw.pop("consensus_mode", True)
        with pytest.raises(RuntimeError, match="several candidates"):
            TS._model_sample(model, f, b, consensus=mode, **kw)


def _beam_engine(dev, path, **kw):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs("tiny", seed=4321)
    return d, DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, path=path, **kw)


def _backtrack_from(eng, k):
    """DecodeEngine._backtrack_host from slot k[b] instead of slot 0"""
    B, beam, T, Nr = eng.B, eng.beam, eng.T, eng.N
    words, parent, att = eng.words[1:].view(T, B, beam), eng.parent.view(T, B, beam), eng.att_steps.view(T, B, beam, Nr)
    ar = torch.arange(B, device=words.device)
    seq, atts = [], []
    for t in range(T - 1, -1, -1):
        seq.append(words[t, ar, k])
        k_parent = parent[t, ar, k]
        atts.append(att[t, ar, k_parent])
        k = k_parent
    return torch.stack(seq[::-1], 1), torch.stack(atts[::-1], 1)


@pytest.mark.parametrize("path", ["ring", "tile"])
def test_beam_engine_picks_among_its_hypotheses(dev, path):
    d, eng = _beam_engine(dev, path, beam=N, beam_history=True)
    table = _table(d, dev)
    eng.run()
    hyp, score = eng.hypotheses()
    seq, att, lp, pick, util = eng.consensus(table)
    assert lp is None and seq.shape == (d.B, d.T) and att.shape == (d.B, d.T, d.N) and util.shape == (d.B * N,)
    ar = torch.arange(d.B, device=dev)
    live = torch.isfinite(score)
    u2, p2, best2 = table.consensus(hyp.reshape(d.B * N, d.T), N, live=live.reshape(-1))
    assert torch.equal(util, u2) and torch.equal(pick, p2)
    assert torch.equal(seq, hyp[ar, pick.long()]) and torch.equal(seq, best2)
    h_seq, h_att = _backtrack_from(eng, pick.long())
    assert torch.equal(seq, h_seq) and torch.equal(att.view(torch.int32), h_att.contiguous().view(torch.int32))
    assert live[ar, pick.long()].all() and float(util.max()) > 0
    # a dead slot is never picked: kill the picked slot of every clip and choose again
    eng.score[d.T & 1].view(d.B, N)[ar, pick.long()] = float("-inf")
    seq_b, att_b, _, pick_b, util_b = eng.consensus(table)
    assert (pick_b != pick).all() and not util_b.view(d.B, N)[ar, pick.long()].any()
    assert torch.equal(seq_b, hyp[ar, pick_b.long()])
    h_seq, h_att = _backtrack_from(eng, pick_b.long())
    assert torch.equal(seq_b, h_seq) and torch.equal(att_b.view(torch.int32), h_att.contiguous().view(torch.int32))


def test_sample_with_beam_search_returns_the_picked_hypothesis(dev):
    d, model, f, b = _model(dev)
    model.consensus_table = _table(d, dev)
    seq, att, none = TS._model_sample(model, f, b, beam_size=N, consensus=True)
    eng = model._engine_cache[1]
    last = model.last_consensus
    assert none is None and eng.beam_hist and last["candidates"].shape == (d.B, N, d.T)
    ar = torch.arange(d.B, device=dev)
    assert torch.equal(seq, last["candidates"][ar, last["pick"].long()])
    h_seq, h_att = _backtrack_from(eng, last["pick"].long())
    assert torch.equal(seq, h_seq) and torch.equal(att.view(torch.int32), h_att.contiguous().view(torch.int32))
    model._engine_cache = None
    plain = TS._model_sample(model, f, b, beam_size=N)                       # the candidates hold the plain call's rank-0 hypothesis
    assert torch.equal(plain[0], last["candidates"][:, 0])


def test_engine_refusals_name_their_reason(dev):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs("tiny", seed=4321)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    table = _table(d, dev)
    for eng, why in ((DecodeEngine(W, fd, d.T, UNK), "one candidate per clip"),
                     (DecodeEngine(W, fd, d.T, UNK, temperature=1.0, sample_n=1, seed=1), "one candidate per clip"),
                     (DecodeEngine(W, fd, d.T, UNK, forced_n=2), "forced"),
                     (DecodeEngine(W, fd, d.T, UNK, temperature=1.0, sample_n=2, seed=1, mix=True), "mix"),
                     (DecodeEngine(W, fd, d.T, UNK, beam=N), "beam_history=True")):
        with pytest.raises(RuntimeError, match=why):
            eng.consensus(table)


def test_trainer_eval_and_sample_with_consensus(dev, tmp_path):
    from cvc import main as cvc_main
    from cvc.misc import utils
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "12", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "6",
              "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100", "--exp_name", "c", "--learning_rate", "0.001",
              "--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/", "--id", "c1", "--language_eval"]
    assert cvc_main.main(common + ["--consensus", "samples", "--consensus_samples", str(N), "--val_metrics", "device"]) == 0
    tr = cvc_main.LAST_TRAINER
    model = getattr(tr.model, "module", tr.model)
    assert model.consensus == "samples" and model.consensus_table is tr.cider() and model.last_consensus is not None
    assert tr.submission_file is not None
    results = json.load(open(tr.submission_file))["results"]
    assert len(results) == 12
    # re-decode the first validation batch: a new engine draws the noise the evaluation's first batch drew
    model._engine_cache = None
    model.eval()
    bt = tr._prepare(next(iter(tr.val_loader)), False)
    with torch.no_grad():
        seq, att, lp = tr._call(bt, True)
    last = model.last_consensus
    assert seq.shape == (4, 6) and last["candidates"].shape == (4 * N, 6)
    assert torch.equal(seq, last["candidates"][torch.arange(4, device=dev) * N + last["pick"]])
    ds = tr.dataset
    sents = utils.decode_sequence(ds.itow, None, None, None, None, seq, tr.opts.vocab_size, tr.opts)
    for k, seg_id in enumerate(bt["seg_id"]):
        vid, seg = seg_id.split("_segment_")
        entry = [e for e in results[vid] if e["segment"] == str(int(seg))]
        assert len(entry) == 1 and entry[0]["sentence"] == sents[k], (seg_id, entry, sents[k])
    # Trainer.sample(consensus=True): all n sentences, the pick and the utilities
    path = tr.sample(N, 1.0, seed=5, consensus=True)
    out = json.load(open(path))
    entries = [e for segs in out.values() for e in segs]
    assert len(entries) == 12
    for e in entries:
        assert len(e["sentences"]) == N and len(e["utilities"]) == N and 0 <= e["consensus"] < N
        assert e["utilities"][e["consensus"]] == max(e["utilities"]) and e["consensus"] == e["utilities"].index(max(e["utilities"]))
    last = model.last_consensus                                             # the last batch's tensors
    tail = [e for vid in out for e in out[vid]][-4:]
    assert [e["consensus"] for e in tail] == last["pick"].tolist()
    assert [e["utilities"] for e in tail] == last["utility"].view(-1, N).tolist()
    model._engine_cache = None                                              # (a cached engine would draw fresh noise)
    plain = json.load(open(tr.sample(N, 1.0, seed=5)))
    assert all("consensus" not in e and "utilities" not in e for segs in plain.values() for e in segs)
    assert [e["sentences"] for segs in plain.values() for e in segs] == [e["sentences"] for e in entries]
    # consensus off: the evaluation is the one of a run that never heard of the switch
    model.consensus = "off"
    tr.eval(0)
    off = {k: [e["sentence"] for e in v] for k, v in tr.predictions.items()}
    assert cvc_main.main(common + ["--resume", "True", "--inference_only"]) == 0
    tr2 = cvc_main.LAST_TRAINER
    assert getattr(tr2.model, "module", tr2.model).consensus == "off"
    assert {k: [e["sentence"] for e in v] for k, v in tr2.predictions.items()} == off
