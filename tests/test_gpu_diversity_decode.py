"""Caption-set diversity on the decode side: DecodeEngine.set_diversity over samples and over the hypotheses of the history, diverse and
stochastic beams, Trainer.sample(diversity=True), python -m cvc.sample --diversity and cvc.main --val_diversity -- the tiny models of
the consensus decode tests, sets of 3 or 4 captions, T <= 8.  The kernel itself is pinned in tests/test_gpu_diversity.py; here the
engine must score exactly the candidates and the live mask its consensus selection uses, and leave itself as it was."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from cvc import synth
import diversity_ref as D
import overlap_ref as O
import test_gpu_sampling as TS               # the tiny models' inputs
import test_gpu_consensus_decode as CD

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
N = 4


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _engine(dev, **kw):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs("tiny", seed=4321)
    return d, DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, **kw)


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


ENGINES = {"samples": dict(temperature=0.9, sample_n=N, seed=3),
           "history beam": dict(beam=N, beam_history=True),
           "diverse beam": dict(beam=N, beam_history=True, beam_groups=2, diversity=0.5),
           "stochastic beam": dict(beam=N, beam_history=True, stochastic=True, stochastic_tau=0.9, seed=5)}


@pytest.mark.parametrize("name", list(ENGINES))
def test_engine_scores_its_own_candidates_and_stays_as_it_was(dev, name):
    from cvc import metrics
    d, eng = _engine(dev, **ENGINES[name])
    res = eng.run()
    before = [None if x is None else x.clone() for x in res]
    launches = eng._launches
    out = eng.set_diversity()
    if eng.sampling:
        cand, live = res[0].contiguous(), None
    else:
        hyp, score = eng.hypotheses()[:2]
        cand, live = hyp.reshape(d.B * N, d.T), torch.isfinite(score).reshape(-1)
    assert cand.shape == (d.B * N, d.T) and out["stats"].shape == (d.B, 12) and out["mbleu"].shape == (d.B * N, 4)
    assert _same(out, metrics.set_diversity(cand.contiguous(), N, live))
    st = out["stats"].cpu().long()
    assert torch.equal(st, torch.from_numpy(D.set_stats(cand.cpu().numpy(), N, None if live is None else live.cpu().numpy())))
    assert int(st[:, 8].min()) >= 2 and int(st[:, 4].sum()) > 0
    if name == "stochastic beam":            # the slots are pairwise distinct by construction
        assert torch.equal(st[:, 9], st[:, 8])
    # nothing of the engine moved: its outputs, its launch list; a second call gives the same
    for x, y in zip(res, before):            # (run() returns views of the engine's buffers)
        assert (x is None and y is None) or torch.equal(x, y)
    assert eng._launches is launches and _same(out, eng.set_diversity())


def test_cold_samples_are_one_caption_per_clip(dev):
    d, eng = _engine(dev, temperature=1e-3, sample_n=N, seed=3)
    eng.run()
    st = eng.set_diversity()["stats"]
    assert (st[:, 8] == N).all() and (st[:, 9] == 1).all()
    assert (st[:, 4:8] % N == 0).all() and (N * st[:, 0:4] <= st[:, 4:8]).all()             # n copies of one caption
    mb = eng.set_diversity()["mbleu_stats"]
    assert torch.equal(mb[:, 0:4], mb[:, 4:8]) and torch.equal(mb[:, 8], mb[:, 9])          # every caption is its references


def test_engine_refusals_name_their_reason(dev):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs("tiny", seed=4321)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    for eng, why in ((DecodeEngine(W, fd, d.T, UNK), "set_diversity: one candidate per clip"),
                     (DecodeEngine(W, fd, d.T, UNK, temperature=1.0, sample_n=1, seed=1), "set_diversity: one candidate per clip"),
                     (DecodeEngine(W, fd, d.T, UNK, forced_n=2), "set_diversity: a forced engine"),
                     (DecodeEngine(W, fd, d.T, UNK, temperature=1.0, sample_n=2, seed=1, mix=True), "set_diversity: a mix engine"),
                     (DecodeEngine(W, fd, d.T, UNK, beam=N), "set_diversity: a beam engine needs beam_history=True")):
        with pytest.raises(RuntimeError, match=why):
            eng.set_diversity()


def _entry_scores(sentences, wtoi):
    """an entry's diversity from its sentences alone, by the restatement"""
    T = max(max(len(s.split()) for s in sentences), 1) + 1
    cand = np.zeros((len(sentences), T), np.int64)
    for j, s in enumerate(sentences):
        ids = [int(wtoi[w]) for w in s.split()]
        cand[j, :len(ids)] = ids
    st = D.set_stats(cand, len(sentences))
    ms, _ = D.mbleu(cand, len(sentences))
    return st[0], (O.corpus(ms.sum(0))[3] if ms[:, 8].sum() > 0 else 0.0), ms


COMMON = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
          "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "6",
          "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100", "--exp_name", "d", "--learning_rate", "0.001"]


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """one tiny cvc.main run with --val_diversity (an epoch and its validation pass); every test below sets what it needs itself"""
    from cvc import main as cvc_main
    tmp = tmp_path_factory.mktemp("diversity")
    common = COMMON + ["--results_dir", str(tmp / "results"), "--checkpoint_path", str(tmp) + "/", "--id", "d1"]
    assert cvc_main.main(common + ["--consensus", "samples", "--consensus_samples", str(N), "--val_metrics", "device",
                                   "--val_diversity"]) == 0
    tr = cvc_main.LAST_TRAINER
    return tr, getattr(tr.model, "module", tr.model), common


def _entries(out):
    return [e for segs in out.values() for e in segs]


def test_val_diversity_puts_the_five_keys_into_lang_stats(run):
    tr, model, _ = run
    assert tr.val_diversity and "val_diversity" in vars(tr.opts)
    model.consensus, tr.val_diversity = "samples", True
    stats = tr.eval(0)
    assert {"Div_1", "Div_2", "mBLEU_4", "Unique", "oracle_CIDEr", "CIDEr", "Bleu_4"} <= set(stats)
    assert 0 < stats["Div_1"] <= 1 and 0 < stats["Unique"] <= 1 and stats["oracle_CIDEr"] >= stats["CIDEr"] - 1e-9
    assert model.last_consensus["live"] is None and model.last_consensus["candidates"].shape == (4 * N, 6)
    tr.val_diversity = False
    assert not {"Div_1", "Div_2", "mBLEU_4", "Unique", "oracle_CIDEr"} & set(tr.eval(0))


def test_val_diversity_without_a_candidate_set_is_refused(run):
    tr, model, _ = run
    model.consensus, tr.val_diversity = "off", True
    try:
        with pytest.raises(RuntimeError, match="val_diversity needs"):
            tr.eval(0)
    finally:
        model.consensus, tr.val_diversity = "samples", False


def test_beam_consensus_keeps_the_live_mask_it_used(dev):
    from cvc import metrics
    d, model, f, b = CD._model(dev)
    model.consensus_table = CD._table(d, dev)
    TS._model_sample(model, f, b, beam_size=N, consensus=True)
    last, eng = model.last_consensus, model._engine_cache[1]
    assert last["live"].shape == (d.B, N) and last["live"].dtype == torch.bool
    assert torch.equal(last["live"], torch.isfinite(eng.hypotheses()[1]))
    assert _same(eng.set_diversity(), metrics.set_diversity(last["candidates"].reshape(d.B * N, d.T), N, last["live"].reshape(-1)))


def test_trainer_sample_writes_entry_and_summary_keys_that_equal_the_restatement(run, capsys):
    from cvc import metrics
    tr, model, _ = run
    n = 3
    model.consensus, model._engine_cache = "off", None
    out = json.load(open(tr.sample(n, 1.0, seed=5, diversity=True)))
    summary = out.pop("diversity")
    assert summary == tr.sample_diversity and {"oracle_CIDEr", "mean_CIDEr", *metrics.DIVERSITY_KEYS} == set(summary)
    assert json.dumps(tr.sample_diversity) in capsys.readouterr().out
    entries = _entries(out)
    assert len(entries) == 8 and summary["Sets"] == 8
    all_st, all_ms = [], []
    wtoi = {w: int(i) for i, w in tr.dataset.itow.items()}
    assert len(wtoi) == len(tr.dataset.itow)                                 # (words name their ids one to one)
    for e in entries:
        st, mb4, ms = _entry_scores(e["sentences"], wtoi)
        dv = e["diversity"]
        assert set(dv) == {"div1", "div2", "mbleu4", "unique"} and dv["unique"] == st[9] and st[4] > 0
        assert dv["div1"] == float(np.float32(st[0]) / np.float32(st[4])) and dv["div2"] == float(np.float32(st[1]) / np.float32(st[4]))
        assert abs(dv["mbleu4"] - mb4) <= 1e-12 * abs(mb4)
        all_st.append(st), all_ms.append(ms)
    want = D.result(np.stack(all_st), np.concatenate(all_ms))
    for k in want:
        assert abs(summary[k] - want[k]) <= 1e-12 * abs(want[k]), k
    assert summary["oracle_CIDEr"] >= summary["mean_CIDEr"] >= 0           # (a random tiny model's samples may share nothing with the references)


def test_trainer_sample_with_diversity_off_writes_the_file_it_wrote_before(run):
    tr, model, _ = run
    n = 3
    model.consensus, model._engine_cache = "off", None
    on = json.load(open(tr.sample(n, 1.0, seed=5, diversity=True)))
    model._engine_cache = None                                              # (a cached engine would draw fresh noise)
    off = open(tr.sample(n, 1.0, seed=5, diversity=False)).read()
    model._engine_cache = None
    plain = open(tr.sample(n, 1.0, seed=5)).read()
    assert off == plain and "diversity" not in plain
    del on["diversity"]
    for e in _entries(on):
        del e["diversity"]
    assert json.loads(plain) == on


def test_trainer_sample_diversity_composes_with_the_other_switches(run):
    tr, model, _ = run
    n = 3
    model.consensus, model._engine_cache = "off", None
    wor = json.load(open(tr.sample(n, 0.9, seed=4, without_replacement=True, consensus=True, diversity=True)))
    assert wor.pop("diversity")["Sets"] == 8
    for e in _entries(wor):                                                 # pairwise distinct draws: unique == live (a filler's G is -inf)
        assert e["diversity"]["unique"] == sum(1 for g in e["G"] if np.isfinite(g)) >= 1 and "consensus" in e
    tk = json.load(open(tr.sample(n, 1.0, seed=4, top_k=5, top_p=0.9, constraints=dict(no_immediate_repeat=True), diversity=True)))
    assert tk.pop("diversity")["Sets"] == 8 and all("diversity" in e for e in _entries(tk))


def test_trainer_sample_refuses_the_diversity_of_one_caption(run):
    tr, _, _ = run
    with pytest.raises(RuntimeError, match="n > 1 captions per segment"):
        tr.sample(1, 1.0, diversity=True)


def test_sample_command_line_writes_the_keys(run):
    from cvc import main as cvc_main
    from cvc import sample as cvc_sample
    _, _, common = run
    assert cvc_sample.main(common + ["--resume", "True", "--temperature", "0.8", "--sample_n", "2", "--sample_seed", "4",
                                     "--diversity"]) == 0
    tr2 = cvc_main.LAST_TRAINER
    path = glob.glob(os.path.join(tr2.opts.results_dir, "*_samples.json"))
    assert len(path) == 1
    cli = json.load(open(path[0]))
    assert cli.pop("diversity")["Sets"] == 8 and all(len(e["sentences"]) == 2 and "diversity" in e for e in _entries(cli))
