"""Spectral set diversity on the decode side: DecodeEngine.set_spectrum over samples and over the hypotheses of the history, diverse
and stochastic beams, Trainer.sample(self_cider=True) and cvc.main --val_diversity --val_self_cider -- the tiny models of the
diversity decode tests, sets of 3 or 4 captions, T <= 8.  The kernel itself is pinned in tests/test_gpu_spectrum.py; here the engine
must score exactly the candidates and the live mask its consensus selection uses, and leave itself as it was."""
import json
import math
import pickle

import pytest
import torch

import spectrum_ref as S
import test_gpu_consensus_decode as CD
import test_gpu_diversity_decode as DD

pytestmark = pytest.mark.gpu

N = DD.N


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(DD.ENGINES))
def test_engine_scores_its_own_candidates_and_stays_as_it_was(dev, name):
    from cvc import metrics
    d, eng = DD._engine(dev, **DD.ENGINES[name])
    table = CD._table(d, dev)
    res = eng.run()
    before = [None if x is None else x.clone() for x in res]
    launches = eng._launches
    lsa, cid = eng.set_spectrum(), eng.set_spectrum(table)
    if eng.sampling:
        cand, live = res[0].contiguous(), None
    else:
        hyp, score = eng.hypotheses()[:2]
        cand, live = hyp.reshape(d.B * N, d.T), torch.isfinite(score).reshape(-1)
    assert lsa["lam"].shape == (d.B, 32) and lsa["score"].shape == (d.B, 2) and lsa["info"].shape == (d.B, 2) and "gram" not in lsa
    assert DD._same(lsa, metrics.set_spectrum(cand.contiguous(), N, live))
    assert DD._same(cid, metrics.set_spectrum(cand.contiguous(), N, live, cider=table))
    assert DD._same(cid, table.self_cider(cand.contiguous(), N, live))
    m = [len(S.live_rows(cand.cpu().numpy(), N, None if live is None else live.cpu().numpy(), k)) for k in range(d.B)]
    assert lsa["info"][:, 0].tolist() == m and cid["info"][:, 0].tolist() == m and min(m) >= 2
    for out in (lsa, cid):
        assert (out["info"][:, 1] >= 1).all() and (out["score"] >= 0).all() and (out["score"] <= 1).all()
    # nothing of the engine moved: its outputs, its launch list; a second call gives the same
    for x, y in zip(res, before):            # (run() returns views of the engine's buffers)
        assert (x is None and y is None) or torch.equal(x, y)
    assert eng._launches is launches and DD._same(lsa, eng.set_spectrum()) and DD._same(cid, eng.set_spectrum(table))


def test_cold_samples_score_zero(dev):
    # n copies of one caption: K is exactly rank 1 (equal rows give s_n = 1 exactly; lsa is exact anyway), so lam_1 = tr up to the
    # solve's own error, at most 256 u tr over the whole spectrum: score 0 <= -log(1 - 256 u) / log 2 < 1e-13, and the other
    # eigenvalues, at most 256 u tr each, put score 1 at most at (N - 1) sqrt(256 u) / log N < 4e-7
    d, eng = DD._engine(dev, temperature=1e-3, sample_n=N, seed=3)
    table = CD._table(d, dev)
    eng.run()
    assert (eng.set_diversity()["stats"][:, 9] == 1).all()
    for out in (eng.set_spectrum(), eng.set_spectrum(table)):
        assert (out["info"][:, 0] == N).all()
        assert float(out["score"][:, 0].max()) <= 1e-13 and float(out["score"][:, 1].max()) <= (N - 1) * math.sqrt(256 * S.U) / math.log(N)


def test_engine_refusals_name_their_reason(dev):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = DD.TS._inputs("tiny", seed=4321)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    for eng, why in ((DecodeEngine(W, fd, d.T, DD.UNK), "set_spectrum: one candidate per clip"),
                     (DecodeEngine(W, fd, d.T, DD.UNK, forced_n=2), "set_spectrum: a forced engine"),
                     (DecodeEngine(W, fd, d.T, DD.UNK, temperature=1.0, sample_n=2, seed=1, mix=True), "set_spectrum: a mix engine"),
                     (DecodeEngine(W, fd, d.T, DD.UNK, beam=N), "set_spectrum: a beam engine needs beam_history=True")):
        with pytest.raises(RuntimeError, match=why):
            eng.set_spectrum()


@pytest.fixture(scope="module")
def run(dev, tmp_path_factory):
    """one tiny cvc.main run with --val_diversity --val_self_cider over the on-disk fixture dataset (an epoch and its validation pass)"""
    from cvc import main as cvc_main
    from cvc import synth
    from cvc.data_fixture import write_tiny_anet_dataset, CLASSES, VG_CLASSES
    tmp = tmp_path_factory.mktemp("spectrum")
    root = tmp / "anet"
    o = write_tiny_anet_dataset(str(root), seed=7, feat=24, rgb_dim=2048, bn_dim=1024, n_videos=6)
    tables = synth.detectron_tables(synth.Dims(G=24, DET=len(CLASSES)), 7, n_vg=len(VG_CLASSES) + 1)
    wdir = root / "detectron"
    wdir.mkdir()
    for k in ("fc7_w", "fc7_b", "cls_score_w", "cls_score_b"):
        pickle.dump(tables[k], open(wdir / (k + ".pkl"), "wb"))
    argv = ["--no_cfg", "--max_epochs", "1", "--batch_size", "2", "--num_workers", "0", "--seq_per_img", "1",
            "--input_dic", o.input_dic, "--input_json", o.input_json, "--grd_reference", o.grd_reference, "--proposal_h5", o.proposal_h5,
            "--feature_root", o.feature_root, "--seg_feature_root", o.seg_feature_root, "--glove_path", o.glove_path,
            "--vg_vocab_file", o.vg_vocab_file, "--detectron_weights_dir", str(wdir), "--exclude_bgd_det",
            "--num_sampled_frm", "2", "--num_prop_per_frm", "5", "--t_attn_size", "6", "--att_feat_size", "24", "--vis_encoding_size", "24",
            "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "8",
            "--train_split", "training", "--val_split", "validation", "--tensorboard", "0", "--disp_interval", "100",
            "--checkpoint_path", str(tmp) + "/", "--exp_name", "disk", "--learning_rate", "0.001",
            "--results_dir", str(tmp / "results"), "--id", "s1"]
    assert cvc_main.main(argv + ["--val_metrics", "device", "--consensus", "samples", "--consensus_samples", str(N), "--val_diversity",
                                 "--val_self_cider"]) == 0
    tr = cvc_main.LAST_TRAINER
    history = pickle.load(open(tmp / "disk" / "histories_s1.pkl", "rb"))["val_result_history"][0]
    return tr, getattr(tr.model, "module", tr.model), history


DIV = {"Div_1", "Div_2", "mBLEU_4", "Unique", "oracle_CIDEr"}


def test_val_self_cider_puts_both_scores_into_lang_stats_and_they_equal_a_re_decode(run):
    from cvc import metrics
    from cvc.prefetch import DevicePrefetcher
    tr, model, history = run
    assert tr.val_self_cider and tr.val_diversity and "val_self_cider" in vars(tr.opts)
    assert {"Self_CIDEr", "LSA"} <= set(history)                            # written to the history like the other scores
    model._engine_cache = None                                              # (a fresh engine draws the seed's noise again)
    stats = tr.eval(0)
    assert set(stats) == set(metrics.KEYS) | DIV | {"Self_CIDEr", "LSA"}
    assert stats["Self_CIDEr"] == history["Self_CIDEr"] and stats["LSA"] == history["LSA"]      # the weights have not moved
    scorer = metrics.SpectrumScorer(tr._val_cider)
    model._engine_cache = None
    with torch.no_grad():
        for b in DevicePrefetcher(tr.val_loader, lambda raw: tr._prepare(raw, False), tr.device):
            tr._call(b, True)
            cand = model.last_consensus["candidates"]
            assert model.last_consensus.get("live") is None
            scorer.add(cand.reshape(-1, cand.size(-1)), N)
    want = scorer.result()
    print("[spectrum eval] eval %r re-decode %r" % ({k: stats[k] for k in ("Self_CIDEr", "LSA")}, want))
    assert want["Spectrum_sets"] > 0 and 0 <= want["Self_CIDEr"] <= 1 and 0 <= want["LSA"] <= 1
    assert abs(stats["Self_CIDEr"] - want["Self_CIDEr"]) <= 1e-12 and abs(stats["LSA"] - want["LSA"]) <= 1e-12
    # the new switch off: the keys of before
    tr.val_self_cider = False
    try:
        assert set(tr.eval(0)) == set(metrics.KEYS) | DIV
        tr.val_diversity = False
        assert set(tr.eval(0)) == set(metrics.KEYS)
    finally:
        tr.val_diversity = tr.val_self_cider = True


def _entries(out):
    return [e for segs in out.values() for e in segs]


def test_trainer_sample_writes_the_new_keys_and_the_file_of_before_without_them(run):
    from cvc import metrics
    tr, model, _ = run
    n = 3
    model.consensus, model._engine_cache = "off", None
    try:
        on = json.load(open(tr.sample(n, 1.0, seed=5, diversity=True, self_cider=True)))
        summary = on.pop("diversity")
        assert summary == tr.sample_diversity
        assert set(summary) == {"oracle_CIDEr", "mean_CIDEr", *metrics.DIVERSITY_KEYS, "Self_CIDEr", "LSA"}
        entries = _entries(on)
        assert entries and all(set(e["diversity"]) == {"div1", "div2", "mbleu4", "unique", "selfcider", "lsa"} for e in entries)
        assert all(0 <= e["diversity"]["selfcider"] <= 1 and 0 <= e["diversity"]["lsa"] <= 1 for e in entries)
        # the summary is the mean of the entries' scores (every set has n >= 2 live captions; one without a word is not counted)
        worded = [e for e in entries if any(s.split() for s in e["sentences"])]
        assert abs(summary["LSA"] - math.fsum(e["diversity"]["lsa"] for e in worded) / len(worded)) <= 1e-12
        assert abs(summary["Self_CIDEr"] - math.fsum(e["diversity"]["selfcider"] for e in worded) / len(worded)) <= 1e-12
        model._engine_cache = None
        off = json.load(open(tr.sample(n, 1.0, seed=5, diversity=True)))
        assert set(off["diversity"]) == {"oracle_CIDEr", "mean_CIDEr", *metrics.DIVERSITY_KEYS}
        assert all(set(e["diversity"]) == {"div1", "div2", "mbleu4", "unique"} for e in _entries({k: v for k, v in off.items() if k != "diversity"}))
        for e in entries:
            del e["diversity"]["selfcider"], e["diversity"]["lsa"]
        del summary["Self_CIDEr"], summary["LSA"]
        assert off == {**on, "diversity": summary}
        with pytest.raises(RuntimeError, match="needs diversity=True"):
            tr.sample(n, 1.0, self_cider=True)
    finally:
        model.consensus, model._engine_cache = "samples", None
