"""Caption-set diversity without a GPU: the plain-Python restatement (tests/diversity_ref.py) on hand-worked cases and against the
overlap restatement, the result() formulae of cvc.metrics from given sums, the command line, the block's declaration and host-side
refusals, and Trainer.sample's refusal of a set of one."""
import ctypes
import math
import subprocess

import numpy as np
import pytest
import torch

import diversity_ref as D
import overlap_ref as O

A, B, C = 7, 8, 9


def test_hand_worked_two_rows():
    cand = np.array([[A, B, A, B, 0], [A, B, C, 0, A]])                     # "a b a b" / "a b c" (+ garbage behind the end mark)
    st = D.set_stats(cand, 2)[0]
    # 1-grams a b c; 2-grams ab ba bc; 3-grams aba bab abc; 4-grams abab
    assert st.tolist() == [3, 3, 3, 1, 7, 5, 3, 1, 2, 2, 2, 0]
    assert D.div(st.reshape(1, 12))[0].tolist() == [3 / 7, 3 / 7]
    ms, mb = D.mbleu(cand, 2)
    assert ms[0].tolist() == [2, 1, 0, 0, 4, 3, 2, 1, 4, 3]                  # a and b clipped to one each; ab once
    assert ms[1].tolist() == [2, 1, 0, 0, 3, 2, 1, 0, 3, 4]


def test_duplicate_pair_is_one_caption_with_mbleu_at_its_maximum():
    cand = np.array([[A, B, C, A, 0, 0], [A, B, C, A, 0, 5]])
    st = D.set_stats(cand, 2)[0]
    assert st[8] == 2 and st[9] == 1 and st[10] == 2 and st[:4].tolist() == [3, 3, 2, 1] and st[4:8].tolist() == [8, 6, 4, 2]
    ms, mb = D.mbleu(cand, 2)
    for r in range(2):
        assert ms[r].tolist() == [4, 3, 2, 1, 4, 3, 2, 1, 4, 4]
        assert np.allclose(mb[r], 1.0, rtol=0, atol=1e-9)
    assert abs(D.result(st.reshape(1, 12), ms)["mBLEU_4"] - 1.0) < 1e-9 and D.result(st.reshape(1, 12), ms)["Unique"] == 0.5


def test_live_mask_and_degenerate_sets():
    cand = np.array([[A, B, 0], [A, B, 0], [C, 0, 0], [0, A, A]])
    st = D.set_stats(cand, 4, [1, 0, 1, 1])[0]
    assert st.tolist() == [3, 1, 0, 0, 3, 1, 0, 0, 3, 3, 3, 0]               # the dead duplicate counts nowhere; L = 0 is a caption
    ms, _ = D.mbleu(cand, 4, [1, 0, 1, 1])
    assert not ms[1].any() and ms[3].tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    one = D.set_stats(cand, 4, [0, 0, 1, 0])[0]
    assert one[8:11].tolist() == [1, 1, 0] and not D.mbleu(cand, 4, [0, 0, 1, 0])[0].any()
    none = D.set_stats(cand, 4, [0, 0, 0, 0])[0]
    assert not none.any() and D.div(none.reshape(1, 12)).tolist() == [[0.0, 0.0]]
    assert D.set_stats(cand, 1)[:, 10].tolist() == [0, 0, 0, 0] and not D.mbleu(cand, 1)[0].any()


@pytest.mark.parametrize("per_clip,T", [(2, 3), (5, 8), (9, 20)])
def test_mbleu_rows_are_the_overlap_restatement_on_gathered_references(per_clip, T):
    cand, live = D.case(11 + per_clip, 4, per_clip, T)
    ms, mb = D.mbleu(cand, per_clip, live)
    refs, nref = D.gathered(cand, per_clip, live)
    for r in range(len(cand)):
        o = O.score_batch(cand[r:r + 1], refs[r:r + 1], nref[r:r + 1])
        if nref[r] == 0:
            assert not ms[r].any() and not mb[r].any()
        else:
            assert ms[r].tolist() == o["stats"][0].tolist() and mb[r].tolist() == o["bleu"][0].tolist()
    st = D.set_stats(cand, per_clip, live)
    assert (st[:, 8] == live.reshape(-1, per_clip).sum(1)).all() and (st[:, 9] <= st[:, 8]).all() and (st[:, :4] <= st[:, 4:8]).all()


def test_generator_makes_its_kinds():
    cand, live = D.case(3, 7, 9, 20)
    L = np.array([len(O.words(r)) for r in cand])
    assert (L == 0).any() and (L == 20).any() and cand.max() > 60000 and cand[:9].max() <= 5
    assert live.reshape(7, 9)[1].sum() == 0 and live.reshape(7, 9)[2].sum() == 1 and live.reshape(7, 9)[0].all()
    st = D.set_stats(cand, 9)
    assert (st[:, 9] < st[:, 8]).any()                                       # identical rows
    assert any(r[len(O.words(r)) + 1:].any() for r in cand if len(O.words(r)) < 19)       # garbage behind the end mark


def test_result_formulae_from_given_sums():
    from cvc import metrics
    mb = [30, 20, 10, 5, 40, 36, 32, 28, 40, 44]
    ints = mb + [6, 8, 2]
    res = metrics.diversity_from_sums(ints, [0.9, 0.5, 2.0, 3.0, 2.0, 8.0, 8.0])
    assert res["Div_1"] == 0.45 and res["Div_2"] == 0.25 and res["Unique"] == 0.75 and res["Sets"] == 2
    assert res["oracle_CIDEr"] == 1.5 and res["mean_CIDEr"] == 1.0
    bleu = metrics.corpus_bleu(mb)
    assert [res["mBLEU_%d" % k] for k in (1, 2, 3, 4)] == [float(x) for x in bleu]
    assert np.allclose(bleu, O.corpus(mb), rtol=1e-15, atol=0)
    bp = math.exp(1 - 44 / 40)
    assert abs(res["mBLEU_1"] - bp * 30 / 40) < 1e-9
    no_refs = metrics.diversity_from_sums(ints, [0.9, 0.5, 2.0, 0, 0, 0, 0])
    assert "oracle_CIDEr" not in no_refs and "mean_CIDEr" not in no_refs and set(no_refs) == set(metrics.DIVERSITY_KEYS)
    empty = metrics.DiversityScorer().result()
    assert empty == {**{k: 0.0 for k in metrics.DIVERSITY_KEYS}, "Sets": 0}


def test_scorer_merges_sums_on_the_host():
    from cvc import metrics
    s = metrics.DiversityScorer()
    s.add_sums(list(range(13)), [0.5, 0.25, 1, 0, 0, 0, 0])
    s.add_sums(torch.arange(13), [0.5, 0.25, 1, 2.0, 1, 3.0, 2])
    ints, fl = s.sums()
    assert ints == [2 * i for i in range(13)] and fl == [1.0, 0.5, 2.0, 2.0, 1.0, 3.0, 2.0]
    assert s.result() == metrics.diversity_from_sums(ints, fl)
    ref = D.result(np.array([[3, 3, 3, 1, 7, 5, 3, 1, 2, 2, 2, 0]]), np.array([[2, 1, 0, 0, 4, 3, 2, 1, 4, 3], [2, 1, 0, 0, 3, 2, 1, 0, 3, 4]]))
    got = metrics.diversity_from_sums([4, 2, 0, 0, 7, 5, 3, 1, 7, 7, 2, 2, 1], [3 / 7, 3 / 7, 1.0, 0, 0, 0, 0])
    assert got.keys() == ref.keys() and all(abs(got[k] - ref[k]) <= 1e-12 * abs(ref[k]) for k in ref)


def test_command_line():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    from cvc import sample as cvc_sample
    o = cvc_main.build_parser().parse_args([])
    assert not hasattr(o, "val_diversity")                                   # default off: no key in the options
    cvc_main.check_val_diversity_flag(o)
    assert not hasattr(cvc_opts.build_parser().parse_args([]), "val_diversity")
    ok = cvc_main.build_parser().parse_args(["--val_diversity", "--val_metrics", "device", "--consensus", "samples"])
    assert ok.val_diversity is True
    cvc_main.check_val_diversity_flag(ok)
    cvc_main.check_val_diversity_flag(cvc_main.build_parser().parse_args(["--val_diversity", "--val_metrics", "device", "--consensus", "beam"]))
    with pytest.raises(SystemExit, match="--val_metrics device"):
        cvc_main.check_val_diversity_flag(cvc_main.build_parser().parse_args(["--val_diversity", "--consensus", "samples"]))
    with pytest.raises(SystemExit, match="--consensus samples"):
        cvc_main.check_val_diversity_flag(cvc_main.build_parser().parse_args(["--val_diversity", "--val_metrics", "device"]))
    with pytest.raises(SystemExit, match="--val_metrics device"):           # the run ends before any set-up (no GPU is looked for)
        cvc_main.main(["--no_cfg", "--val_diversity"])
    own, rest = cvc_sample.parse(["--sample_n", "4", "--diversity", "--no_cfg"])
    assert own.diversity and own.sample_n == 4 and rest == ["--no_cfg"]
    assert not cvc_sample.parse([])[0].diversity
    own, _ = cvc_sample.parse(["--sample_n", "3", "--diversity", "--without_replacement", "--consensus"])
    assert own.diversity and own.without_replacement and own.consensus
    with pytest.raises(SystemExit, match="--diversity needs --sample_n > 1"):
        cvc_sample.parse(["--sample_n", "1", "--diversity"])


def test_block_declared_listed_bound_and_not_exported():
    import build_hip
    from cvc import hip
    from test_cabi import declared_functions, BLOCKS_H
    n = "cvc_caption_set_stats"
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    assert n in declared_functions(BLOCKS_H) and n in hip.BLOCKS and n in hip.SIGNATURES and callable(hip.caption_set_stats)
    assert lib.cvc_block(n.encode())
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip.build(verbose=False)], text=True)
    assert n not in {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_bad_arguments_return_badarg_before_any_launch():
    from cvc import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # non-null; never dereferenced: every call below is refused on the host

    def call(cand=p, live=None, rows=6, T=5, per=3, set_stats=p, mbleu_stats=p, mbleu=p):
        return lib.cvc_caption_set_stats(cand, live, rows, T, per, set_stats, mbleu_stats, mbleu, None)
    assert call(cand=None) == -1 and call(set_stats=None) == -1 and call(mbleu_stats=None) == -1 and call(mbleu=None) == -1
    assert call(per=0) == -1 and call(rows=33, per=33) == -1
    assert call(T=0) == -1 and call(T=64) == -1
    assert call(rows=7) == -1 and call(rows=0) == -1                       # rows % per_clip != 0


def test_wrappers_refuse_what_does_not_fit():
    from cvc import hip, metrics
    cand = torch.zeros(6, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.caption_set_stats(cand, 4)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.caption_set_stats(cand, 3, live=torch.ones(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):                         # no CPU fallback
        metrics.set_diversity(cand, 3)
    with pytest.raises(RuntimeError, match="T = 63"):
        metrics.set_diversity(torch.zeros(4, 64, dtype=torch.int64), 2)
    with pytest.raises(RuntimeError, match="per_clip = 32"):
        metrics.set_diversity(torch.zeros(66, 5, dtype=torch.int64), 33)
    with pytest.raises(RuntimeError, match="go together"):
        metrics.DiversityScorer().add(cand, 3, refs=torch.zeros(2, 1, 3, dtype=torch.int64))


def test_trainer_sample_refuses_a_set_of_one():
    from cvc.trainer import Trainer
    tr = Trainer.__new__(Trainer)                # the refusal comes before anything of the trainer is touched but its model
    tr.model = torch.nn.Linear(1, 1)
    with pytest.raises(RuntimeError, match="n > 1 captions per segment"):
        tr.sample(1, 1.0, diversity=True)
