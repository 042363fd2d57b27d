"""The restatement of BLEU / ROUGE-L (tests/overlap_ref.py) against hand-checked anchors, and the host side of cvc.metrics: corpus_bleu,
DeviceScorer's sums on CPU tensors, the --scst_reward parser.  No GPU.  Every test prints its figures before it asserts."""
import math

import numpy as np
import pytest
import torch

import overlap_ref as R

VOCAB = {}


def ids(sentence, T=None, pad=0):
    """words -> ids from 1 on (a private vocabulary), 0-terminated and padded to T when T is given"""
    out = [VOCAB.setdefault(w, len(VOCAB) + 1) for w in sentence.split()]
    if T is not None:
        out = out + [0] + [pad] * (T - len(out) - 1)
        out = out[:T]
    return out


def test_the_times_seven():
    cand = ids("the the the the the the the")
    refs = [ids("the cat is on the mat"), ids("there is a cat on the mat")]
    st = R.bleu_stats(cand, refs)
    b = R.bleu_from_stats(st)
    print(f"[overlap ref] the x 7: stats {st}, BLEU {[float(x) for x in b]}")
    assert st[0] == 2 and st[4] == 7 and st[1] == 0 and st[5] == 6 and st[8] == 7 and st[9] == 7
    assert abs(float(b[0]) - 2.0 / 7.0) < 1e-9


def test_bleu_from_given_statistics():
    b = [float(x) for x in R.bleu_from_stats([5, 3, 2, 1, 6, 5, 4, 3, 6, 7])]
    print(f"[overlap ref] (5,3,2,1 | 6,5,4,3 | 6 | 7): BLEU {b}")
    np.testing.assert_allclose(b, [0.705401, 0.598553, 0.533250, 0.454802], rtol=0, atol=5e-7)
    b32 = [float(x) for x in R.bleu_from_stats([5, 3, 2, 1, 6, 5, 4, 3, 6, 7], True, np.float32)]
    assert all(isinstance(x, np.float32) for x in R.bleu_from_stats([5, 3, 2, 1, 6, 5, 4, 3, 6, 7], True, np.float32))
    np.testing.assert_allclose(b32, b, rtol=0, atol=1e-6)


def test_rouge_l_anchors():
    ref = [ids("police kill the gunman")]
    a, la = R.rouge_l(ids("police killed the gunman"), ref)
    b, lb = R.rouge_l(ids("the gunman police killed"), ref)
    print(f"[overlap ref] ROUGE-L {float(a)} (lcs {la}), {float(b)} (lcs {lb})")
    assert la == [3] and abs(float(a) - 0.75) < 1e-12
    assert lb == [2] and abs(float(b) - 0.5) < 1e-12
    assert R.lcs([], [1, 2]) == 0 and R.lcs([1, 2, 3], [1, 2, 3]) == 3 and R.lcs([1, 2, 3], [3, 2, 1]) == 1


def test_length_tie_takes_the_shorter_reference():
    st = R.bleu_stats([1, 2, 3, 4, 5, 0], [[9, 9, 9, 9, 0, 0, 0], [9, 9, 9, 9, 9, 9, 0]])
    print(f"[overlap ref] Lc 5, references of 4 and 6 words: ref_len {st[9]}")
    assert st[8] == 5 and st[9] == 4
    assert R.bleu_stats([1, 2, 3, 4, 5, 0], [[9, 9, 9, 9, 9, 9, 0], [9, 9, 9, 9, 0, 0, 0]])[9] == 4


def test_empty_candidate_and_no_reference():
    out = R.score_batch([[0, 3, 4, 5], [3, 4, 5, 0]], [[[3, 4, 5, 0]], [[3, 4, 5, 0]]], [1, 0])
    print(f"[overlap ref] Lc = 0: {out['stats'][0].tolist()} {out['bleu'][0].tolist()} {out['rouge'][0]}; no reference: "
          f"{out['stats'][1].tolist()} {out['bleu'][1].tolist()} {out['rouge'][1]}")
    assert out["stats"][0].tolist() == [0] * 9 + [3] and not out["bleu"][0].any() and out["rouge"][0] == 0.0 and out["lcs"][0, 0] == 0
    assert out["stats"][1].tolist() == [0, 0, 0, 0, 3, 2, 1, 0, 3, 0] and not out["bleu"][1].any() and out["rouge"][1] == 0.0
    assert out["lcs"][1, 0] == -1


def test_words_behind_the_end_mark_change_nothing():
    T = 9
    a = R.score_batch([ids("a man is cooking", T)], [[ids("a man is cooking food", T), ids("man cooking", T)]], [2])
    b = R.score_batch([ids("a man is cooking", T, pad=VOCAB["man"])], [[ids("a man is cooking food", T, pad=VOCAB["a"]),
                                                                         ids("man cooking", T, pad=7)]], [2])
    print(f"[overlap ref] stats {a['stats'][0].tolist()}, BLEU {a['bleu'][0].tolist()}, ROUGE-L {a['rouge'][0]}")
    for k in ("stats", "lcs", "bleu", "rouge"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["stats"][0].tolist() == [4, 3, 2, 1, 4, 3, 2, 1, 4, 5] and a["lcs"][0].tolist() == [4, 2]


def test_corpus_bleu_of_one_row_is_its_sentence_bleu():
    from cvc import metrics
    for st in ([5, 3, 2, 1, 6, 5, 4, 3, 6, 7], [2, 0, 0, 0, 7, 6, 5, 4, 7, 7], [3, 2, 1, 0, 3, 2, 1, 0, 3, 3]):
        got, want = metrics.corpus_bleu(torch.tensor(st)), np.array([float(x) for x in R.bleu_from_stats(st)])
        print(f"[metrics] corpus_bleu{tuple(st)} = {got.tolist()}, restatement {want.tolist()}")
        assert got.dtype == np.float64
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert not metrics.corpus_bleu([0] * 10).any()


def test_device_scorer_sums_on_cpu_tensors():
    from cvc import metrics
    s = metrics.DeviceScorer(None)
    a, b = [5, 3, 2, 1, 6, 5, 4, 3, 6, 7], [2, 0, 0, 0, 7, 6, 5, 4, 7, 7]
    s.add_sums(torch.tensor(a), 0.75, 3.0, 1)
    s.add_sums(torch.tensor(b, dtype=torch.int32), torch.tensor(0.5), torch.tensor([1.0]), 3)
    res = s.result()
    want = R.corpus([x + y for x, y in zip(a, b)])
    print(f"[metrics] DeviceScorer on the CPU: {res}")
    assert list(res) == ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"] and all(isinstance(v, float) for v in res.values())
    np.testing.assert_allclose([res["Bleu_%d" % k] for k in (1, 2, 3, 4)], want, rtol=1e-12, atol=0)
    assert res["ROUGE_L"] == 1.25 / 4 and res["CIDEr"] == 1.0
    assert s.sums() == ([x + y for x, y in zip(a, b)], 1.25, 4.0, 4.0)
    empty = metrics.DeviceScorer(None).result()
    assert all(v == 0.0 for v in empty.values()) and len(empty) == 6


def test_scst_reward_parser():
    from cvc import metrics
    from cvc.main import build_parser
    default = metrics.parse_reward_weights(build_parser().parse_args([]).scst_reward)
    mix = metrics.parse_reward_weights("rougel:0.5, cider:1,bleu4:0.5")
    print(f"[metrics] --scst_reward default {default}, mix {mix}")
    assert default == {"cider": 1.0} and metrics.is_cider_only(default) and metrics.is_cider_only(None)
    assert list(mix.items()) == [("cider", 1.0), ("bleu4", 0.5), ("rougel", 0.5)] and not metrics.is_cider_only(mix)
    assert metrics.is_cider_only(metrics.parse_reward_weights("cider:1,bleu2:0"))
    assert not metrics.is_cider_only(metrics.parse_reward_weights("cider:2")) and not metrics.is_cider_only({"bleu4": 1.0})
    assert build_parser().parse_args([]).val_metrics == "none"
    for bad in ("meteor:1", "cider:-1", "bleu5:1", "cider:x", "", "cider:1,cider:2", "rougel:nan"):
        with pytest.raises(SystemExit):
            metrics.parse_reward_weights(bad)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--val_metrics", "toolkit"])
