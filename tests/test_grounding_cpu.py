"""Grounding F1 of generated captions without a GPU: the restatement (tests/grounding_ref.py) on a hand-worked clip, number by number;
cvc.metrics.grounding_result on hand-made tables; cvc.misc.utils.word_class_table against Trainer._collect_grounding's per-word rule;
the guard for the GPU cases (the restatement alone must see hits AND misses on them); the block's declaration and host-side refusals."""
import ctypes
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grounding_ref as R

INF = float("inf")


def hand_worked_clip():
    """2 frames x 3 proposals, one caption "a man dog men bike" (men: the class of man again), four annotated boxes in five rows:
    words 2 / 6 -> class 1 (man), 3 -> 2 (dog), 4 -> 3 (ball), 5 -> 4 (bike), 7 -> 5 (woman)"""
    word_cls = np.array([0, 0, 1, 2, 3, 4, 1, 5, 0, 0], dtype=np.int32)
    seq = np.array([[1, 2, 3, 6, 5, 0, 2, 2]], dtype=np.int64)                       # (what stands behind the 0 is ignored)
    ppls = np.zeros((1, 6, 7), dtype=np.float32)
    ppls[0, :, :4] = [[0, 0, 100, 100], [200, 200, 300, 300], [50, 50, 150, 150],   # frame 0
                      [0, 0, 100, 100], [10, 10, 110, 110], [400, 400, 500, 500]]   # frame 1
    att = np.full((1, 8, 6), 0.1, dtype=np.float32)
    att[0, 1] = [.5, .2, .3, .1, .6, .3]             # man: slot 0, slot 4
    att[0, 2] = [.1, .4, .4, .2, .2, .7]             # dog: equal maxima in frame 0 -> slot 1; slot 5
    att[0, 3] = [.1, .2, .9, .1, .1, .8]             # men: slot 2, slot 5 -- NOT the representative of class 1
    att[0, 4] = [.7, .2, .1, -INF, -INF, -INF]       # bike: slot 0; a frame of -inf -> its first slot, 3
    gt = np.zeros((1, 6, 6), dtype=np.float32)
    gt[0] = [[0, 0, 100, 100, 0, 1],                 # man in frame 0: the representative's pick, slot 0 (men's slot 2 would miss)
             [10, 10, 110, 110, 1, 1],               # a multi-label box, man ..
             [10, 10, 110, 110, 1, 5],               # .. and woman, which the caption does not predict
             [200, 200, 300, 250, 0, 2],             # dog: half of slot 1 -> IoU exactly 1/2: a miss
             [0, 0, 10, 10, 1, 3],                   # ball: not predicted
             [0, 0, 100, 100, 0, 1]]                 # behind nbox: does not count
    return dict(seq=seq, att=att, ppls=ppls, gt_bboxs=gt, nbox=np.array([5], dtype=np.int32), word_cls=word_cls, frames=2, n_per=3,
                n_classes=5, per_clip=1)


def test_hand_worked_clip_number_by_number():
    out = R.score_batch(**hand_worked_clip())
    want_pick = np.full((8, 2), -1)
    want_pick[1], want_pick[2], want_pick[3], want_pick[4] = [0, 4], [1, 5], [2, 5], [0, 3]
    assert np.array_equal(out["pick"][0], want_pick)
    #                                gt gt_pred gt_hit pred pred_in_gt pred_hit
    assert out["table"].tolist() == [[0, 0, 0, 0, 0, 0],
                                     [2, 2, 2, 1, 1, 1],         # man: both boxes hit by the representative
                                     [1, 1, 0, 1, 1, 0],         # dog: IoU 1/2 is a miss
                                     [1, 0, 0, 0, 0, 0],         # ball: annotated, not predicted
                                     [0, 0, 0, 1, 0, 0],         # bike: predicted, not annotated
                                     [1, 0, 0, 0, 0, 0]]         # woman: the multi-label box's second class
    assert out["counts"].tolist() == [[5, 3, 2, 3, 2, 1]]
    assert out["f1"][0] == pytest.approx(4.0 / 11.0, abs=1e-15)                  # P = 1/3, R = 2/5
    res = R.result(out["table"])
    want = {"Prec_all": 0.25, "Recall_all": 0.25, "F1_all": 0.25, "Prec_loc": 0.5, "Recall_loc": 0.5, "F1_loc": 0.5,
            "F1_all_micro": 4.0 / 11.0, "F1_loc_micro": 4.0 / 7.0}
    assert set(res) == set(R.KEYS) == set(want)
    for k, v in want.items():
        assert res[k] == pytest.approx(v, abs=1e-15), k
    # the representative matters: with men in front of man, class 1's pick in frame 0 is slot 2, which misses box 0
    c = hand_worked_clip()
    c["seq"][0, 1], c["seq"][0, 3] = 6, 2
    c["att"][0, [1, 3]] = c["att"][0, [3, 1]]
    assert R.score_batch(**c)["table"][1].tolist() == [2, 2, 0, 1, 1, 0]


def test_hit_rule():
    assert R.hit([0, 0, 100, 100], [0, 0, 100, 100])
    assert not R.hit([0, 0, 100, 100], [0, 0, 50, 100])                          # exactly 1/2
    assert R.hit([0, 0, 100, 100], [0, 0, 51, 100])
    assert not R.hit([0, 0, 100, 100], [100, 0, 200, 100])                       # touching: w = 0
    assert not R.hit([0, 0, 0, 0], [0, 0, 0, 0])                                 # the zero box of a trimmed slot
    assert R.frame_pick(np.array([-INF, -INF, 1.0, -INF], dtype=np.float32), 1, 2, 3) == 2       # slot 3 >= P: -inf
    assert R.frame_pick(np.array([np.nan, np.nan, 0.5, 0.5], dtype=np.float32), 0, 2, 4) == 0
    assert R.frame_pick(np.array([0.0, 0.0, 0.5, 0.5], dtype=np.float32), 1, 2, 4) == 2


def test_grounding_result_on_hand_made_tables():
    from cvc import metrics
    assert metrics.GROUNDING_COLUMNS == R.COLUMNS and metrics.GROUNDING_KEYS == R.KEYS
    zero = metrics.grounding_result(np.zeros((4, 6), dtype=np.int64))                              # an empty table
    assert set(zero) == set(R.KEYS) and all(v == 0.0 for v in zero.values())
    t = np.array([[0, 0, 0, 0, 0, 0], [4, 2, 1, 2, 2, 1], [3, 0, 0, 0, 0, 0], [0, 0, 0, 5, 0, 0]])   # class 2 never predicted, 3 never annotated
    got = metrics.grounding_result(torch.from_numpy(t))
    assert got["Prec_all"] == pytest.approx((0.5 + 0.0) / 2) and got["Recall_all"] == pytest.approx((0.25 + 0.0) / 2)
    assert got["Prec_loc"] == pytest.approx(0.5) and got["Recall_loc"] == pytest.approx(0.5)
    assert got["F1_all"] == pytest.approx(2 * 0.25 * 0.125 / 0.375) and got["F1_loc"] == pytest.approx(0.5)
    assert got["F1_all_micro"] == pytest.approx(2 * (1 / 7) * (1 / 7) / (2 / 7)) and got["F1_loc_micro"] == pytest.approx(0.5)
    none_hit = metrics.grounding_result(np.array([[0] * 6, [3, 3, 0, 2, 2, 0]]))                   # P + R = 0
    assert none_hit["F1_all"] == 0.0 and none_hit["F1_loc"] == 0.0 and none_hit["F1_all_micro"] == 0.0 and none_hit["F1_loc_micro"] == 0.0
    rng = np.random.default_rng(0)
    for _ in range(20):
        t = np.sort(rng.integers(0, 9, (7, 6)), axis=1)[:, ::-1] * (rng.random((7, 1)) < 0.7)
        got, want = metrics.grounding_result(t), R.result(t)
        for k in R.KEYS:
            assert got[k] == pytest.approx(want[k], abs=1e-15), (k, t)


def test_scorer_merges_tables_on_the_host():
    from cvc import metrics
    s = metrics.GroundingScorer(torch.zeros(5, dtype=torch.int32), 3, 2)
    assert s.sums().tolist() == [[0] * 6] * 4 and all(v == 0.0 for v in s.result().values())
    a, b = np.arange(24).reshape(4, 6), np.ones((4, 6), dtype=np.int64)
    s.add_sums(a)
    s.add_sums(torch.from_numpy(b))
    assert np.array_equal(s.sums(), a + b) and s.result() == metrics.grounding_result(a + b)


def test_word_class_table_is_the_per_word_rule_of_collect_grounding(tmp_path):
    from cvc.data_fixture import write_tiny_anet_dataset, WORDS, CLASSES
    from cvc.misc.dataloader_anet import ANetEntitiesDataset
    from cvc.misc import utils
    o = write_tiny_anet_dataset(str(tmp_path / "anet"), seed=7)
    ds = ANetEntitiesDataset(o, split="training", seq_per_img=1)
    opts = SimpleNamespace(**{k: getattr(ds, k) for k in ("wtol", "wtod", "itow", "itod", "vocab_size")})
    table = utils.word_class_table(opts)
    assert table.dtype == torch.int32 and tuple(table.shape) == (ds.vocab_size,) and int(table[0]) == 0
    lemma_det = {opts.wtol[k]: i for k, i in opts.wtod.items() if k in opts.wtol}                   # Trainer._collect_grounding
    n_obj = 0
    for w in range(1, ds.vocab_size):
        lemma = opts.wtol[opts.itow[str(w)]]
        want = lemma_det[lemma] if lemma in lemma_det else 0
        assert int(table[w]) == want, (w, opts.itow[str(w)])
        if want:
            assert opts.itod[want] == opts.itow[str(w)]
            n_obj += 1
    assert n_obj == len(CLASSES) and len(WORDS) + 1 == ds.vocab_size
    # a lemma table that folds two words into one class, and a class name that is no word of the vocabulary
    o2 = SimpleNamespace(wtol={"man": "man", "men": "man", "dog": "dog", "a": "a"}, wtod={"man": 1, "dog": 2, "zebra": 3},
                         itow={"1": "a", "2": "men", "3": "dog", "4": "man", "5": "xyz"}, vocab_size=6)
    assert utils.word_class_table(o2).tolist() == [0, 0, 1, 2, 1, 0]


def test_the_gpu_cases_hold_hits_and_misses():
    """the guard for tests/test_gpu_grounding.py: by the restatement alone, the case list's six column sums are > 0 with
    pred_hit < pred_in_gt < pred and gt_hit < gt_pred < gt -- a kernel that returns zeros, or that hits everything, cannot pass; the
    special inputs the list promises are really in it"""
    total = np.zeros(6, dtype=np.int64)
    seen = dict(tie=0, inf_frame=0, no_zero=0, first_zero=0, big_id=0, nbox0=0, nboxK=0, frame_neg=0, frame_big=0, trimmed_pick=0)
    for key in R.CASES:
        inp, out = R.case(key)
        rows, per_clip, T, F, Np, P, K, C, V = key
        s = out["table"].sum(0)
        print(f"[grounding] case {key}: column sums {s.tolist()}, object words {int((out['pick'][:, :, 0] >= 0).sum())}")
        assert np.array_equal(out["counts"].sum(0), s) and out["table"][0].sum() == 0
        if K == 100:                                                       # (the cases with a handful of boxes add to the total)
            gt, gt_pred, gt_hit, pred, pred_in_gt, pred_hit = s.tolist()
            assert 0 < pred_hit < pred_in_gt < pred and 0 < gt_hit < gt_pred < gt, key
        total += s
        seq, att, nbox, gtb = inp["seq"], inp["att"], inp["nbox"], inp["gt_bboxs"]
        seen["no_zero"] += int((seq != 0).all(1).sum())
        seen["first_zero"] += int((seq[:, 0] == 0).sum())
        seen["big_id"] += int((seq >= V).sum())
        seen["nbox0"] += int((nbox == 0).sum())
        seen["nboxK"] += int((nbox == K).sum() if K == 100 else 0)
        for b in range(len(nbox)):
            seen["frame_neg"] += int((gtb[b, :nbox[b], 4] < 0).sum())
            seen["frame_big"] += int((gtb[b, :nbox[b], 4] >= F).sum())
        seen["trimmed_pick"] += int((out["pick"] >= P).sum())
        for r, t in zip(*np.nonzero(out["pick"][:, :, 0] >= 0)):
            for f in range(F):
                w = att[r, t, f * Np:min((f + 1) * Np, P)]
                if w.size and np.isneginf(w).all():
                    seen["inf_frame"] += 1
                elif w.size and (w == w.max()).sum() > 1:
                    seen["tie"] += 1
    gt, gt_pred, gt_hit, pred, pred_in_gt, pred_hit = total.tolist()
    print(f"[grounding] all cases: column sums {total.tolist()}; {seen}")
    assert 0 < pred_hit < pred_in_gt < pred and 0 < gt_hit < gt_pred < gt
    assert all(v > 0 for v in seen.values()), seen
    assert {(k[3], k[4]) for k in R.CASES} == {(2, 5), (3, 64), (2, 70), (10, 100)}
    assert {k[2] for k in R.CASES} >= {8, 63} and {k[0] for k in R.CASES} >= {1, 5, 64} and {k[1] for k in R.CASES} == {1, 3}


def test_block_declared_listed_bound_and_not_exported():
    import build_hip
    from cvc import hip
    from test_cabi import declared_functions, BLOCKS_H
    n = "cvc_grounding_f1"
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    assert n in declared_functions(BLOCKS_H) and n in hip.BLOCKS and n in hip.SIGNATURES
    assert lib.cvc_block(n.encode())
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip.build(verbose=False)], text=True)
    assert n not in {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_bad_arguments_return_before_any_launch():
    from cvc import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # non-null; never dereferenced: every call below is refused on the host

    def call(rows=6, T=8, P=10, F=2, Np=5, K=4, C=3, V=9, per=3, **null):
        ptr = {k: (None if k in null else p) for k in ("seq", "att", "ppls", "gt", "nbox", "word_cls", "pick", "counts", "f1", "table")}
        return lib.cvc_grounding_f1(ptr["seq"], ptr["att"], ptr["ppls"], ptr["gt"], ptr["nbox"], ptr["word_cls"], rows, T, P, F, Np, K, C, V,
                                    per, ptr["pick"], ptr["counts"], ptr["f1"], ptr["table"], None)
    for k in ("seq", "att", "ppls", "gt", "nbox", "word_cls", "pick", "counts", "f1", "table"):
        assert call(**{k: None}) == -1, k
    assert call(rows=0) == -1 and call(rows=7) == -1 and call(per=0) == -1
    assert call(T=0) == -1 and call(T=64) == -1
    assert call(P=0) == -1 and call(P=11) == -1                            # more slots than F * Np
    assert call(F=0) == -1 and call(Np=0) == -1 and call(K=0) == -1 and call(C=0) == -1 and call(V=0) == -1
    assert call(F=1 << 20, Np=1 << 12) == -1                               # F * Np overflows an int
    assert call(T=63, F=200, Np=1, P=200) == -2 and call(K=5000) == -2     # the picks / the boxes do not fit the kernel's LDS


def test_wrappers_refuse_what_does_not_fit():
    from cvc import hip, metrics
    seq, att = torch.zeros(6, 8, dtype=torch.int64), torch.zeros(6, 8, 10)
    ppls, gt, nbox = torch.zeros(2, 10, 7), torch.zeros(2, 4, 6), torch.zeros(2, dtype=torch.int32)
    wc, table = torch.zeros(9, dtype=torch.int32), torch.zeros(4, 6, dtype=torch.int32)
    ok = dict(seq=seq, att=att, ppls=ppls, gt_bboxs=gt, nbox=nbox, word_cls=wc, frames=2, table=table)
    bad = [dict(att=att[:, :7]), dict(att=att[:, :, :9]), dict(ppls=ppls[:, :, :6]), dict(gt_bboxs=gt[:1]), dict(gt_bboxs=gt[:, :, :5]),
           dict(nbox=nbox[:1]), dict(table=table[:1]), dict(table=table[:, :5]), dict(frames=0), dict(word_cls=wc.view(3, 3))]
    for kw in bad:
        with pytest.raises(RuntimeError, match="do not fit"):
            hip.grounding_f1(**{**ok, **kw})
    with pytest.raises(RuntimeError, match="per clip"):
        hip.grounding_f1(**{**ok, "seq": seq[:5], "att": att[:5]})
    with pytest.raises(RuntimeError, match="props_per_frame"):
        hip.grounding_f1(**{**ok, "frames": 3})                            # 10 slots are not 3 equal frames
    with pytest.raises(RuntimeError, match="do not fit 2 frames of 4"):
        hip.grounding_f1(**ok, props_per_frame=4)
    with pytest.raises(RuntimeError, match="GPU"):                         # no CPU fallback
        hip.grounding_f1(**ok)
    with pytest.raises(RuntimeError, match="T = 63"):
        metrics.grounding(torch.zeros(2, 64, dtype=torch.int64), torch.zeros(2, 64, 10), ppls, gt, nbox, wc, 2, table=table)
    with pytest.raises(RuntimeError, match="table must be"):
        metrics.grounding(seq, att, ppls, gt, nbox, wc, 2, table=table[:1])
