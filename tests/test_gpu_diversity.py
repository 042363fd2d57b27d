"""cvc_caption_set_stats (csrc/diversity.hip; cvc.metrics.set_diversity, DiversityScorer) against the plain-Python restatement
(tests/diversity_ref.py) and against the route through what existed: cvc.metrics.overlap on references gathered per row.  Integers
exactly, the mBLEU rows bit for bit, the corpus scores against fp64.  Tiny shapes: at most 7 clips of 32 rows of 63 ids."""
import numpy as np
import pytest
import torch

import diversity_ref as D

pytestmark = pytest.mark.gpu

PER_CLIP = (1, 2, 5, 8, 9, 32)          # (8 | 9: the two instantiations; 32 > 16: a wave takes two rows)
TS = (1, 2, 3, 4, 20, 63)               # (T < 4: orders without an n-gram; 63: the last lane)
_cache = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _case(per_clip, T, clips):
    """the case and its reference, computed once"""
    key = (per_clip, T, clips)
    if key not in _cache:
        cand, live = D.case(1000 * per_clip + 10 * T + clips, clips, per_clip, T)
        ms, _ = D.mbleu(cand, per_clip, live)
        _cache[key] = (cand, live, D.set_stats(cand, per_clip, live), ms)
    return _cache[key]


def _gathered_overlap(cand, per_clip, live, dev):
    from cvc import metrics
    refs, nref = D.gathered(cand, per_clip, live)
    ov = metrics.overlap(torch.from_numpy(cand).to(dev), torch.from_numpy(refs).to(dev), torch.from_numpy(nref).to(dev), per_clip=1)
    scored = torch.from_numpy(nref > 0).to(dev).unsqueeze(1)
    return torch.where(scored, ov["stats"], torch.zeros_like(ov["stats"])), torch.where(scored, ov["bleu"], torch.zeros_like(ov["bleu"]))


@pytest.mark.parametrize("clips", [1, 7])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("per_clip", PER_CLIP)
def test_integers_equal_the_reference_and_mbleu_rows_are_overlap_s_bits(dev, per_clip, T, clips):
    from cvc import metrics
    cand, live, st_ref, ms_ref = _case(per_clip, T, clips)
    out = metrics.set_diversity(torch.from_numpy(cand).to(dev), per_clip, torch.from_numpy(live).to(dev))
    assert out["stats"].shape == (clips, 12) and out["stats"].dtype == torch.int32 and out["mbleu_stats"].shape == (clips * per_clip, 10)
    assert out["mbleu"].shape == (clips * per_clip, 4) and out["mbleu"].dtype == torch.float32 and out["div"].shape == (clips, 2)
    assert torch.equal(out["stats"].cpu().long(), torch.from_numpy(st_ref)), (out["stats"].cpu(), st_ref)
    assert torch.equal(out["mbleu_stats"].cpu().long(), torch.from_numpy(ms_ref))
    ov_stats, ov_bleu = _gathered_overlap(cand, per_clip, live, dev)
    assert torch.equal(out["mbleu_stats"], ov_stats)
    assert torch.equal(out["mbleu"].view(torch.int32), ov_bleu.view(torch.int32))
    # div: one correctly rounded fp32 division of two exact integers -- within 1 ulp of the fp64 quotient
    want = D.div(st_ref)
    got = out["div"].cpu().numpy()
    assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all()
    if live.all() and per_clip > 1:                                         # live=None is "every row counts"
        out2 = metrics.set_diversity(torch.from_numpy(cand).to(dev), per_clip)
        assert all(torch.equal(out[k].view(torch.int32), out2[k].view(torch.int32)) for k in out)


def test_no_live_mask_is_all_live(dev):
    from cvc import metrics
    cand, _, _, _ = _case(5, 20, 7)
    out = metrics.set_diversity(torch.from_numpy(cand).to(dev), 5)
    assert torch.equal(out["stats"].cpu().long(), torch.from_numpy(D.set_stats(cand, 5)))
    assert torch.equal(out["mbleu_stats"].cpu().long(), torch.from_numpy(D.mbleu(cand, 5)[0]))
    ov_stats, ov_bleu = _gathered_overlap(cand, 5, None, dev)
    assert torch.equal(out["mbleu_stats"], ov_stats) and torch.equal(out["mbleu"].view(torch.int32), ov_bleu.view(torch.int32))


def test_a_clip_alone_equals_the_clip_in_a_batch_and_two_runs_are_bit_equal(dev):
    from cvc import metrics
    for per_clip, T in ((5, 20), (9, 63), (32, 20)):
        cand, live, _, _ = _case(per_clip, T, 7)
        c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
        a, b = metrics.set_diversity(c, per_clip, l), metrics.set_diversity(c, per_clip, l)
        assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
        for clip in (0, 3, 6):
            rows = slice(clip * per_clip, (clip + 1) * per_clip)
            one = metrics.set_diversity(c[rows].contiguous(), per_clip, l[rows].contiguous())
            assert torch.equal(one["stats"][0], a["stats"][clip]) and torch.equal(one["mbleu_stats"], a["mbleu_stats"][rows])
            assert torch.equal(one["mbleu"].view(torch.int32), a["mbleu"][rows].view(torch.int32))


def test_every_output_is_overwritten(dev):
    from cvc import hip
    for per_clip, T, clips in ((5, 20, 7), (32, 4, 7), (1, 3, 7)):
        cand, live, st_ref, ms_ref = _case(per_clip, T, clips)
        c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
        st = torch.full((clips, 12), -77, dtype=torch.int32, device=dev)
        ms = torch.full((clips * per_clip, 10), -77, dtype=torch.int32, device=dev)
        mb = torch.full((clips * per_clip, 4), float("nan"), device=dev)
        hip._check(hip.lib().cvc_caption_set_stats(c.data_ptr(), l.data_ptr(), clips * per_clip, T, per_clip, st.data_ptr(), ms.data_ptr(),
                                                   mb.data_ptr(), hip._stream()), "cvc_caption_set_stats")
        assert torch.equal(st.cpu().long(), torch.from_numpy(st_ref)) and torch.equal(ms.cpu().long(), torch.from_numpy(ms_ref))
        assert not torch.isnan(mb).any() and (st[:, 11] == 0).all()


def test_graph_replay_on_new_inputs_equals_the_eager_call(dev):
    from cvc import metrics
    per_clip, T, clips = 9, 20, 7
    cand, live, _, _ = _case(per_clip, T, clips)
    cand2, live2 = D.case(99, clips, per_clip, T)
    c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.set_diversity(c, per_clip, l)                               # (warm-up: the library is loaded outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.set_diversity(c, per_clip, l)
    c.copy_(torch.from_numpy(cand2))
    l.copy_(torch.from_numpy(live2))
    g.replay()
    torch.cuda.synchronize()
    eager = metrics.set_diversity(c, per_clip, l)
    assert all(torch.equal(out[k].view(torch.int32), eager[k].view(torch.int32)) for k in out)
    assert torch.equal(out["stats"].cpu().long(), torch.from_numpy(D.set_stats(cand2, per_clip, live2)))


def _table_and_refs(T, clips, dev):
    from cvc.cider import CiderD
    import consensus_ref as C
    rng = np.random.default_rng(17)
    table = CiderD.from_captions([C.clip_candidates(rng, 1, T, 6, garbage=False)[0] for _ in range(100)], dev)
    refs = np.stack([C.clip_candidates(rng, 3, T, 6, garbage=False) for _ in range(clips)])
    nref = rng.integers(1, 4, clips)
    return table, torch.from_numpy(refs).to(dev), torch.from_numpy(nref).to(dev)


def test_scorer_result_against_fp64_and_the_oracle_against_the_host(dev):
    from cvc import metrics
    T = 20
    scorer, stats, mstats, ciders, lives = metrics.DiversityScorer(), [], [], [], []
    for per_clip, clips in ((5, 7), (5, 3)):                                # two batches of the same set size
        cand, live, st_ref, ms_ref = _case(per_clip, T, clips)
        table, refs, nref = _table_and_refs(T, clips, dev)
        c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
        out = scorer.add(c, per_clip, l, refs, nref, table)
        assert torch.equal(out["cider"].view(torch.int32), table.score(c, refs, nref).view(torch.int32))
        stats.append(st_ref), mstats.append(ms_ref), ciders.append(out["cider"].cpu().numpy()), lives.append(live)
    res = scorer.result()
    want = D.result(np.concatenate(stats), np.concatenate(mstats))
    want["oracle_CIDEr"], want["mean_CIDEr"] = D.oracle(np.concatenate(ciders), 5, np.concatenate(lives))
    assert res.keys() == want.keys() and res["Sets"] == 10 and want["mean_CIDEr"] > 0 and want["oracle_CIDEr"] >= want["mean_CIDEr"]
    for k in want:
        assert abs(res[k] - want[k]) <= 1e-12 * abs(want[k]), (k, res[k], want[k])
    ints, fl = scorer.sums()
    other = metrics.DiversityScorer()
    other.add_sums(ints, fl)
    assert other.result() == res
    # without references: the same scores but the oracle's
    plain = metrics.DiversityScorer()
    cand, live, _, _ = _case(5, T, 7)
    plain.add(torch.from_numpy(cand).to(dev), 5, torch.from_numpy(live).to(dev))
    assert set(plain.result()) == set(metrics.DIVERSITY_KEYS)


def test_bad_shapes_are_refused_by_the_library(dev):
    from cvc import hip
    z = torch.zeros(8, 8, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="cvc_caption_set_stats failed: bad argument"):
        hip._check(hip.lib().cvc_caption_set_stats(z.data_ptr(), None, 7, 8, 2, z.data_ptr(), z.data_ptr(), z.data_ptr(), None),
                   "cvc_caption_set_stats")
