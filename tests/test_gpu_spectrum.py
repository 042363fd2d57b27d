"""cvc_caption_set_spectrum (csrc/spectrum.hip; cvc.metrics.set_spectrum, SpectrumScorer) against the numpy restatement
(tests/spectrum_ref.py): the similarity matrix exactly (lsa) / within the float32 restatement's own error (cider), the eigenvalues
against eigvalsh of the kernel's own matrix, the scores against their fp64 expressions.  Tiny shapes: at most 7 clips of 32 rows of
63 ids.  Every case prints its measured worst ratios (pytest -s) -- DESIGN section 7 quotes them."""
import math

import numpy as np
import pytest
import torch

import spectrum_ref as S

pytestmark = pytest.mark.gpu

PER_CLIP = (1, 2, 5, 8, 9, 32)          # (8 | 9: the two instantiations; 32 > 16: a wave takes two rows; odd m: the padded index)
TS = (1, 2, 3, 4, 20, 63)               # (T < 4: orders without an n-gram; 63: the last lane)
TABLES = ("empty", "small", "every")    # G = 0; a table that knows some keys; one that holds every key of the case
ULP1 = 2.0 ** -23                       # one fp32 ulp of 1
_cache = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _table(kind, cand, T, dev=None):
    from cvc.cider import CiderD
    if kind == "empty":
        return CiderD(np.zeros(0, np.uint64), np.zeros(0, np.float32), 100, dev)
    if kind == "small":
        rng = np.random.default_rng(3)
        return CiderD.from_captions([rng.integers(1, 6, T) for _ in range(40)], dev)
    return CiderD.from_captions(list(cand), dev)


def _case(per_clip, T, clips):
    """the case, its table and the references of both modes, computed once"""
    key = (per_clip, T, clips)
    if key not in _cache:
        cand, live = S.case(1000 * per_clip + 10 * T + clips, clips, per_clip, T)
        kind = TABLES[(PER_CLIP.index(per_clip) + TS.index(T) + clips) % 3]
        table = _table(kind, cand, T)
        tab, unseen = S.table_of(table)
        ref = []
        for c in range(clips):
            ws = S.live_rows(cand, per_clip, live, c)
            ref.append(dict(m=len(ws), lsa=S.gram64(ws, "lsa"), k64=S.gram64(ws, "cider", tab, unseen),
                            k32=S.gram32(ws, "cider", tab, unseen)))
        _cache[key] = (cand, live, table, ref)
    return _cache[key]


def _check_spectrum(out, ms, what):
    """what holds for either mode, given the kernel's own gram: symmetry, padding, eigenvalues, info, scores -> measured ratios"""
    gram, lam = out["gram"].cpu().numpy(), out["lam"].cpu().numpy()
    score, info = out["score"].cpu().numpy(), out["info"].cpu().numpy()
    assert gram.dtype == np.float32 and lam.dtype == np.float64 and score.dtype == np.float32 and info.dtype == np.int32
    worst_lam = worst_score = 0.0
    for c, m in enumerate(ms):
        g = gram[c].astype(np.float64)
        assert np.array_equal(gram[c], gram[c].T), what
        assert (gram[c][m:] == 0).all() and (gram[c][:, m:] == 0).all(), what
        assert info[c, 0] == m and 1 <= info[c, 1] <= 16, (what, info[c])
        tr = float(np.trace(g))
        want = S.spectrum(g[:m, :m])
        assert (lam[c][m:] == 0).all() and (np.diff(lam[c][:m]) <= 0).all(), what
        err = float(np.abs(lam[c] - want).max())
        assert err <= 256 * S.U * tr, (what, c, m, err / (S.U * tr) if tr else err)
        if tr > 0:
            worst_lam = max(worst_lam, err / (S.U * tr))
        s0, s1 = S.scores(lam[c], tr, m)
        worst_score = max(worst_score, abs(float(score[c, 0]) - s0), abs(float(score[c, 1]) - s1))
        assert abs(float(score[c, 0]) - s0) <= 1e-6 and abs(float(score[c, 1]) - s1) <= 1e-6, (what, c, score[c], s0, s1)
        assert 0.0 <= score[c, 0] <= 1.0 and 0.0 <= score[c, 1] <= 1.0, (what, score[c])
        if m < 2:
            assert score[c, 0] == 0 and score[c, 1] == 0
    return worst_lam, worst_score, int(info[:, 1].max())


@pytest.mark.parametrize("clips", [1, 7])
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("per_clip", PER_CLIP)
def test_matrix_eigenvalues_and_scores_against_the_restatement(dev, per_clip, T, clips):
    from cvc import metrics
    cand, live, table, ref = _case(per_clip, T, clips)
    c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
    ms = [r["m"] for r in ref]
    lsa = metrics.set_spectrum(c, per_clip, l, want_gram=True)
    assert lsa["gram"].shape == (clips, 32, 32) and lsa["lam"].shape == (clips, 32) and lsa["score"].shape == (clips, 2)
    assert lsa["info"].shape == (clips, 2)
    g = lsa["gram"].cpu().numpy()
    for k, r in enumerate(ref):                                             # integers below 2^24: exact
        assert np.array_equal(g[k].astype(np.float64), S.padded(r["lsa"])), (k, g[k][:r["m"], :r["m"]], r["lsa"])
    wl, ws, sw = _check_spectrum(lsa, ms, "lsa")
    cid = metrics.set_spectrum(c, per_clip, l, cider=table, want_gram=True)
    g = cid["gram"].cpu().numpy()
    worst_k = 0.0
    for k, r in enumerate(ref):                                             # within 4 x the float32 restatement's own error
        own = np.abs(r["k32"].astype(np.float64) - r["k64"])
        bound = S.padded(np.maximum(4 * own, ULP1))
        err = np.abs(g[k].astype(np.float64) - S.padded(r["k64"]))
        worst_k = max(worst_k, float((err[:r["m"], :r["m"]] / bound[:r["m"], :r["m"]]).max()) if r["m"] else 0.0)
        assert (err <= bound).all(), (k, float(err.max()))
    cl, cs, csw = _check_spectrum(cid, ms, "cider")
    print("SPECTRUM per_clip=%d T=%d clips=%d table=%d: gram err / bound %.3f, lam err / (u tr) lsa %.2f cider %.2f, score err lsa %.2e "
          "cider %.2e, sweeps lsa %d cider %d" % (per_clip, T, clips, len(table), worst_k, wl, cl, ws, cs, sw, csw))
    without = metrics.set_spectrum(c, per_clip, l, cider=table)               # gram = null: the same spectrum
    assert "gram" not in without and all(torch.equal(without[k].view(torch.int32), cid[k].view(torch.int32)) for k in without)
    if live.all() and per_clip > 1:                                         # live=None is "every row counts"
        out2 = metrics.set_spectrum(c, per_clip, cider=table, want_gram=True)
        assert all(torch.equal(cid[k].view(torch.int32), out2[k].view(torch.int32)) for k in cid)


def test_no_live_mask_is_all_live_and_self_cider_is_the_thin_caller(dev):
    from cvc import metrics
    cand, _, table, _ = _case(5, 20, 7)
    c = torch.from_numpy(cand).to(dev)
    out = metrics.set_spectrum(c, 5, want_gram=True)
    for k in range(7):
        assert np.array_equal(out["gram"][k].cpu().numpy().astype(np.float64), S.padded(S.gram64(S.live_rows(cand, 5, None, k), "lsa")))
    assert (out["info"][:, 0] == 5).all()
    a, b = table.self_cider(c, 5), metrics.set_spectrum(c, 5, cider=table)
    assert a.keys() == b.keys() and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def test_a_clip_alone_equals_the_clip_in_a_batch_and_two_runs_are_bit_equal(dev):
    from cvc import metrics
    for per_clip, T in ((5, 20), (9, 63), (32, 20)):
        cand, live, table, _ = _case(per_clip, T, 7)
        c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
        for tab in (None, table):
            a, b = (metrics.set_spectrum(c, per_clip, l, cider=tab, want_gram=True) for _ in range(2))
            assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)
            for clip in (0, 3, 4, 6):
                rows = slice(clip * per_clip, (clip + 1) * per_clip)
                one = metrics.set_spectrum(c[rows].contiguous(), per_clip, l[rows].contiguous(), cider=tab, want_gram=True)
                assert all(torch.equal(one[k][0].view(torch.int32), a[k][clip].view(torch.int32)) for k in a)


def test_every_output_is_overwritten(dev):
    from cvc import hip
    for per_clip, T, clips in ((5, 20, 7), (32, 4, 7), (1, 3, 7)):
        cand, live, _, _ = _case(per_clip, T, clips)
        c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
        gram = torch.full((clips, 32, 32), float("nan"), device=dev)
        lam = torch.full((clips, 32), float("nan"), device=dev, dtype=torch.float64)
        score = torch.full((clips, 2), float("nan"), device=dev)
        info = torch.full((clips, 2), -77, dtype=torch.int32, device=dev)
        hip._check(hip.lib().cvc_caption_set_spectrum(c.data_ptr(), l.data_ptr(), clips * per_clip, T, per_clip, 1, None, None, 0, 0.0,
                                                      gram.data_ptr(), lam.data_ptr(), score.data_ptr(), info.data_ptr(), hip._stream()),
                   "cvc_caption_set_spectrum")
        assert not torch.isnan(gram).any() and not torch.isnan(lam).any() and not torch.isnan(score).any() and (info != -77).all()


def test_graph_replay_on_new_inputs_equals_the_eager_call(dev):
    from cvc import metrics
    per_clip, T, clips = 9, 20, 7
    cand, live, table, _ = _case(per_clip, T, clips)
    cand2, live2 = S.case(99, clips, per_clip, T)
    c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
    table.to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        metrics.set_spectrum(c, per_clip, l, cider=table)                   # (warm-up: the library is loaded outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = metrics.set_spectrum(c, per_clip, l, cider=table, want_gram=True)
        out_lsa = metrics.set_spectrum(c, per_clip, l)
    c.copy_(torch.from_numpy(cand2))
    l.copy_(torch.from_numpy(live2))
    g.replay()
    torch.cuda.synchronize()
    eager, eager_lsa = metrics.set_spectrum(c, per_clip, l, cider=table, want_gram=True), metrics.set_spectrum(c, per_clip, l)
    assert all(torch.equal(out[k].view(torch.int32), eager[k].view(torch.int32)) for k in out)
    assert all(torch.equal(out_lsa[k].view(torch.int32), eager_lsa[k].view(torch.int32)) for k in out_lsa)
    assert [int(x) for x in out["info"][:, 0].tolist()] == [len(S.live_rows(cand2, per_clip, live2, k)) for k in range(clips)]


def test_scorer_against_fp64_means(dev):
    from cvc import metrics
    scorer, s0, s1, m0, ok0, ok1 = None, [], [], [], [], []
    for per_clip, clips in ((5, 7), (5, 1)):                                # two batches of the same set size
        cand, live, table, ref = _case(per_clip, 20, clips)
        scorer = scorer or metrics.SpectrumScorer(table)
        c, l = torch.from_numpy(cand).to(dev), torch.from_numpy(live).to(dev)
        outs = scorer.add(c, per_clip, l)
        s0 += outs["cider"]["score"][:, 0].tolist()
        s1 += outs["lsa"]["score"][:, 1].tolist()
        m0 += [r["m"] for r in ref]
        ok0 += (outs["cider"]["lam"][:, 0] > 0).tolist()
        ok1 += (outs["lsa"]["lam"][:, 0] > 0).tolist()
    res = scorer.result()
    want = {"Self_CIDEr": S.headline(s0, m0, ok0), "LSA": S.headline(s1, m0, ok1), "Spectrum_sets": sum(1 for m in m0 if m >= 2)}
    assert res.keys() == want.keys() and res["Spectrum_sets"] == want["Spectrum_sets"] and want["Self_CIDEr"] > 0 and want["LSA"] > 0
    assert abs(res["Self_CIDEr"] - want["Self_CIDEr"]) <= 1e-12 and abs(res["LSA"] - want["LSA"]) <= 1e-12
    other = metrics.SpectrumScorer()
    other.add_sums(scorer.sums())
    assert other.result() == res
    only_lsa = metrics.SpectrumScorer()
    cand, live, _, _ = _case(5, 20, 7)
    assert set(only_lsa.add(torch.from_numpy(cand).to(dev), 5, torch.from_numpy(live).to(dev))) == {"lsa"}
    assert only_lsa.result()["Self_CIDEr"] == 0.0 and abs(only_lsa.result()["LSA"] - S.headline(s1[:7], m0[:7], ok1[:7])) <= 1e-12


def test_bad_arguments_are_refused_by_the_library(dev):
    from cvc import hip
    z = torch.zeros(8, 8, dtype=torch.int64, device=dev)
    p = z.data_ptr()

    def call(cand=p, rows=8, T=8, per=2, mode=1, keys=None, idf=None, G=0, lam=p, score=p, info=p):
        return hip.lib().cvc_caption_set_spectrum(cand, None, rows, T, per, mode, keys, idf, G, 0.0, None, lam, score, info, None)
    for rc in (call(rows=7), call(cand=None), call(lam=None), call(score=None), call(info=None), call(rows=0), call(per=0),
               call(rows=33, per=33), call(T=0), call(T=64), call(mode=2), call(mode=0, G=3), call(mode=0, G=3, keys=p)):
        assert rc == -1
    with pytest.raises(RuntimeError, match="cvc_caption_set_spectrum failed: bad argument"):
        hip._check(call(rows=7), "cvc_caption_set_spectrum")
