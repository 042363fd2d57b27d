"""cvc_consensus_mix (csrc/consensus_mix.hip): its raw pair metrics bit for bit against cvc_cider_d and cvc_caption_overlap on gathered
single references, its utilities against the fp64 restatement (tests/consensus_mix_ref.py), the pick, reproducibility, and the
decode engine's use of it.

Tolerance of the utilities, the project's rule: the reference is the restatement in fp64, the yardstick the SAME restatement in fp32
on the CPU; the kernel's largest error may be 4 x the yardstick's largest error on the same case, with a floor of 2^-20 (one fp32 ulp
of a value in [0.5, 1), the scale of BLEU and ROUGE-L) and 10 x that where the utility has a CIDEr-D term (scale [0, 10]).  pick is
checked exactly against the kernel's own utilities, and against fp64 through the utility of the picked row (within 2 x bound of the
clip's fp64 maximum: near-duplicates make near-ties the norm).  Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

from cvc import synth
import consensus_ref as C
import consensus_mix_ref as M

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
ALL = {k: 1.0 for k in M.NAMES}
_TABLES = {}


def _dev():
    return torch.device("cuda:0")


def _t(a, dt):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev(), dt)


def _table(key, train):
    from cvc.cider import CiderD
    if key not in _TABLES:
        _TABLES[key] = CiderD.from_captions(train, _dev())
    return _TABLES[key]


def _run(table, cand, n, live, utility, logw=None, want_pairs=False):
    from cvc import metrics
    return metrics.consensus(_t(cand, torch.int64), n, utility, table, _t(logw, torch.float32), _t(live, torch.int32), want_pairs)


def _bound(utility, yard):
    return max(4.0 * yard, FLOOR * (10.0 if utility.get("cider", 0.0) > 0 else 1.0))


def _check(label, cand, n, live, out, u64, u32, utility):
    u, pick, best = (out[k].cpu().numpy() for k in ("utility", "pick", "best"))
    rows = cand.shape[0]
    err, yard = float(np.abs(u.astype(np.float64) - u64).max()), float(np.abs(u32 - u64).max())
    bound = _bound(utility, yard)
    m64 = np.where(live, u64, -np.inf).reshape(-1, n)
    has = live.reshape(-1, n).any(1)
    picked64 = u64.reshape(-1, n)[np.arange(rows // n), pick]
    gap = float((m64.max(1) - picked64)[has].max()) if has.any() else 0.0
    print(f"[consensus_mix] {label}: kernel max |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e}); live rows "
          f"{int(live.sum())}/{rows}, non-zero fp64 utilities {np.count_nonzero(u64[live])}; largest fp64 shortfall of a picked row "
          f"{gap:.3e} (allowed {2 * bound:.3e})")
    assert err <= bound, (label, err, yard)
    assert not u[~live].any()                                              # a dead row's utility is 0
    assert np.array_equal(pick, C.picks(u, live, n)), label               # exact: the first live arg-max of the kernel's own utilities
    assert live.reshape(-1, n)[np.arange(rows // n), pick][has].all()     # a dead row is never picked
    assert not pick[~has].any()                                           # a clip without a live row: 0
    assert gap <= 2 * bound, (label, gap)
    assert np.array_equal(best, cand.reshape(-1, n, cand.shape[1])[np.arange(rows // n), pick]), label
    return bound


def _gathered(table, cand, n, live):
    """the route without the block: every live ordered pair (i, j) as one candidate row with one reference -> (index arrays i, j,
    cvc_cider_d's reward [P], cvc_caption_overlap's bleu [P, 4] and rouge [P])"""
    from cvc import metrics
    idx = [(i, j) for i in range(cand.shape[0]) for j in range(n) if i // n * n + j != i and live[i] and live[i // n * n + j]]
    ii, jj = np.array([i for i, _ in idx]), np.array([j for _, j in idx])
    rows = _t(cand[ii], torch.int64)
    refs = _t(cand[ii // n * n + jj][:, None, :], torch.int64)
    nref = torch.ones(len(idx), dtype=torch.int32, device=_dev())
    ov = metrics.overlap(rows, refs, nref)
    return ii, jj, table.score(rows, refs, nref), ov["bleu"], ov["rouge"]


@pytest.mark.parametrize("clips,n,T,V", M.CASES)
def test_pairs_have_the_bits_of_the_kernels_they_restate(clips, n, T, V):
    c = M.case(clips, n, T, V)
    cand, live = c["cand"], c["live"]
    table = _table((clips, n, T, V), c["train"])
    ii, jj, cider, bleu, rouge = _gathered(table, cand, n, live)
    ti, tj = _t(ii, torch.int64), _t(jj, torch.int64)
    for utility, lw in ((ALL, None), (M.MIXED, c["logw"]["inf"])):          # (the weights do not enter the pair metrics)
        pairs = _run(table, cand, n, live, utility, lw, want_pairs=True)["pairs"]
        assert pairs.shape == (clips, n, n, 6)
        flat = pairs.view(clips * n, n, 6)
        got = flat[ti, tj]
        on = [k for k, name in enumerate(M.NAMES) if utility.get(name, 0.0) > 0]
        same = {M.NAMES[k]: int((got[:, k] == (cider if k == 0 else rouge if k == 5 else bleu[:, k - 1])).sum()) for k in on}
        print(f"[consensus_mix] {(clips, n, T, V)} {sorted(utility)}: of {len(ii)} live ordered pairs bit-equal {same}; non-zero "
              f"{ {M.NAMES[k]: int((got[:, k] != 0).sum()) for k in on} }")
        if 0 in on:
            assert torch.equal(got[:, 0], cider)
        if all(k in on for k in (1, 2, 3, 4)):
            assert torch.equal(got[:, 1:5], bleu)
        else:
            assert torch.equal(got[:, 4], bleu[:, 3]) and not got[:, 1:4].any()         # a coefficient of 0: not computed, zeros
        assert torch.equal(got[:, 5], rouge)
        rest = flat.clone()
        rest[ti, tj] = 0
        assert not rest.any()                                               # the diagonal, dead rows
    if T >= 4 and n >= 5:                                                   # not vacuous
        assert int((bleu[:, 3] > M.BLEU4_NONZERO).sum()) >= 0.5 * len(ii) and int((cider > 0).sum()) >= 0.5 * len(ii)


@pytest.mark.parametrize("kind", M.LOGW_KINDS)
@pytest.mark.parametrize("clips,n,T,V", M.CASES)
def test_utilities_and_pick_vs_fp64(clips, n, T, V, kind):
    c = M.case(clips, n, T, V)
    table = _table((clips, n, T, V), c["train"])
    for utility in M.COEFS:
        u64, u32 = M.expected(c, n, utility, kind)
        out = _run(table, c["cand"], n, c["live"], utility, c["logw"][kind])
        _check(f"{(clips, n, T, V)} {kind} {'+'.join(utility)}", c["cand"], n, c["live"], out, u64, u32, utility)


@pytest.mark.parametrize("clips,n,T,V", M.CASES)
def test_uniform_cider_only_against_consensus_cider(clips, n, T, V):
    """the same quantity by another order of additions (the old kernel adds the references per n-gram order and averages the four
    sums; this one adds whole pair scores): held to the bound, the differing bits are counted and printed"""
    c = M.case(clips, n, T, V)
    table = _table((clips, n, T, V), c["train"])
    u64, u32 = M.expected(c, n, {"cider": 1.0}, "uniform")
    bound = _bound({"cider": 1.0}, float(np.abs(u32 - u64).max()))
    new = _run(table, c["cand"], n, c["live"], {"cider": 1.0})
    old_u, old_pick, old_best = table.consensus(_t(c["cand"], torch.int64), n, live=_t(c["live"], torch.int32))
    diff = float((new["utility"] - old_u).abs().max())
    print(f"[consensus_mix] {(clips, n, T, V)} uniform, CIDEr-D alone: {int((new['utility'] == old_u).sum())}/{old_u.numel()} utilities "
          f"bit-equal to cvc_consensus_cider, max |diff| {diff:.3e} (bound {bound:.3e}); picks equal: {bool(torch.equal(new['pick'], old_pick))}")
    assert diff <= bound
    if n == 2:                                   # one reference: one addition order
        assert torch.equal(new["utility"], old_u) and torch.equal(new["pick"], old_pick) and torch.equal(new["best"], old_best)


def test_deterministic_and_independent_of_the_other_clips():
    clips, n, T, V = 4, 5, 20, 23
    c = M.case(clips, n, T, V)
    table = _table((clips, n, T, V), c["train"])
    lw = c["logw"]["inf"]
    keys = ("utility", "pick", "best", "pairs")
    a = _run(table, c["cand"], n, c["live"], M.MIXED, lw, want_pairs=True)
    b = _run(table, c["cand"], n, c["live"], M.MIXED, lw, want_pairs=True)
    for k in keys:
        assert torch.equal(a[k], b[k])
    for clip in range(clips):
        sl = slice(clip * n, (clip + 1) * n)
        one = _run(table, c["cand"][sl], n, c["live"][sl], M.MIXED, lw[sl], want_pairs=True)     # alone in its launch
        for k, per in zip(keys, (n, 1, 1, 1)):
            assert torch.equal(a[k][clip * per:(clip + 1) * per], one[k]), (clip, k)
    big, bn = M.case(3, 32, 20, 23), 32          # the 32-row instantiation: clip 0 alone and with two clips appended
    tb = _table((3, 32, 20, 23), big["train"])
    full = _run(tb, big["cand"], bn, big["live"], M.MIXED, big["logw"]["finite"], want_pairs=True)
    one = _run(tb, big["cand"][:bn], bn, big["live"][:bn], M.MIXED, big["logw"]["finite"][:bn], want_pairs=True)
    for k, per in zip(keys, (bn, 1, 1, 1)):
        assert torch.equal(full[k][:per], one[k]), k


def test_replays_from_a_graph_bit_for_bit():
    from cvc import hip
    clips, n, T, V = 4, 5, 20, 23
    c = M.case(clips, n, T, V)
    table = _table((clips, n, T, V), c["train"])
    coef = [M.MIXED.get(k, 0.0) for k in M.NAMES]
    cand, live, lw = _t(c["cand"], torch.int64), _t(c["live"], torch.int32), _t(c["logw"]["finite"], torch.float32)
    o_cand, o_live, _ = M.make_inputs(clips, n, T, V, seed=99)
    other, olive, olw = _t(o_cand, torch.int64), _t(o_live, torch.int32), _t(c["logw"]["inf"], torch.float32)

    def run(x, l, w):
        return hip.consensus_mix(x, n, coef, table.keys, table.idf, table.idf_unseen, table.sigma, live=l, logw=w, want_pairs=True)
    s_cand, s_live, s_lw = cand.clone(), live.clone(), lw.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(s_cand, s_live, s_lw)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = run(s_cand, s_live, s_lw)
    for x, l, w in ((other, olive, olw), (cand, live, lw)):
        s_cand.copy_(x)
        s_live.copy_(l)
        s_lw.copy_(w)
        g.replay()
        for got, want in zip(out, run(x, l, w)):
            assert torch.equal(got, want)
    assert not torch.equal(run(other, olive, olw)[0], run(cand, live, lw)[0])


def test_bad_arguments_surface_as_runtime_errors():
    from cvc import hip
    c = M.case(3, 2, 4, 7)
    table = _table((3, 2, 4, 7), c["train"])

    def call(rows, T, per, coef=(1, 0, 0, 0, 0.5, 0.5), sigma=6.0):
        return hip.consensus_mix(torch.zeros(rows, T, dtype=torch.int64, device=_dev()), per, coef, table.keys, table.idf,
                                 table.idf_unseen, sigma)
    for bad in (dict(rows=33, T=8, per=33), dict(rows=4, T=64, per=2), dict(rows=4, T=8, per=2, coef=(0,) * 6),
                dict(rows=4, T=8, per=2, coef=(1, 0, 0, -1, 0, 0)), dict(rows=4, T=8, per=2, sigma=0.0)):
        with pytest.raises(RuntimeError, match="cvc_consensus_mix failed: bad argument"):
            call(**bad)
    u, p, b, _ = call(4, 8, 2)                                              # the same call within the limits runs
    assert u.shape == (4,) and p.tolist() == [0, 0] and not b.any()
    u, p, b, _ = hip.consensus_mix(torch.zeros(4, 8, dtype=torch.int64, device=_dev()), 2, (0, 0, 0, 0, 1, 0))     # no table needed
    assert not u.any()


# ---------------------------------------------------------------- the decode engine
N = 4
UNK = synth.UNK_IDX


def _beam_engine(**kw):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    import test_gpu_sampling as TS
    d, sd, f_np, P, f = TS._inputs("tiny", seed=4321)
    return d, DecodeEngine(DecodeWeights(to_dev(sd, _dev())), to_dev(f_np, _dev()), d.T, UNK, **kw)


def _decode_table(d):
    from cvc.cider import CiderD
    rng = np.random.default_rng(17)
    return CiderD.from_captions([C.clip_candidates(rng, 1, d.T, d.V, garbage=False)[0] for _ in range(200)], _dev())


def test_beam_engine_with_model_weights():
    from cvc import metrics
    d, eng = _beam_engine(beam=N, beam_history=True)
    table = _decode_table(d)
    eng.run()
    hyp, score = eng.hypotheses()
    cand, live = hyp.reshape(d.B * N, d.T).contiguous(), torch.isfinite(score).reshape(-1)
    ar = torch.arange(d.B, device=_dev())
    # the defaults are the launch consensus() has always made
    old = eng.consensus(table)
    for same in (eng.consensus(table, utility=None, weights="uniform"), eng.consensus(table, {"cider": 1.0}, "uniform", 3.0)):
        for x, y in zip(old, same):
            assert (x is None and y is None) or torch.equal(x, y)
        assert eng.consensus_logw is None and eng.consensus_pairs is None
    u0, p0, _ = table.consensus(cand, N, live=live)
    assert torch.equal(old[4], u0) and torch.equal(old[3], p0)
    # model weights: the block on hypotheses() and alpha * score
    alpha = 0.7
    seq, att, lp, pick, util = eng.consensus(table, M.MIXED, "model", alpha)
    want = metrics.consensus(cand, N, M.MIXED, table, (score.reshape(-1) * alpha).contiguous(), live, want_pairs=True)
    assert lp is None and torch.equal(util, want["utility"]) and torch.equal(pick, want["pick"]) and torch.equal(seq, want["best"])
    assert torch.equal(seq, hyp[ar, pick.long()]) and torch.equal(eng.consensus_logw, score.reshape(-1) * alpha)
    assert float(util.max()) > 0 and not torch.equal(util, old[4])
    # a large alpha: all weight on the clip's most probable hypothesis, every other row's utility is its pair utility against that one
    s = score.clone().masked_fill(~torch.isfinite(score), float("-inf"))
    top2 = s.topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    assert gap > 0, "two hypotheses of one clip share the top score: the fixture cannot show the limit"
    big = 64.0 / gap
    util_b = eng.consensus(table, M.MIXED, "model", big)[4].view(d.B, N)
    jmax = s.argmax(1)
    pr = want["pairs"]                                                       # [B, N, N, 6]
    upair = (pr[..., 0] * 1.0 + pr[..., 4] * 0.5) + pr[..., 5] * 0.5         # the kernel's order of additions
    against_top = upair[ar, :, jmax]                                         # [B, N]: u(i, jmax)
    others = torch.ones(d.B, N, dtype=torch.bool, device=_dev())
    others[ar, jmax] = False
    others &= torch.isfinite(score)
    err = float((util_b - against_top)[others].abs().max())
    print(f"[consensus_mix] engine, alpha = {big:.1f} (top-2 score gap {gap:.4f}): max |utility - u(i, argmax score)| {err:.3e} "
          f"(bound {10 * FLOOR:.3e})")
    assert err <= 10 * FLOOR
    # want_pairs keeps the pair metrics, also for the default utility
    eng.consensus(table, want_pairs=True)
    assert eng.consensus_pairs.shape == (d.B, N, N, 6) and torch.equal(eng.consensus_pairs[..., 0], want["pairs"][..., 0])


def test_model_weights_are_refused_for_draws_before_any_launch():
    d, smp = _beam_engine(temperature=1.0, sample_n=N, seed=1)
    table = _decode_table(d)
    with pytest.raises(RuntimeError, match="weights='model' on a sampling engine"):
        smp.consensus(table, weights="model")                               # (not even run(): nothing was launched)
    d, sto = _beam_engine(beam=N, beam_history=True, stochastic=True, stochastic_tau=1.0, seed=1)
    with pytest.raises(RuntimeError, match="weights='model' on a stochastic beam"):
        sto.consensus(table, weights="model")
    d, eng = _beam_engine(beam=N, beam_history=True)
    for bad, why in ((dict(weights="sometimes"), "weights must be"), (dict(alpha=-1.0), "alpha must be"),
                     (dict(alpha=float("nan")), "alpha must be"), (dict(utility={"meteor": 1.0}), "unknown metrics"),
                     (dict(utility={"cider": 0.0}, weights="model"), "weights nothing")):
        with pytest.raises(RuntimeError, match=why):
            eng.consensus(table, **bad)
    smp.run()                                    # a sampling engine takes a utility mix with uniform weights
    seq, att, lp, pick, util = smp.consensus(table, {"bleu4": 1.0, "rougel": 1.0})
    assert seq.shape == (d.B, d.T) and lp.shape == (d.B, d.T) and util.shape == (d.B * N,) and smp.consensus_logw is None


def test_model_sample_passes_the_switches_on():
    import test_gpu_sampling as TS
    from helpers import build_model, to_dev
    from cvc import metrics
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), _dev())
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), _dev()), to_dev(synth.label_glue_batch(d, 99), _dev())
    table = model.consensus_table = _decode_table(d)
    plain = TS._model_sample(model, f, b, beam_size=N, consensus=True)
    assert model.last_consensus["weights"] is None and "pairs" not in model.last_consensus
    model.consensus_pairs = True
    seq, att, none = TS._model_sample(model, f, b, beam_size=N, consensus=True, consensus_utility=M.MIXED, consensus_weights="model",
                                      consensus_alpha=0.5)
    last, eng = model.last_consensus, model._engine_cache[1]
    score = eng.hypotheses()[1]
    assert none is None and torch.equal(last["weights"], score.reshape(-1) * 0.5) and last["pairs"].shape == (d.B, N, N, 6)
    want = metrics.consensus(last["candidates"].reshape(d.B * N, d.T).contiguous(), N, M.MIXED, table, last["weights"],
                             last["live"].reshape(-1))
    assert torch.equal(last["utility"], want["utility"]) and torch.equal(last["pick"], want["pick"]) and torch.equal(seq, want["best"])
    # the attributes are the arguments' defaults
    model.consensus, model.consensus_utility, model.consensus_weights, model.consensus_alpha = "beam", M.MIXED, "model", 0.5
    again = TS._model_sample(model, f, b, beam_size=N)
    assert torch.equal(again[0], seq) and torch.equal(model.last_consensus["utility"], last["utility"])
    with pytest.raises(RuntimeError, match="consensus_weights = 'model'"):
        TS._model_sample(model, f, b, sample_max=0, sample_n=N, temperature=1.0, seed=1, consensus=True)
    # back at the defaults the plain selection returns, bit for bit
    model.consensus_utility, model.consensus_weights, model.consensus_pairs = None, "uniform", False
    back = TS._model_sample(model, f, b, beam_size=N)
    assert torch.equal(back[0], plain[0]) and torch.equal(back[1].view(torch.int32), plain[1].view(torch.int32))
