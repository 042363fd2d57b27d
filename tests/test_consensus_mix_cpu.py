"""Consensus selection under a weighted utility mix without a GPU: the restatement (tests/consensus_mix_ref.py) against the references
it is built on, the weights' edges, the inputs' generator, the command line, the block's declaration and the refusals of every layer."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import cider_ref as R
import consensus_ref as C
import consensus_mix_ref as M
import overlap_ref as OV


def _live_pairs(live, n):
    return [(i, j) for i in range(live.shape[0]) for j in range(n) if i // n * n + j != i and live[i] and live[i // n * n + j]]


# ---------------------------------------------------------------- the restatement against what exists
@pytest.mark.parametrize("clips,n,T,V", M.CASES)
def test_uniform_cider_only_is_consensus_ref(clips, n, T, V):
    """CIDEr-D over a reference set is the mean of its single-reference values: with uniform weights and cider alone the weighted
    form restates consensus_ref's utility"""
    c = M.case(clips, n, T, V)
    u = M.expected(c, n, {"cider": 1.0}, "uniform")[0]
    want = C.utilities(c["cand"], n, c["live"], c["df"], c["n_doc"])
    print(f"[consensus_mix] {(clips, n, T, V)}: max |weighted form - consensus_ref| {np.abs(u - want).max():.3e}")
    assert np.abs(u - want).max() <= 1e-12


@pytest.mark.parametrize("clips,n,T,V", M.CASES[:4])
def test_bleu_and_rouge_pairs_are_overlap_ref_on_single_references(clips, n, T, V):
    c = M.case(clips, n, T, V)
    cand, live = c["cand"], c["live"]
    idx = _live_pairs(live, n)
    rows = np.stack([cand[i] for i, _ in idx])
    refs = np.stack([cand[i // n * n + j] for i, j in idx])[:, None, :]
    for dt, p in ((np.float64, c["p64"]), (np.float32, c["p32"])):
        want = OV.score_batch(rows, refs, np.ones(len(idx), dtype=np.int32), dt)
        got = np.stack([p[i, j] for i, j in idx])
        assert np.array_equal(got[:, 1:5], want["bleu"]) and np.array_equal(got[:, 5], want["rouge"])
    dead = [(i, j) for i in range(live.shape[0]) for j in range(n) if (i, j) not in set(idx)]
    assert not any(c["p64"][i, j].any() for i, j in dead)                   # the diagonal and dead rows


def test_a_utility_mix_is_the_weighted_sum_of_its_parts():
    clips, n, T, V = 4, 5, 20, 23
    c = M.case(clips, n, T, V)
    parts = [M.expected(c, n, {k: 1.0}, "uniform")[0] for k in ("cider", "bleu4", "rougel")]
    mix = M.expected(c, n, M.MIXED, "uniform")[0]
    assert np.abs(mix - (parts[0] + 0.5 * parts[1] + 0.5 * parts[2])).max() <= 1e-12
    assert np.count_nonzero(parts[1]) and np.count_nonzero(parts[2])


# ---------------------------------------------------------------- weights
def test_weight_edges():
    live = np.ones(4, dtype=bool)
    ninf = -np.inf
    assert M.weights(None, live, 4).tolist() == [1, 1, 1, 1]
    assert M.weights(np.array([ninf] * 4, np.float32), live, 4).tolist() == [0, 0, 0, 0]           # an all -inf clip: no NaN
    w = M.weights(np.array([0.0, np.nan, ninf, -1.0], np.float32), live, 4)
    assert w[0] == 1.0 and w[1] == 0.0 and w[2] == 0.0 and w[3] == np.exp(-1.0)                      # NaN counts as -inf
    assert M.weights(np.array([np.nan, -3.0, -3.0, -5.0], np.float32), live, 4)[:3].tolist() == [0, 1, 1]
    # the maximum is over the LIVE rows: a dead row's large log-weight scales nothing
    w = M.weights(np.array([50.0, -2.0, -3.0, ninf], np.float32), np.array([0, 1, 1, 1], bool), 4)
    assert w.tolist() == [0.0, 1.0, float(np.exp(-1.0)), 0.0]
    pairs = np.zeros((4, 4, 6))
    pairs[:, :, 0] = [[0, 1, 2, 3], [4, 0, 5, 6], [7, 8, 0, 9], [1, 2, 3, 0]]
    for dt in (np.float64, np.float32):
        # all -inf: every denominator is 0 -> utilities 0, and the pick is the first live row
        u = M.utilities(pairs, np.zeros(4), live, 4, {"cider": 1.0}, dt)
        assert not u.any() and M.picks(u, live, 4).tolist() == [0]
        # one live row: no other live row -> 0; a clip's only weighted row gives every other row u(i, that row) and itself 0
        one = np.array([0, 0, 1, 0], bool)
        assert not M.utilities(pairs, M.weights(None, one, 4), one, 4, {"cider": 1.0}, dt).any()
        u = M.utilities(pairs, np.array([0.0, 1.0, 0.0, 0.0]), live, 4, {"cider": 1.0}, dt)
        assert u.tolist() == [1.0, 0.0, 8.0, 2.0]
        # a row of weight 0 is still a candidate
        u = M.utilities(pairs, np.array([1.0, 0.0, 1.0, 1.0]), live, 4, {"cider": 1.0}, dt)
        assert u[1] == 5.0 and u[0] == 2.5


def test_weighted_utilities_follow_the_definition():
    clips, n, T, V = 4, 5, 20, 23
    c = M.case(clips, n, T, V)
    live, p = c["live"], c["p64"]
    for kind in ("finite", "inf"):
        lw = c["logw"][kind]
        u = M.expected(c, n, M.MIXED, kind)[0]
        clean = np.where(np.isnan(lw), -np.inf, lw.astype(np.float64))
        for i in np.flatnonzero(live):
            c0 = i // n * n
            js = [j for j in range(n) if c0 + j != i and live[c0 + j]]
            top = max(clean[r] for r in range(c0, c0 + n) if live[r])
            w = np.array([np.exp(clean[c0 + j] - top) if clean[c0 + j] > -np.inf else 0.0 for j in js])
            util = np.array([p[i, j, 0] + 0.5 * p[i, j, 4] + 0.5 * p[i, j, 5] for j in js])
            want = float((w * util).sum() / w.sum()) if js and w.sum() > 0 else 0.0
            assert abs(u[i] - want) <= 1e-12


# ---------------------------------------------------------------- the inputs
@pytest.mark.parametrize("clips,n,T,V", M.CASES)
def test_generator_gives_pairs_worth_comparing(clips, n, T, V):
    c = M.case(clips, n, T, V)
    cand, live = c["cand"], c["live"]
    assert cand.shape == (clips * n, T) and cand.min() >= 0 and cand.max() < V
    if clips >= 3:
        per = live.reshape(clips, n).sum(1)
        assert per[-1] == 0 and per[-2] == 1
    if n >= 5:
        assert cand[1, 0] == 0 and cand[1, 1:].any() and live[1]            # an empty caption, words behind its end mark
        assert (cand[2] != 0).all() and live[2]                             # no end mark
    if T >= 4 and n >= 5:
        idx = _live_pairs(live, n)
        nz = sum(c["p64"][i, j, 4] > M.BLEU4_NONZERO for i, j in idx)
        has = np.array([live[i] and live[i // n * n:(i // n + 1) * n].sum() > 1 for i in range(clips * n)])
        u = M.expected(c, n, M.MIXED, "uniform")[0]
        print(f"[consensus_mix] {(clips, n, T, V)}: BLEU-4 > {M.BLEU4_NONZERO} on {nz}/{len(idx)} live ordered pairs, mixed utility "
              f"non-zero on {np.count_nonzero(u[has])}/{has.sum()} rows with another live row")
        assert nz >= 0.5 * len(idx) and np.count_nonzero(u[has]) >= 0.9 * has.sum()


# ---------------------------------------------------------------- command line
def test_command_line():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    P = cvc_main.build_parser
    o = P().parse_args([])
    assert not any(hasattr(o, k) for k in ("consensus_utility", "consensus_weights", "consensus_alpha"))         # absent: no key
    cvc_main.check_consensus_mix_flags(o)
    assert not hasattr(o, "consensus_utility")
    assert not hasattr(cvc_opts.build_parser().parse_args([]), "consensus_utility")                              # flags of cvc.main
    o = P().parse_args(["--consensus", "beam", "--consensus_utility", "rougel:0.5,cider:1,bleu4:0.5", "--consensus_weights", "model",
                        "--consensus_alpha", "0.5"])
    cvc_main.check_consensus_mix_flags(o)
    assert o.consensus_utility == {"cider": 1.0, "bleu4": 0.5, "rougel": 0.5} and list(o.consensus_utility) == ["cider", "bleu4", "rougel"]
    assert (o.consensus_weights, o.consensus_alpha) == ("model", 0.5)
    o = P().parse_args(["--consensus", "samples", "--consensus_utility", "bleu4"])
    cvc_main.check_consensus_mix_flags(o)
    assert o.consensus_utility == {"bleu4": 1.0}
    with pytest.raises(SystemExit):
        P().parse_args(["--consensus_weights", "sometimes"])

    def refused(argv, match, sample=None):
        with pytest.raises(SystemExit, match=match):
            cvc_main.check_consensus_mix_flags(P().parse_args(argv), sample)
    refused(["--consensus_utility", "bleu4:1"], "--consensus_utility .*needs --consensus samples")               # no selection at all
    refused(["--consensus_weights", "uniform"], "--consensus_weights")
    refused(["--consensus_alpha", "2"], "--consensus_alpha")
    refused(["--consensus", "samples", "--consensus_weights", "model"], "--consensus_weights model")            # draws
    refused(["--consensus", "beam", "--stochastic_beam", "--beam_size", "4", "--consensus_weights", "model"], "--consensus_weights model")
    refused(["--consensus", "beam", "--consensus_utility", "meteor:1"], "--consensus_utility: unknown metric")
    refused(["--consensus", "beam", "--consensus_utility", "cider:-1"], "--consensus_utility: the weight")
    refused(["--consensus", "beam", "--consensus_utility", "cider:0"], "--consensus_utility: every weight is 0")
    refused(["--consensus", "beam", "--consensus_utility", ""], "--consensus_utility: no metric")
    refused(["--consensus", "beam", "--consensus_alpha", "-1"], "--consensus_alpha")
    refused(["--consensus", "beam", "--consensus_alpha", "nan"], "--consensus_alpha")
    refused(["--consensus", "beam", "--consensus_alpha", "inf"], "--consensus_alpha")
    # python -m cvc.sample: its own --consensus is the selection (position 5 of the tuple), its candidates are draws
    s_on, s_off = (4, 1.0, 0, 0, 1.0, True, False, False), (4, 1.0, 0, 0, 1.0, False, False, False)
    o = P().parse_args(["--consensus_utility", "bleu4:1,rougel:1"])
    cvc_main.check_consensus_mix_flags(o, s_on)
    assert o.consensus_utility == {"bleu4": 1.0, "rougel": 1.0}
    refused(["--consensus_utility", "bleu4:1"], "--consensus_utility", s_off)
    refused(["--consensus_weights", "model"], "--consensus_weights model", s_on)
    # the message of --scst_reward still names --scst_reward
    from cvc.metrics import parse_reward_weights
    with pytest.raises(SystemExit, match="--scst_reward: unknown metric"):
        parse_reward_weights("meteor:1")


# ---------------------------------------------------------------- the block and the wrappers
def test_block_declared_listed_bound_and_not_exported():
    import build_hip
    from cvc import hip
    from test_cabi import declared_functions, BLOCKS_H
    n = "cvc_consensus_mix"
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    assert n in declared_functions(BLOCKS_H) and n in hip.BLOCKS and n in hip.SIGNATURES
    assert lib.cvc_block(n.encode())
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip.build(verbose=False)], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert n not in exported and len(exported) == 70, len(exported)


def test_bad_arguments_return_badarg_before_any_launch():
    from cvc import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # non-null; never dereferenced: every call below is refused on the host
    nan, inf = float("nan"), float("inf")

    def call(cand=p, live=None, logw=None, rows=6, T=5, per=3, keys=p, idf=p, G=1, sigma=6.0, coef=(1, 0, 0, 0, 0.5, 0.5), utility=p,
             pick=p, best=p, pairs=None):
        arr = None if coef is None else (ctypes.c_float * 6)(*coef)            # (kept alive over the call)
        return lib.cvc_consensus_mix(cand, live, logw, rows, T, per, keys, idf, G, 1.0, sigma, None if arr is None else ctypes.addressof(arr),
                                     utility, pick, best, pairs, None)
    assert call(cand=None) == -1 and call(utility=None) == -1 and call(pick=None) == -1 and call(best=None) == -1 and call(coef=None) == -1
    assert call(rows=7) == -1 and call(rows=0) == -1 and call(rows=-3) == -1
    assert call(per=0) == -1 and call(rows=33, per=33) == -1
    assert call(T=0) == -1 and call(T=64) == -1
    assert call(coef=(0, 0, 0, 0, 0, 0)) == -1                               # nothing weighted
    for bad in (-1.0, nan, inf, -inf):
        for k in range(6):
            coef = [1.0] * 6
            coef[k] = bad
            assert call(coef=coef) == -1, (bad, k)
    assert call(sigma=0.0) == -1 and call(sigma=-1.0) == -1 and call(sigma=nan) == -1
    assert call(keys=None) == -1 and call(idf=None) == -1 and call(G=-1) == -1                   # cider weighted: the table counts


def test_wrappers_refuse_by_name():
    from cvc import hip, metrics
    from cvc.cider import CiderD
    t = CiderD.from_captions([np.array([1, 2, 0])])
    keys, idf = torch.from_numpy(t.keys_host.view(np.int64).copy()), torch.from_numpy(t.idf_host.copy())
    cand = torch.zeros(6, 3, dtype=torch.int64)
    one = [1, 0, 0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.consensus_mix(cand, 4, one, keys, idf)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.consensus_mix(cand, 3, one, keys, idf, live=torch.ones(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.consensus_mix(cand, 3, one, keys, idf, logw=torch.zeros(5))
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.consensus_mix(cand, 3, one, keys, idf[:1])
    with pytest.raises(RuntimeError, match="coef holds 5"):
        hip.consensus_mix(cand, 3, one[:5], keys, idf)
    with pytest.raises(RuntimeError, match="CIDEr coefficient needs the idf table"):
        hip.consensus_mix(cand, 3, one)
    with pytest.raises(RuntimeError, match="GPU"):                          # no CPU fallback
        hip.consensus_mix(cand, 3, [0, 0, 0, 0, 1, 0])
    with pytest.raises(RuntimeError, match="utility weights cider, which needs table"):
        metrics.consensus(cand, 3, {"cider": 1.0, "bleu4": 0.5})
    with pytest.raises(RuntimeError, match="unknown metrics"):
        metrics.consensus(cand, 3, {"meteor": 1.0}, t)
    with pytest.raises(RuntimeError, match="finite numbers >= 0"):
        metrics.consensus(cand, 3, {"bleu4": -0.5}, t)
    with pytest.raises(RuntimeError, match="finite numbers >= 0"):
        metrics.consensus(cand, 3, {"bleu4": float("nan")}, t)
    with pytest.raises(RuntimeError, match="weights nothing"):
        metrics.consensus(cand, 3, {"bleu4": 0.0}, t)
    with pytest.raises(RuntimeError, match="T = 63"):
        metrics.consensus(torch.zeros(4, 64, dtype=torch.int64), 2, {"bleu4": 1.0})
    with pytest.raises(RuntimeError, match="per_clip = 32"):
        metrics.consensus(torch.zeros(66, 5, dtype=torch.int64), 33, {"bleu4": 1.0})
    assert metrics.utility_coefficients({"rougel": 2, "cider": 1}) == [1.0, 0, 0, 0, 0, 2.0]


def test_sample_refuses_the_switches_by_name_before_anything_runs():
    from cvc import synth
    from cvc.cider import CiderD
    from helpers import build_model
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 1), torch.device("cpu"))
    assert (model.consensus_utility, model.consensus_weights, model.consensus_alpha, model.consensus_pairs) == (None, "uniform", 1.0, False)
    model.consensus_table = CiderD.from_captions([np.array([1, 2, 0])])
    none = [None] * 11
    with pytest.raises(RuntimeError, match="consensus_weights must be"):
        model._sample(*none, consensus="beam", consensus_weights="sometimes")
    with pytest.raises(RuntimeError, match="consensus_alpha must be"):
        model._sample(*none, consensus="beam", consensus_alpha=-1.0)
    with pytest.raises(RuntimeError, match="consensus_alpha must be"):
        model._sample(*none, consensus="beam", consensus_alpha=float("nan"))
    with pytest.raises(RuntimeError, match="consensus_utility: utility names unknown"):
        model._sample(*none, consensus="beam", consensus_utility={"meteor": 1.0})
    with pytest.raises(RuntimeError, match="consensus_utility: utility weights nothing"):
        model._sample(*none, consensus="beam", consensus_utility={"cider": 0.0})
    m2 = build_model(d, synth.hot_path_state_dict(d, 1), torch.device("cpu"), consensus="beam", consensus_utility={"bleu4": 1.0},
                     consensus_weights="model", consensus_alpha=0.0)
    assert (m2.consensus_utility, m2.consensus_weights, m2.consensus_alpha) == ({"bleu4": 1.0}, "model", 0.0)
