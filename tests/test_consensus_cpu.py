"""Consensus caption selection without a GPU: the fp64 restatement (tests/consensus_ref.py) against cider_ref, the pick rule, the
command line, the block's declaration and host-side refusals, and the refusals of CiderD.consensus and model._sample."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import cider_ref as R
import consensus_ref as C


def _table():
    rng = np.random.default_rng(3)
    train = [C.clip_candidates(rng, 1, 8, 23, garbage=False)[0] for _ in range(200)]
    return train, R.doc_freq(train)


def test_two_candidates_are_each_other_s_single_reference():
    train, (df, n_doc) = _table()
    a, b = [2, 3, 3, 3, 0, 9, 9, 9], [2, 3, 6, 5, 7, 0, 0, 0]              # (a repeats a word: the clipping bites one way only)
    for dt in (np.float64, np.float32):
        u = C.utilities(np.array([a, b]), 2, None, df, n_doc, dt)
        assert u[0] == float(R.score(a, [b], df, n_doc, dt=dt)[0]) and u[1] == float(R.score(b, [a], df, n_doc, dt=dt)[0])
    assert u[0] > 0 and u[0] != u[1]                                        # CIDEr-D is not symmetric


def test_references_are_the_other_live_rows_in_ascending_order():
    train, (df, n_doc) = _table()
    rng = np.random.default_rng(4)
    cand = C.clip_candidates(rng, 5, 8, 23)
    live = np.array([1, 0, 1, 1, 0], dtype=bool)
    u = C.utilities(cand, 5, live, df, n_doc)
    assert u[1] == 0 and u[4] == 0
    assert u[0] == float(R.score(cand[0], [cand[2], cand[3]], df, n_doc)[0])
    assert u[3] == float(R.score(cand[3], [cand[0], cand[2]], df, n_doc)[0])


def test_dead_rows_and_single_live_rows_give_zero():
    train, (df, n_doc) = _table()
    rng = np.random.default_rng(5)
    cand = np.concatenate([C.clip_candidates(rng, 3, 8, 23) for _ in range(3)])
    live = np.array([0, 0, 0, 0, 1, 0, 1, 1, 1], dtype=bool)               # no live row, one live row, all live
    u = C.utilities(cand, 3, live, df, n_doc)
    assert not u[:6].any() and (u[6:] > 0).all()
    assert not C.utilities(cand[:1], 1, None, df, n_doc).any()              # one candidate per clip: nothing to agree with


def test_pick_rule():
    u = np.array([1.0, 3.0, 3.0, 2.0,   5.0, 1.0, 1.0, 0.5,   9.0, 9.0, 9.0, 9.0,   0.0, 0.0, 0.0, 0.0])
    live = np.array([1, 1, 1, 1,   0, 1, 1, 1,   0, 0, 0, 0,   0, 0, 1, 1], dtype=bool)
    assert C.picks(u, live, 4).tolist() == [1, 1, 0, 2]                     # tie: lowest index; dead maximum skipped; no live row: 0
    assert C.picks(u, None, 4).tolist() == [1, 0, 0, 0]


def test_generator_shapes_and_kinds():
    rng = np.random.default_rng(6)
    c = C.clip_candidates(rng, 12, 9, 23, garbage=False)
    L = len(R.words(c[0])) - 1
    assert c.shape == (12, 9) and 1 <= L < 9 and c.min() >= 0 and c.max() < 23
    assert np.array_equal(c[0], c[6])                                       # j % 6 == 0: the base
    assert len(R.words(c[3])) - 1 == (L + 1) // 2 and np.array_equal(c[3][:(L + 1) // 2], c[0][:(L + 1) // 2])
    assert np.array_equal(c[4][:L], c[0][:L]) and len(R.words(c[4])) == min(L + 2, 9)
    assert (C.clip_candidates(rng, 4, 1, 5) == 0).all()                     # T = 1: the end mark alone


def test_command_line():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    from cvc import sample as cvc_sample
    o = cvc_main.build_parser().parse_args([])
    assert (o.consensus, o.consensus_samples, o.consensus_temperature, o.consensus_seed) == ("off", 16, 1.0, 1)
    for v in ("off", "samples", "beam"):
        assert cvc_main.build_parser().parse_args(["--consensus", v]).consensus == v
    with pytest.raises(SystemExit):
        cvc_main.build_parser().parse_args(["--consensus", "maybe"])
    o = cvc_main.build_parser().parse_args(["--consensus", "samples", "--consensus_samples", "4", "--consensus_temperature", "0.7",
                                            "--consensus_seed", "9"])
    assert (o.consensus_samples, o.consensus_temperature, o.consensus_seed) == (4, 0.7, 9)
    assert not hasattr(cvc_opts.build_parser().parse_args([]), "consensus")              # flags of cvc.main, not of cvc.opts
    own, rest = cvc_sample.parse(["--sample_n", "4", "--consensus", "--no_cfg"])
    assert own.consensus and own.sample_n == 4 and rest == ["--no_cfg"]
    assert not cvc_sample.parse([])[0].consensus
    with pytest.raises(SystemExit):
        cvc_sample.parse(["--sample_n", "1", "--consensus"])


def test_block_declared_listed_bound_and_not_exported():
    import build_hip
    from cvc import hip
    from test_cabi import declared_functions, BLOCKS_H
    n = "cvc_consensus_cider"
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    assert n in declared_functions(BLOCKS_H) and n in hip.BLOCKS and n in hip.SIGNATURES
    assert lib.cvc_block(n.encode())
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip.build(verbose=False)], text=True)
    assert n not in {l.split()[-1] for l in out.splitlines() if " T " in l}


def test_bad_arguments_return_badarg_before_any_launch():
    from cvc import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # non-null; never dereferenced: every call below is refused on the host

    def call(cand=p, live=None, rows=6, T=5, per=3, keys=p, idf=p, G=1, sigma=6.0, utility=p, pick=p, best=p):
        return lib.cvc_consensus_cider(cand, live, rows, T, per, keys, idf, G, 1.0, sigma, utility, pick, best, None)
    assert call(cand=None) == -1 and call(utility=None) == -1 and call(pick=None) == -1 and call(best=None) == -1
    assert call(keys=None) == -1 and call(idf=None) == -1                  # G > 0 with null tables
    assert call(rows=7) == -1 and call(rows=0) == -1                       # rows % per_clip != 0
    assert call(per=0) == -1 and call(rows=33, per=33) == -1
    assert call(T=0) == -1 and call(T=64) == -1
    assert call(sigma=0.0) == -1 and call(sigma=-1.0) == -1 and call(G=-1) == -1


def test_wrappers_refuse_what_does_not_fit():
    from cvc import hip
    from cvc.cider import CiderD
    t = CiderD.from_captions([np.array([1, 2, 0])])
    keys, idf = torch.from_numpy(t.keys_host.view(np.int64).copy()), torch.from_numpy(t.idf_host.copy())
    cand = torch.zeros(6, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.consensus_cider(cand, 4, keys, idf, t.idf_unseen)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.consensus_cider(cand, 3, keys, idf, t.idf_unseen, live=torch.ones(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.consensus_cider(cand, 3, keys, idf[:1], t.idf_unseen)
    with pytest.raises(RuntimeError, match="GPU"):                         # no CPU fallback
        hip.consensus_cider(cand, 3, keys, idf, t.idf_unseen)
    with pytest.raises(RuntimeError, match="T = 63"):
        t.consensus(torch.zeros(4, 64, dtype=torch.int64), 2)
    with pytest.raises(RuntimeError, match="per_clip = 32"):
        t.consensus(torch.zeros(66, 5, dtype=torch.int64), 33)


def test_sample_with_consensus_and_no_table_raises_before_anything_runs():
    from cvc import synth
    from helpers import build_model
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 1), torch.device("cpu"))
    assert model.consensus == "off" and model.consensus_table is None and model.last_consensus is None
    for mode in (True, "samples", "beam"):
        with pytest.raises(RuntimeError, match="consensus_table"):
            model._sample(*([None] * 11), consensus=mode)
    with pytest.raises(RuntimeError, match="consensus must be"):
        model._sample(*([None] * 11), consensus="maybe")
    assert build_model(d, synth.hot_path_state_dict(d, 1), torch.device("cpu"), consensus="samples", consensus_samples=4).consensus == "samples"
