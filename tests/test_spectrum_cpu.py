"""Spectral caption-set diversity (Self-CIDEr, LSA; csrc/spectrum.hip, cvc.metrics.set_spectrum / SpectrumScorer) without a GPU: the
definitions on hand-worked sets through the numpy restatement (tests/spectrum_ref.py), the restated Jacobi against eigvalsh, the
result formulae, the flags, the block's declaration and the host-side refusals."""
import ctypes
import math
import subprocess

import numpy as np
import pytest
import torch

import spectrum_ref as S

UNSEEN = np.float32(math.log(100.0))


def _clip(rows, T=6):
    out = np.zeros((len(rows), T), np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _k_lam_scores(rows, mode="cider", live=None, table=None, unseen=UNSEEN):
    cand = _clip(rows)
    ws = S.live_rows(cand, len(rows), live, 0)
    K = S.gram64(ws, mode, table or {}, unseen)
    lam = S.spectrum(K)
    return K, lam, S.scores(lam, float(np.trace(K)), len(ws)), len(ws)


def test_hand_worked_two_rows():
    # "a b" / "a c", an empty table: every idf is idf_unseen and cancels.  Unigrams: cos = 1/2; bigrams: nothing shared; orders 3, 4:
    # no n-gram, s = 0.  K[a, a] = min(L, 4) / 4 = 1/2, K[a, b] = 1/4 * 1/2.
    K, lam, sc, m = _k_lam_scores([[1, 2], [1, 3]])
    assert m == 2 and np.allclose(K, [[0.5, 0.125], [0.125, 0.5]], rtol=0, atol=1e-16)
    assert np.allclose(lam[:2], [0.625, 0.375], rtol=0, atol=1e-15) and (lam[2:] == 0).all()
    assert abs(sc[0] - -math.log2(0.625)) < 1e-14
    want1 = -math.log2(math.sqrt(0.625) / (math.sqrt(0.625) + math.sqrt(0.375)))
    assert abs(sc[1] - want1) < 1e-14
    K32 = S.gram32(S.live_rows(_clip([[1, 2], [1, 3]]), 2, None, 0), "cider", {}, UNSEEN)
    assert K32.dtype == np.float32 and np.array_equal(K32, np.float32([[0.5, 0.125], [0.125, 0.5]]))


@pytest.mark.parametrize("m", [2, 3, 5])
def test_identical_captions_score_zero_and_disjoint_captions_score_one(m):
    K, lam, sc, _ = _k_lam_scores([[4, 5, 6, 7, 8]] * m)
    tr = float(np.trace(K))
    assert abs(tr - m) < 1e-14 and abs(lam[0] - tr) < 1e-14 * tr and abs(sc[0]) < 1e-14 and abs(sc[1]) < 1e-7
    K32 = S.gram32(S.live_rows(_clip([[4, 5, 6, 7, 8]] * m), m, None, 0), "cider", {}, UNSEEN)
    assert np.array_equal(K32, np.ones((m, m), np.float32))                 # equal rows: exactly rank 1 in float32 too
    K, lam, sc, _ = _k_lam_scores([[10 * a + 1, 10 * a + 2, 10 * a + 3, 10 * a + 4] for a in range(m)])
    assert np.allclose(K, np.eye(m), rtol=0, atol=1e-15) and abs(sc[0] - 1) < 1e-14 and abs(sc[1] - 1) < 1e-14


def test_dead_rows_empty_rows_and_sets_of_one_or_none():
    rows = [[1, 2, 3, 4], [5, 6, 7, 8], [1, 2, 3, 4]]
    K, lam, sc, m = _k_lam_scores(rows, live=[1, 1, 0])                      # the dead row is left out of m
    assert m == 2 and np.allclose(K, np.eye(2), atol=1e-15) and abs(sc[0] - 1) < 1e-14
    K, lam, sc, m = _k_lam_scores([[1, 2, 3, 4], [], [5, 6, 7, 8]])          # a live row with L = 0: counted, a zero row
    assert m == 3 and (K[1] == 0).all() and (K[:, 1] == 0).all() and abs(float(np.trace(K)) - 2) < 1e-15
    assert abs(sc[0] - math.log(2) / math.log(3)) < 1e-14
    for live in ([1, 0, 0], [0, 0, 0]):                                     # m = 1, m = 0
        K, lam, sc, m = _k_lam_scores(rows, live=live)
        assert m == sum(live) and sc == (0.0, 0.0) and (lam[m:] == 0).all()
    assert _k_lam_scores([[], []])[2] == (0.0, 0.0)                          # tr = 0


def test_a_table_weighs_the_words():
    # idf(a) = 0 (in every document): "a b" / "a c" share nothing that weighs -- the unigram cosine is 0; an absent key is unseen
    table = {S.key_of((1,)): np.float32(0.0)}
    K, _, _, _ = _k_lam_scores([[1, 2], [1, 3]], table=table)
    assert np.allclose(K, [[0.5, 0], [0, 0.5]], atol=1e-16)
    table = {S.key_of((1,)): np.float32(1.0), S.key_of((2,)): np.float32(2.0)}          # (3,) unseen: idf = 3
    K, _, _, _ = _k_lam_scores([[1, 2], [1, 3]], table=table, unseen=np.float32(3.0))
    assert abs(K[0, 1] - 0.25 * 1 / (math.sqrt(5) * math.sqrt(10))) < 1e-16


def test_lsa_counts():
    K, lam, sc, m = _k_lam_scores([[1, 1, 2], [1, 2]], mode="lsa")           # "a a b" / "a b": counts (2, 1) and (1, 1)
    assert np.array_equal(K, [[5, 3], [3, 2]])
    l1, l2 = (7 + math.sqrt(45)) / 2, (7 - math.sqrt(45)) / 2
    assert np.allclose(lam[:2], [l1, l2], rtol=1e-14)
    assert abs(sc[0] - -math.log2(l1 / 7)) < 1e-13 and abs(sc[1] - -math.log2(math.sqrt(l1) / (math.sqrt(l1) + math.sqrt(l2)))) < 1e-13
    assert np.array_equal(S.gram32(S.live_rows(_clip([[1, 1, 2], [1, 2]]), 2, None, 0), "lsa"), np.float32([[5, 3], [3, 2]]))


def test_float32_restatement_stays_near_fp64_on_the_generated_cases():
    worst = 0.0
    for per_clip, T in ((5, 20), (9, 4), (32, 3)):
        cand, live = S.case(11 * per_clip + T, 7, per_clip, T)
        for clip in range(7):
            ws = S.live_rows(cand, per_clip, live, clip)
            K64, K32 = S.gram64(ws, "cider", {}, UNSEEN), S.gram32(ws, "cider", {}, UNSEEN)
            assert np.array_equal(K32, K32.T)
            worst = max(worst, float(np.abs(K32 - K64).max()) if len(ws) else 0.0)
            assert np.array_equal(S.gram32(ws, "lsa").astype(np.float64), S.gram64(ws, "lsa"))
    assert worst < 16 * 2.0 ** -24                  # a handful of float32 roundings of values <= 1


def test_restated_jacobi_against_eigvalsh():
    rng = np.random.default_rng(5)
    worst, most = 0.0, 0
    for m in (1, 2, 3, 8, 9, 31, 32):
        for kind in ("full", "rank1", "paired", "zero_row"):
            X = rng.random((m, 6))
            if kind == "rank1":
                X[:] = X[0]
            elif kind == "paired":
                X[1::2] = X[0::2][:X[1::2].shape[0]]
            elif kind == "zero_row":
                X[m // 2] = 0
            K = X @ X.T
            K = (K + K.T) / 2
            lam, sweeps = S.jacobi(K)
            want = np.linalg.eigvalsh(K)[::-1]
            tr = float(np.trace(K))
            assert 1 <= sweeps <= 16
            if tr > 0:
                worst = max(worst, float(np.abs(lam - want).max()) / (S.U * tr))
            most = max(most, sweeps)
    assert worst <= 256 and most <= 12, (worst, most)


def test_result_formulae_and_merging_of_sums():
    from cvc import metrics
    assert metrics.SPECTRUM_KEYS == ("Self_CIDEr", "LSA", "Spectrum_sets")
    assert metrics.spectrum_from_sums([1.5, 3, 1.0, 4, 5]) == {"Self_CIDEr": 0.5, "LSA": 0.25, "Spectrum_sets": 5}
    assert metrics.SpectrumScorer().result() == {"Self_CIDEr": 0.0, "LSA": 0.0, "Spectrum_sets": 0}
    s = metrics.SpectrumScorer()
    s.add_sums([1.5, 3, 1.0, 4, 5])
    s.add_sums(torch.tensor([0.5, 1, 1.0, 4, 4], dtype=torch.float64))
    assert s.sums() == [2.0, 4.0, 2.0, 8.0, 9.0] and s.result() == {"Self_CIDEr": 0.5, "LSA": 0.25, "Spectrum_sets": 9}
    with pytest.raises(RuntimeError, match="nothing to score"):
        metrics.SpectrumScorer(None, lsa=False)
    assert S.headline([0.5, 0.9, 0.1], [2, 1, 3], [True, True, True]) == 0.3


def test_command_line():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    from cvc import sample as cvc_sample
    o = cvc_main.build_parser().parse_args([])
    assert not hasattr(o, "val_self_cider") and not hasattr(o, "val_diversity")         # default off: no key in the options
    cvc_main.check_val_diversity_flag(o)
    assert not hasattr(cvc_opts.build_parser().parse_args([]), "val_self_cider")
    ok = cvc_main.build_parser().parse_args(["--val_diversity", "--val_self_cider", "--val_metrics", "device", "--consensus", "samples"])
    assert ok.val_self_cider is True and ok.val_diversity is True
    cvc_main.check_val_diversity_flag(ok)
    only_div = cvc_main.build_parser().parse_args(["--val_diversity", "--val_metrics", "device", "--consensus", "samples"])
    assert not hasattr(only_div, "val_self_cider")
    with pytest.raises(SystemExit, match="--val_self_cider needs --val_diversity"):
        cvc_main.check_val_diversity_flag(cvc_main.build_parser().parse_args(["--val_self_cider", "--val_metrics", "device",
                                                                              "--consensus", "samples"]))
    with pytest.raises(SystemExit, match="--val_self_cider needs --val_diversity"):     # the run ends before any set-up
        cvc_main.main(["--no_cfg", "--val_self_cider"])
    with pytest.raises(SystemExit, match="--val_metrics device"):
        cvc_main.main(["--no_cfg", "--val_diversity", "--val_self_cider"])
    own, rest = cvc_sample.parse(["--sample_n", "4", "--diversity", "--self_cider", "--no_cfg"])
    assert own.diversity and own.self_cider and rest == ["--no_cfg"]
    assert not cvc_sample.parse(["--sample_n", "4", "--diversity"])[0].self_cider
    with pytest.raises(SystemExit, match="--self_cider needs --diversity"):
        cvc_sample.parse(["--sample_n", "4", "--self_cider"])


def test_trainer_refusals():
    from cvc.trainer import Trainer
    tr = Trainer.__new__(Trainer)                # the refusal comes before anything of the trainer is touched but its model
    tr.model = torch.nn.Linear(1, 1)
    with pytest.raises(RuntimeError, match="needs diversity=True"):
        tr.sample(5, 1.0, self_cider=True)
    with pytest.raises(RuntimeError, match="needs val_diversity=True"):
        Trainer(None, None, torch.nn.Linear(1, 1), None, None, None, val_self_cider=True)


def test_block_declared_listed_bound_and_not_exported():
    import build_hip
    from cvc import hip
    from test_cabi import declared_functions, BLOCKS_H
    n = "cvc_caption_set_spectrum"
    lib = hip.lib()
    lib.cvc_block.restype = ctypes.c_void_p
    decl = declared_functions(BLOCKS_H)
    assert n in decl and n in hip.BLOCKS and n in hip.SIGNATURES and callable(hip.caption_set_spectrum)
    assert len(hip.SIGNATURES[n]) == 15
    assert lib.cvc_block(n.encode())
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip.build(verbose=False)], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert n not in exported and len(exported) == 70                         # the exported core surface stays at 70 entry points
    assert "spectrum.hip" in build_hip.NO_SCRATCH_KERNELS                    # the build refuses scratch or spills for the kernel


def test_bad_arguments_return_badarg_before_any_launch():
    from cvc import hip
    lib = hip.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                    # non-null; never dereferenced: every call below is refused on the host

    def call(cand=p, live=None, rows=6, T=5, per=3, mode=0, keys=p, idf=p, G=4, gram=None, lam=p, score=p, info=p):
        return lib.cvc_caption_set_spectrum(cand, live, rows, T, per, mode, keys, idf, G, 1.0, gram, lam, score, info, None)
    assert call(cand=None) == -1 and call(lam=None) == -1 and call(score=None) == -1 and call(info=None) == -1
    assert call(keys=None) == -1 and call(idf=None) == -1                  # mode cider with G > 0 needs the table
    assert call(per=0) == -1 and call(rows=33, per=33) == -1
    assert call(T=0) == -1 and call(T=64) == -1
    assert call(rows=7) == -1 and call(rows=0) == -1                       # rows % per_clip != 0
    assert call(mode=2) == -1 and call(mode=-1) == -1


def test_wrappers_refuse_what_does_not_fit():
    from cvc import hip, metrics
    from cvc.cider import CiderD
    cand = torch.zeros(6, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.caption_set_spectrum(cand, 4, "lsa")
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.caption_set_spectrum(cand, 3, "lsa", live=torch.ones(5, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="do not fit"):
        hip.caption_set_spectrum(cand, 3, "cider", torch.zeros(3, dtype=torch.int64), torch.zeros(2))
    with pytest.raises(RuntimeError, match="one of"):
        hip.caption_set_spectrum(cand, 3, "pca")
    with pytest.raises(RuntimeError, match="needs the idf table"):
        hip.caption_set_spectrum(cand, 3, "cider")
    with pytest.raises(RuntimeError, match="GPU"):                         # no CPU fallback
        metrics.set_spectrum(cand, 3)
    with pytest.raises(RuntimeError, match="T = 63"):
        metrics.set_spectrum(torch.zeros(4, 64, dtype=torch.int64), 2)
    with pytest.raises(RuntimeError, match="per_clip = 32"):
        metrics.set_spectrum(torch.zeros(66, 5, dtype=torch.int64), 33)
    with pytest.raises(RuntimeError, match="T = 63"):
        CiderD(np.zeros(0, np.uint64), np.zeros(0, np.float32), 10).self_cider(torch.zeros(4, 64, dtype=torch.int64), 2)
