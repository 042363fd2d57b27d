"""Lexically constrained beam search (forced words per clip) without a GPU: the two building blocks in the library's table and their
host-side argument checks, the engine's and the model's refusals, the host helper that turns detections into forced words, the docs,
and the fp64 reference (tests/force_ref.py): with no active entry bank 0 is beam_constrain_ref.decode at beam bd, the invariant
holds, the margins of the committed cases allow an exact GPU comparison, and the ranking key."""
import ctypes
import inspect
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from cvc import synth
from oracle import ref_cpu as O
import tile_path_cases as T
import beam_constrain_ref as BR
import force_ref as FR
import force_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNK = synth.UNK_IDX
NAMES = ("cvc_beam_select_force_parts", "cvc_beam_rank_force")
BADARG, TOOBIG = -1, -2


# ------------------------------------------------------------------ the blocks: table, binding, argument checks
def test_blocks_are_in_the_table_and_bound_with_the_headers_argument_counts():
    import subprocess
    import build_hip
    from cvc import hip
    so = build_hip.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read(), flags=re.S)
    lib = ctypes.CDLL(so)
    lib.cvc_block.restype = ctypes.c_void_p
    lib.cvc_block.argtypes = [ctypes.c_char_p]
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    blocks_src = open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "blocks.hip")).read()
    nargs = {}
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert m, name
        nargs[name] = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in hip.BLOCKS and len(hip.SIGNATURES[name]) == nargs[name], name
        assert lib.cvc_block(name.encode()), name
        assert not re.search(r"\b" + name + r"\b", exported), name                       # the exported ABI does not grow
        assert f"CVC_B({name})" in blocks_src
    # the history block's arguments + force, nforce, nmet; the ranking's + force, nforce, V, unk_idx, nmet
    assert nargs[NAMES[0]] == len(hip.SIGNATURES["cvc_beam_select_hist_parts"]) + 3
    assert nargs[NAMES[1]] == len(hip.SIGNATURES["cvc_beam_rank"]) + 5
    # one definition: the header states the rule, the kernels' comment states it, the workspace size is said
    header = open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read()
    beam = open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "beam.hip")).read()
    for text in (header, beam):
        assert all(k in text for k in ("ACTIVE iff 0 < w < V", "Routing uses", "invariant", "21 * B * beam floats"))
    assert "bd + 2 C" in beam and "64 at beam 8, C = 3" in beam                            # the sufficiency argument, in the kernel comment


def test_host_argument_checks_return_their_codes_and_launch_nothing():
    from cvc import hip
    L = hip.lib()
    fake, fake2 = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def call(parts=fake, nparts=1, score=fake, done=fake, B=3, beam=6, V=50, t=0, hin=fake, hout=fake2, hstride=18, n=0, min_len=0,
             nban=0, ban=None, force=fake, C=2, parent=fake, word=fake, score_out=fake, done_out=fake, ws=fake):
        c = hip.Constraint(n, 0, min_len, nban, ban, None, 0)
        return L.cvc_beam_select_force_parts(parts, nparts, 0, None, score, done, B, beam, V, 1, t, hin, hout, hstride, c, force, C,
                                             parent, word, score_out, done_out, None, None, ws, None)

    # every check of the history block
    for kw in (dict(parts=None), dict(score=None), dict(done=None), dict(parent=None), dict(word=None), dict(score_out=None),
               dict(done_out=None), dict(ws=None), dict(nparts=0), dict(B=0), dict(beam=0), dict(beam=9), dict(V=6), dict(V=8193),
               dict(t=3, hin=None), dict(hout=None), dict(hin=fake, hout=fake), dict(hstride=17), dict(n=-1), dict(n=65), dict(min_len=-1),
               dict(nban=257, ban=fake), dict(nban=3, ban=None)):
        assert call(**kw) == BADARG, kw
    assert call(t=-1) == TOOBIG and call(t=65) == TOOBIG
    # the forced words
    for kw in (dict(force=None), dict(C=0), dict(C=-1), dict(C=4), dict(C=3), dict(beam=8, C=2), dict(beam=5, C=1), dict(beam=7, C=3)):
        assert call(**kw) == BADARG, kw

    def rank(h=fake, stride=18, sc=fake, force=fake, C=2, B=3, beam=6, T=10, V=50, alpha=0.7, order=fake, norm=fake, ln=fake, nmet=fake):
        return L.cvc_beam_rank_force(h, stride, sc, force, C, B, beam, T, V, 1, alpha, order, norm, ln, nmet, None)

    for kw in (dict(h=None), dict(sc=None), dict(order=None), dict(norm=None), dict(ln=None), dict(B=0), dict(beam=0), dict(beam=9),
               dict(T=0), dict(stride=17), dict(alpha=-0.5), dict(alpha=float("inf")), dict(alpha=float("nan")),
               dict(force=None), dict(nmet=None), dict(C=0), dict(C=4), dict(V=0)):
        assert rank(**kw) == BADARG, kw
    assert rank(T=65) == TOOBIG


# ------------------------------------------------------------------ the engine's and the model's refusals, the helper, the docs
def test_engine_refuses_before_anything_is_allocated():
    from cvc.decode import DecodeEngine
    assert inspect.signature(DecodeEngine.__init__).parameters["force_n"].default == 0
    W = types.SimpleNamespace(V=50, R=32, A=32, E=32)
    new = lambda T=4, W=W, **kw: DecodeEngine.__init__(object.__new__(DecodeEngine), W, {}, T, 1, **kw)
    with pytest.raises(RuntimeError, match=r"force_n needs beam_history=True"):
        new(beam=6, force_n=2)
    with pytest.raises(RuntimeError, match=r"force_n.*beam > 1"):
        new(force_n=1)
    with pytest.raises(RuntimeError, match=r"force_n = 3 needs beam % \(force_n \+ 1\) == 0"):
        new(beam=6, beam_history=True, force_n=3)
    for bad in (-1, 4, 1.0, True, None):
        with pytest.raises(RuntimeError, match="force_n must be an integer in 0 .. 3"):
            new(beam=6, beam_history=True, force_n=bad)
    with pytest.raises(RuntimeError, match=r"force_n and beam_groups > 1 exclude"):
        new(beam=6, beam_history=True, force_n=2, beam_groups=3)
    # gsk / gate_ksplit / lang_ksx, sampling, the teacher-forced mode and bf16 weights stay exclusive with beam search
    on = dict(beam=6, beam_history=True, force_n=2, length_penalty=0.7, no_repeat_ngram=2)
    for kw in (dict(gsk=True), dict(gate_ksplit=True), dict(lang_ksx=True)):
        with pytest.raises(RuntimeError, match="default schedules"):
            new(**on, **kw)
    for kw in (dict(temperature=0.7), dict(forced_n=1), dict(weights_dtype="bf16")):
        with pytest.raises(RuntimeError, match="beam search"):
            new(**on, **kw)
    with pytest.raises(RuntimeError, match="T <= 64"):
        new(T=65, **on)


def test_load_force_words_refuses_bad_words_before_it_copies():
    from cvc.decode import DecodeEngine
    e = object.__new__(DecodeEngine)
    e.forcing, e.B, e.force_n, e.W, e.cons = True, 3, 2, types.SimpleNamespace(V=50), (0, False, 0, (7, 9), ())
    with pytest.raises(RuntimeError, match=r"load_force_words: words must be integers \[3, 2\]"):
        e.load_force_words(np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(RuntimeError, match=r"load_force_words: words must be integers \[3, 2\]"):
        e.load_force_words(torch.zeros(3, 2))
    with pytest.raises(RuntimeError, match=r"ids outside \[0, V = 50\): \[50, 77\]"):
        e.load_force_words([[4, 50], [-1, 77], [5, 6]])
    with pytest.raises(RuntimeError, match=r"ban_words forbids cannot be forced: \[9\]"):
        e.load_force_words(torch.tensor([[4, 9], [-1, 3], [5, 6]]))
    e.forcing = False
    with pytest.raises(RuntimeError, match="force_n = 0"):
        e.load_force_words([[4, 5], [-1, 3], [5, 6]])


def test_detected_force_words_on_a_hand_made_proposal_array():
    from cvc.misc.utils import detected_force_words
    itod = {"1": "dog", "2": "hot dog", "3": "frisbee", "4": "zebra", "5": "cat", "6": "UNK", "7": "end", "8": "man"}
    wtoi = {"dog": "11", "frisbee": "12", "cat": "13", "UNK": str(UNK), "end": "0", "man": "14", "hot": "15"}      # (the loader's values are strings)
    P = np.zeros((4, 6, 7), dtype=np.float32)
    row = lambda cls, score: [0, 0, 1, 1, 0, cls, score]
    # clip 0: dog twice (its best score counts), frisbee, cat; a better-scored cat lies past the valid count
    P[0] = [row(1, 0.5), row(3, 0.8), row(1, 0.9), row(5, 0.6), row(5, 0.99), row(8, 0.95)]
    # clip 1: classes without a single vocabulary word (two words, not in the vocabulary, UNK, word 0, background 0) and one that has
    P[1] = [row(2, 0.9), row(4, 0.9), row(6, 0.9), row(7, 0.9), row(0, 0.9), row(8, 0.1)]
    # clip 2: equal scores -> the lower class index first
    P[2] = [row(8, 0.7), row(5, 0.7), row(3, 0.7), row(1, 0.2), row(0, 0), row(0, 0)]
    # clip 3: no valid proposal
    P[3] = [row(1, 0.9)] * 6
    num = np.zeros((4, 7), dtype=np.float32)
    num[:, 1] = [4, 6, 4, 0]
    for args in ((torch.from_numpy(P), torch.from_numpy(num)), (P, num)):
        assert detected_force_words(*args, 3, itod, wtoi, UNK).tolist() == [[11, 12, 13], [14, -1, -1], [12, 13, 14], [-1, -1, -1]]
        assert detected_force_words(*args, 2, itod, wtoi, UNK).tolist() == [[11, 12], [14, -1], [12, 13], [-1, -1]]
        assert detected_force_words(*args, 1, itod, wtoi, UNK).tolist() == [[11], [14], [12], [-1]]
    out = detected_force_words(P, num, 2, {k: "cls%d" % k for k in range(1, 9)}, {"UNK": UNK}, UNK)      # the synthetic dataset's maps
    assert out.dtype == torch.int64 and out.tolist() == [[-1, -1]] * 4


def test_model_cli_and_docs_know_the_switches():
    from cvc.model import captioner
    from cvc.decode import DecodeEngine
    from cvc import main as cvc_main
    src = inspect.getsource(captioner)
    assert re.search(r"beam_history=beam > 1 and \(any\(cons\.values\(\)\).*or force_n > 0\)", src)
    # the engine-cache key is made of every option _sample passes on (the key itself: tests/test_decode_mode_cpu.py)
    call = re.search(r'self\._decode_engine\(\s*"_engine_cache".*?\*\*cons\)', src, re.S).group(0)
    assert "top_k=k, top_p=p" in call and "force_n=force_n" in call
    assert "force_words" in inspect.signature(captioner.DecodeAndGroundCaptionerGVDROI._sample).parameters
    main_src = inspect.getsource(cvc_main)
    assert all(f'"--{k}"' in main_src for k in ("force_words", "force_detected"))
    assert 'word_ids(opt.force_words, opt.wtoi, "--force_words")' in main_src             # the resolver of --ban_words
    from cvc import opts as cvc_opts                           # ... of this entry point, not of the pinned reference option surface
    assert not {a.dest for a in cvc_opts.build_parser()._actions} & {"force_words", "force_detected"}
    doc = DecodeEngine.__init__.__doc__
    assert all(k in doc for k in ("force_n", "load_force_words", "cvc_beam_select_force_parts", "cvc_beam_rank_force"))
    assert "nmet" in DecodeEngine.hypotheses.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### Forced words" in design
    sect = design.split("### Forced words")[1]
    assert all(k in sect for k in ("cvc_beam_select_force_parts", "cvc_beam_rank_force", "force_n", "LDS", "VGPR", "not measured"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "force_n" in readme and "--force_words" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_beam_forced.py"))


# ------------------------------------------------------------------ the reference
def test_the_active_entries():
    assert FR.active([5, 7, 9], 50, UNK) == [True, True, True]
    assert FR.active([-1, 0, UNK], 50, UNK) == [False, False, False]
    assert FR.active([50, 49, 49], 50, UNK) == [False, True, False]
    assert FR.active([7, 7, 7], 50, UNK) == [True, False, False]
    assert FR.active([1000], 50, UNK) == [False]


@pytest.mark.parametrize("name,seed,bd,C,rules", [("tiny", 4321, 2, 1, dict(no_repeat_ngram=2)), ("cfg1", 4321, 2, 2, dict(no_repeat_ngram=2)),
                                                  ("cfg1", 5, 1, 3, {})])
def test_with_no_active_entry_bank_zero_is_the_constrained_beam_reference(name, seed, bd, C, rules):
    d = synth.CONFIGS[name]
    P, f = O.to_torch(synth.hot_path_state_dict(d, seed)), O.to_torch(synth.clip_features(d, seed))
    beam = (C + 1) * bd
    force = np.array([[-1, 0, UNK], [d.V, d.V + 5, -7], [UNK, UNK, 0]] * d.B, dtype=np.int32)[:d.B, :C]
    with torch.no_grad():
        wide = FR.decode(P, f, d.T, UNK, beam, force, **rules)
        narrow = BR.decode(P, f, d.T, UNK, bd, **rules)
    assert narrow["margin"].min() >= FR.MARGIN_MIN
    assert torch.equal(wide["seq"][:, :bd], narrow["seq"]) and torch.equal(wide["parent"][:, :, :bd], narrow["parent"])
    assert torch.equal(wide["word"][:, :, :bd], narrow["word"])
    # (the oracle's fp32 decoder step on beam rows and on bd rows: other GEMM blocking, not the same bits)
    np.testing.assert_allclose(wide["score"][:, :bd].numpy(), narrow["score"].numpy(), rtol=0, atol=5e-5)
    assert bool((wide["score"][:, bd:] == -math.inf).all()) and not bool(wide["live"][:, :, bd:].any())      # the other banks: fillers
    assert int(wide["nmet"].max()) == 0 and int(wide["final_nmet"].max()) == 0
    assert np.array_equal(wide["order"][:, :bd], np.tile(np.arange(bd), (d.B, 1)))


# measured on this reference: the smallest selection margin (the issue's table), the smallest gap of the final norm order among slots
# that met equally many forced words (inf: no two such slots), clips whose best hypothesis is not slot 0 -- per case of FR.ENGINE_CASES
EXPECT = [(1.43e-3, 3.17, 2), (1.44e-3, 2.34e-3, 3), (1.49e-3, math.inf, 3), (4.48e-3, 4.48e-3, 3), (2.07e-3, 1.36e-3, 2),
          (1.76e-3, 7.12e-4, 4), (6.46e-3, math.inf, 4), (1.68e-3, 8.83e-4, 4)]


@pytest.mark.parametrize("i", range(len(FR.ENGINE_CASES)))
def test_the_margins_allow_an_exact_comparison_and_the_invariant_holds(i):
    name, seed, beam, C, alpha, eos, rules = FR.ENGINE_CASES[i]
    d, P, f, force, r = FR.shared_decode(i)
    bd = beam // (C + 1)
    sel, rk, moved = EXPECT[i]
    print(FR.ENGINE_CASES[i], "selection margin", r["margin"].min(), "rank margin", r["rank_margin"], "best != slot 0",
          int((r["order"][:, 0] != 0).sum()), "len", r["len"].min(), r["len"].max())
    assert r["margin"].min() >= FR.MARGIN_MIN and r["rank_margin"] >= FR.MARGIN_MIN
    assert abs(r["margin"].min() - sel) <= 0.05 * sel + 1e-5                               # the table's figures
    assert (r["rank_margin"] == rk) if math.isinf(rk) else abs(r["rank_margin"] - rk) <= 0.05 * rk + 1e-5
    assert int((r["order"][:, 0] != 0).sum()) == moved
    assert force.shape == (d.B, C) and bool((force[::3, C - 1] == -1).all())               # clips with b % 3 == 0 lost their last entry
    # the invariant: every finite hypothesis of bank j holds exactly j active forced words (decode() asserts it at every step too)
    assert not FR.invariant_violations(dict(hist=r["seq"].view(-1, d.T).numpy(), score=r["score"]), force, beam, d.V, UNK)
    finite = torch.isfinite(r["score"])
    assert np.array_equal(r["final_nmet"][finite.numpy()], np.broadcast_to(r["bank"], (d.B, beam))[finite.numpy()])
    for b in range(d.B):
        nact = sum(FR.active(force[b], d.V, UNK))
        want = {int(w) for w, a in zip(force[b], FR.active(force[b], d.V, UNK)) if a}
        assert bool(finite[b, nact * bd])                                                  # every clip reaches its top bank ...
        assert not bool(finite[b, (nact + 1) * bd:].any())                                 # ... and no bank above it exists
        best = int(r["order"][b, 0])
        assert best // bd == nact and want <= set(r["seq"][b, best].tolist())              # run()'s caption holds every forced word
        assert r["norm"][b, best] == max(r["norm"][b, k] for k in range(nact * bd, (nact + 1) * bd) if finite[b, k])
    assert torch.equal(BR.backtrack_all(r["word"], r["parent"])[finite], r["seq"][finite])  # the histories are the parents walked back
    n = rules.get("no_repeat_ngram", 0)
    for h in r["seq"][finite].tolist():
        assert UNK not in h and (n == 0 or not BR.repeats_ngram(BR.cut(h), n))
    if eos > 0:                                                # the length penalty has lengths to rank
        assert r["len"].min() < r["len"].max()


@pytest.mark.parametrize("alpha", [0.0, 0.7])
def test_the_ranking_key(alpha):
    B, beam, Tn, V, hist, score, force = FC.rank_case()
    seq = hist.T.reshape(B, beam, Tn)
    r = FR.rank(seq, score.reshape(B, beam), alpha, force, V, UNK)
    want_nmet = [[0, 0, 1, 3, 1, 2], [1, 0, 1, 0, 0, 1], [2, 1, 2, 0, 1, 0], [1, 1, 0, 2, 3, 3]]
    assert r["nmet"].tolist() == want_nmet
    for b in range(B):
        o, norm, nmet = r["order"][b], r["norm"][b], r["nmet"][b]
        assert sorted(o.tolist()) == list(range(beam))
        cls = [2 if np.isnan(norm[k]) else 1 if norm[k] == -np.inf else 0 for k in o]
        assert cls == sorted(cls)                                                          # finite, then -inf, then NaN
        for a, c in zip(o[:-1], o[1:]):
            if np.isnan(norm[a]) == np.isnan(norm[c]) and (norm[a] == -np.inf) == (norm[c] == -np.inf):
                assert nmet[a] >= nmet[c]
                if nmet[a] == nmet[c] and not np.isnan(norm[a]):
                    assert norm[a] > norm[c] or (norm[a] == norm[c] and a < c)
                if nmet[a] == nmet[c] and np.isnan(norm[a]):
                    assert a < c
    if alpha == 0.0:
        assert r["order"].tolist() == [[3, 5, 4, 2, 1, 0], [0, 2, 4, 1, 3, 5], [1, 5, 3, 2, 0, 4], [4, 3, 0, 1, 2, 5]]
    # a slot with a worse norm that met more comes first; a -inf slot that met everything still follows every finite slot
    assert list(r["order"][0]).index(3) < list(r["order"][0]).index(1) and r["norm"][0, 3] < r["norm"][0, 1]
    assert r["order"][3, -1] == 5 and r["nmet"][3, 5] == 3
    # with no active entry the order is beam_groups_ref's
    import beam_groups_ref as GR
    none = FR.rank(seq, score.reshape(B, beam), alpha, np.full((B, 2), -1), V, UNK)
    assert np.array_equal(none["order"], GR.rank(seq, score.reshape(B, beam), alpha)["order"]) and int(none["nmet"].max()) == 0


# ------------------------------------------------------------------ the block cases
@pytest.mark.parametrize("si,beam,C", FC.BLOCK_CASES)
def test_the_block_cases_hold_what_they_are_meant_to_hold(si, beam, C):
    V = FC.SHAPES[si][0]
    rules, hist, force = FC.rules_of(si), FC.planted_history(si, beam), FC.force_of(si, C)
    bd = beam // (C + 1)
    seen_n, off_bank, outside, inside, banned_forced, banned_unmet, fillers = set(), False, False, False, False, False, False
    for t in FC.STEPS:
        c = FC.base_case(si, beam, t == 0)
        r = FC.block_ref(si, beam, C, t)
        assert not FR.gap_violations(r, T.GAP), (si, beam, C, t, FR.gap_violations(r, T.GAP)[:3])      # exactly tied or a grid step apart
        assert not FR.invariant_violations(r, force, beam, V, c["unk"])
        assert bool(c["done"].any()) == (t != 0) and not bool(c["done"].all())           # frozen rows (drawn at 40 %) next to live ones
        ban = FR.CR.banned(hist.T, t, V, c["unk"], **rules)
        x = c["logits"].double().clone()
        x[torch.from_numpy(ban)] = -math.inf
        top = torch.sort(x, dim=1, descending=True, stable=True).indices
        for row, (have, unmet) in enumerate(FR.met_sets(force, hist.T, t, beam, V, c["unk"])):
            if t > 0:
                seen_n.add(len(have))
                off_bank |= len(have) != (row % beam) // bd
            if bool(c["done"][row]):
                continue
            outside |= any(w not in top[row, :beam].tolist() for w in unmet)
            inside |= any(w in top[row, :bd + C].tolist() and not ban[row, w] for w in unmet)
            banned_forced |= any(ban[row, w] for w in have)
            banned_unmet |= any(ban[row, w] for w in unmet)
        fillers |= not bool(r["live"].all())
    nact = max(sum(FR.active(f, V, FC.UNK)) for f in force)
    assert seen_n == set(range(nact + 1)) and off_bank          # rows of every n, and rows whose n is not their slot's bank
    assert inside and banned_forced and fillers                 # a forced word among a row's first bd + C entries; one the bigram rule bans
    assert outside or V == 8                                    # a forced word outside a row's top-`beam` (V = 8: the list holds most of the row)
    assert banned_unmet == (V == 8 and C == 3)                  # V = 8: clip 0 forces a word of ban_words
