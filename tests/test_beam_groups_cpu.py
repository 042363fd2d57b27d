"""Diverse (group) beam search and the length-normalised final ranking without a GPU: the three building blocks in the library's
table and their host-side argument checks, the engine's and the model's refusals, the docs, and the fp64 reference
(tests/beam_groups_ref.py): with one group and no penalty it is beam_constrain_ref.decode, with lambda = 0 every group is the
width-bd beam search, and the margins of the committed cases allow an exact GPU comparison."""
import ctypes
import inspect
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
import beam_groups_ref as GR
import beam_groups_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNK = synth.UNK_IDX
NAMES = ("cvc_beam_select_groups_parts", "cvc_beam_rank", "cvc_beam_backtrack_from")
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
    # the history block's arguments + groups, lambda; the backtrack's + start, start_stride
    assert nargs[NAMES[0]] == len(hip.SIGNATURES["cvc_beam_select_hist_parts"]) + 2
    assert nargs[NAMES[1]] == 11
    assert nargs[NAMES[2]] == len(hip.SIGNATURES["cvc_beam_backtrack"]) + 2
    beam = open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "beam.hip")).read()
    merge = beam.split("void beam_merge_kernel(")[1].split("__global__")[0]
    assert "atomic" not in merge


def test_host_argument_checks_return_their_codes_and_launch_nothing():
    from cvc import hip
    L = hip.lib()
    fake, fake2 = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def call(parts=fake, nparts=1, score=fake, done=fake, B=3, beam=6, V=50, t=0, hin=fake, hout=fake2, hstride=18, n=0, min_len=0,
             nban=0, ban=None, groups=2, lam=0.5, parent=fake, word=fake, score_out=fake, done_out=fake, ws=fake):
        c = hip.Constraint(n, 0, min_len, nban, ban, None, 0)
        return L.cvc_beam_select_groups_parts(parts, nparts, 0, None, score, done, B, beam, V, 1, t, hin, hout, hstride, c, groups, lam,
                                              parent, word, score_out, done_out, None, ws, None)

    # every check of the history block
    for kw in (dict(parts=None), dict(score=None), dict(done=None), dict(parent=None), dict(word=None), dict(score_out=None),
               dict(done_out=None), dict(ws=None), dict(nparts=0), dict(B=0), dict(beam=0), dict(beam=9, groups=3), dict(V=6), dict(V=8193),
               dict(t=3, hin=None), dict(hout=None), dict(hin=fake, hout=fake), dict(hstride=17), dict(n=-1), dict(n=65), dict(min_len=-1),
               dict(nban=257, ban=fake), dict(nban=3, ban=None)):
        assert call(**kw) == BADARG, kw
    assert call(t=-1) == TOOBIG and call(t=65) == TOOBIG
    # the groups
    for kw in (dict(groups=0), dict(groups=-1), dict(groups=4), dict(groups=5), dict(groups=7), dict(groups=12), dict(lam=-1e-3),
               dict(lam=float("inf")), dict(lam=float("-inf")), dict(lam=float("nan"))):
        assert call(**kw) == BADARG, kw

    def rank(h=fake, stride=18, sc=fake, B=3, beam=6, T=10, alpha=0.7, order=fake, norm=fake, ln=fake):
        return L.cvc_beam_rank(h, stride, sc, B, beam, T, alpha, order, norm, ln, None)

    for kw in (dict(h=None), dict(sc=None), dict(order=None), dict(norm=None), dict(ln=None), dict(B=0), dict(beam=0), dict(beam=9),
               dict(T=0), dict(stride=17), dict(alpha=-0.5), dict(alpha=float("inf")), dict(alpha=float("nan"))):
        assert rank(**kw) == BADARG, kw
    assert rank(T=65) == TOOBIG

    def back(words=fake, parent=fake, att=fake, B=3, beam=6, T=10, N=7, start=fake, stride=1, seq=fake, out=fake):
        return L.cvc_beam_backtrack_from(words, parent, att, B, beam, T, N, start, stride, seq, out, None)

    for kw in (dict(words=None), dict(parent=None), dict(att=None), dict(start=None), dict(seq=None), dict(out=None), dict(B=0),
               dict(beam=0), dict(T=0), dict(T=257), dict(N=0), dict(stride=0)):
        assert back(**kw) == BADARG, kw


# ------------------------------------------------------------------ the engine's and the model's refusals, the docs
def test_engine_refuses_before_anything_is_allocated():
    from cvc.decode import DecodeEngine
    params = inspect.signature(DecodeEngine.__init__).parameters
    assert params["beam_groups"].default == 1 and params["diversity"].default == 0.0 and params["length_penalty"].default == 0.0
    W = types.SimpleNamespace(V=50, R=32, A=32, E=32)
    new = lambda T=4, W=W, **kw: DecodeEngine.__init__(object.__new__(DecodeEngine), W, {}, T, 1, **kw)
    with pytest.raises(RuntimeError, match=r"beam_groups > 1 needs beam_history=True"):
        new(beam=6, beam_groups=2)
    with pytest.raises(RuntimeError, match=r"length_penalty != 0 needs beam_history=True"):
        new(beam=6, length_penalty=0.7)
    with pytest.raises(RuntimeError, match=r"beam_groups > 1.*beam > 1"):
        new(beam_groups=2)
    with pytest.raises(RuntimeError, match=r"length_penalty != 0.*beam > 1"):
        new(length_penalty=0.7)
    with pytest.raises(RuntimeError, match=r"beam_groups = 4 must divide beam = 6"):
        new(beam=6, beam_history=True, beam_groups=4)
    with pytest.raises(RuntimeError, match=r"diversity.*negative"):
        new(beam=6, beam_history=True, beam_groups=2, diversity=-0.5)
    with pytest.raises(RuntimeError, match=r"diversity.*beam_groups > 1"):
        new(beam=6, beam_history=True, diversity=0.5)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(RuntimeError, match="beam_groups must be an integer"):
            new(beam=6, beam_history=True, beam_groups=bad)
    with pytest.raises(RuntimeError, match="length_penalty must be"):
        new(beam=6, beam_history=True, length_penalty=-1.0)
    with pytest.raises(RuntimeError, match="diversity must be"):
        new(beam=6, beam_history=True, beam_groups=2, diversity=float("inf"))
    # gsk / gate_ksplit / lang_ksx, sampling, the forced mode and bf16 weights stay exclusive with beam search
    on = dict(beam=6, beam_history=True, beam_groups=3, diversity=0.5, length_penalty=0.7)
    for kw in (dict(gsk=True), dict(gate_ksplit=True), dict(lang_ksx=True)):
        with pytest.raises(RuntimeError, match="default schedules"):
            new(**on, **kw)
    for kw in (dict(temperature=0.7), dict(forced_n=1), dict(weights_dtype="bf16")):
        with pytest.raises(RuntimeError, match="beam search"):
            new(**on, **kw)
    with pytest.raises(RuntimeError, match="T <= 64"):
        new(T=65, **on)


def test_model_cli_and_docs_know_the_switches():
    from cvc.model import captioner
    from cvc.decode import DecodeEngine
    from cvc import main as cvc_main
    src = inspect.getsource(captioner)
    assert re.search(r"beam_history=beam > 1 and \(any\(cons\.values\(\)\) or groups > 1", src)
    # the engine-cache key is made of every option _sample passes on (the key itself: tests/test_decode_mode_cpu.py)
    call = re.search(r'self\._decode_engine\(\s*"_engine_cache".*?\*\*cons\)', src, re.S).group(0)
    assert "beam_groups=groups, diversity=lam, length_penalty=alpha" in call
    params = inspect.signature(captioner.DecodeAndGroundCaptionerGVDROI._sample).parameters
    assert all(k in params for k in ("beam_groups", "diversity_lambda", "length_penalty"))
    main_src = inspect.getsource(cvc_main)
    assert all(f'"--{k}"' in main_src for k in ("group_size", "diversity_lambda", "length_penalty"))
    from cvc import opts as cvc_opts                           # ... of this entry point, not of the pinned reference option surface
    known = {a.dest for a in cvc_opts.build_parser()._actions}
    assert not known & {"group_size", "diversity_lambda", "length_penalty"}
    doc = DecodeEngine.__init__.__doc__
    assert all(k in doc for k in ("beam_groups", "diversity", "length_penalty", "cvc_beam_rank", "cvc_beam_backtrack_from"))
    assert "ranked" in DecodeEngine.hypotheses.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### Diverse beam search" in design
    sect = design.split("### Diverse beam search")[1]
    assert all(k in sect for k in ("cvc_beam_select_groups_parts", "cvc_beam_rank", "length_penalty", "LDS", "VGPR"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "beam_groups" in readme and "length_penalty" in readme
    assert os.path.exists(os.path.join(ROOT, "profiles", "diverse_beam.md")) and os.path.exists(os.path.join(ROOT, "tools", "bench_beam_diverse.py"))


# ------------------------------------------------------------------ the reference
def _inputs(name, seed):
    d = synth.CONFIGS[name]
    return d, O.to_torch(synth.hot_path_state_dict(d, seed)), O.to_torch(synth.clip_features(d, seed))


@pytest.mark.parametrize("name,seed,beam,rules", [("tiny", 4321, 2, dict(no_repeat_ngram=2)), ("cfg1", 4321, 3, {}),
                                                   ("cfg1", 5, 5, dict(no_repeat_ngram=3))])
def test_with_one_group_the_reference_is_the_constrained_beam_reference(name, seed, beam, rules):
    d, P, f = _inputs(name, seed)
    with torch.no_grad():
        a = BR.decode(P, f, d.T, UNK, beam, **rules)
        b = GR.decode(P, f, d.T, UNK, beam, 1, 0.0, 0.0, **rules)
    assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["score"], b["score"]) and np.array_equal(a["nbanned"], b["nbanned"])
    assert torch.equal(a["parent"], b["parent"]) and torch.equal(a["word"], b["word"])
    np.testing.assert_allclose(a["margin"], b["margin"], rtol=0, atol=0)
    assert np.array_equal(b["order"], np.tile(np.arange(beam), (d.B, 1)))            # alpha = 0: slot order is rank order
    assert np.array_equal(b["norm"], b["score"].numpy()) and np.array_equal(b["len"], GR.lengths(a["seq"].numpy()))


@pytest.mark.parametrize("name,seed,beam,groups,rules", [("tiny", 4321, 6, 3, dict(no_repeat_ngram=2)), ("tiny", 4321, 4, 2, dict(no_repeat_ngram=2)),
                                                          ("cfg1", 4321, 6, 2, dict(no_repeat_ngram=2)), ("cfg1", 4321, 4, 2, dict(no_repeat_ngram=2)),
                                                          ("cfg1", 5, 4, 4, {})])
def test_with_lambda_zero_every_group_is_the_narrower_beam_search(name, seed, beam, groups, rules):
    d, P, f = _inputs(name, seed)
    bd = beam // groups
    with torch.no_grad():
        wide = GR.decode(P, f, d.T, UNK, beam, groups, 0.0, 0.0, **rules)
        narrow = BR.decode(P, f, d.T, UNK, bd, **rules)
    print(name, seed, beam, groups, "narrow margin", narrow["margin"].min())
    assert narrow["margin"].min() >= GR.MARGIN_MIN              # (the GPU test compares engines of these widths exactly)
    for g in range(groups):
        assert torch.equal(wide["seq"][:, g * bd:(g + 1) * bd], narrow["seq"]), g
        # (the oracle's fp32 decoder step on beam rows and on bd rows: other GEMM blocking, not the same bits)
        np.testing.assert_allclose(wide["score"][:, g * bd:(g + 1) * bd].numpy(), narrow["score"].numpy(), rtol=0, atol=5e-5)
        assert torch.equal(wide["parent"][:, :, g * bd:(g + 1) * bd], narrow["parent"] + g * bd)


# measured on this reference: the smallest selection margin, the smallest gap of the final norm order, clips whose best hypothesis
# by norm is not slot 0 -- per case of GR.ENGINE_CASES (the share of distinct hypotheses per clip is 1.0 in every grouped case and
# asserted below)
EXPECT = [(9.79e-4, 2.43e-2, 1), (2.57e-3, 2.50e-3, 3), (2.69e-3, 2.35e-2, 0), (5.11e-4, 2.85e-3, 3), (1.63e-3, 3.12e-3, 4),
          (5.60e-4, 1.22e-2, 3), (1.63e-3, 3.58e-2, 4), (2.60e-4, 5.88e-3, 3)]


@pytest.mark.parametrize("i", range(len(GR.ENGINE_CASES)))
def test_the_margins_allow_an_exact_comparison(i):
    name, seed, beam, groups, lam, alpha, eos, rules = GR.ENGINE_CASES[i]
    d, P, f, r = GR.shared_decode(i)
    sel, rk, moved = EXPECT[i]
    print(GR.ENGINE_CASES[i], "selection margin", r["margin"].min(), "rank margin", r["rank_margin"], "best != slot 0",
          int((r["order"][:, 0] != 0).sum()), "len", r["len"].min(), r["len"].max())
    assert r["margin"].min() > GR.MARGIN_MIN and r["rank_margin"] > GR.MARGIN_MIN
    assert abs(r["margin"].min() - sel) <= 0.05 * sel + 1e-5 and abs(r["rank_margin"] - rk) <= 0.05 * rk + 1e-5      # the table's figures
    assert int((r["order"][:, 0] != 0).sum()) == moved
    assert bool(torch.isfinite(r["score"]).all())
    # every parent lies in its own group; the histories are the parents walked back
    bd = beam // groups
    assert torch.equal(r["parent"] // bd, (torch.arange(beam) // bd).expand(d.T, d.B, beam))
    assert torch.equal(BR.backtrack_all(r["word"], r["parent"]), r["seq"])
    seq = r["seq"].view(-1, d.T).tolist()
    n = rules.get("no_repeat_ngram", 0)
    for h in seq:
        assert UNK not in h and (n == 0 or not BR.repeats_ngram(BR.cut(h), n)) and 0 not in h[:rules.get("min_len", 0)]
    if eos > 0:                                                # the length penalty has lengths to rank
        assert r["len"].min() < r["len"].max()
    if groups > 1:                                             # what the groups are for: the clip's hypotheses differ
        assert np.mean([len({tuple(h) for h in r["seq"][b].tolist()}) / beam for b in range(d.B)]) == 1.0


@pytest.mark.parametrize("si,beam,groups", GC.BLOCK_CASES)
def test_the_block_cases_augmented_values_are_tied_or_a_gap_apart(si, beam, groups):
    rules, hist = GC.rules_of(si), GC.planted_history(si, beam)
    penalised = False
    for t in GC.STEPS:
        c = GC.base_case(si, beam, t == 0)
        for lam in (0.0, GC.LAMBDA):
            r = GC.block_ref(c, t, hist, rules, groups, lam)
            assert not GR.aug_gap_violations(r, T.GAP), (si, beam, groups, t, lam, GR.aug_gap_violations(r, T.GAP)[:3])
        free = GC.block_ref(c, t, hist, rules, groups, 0.0)
        penalised |= not (torch.equal(free["parent"], r["parent"]) and torch.equal(free["word"], r["word"]))
        assert bool((c["done"].float().mean() > 0.2)) == (t != 0)
        if GC.SHAPES[si][0] == 8 and t == 0 and beam // groups > 2:  # two allowed words on one live row per group: fillers
            assert not bool(r["live"].all())
    # the penalty decides some selection of the case (V = 8: two allowed words per row, it has little to choose from)
    assert penalised == (groups > 1) or (GC.SHAPES[si][0] == 8 and not penalised)


def test_the_rounding_case_is_decided_by_the_separately_rounded_product():
    """fp32 arithmetic of the case, operation by operation (numpy rounds each): the rule's value of the penalised word ties with the
    other word exactly, a fused multiply-add would put it strictly above -- and the fp64 reference sees the same exact tie"""
    c, t, hist, lam, P, Q = GC.rounding_case()
    f = np.float32
    p3 = f(f(lam) * f(3))
    assert float(p3) > float(f(lam)) * 3 and float(p3) >= 200.0                       # the product rounds up
    rule = f(f(200) - p3)                                                             # one rounded multiply, one rounded subtract
    fused = f(200.0 - float(f(lam)) * 3)                                              # the exact product, one rounding
    assert float(f(200) - p3) == 200.0 - float(p3)                                    # (the subtraction itself is exact)
    assert f(f(200) + f(-float(p3))) == rule and fused > rule and Q < P
    r = GR.step(c["logits"], c["score"], c["done"], hist.T, t, c["B"], c["beam"], c["unk"], c["beam"], lam)
    assert bool(r["live"].all())
    assert r["word"].tolist() == [[P, P, P, Q]] * c["B"] and r["parent"].tolist() == [[0, 1, 2, 3]] * c["B"]
    assert r["aug"][:, 3].tolist() == [float(rule)] * c["B"] and r["score"][:, 3].tolist() == [float(rule)] * c["B"]
    aug3 = r["augmented"][3].view(c["B"], c["V"])
    assert bool((aug3[:, P] == aug3[:, Q]).all())                                     # the exact tie, in fp64 too
