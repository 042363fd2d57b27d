"""Stochastic beam search without a GPU: the fp64 restatement tests/sbs_ref.py reproduces the sampling-without-replacement
statistics on the toy (history-dependent logits, word 0 ends a caption), yields no NaN on frozen / all-banned / -inf rows; the block
is in the library's table with the header's argument count and its host checks return their codes before any launch; every refusal
of the engine, the trainer and the command line raises with its message; the new flags parse and their defaults change nothing."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

from cvc import synth
import sbs_ref as S
import sample_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cvc_beam_select_stoch_parts"
BADARG, TOOBIG = -1, -2
TRIALS = 50000


# ------------------------------------------------------------------ the statistics of the rule, in fp64
@pytest.mark.parametrize("V,unk", [(4, -1), (5, 3)])
@pytest.mark.parametrize("tau", [1.0, 0.7])
def test_the_toy_is_a_sample_without_replacement(tau, V, unk):
    """T = 3, beam 3, 50 000 trials, fixed seeds: slot 0 against p(a) and the ordered pair (slot 0, slot 1) against
    p(a) p(b) / (1 - p(a)) under q_tau, per step renormalised over the words other than UNK; chi-square at p = 1e-4"""
    table = S.toy_table(V, 3, 11)
    hist, live, G, logq, score = S.toy_run(table, TRIALS, 3, tau, seed=5, unk=unk)
    seqs, probs = S.toy_sequences(table, tau, unk)
    assert len(seqs) == 40 and abs(probs.sum() - 1.0) < 1e-12 and live.all() and not (hist == unk).any()
    (c1, d1), (c2, d2) = S.toy_chi_squares(hist, seqs, probs)
    assert c1 < SO.chi_square_critical(d1), (c1, d1)
    assert c2 < SO.chi_square_critical(d2), (c2, d2)
    # draw order, distinct captions, and logq is the caption's log-prob under q_tau
    assert (G[:, 1:] <= G[:, :-1]).all()
    assert (hist[:, 0] != hist[:, 1]).any(1).all() and (hist[:, 0] != hist[:, 2]).any(1).all() and (hist[:, 1] != hist[:, 2]).any(1).all()
    index = {s: i for i, s in enumerate(seqs)}
    first = np.array([index[tuple(int(w) for w in h)] for h in hist[:200, 0]])
    assert np.allclose(logq[:200, 0], np.log(probs[first]), atol=1e-9)


def test_a_wrong_normaliser_fails_the_check():
    """the check has teeth: slot 0 held against the distribution with UNK's mass left in (the full-row normaliser) is rejected"""
    table = S.toy_table(5, 3, 11)
    hist, *_ = S.toy_run(table, TRIALS, 3, 1.0, seed=5, unk=3)
    seqs, probs = S.toy_sequences(table, 1.0, 3)
    wrong = np.array([np.prod([np.exp(table[t][(s[t - 1] + 1) if t else 0][w] - S._lse(table[t][(s[t - 1] + 1) if t else 0], 0))
                               for t, w in enumerate(s) if not (t and s[t - 1] == 0)]) for s in seqs])
    index = {s: i for i, s in enumerate(seqs)}
    counts = np.bincount([index[tuple(int(w) for w in h)] for h in hist[:, 0]], minlength=len(seqs))
    stat, df = SO.chi_square(counts, wrong / wrong.sum())
    assert stat > SO.chi_square_critical(df)


def test_frozen_all_banned_and_minus_inf_rows_yield_no_nan():
    B, beam, V, t = 2, 4, 9, 2
    rows = B * beam
    rng = np.random.default_rng(3)
    z = rng.normal(0, 3, (rows, V))
    score, logq = -rng.random(rows) * 5, -rng.random(rows) * 5
    G = logq + 0.3
    done = np.zeros(rows, dtype=bool)
    done[[0, 5]] = True                                          # frozen rows, with keys above every live row's: they are selected
    G[[0, 5]] = 5.0
    G[[1, 6]], logq[[1, 6]], score[[1, 6]] = -np.inf, -np.inf, -np.inf      # rows at -inf
    ban = np.zeros((rows, V), dtype=bool)
    ban[:, 1] = True
    ban[[2, 7]] = True                                           # every word banned
    hist = rng.integers(2, V, (rows, t))
    r = S.step(z, score, logq, G, done, hist, t, B, beam, 1, 0.8, S.noise(1, 1, t, rows, V), ban=ban)
    for k in ("score", "logq", "G", "sorted", "margin"):
        assert not np.isnan(r[k]).any(), k
    assert r["live"].all()                                       # one live row per clip offers V - 1 >= beam words
    assert not np.isin(r["parent"][0], [1, 2]).any() and not np.isin(r["parent"][1], [2, 3]).any()      # the -inf rows and the all-banned rows are nobody's parent
    fr = r["parent"] == np.array([[0], [1]])                     # children of the frozen rows: word 0, everything carried
    assert fr.sum() == 2 and (r["word"][fr] == 0).all()
    assert np.array_equal(r["G"][fr], G[[0, 5]]) and np.array_equal(r["logq"][fr], logq[[0, 5]]) and np.array_equal(r["score"][fr], score[[0, 5]])
    # a clip with nothing live: fillers at -inf, still no NaN
    r2 = S.step(z, score, logq, np.full(rows, -np.inf), done, hist, t, B, beam, 1, 0.8, S.noise(1, 1, t, rows, V), ban=ban)
    assert not r2["live"].any() and all(not np.isnan(r2[k]).any() for k in ("score", "logq", "G"))
    # the conditioning itself: the arg-max child keeps the parent's key, children lie below it, -inf stays -inf
    g = np.array([-1.0, -3.0, -np.inf, -1.0 - 1e-12])
    out = S.condition(-0.5, -1.0, g)
    assert out[0] == -0.5 and out[1] < -0.5 and out[2] == -np.inf and out[3] < -0.5 and not np.isnan(out).any()
    want = -np.log(np.exp(0.5) - np.exp(1.0) + np.exp(3.0))
    assert abs(out[1] - want) < 1e-12


# ------------------------------------------------------------------ the block: table, binding, argument checks
def test_the_block_is_in_the_table_and_bound_with_the_headers_argument_count():
    import subprocess
    import build_hip
    from cvc import hip
    so = build_hip.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "cvc_hip_blocks.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m
    nargs = len([a for a in m.group(1).split(",") if a.strip()])
    assert NAME in hip.BLOCKS and len(hip.SIGNATURES[NAME]) == nargs == len(hip.SIGNATURES["cvc_beam_select_hist_parts"]) + 6
    lib = ctypes.CDLL(so)
    lib.cvc_block.restype = ctypes.c_void_p
    lib.cvc_block.argtypes = [ctypes.c_char_p]
    assert lib.cvc_block(NAME.encode())
    exported = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert not re.search(r"\b" + NAME + r"\b", exported)          # the exported ABI does not grow
    assert f"CVC_B({NAME})" in open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "blocks.hip")).read()
    beam = open(os.path.join(ROOT, "cyclical-visual-captioning_amd", "csrc", "beam.hip")).read()
    for text in (header, beam):
        assert "26 * B * beam floats" in text and "CVC_SBS_SITE" in text and "candidates ONLY" in text
    site = int(re.search(r"#define CVC_SBS_SITE (0x[0-9A-Fa-f]+)u", header).group(1), 16)
    assert site == S.SBS_SITE
    others = [int(re.search(r"#define " + k + r" (0x[0-9A-Fa-f]+)u", header).group(1), 16) for k in ("CVC_SAMPLE_SITE", "CVC_MIX_SITE")]
    assert all(abs(site - o) > 64 for o in others) and site > 0x200 + 256          # the dropout sites end below 0x300


def test_host_argument_checks_return_their_codes_and_launch_nothing():
    from cvc import hip
    L = hip.lib()
    fake, fake2, fake3, fake4 = (ctypes.c_void_p(v) for v in (16, 4096, 8192, 12288))

    def call(parts=fake, nparts=1, score=fake, done=fake, B=3, beam=5, V=50, t=0, hin=fake, hout=fake2, hstride=15, n=0, inv_tau=1.0,
             state=fake, logq=fake, G=fake3, parent=fake, word=fake, score_out=fake2, done_out=fake, logq_out=fake2, G_out=fake4, ws=fake):
        c = hip.Constraint(n, 0, 0, 0, None, None, 0)
        return L.cvc_beam_select_stoch_parts(parts, nparts, 0, None, score, done, B, beam, V, 1, t, hin, hout, hstride, c, inv_tau, state,
                                             logq, G, parent, word, score_out, done_out, logq_out, G_out, None, ws, None)

    # the history block's checks
    for kw in (dict(parts=None), dict(score=None), dict(done=None), dict(parent=None), dict(word=None), dict(score_out=None),
               dict(done_out=None), dict(ws=None), dict(nparts=0), dict(B=0), dict(beam=0), dict(beam=9), dict(V=5), dict(V=8193),
               dict(t=3, hin=None), dict(hout=None), dict(hin=fake, hout=fake), dict(hstride=14), dict(n=-1), dict(n=65)):
        assert call(**kw) == BADARG, kw
    assert call(t=-1) == TOOBIG and call(t=65) == TOOBIG
    # its own
    for kw in (dict(inv_tau=0.0), dict(inv_tau=-2.0), dict(inv_tau=float("inf")), dict(inv_tau=float("nan")), dict(state=None),
               dict(logq=None), dict(G=None), dict(logq_out=None), dict(G_out=None), dict(logq=fake2, logq_out=fake2),
               dict(G=fake4, G_out=fake4), dict(score=fake2, score_out=fake2)):
        assert call(**kw) == BADARG, kw


# ------------------------------------------------------------------ refusals, flags, docs
def test_engine_refuses_before_anything_is_allocated():
    from cvc.decode import DecodeEngine
    params = inspect.signature(DecodeEngine.__init__).parameters
    assert params["stochastic"].default is False and params["stochastic_tau"].default == 1.0
    W = types.SimpleNamespace(V=50, R=32, A=32, E=32)
    new = lambda T=4, **kw: DecodeEngine.__init__(object.__new__(DecodeEngine), W, {}, T, 1, **kw)
    on = dict(beam=4, beam_history=True, stochastic=True)
    head = r"stochastic beam search \(stochastic=True\) is refused: "
    for kw in (dict(stochastic=True), dict(beam=4, stochastic=True), dict(beam_history=True, stochastic=True)):
        with pytest.raises(RuntimeError, match=(head + "it is a beam search.*beam > 1 and beam_history=True") if kw.get("beam") or not kw.get("beam_history")
                           else "beam_history.*needs beam > 1"):
            new(**kw)
    with pytest.raises(RuntimeError, match=head + "beam_groups > 1 / diversity"):
        new(**on, beam_groups=2)
    with pytest.raises(RuntimeError, match=head + "beam_groups > 1 / diversity"):
        new(**on, beam_groups=2, diversity=0.5)
    with pytest.raises(RuntimeError, match=head + "length_penalty"):
        new(**on, length_penalty=0.7)
    with pytest.raises(RuntimeError, match=head + "force_n"):
        new(**on, force_n=1)
    with pytest.raises(RuntimeError, match=head + "it takes no sampling temperature"):
        new(**on, temperature=0.7)
    for kw in (dict(gsk=True), dict(gate_ksplit=True), dict(lang_ksx=True)):
        with pytest.raises(RuntimeError, match="default schedules"):
            new(**on, **kw)
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match=head + "stochastic_tau must be a positive finite number"):
            new(**on, stochastic_tau=tau)
    with pytest.raises(RuntimeError, match="stochastic must be a bool"):
        new(beam=4, beam_history=True, stochastic=1)
    # the refusal the existing tests pin stays: a temperature with beam > 1 and no switch
    with pytest.raises(RuntimeError, match="sampling \\(temperature\\) and beam search \\(beam > 1\\) exclude each other"):
        new(beam=4, beam_history=True, temperature=0.7)


def test_trainer_and_cli_refusals():
    from cvc import sample as cvc_sample
    from cvc.trainer import Trainer
    t = object.__new__(Trainer)
    t.model = types.SimpleNamespace(eval=lambda: None)
    t.opts, t.dataset = None, None
    t._segment_timestamps = lambda: {}
    with pytest.raises(RuntimeError, match="without_replacement is refused with top_k / top_p"):
        t.sample(3, 1.0, without_replacement=True, top_k=4)
    with pytest.raises(RuntimeError, match="without_replacement is refused with top_k / top_p"):
        t.sample(3, 1.0, without_replacement=True, top_p=0.9)
    with pytest.raises(RuntimeError, match="without_replacement draws n > 1"):
        t.sample(1, 1.0, without_replacement=True)
    for flags, msg in ((["--without_replacement", "--sample_n", "5", "--top_k", "3"], "refused with --top_k / --top_p"),
                       (["--without_replacement", "--sample_n", "5", "--top_p", "0.5"], "refused with --top_k / --top_p"),
                       (["--without_replacement", "--sample_n", "1"], "needs --sample_n > 1")):
        with pytest.raises(SystemExit, match=msg):
            cvc_sample.parse(flags)
    own, rest = cvc_sample.parse(["--sample_n", "5", "--without_replacement", "--temperature", "0.7", "--id", "x"])
    assert own.without_replacement and own.temperature == 0.7 and rest == ["--id", "x"]
    assert cvc_sample.parse(["--id", "x"])[0].without_replacement is False


def test_the_flags_parse_and_their_defaults_leave_opt_as_it_was():
    from cvc import main as cvc_main
    from cvc import opts as cvc_opts
    p = cvc_main.build_parser()
    base = vars(p.parse_args([]))
    assert (base["stochastic_beam"], base["stochastic_tau"], base["sample_seed"]) == (False, 1.0, 0)
    on = vars(p.parse_args(["--beam_size", "5", "--stochastic_beam", "--stochastic_tau", "0.7", "--sample_seed", "3", "--consensus", "beam"]))
    assert (on["stochastic_beam"], on["stochastic_tau"], on["sample_seed"], on["beam_size"], on["consensus"]) == (True, 0.7, 3, 5, "beam")
    new = {"stochastic_beam", "stochastic_tau", "sample_seed"}
    assert {k: v for k, v in on.items() if k not in new | {"beam_size", "consensus"}} == {k: v for k, v in base.items()
                                                                                          if k not in new | {"beam_size", "consensus"}}
    # flags of cvc.main, not of the reference's option surface
    assert not {a.dest for a in cvc_opts.build_parser()._actions} & new
    # the model's defaults: no opts attribute -> off
    from cvc.model import captioner
    src = inspect.getsource(captioner)
    assert 'bool(getattr(opts, "stochastic_beam", False))' in src and 'float(getattr(opts, "stochastic_tau", 1.0))' in src
    sig = inspect.signature(captioner.DecodeAndGroundCaptionerGVDROI._sample).parameters
    assert sig["stochastic_beam"].default is None and sig["stochastic_tau"].default is None


def test_docs_and_tooling_know_the_feature():
    from cvc.decode import DecodeEngine
    doc = DecodeEngine.__init__.__doc__
    assert all(k in doc for k in ("stochastic_tau", NAME, "WITHOUT", "draw order"))
    assert "G" in DecodeEngine.hypotheses.__doc__ and "logq" in DecodeEngine.hypotheses.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### Stochastic beam search" in design
    sect = design.split("### Stochastic beam search")[1]
    assert all(k in sect for k in (NAME, "candidate-only", "Out of scope", "VGPR", "lseq"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "--stochastic_beam" in readme and "--without_replacement" in readme
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_beam_stochastic.py"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "beam_stochastic.md"))
