"""Constrained beam search on the GPU (pytest -m gpu): the selection block cvc_beam_select_hist_parts (csrc/beam.hip, the HIST forms
of the beam row scan and merge) against the fp64 reference (tests/beam_constrain_ref.py) on every clip, the block with nothing banned
against the plain beam blocks bit for bit, the engine with beam_history=True against the plain beam engine, its n-best against host
backtracking, the constrained engine against the reference decoder on tile and ring, graph replay, and the model / CLI plumbing.

The block cases are the integer-logit cases of tests/tile_path_cases.py::beam_case (candidates of different rows at least 0.11
apart, ties inside a row exact): parent, word, done and the histories are compared exactly, the scores at its SCORE_TOL."""
import functools

import numpy as np
import pytest
import torch

from cvc import synth
import tile_path_cases as T
from tile_path_cases import SCORE_TOL, close, nan_buf, same_bits
import beam_constrain_ref as BR
import test_gpu_tile_path as TP               # the plain blocks' launcher and its sentinels
import test_gpu_sampling as TS                # the engine inputs

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
BADARG, TOOBIG = -1, -2
T_HIST = 65                                   # steps a history buffer holds: t <= 64 writes step t
bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def hist_run(c, dev, t, hist, rules, null_desc=False, with_nbanned=True, hist_pad=0, same_buffers=False, t_arg=None, null_out=False, stride_arg=None):
    """cvc_beam_select_hist_parts on a tile_path_cases beam case.  hist [T_HIST, rows] int64 (host).  Every output is pre-filled
    with a value no launch writes.  -> rc, parent, word, score, done, hist_out [T_HIST, rows], nbanned"""
    from cvc import hip
    L = hip.lib()
    rows, V, nparts, stride = c["B"] * c["beam"], c["V"], c["nparts"], c["part_stride"]
    buf = nan_buf(nparts * stride + 8, dev=dev)
    for p in range(nparts):
        buf[p * stride:p * stride + rows * V] = c["parts"][p].reshape(-1).to(dev)
    bias = None
    if c["bias_v"] is not None:
        bo = 1 if c["bias_shift"] else 0
        bias = nan_buf(V + 4, dev=dev)
        bias[bo:bo + V] = c["bias_v"].to(dev)
        bias = bias[bo:bo + V]
    score, done = c["score"].to(dev), c["done"].to(dev)
    parent = torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev)
    word = torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev)
    score_out = nan_buf(rows, dev=dev)
    done_out = torch.full((rows,), TP.DONE_FILL, dtype=torch.uint8, device=dev)
    nb = torch.full((rows,), TP.SENT, dtype=torch.int32, device=dev)
    ws = nan_buf(17 * rows, dev=dev)
    hs = rows + hist_pad
    hin = torch.full((T_HIST, hs), TP.SENT, dtype=torch.int64, device=dev)
    hin[:, :rows] = torch.from_numpy(np.ascontiguousarray(hist)).to(dev)
    hout = torch.full((T_HIST, hs), TP.SENT, dtype=torch.int64, device=dev)
    i32 = lambda ids: torch.tensor(list(ids) or [0], dtype=torch.int32, device=dev)
    ban, bad = list(rules.get("ban_words", ())), list(rules.get("bad_endings", ()))
    ban_d, bad_d = i32(ban), i32(bad)
    desc = None if null_desc else hip.Constraint(int(rules.get("no_repeat_ngram", 0)), int(bool(rules.get("no_immediate_repeat", False))),
                                                 int(rules.get("min_len", 0)), len(ban), ban_d.data_ptr(), bad_d.data_ptr(), len(bad))
    rc = L.cvc_beam_select_hist_parts(buf.data_ptr(), nparts, stride, TP.P(bias), score.data_ptr(), done.data_ptr(), c["B"], c["beam"], V,
                                      c["unk"], t if t_arg is None else t_arg, hin.data_ptr(),
                                      None if null_out else (hin if same_buffers else hout).data_ptr(), hs if stride_arg is None else stride_arg, desc, parent.data_ptr(),
                                      word.data_ptr(), score_out.data_ptr(), done_out.data_ptr(), nb.data_ptr() if with_nbanned else None,
                                      ws.data_ptr(), TP.st())
    torch.cuda.synchronize()
    return rc, parent, word, score_out, done_out, hout[:, :rows], nb, hout, hin


def untouched(out, rows):
    rc, parent, word, score, done, hist_out, nb, hout, hin = out
    return (bool((parent == TP.SENT).all()) and bool((word == TP.SENT).all()) and bool(torch.isnan(score).all()) and
            bool((done == TP.DONE_FILL).all()) and bool((hout == TP.SENT).all()) and bool((nb == TP.SENT).all()))


# ------------------------------------------------------------------ 1. the block against the reference, every clip
# (B, beam, V, nparts, bias, planted columns): float4 scan; the engine's shape; V = 8192; the general scan; a small one; V = 8 with
# five words banned (a row has fewer finite candidates than beam)
SHAPES = [(3, 5, 2052, 1, False, (0, 30, 700, 2051)), (64, 5, 5000, 6, True, (0, 1666, 4999)), (1, 8, 8192, 8, True, (0, 5000, 8191)),
          (3, 5, 1025, 5, True, (0, 341, 1024)), (2, 3, 50, 3, True, (0, 16, 49)), (3, 5, 8, 1, False, (6,))]
MODES = ["n1", "n2", "n3", "immediate", "min_len", "lists", "all"]


@functools.lru_cache(maxsize=None)
def base_case(si, first):
    """the beam case of a shape (first step or not: frozen rows 0.4), shared by its modes and never modified"""
    B, beam, V, nparts, bias, plant = SHAPES[si]
    return T.beam_case(f"hist{si}", B, beam, V, 700 + si, plant=plant, first=first, nparts=nparts, bias=bias, frozen=0.0 if first else 0.4)


@functools.lru_cache(maxsize=None)
def planted_history(si):
    """[T_HIST, rows]: every row a random walk over a small pool of words, two thirds of them the planted maxima, so that n-grams
    repeat and the rules ban a planted maximum in part of the rows"""
    B, beam, V, nparts, bias, plant = SHAPES[si]
    g = T.gen(900 + si)
    pool = list(plant) * 2 + [2, 3, V - 1]
    idx = torch.randint(0, len(pool), (T_HIST, B * beam), generator=g)
    h = torch.tensor(pool, dtype=torch.int64)[idx].numpy()
    h[:3, 1::2] = np.array([2, 3, 2]).reshape(3, 1)             # odd rows start on plain words: nothing planted is banned early
    return h


def rules_of(mode, si):
    B, beam, V, nparts, bias, plant = SHAPES[si]
    r = {}
    if mode in ("n1", "n2", "n3"):
        r["no_repeat_ngram"] = int(mode[1])
    if mode in ("immediate", "all"):
        r["no_immediate_repeat"] = True
    if mode in ("min_len", "all"):
        r["min_len"] = 70
    if mode in ("lists", "all"):
        r["ban_words"] = [plant[-1], 2, V + 5, UNK]             # a planted maximum, a plain word, an id outside [0, V), UNK again
        r["bad_endings"] = [plant[-1], 3]
    if mode == "all":
        r["no_repeat_ngram"] = 2
    if V == 8:                                                  # five words banned: two candidates per row are left
        r["ban_words"] = sorted(set(r.get("ban_words", [])) | {0, 2, 3, 4, 5})
    return r


def check_block(label, c, out, t, hist, rules, dev):
    rc, parent, word, score, done, hist_out, nb, hout, hin = out
    B, beam, V = c["B"], c["beam"], c["V"]
    rows = B * beam
    assert rc == 0, (label, rc)
    r = BR.step(c["logits"], c["score"], c["done"], hist.T, t, B, beam, c["unk"], **rules)
    parent, word, score, done = parent.view(B, beam).cpu(), word.view(B, beam).cpu(), score.view(B, beam).cpu(), done.view(B, beam).cpu()
    assert bool(((parent >= 0) & (parent < beam) & (word >= 0) & (word < V)).all()), f"{label}: parent / word out of range"
    live = r["live"]
    assert torch.equal(parent[live], r["parent"][live]), f"{label}: parent"
    assert torch.equal(word[live], r["word"][live]), f"{label}: word"
    assert torch.equal(done[live].bool(), r["done"][live]) and bool((done <= 1).all()), f"{label}: done"
    close(score[live], r["score"][live].float(), **SCORE_TOL)
    assert bool((score[~live] == -float("inf")).all()), f"{label}: a filler is not -inf"
    assert np.array_equal(nb.cpu().numpy(), r["nbanned"]), (label, nb[:8], r["nbanned"][:8])
    # the histories: the parent's steps gathered, the word appended -- every slot follows the launch's own parent and word, and on
    # the live slots those are the reference's
    ho = hist_out.cpu().numpy()
    src = (parent + torch.arange(B).view(-1, 1) * beam).view(-1).numpy()
    assert np.array_equal(ho[:t], hist[:t][:, src]), f"{label}: gathered history"
    assert np.array_equal(ho[t], word.view(-1).numpy()), f"{label}: appended word"
    assert (ho[t + 1:] == TP.SENT).all() and bool((hout[:, rows:] == TP.SENT).all()), f"{label}: wrote past step t"
    lv = live.view(-1).numpy()
    assert np.array_equal(ho[:t + 1][:, lv], r["hist"].T[:, lv]), f"{label}: history against the reference"
    assert np.array_equal(hin[:, :rows].cpu().numpy(), hist), f"{label}: hist_in changed"
    return r


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_block_vs_reference_on_every_clip(dev, si, mode):
    B, beam, V, nparts, bias, plant = SHAPES[si]
    rules = rules_of(mode, si)
    n = rules.get("no_repeat_ngram", 2)
    hist = planted_history(si)
    hit_some = some_banned = some_free = False
    for t in sorted({0, 1, n - 1, n, 63, 64}):
        c = base_case(si, t == 0)
        if mode == "n1" and t in (0, 1):
            assert not T.gap_violations(c)                      # (every mode removes candidates of these two cases, and adds none)
        label = f"shape {SHAPES[si][:4]} {mode} t={t}"
        first = hist_run(c, dev, t, hist, rules, hist_pad=3 if si == 4 else 0)
        r = check_block(label, c, first, t, hist, rules, dev)
        again = hist_run(c, dev, t, hist, rules, hist_pad=3 if si == 4 else 0)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first[1:7], again[1:7])), f"{label}: two launches differ"
        # what the ban decided: the selection with UNK alone banned is another one in some clips
        free = BR.step(c["logits"], c["score"], c["done"], hist.T, t, B, beam, c["unk"])
        hit_some |= not (torch.equal(free["parent"], r["parent"]) and torch.equal(free["word"], r["word"]))
        if V == 8 and t == 0:
            assert 1 <= int(r["live"].sum()) <= 2 * B           # first step, at most two allowed words: three or more fillers per clip
        if t >= max(n, 1):                                      # a planted maximum is banned in some live rows, in others none is
            from constrain_ref import banned
            b_ = banned(hist.T, t, V, c["unk"], **rules)[:, list(plant)].any(1)[~c["done"].bool().numpy()]
            some_banned |= bool(b_.any())
            some_free |= bool((~b_).any())
    assert hit_some or B < 64, f"shape {SHAPES[si][:4]} {mode}: the ban never changed a selection"      # (64 clips: some clip's best row is hit)
    assert (some_banned or (mode == "min_len" and 0 not in plant)) and (some_free or mode in ("min_len", "lists", "all") or V == 8), f"shape {SHAPES[si][:4]} {mode}: planted maxima"


def test_refusals_leave_the_outputs_untouched(dev):
    c = base_case(4, False)
    hist = planted_history(4)
    rows = c["B"] * c["beam"]
    for kw, code in ((dict(t_arg=65), TOOBIG), (dict(t_arg=-1), TOOBIG), (dict(same_buffers=True), BADARG), (dict(null_out=True), BADARG),
                     (dict(stride_arg=rows - 1), BADARG)):
        out = hist_run(c, dev, 3, hist, {}, **kw)
        assert out[0] == code and untouched(out, rows), kw
    for rules in (dict(no_repeat_ngram=65), dict(no_repeat_ngram=-1), dict(min_len=-1), dict(ban_words=list(range(257))),
                  dict(bad_endings=list(range(257)))):
        out = hist_run(c, dev, 3, hist, rules)
        assert out[0] == BADARG and untouched(out, rows), rules


# ------------------------------------------------------------------ 2. nothing banned is the plain block
@pytest.mark.parametrize("name", ["frozen_mix", "tie_many", "general_V1025_np5", "fast_V5000_np6", "first_step", "neg_inf"])
def test_with_nothing_banned_the_block_is_the_plain_block(dev, name):
    """c = NULL, and rules that never fire: parent, word, score and done with the bits of cvc_beam_select / cvc_beam_select_parts on
    the same inputs -- a float4-scan case, a general-scan case, a slab case, the first step, fewer finite candidates than beam"""
    from cvc import hip
    c = T.shared_beam_case(name)
    plain = TP.beam_run(hip.lib(), c, dev)
    torch.cuda.synchronize()
    assert plain[0] == 0
    rows = c["B"] * c["beam"]
    g = T.gen(41)
    hist = torch.randint(0, c["V"], (T_HIST, rows), generator=g).numpy()
    hist[:, ::2] = np.arange(T_HIST).reshape(-1, 1) % c["V"] + 2                          # (rows without a repeated word among the last 5)
    t = 0 if c["first"] else 5
    never = dict(no_repeat_ngram=64, ban_words=[c["V"] + 3, c["unk"]], bad_endings=[c["V"] + 1])
    for what, kw in (("NULL descriptor", dict(null_desc=True)), ("rules that never fire", dict(rules=never)),
                     ("no nbanned output", dict(null_desc=True, with_nbanned=False))):
        rules = kw.pop("rules", {})
        out = hist_run(c, dev, t, hist, rules, **kw)
        assert out[0] == 0
        for a, b, nm in zip(plain[1:], out[1:5], ("parent", "word", "score", "done")):
            assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b), f"{name}, {what}: {nm} differs from the plain block"
        assert bool((out[6] == (1 if kw.get("with_nbanned", True) else TP.SENT)).all())
        src = (out[1].view(c["B"], c["beam"]).cpu() + torch.arange(c["B"]).view(-1, 1) * c["beam"]).view(-1).numpy()
        ho = out[5].cpu().numpy()
        assert np.array_equal(ho[:t], hist[:t][:, src]) and np.array_equal(ho[t], out[2].cpu().numpy())


# ------------------------------------------------------------------ 3. the engine
def _engine(dev, name, seed, beam, path, **kw):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs(name, seed=seed)
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, beam=beam, path=path, **kw)
    assert eng.tile == (path == "tile") and not eng.packed
    return d, eng


def _grab(eng):
    seq, att, score = eng.run()
    return dict(seq=seq.clone(), att=att.clone(), score=score.clone(), words=eng.words.clone(), parent=eng.parent.clone(),
                done=eng.done.clone())


def _same(a, b, what):
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("name,beam,path", [("tiny", 2, "ring"), ("tiny", 3, "tile"), ("cfg1", 5, "tile"), ("cfg1", 3, "ring")])
def test_beam_history_alone_is_the_plain_beam_engine_and_gives_the_n_best(dev, name, beam, path):
    from cvc import hip
    d, plain = _engine(dev, name, 4321, beam, path, driver=False)
    assert plain._plan is None and not plain.beam_hist
    d, eng = _engine(dev, name, 4321, beam, path, beam_history=True)
    assert eng.beam_hist and eng._plan is None and not eng.constrained and not eng.given
    assert eng.bhist.shape == (2, d.T, d.B * beam) and eng.bhist.dtype == torch.int64
    sel = [fn for nm, fn, _ in eng._python_launches() if nm == "word_select"]
    assert len(sel) == d.T and all(fn is hip.lib().cvc_beam_select_hist_parts for fn in sel)
    a, b = _grab(plain), _grab(eng)
    _same(a, b, f"{name} beam {beam} {path}")
    seq, score = eng.hypotheses()
    assert seq.shape == (d.B, beam, d.T) and score.shape == (d.B, beam)
    host = BR.backtrack_all(eng.words[1:].view(d.T, d.B, beam).cpu(), eng.parent.view(d.T, d.B, beam).cpu())
    assert torch.equal(seq.cpu(), host)
    assert torch.equal(seq[:, 0], b["seq"]) and torch.equal(bits(score), bits(b["score"]))
    assert torch.equal(eng._backtrack_host()[0], b["seq"])
    with pytest.raises(RuntimeError, match="beam_history"):
        plain.hypotheses()


@pytest.mark.parametrize("path", ["tile", "ring"])
@pytest.mark.parametrize("i", range(len(BR.ENGINE_CASES)))
def test_constrained_engine_vs_reference_decoder(dev, i, path):
    name, seed, beam, rules = BR.ENGINE_CASES[i]
    d, P, f, ref = BR.shared_decode(i)
    assert ref["fired"].any(1).all() and ref["margin"].min() >= BR.MARGIN_MIN and bool(torch.isfinite(ref["score"]).all())
    d, eng = _engine(dev, name, seed, beam, path, beam_history=True, **rules)
    assert eng.constrained and eng.beam_hist and eng._plan is None and eng.nbanned.shape == (d.T, d.B * beam)
    seq0, att0, score0 = eng.run()
    seq, score = eng.hypotheses()
    err = float((score.cpu().double() - ref["score"]).abs().max())
    print(f"constrained beam {name} seed {seed} beam {beam} {rules} {path}: max |score - ref| = {err:.3e}, smallest margin "
          f"{ref['margin'].min():.3e}, fired steps {int(ref['fired'].sum())}")
    assert torch.equal(seq.cpu(), ref["seq"])                                    # all hypotheses, exact
    assert np.array_equal(eng.nbanned.cpu().numpy(), ref["nbanned"])
    np.testing.assert_allclose(score.cpu().double().numpy(), ref["score"].numpy(), rtol=0, atol=2e-4)
    assert torch.equal(seq0, seq[:, 0]) and torch.equal(bits(score0), bits(score))
    n = rules["no_repeat_ngram"]
    for h in seq.reshape(-1, d.T).tolist():
        assert not BR.repeats_ngram(BR.cut(h), n) and UNK not in h
    assert torch.equal(eng.words[1:].view(d.T, d.B, beam).cpu(), ref["word"]) and torch.equal(eng.parent.view(d.T, d.B, beam).cpu(), ref["parent"])


@pytest.mark.parametrize("name,beam,path", [("tiny", 3, "tile"), ("tiny", 2, "ring"), ("cfg1", 5, "tile")])
def test_rules_that_never_fire_give_the_beam_history_engine(dev, name, beam, path):
    d, a = _engine(dev, name, 4321, beam, path, beam_history=True)
    d, b = _engine(dev, name, 4321, beam, path, beam_history=True, no_repeat_ngram=64)          # T <= 10: no earlier window
    assert b.constrained
    ra, rb = _grab(a), _grab(b)
    _same(ra, rb, f"{name} {path}")
    assert torch.equal(a.bhist[d.T & 1], b.bhist[d.T & 1]) and bool((b.nbanned == 1).all())


@pytest.mark.parametrize("name,beam,path", [("tiny", 3, "tile"), ("tiny", 2, "ring"), ("cfg1", 3, "tile")])
def test_eager_equals_a_captured_graph_across_two_batches(dev, name, beam, path):
    from helpers import to_dev
    d, sd, f_np, _, _ = TS._inputs(name)
    fd, f2 = to_dev(f_np, dev), to_dev(synth.clip_features(d, 777), dev)
    kw = dict(beam_history=True, no_repeat_ngram=2, min_len=2, own_features=True)
    _, e = _engine(dev, name, 4321, beam, path, **kw)
    _, g = _engine(dev, name, 4321, beam, path, **kw)
    g.capture()
    assert g.graph is not None
    grab = lambda x: list(_grab(x).values()) + [x.hypotheses()[0].clone(), x.nbanned.clone()]
    first = None
    for feats in (fd, f2, fd):
        e.load_features(feats)
        g.load_features(feats)
        re_, rg = grab(e), grab(g)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(re_, rg))
        for h in rg[-2].reshape(-1, d.T).tolist():
            assert not BR.repeats_ngram(BR.cut(h), 2) and 0 not in h[:2]
        if first is None:
            first = rg
        elif feats is fd:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, rg))      # the first batch again: the same decode
    g.load_features(f2)
    assert not torch.equal(bits(first[1]), bits(grab(g)[1]))        # another batch: other attention maps


# ------------------------------------------------------------------ 4. model, CLI
def test_model_sample_builds_a_history_engine_and_rebinds_when_a_constraint_changes(dev):
    from helpers import build_model, to_dev
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=True)
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, 99), dev)
    s0 = TS._model_sample(model, f, b, beam_size=3)
    e0 = model._engine_cache[1]
    assert s0[2] is None and e0.beam == 3 and not e0.beam_hist and not e0.constrained
    s1 = TS._model_sample(model, f, b, beam_size=3, no_repeat_ngram=2)
    e1 = model._engine_cache[1]
    assert e1 is not e0 and e1.beam_hist and e1.constrained and e1.cons[0] == 2 and e1.graph is not None
    assert s1[2] is None and s1[0].shape == (d.B, d.T) and s1[1].shape[:2] == (d.B, d.T)          # what a beam _sample returns
    for h in e1.hypotheses()[0].reshape(-1, d.T).tolist():
        assert not BR.repeats_ngram(BR.cut(h), 2)
    assert any(BR.repeats_ngram(BR.cut(h), 2) for h in s0[0].tolist())                             # the free beam decode repeats
    TS._model_sample(model, f, b, beam_size=3, no_repeat_ngram=2)
    assert model._engine_cache[1] is e1                          # same rules: the cached engine
    w = int(s1[0][0, 0])
    s2 = TS._model_sample(model, f, b, beam_size=3, no_repeat_ngram=2, ban_words=[w])
    e2 = model._engine_cache[1]
    assert e2 is not e1 and e2.beam_hist and e2.cons[3] == (w,) and not (e2.hypotheses()[0] == w).any()
    s3 = TS._model_sample(model, f, b, beam_size=3)
    assert not model._engine_cache[1].beam_hist and torch.equal(s3[0], s0[0]) and torch.equal(bits(s3[1]), bits(s0[1]))


def test_cli_flags_reach_the_engine(dev, tmp_path):
    from cvc import main as cvc_main
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16",
              "--seq_length", "6", "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100",
              "--exp_name", "s", "--learning_rate", "0.001", "--results_dir", str(tmp_path / "results"),
              "--checkpoint_path", str(tmp_path) + "/", "--id", "s1"]
    flags = ["--beam_size", "5", "--no_repeat_ngram", "3", "--min_caption_len", "5"]
    assert cvc_main.main(common + flags) == 0                  # one epoch, then the evaluation decodes under the rules
    tr = cvc_main.LAST_TRAINER
    e = getattr(tr.model, "module", tr.model)._engine_cache[1]
    assert e.beam == 5 and e.beam_hist and e.constrained and e.cons == (3, False, 5, (), ())
    seq, score = e.hypotheses()
    for h, s in zip(seq.reshape(-1, 6).tolist(), score.reshape(-1).tolist()):
        if np.isfinite(s):
            assert not BR.repeats_ngram(BR.cut(h), 3) and 0 not in h[:5] and UNK not in h
