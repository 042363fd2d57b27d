"""Diverse (group) beam search and the length-normalised final ranking on the GPU (pytest -m gpu): the selection block
cvc_beam_select_groups_parts (csrc/beam.hip, the GROUPS form of the beam merge) against the fp64 reference
(tests/beam_groups_ref.py) on every clip, one group against cvc_beam_select_hist_parts bit for bit, cvc_beam_rank and
cvc_beam_backtrack_from against the host, the engine against the reference decoder on tile and ring, lambda = 0 against the narrower
beam engine, graph replay, and the model / CLI plumbing.

The block cases are the integer-logit cases of tests/tile_path_cases.py::beam_case with planted histories and 40 % frozen rows;
tests/test_beam_groups_cpu.py asserts that their augmented values are exactly tied or at least GAP apart too, so parent, word, done,
the histories and nbanned are compared exactly and the scores at SCORE_TOL."""
import numpy as np
import pytest
import torch

from cvc import synth
import tile_path_cases as T
from tile_path_cases import SCORE_TOL, close, nan_buf
import beam_constrain_ref as BR
import beam_groups_ref as GR
import beam_groups_cases as GC
import test_gpu_tile_path as TP               # the sentinels
import test_gpu_sampling as TS                # the model's inputs

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
BADARG, TOOBIG = -1, -2
T_HIST = GC.T_HIST
bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def groups_run(c, dev, t, hist, rules, groups, lam, hist_block=False, t_arg=None):
    """cvc_beam_select_groups_parts (hist_block: cvc_beam_select_hist_parts) on a tile_path_cases beam case.  hist [T_HIST, rows]
    int64 (host).  Every output is pre-filled with a value no launch writes.
    -> rc, parent, word, score, done, hist_out [T_HIST, rows], nbanned"""
    from cvc import hip
    L = hip.lib()
    rows, V, nparts, stride = c["B"] * c["beam"], c["V"], c["nparts"], c["part_stride"]
    buf = nan_buf(nparts * stride + 8, dev=dev)
    for p in range(nparts):
        buf[p * stride:p * stride + rows * V] = c["parts"][p].reshape(-1).to(dev)
    bias = None
    if c["bias_v"] is not None:
        bias = nan_buf(V + 4, dev=dev)
        bias[:V] = c["bias_v"].to(dev)
        bias = bias[:V]
    score, done = c["score"].to(dev), c["done"].to(dev)
    parent = torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev)
    word = torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev)
    score_out = nan_buf(rows, dev=dev)
    done_out = torch.full((rows,), TP.DONE_FILL, dtype=torch.uint8, device=dev)
    nb = torch.full((rows,), TP.SENT, dtype=torch.int32, device=dev)
    ws = nan_buf(17 * rows, dev=dev)
    hin = torch.from_numpy(np.ascontiguousarray(hist)).to(dev)
    hout = torch.full((T_HIST, rows), TP.SENT, dtype=torch.int64, device=dev)
    i32 = lambda ids: torch.tensor(list(ids) or [0], dtype=torch.int32, device=dev)
    ban, bad = list(rules.get("ban_words", ())), list(rules.get("bad_endings", ()))
    ban_d, bad_d = i32(ban), i32(bad)
    desc = hip.Constraint(int(rules.get("no_repeat_ngram", 0)), int(bool(rules.get("no_immediate_repeat", False))),
                          int(rules.get("min_len", 0)), len(ban), ban_d.data_ptr(), bad_d.data_ptr(), len(bad))
    head = (buf.data_ptr(), nparts, stride, TP.P(bias), score.data_ptr(), done.data_ptr(), c["B"], c["beam"], V, c["unk"],
            t if t_arg is None else t_arg, hin.data_ptr(), hout.data_ptr(), rows, desc)
    tail = (parent.data_ptr(), word.data_ptr(), score_out.data_ptr(), done_out.data_ptr(), nb.data_ptr(), ws.data_ptr(), TP.st())
    if hist_block:
        rc = L.cvc_beam_select_hist_parts(*head, *tail)
    else:
        rc = L.cvc_beam_select_groups_parts(*head, groups, lam, *tail)
    torch.cuda.synchronize()
    return rc, parent, word, score_out, done_out, hout, nb


def untouched(out):
    rc, parent, word, score, done, hout, nb = out
    return (bool((parent == TP.SENT).all()) and bool((word == TP.SENT).all()) and bool(torch.isnan(score).all()) and
            bool((done == TP.DONE_FILL).all()) and bool((hout == TP.SENT).all()) and bool((nb == TP.SENT).all()))


def check_block(label, c, out, t, hist, rules, groups, lam):
    rc, parent, word, score, done, hout, nb = out
    B, beam, V = c["B"], c["beam"], c["V"]
    bd = beam // groups
    assert rc == 0, (label, rc)
    r = GC.block_ref(c, t, hist, rules, groups, lam)
    parent, word, score, done = parent.view(B, beam).cpu(), word.view(B, beam).cpu(), score.view(B, beam).cpu(), done.view(B, beam).cpu()
    assert bool(((parent >= 0) & (parent < beam) & (word >= 0) & (word < V)).all()), f"{label}: parent / word out of range"
    assert torch.equal(parent // bd, (torch.arange(beam) // bd).expand(B, beam)), f"{label}: a parent outside its group"
    live = r["live"]
    assert torch.equal(parent[live], r["parent"][live]), f"{label}: parent"
    assert torch.equal(word[live], r["word"][live]), f"{label}: word"
    assert torch.equal(done[live].bool(), r["done"][live]) and bool((done <= 1).all()), f"{label}: done"
    close(score[live], r["score"][live].float(), **SCORE_TOL)                  # the UNAUGMENTED score
    assert bool((score[~live] == -float("inf")).all()), f"{label}: a filler is not -inf"
    assert np.array_equal(nb.cpu().numpy(), r["nbanned"]), (label, nb[:8], r["nbanned"][:8])
    ho = hout.cpu().numpy()
    src = (parent + torch.arange(B).view(-1, 1) * beam).view(-1).numpy()
    assert np.array_equal(ho[:t], hist[:t][:, src]), f"{label}: gathered history"
    assert np.array_equal(ho[t], word.view(-1).numpy()), f"{label}: appended word"
    assert (ho[t + 1:] == TP.SENT).all(), f"{label}: wrote past step t"
    lv = live.view(-1).numpy()
    assert np.array_equal(ho[:t + 1][:, lv], r["hist"].T[:, lv]), f"{label}: history against the reference"
    return r


# ------------------------------------------------------------------ 1. the block against the reference, every clip
@pytest.mark.parametrize("si,beam,groups", GC.BLOCK_CASES)
def test_block_vs_reference_on_every_clip(dev, si, beam, groups):
    rules, hist = GC.rules_of(si), GC.planted_history(si, beam)
    penalised = False
    for t in GC.STEPS:
        c = GC.base_case(si, beam, t == 0)
        label = f"V={c['V']} beam={beam} G={groups} t={t}"
        first = groups_run(c, dev, t, hist, rules, groups, GC.LAMBDA)
        r = check_block(label, c, first, t, hist, rules, groups, GC.LAMBDA)
        again = groups_run(c, dev, t, hist, rules, groups, GC.LAMBDA)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first[1:], again[1:])), f"{label}: two launches differ"
        free = GC.block_ref(c, t, hist, rules, groups, 0.0)
        penalised |= not (torch.equal(free["parent"], r["parent"]) and torch.equal(free["word"], r["word"]))
        if groups == 1:                 # one group: the history block, bit for bit in every output
            plain = groups_run(c, dev, t, hist, rules, 1, 0.0, hist_block=True)
            assert plain[0] == 0
            for a, b, nm in zip(plain[1:], first[1:], ("parent", "word", "score", "done", "hist", "nbanned")):
                assert torch.equal(bits(a), bits(b)), f"{label}: {nm} differs from cvc_beam_select_hist_parts"
    # (V = 8: two allowed words per row, the penalty has little to choose from)
    assert penalised == (groups > 1) or (GC.SHAPES[si][0] == 8 and not penalised), f"V={GC.SHAPES[si][0]} beam={beam} G={groups}: the penalty never changed a selection"


def test_the_penalty_is_a_rounded_multiply_then_a_rounded_subtract(dev):
    """GC.rounding_case(): the penalised word ties exactly with another word of its row when lambda * pen is rounded on its own and
    the lower word wins; a fused multiply-add would choose the penalised word"""
    c, t, hist, lam, P, Q = GC.rounding_case()
    B, beam = c["B"], c["beam"]
    out = groups_run(c, dev, t, hist, {}, beam, lam)
    assert out[0] == 0
    r = GR.step(c["logits"], c["score"], c["done"], hist.T, t, B, beam, c["unk"], beam, lam)
    assert out[2].view(B, beam).cpu().tolist() == [[P, P, P, Q]] * B == r["word"].tolist()
    assert out[1].view(B, beam).cpu().tolist() == [[0, 1, 2, 3]] * B
    assert torch.equal(out[3].view(B, beam).cpu().double(), r["score"])               # exact values: the scores too, bit for bit


def test_refusals_leave_the_outputs_untouched(dev):
    c, hist = GC.base_case(1, 6, False), GC.planted_history(1, 6)
    for kw in (dict(groups=0), dict(groups=-2), dict(groups=4), dict(groups=7), dict(lam=-0.5), dict(lam=float("inf")), dict(lam=float("nan"))):
        a = dict(groups=2, lam=0.5)
        a.update(kw)
        out = groups_run(c, dev, 3, hist, {}, a["groups"], a["lam"])
        assert out[0] == BADARG and untouched(out), kw
    for t_arg in (-1, 65):              # the history block's checks still hold
        out = groups_run(c, dev, 3, hist, {}, 2, 0.5, t_arg=t_arg)
        assert out[0] == TOOBIG and untouched(out), t_arg
    out = groups_run(c, dev, 3, hist, dict(no_repeat_ngram=65), 2, 0.5)
    assert out[0] == BADARG and untouched(out)


@pytest.mark.parametrize("si,beam,groups", [(1, 6, 2), (1, 6, 6), (2, 6, 3), (2, 8, 4)])
def test_a_large_lambda_keeps_the_groups_words_apart(dev, si, beam, groups):
    """lambda far above the score range: every row of these cases holds more than `beam` finite candidates, so a group always finds
    bd words no earlier group took from a live parent"""
    rules, hist, lam = GC.rules_of(si), GC.planted_history(si, beam), 1000.0
    bd = beam // groups
    overlap_free = False
    for t in (1, 2, 63):
        c = GC.base_case(si, beam, False)
        B, V = c["B"], c["V"]
        out = groups_run(c, dev, t, hist, rules, groups, lam)
        r = check_block(f"large lambda V={V} beam={beam} G={groups} t={t}", c, out, t, hist, rules, groups, lam)
        parent, word, score = out[1].view(B, beam).cpu(), out[2].view(B, beam).cpu(), out[3].view(B, beam).cpu()
        frozen = c["done"].bool().view(B, beam)

        def overlaps(parent, word, score):
            n = 0
            for b in range(B):
                seen = set()
                for g in range(groups):
                    mine = {int(word[b, k]) for k in range(g * bd, (g + 1) * bd)
                            if not bool(frozen[b, parent[b, k]]) and np.isfinite(float(score[b, k]))}
                    n += len(mine & seen)
                    seen |= mine
            return n
        assert overlaps(parent, word, score) == 0
        free = GC.block_ref(c, t, hist, rules, groups, 0.0)
        overlap_free |= overlaps(free["parent"], free["word"], free["score"]) > 0
    assert overlap_free                 # without the penalty the groups do choose the same words


# ------------------------------------------------------------------ 2. the final ranking, backtracking from a slot
@pytest.mark.parametrize("alpha", [0.0, 0.7, 1.0])
def test_rank_on_planted_histories(dev, alpha):
    from cvc import hip
    B, beam, Tn, hist, score = GC.rank_case()
    rows = B * beam
    pad = 3
    hd = torch.full((Tn, rows + pad), 7, dtype=torch.int64, device=dev)
    hd[:, :rows] = torch.from_numpy(hist).to(dev)
    sc = torch.from_numpy(score).to(dev)
    order = torch.full((B, beam), TP.SENT, dtype=torch.int64, device=dev)
    norm = nan_buf(rows, dev=dev)
    ln = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    L = hip.lib()
    call = lambda **kw: L.cvc_beam_rank(*[{**dict(h=hd.data_ptr(), s=rows + pad, sc=sc.data_ptr(), B=B, beam=beam, T=Tn, a=alpha,
                                                  o=order.data_ptr(), n=norm.data_ptr(), l=ln.data_ptr(), st=TP.st()), **kw}[k]
                                          for k in ("h", "s", "sc", "B", "beam", "T", "a", "o", "n", "l", "st")])
    for kw, code in ((dict(h=None), BADARG), (dict(sc=None), BADARG), (dict(o=None), BADARG), (dict(n=None), BADARG), (dict(l=None), BADARG),
                     (dict(B=0), BADARG), (dict(beam=0), BADARG), (dict(beam=9), BADARG), (dict(T=0), BADARG), (dict(T=65), TOOBIG),
                     (dict(s=rows - 1), BADARG), (dict(a=-0.1), BADARG), (dict(a=float("inf")), BADARG), (dict(a=float("nan")), BADARG)):
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert bool((order == TP.SENT).all()) and bool(torch.isnan(norm).all()) and bool((ln == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    ref = GR.rank(hist.T.reshape(B, beam, Tn), score.reshape(B, beam), alpha)
    assert np.array_equal(ln.view(B, beam).cpu().numpy(), ref["len"])
    assert np.array_equal(order.cpu().numpy(), ref["order"])
    got, want = norm.view(B, beam).cpu(), torch.from_numpy(ref["norm"]).float()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    ok = ~torch.isnan(want)
    if alpha == 0.0:
        assert torch.equal(bits(got[ok]), bits(torch.from_numpy(score).view(B, beam)[ok]))
    else:
        inf = torch.isinf(want)
        assert torch.equal(got[inf], want[inf])
        close(got[ok & ~inf], want[ok & ~inf], **SCORE_TOL)


@pytest.mark.parametrize("B,beam,Tn,N", [(3, 5, 2, 7), (64, 8, 20, 100), (1, 8, 64, 1)])
def test_backtrack_from_a_slot(dev, B, beam, Tn, N):
    from cvc import hip
    L = hip.lib()
    c = T.backtrack_inputs(50 + B, B, beam, Tn, N)
    words, parent, att = c["words"].to(dev), c["parent"].to(dev), c["att"].to(dev)
    g = T.gen(60 + B)
    order = torch.randint(0, beam, (B, beam), generator=g)
    order[0, 0] = beam + 3                                        # clamped like a parent
    if B > 1:
        order[1, 0] = -2

    def run(fn, *start):
        seq = torch.full((B, Tn), TP.SENT, dtype=torch.int64, device=dev)
        out = nan_buf(B * Tn * N, dev=dev).view(B, Tn, N)
        rc = fn(words.data_ptr(), parent.data_ptr(), att.data_ptr(), B, beam, Tn, N, *start, seq.data_ptr(), out.data_ptr(), TP.st())
        torch.cuda.synchronize()
        return rc, seq.cpu(), out.cpu()
    od = order.to(dev)
    rc, seq, out = run(L.cvc_beam_backtrack_from, od.data_ptr(), beam)                  # column 0 of an order, in place
    assert rc == 0
    for b in range(B):
        k = min(max(int(order[b, 0]), 0), beam - 1)
        for t in range(Tn - 1, -1, -1):
            assert int(seq[b, t]) == int(c["words"][t, b * beam + k])
            kp = min(max(int(c["parent"][t, b * beam + k]), 0), beam - 1)
            assert torch.equal(out[b, t], c["att"][t, b * beam + kp])
            k = kp
    zeros = torch.zeros(B, dtype=torch.int64, device=dev)
    rc0, seq0, out0 = run(L.cvc_beam_backtrack_from, zeros.data_ptr(), 1)
    rcp, seqp, outp = run(L.cvc_beam_backtrack)
    assert rc0 == 0 and rcp == 0 and torch.equal(seq0, seqp) and torch.equal(bits(out0), bits(outp))
    rc, seq, out = run(L.cvc_beam_backtrack_from, None, 1)
    assert rc == BADARG and bool((seq == TP.SENT).all()) and bool(torch.isnan(out).all())
    assert run(L.cvc_beam_backtrack_from, zeros.data_ptr(), 0)[0] == BADARG


# ------------------------------------------------------------------ 3. the engine
def _engine(dev, i, path, **kw):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    name, seed, beam, groups, lam, alpha, eos, rules = GR.ENGINE_CASES[i]
    d, sd, f_np = GR.case_inputs(i)
    args = dict(beam=beam, path=path, beam_history=True, beam_groups=groups, diversity=lam, length_penalty=alpha, **rules)
    args.update(kw)
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, **args)
    assert eng.tile == (path == "tile") and not eng.packed and eng._plan is None
    return d, eng


@pytest.mark.parametrize("path", ["tile", "ring"])
@pytest.mark.parametrize("i", range(len(GR.ENGINE_CASES)))
def test_engine_vs_reference_decoder(dev, i, path):
    from cvc import hip
    name, seed, beam, groups, lam, alpha, eos, rules = GR.ENGINE_CASES[i]
    d, P, f, ref = GR.shared_decode(i)
    assert min(ref["margin"].min(), ref["rank_margin"]) >= GR.MARGIN_MIN and bool(torch.isfinite(ref["score"]).all())
    d, eng = _engine(dev, i, path)
    assert eng.ranked and eng.grouped == (groups > 1) and eng.beam_hist
    sel = [fn for nm, fn, _ in eng._python_launches() if nm == "word_select"]
    want = hip.lib().cvc_beam_select_groups_parts if groups > 1 else hip.lib().cvc_beam_select_hist_parts
    assert len(sel) == d.T and all(fn is want for fn in sel)
    seq0, att0, score0 = eng.run()
    seq, score = eng.hypotheses()
    err = float((score.cpu().double() - ref["score"]).abs().max())
    print(f"diverse beam {GR.ENGINE_CASES[i]} {path}: max |score - ref| = {err:.3e}, smallest margins {ref['margin'].min():.3e} / "
          f"{ref['rank_margin']:.3e}")
    assert torch.equal(seq.cpu(), ref["seq"])                                    # all hypotheses, exact
    assert torch.equal(eng.words[1:].view(d.T, d.B, beam).cpu(), ref["word"]) and torch.equal(eng.parent.view(d.T, d.B, beam).cpu(), ref["parent"])
    if eng.constrained:
        assert np.array_equal(eng.nbanned.cpu().numpy(), ref["nbanned"])
    np.testing.assert_allclose(score.cpu().double().numpy(), ref["score"].numpy(), rtol=0, atol=2e-4)
    assert np.array_equal(eng.order.cpu().numpy(), ref["order"]) and np.array_equal(eng.hyp_len.cpu().numpy(), ref["len"])
    np.testing.assert_allclose(eng.norm.cpu().double().numpy(), ref["norm"], rtol=0, atol=2e-4)
    # run() returns the best hypothesis by norm and its attention rows; ranked=True the n-best in that order
    o = torch.from_numpy(ref["order"])
    best = o[:, 0]
    assert torch.equal(seq0.cpu(), ref["seq"][torch.arange(d.B), best]) and torch.equal(bits(score0), bits(score))
    host_seq, host_att = _host_backtrack(eng, best.to(dev))
    assert torch.equal(seq0, host_seq) and torch.equal(bits(att0), bits(host_att))
    rseq, rscore, rnorm, rgroup = eng.hypotheses(ranked=True)
    assert torch.equal(rseq.cpu(), ref["seq"].gather(1, o.unsqueeze(2).expand(-1, -1, d.T)))
    assert torch.equal(bits(rscore), bits(score.gather(1, eng.order))) and torch.equal(bits(rnorm), bits(eng.norm.gather(1, eng.order)))
    assert np.array_equal(rgroup.cpu().numpy(), ref["group"][ref["order"]])
    n = rules.get("no_repeat_ngram", 0)
    for h in seq.reshape(-1, d.T).tolist():
        assert UNK not in h and (n == 0 or not BR.repeats_ngram(BR.cut(h), n))
        assert 0 not in h[:rules.get("min_len", 0)]


def _host_backtrack(eng, start):
    B, beam, Tn, N = eng.B, eng.beam, eng.T, eng.N
    words, parent, att = eng.words[1:].view(Tn, B, beam), eng.parent.view(Tn, B, beam), eng.att_steps.view(Tn, B, beam, N)
    k, ar = start.clone(), torch.arange(B, device=start.device)
    seq, atts = [], []
    for t in range(Tn - 1, -1, -1):
        seq.append(words[t, ar, k])
        kp = parent[t, ar, k]
        atts.append(att[t, ar, kp])
        k = kp
    seq.reverse()
    atts.reverse()
    return torch.stack(seq, 1), torch.stack(atts, 1)


# (the narrow engines are cases of beam_constrain_ref.ENGINE_CASES: seed 4321, no_repeat_ngram = 2, margins >= 1.4e-3)
@pytest.mark.parametrize("name,beam,groups,path", [("tiny", 6, 3, "tile"), ("tiny", 4, 2, "ring"), ("cfg1", 6, 2, "tile"), ("cfg1", 4, 2, "ring")])
def test_with_lambda_zero_every_group_is_the_narrower_beam_engine(dev, name, beam, groups, path):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, _, _ = TS._inputs(name)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    bd = beam // groups
    wide = DecodeEngine(W, fd, d.T, UNK, beam=beam, path=path, beam_history=True, beam_groups=groups, no_repeat_ngram=2)
    wide.run()
    seq, score = (x.clone() for x in wide.hypotheses())
    narrow = DecodeEngine(W, fd, d.T, UNK, beam=bd, path=path, beam_history=True, no_repeat_ngram=2)
    narrow.run()
    nseq, nscore = narrow.hypotheses()
    for g in range(groups):
        assert torch.equal(seq[:, g * bd:(g + 1) * bd], nseq), f"group {g}"
        close(score[:, g * bd:(g + 1) * bd].cpu(), nscore.cpu(), rtol=0, atol=2e-4)


@pytest.mark.parametrize("i,path", [(0, "tile"), (1, "ring"), (4, "tile")])
def test_eager_equals_a_captured_graph_across_two_batches(dev, i, path):
    from helpers import to_dev
    name, seed, beam, groups, lam, alpha, eos, rules = GR.ENGINE_CASES[i]
    d, e = _engine(dev, i, path, own_features=True)
    d, g = _engine(dev, i, path, own_features=True)
    g.capture()
    assert g.graph is not None
    _, _, f_np = GR.case_inputs(i)
    fd, f2 = to_dev(f_np, dev), to_dev(synth.clip_features(d, 777), dev)

    def grab(x):
        out = [t.clone() for t in x.run()] + [x.order.clone(), x.norm.clone(), x.hyp_len.clone(), x.words.clone(), x.parent.clone()]
        return out + [t.clone() for t in x.hypotheses(ranked=True)]
    first = None
    for feats in (fd, f2, fd):
        e.load_features(feats)
        g.load_features(feats)
        re_, rg = grab(e), grab(g)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(re_, rg))
        if first is None:
            first = rg
        elif feats is fd:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, rg))      # the first batch again: the same decode
    g.load_features(f2)
    assert not torch.equal(bits(first[1]), bits(grab(g)[1]))        # another batch: other attention maps


# ------------------------------------------------------------------ 4. model, CLI
def test_model_sample_rebinds_when_one_of_the_three_values_changes(dev):
    from helpers import build_model, to_dev
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=True)
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, 99), dev)
    s0 = TS._model_sample(model, f, b, beam_size=6)
    e0 = model._engine_cache[1]
    assert not e0.beam_hist and not getattr(e0, "ranked", False)
    s1 = TS._model_sample(model, f, b, beam_size=6, beam_groups=3, diversity_lambda=0.5)
    e1 = model._engine_cache[1]
    assert e1 is not e0 and e1.beam_hist and e1.grouped and e1.groups == 3 and e1.diversity == 0.5 and e1.graph is not None
    assert s1[2] is None and s1[0].shape == (d.B, d.T)
    assert torch.equal(s1[0], e1.hypotheses(ranked=True)[0][:, 0])
    TS._model_sample(model, f, b, beam_size=6, beam_groups=3, diversity_lambda=0.5)
    assert model._engine_cache[1] is e1                          # the same values: the cached engine
    TS._model_sample(model, f, b, beam_size=6, beam_groups=3, diversity_lambda=0.25)
    e2 = model._engine_cache[1]
    assert e2 is not e1 and e2.diversity == 0.25
    TS._model_sample(model, f, b, beam_size=6, beam_groups=2, diversity_lambda=0.25)
    e3 = model._engine_cache[1]
    assert e3 is not e2 and e3.groups == 2
    TS._model_sample(model, f, b, beam_size=6, beam_groups=2, diversity_lambda=0.25, length_penalty=0.7)
    e4 = model._engine_cache[1]
    assert e4 is not e3 and e4.length_penalty == 0.7
    TS._model_sample(model, f, b, beam_size=6, length_penalty=0.7, no_repeat_ngram=2)
    e5 = model._engine_cache[1]
    assert e5 is not e4 and e5.ranked and not e5.grouped and e5.constrained and e5.beam_hist
    s6 = TS._model_sample(model, f, b, beam_size=6)
    assert not model._engine_cache[1].beam_hist and torch.equal(s6[0], s0[0]) and torch.equal(bits(s6[1]), bits(s0[1]))


def test_cli_flags_reach_the_engine(dev, tmp_path):
    from cvc import main as cvc_main
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16",
              "--seq_length", "6", "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100",
              "--exp_name", "s", "--learning_rate", "0.001", "--results_dir", str(tmp_path / "results"),
              "--checkpoint_path", str(tmp_path) + "/", "--id", "s1"]
    flags = ["--beam_size", "6", "--group_size", "3", "--diversity_lambda", "0.5", "--length_penalty", "0.7"]
    assert cvc_main.main(common + flags) == 0                  # one epoch, then the evaluation decodes in groups
    tr = cvc_main.LAST_TRAINER
    e = getattr(tr.model, "module", tr.model)._engine_cache[1]
    assert e.beam == 6 and e.beam_hist and e.grouped and (e.groups, e.diversity, e.length_penalty) == (3, 0.5, 0.7)
    seq, score, norm, group = e.hypotheses(ranked=True)
    assert seq.shape == (e.B, 6, 6) and sorted(group[0].tolist()) == [0, 0, 1, 1, 2, 2]
    fin = torch.isfinite(norm)
    assert bool((norm[:, :-1] >= norm[:, 1:])[fin[:, :-1] & fin[:, 1:]].all())
