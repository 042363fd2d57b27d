"""Lexically constrained beam search (forced words per clip) on the GPU (pytest -m gpu): the selection block
cvc_beam_select_force_parts (csrc/beam.hip, the FORCE form of the row scan and the BANKS form of the beam merge) against the fp64
reference (tests/force_ref.py) on every clip, with no active entry against cvc_beam_select_hist_parts at beam bd, cvc_beam_rank_force
against the host, the engine against the reference decoder on tile and ring, graph replay across batches with other forced words,
force_n = 0 against the history engine, and the model / CLI plumbing.

The block cases are the integer-logit cases of tests/tile_path_cases.py::beam_case with planted histories and 40 % frozen rows
(tests/force_cases.py); tests/test_beam_forced_cpu.py asserts that the candidates of a bank are exactly tied or at least GAP apart, so
parent, word, done, the histories, nbanned and nmet are compared exactly and the scores at SCORE_TOL.  Filler slots (fewer finite
candidates than bd in a bank -- common here: bank j is empty while t < j) are compared by score and by range only."""
import numpy as np
import pytest
import torch

from cvc import synth
import tile_path_cases as T
from tile_path_cases import SCORE_TOL, close, nan_buf
import force_ref as FR
import force_cases as FC
import test_gpu_tile_path as TP               # the sentinels
import test_gpu_sampling as TS                # the model's inputs
import test_gpu_beam_groups as TG             # the host backtrack

pytestmark = pytest.mark.gpu

UNK = synth.UNK_IDX
BADARG, TOOBIG = -1, -2
T_HIST = FC.T_HIST
bits = lambda x: x.view(torch.int32) if x.is_floating_point() else x
NAMES = ("parent", "word", "score", "done", "hist", "nbanned", "nmet")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def force_run(c, dev, t, hist, rules, force, hist_block=False, t_arg=None, C_arg=None, no_force=False):
    """cvc_beam_select_force_parts (hist_block: cvc_beam_select_hist_parts) on a tile_path_cases beam case.  hist [T_HIST, rows]
    int64 (host), force [B, C] int32 (host).  Every output is pre-filled with a value no launch writes.
    -> rc, parent, word, score, done, hist_out [T_HIST, rows], nbanned, nmet"""
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
    nm = torch.full((rows,), TP.SENT, dtype=torch.int32, device=dev)
    ws = nan_buf(21 * rows, dev=dev)
    hin = torch.from_numpy(np.ascontiguousarray(hist)).to(dev)
    hout = torch.full((T_HIST, rows), TP.SENT, dtype=torch.int64, device=dev)
    i32 = lambda ids: torch.tensor(list(ids) or [0], dtype=torch.int32, device=dev)
    ban, bad = list(rules.get("ban_words", ())), list(rules.get("bad_endings", ()))
    ban_d, bad_d = i32(ban), i32(bad)
    fd = torch.from_numpy(np.ascontiguousarray(force, dtype=np.int32)).to(dev)
    desc = hip.Constraint(int(rules.get("no_repeat_ngram", 0)), int(bool(rules.get("no_immediate_repeat", False))),
                          int(rules.get("min_len", 0)), len(ban), ban_d.data_ptr(), bad_d.data_ptr(), len(bad))
    head = (buf.data_ptr(), nparts, stride, TP.P(bias), score.data_ptr(), done.data_ptr(), c["B"], c["beam"], V, c["unk"],
            t if t_arg is None else t_arg, hin.data_ptr(), hout.data_ptr(), rows, desc)
    tail = (parent.data_ptr(), word.data_ptr(), score_out.data_ptr(), done_out.data_ptr(), nb.data_ptr())
    if hist_block:
        rc = L.cvc_beam_select_hist_parts(*head, *tail, ws.data_ptr(), TP.st())
    else:
        rc = L.cvc_beam_select_force_parts(*head, None if no_force else fd.data_ptr(), force.shape[1] if C_arg is None else C_arg, *tail,
                                           nm.data_ptr(), ws.data_ptr(), TP.st())
    torch.cuda.synchronize()
    return rc, parent, word, score_out, done_out, hout, nb, nm


def untouched(out):
    rc, parent, word, score, done, hout, nb, nm = out
    return (bool((parent == TP.SENT).all()) and bool((word == TP.SENT).all()) and bool(torch.isnan(score).all()) and
            bool((done == TP.DONE_FILL).all()) and bool((hout == TP.SENT).all()) and bool((nb == TP.SENT).all()) and
            bool((nm == TP.SENT).all()))


def check_block(label, c, out, t, hist, force, r):
    rc, parent, word, score, done, hout, nb, nm = out
    B, beam, V = c["B"], c["beam"], c["V"]
    assert rc == 0, (label, rc)
    parent, word, score, done = parent.view(B, beam).cpu(), word.view(B, beam).cpu(), score.view(B, beam).cpu(), done.view(B, beam).cpu()
    assert bool(((parent >= 0) & (parent < beam) & (word >= 0) & (word < V)).all()), f"{label}: parent / word out of range"
    live = r["live"]
    assert torch.equal(parent[live], r["parent"][live]), f"{label}: parent"
    assert torch.equal(word[live], r["word"][live]), f"{label}: word"
    assert torch.equal(done[live].bool(), r["done"][live]) and bool((done <= 1).all()), f"{label}: done"
    close(score[live], r["score"][live].float(), **SCORE_TOL)
    assert bool((score[~live] == -float("inf")).all()), f"{label}: a filler is not -inf"
    assert np.array_equal(nb.cpu().numpy(), r["nbanned"]), (label, nb[:8], r["nbanned"][:8])
    assert np.array_equal(nm.cpu().numpy(), r["nmet"]), (label, nm[:8], r["nmet"][:8])
    ho = hout.cpu().numpy()
    src = (parent + torch.arange(B).view(-1, 1) * beam).view(-1).numpy()
    assert np.array_equal(ho[:t], hist[:t][:, src]), f"{label}: gathered history"
    assert np.array_equal(ho[t], word.view(-1).numpy()), f"{label}: appended word"
    assert (ho[t + 1:] == TP.SENT).all(), f"{label}: wrote past step t"
    lv = live.view(-1).numpy()
    assert np.array_equal(ho[:t + 1][:, lv], r["hist"].T[:, lv]), f"{label}: history against the reference"
    # the invariant, on what the block wrote: a finite slot of bank j holds exactly j active forced words
    assert not FR.invariant_violations(dict(hist=ho[:t + 1].T, score=score), force, beam, V, c["unk"]), f"{label}: invariant"


# ------------------------------------------------------------------ 1. the block against the reference, every clip
@pytest.mark.parametrize("si,beam,C", FC.BLOCK_CASES)
def test_block_vs_reference_on_every_clip(dev, si, beam, C):
    rules, hist, force = FC.rules_of(si), FC.planted_history(si, beam), FC.force_of(si, C)
    for t in FC.STEPS:
        c = FC.base_case(si, beam, t == 0)
        label = f"V={c['V']} beam={beam} C={C} t={t}"
        first = force_run(c, dev, t, hist, rules, force)
        check_block(label, c, first, t, hist, force, FC.block_ref(si, beam, C, t))
        again = force_run(c, dev, t, hist, rules, force)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first[1:], again[1:])), f"{label}: two launches differ"


@pytest.mark.parametrize("si,beam,C", FC.BLOCK_CASES)
def test_with_no_active_entry_bank_zero_is_the_history_block_at_beam_bd(dev, si, beam, C):
    """every entry -1 and the rows of the other banks at -inf (what they hold in a decode without forced words): slots [0, bd) are
    cvc_beam_select_hist_parts at beam bd on the inputs of the clip's rows [0, bd), bit for bit"""
    rules, hist = FC.rules_of(si), FC.planted_history(si, beam)
    bd = beam // (C + 1)
    none = np.full((FC.B, C), -1, dtype=np.int32)
    rows = torch.arange(FC.B * beam)
    keep = rows[rows % beam < bd]
    for t in FC.STEPS:
        c = dict(FC.base_case(si, beam, t == 0))
        V = c["V"]
        c["score"] = torch.where(rows % beam < bd, c["score"], torch.full_like(c["score"], -float("inf")))
        wide = force_run(c, dev, t, hist, rules, none)
        narrow_c = dict(c, beam=bd, score=c["score"][keep], done=c["done"][keep], parts=c["parts"][:, keep], part_stride=len(keep) * V)
        narrow = force_run(narrow_c, dev, t, hist[:, keep.numpy()], rules, none, hist_block=True)
        assert wide[0] == 0 and narrow[0] == 0
        label = f"V={V} beam={beam} C={C} t={t}"
        sl = lambda x, w: x.view(FC.B, w)[:, :bd].cpu()
        fin = torch.isfinite(sl(narrow[3], bd))
        assert torch.equal(torch.isfinite(sl(wide[3], beam)), fin), f"{label}: fillers"
        for a, b, nm in zip(wide[1:5], narrow[1:5], NAMES):
            assert torch.equal(bits(sl(a, beam))[fin], bits(sl(b, bd))[fin]), f"{label}: {nm} differs from cvc_beam_select_hist_parts"
        hw, hn = wide[5][:t + 1].view(t + 1, FC.B, beam)[:, :, :bd].cpu(), narrow[5][:t + 1].view(t + 1, FC.B, bd).cpu()
        assert torch.equal(hw[:, fin], hn[:, fin]), f"{label}: histories"
        assert bool((wide[3].view(FC.B, beam)[:, bd:] == -float("inf")).all()), f"{label}: the other banks are not fillers"
        assert torch.equal(wide[6].view(FC.B, beam)[:, :bd], narrow[6].view(FC.B, bd)) and bool((wide[7] == 0).all())


def test_refusals_leave_the_outputs_untouched(dev):
    c, hist, force = FC.base_case(1, 6, False), FC.planted_history(1, 6), FC.force_of(1, 2)
    for kw in (dict(C_arg=0), dict(C_arg=-1), dict(C_arg=4), dict(C_arg=3), dict(C_arg=4), dict(no_force=True)):
        out = force_run(c, dev, 3, hist, {}, force, **kw)
        assert out[0] == BADARG and untouched(out), kw
    for t_arg in (-1, 65):              # the history block's checks still hold
        out = force_run(c, dev, 3, hist, {}, force, t_arg=t_arg)
        assert out[0] == TOOBIG and untouched(out), t_arg
    out = force_run(c, dev, 3, hist, dict(no_repeat_ngram=65), force)
    assert out[0] == BADARG and untouched(out)


# ------------------------------------------------------------------ 2. the final ranking
@pytest.mark.parametrize("alpha", [0.0, 0.7])
def test_rank_force_on_planted_histories(dev, alpha):
    from cvc import hip
    B, beam, Tn, V, hist, score, force = FC.rank_case()
    rows, C = B * beam, force.shape[1]
    pad = 3
    hd = torch.full((Tn, rows + pad), 7, dtype=torch.int64, device=dev)
    hd[:, :rows] = torch.from_numpy(hist).to(dev)
    sc, fd = torch.from_numpy(score).to(dev), torch.from_numpy(force).to(dev)
    order = torch.full((B, beam), TP.SENT, dtype=torch.int64, device=dev)
    norm = nan_buf(rows, dev=dev)
    ln = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    nm = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    L = hip.lib()
    keys = ("h", "s", "sc", "f", "C", "B", "beam", "T", "V", "unk", "a", "o", "n", "l", "m", "st")
    call = lambda **kw: L.cvc_beam_rank_force(*[{**dict(h=hd.data_ptr(), s=rows + pad, sc=sc.data_ptr(), f=fd.data_ptr(), C=C, B=B, beam=beam,
                                                        T=Tn, V=V, unk=UNK, a=alpha, o=order.data_ptr(), n=norm.data_ptr(), l=ln.data_ptr(),
                                                        m=nm.data_ptr(), st=TP.st()), **kw}[k] for k in keys])
    for kw, code in ((dict(h=None), BADARG), (dict(sc=None), BADARG), (dict(o=None), BADARG), (dict(n=None), BADARG), (dict(l=None), BADARG),
                     (dict(B=0), BADARG), (dict(beam=0), BADARG), (dict(beam=9), BADARG), (dict(T=0), BADARG), (dict(T=65), TOOBIG),
                     (dict(s=rows - 1), BADARG), (dict(a=-0.1), BADARG), (dict(a=float("inf")), BADARG), (dict(a=float("nan")), BADARG),
                     (dict(f=None), BADARG), (dict(m=None), BADARG), (dict(C=0), BADARG), (dict(C=4), BADARG), (dict(V=0), BADARG)):
        assert call(**kw) == code, kw
    torch.cuda.synchronize()
    assert bool((order == TP.SENT).all()) and bool(torch.isnan(norm).all()) and bool((ln == -7).all()) and bool((nm == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    ref = FR.rank(hist.T.reshape(B, beam, Tn), score.reshape(B, beam), alpha, force, V, UNK)
    assert np.array_equal(ln.view(B, beam).cpu().numpy(), ref["len"])
    assert np.array_equal(nm.view(B, beam).cpu().numpy(), ref["nmet"])
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
    # with no active entry: cvc_beam_rank's order, norm and len, bit for bit
    o2, n2, l2 = torch.zeros_like(order), torch.zeros_like(norm), torch.zeros_like(ln)
    assert L.cvc_beam_rank(hd.data_ptr(), rows + pad, sc.data_ptr(), B, beam, Tn, alpha, o2.data_ptr(), n2.data_ptr(), l2.data_ptr(), TP.st()) == 0
    none = torch.full((B, C), -1, dtype=torch.int32, device=dev)
    assert call(f=none.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(order, o2) and torch.equal(bits(norm), bits(n2)) and torch.equal(ln, l2) and bool((nm == 0).all())


# ------------------------------------------------------------------ 3. the engine
def _engine(dev, i, path, **kw):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    name, seed, beam, C, alpha, eos, rules = FR.ENGINE_CASES[i]
    d, sd, f_np, force = FR.case_inputs(i)
    args = dict(beam=beam, path=path, beam_history=True, force_n=C, length_penalty=alpha, **rules)
    args.update(kw)
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, UNK, **args)
    assert eng.tile == (path == "tile") and not eng.packed and eng._plan is None
    return d, eng.load_force_words(force)


@pytest.mark.parametrize("path", ["tile", "ring"])
@pytest.mark.parametrize("i", range(len(FR.ENGINE_CASES)))
def test_engine_vs_reference_decoder(dev, i, path):
    from cvc import hip
    name, seed, beam, C, alpha, eos, rules = FR.ENGINE_CASES[i]
    d, P, f, force, ref = FR.shared_decode(i)
    assert min(ref["margin"].min(), ref["rank_margin"]) >= FR.MARGIN_MIN
    d, eng = _engine(dev, i, path)
    assert eng.ranked and eng.forcing and eng.beam_hist and not eng.grouped
    sel = [fn for nm, fn, _ in eng._python_launches() if nm == "word_select"]
    assert len(sel) == d.T and all(fn is hip.lib().cvc_beam_select_force_parts for fn in sel)
    seq0, att0, score0 = eng.run()
    seq, score = eng.hypotheses()
    fin = torch.isfinite(ref["score"])                                           # the hypotheses; the other slots are fillers
    assert torch.equal(torch.isfinite(score.cpu()), fin) and bool((score.cpu()[~fin] == -float("inf")).all())
    err = float((score.cpu().double() - ref["score"])[fin].abs().max())
    print(f"forced beam {FR.ENGINE_CASES[i]} {path}: max |score - ref| = {err:.3e}, smallest margins {ref['margin'].min():.3e} / "
          f"{ref['rank_margin']:.3e}")
    assert torch.equal(seq.cpu()[fin], ref["seq"][fin])                          # all hypotheses, exact
    live = ref["live"]
    words, parent = eng.words[1:].view(d.T, d.B, beam).cpu(), eng.parent.view(d.T, d.B, beam).cpu()
    assert torch.equal(words[live], ref["word"][live]) and torch.equal(parent[live], ref["parent"][live])
    assert bool(((words >= 0) & (words < d.V) & (parent >= 0) & (parent < beam)).all())
    # nbanned / nmet of the rows entering step t: every row at t = 0, then the slots step t - 1 filled with a hypothesis
    entering = torch.cat([torch.ones(1, d.B * beam, dtype=torch.bool), live[:-1].view(d.T - 1, -1)], 0).numpy()
    assert np.array_equal(eng.nmet.cpu().numpy()[entering], ref["nmet"][entering])
    if eng.constrained:
        assert np.array_equal(eng.nbanned.cpu().numpy()[entering], ref["nbanned"][entering])
    assert err <= 2e-4
    fn = fin.numpy()
    assert np.array_equal(eng.hyp_len.cpu().numpy()[fn], ref["len"][fn]) and np.array_equal(eng.final_nmet.cpu().numpy()[fn], ref["final_nmet"][fn])
    np.testing.assert_allclose(eng.norm.cpu().double().numpy()[fn], ref["norm"][fn], rtol=0, atol=2e-4)
    order = eng.order.cpu().numpy()
    for b in range(d.B):                # the hypotheses in the reference's order, then the fillers (what they hold is not part of the rule)
        nf = int(fn[b].sum())
        assert np.array_equal(order[b, :nf], ref["order"][b, :nf]) and sorted(order[b].tolist()) == list(range(beam))
    # run() returns the best hypothesis by the key and its attention rows; ranked=True the n-best in that order
    o = eng.order.cpu()
    best = torch.from_numpy(ref["order"])[:, 0]
    assert torch.equal(seq0.cpu(), ref["seq"][torch.arange(d.B), best]) and torch.equal(bits(score0), bits(score))
    host_seq, host_att = TG._host_backtrack(eng, best.to(dev))
    assert torch.equal(seq0, host_seq) and torch.equal(bits(att0), bits(host_att))
    rseq, rscore, rnorm, rnmet = eng.hypotheses(ranked=True)
    assert torch.equal(rseq.cpu(), seq.cpu().gather(1, o.unsqueeze(2).expand(-1, -1, d.T)))
    assert torch.equal(bits(rscore), bits(score.gather(1, eng.order))) and torch.equal(bits(rnorm), bits(eng.norm.gather(1, eng.order)))
    assert torch.equal(rnmet, eng.final_nmet.gather(1, eng.order))
    for b in range(d.B):                # what the feature is for: the returned caption holds every forced word of the clip
        want = {int(w) for w, a in zip(force[b], FR.active(force[b], d.V, UNK)) if a}
        assert want <= set(seq0[b].tolist()) and int(rnmet[b, 0]) == len(want)


@pytest.mark.parametrize("i,path", [(1, "tile"), (4, "ring"), (5, "tile")])
def test_eager_equals_a_captured_graph_across_two_batches(dev, i, path):
    from helpers import to_dev
    name, seed, beam, C, alpha, eos, rules = FR.ENGINE_CASES[i]
    d, e = _engine(dev, i, path, own_features=True)
    d, g = _engine(dev, i, path, own_features=True)
    g.capture()
    assert g.graph is not None
    _, _, f_np, force = FR.case_inputs(i)
    fd, f2 = to_dev(f_np, dev), to_dev(synth.clip_features(d, 777), dev)
    force2 = FR.force_words(d.B, C, d.V, UNK, 777)
    assert not np.array_equal(force, force2)

    def grab(x):
        out = [t.clone() for t in x.run()] + [x.order.clone(), x.norm.clone(), x.hyp_len.clone(), x.final_nmet.clone(), x.nmet.clone(),
                                              x.words.clone(), x.parent.clone()]
        return out + [t.clone() for t in x.hypotheses(ranked=True)]
    first = None
    for feats, words in ((fd, force), (f2, force2), (fd, force)):
        for x in (e, g):
            x.load_features(feats)
            x.load_force_words(words)
        re_, rg = grab(e), grab(g)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(re_, rg))
        if first is None:
            first = rg
        elif words is force:
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, rg))      # the first batch again: the same decode
    g.load_force_words(force2)                                      # the same clips, other forced words: another decode from the same graph
    other = grab(g)
    assert not torch.equal(other[0], first[0])
    for b in range(d.B):
        want = {int(w) for w, a in zip(force2[b], FR.active(force2[b], d.V, UNK)) if a}
        nmax = int(other[6][b][torch.isfinite(other[4][b])].max())           # (among the hypotheses: a filler's history is arbitrary)
        assert nmax <= len(want) and int(other[-1][b, 0]) == nmax


@pytest.mark.parametrize("path", ["tile", "ring"])
def test_force_n_zero_is_the_history_engine(dev, path):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, _, _ = TS._inputs("tiny")
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    kw = dict(beam=4, path=path, beam_history=True, no_repeat_ngram=2)
    a, b = DecodeEngine(W, fd, d.T, UNK, **kw), DecodeEngine(W, fd, d.T, UNK, force_n=0, **kw)
    assert not b.forcing and not b.ranked and not hasattr(b, "force_words") and b.beam_ws.numel() == a.beam_ws.numel()
    la, lb = a._python_launches(), b._python_launches()
    assert [(n, f) for n, f, _ in la] == [(n, f) for n, f, _ in lb] and [len(x[2]) for x in la] == [len(x[2]) for x in lb]
    ra, rb = [t.clone() for t in a.run()], [t.clone() for t in b.run()]
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(ra, rb))
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.hypotheses(), b.hypotheses()))
    with pytest.raises(RuntimeError, match="force_n = 0"):
        b.load_force_words(np.zeros((d.B, 1), dtype=np.int64))


# ------------------------------------------------------------------ 4. model, CLI
def test_model_sample_rebinds_when_the_number_of_forced_words_changes(dev):
    from helpers import build_model, to_dev
    d = synth.CONFIGS["tiny"]
    model = build_model(d, synth.hot_path_state_dict(d, 99), dev, hip_graph=True)
    f, b = to_dev(synth.clip_features(d, 99, full_mask_clip=2), dev), to_dev(synth.label_glue_batch(d, 99), dev)
    s0 = TS._model_sample(model, f, b, beam_size=6)
    e0 = model._engine_cache[1]
    assert not e0.beam_hist and not getattr(e0, "forcing", False)
    s1 = TS._model_sample(model, f, b, beam_size=6, force_words=[5, 7])
    e1 = model._engine_cache[1]
    assert e1 is not e0 and e1.beam_hist and e1.forcing and e1.force_n == 2 and e1.graph is not None
    assert e1.force_words.cpu().tolist() == [[5, 7]] * d.B
    assert s1[2] is None and s1[0].shape == (d.B, d.T) and torch.equal(s1[0], e1.hypotheses(ranked=True)[0][:, 0])
    nm = e1.hypotheses(ranked=True)[3][:, 0]
    for r in range(d.B):
        assert int(nm[r]) == len({5, 7} & set(s1[0][r].tolist()))
    per_clip = torch.tensor([[9, 11], [-1, 13], [15, 9]], device=dev)[:d.B]
    s2 = TS._model_sample(model, f, b, beam_size=6, force_words=per_clip)            # the same C: the cached engine, other words
    assert model._engine_cache[1] is e1 and e1.force_words.cpu().tolist() == per_clip.cpu().tolist()
    assert torch.equal(s2[0], e1.hypotheses(ranked=True)[0][:, 0]) and not torch.equal(s2[0], s1[0])
    TS._model_sample(model, f, b, beam_size=6, force_words=[5])
    e3 = model._engine_cache[1]
    assert e3 is not e1 and e3.force_n == 1
    TS._model_sample(model, f, b, beam_size=6, force_words=[5], no_repeat_ngram=2, length_penalty=0.7)
    e4 = model._engine_cache[1]
    assert e4 is not e3 and e4.forcing and e4.constrained and e4.length_penalty == 0.7
    with pytest.raises(RuntimeError, match="force_n"):
        TS._model_sample(model, f, b, beam_size=6, force_words=[5, 7, 9])           # 6 % 4 != 0
    s6 = TS._model_sample(model, f, b, beam_size=6)
    assert not model._engine_cache[1].beam_hist and torch.equal(s6[0], s0[0]) and torch.equal(bits(s6[1]), bits(s0[1]))


def test_cli_flags_reach_the_engine(dev, tmp_path):
    from cvc import main as cvc_main
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16",
              "--seq_length", "6", "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100",
              "--exp_name", "s", "--learning_rate", "0.001", "--results_dir", str(tmp_path / "results"),
              "--checkpoint_path", str(tmp_path) + "/", "--id", "s1"]
    assert cvc_main.main(common + ["--beam_size", "6", "--force_words", "5,7", "--length_penalty", "0.7"]) == 0
    tr = cvc_main.LAST_TRAINER
    e = getattr(tr.model, "module", tr.model)._engine_cache[1]
    assert e.beam == 6 and e.beam_hist and e.forcing and e.force_n == 2 and e.length_penalty == 0.7
    assert e.force_words.cpu().tolist() == [[5, 7]] * e.B
    seq, score, norm, nmet = e.hypotheses(ranked=True)
    assert seq.shape == (e.B, 6, 6)
    fin = torch.isfinite(norm)
    assert bool((nmet[:, :-1] >= nmet[:, 1:])[fin[:, :-1] & fin[:, 1:]].all())
    # the synthetic dataset's detection classes are no vocabulary words: --force_detected finds nothing to force, bank 0 decodes
    assert cvc_main.main(common + ["--beam_size", "6", "--force_detected", "2"]) == 0
    e = getattr(cvc_main.LAST_TRAINER.model, "module", cvc_main.LAST_TRAINER.model)._engine_cache[1]
    assert e.forcing and e.force_n == 2 and bool((e.force_words == -1).all()) and bool((e.final_nmet == 0).all())
    for bad in (["--force_words", "5,7,9,11"], ["--force_detected", "4"], ["--force_words", "5", "--force_detected", "1"]):
        with pytest.raises(SystemExit):
            cvc_main.main(common + ["--beam_size", "6"] + bad)
