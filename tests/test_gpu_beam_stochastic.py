"""GPU tests (pytest -m gpu) of stochastic beam search: the block cvc_beam_select_stoch_parts (csrc/beam.hip, the STOCH forms of the
row scan and the merge) against the fp64 restatement tests/sbs_ref.py, its statistics on the device, its per-step invariants, and
the engine / model / trainer switches on top of it.  Figures: profiles/beam_stochastic.md.

Tolerances.  ERR_BOUND is the largest |G_out - ref| and |logq_out - ref| MEASURED on the device over the block cases of this file
(printed by every run; profiles/beam_stochastic.md holds the figures); the test asserts 4 x ERR_BOUND (the factor covers the
spread across inputs and compilers) and compares parent / word on every clip-step whose reference margin -- the smallest gap among
the best beam + 1 keys -- exceeds DELTA = 2 x ERR_BOUND.  The share of clip-steps under DELTA is asserted <= 2 % on the reference
alone, before the kernel's output is looked at."""
import functools

import numpy as np
import pytest
import torch

from cvc import synth
import sbs_ref as S
import sample_oracle as SO
import test_gpu_tile_path as TP               # P(), st(), the sentinels
from tile_path_cases import SCORE_TOL, nan_buf

pytestmark = pytest.mark.gpu

BADARG, TOOBIG = -1, -2
ERR_BOUND = 1.03e-5                           # measured: profiles/beam_stochastic.md
G_TOL = 4 * ERR_BOUND
DELTA = 2 * ERR_BOUND
assert G_TOL <= 1e-4
T_HIST = 8
UNK = 1


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def rng_state(seed, call, dev):
    lo, hi = SO.seed_words(seed)
    return torch.from_numpy(np.array([lo, hi, call, 0], dtype=np.uint32).view(np.int32)).to(dev)


def stoch_launch(dev, parts, stride, nparts, bias, score, done, B, beam, V, unk, t, hin, hout, hs, desc, inv_tau, state, logq, G, outs):
    """the raw call; outs = (parent, word, score_out, done_out, logq_out, G_out, nbanned, ws) device tensors or None"""
    from cvc import hip
    p = lambda x: None if x is None else x.data_ptr()
    return hip.lib().cvc_beam_select_stoch_parts(p(parts), nparts, stride, p(bias), p(score), p(done), B, beam, V, unk, t, p(hin), p(hout), hs,
                                                 desc, inv_tau, p(state), p(logq), p(G), *(p(o) for o in outs), TP.st())


def constraint(rules, dev):
    from cvc import hip
    i32 = lambda ids: torch.tensor(list(ids) or [0], dtype=torch.int32, device=dev)
    ban, bad = list(rules.get("ban_words", ())), list(rules.get("bad_endings", ()))
    ban_d, bad_d = i32(ban), i32(bad)
    return hip.Constraint(int(rules.get("no_repeat_ngram", 0)), int(bool(rules.get("no_immediate_repeat", False))),
                          int(rules.get("min_len", 0)), len(ban), ban_d.data_ptr(), bad_d.data_ptr(), len(bad)), (ban_d, bad_d)


# ------------------------------------------------------------------ 1. the block against the reference
STEPS = ["t0", "mid", "rules"]
LOADERS = [(1, False), (1, True), (3, False), (3, True)]        # (nparts, bias)
EXTRA = [(5, 4100, 6, True), (8, 1024, 2, False), (5, 8192, 8, True)]      # fused slabs (NP = 6, 2, 8; NG = 5, 1, 8), beyond the base table


@functools.lru_cache(maxsize=None)
def block_case(B, beam, V, nparts, bias, step):
    """N(0, 3) logits as nparts slabs (+ bias) whose fp32 sum in the loader's order is z; the state of the step"""
    g = torch.Generator().manual_seed(1000 * beam + V + 7 * nparts + (3 if bias else 0) + {"t0": 0, "mid": 50000, "rules": 90000}[step])
    rows = B * beam
    parts = torch.randn(nparts, rows, V, generator=g) * (3.0 / np.sqrt(nparts + (1 if bias else 0)))
    bias_v = torch.randn(V, generator=g) * (3.0 / np.sqrt(nparts + 1)) if bias else None
    z = parts[0].clone()
    for p in range(1, nparts):
        z = z + parts[p]
    if bias_v is not None:
        z = z + bias_v
    t = {"t0": 0, "mid": 3, "rules": 4}[step]
    score = torch.zeros(rows)
    logq = torch.zeros(rows)
    G = torch.zeros(rows)
    done = torch.zeros(rows, dtype=torch.uint8)
    pool = [0, 2, 3, min(5, V - 1), V - 1]
    hist = np.zeros((T_HIST, rows), dtype=np.int64)
    rules = {}
    if t > 0:
        hist[:t] = np.array(pool)[torch.randint(1, len(pool), (t, rows), generator=g).numpy()]
        hist[0] = 6 + np.arange(rows) % beam                  # the rows of a clip enter with pairwise distinct histories
        score = -(torch.rand(rows, generator=g) * 8 + 2) * t
        logq = -(torch.rand(rows, generator=g) * 6 + 1) * t
        # a reachable state: a row's key is its sampling log-prob plus Gumbel noise (G = max of g over the row's step, g = phi +
        # gumbel), so G - logq = O(1).  Keys far above logq + noise never occur in a search, and there the conditioning
        # exp(-G) - exp(-Z) + exp(-g) cancels catastrophically whatever the arithmetic: the measured bound would be the inputs'.
        u = torch.rand(rows, generator=g).clamp(1e-6, 1 - 1e-6)
        G = logq - torch.log(-torch.log(u))
        order = (torch.argsort(G.view(B, beam), 1, descending=True) + torch.arange(B).view(-1, 1) * beam).view(-1)      # draw order
        score, logq, G = score[order].contiguous(), logq[order].contiguous(), G[order].contiguous()
    if step == "mid":                         # per clip: one frozen row (its history ends in 0) and one row at -inf
        for b in range(B):
            kf, ki = (b % beam), ((b + 1) % beam)
            done[b * beam + kf] = 1
            hist[t - 1, b * beam + kf] = 0
            for a in (score, logq, G):
                a[b * beam + ki] = -float("inf")
    if step == "rules":
        rules = dict(no_repeat_ngram=2, min_len=t + 2)
    return dict(B=B, beam=beam, V=V, nparts=nparts, parts=parts, bias=bias_v, z=z, t=t, score=score, logq=logq, G=G, done=done,
                hist=hist, rules=rules)


def run_block(c, dev, tau, seed, call):
    B, beam, V, nparts, t = c["B"], c["beam"], c["V"], c["nparts"], c["t"]
    rows = B * beam
    stride = rows * V + 4 * 3                                   # a multiple of 4 past the slab: the fused forms stay aligned
    buf = nan_buf(nparts * stride + 8, dev=dev)
    for p in range(nparts):
        buf[p * stride:p * stride + rows * V] = c["parts"][p].reshape(-1).to(dev)
    bias = None if c["bias"] is None else c["bias"].to(dev)
    hin = torch.full((T_HIST, rows), TP.SENT, dtype=torch.int64, device=dev)
    hin[:] = torch.from_numpy(c["hist"]).to(dev)
    hout = torch.full((T_HIST, rows), TP.SENT, dtype=torch.int64, device=dev)
    outs = (torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev), torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev),
            nan_buf(rows, dev=dev), torch.full((rows,), TP.DONE_FILL, dtype=torch.uint8, device=dev), nan_buf(rows, dev=dev),
            nan_buf(rows, dev=dev), torch.full((rows,), TP.SENT, dtype=torch.int32, device=dev), nan_buf(26 * rows, dev=dev))
    desc, keep = constraint(c["rules"], dev)
    state = rng_state(seed, call, dev)
    rc = stoch_launch(dev, buf, stride, nparts, bias, c["score"].to(dev), c["done"].to(dev), B, beam, V, UNK, t, hin, hout, rows,
                      desc if c["rules"] else None, 1.0 / tau, state, c["logq"].to(dev), c["G"].to(dev), outs)
    torch.cuda.synchronize()
    return rc, [o.cpu() for o in outs], hout.cpu().numpy()


def reference(c, tau, seed, call):
    rows = c["B"] * c["beam"]
    return S.step(c["z"].numpy(), c["score"].numpy(), c["logq"].numpy(), c["G"].numpy(), c["done"].numpy(), c["hist"].T, c["t"], c["B"],
                  c["beam"], UNK, tau, S.noise(seed, call, c["t"], rows, c["V"]), **c["rules"])


def check_invariants(label, c, parent, word, score, logq, G, hist_out):
    """G_out <= G_in[parent]; slots non-increasing in G; finite slots of a clip pairwise distinct; no NaN"""
    B, beam, t = c["B"], c["beam"], c["t"]
    for name, a in (("score_out", score), ("logq_out", logq), ("G_out", G)):
        assert not bool(torch.isnan(a).any()), f"{label}: NaN in {name}"
    Gin = c["G"].view(B, beam).clone()
    if t == 0:
        Gin[:, 1:] = -float("inf")
    assert bool((G.view(B, beam) <= Gin.gather(1, parent.view(B, beam))).all()), f"{label}: a child's key exceeds its parent's"
    assert bool((G.view(B, beam)[:, 1:] <= G.view(B, beam)[:, :-1]).all()), f"{label}: slots are not in draw order"
    h = hist_out[:t + 1].T.reshape(B, beam, t + 1)
    fin = torch.isfinite(G).view(B, beam).numpy()
    for b in range(B):
        live = [tuple(h[b, k]) for k in range(beam) if fin[b, k]]
        assert len(set(live)) == len(live), f"{label}: clip {b} holds a caption twice"


def check_block(label, c, tau, seed, call, dev, errs):
    B, beam, V, t = c["B"], c["beam"], c["V"], c["t"]
    rows = B * beam
    r = reference(c, tau, seed, call)
    for k in ("score", "logq", "G"):
        assert not np.isnan(r[k]).any(), f"{label}: the reference yields NaN"
    sure = r["margin"] > DELTA                                   # judged on the reference alone
    rc, (parent, word, score, done, logq, G, nb, ws), hout = run_block(c, dev, tau, seed, call)
    assert rc == 0, (label, rc)
    assert bool(((parent >= 0) & (parent < beam) & (word >= 0) & (word < V)).all()), f"{label}: parent / word out of range"
    check_invariants(label, c, parent, word, score, logq, G, hout)
    pa, wo = parent.view(B, beam).numpy(), word.view(B, beam).numpy()
    live = r["live"] & sure[:, None]
    assert np.array_equal(pa[live], r["parent"][live]) and np.array_equal(wo[live], r["word"][live]), f"{label}: parent / word"
    assert np.array_equal(done.view(B, beam).numpy()[live].astype(bool), r["done"][live]), f"{label}: done"
    f64 = lambda a: a.view(B, beam).double().numpy()
    for name, got, want in (("G_out", f64(G), r["G"]), ("logq_out", f64(logq), r["logq"])):
        err = float(np.abs(got[live] - want[live]).max()) if live.any() else 0.0
        errs.append(err)
        assert err <= G_TOL, f"{label}: {name} off by {err:.3e} > {G_TOL:.1e}"
    torch.testing.assert_close(score.view(B, beam)[torch.from_numpy(live)], torch.from_numpy(r["score"][live]).float(), **SCORE_TOL)
    # score_out: the history block's candidate expression on the scan's own lse (workspace: 16 floats of candidates per row, then lse)
    lse = ws[16 * rows:17 * rows]
    k_abs = (parent.view(B, beam) + torch.arange(B).view(-1, 1) * beam).view(-1)
    cand = c["score"][k_abs] + (c["z"][k_abs, word] - lse[k_abs])
    cand = torch.where(c["done"][k_abs].bool(), c["score"][k_abs], cand)
    fin = torch.isfinite(G)
    assert torch.equal(score[fin].view(torch.int32), cand[fin].view(torch.int32)), f"{label}: score_out is not the history block's bits"
    dead = ~r["live"] & sure[:, None]
    for a in (score, logq, G):
        assert bool((a.view(B, beam)[torch.from_numpy(dead)] == -float("inf")).all()), f"{label}: a filler is not -inf"
    assert np.array_equal(nb.numpy(), r["nbanned"]), f"{label}: nbanned"
    src = (pa + np.arange(B)[:, None] * beam).reshape(-1)
    assert np.array_equal(hout[:t], c["hist"][:t][:, src]) and np.array_equal(hout[t], wo.reshape(-1)), f"{label}: histories"
    assert (hout[t + 1:] == TP.SENT).all(), f"{label}: wrote past step t"
    lv = live.reshape(-1)
    assert np.array_equal(hout[:t + 1][:, lv], r["hist"].T[:, lv]), f"{label}: history against the reference"
    return r, (parent, word, score, done, logq, G)


def all_block_cases(beam, V):
    for nparts, bias in LOADERS:
        for step in STEPS:
            yield block_case(3, beam, V, nparts, bias, step), f"beam{beam} V{V} np{nparts} bias{int(bias)} {step}"


def test_margins_leave_at_most_two_percent_of_the_clip_steps_out():
    """on the reference alone, over every case of this file (the share is re-checked for the inputs actually used)"""
    skipped = total = 0
    for beam in (2, 5, 8):
        for V in (37, 1024, 4100):
            for c, label in all_block_cases(beam, V):
                for tau in (1.0, 0.7):
                    r = reference(c, tau, 11, 2)
                    skipped += int((r["margin"] <= DELTA).sum())
                    total += c["B"]
    print(f"margin <= {DELTA:.1e}: {skipped} of {total} clip-steps")
    assert skipped <= 0.02 * total, (skipped, total)


@pytest.mark.parametrize("V", [37, 1024, 4100])
@pytest.mark.parametrize("beam", [2, 5, 8])
def test_block_vs_reference(dev, beam, V):
    errs = []
    for c, label in all_block_cases(beam, V):
        for tau in (1.0, 0.7):
            check_block(f"{label} tau{tau}", c, tau, 11, 2, dev, errs)
    print(f"beam {beam} V {V}: max |G_out - ref|, |logq_out - ref| = {max(errs):.3e}")


@pytest.mark.parametrize("beam,V,nparts,bias", EXTRA)
def test_block_vs_reference_on_the_fused_slab_forms(dev, beam, V, nparts, bias):
    errs = []
    for step in STEPS:
        check_block(f"beam{beam} V{V} np{nparts} {step}", block_case(3, beam, V, nparts, bias, step), 0.7, 5, 9, dev, errs)
    print(f"fused beam {beam} V {V} np {nparts}: max error = {max(errs):.3e}")


def test_the_block_is_deterministic_and_the_call_counter_changes_the_draw(dev):
    c = block_case(3, 5, 1024, 1, False, "mid")
    a = run_block(c, dev, 1.0, 3, 1)[1]
    b = run_block(c, dev, 1.0, 3, 1)[1]
    d = run_block(c, dev, 1.0, 3, 2)[1]
    for x, y in zip(a[:7], b[:7]):
        assert torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)
    assert not torch.equal(a[1], d[1]), "another call counter drew the same words"


def test_all_banned_rows_and_refusals(dev):
    """a step whose every word is banned (min_len bans 0, the list bans the rest): fillers at -inf, no NaN; then every refusal"""
    c = dict(block_case(3, 2, 37, 1, False, "rules"))
    c["rules"] = dict(ban_words=list(range(37)))
    rc, (parent, word, score, done, logq, G, nb, ws), hout = run_block(c, dev, 1.0, 1, 1)
    assert rc == 0
    for a in (score, logq, G):
        assert bool((a == -float("inf")).all()), a
    assert bool((nb == 37).all())
    B, beam, V = 3, 2, 37
    rows = B * beam
    z = lambda *s: torch.zeros(*s, device=dev)
    zi = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt, device=dev)
    buf, sc, lq, G_in, dn = z(rows * V), z(rows), z(rows), z(rows), zi(rows, dt=torch.uint8)
    hin, ho = zi(T_HIST, rows), torch.full((T_HIST, rows), TP.SENT, dtype=torch.int64, device=dev)
    state = rng_state(1, 1, dev)

    def call(inv_tau=1.0, st=state, lq_in=lq, g_in=G_in, outs=None, t=1):
        o = [torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev), torch.full((rows,), TP.SENT, dtype=torch.int64, device=dev),
             nan_buf(rows, dev=dev), torch.full((rows,), TP.DONE_FILL, dtype=torch.uint8, device=dev), nan_buf(rows, dev=dev),
             nan_buf(rows, dev=dev), torch.full((rows,), TP.SENT, dtype=torch.int32, device=dev), nan_buf(26 * rows, dev=dev)]
        for i, v in (outs or {}).items():
            o[i] = v
        rc = stoch_launch(dev, buf, rows * V, 1, None, sc, dn, B, beam, V, UNK, t, hin, ho, rows, None, inv_tau, st, lq_in, g_in, o)
        torch.cuda.synchronize()
        clean = all(bool(torch.isnan(x).all()) if x.is_floating_point() else bool((x == (TP.DONE_FILL if x.dtype == torch.uint8 else TP.SENT)).all())
                    for x in o[:7] if x is not None and x.data_ptr() not in (lq_in.data_ptr(), g_in.data_ptr(), sc.data_ptr()))
        return rc, clean and bool((ho == TP.SENT).all())

    assert call() == (0, False)                                  # the accepted call writes
    ho.fill_(TP.SENT)
    for kw in (dict(inv_tau=0.0), dict(inv_tau=-1.0), dict(inv_tau=float("inf")), dict(inv_tau=float("nan")), dict(st=None),
               dict(lq_in=None), dict(g_in=None), dict(outs={4: None}), dict(outs={5: None}), dict(outs={4: lq}), dict(outs={5: G_in}),
               dict(outs={2: sc})):
        if kw.get("lq_in", 0) is None or kw.get("g_in", 0) is None:
            o = [zi(rows), zi(rows), z(rows), zi(rows, dt=torch.uint8), z(rows), z(rows), zi(rows, dt=torch.int32), z(26 * rows)]
            rc = stoch_launch(dev, buf, rows * V, 1, None, sc, dn, B, beam, V, UNK, 1, hin, ho, rows, None, 1.0, state,
                              kw.get("lq_in", lq), kw.get("g_in", G_in), o)
            assert rc == BADARG, kw
            continue
        assert call(**kw) == (BADARG, True), kw
    assert call(t=65) == (TOOBIG, True)


# ------------------------------------------------------------------ 2. statistics on the device: the toy through the block
@pytest.mark.parametrize("tau", [1.0, 0.7])
def test_toy_statistics_on_the_device(dev, tau):
    """V = 5 with UNK, T = 3, beam 3, one clip per trial, 4 launches of 12 800 clips; logits gathered between the steps from a table
    by the row's last word.  Slot 0 against p(a), the ordered pair (slot 0, slot 1) against p(a) p(b) / (1 - p(a))."""
    V, T, beam, unk, B, launches = 5, 3, 3, 3, 12800, 4
    table = S.toy_table(V, T, 11)
    tab = torch.from_numpy(table).float().to(dev)
    rows = B * beam
    hists = []
    for n in range(launches):
        state = rng_state(77, n + 1, dev)
        score, logq, G = [torch.zeros(2, rows, device=dev) for _ in range(3)]
        done = torch.zeros(2, rows, dtype=torch.uint8, device=dev)
        hist = torch.zeros(2, T, rows, dtype=torch.int64, device=dev)
        parent, word = torch.zeros(rows, dtype=torch.int64, device=dev), torch.zeros(rows, dtype=torch.int64, device=dev)
        ws = torch.zeros(26 * rows, device=dev)
        for t in range(T):
            rd, wr = t & 1, (t + 1) & 1
            last = hist[rd][t - 1] + 1 if t else torch.zeros(rows, dtype=torch.int64, device=dev)
            z = tab[t][last].contiguous()
            rc = stoch_launch(dev, z, 0, 1, None, score[rd], done[rd], B, beam, V, unk, t, hist[rd], hist[wr], rows, None, 1.0 / tau,
                              state, logq[rd], G[rd], (parent, word, score[wr], done[wr], logq[wr], G[wr], None, ws))
            assert rc == 0
            Gin = G[rd].view(B, beam).clone()
            if t == 0:
                Gin[:, 1:] = -float("inf")
            Go = G[wr].view(B, beam)
            assert not bool(torch.isnan(Go).any()) and bool((Go <= Gin.gather(1, parent.view(B, beam))).all())
            assert bool((Go[:, 1:] <= Go[:, :-1]).all())
        assert bool(torch.isfinite(G[T & 1]).all())             # 40 captions >= 3 slots: every slot is live
        hists.append(hist[T & 1].permute(1, 0).reshape(B, beam, T).cpu().numpy())
    h = np.concatenate(hists, 0)
    assert (h[:, 0] != h[:, 1]).any(1).all() and (h[:, 0] != h[:, 2]).any(1).all() and (h[:, 1] != h[:, 2]).any(1).all()
    seqs, probs = S.toy_sequences(table, tau, unk)
    (c1, d1), (c2, d2) = S.toy_chi_squares(h, seqs, probs)
    print(f"tau {tau}: slot 0 chi2 {c1:.1f} (df {d1}, critical {SO.chi_square_critical(d1):.1f}); pair chi2 {c2:.1f} (df {d2}, "
          f"critical {SO.chi_square_critical(d2):.1f})")
    assert c1 < SO.chi_square_critical(d1), (c1, d1)
    assert c2 < SO.chi_square_critical(d2), (c2, d2)


# ------------------------------------------------------------------ 3. the engine
# The engine's logits are the GPU model's (split-product GEMMs) and the reference's the CPU oracle's: a clip is compared where every
# step's reference margin exceeds ENGINE_MARGIN, and scores, keys and log-probs at ENGINE_TOL -- the margin and the score tolerance
# of the history engine's test against its reference decoder (tests/test_gpu_beam_constrained.py: MARGIN_MIN, atol 2e-4).
ENGINE_MARGIN = 2e-4
ENGINE_TOL = 2e-4
ENGINE_CASES = [("tiny", 3, "tile", 1.0, {}), ("tiny", 3, "ring", 0.7, {}), ("cfg1", 5, "tile", 0.7, dict(no_repeat_ngram=2, min_len=2)),
                ("cfg1", 5, "ring", 1.0, {}), ("cfg1", 2, "tile", 1.0, dict(no_immediate_repeat=True, ban_words=[3], bad_endings=[4]))]
SEED = 20


def _engine(dev, name, beam, path, tau, seed=SEED, **kw):
    import test_gpu_sampling as TS
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, P, f = TS._inputs(name)
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, synth.UNK_IDX, beam=beam, path=path, beam_history=True,
                       stochastic=True, stochastic_tau=tau, seed=seed, **kw)
    assert eng.tile == (path == "tile") and not eng.packed and eng.stoch and eng._plan is None
    return d, P, f, eng


@functools.lru_cache(maxsize=None)
def _ref_decode(name, beam, tau, call, rules_key=()):
    import test_gpu_sampling as TS
    d, sd, f_np, P, f = TS._inputs(name)
    with torch.no_grad():
        return S.decode(P, f, d.T, synth.UNK_IDX, beam, tau, SEED, call, **dict(rules_key))


def _check_engine(label, d, eng, ref, beam):
    seq, score, G, logq = (x.cpu() for x in eng.hypotheses())
    assert seq.shape == (d.B, beam, d.T) and score.shape == G.shape == logq.shape == (d.B, beam)
    assert not bool(torch.isnan(G).any() | torch.isnan(score).any() | torch.isnan(logq).any())
    assert bool((G[:, 1:] <= G[:, :-1]).all()), f"{label}: slots are not in draw order"
    for b in range(d.B):
        live = [tuple(h) for h, g in zip(seq[b].tolist(), G[b].tolist()) if np.isfinite(g)]
        assert len(set(live)) == len(live) and all(synth.UNK_IDX not in h for h in live), f"{label}: clip {b}"
    sure = ref["margin"].min(1) > ENGINE_MARGIN
    print(f"{label}: {int(sure.sum())} of {d.B} clips above the margin, smallest margin {ref['margin'].min():.2e}")
    assert sure.any(), f"{label}: no clip is comparable"
    assert np.array_equal(seq.numpy()[sure], ref["seq"][sure]), f"{label}: captions"
    m = ref["live"] & sure[:, None]
    for name, got, want in (("score", score, ref["score"]), ("G", G, ref["G"]), ("logq", logq, ref["logq"])):
        err = float(np.abs(got.double().numpy()[m] - want[m]).max())
        assert err <= ENGINE_TOL, f"{label}: {name} off by {err:.2e}"
    return sure


@pytest.mark.parametrize("name,beam,path,tau,rules", ENGINE_CASES)
def test_engine_vs_reference_decoder(dev, name, beam, path, tau, rules):
    from cvc import hip
    d, P, f, eng = _engine(dev, name, beam, path, tau, **rules)
    sel = [fn for nm, fn, _ in eng._python_launches() if nm == "word_select"]
    assert len(sel) == d.T and all(fn is hip.lib().cvc_beam_select_stoch_parts for fn in sel)
    assert eng._python_launches()[0][0] == "sample_advance"
    seq0, att0, score0 = eng.run()
    ref = _ref_decode(name, beam, tau, 1, tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in rules.items())))
    sure = _check_engine(f"{name} beam {beam} {path} tau {tau} {rules}", d, eng, ref, beam)
    hyp = eng.hypotheses()
    assert torch.equal(seq0, hyp[0][:, 0]) and torch.equal(score0.view(torch.int32), hyp[1].view(torch.int32))      # run() returns slot 0
    if rules:
        assert np.array_equal(eng.nbanned.cpu().numpy()[:, np.repeat(sure, beam)], ref["nbanned"][:, np.repeat(sure, beam)])
    with pytest.raises(RuntimeError, match="draw order"):
        eng.hypotheses(ranked=True)


@pytest.mark.parametrize("name,beam,path", [("tiny", 3, "tile"), ("cfg1", 5, "ring")])
def test_a_captured_graph_draws_afresh_and_a_rebuilt_engine_repeats(dev, name, beam, path):
    import test_gpu_sampling as TS
    from helpers import to_dev
    d, P, f, eng = _engine(dev, name, beam, path, 1.0, own_features=True)
    eng.capture()
    assert eng.graph is not None
    draws = []
    for call in (1, 2):
        eng.run()
        _check_engine(f"{name} {path} replay {call}", d, eng, _ref_decode(name, beam, 1.0, call), beam)
        draws.append([x.clone() for x in eng.hypotheses()])
    assert not torch.equal(draws[0][0], draws[1][0]), "two replays drew the same captions"
    d, P, f, again = _engine(dev, name, beam, path, 1.0)
    again.run()
    for a, b in zip(draws[0], again.hypotheses()):
        assert torch.equal(a.view(torch.int32) if a.is_floating_point() else a, b.view(torch.int32) if b.is_floating_point() else b)
    # the graph serves a new batch, and the first batch again under a re-seeded state repeats the first draw
    eng.load_features(to_dev(synth.clip_features(d, 777), dev))
    eng.run()
    assert not torch.equal(eng.hypotheses()[0], draws[0][0])
    eng.load_features(to_dev(TS._inputs(name)[2], dev))
    eng.seed(SEED)
    eng.run()
    assert torch.equal(eng.hypotheses()[0], draws[0][0]) and torch.equal(eng.hypotheses()[2].view(torch.int32), draws[0][2].view(torch.int32))


def test_consensus_and_model_sample(dev):
    import test_gpu_sampling as TS
    import test_gpu_consensus_decode as CD
    d, model, f, b = CD._model(dev, graph=True)
    table = model.consensus_table = CD._table(d, dev)
    plain = TS._model_sample(model, f, b, beam_size=4)
    assert not model._engine_cache[1].beam_hist                  # every switch off: the plain beam engine
    s = TS._model_sample(model, f, b, beam_size=4, stochastic_beam=True, stochastic_tau=0.9, seed=5)
    e = model._engine_cache[1]
    assert e.stoch and e.beam_hist and e.graph is not None and s[2] is None and s[0].shape == (d.B, d.T)
    last = model.last_stochastic
    assert last["seq"].shape == (d.B, 4, d.T) and torch.equal(last["seq"][:, 0], s[0])
    assert bool((last["G"][:, 1:] <= last["G"][:, :-1]).all()) and bool((last["logq"] <= 0).all())
    for hyps in last["seq"].tolist():
        assert len({tuple(h) for h in hyps}) == 4
    s2 = TS._model_sample(model, f, b, beam_size=4, stochastic_beam=True, stochastic_tau=0.9, seed=5)     # cached engine: fresh noise
    assert model._engine_cache[1] is e and not torch.equal(model.last_stochastic["seq"], last["seq"])
    # consensus over the distinct samples: the engine's pick is the table's over hypotheses(), fillers not live
    seq_c, att_c, none_c = TS._model_sample(model, f, b, beam_size=4, stochastic_beam=True, stochastic_tau=0.9, seed=5, consensus="beam")
    e2 = model._engine_cache[1]
    hyp = e2.hypotheses()
    u, p, best = table.consensus(hyp[0].reshape(d.B * 4, d.T).contiguous(), 4, live=torch.isfinite(hyp[1]).reshape(-1))
    assert none_c is None and torch.equal(seq_c, best) and torch.equal(model.last_consensus["pick"], p)
    after = TS._model_sample(model, f, b, beam_size=4)
    assert torch.equal(after[0], plain[0]) and torch.equal(after[1].view(torch.int32), plain[1].view(torch.int32))


def test_trainer_sample_without_replacement_writes_n_distinct_captions(dev, tmp_path):
    import json
    from cvc import main as cvc_main
    from cvc import sample as cvc_sample
    common = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "8", "--num_prop_per_frm", "7",
              "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16",
              "--seq_length", "4", "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "100",
              "--exp_name", "s", "--learning_rate", "0.001", "--results_dir", str(tmp_path / "results"),
              "--checkpoint_path", str(tmp_path) + "/", "--id", "s1"]
    assert cvc_main.main(common + ["--beam_size", "3", "--stochastic_beam", "--stochastic_tau", "0.9", "--sample_seed", "2"]) == 0
    tr = cvc_main.LAST_TRAINER
    e = getattr(tr.model, "module", tr.model)._engine_cache[1]
    assert e.stoch and e.beam == 3 and abs(e.stoch_inv_tau - 1 / 0.9) < 1e-12
    path = tr.sample(3, 0.8, seed=4, without_replacement=True)
    out = json.load(open(path))
    assert len(out) == 8
    for segs in out.values():
        for e in segs:
            assert len(e["sentences"]) == 3 and len(e["logprobs"]) == 3 and len(e["logq"]) == 3 and len(e["G"]) == 3
            assert all(a >= b for a, b in zip(e["G"], e["G"][1:])) and all(lp <= 0 for lp in e["logprobs"] + e["logq"])
    seqs = getattr(tr.model, "module", tr.model).last_stochastic["seq"]
    for hyps in seqs.tolist():
        assert len({tuple(h) for h in hyps}) == 3
    with pytest.raises(RuntimeError, match="top_k / top_p"):
        tr.sample(3, 0.8, seed=4, without_replacement=True, top_k=5)
    assert cvc_sample.main(common + ["--resume", "True", "--temperature", "0.8", "--sample_n", "2", "--sample_seed", "4",
                                     "--without_replacement"]) == 0
    out2 = json.load(open(path))
    assert len(out2) == 8 and all(len(e["sentences"]) == 2 and len(e["G"]) == 2 for segs in out2.values() for e in segs)
