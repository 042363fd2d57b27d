"""Teacher-forced decode on the GPU (pytest -m gpu): the selection block (csrc/forced.hip) against tests/forced_ref.py and, on the
words they draw, against the sampling blocks bit for bit (one row loader: csrc/select_row.h), the engine's three paths against the CPU oracle over given words, graph replay across caption sets, consistency with the greedy engine, the
frame-masked output against the oracle's training pass, and the model / trainer plumbing."""
import functools
import json

import numpy as np
import pytest
import torch

from cvc import synth
import forced_ref as FR
import test_gpu_sampling as TS               # the plain sampling block's launcher, the generator state
import test_gpu_sampling_trunc as TT         # the truncating block's launcher
from test_gpu_sampling import SEQ_TOL, LOGPROB_TOL

pytestmark = pytest.mark.gpu

BADARG, TOOBIG = -1, -2
BLOCK_TOL = 2e-6                          # log-prob of the block against fp64 (tests/test_gpu_sampling_trunc.py, same quantity)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    from cvc import hip
    hip.lib()
    return torch.device("cuda:0")


def bits(x):
    return x.view(torch.int32) if x.is_floating_point() else x


def forced_block(parts, bias, words, V, logprob=True, rank=True, M=None, nparts=None, stride=None, word_stride=1):
    from cvc import hip
    nparts = parts.shape[0] if nparts is None else nparts
    M = parts.shape[1] if M is None else M
    lp = torch.full((max(M, 1),), 7.0, device=parts.device) if logprob else None
    rk = torch.full((max(M, 1),), -7, dtype=torch.int32, device=parts.device) if rank else None
    rc = hip.lib().cvc_forced_select_parts(parts.data_ptr(), nparts, M * V if stride is None else stride,
                                           None if bias is None else bias.data_ptr(), M, V,
                                           None if words is None else words.data_ptr(), word_stride,
                                           None if lp is None else lp.data_ptr(), None if rk is None else rk.data_ptr(), hip._stream())
    return rc, lp, rk


# ------------------------------------------------------------------ the selection block against the reference
NCASE = 10


@pytest.mark.parametrize("M,V,nparts,with_bias", [(1, 50, 1, False), (3, 33, 2, True), (64, 50, 4, True), (65, 500, 6, True),
                                                  (64, 5000, 1, False), (64, 5000, 6, True), (2, 8192, 8, True)])
def test_forced_block_vs_reference(dev, M, V, nparts, with_bias):
    unk = synth.UNK_IDX
    g = torch.Generator().manual_seed(M * 131 + V + nparts)
    parts = torch.randn(nparts, M, V, generator=g) * (1.5 / np.sqrt(nparts))
    bias = torch.randn(V, generator=g) * 0.3 if with_bias else None
    LO, MID, HI = 3, 10, 20                              # the tie columns: equal bias, so equal slabs give equal logits
    if bias is not None:
        bias[LO] = bias[HI] = bias[MID]
    words = torch.randint(0, V, (M,), generator=g, dtype=torch.int64)
    case_of = [(r + M) % NCASE for r in range(M)]        # every case occurs at M >= 10; the small shapes take what fits
    z0 = FR.finished(parts, bias)
    for r, c in enumerate(case_of):
        if c == 0:                                       # the arg-max itself
            words[r] = int(z0[r].argmax())
        elif c == 1:                                     # an exact duplicate of z[w] at a LOWER index: counted
            parts[:, r, LO] = parts[:, r, MID]
            words[r] = MID
        elif c == 2:                                     # ... at a HIGHER index: not counted
            parts[:, r, HI] = parts[:, r, MID]
            words[r] = MID
        elif c == 3:
            words[r] = V - 1
        elif c == 4:
            words[r] = 0
        elif c == 5:                                     # UNK holds the largest logit and is the given word: rank 0, not suppressed
            parts[0, r, unk] += 60.0
            words[r] = unk
        elif c == 6:
            words[r] = V
        elif c == 7:
            words[r] = -1
        elif c == 8:                                     # a NaN logit elsewhere in the row
            parts[0, r, (int(words[r]) + 1) % V] = float("nan")
    z = FR.finished(parts, bias)
    lp_ref, rk_ref = FR.forced_select(z, words.numpy())
    # the planted rows say what they were planted for (checks of the reference's inputs, brute force)
    zn = z.numpy()
    for r, c in enumerate(case_of):
        w = int(words[r])
        if c in (0, 5):
            assert rk_ref[r] == 0 and w == int(np.nanargmax(zn[r]))
        elif c == 1:
            assert zn[r, LO] == zn[r, MID] and rk_ref[r] == int((zn[r] > zn[r, MID]).sum()) + 1
        elif c == 2:
            assert zn[r, HI] == zn[r, MID] and rk_ref[r] == int((zn[r] > zn[r, MID]).sum()) + int(zn[r, LO] == zn[r, MID])
        elif c in (6, 7):
            assert rk_ref[r] == -1 and np.isnan(lp_ref[r])
        elif c == 8:
            assert np.isnan(lp_ref[r]) and rk_ref[r] >= 0

    pd_, bd, wd = parts.contiguous().to(dev), None if bias is None else bias.to(dev), words.to(dev)
    rc, lp, rk = forced_block(pd_, bd, wd, V)
    assert rc == 0
    assert np.array_equal(rk.cpu().numpy(), rk_ref), (rk.cpu().numpy(), rk_ref)              # every row, exact
    np.testing.assert_allclose(lp.cpu().double().numpy(), lp_ref, rtol=0, atol=BLOCK_TOL, equal_nan=True)
    assert torch.equal(wd.cpu(), words)                                                       # the block writes no word
    # bitwise deterministic run to run; the finished-matrix form (nparts = 1, no bias) gives the same bits
    rc2, lp2, rk2 = forced_block(pd_, bd, wd, V)
    assert rc2 == 0 and torch.equal(bits(lp), bits(lp2)) and torch.equal(rk, rk2)
    rc3, lp3, rk3 = forced_block(z.to(dev).unsqueeze(0).contiguous(), None, wd, V)
    assert rc3 == 0 and torch.equal(bits(lp), bits(lp3)) and torch.equal(rk, rk3)
    # nullable outputs
    rc4, lp4, none4 = forced_block(pd_, bd, wd, V, rank=False)
    rc5, none5, rk5 = forced_block(pd_, bd, wd, V, logprob=False)
    assert rc4 == 0 and rc5 == 0 and none4 is None and none5 is None
    assert torch.equal(bits(lp), bits(lp4)) and torch.equal(rk, rk5)


# ------------------------------------------------------------------ one row loader for every selection block
@pytest.mark.parametrize("M,V,nparts,with_bias", [(3, 33, 2, True),         # scalar loads, 1 logit per thread
                                                  (64, 52, 2, True),        # float4, 2 unrolled slabs
                                                  (5, 5000, 6, True),       # float4, 5 groups, 6 unrolled slabs: the production V
                                                  (64, 4999, 1, False),     # scalar loads, 20 logits per thread
                                                  (33, 8192, 3, True)])     # float4, 8 groups, run-time slab loop
def test_forced_logprob_of_a_drawn_word_is_the_sampling_blocks_bit_for_bit(dev, M, V, nparts, with_bias):
    """the forced block, given the word a sampling block drew, returns that block's log-prob bit for bit on every row: the same
    logits (slab sum in the same order), the same log-sum-exp terms in the same order.  UNK holds the row maximum on every third
    row: out of the samplers' candidates, inside every log-sum-exp."""
    unk, inv_tau, t = synth.UNK_IDX, float(np.float32(1.0 / 0.7)), 5
    g = torch.Generator().manual_seed(M * 131 + V + nparts + 11)
    parts = torch.randn(nparts, M, V, generator=g) * (1.5 / np.sqrt(nparts))
    bias = torch.randn(V, generator=g) * 0.3 if with_bias else None
    parts[0, 0::3, unk] += 60.0
    z = FR.finished(parts, bias)
    assert (z[0::3].argmax(1) == unk).all()
    pd_, bd = parts.contiguous().to(dev), None if bias is None else bias.to(dev)
    state = TS.state_words(12345 + M + V, 3).to(dev)
    w_plain, lp_plain = TS.select_block(pd_, bd, V, unk, inv_tau, state, t)
    w_trunc, lp_trunc, _, _ = TT.trunc_block(pd_, bd, V, unk, inv_tau, 40, 0.9, state, t)
    for label, w, lp in (("plain", w_plain, lp_plain), ("top_k 40, top_p 0.9", w_trunc, lp_trunc)):
        assert int(w.min()) >= 0 and int(w.max()) < V and not bool((w == unk).any()) and bool(torch.isfinite(lp).all()), label
        rc, lp_f, _ = forced_block(pd_, bd, w, V)
        assert rc == 0
        differ = int((bits(lp_f) != bits(lp)).sum())
        print(f"[forced vs {label}] M={M} V={V} nparts={nparts}: {differ} of {M} rows differ in the log-prob's bits")
        assert torch.equal(bits(lp_f), bits(lp)), label


def test_forced_block_word_stride_and_argument_checks(dev):
    M, V = 5, 50
    g = torch.Generator().manual_seed(3)
    parts = torch.randn(2, M, V, generator=g).to(dev)
    words2 = torch.randint(0, V, (M, 2), generator=g, dtype=torch.int64)
    rc, lp, rk = forced_block(parts, None, words2.to(dev), V, word_stride=2)
    lp_ref, rk_ref = FR.forced_select(FR.finished(parts.cpu(), None), words2[:, 0].numpy())
    assert rc == 0 and np.array_equal(rk.cpu().numpy(), rk_ref)
    np.testing.assert_allclose(lp.cpu().double().numpy(), lp_ref, rtol=0, atol=BLOCK_TOL)
    wd = words2[:, 0].contiguous().to(dev)
    assert forced_block(parts, None, None, V)[0] == BADARG                                   # no words
    assert forced_block(parts, None, wd, V, nparts=0)[0] == BADARG
    assert forced_block(parts, None, wd, V, M=0)[0] == BADARG
    assert forced_block(parts, None, wd, 1, M=1, nparts=1)[0] == BADARG                      # V < 2
    assert forced_block(parts, None, wd, V, word_stride=0)[0] == BADARG
    assert forced_block(parts, None, wd, V, stride=M * V - 1)[0] == BADARG                   # slabs overlap
    assert forced_block(parts, None, wd, 8193, M=1, nparts=1)[0] == TOOBIG                   # more than 32 logits per thread
    assert forced_block(parts, None, wd, 8192, M=1 << 19, nparts=1)[0] == TOOBIG             # M * V >= 2^32
    _, lp, rk = forced_block(parts, None, wd, V)                                             # nothing was launched by the refusals
    assert np.array_equal(rk.cpu().numpy(), rk_ref)


# ------------------------------------------------------------------ the engine against the oracle over given words
@functools.lru_cache(maxsize=None)
def _case(name, n, seed=4321):
    """inputs of one configuration, n captions per clip (caption 0 = synth.captions, further ones with the words re-drawn per j,
    same lengths) and the oracle's forced decode over them"""
    from oracle import ref_cpu as O
    d = synth.CONFIGS[name]
    sd, f_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed)
    cap0 = synth.captions(d, seed)
    caps = [cap0] + [np.where(cap0 > 0, synth.randint((d.B, d.T), seed + j, "forced_words", 2, d.V), 0) for j in range(1, n)]
    words = torch.from_numpy(np.stack(caps, 1).reshape(d.B * n, d.T).astype(np.int64))
    lp_ref, att_ref, _ = FR.forced_decode(O.to_torch(sd), O.to_torch(f_np), words, n)
    return d, sd, f_np, words, lp_ref.numpy(), att_ref.numpy()


def _check_vs_oracle(words, att, lp, rank, lp_ref, att_ref, label):
    """ALL rows and steps: the words are given, no row ever diverges"""
    w = words.numpy()
    rows, T = w.shape
    ref_w = np.take_along_axis(lp_ref, w[:, :, None], 2)[:, :, 0]
    dev_lp = np.abs(lp.cpu().numpy() - ref_w).max()
    print(f"[forced] {label}: max |logprob - oracle| {dev_lp:.3e}, max |att - oracle| {np.abs(att.cpu().numpy() - att_ref).max():.3e}")
    assert dev_lp <= LOGPROB_TOL, label
    np.testing.assert_allclose(att.cpu().numpy(), att_ref, **SEQ_TOL)
    rk = rank.cpu().numpy()
    for r in range(rows):
        for t in range(T):
            lo, hi = FR.rank_band(lp_ref[r, t].astype(np.float64), int(w[r, t]), LOGPROB_TOL)
            assert lo <= rk[r, t] <= hi, (label, r, t, int(rk[r, t]), lo, hi)


@pytest.mark.parametrize("name,n,path", [("tiny", 1, "ring"), ("tiny", 3, "tile"), ("cfg1", 1, "packed"), ("cfg1", 5, "tile"),
                                         ("cfg1", 1, "force_tile")])
def test_forced_engine_vs_oracle(dev, name, n, path):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, words, lp_ref, att_ref = _case(name, n)
    kw = dict(path="tile") if path == "force_tile" else {}
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, synth.UNK_IDX, forced_n=n, **kw)
    assert (eng.packed, eng.tile) == (path == "packed", path in ("tile", "force_tile")) and eng._plan is None and eng.nq == n
    eng.load_captions(words.to(dev))
    seq, att, lp, rank = eng.run()
    rows = d.B * n
    assert seq.shape == (rows, d.T) and att.shape == (rows, d.T, d.N) and lp.shape == (rows, d.T) and rank.shape == (rows, d.T)
    assert rank.dtype == torch.int32 and torch.equal(seq.cpu(), words) and int(eng.words[0].abs().sum()) == 0
    _check_vs_oracle(words, att, lp, rank, lp_ref, att_ref, f"{name} n={n} {path}")


def test_forced_paths_agree(dev):
    """packed vs tile vs ring on one cfg1 batch.  With one caption per clip and cfg1's widths path="ring" still binds the packed
    path (the engine's choice of paths, unchanged here), so the ring path gets the same captions twice per clip (n = 2): both of
    its rows per clip must agree with the packed path's one."""
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, words, _, _ = _case("cfg1", 1)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    e_p = DecodeEngine(W, fd, d.T, synth.UNK_IDX, forced_n=1).load_captions(words.to(dev))
    e_t = DecodeEngine(W, fd, d.T, synth.UNK_IDX, forced_n=1, path="tile").load_captions(words.to(dev))
    e_r = DecodeEngine(W, fd, d.T, synth.UNK_IDX, forced_n=2, path="ring").load_captions(words.repeat_interleave(2, 0).to(dev))
    assert e_p.packed and e_t.tile and not (e_r.packed or e_r.tile)
    _, att_p, lp_p, _ = (x.clone() for x in e_p.run())
    _, att_t, lp_t, _ = (x.clone() for x in e_t.run())
    _, att_r, lp_r, _ = (x.clone() for x in e_r.run())
    others = [("tile", att_t, lp_t), ("ring[0]", att_r[0::2], lp_r[0::2]), ("ring[1]", att_r[1::2], lp_r[1::2])]
    for label, att_o, lp_o in others:
        print(f"[forced paths] packed vs {label}: max |logprob diff| {float((lp_p - lp_o).abs().max()):.3e}")
        np.testing.assert_allclose(lp_p.cpu().numpy(), lp_o.cpu().numpy(), rtol=0, atol=LOGPROB_TOL, err_msg=label)
        np.testing.assert_allclose(att_p.cpu().numpy(), att_o.cpu().numpy(), **SEQ_TOL, err_msg=label)


@pytest.mark.parametrize("name,n", [("tiny", 3), ("cfg1", 1)])
def test_forced_graph_is_reused_across_caption_sets(dev, name, n):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, words, _, _ = _case(name, n)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    second = torch.where(words > 0, (words * 7 + 3) % (d.V - 2) + 2, words).flip(0).contiguous()
    g = DecodeEngine(W, fd, d.T, synth.UNK_IDX, forced_n=n).load_captions(words.to(dev)).capture()
    first = [x.clone() for x in g.run()]
    g.load_captions(second.to(dev))
    rg = [x.clone() for x in g.run()]
    e = DecodeEngine(W, fd, d.T, synth.UNK_IDX, forced_n=n).load_captions(second.to(dev))
    re_ = [x.clone() for x in e.run()]
    assert torch.equal(rg[0].cpu(), second) and not torch.equal(bits(first[2]), bits(rg[2]))
    for a, b in zip(rg, re_):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("name,path", [("cfg1", "auto"), ("cfg1", "tile")])
def test_forcing_the_greedy_words_gives_the_greedy_logprobs(dev, name, path):
    from helpers import to_dev
    from oracle import ref_cpu as O
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, _, _, _ = _case(name, 1)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    gr = DecodeEngine(W, fd, d.T, synth.UNK_IDX, path=path)
    seq, att = (x.clone() for x in gr.run())
    lp_g = gr.logprob.t().clone()
    fo = DecodeEngine(W, fd, d.T, synth.UNK_IDX, forced_n=1, path=path).load_captions(seq.contiguous())
    assert (gr.packed, gr.tile) == (fo.packed, fo.tile)
    _, att_f, lp_f, rank = fo.run()
    print(f"[forced vs greedy] {name} {path}: max |logprob diff| {float((lp_f - lp_g).abs().max()):.3e}")
    np.testing.assert_allclose(lp_f.cpu().numpy(), lp_g.cpu().numpy(), rtol=0, atol=BLOCK_TOL)
    np.testing.assert_allclose(att_f.cpu().numpy(), att.cpu().numpy(), rtol=0, atol=1e-6)
    # rank 0 wherever greedy's word was not the UNK-suppressed runner-up: where the oracle's UNK is clearly below the word
    lp_ref, _, _ = FR.forced_decode(O.to_torch(sd), O.to_torch(f_np), seq.cpu(), 1)
    ref_w = torch.gather(lp_ref, 2, seq.cpu().unsqueeze(2))[:, :, 0]
    unk_below = (lp_ref[:, :, synth.UNK_IDX] < ref_w - 2 * LOGPROB_TOL).numpy()
    rk = rank.cpu().numpy()
    assert (rk[unk_below] == 0).all() and ((rk == 0) | (rk == 1)).all() and unk_below.mean() > 0.5


# ------------------------------------------------------------------ refusals
def test_forced_engine_refusals_allocate_nothing(dev):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, words, _, _ = _case("tiny", 1)
    W, fd = DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev)
    d1, sd1, f1, _, _, _ = _case("cfg1", 1)
    W1, fd1 = DecodeWeights(to_dev(sd1, dev)), to_dev(f1, dev)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for w_, f_, kw in ((W, fd, dict(beam=2)), (W, fd, dict(temperature=1.0)), (W, fd, dict(gsk=True)), (W, fd, dict(gate_ksplit=True)),
                       (W, fd, dict(lang_ksx=True)), (W, fd, dict(forced_n=-1)), (W, fd, dict(forced_n=True)),
                       (W1, fd1, dict(forced_n=2, weights_dtype="bf16")),
                       (W1, fd1, dict(embgate=False))):      # the packed path without the embedding-gate schedule
        kw.setdefault("forced_n", 1)
        with pytest.raises(RuntimeError):
            DecodeEngine(w_, f_, d.T if w_ is W else d1.T, synth.UNK_IDX, **kw)
    assert torch.cuda.memory_allocated() == before
    assert DecodeEngine(W1, fd1, d1.T, synth.UNK_IDX, forced_n=1, embgate=False, path="tile").tile      # (the tile path has that form)
    e = DecodeEngine(W, fd, d.T, synth.UNK_IDX)
    with pytest.raises(RuntimeError):
        e.load_captions(words.to(dev))                   # not a forced engine
    f = DecodeEngine(W, fd, d.T, synth.UNK_IDX, forced_n=1)
    with pytest.raises(RuntimeError):
        f.load_captions(words[:, :-1].contiguous().to(dev))
    with pytest.raises(RuntimeError):
        f.load_captions(words.to(dev), torch.zeros(d.T, d.B, d.N + 1, dtype=torch.uint8, device=dev))
    f.load_captions(words.to(dev)).capture()
    with pytest.raises(RuntimeError):                    # a first frame mask after capture: the graph has no frame-masked output
        f.load_captions(words.to(dev), torch.zeros(d.T, d.B, d.N, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------ frame mask, model.score
def _score(model, feats, batch, **kw):
    B = feats["fc_feats"].shape[0]
    dummy = torch.zeros(B, 1, 1, device=feats["fc_feats"].device)
    return model.score(feats, batch["input_seq"], batch["gt_seq"], batch["num"], batch["proposals"], batch["gt_bboxs"],
                       batch["box_mask"], dummy, batch["frm_mask"], batch["sample_idx"], feats["pnt_mask"], **kw)


@pytest.mark.parametrize("name,seed,graph", [("tiny", 4321, False), ("tiny", 99, True), ("cfg1", 4321, False)])
def test_score_grounding_vs_the_oracles_training_pass(dev, name, seed, graph):
    from helpers import build_model, to_dev
    from oracle import ref_cpu as O
    d = synth.CONFIGS[name]
    sd, f_np, b_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed), synth.label_glue_batch(d, seed)
    c = {}
    with torch.no_grad():
        O.cyclical_forward(O.to_torch(sd), O.to_torch(f_np), O.to_torch(b_np), T=d.T, vocab_size=d.V, train_decoder_only=True, collect=c)
    model = build_model(d, sd, dev, hip_graph=graph)
    f, b = to_dev(f_np, dev), to_dev(b_np, dev)
    out = _score(model, f, b, grounding=True)
    eng = model._score_cache[1]
    assert (eng.graph is not None) == graph and eng.fm_steps.shape == (d.T, d.B, d.N)
    assert torch.equal(out["att2_weights"], eng.fm_steps.transpose(0, 1))
    fmo, labels = c["frm_mask_output"].numpy(), c["roi_labels"].numpy()
    assert np.array_equal(out["roi_labels"].cpu().numpy(), labels) and np.array_equal(out["frm_mask_output"].cpu().numpy(), fmo)
    masked = fmo[:, :, 1:]
    for key in ("att2_weights", "ground_weights"):
        got, want = out[key].cpu().numpy(), c[key].numpy()
        assert np.array_equal(got[masked], want[masked]) and (want[masked] == -1e8).all(), key     # equal fill
        np.testing.assert_allclose(got[~masked], want[~masked], **SEQ_TOL)
        pick, hit = FR.ground_picks(got, fmo, labels)
        pick_o, hit_o = FR.ground_picks(want, fmo, labels)
        assert np.array_equal(pick, pick_o) and np.array_equal(hit, hit_o), key
    # log-probs of the GT captions against the same pass's log-softmax, masked as LMCriterion masks them
    gt = torch.from_numpy(b_np["gt_seq"][:, 0])
    ref_w = torch.gather(c["lang"], 2, gt.unsqueeze(2))[:, :, 0]
    np.testing.assert_allclose(out["logprob"].cpu().numpy(), ref_w.numpy(), rtol=0, atol=LOGPROB_TOL)
    assert torch.equal(out["mask"].cpu(), O._text_mask(gt))
    np.testing.assert_allclose(out["seq_logprob"].cpu().numpy(), (ref_w * O._text_mask(gt)).sum(1).numpy(), rtol=0, atol=d.T * LOGPROB_TOL)
    # a second batch through the cached engine (graph replay where asked for): same batch, same bits
    out2 = _score(model, f, b, grounding=True)
    assert model._score_cache[1] is eng
    for k in out:
        assert torch.equal(bits(out[k]), bits(out2[k])), k


@pytest.mark.parametrize("graph", [False, True])
def test_model_score_captions_refusals_and_sample_is_untouched(dev, graph):
    from helpers import build_model, to_dev, model_call
    d, sd, f_np, words3, lp_ref, att_ref = _case("tiny", 3, 99)
    model = build_model(d, sd, dev, hip_graph=graph)
    f, b = to_dev(f_np, dev), to_dev(synth.label_glue_batch(d, 99), dev)
    seq, att, _ = model_call(model, f, b, True)
    eng_before = model._engine_cache[1]
    # default captions: the batch's GT captions
    out = _score(model, f, b)
    gt = b["gt_seq"][:, 0]
    assert out["logprob"].shape == (d.B, d.T) and out["rank"].dtype == torch.int32 and out["att"].shape == (d.B, d.T, d.N)
    assert "att2_weights" not in out
    ref1 = np.take_along_axis(lp_ref.reshape(d.B, 3, d.T, d.V)[:, 0], gt.cpu().numpy()[:, :, None], 2)[:, :, 0]
    np.testing.assert_allclose(out["logprob"].cpu().numpy(), ref1, rtol=0, atol=LOGPROB_TOL)
    # n = 3 captions per clip, both layouts
    o3 = _score(model, f, b, captions=words3.to(dev))
    o3b = _score(model, f, b, captions=words3.view(d.B, 3, d.T).to(dev))
    ref3 = np.take_along_axis(lp_ref, words3.numpy()[:, :, None], 2)[:, :, 0]
    np.testing.assert_allclose(o3["logprob"].cpu().numpy(), ref3, rtol=0, atol=LOGPROB_TOL)
    np.testing.assert_allclose(o3["att"].cpu().numpy(), att_ref, **SEQ_TOL)
    assert all(torch.equal(bits(o3[k]), bits(o3b[k])) for k in o3)
    m = o3["mask"].cpu().numpy()
    w = words3.numpy()
    for r in range(w.shape[0]):                          # the steps up to and including the first 0
        z = np.nonzero(w[r] == 0)[0]
        assert m[r].sum() == (z[0] + 1 if len(z) else d.T) and m[r, :m[r].sum()].all()
    np.testing.assert_allclose(o3["seq_logprob"].cpu().numpy(), (o3["logprob"].cpu().numpy() * m).sum(1), rtol=1e-6, atol=1e-6)
    # refusals
    with pytest.raises(RuntimeError):
        _score(model, f, b, captions=words3.to(dev), grounding=True)
    with pytest.raises(RuntimeError):
        _score(model, f, b, captions=words3[:, :-1].contiguous().to(dev))
    with pytest.raises(RuntimeError):
        _score(model, f, b, captions=words3[:d.B * 3 - 1].to(dev))
    model.seq_per_img = 2
    with pytest.raises(RuntimeError):
        _score(model, f, b, grounding=True)
    model.seq_per_img = 1
    # _sample between / after score calls: same engine, same bits
    seq2, att2, _ = model_call(model, f, b, True)
    assert model._engine_cache[1] is eng_before and torch.equal(seq, seq2) and torch.equal(bits(att), bits(att2))
    assert not model.training


def test_score_with_bf16_weights_equals_fp32_on_the_rounded_checkpoint(dev):
    """the invariant of tests/test_gpu_decode_bf16.py.  The rounded checkpoint is made on the model: its state dict names the two
    LSTM cells twice (the reconstructor shares them), so rounding only the decoder_core.* entries of a dict would be undone when the
    shared parameters are loaded a second time."""
    from helpers import build_model, to_dev
    from cvc.decode import BF16_ROUNDED_KEYS, bf16_round
    d = synth.CONFIGS["cfg1"]
    sd, f_np, b_np = synth.hot_path_state_dict(d, 4321), synth.clip_features(d, 4321), synth.label_glue_batch(d, 4321)
    f, b = to_dev(f_np, dev), to_dev(b_np, dev)
    model = build_model(d, sd, dev)
    o_bf = _score(model, f, b, decode_weights="bf16")
    assert model._score_cache[1].bf16w and model._score_cache[1].packed
    o_32 = _score(model, f, b)                                                               # a switch re-binds
    assert not model._score_cache[1].bf16w
    model_r = build_model(d, sd, dev)
    params = model_r.state_dict(keep_vars=True)
    with torch.no_grad():
        for k in BF16_ROUNDED_KEYS:
            params[k].copy_(bf16_round(params[k]))
    o_r = _score(model_r, f, b)
    for k in ("logprob", "rank", "att", "seq_logprob"):
        assert torch.equal(bits(o_bf[k]), bits(o_r[k])), k
    assert not torch.equal(bits(o_bf["logprob"]), bits(o_32["logprob"]))                     # the mode really rounds
    with pytest.raises(RuntimeError):                                                        # n > 1 runs on the tile path: refused
        _score(model, f, b, captions=b["gt_seq"][:, :2].contiguous(), decode_weights="bf16")


# ------------------------------------------------------------------ trainer and CLI
def test_trainer_scores_and_grounds_the_gt_captions_from_disk(dev, tmp_path):
    """cvc.main over the on-disk dataset with --eval_obj_grounding_gt (one epoch, then eval -> ground_gt), Trainer.score /
    ground_gt on the trainer it leaves, and the CLI on its checkpoint."""
    import pickle
    from cvc import main as cvc_main
    from cvc import score as cvc_score
    from cvc.data_fixture import write_tiny_anet_dataset, CLASSES, VG_CLASSES
    root = tmp_path / "anet"
    o = write_tiny_anet_dataset(str(root), seed=7, feat=24, rgb_dim=2048, bn_dim=1024, n_videos=6)
    d = synth.Dims(G=24, DET=len(CLASSES))
    tables = synth.detectron_tables(d, 7, n_vg=len(VG_CLASSES) + 1)
    wdir = root / "detectron"
    wdir.mkdir()
    for k in ("fc7_w", "fc7_b", "cls_score_w", "cls_score_b"):
        pickle.dump(tables[k], open(wdir / (k + ".pkl"), "wb"))
    argv = ["--no_cfg", "--max_epochs", "1", "--batch_size", "2", "--num_workers", "0", "--seq_per_img", "1",
            "--input_dic", o.input_dic, "--input_json", o.input_json, "--grd_reference", o.grd_reference, "--proposal_h5", o.proposal_h5,
            "--feature_root", o.feature_root, "--seg_feature_root", o.seg_feature_root, "--glove_path", o.glove_path,
            "--vg_vocab_file", o.vg_vocab_file, "--detectron_weights_dir", str(wdir), "--exclude_bgd_det",
            "--num_sampled_frm", "2", "--num_prop_per_frm", "5", "--t_attn_size", "6", "--att_feat_size", "24", "--vis_encoding_size", "24",
            "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "8",
            "--train_split", "training", "--val_split", "validation", "--tensorboard", "0", "--disp_interval", "100",
            "--checkpoint_path", str(tmp_path) + "/", "--exp_name", "disk", "--learning_rate", "0.001",
            "--results_dir", str(tmp_path / "results"), "--id", "g1"]
    assert cvc_main.main(argv + ["--eval_obj_grounding_gt"]) == 0
    tr = cvc_main.LAST_TRAINER
    res = tmp_path / "results"

    def check_grounding(stats):
        assert set(stats) == {"obj_words", "box_accu_att", "box_accu_att_per_cls", "box_accu_grd", "box_accu_grd_per_cls"}
        assert all(0.0 <= stats[k] <= 1.0 for k in stats if k != "obj_words") and stats["obj_words"] > 0
        for stem in ("attn", "grd"):
            got = json.load(open(res / (stem + "-gt-sent-results-validation-g1.json")))
            assert got["eval_mode"] == "GT" and got["results"]
            n_words = 0
            for vid, segs in got["results"].items():
                for seg, e in segs.items():
                    assert set(e) == {"clss", "idx_in_sent", "bbox_for_all_frames"}
                    assert len(e["clss"]) == len(e["idx_in_sent"]) == len(e["bbox_for_all_frames"])
                    assert all(len(bx) == 2 and all(len(f) == 4 for f in bx) for bx in e["bbox_for_all_frames"])      # 2 sampled frames
                    assert all(c in CLASSES for c in e["clss"])
                    n_words += len(e["clss"])
            assert n_words >= stats["obj_words"]

    check_grounding(tr.grounding_gt_stats)                                      # eval ran ground_gt and kept the result to itself
    first = dict(tr.grounding_gt_stats)
    for f in res.glob("*-gt-sent-results-*"):
        f.unlink()
    again = tr.ground_gt()
    check_grounding(again)
    assert again == first                                                       # same checkpoint, same split: deterministic
    stats = tr.score()
    assert set(stats) == {"ppl", "top1"} and np.isfinite(stats["ppl"]) and stats["ppl"] > 1.0 and 0.0 <= stats["top1"] <= 1.0
    scores = json.load(open(res / "densecap-validation-g1_scores.json"))
    grd = json.load(open(o.grd_reference))["annotations"]
    tot_lp = tot_w = 0
    for vid, segs in scores.items():
        for e in segs:
            assert set(e) == {"segment", "timestamp", "logprob", "words", "top1"}
            assert e["logprob"] < 0 and 1 <= e["words"] <= 8 and 0 <= e["top1"] <= e["words"]
            assert e["timestamp"] == [round(t, 2) for t in grd[vid]["segments"][e["segment"]]["timestamps"]]
            tot_lp, tot_w = tot_lp + e["logprob"], tot_w + e["words"]
    assert stats["ppl"] == pytest.approx(np.exp(-tot_lp / tot_w), rel=1e-9)
    # the CLI: its own flag, the rest to cvc.main with the checkpoint loading of an inference-only run
    for f in list(res.glob("*_scores.json")) + list(res.glob("*-gt-sent-results-*")):
        f.unlink()
    assert cvc_score.main(argv + ["--resume", "True", "--ground_gt"]) == 0
    assert json.load(open(res / "densecap-validation-g1_scores.json")) == scores
    check_grounding(again)
