"""bf16-stored decode weights on the GPU (DecodeEngine(weights_dtype="bf16"), csrc/gemm_packed.hip): the two kernels against
fp64 and against the fp32 kernels on the rounded weights, the engine against the CPU oracle on the rounded checkpoint and against the
fp32 engine on rounded weights, idempotence / determinism / reuse, sampling with one caption per clip, the model plumbing and the
refusals."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from cvc import synth

pytestmark = pytest.mark.gpu

OP_TOL = dict(rtol=2e-5, atol=2e-5)       # one fused LSTM cell against fp64 (tests/test_gpu_parity.py)
SEQ_TOL = dict(rtol=1e-4, atol=1e-4)      # attention maps after T recurrent steps
LOGPROB_TOL = 1e-4

# (B, N, F, R, A, E, V, T), seed: the oracle's smallest deciding margin on the ROUNDED checkpoint is 6.4e-4 / 2.4e-4 / 3.9e-3 there,
# and every (clip, step) stays comparable even if every margin below the tie tolerance flipped (checked on the CPU with the oracle)
SMALL = {"w128": ((37, 20, 12, 128, 64, 64, 300, 6), 4242), "w256": ((64, 33, 17, 256, 96, 96, 1000, 8), 4242), "cfg1": ("cfg1", 3)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from cvc import hip
    hip.lib()
    return hip


def close(a, b, **tol):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, **tol)


def same_up_to_zero_sign(a, b):
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | ((a == 0) & (b == 0))).all())


def rounded(sd):
    """the checkpoint the bf16 engine is specified on: the six matrices through bf16_round, everything else untouched"""
    from cvc.decode import BF16_ROUNDED_KEYS, bf16_round
    out = dict(sd)
    for k in BF16_ROUNDED_KEYS:
        out[k] = bf16_round(torch.from_numpy(np.ascontiguousarray(sd[k]))).numpy()
    return out


def dims_of(key):
    spec, seed = SMALL[key]
    if isinstance(spec, str):
        return synth.CONFIGS[spec], seed
    B, N, F, R, A, E, V, T = spec
    return dataclasses.replace(synth.CONFIGS["tiny"], B=B, N=N, F=F, R=R, A=A, E=E, V=V, T=T), seed


@functools.lru_cache(maxsize=None)
def case(key):
    """inputs of one shape and the CPU oracle's greedy decode on the rounded checkpoint"""
    from oracle import ref_cpu as O
    d, seed = dims_of(key)
    sd, f_np = synth.hot_path_state_dict(d, seed), synth.clip_features(d, seed)
    sd_r = rounded(sd)
    with torch.no_grad():
        seq_o, att_o, _, logp_o = O.greedy_sample(O.to_torch(sd_r), O.to_torch(f_np), d.T, synth.UNK_IDX, return_logprobs=True)
    return d, sd, sd_r, f_np, seq_o, att_o, logp_o


def run_clone(eng):
    out = eng.run()
    return out[0].clone(), out[1].clone(), eng.logprob.t().clone()


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("M,K,N,ksplit", [(64, 6144, 8192, 1), (64, 2048, 5000, 1), (17, 256, 96, 1), (64, 2048, 1024, 8), (33, 512, 200, 3)])
def test_bf16w_linear_kernel_vs_fp64_and_the_fp32_kernel(dev, lib, M, K, N, ksplit):
    """cvc_packed_linear_bf16w_fwd against x @ bf16_round(w)^T + b in fp64; yardstick: the fp32 kernel (split mode 2) on a pack of
    the same rounded weights, run here.  rms and max error at most 1.25 x the yardstick's, rms at most 1e-6 of the result's; the
    kernel keeps the fp32 kernel's summation order, so the outputs are also equal bit for bit (up to the sign of zero)."""
    from cvc.decode import bf16_round, pack_weights, pack_weights_bf16, to_quad
    g = torch.Generator(device="cpu").manual_seed(K + N)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
    x = torch.randn(M, K, generator=g).to(dev)
    x[:, ::7] *= 1e-3
    x[:, 3::11] *= 64.0
    x[:, 5::13] *= 1e18                       # wide exponent range: the split terms must not over- / underflow
    w[:, 5::13] *= 1e-18
    x[0, :4] = torch.tensor([0.0, -0.0, 1.0, -2.0 ** -100])
    b = torch.randn(N, generator=g).to(dev)
    wr = bf16_round(w)
    assert torch.isfinite(wr).all() and (wr.abs()[wr != 0] >= 2.0 ** -126).all()      # finite and normal after rounding
    wb, wp, xq = pack_weights_bf16(w), pack_weights(wr), to_quad(x)
    assert wb.element_size() == 2
    ref = x.double() @ wr.double().t() + b.double()
    st = torch.cuda.current_stream().cuda_stream
    L = lib.lib()
    prev = lib.gemm_packed_split(-1)
    try:
        lib.gemm_packed_split(2)
        y_p = torch.zeros(ksplit, M, N, device=dev)
        assert L.cvc_packed_linear_fwd(wp.data_ptr(), xq.data_ptr(), K, b.data_ptr(), M, N, ksplit, y_p.data_ptr(), N, None, st) == 0
    finally:
        lib.gemm_packed_split(prev)
    y_b = torch.zeros(ksplit, M, N, device=dev)
    assert L.cvc_packed_linear_bf16w_fwd(wb.data_ptr(), xq.data_ptr(), K, b.data_ptr(), M, N, ksplit, y_b.data_ptr(), N, None, st) == 0
    err = {}
    for name, y in (("fp32 kernel", y_p), ("bf16w kernel", y_b)):
        e = (y.double().sum(0) - ref).abs()
        err[name] = (e.pow(2).mean().sqrt().item(), e.max().item())
    bitwise = same_up_to_zero_sign(y_b, y_p)
    print(f"[bf16w linear] M={M} K={K} N={N} ksplit={ksplit}: (rms, max) {err}, rms(ref) {ref.pow(2).mean().sqrt().item():.3e}, "
          f"bitwise equal to the fp32 kernel: {bitwise}")
    assert err["bf16w kernel"][0] <= 1.25 * err["fp32 kernel"][0] and err["bf16w kernel"][1] <= 1.25 * err["fp32 kernel"][1], err
    assert err["bf16w kernel"][0] <= 1e-6 * ref.pow(2).mean().sqrt().item(), err
    assert bitwise
    if ksplit == 1:
        # the top-2 / log-sum-exp records of the vocabulary head: the same records as the fp32 kernel's, consumed by cvc_top2_final
        nblk = (N + 31) // 32
        rec_p, rec_b = torch.zeros(nblk, 64, 6, device=dev), torch.zeros(nblk, 64, 6, device=dev)
        try:
            lib.gemm_packed_split(2)
            assert L.cvc_packed_linear_fwd(wp.data_ptr(), xq.data_ptr(), K, b.data_ptr(), M, N, 1, None, N, rec_p.data_ptr(), st) == 0
        finally:
            lib.gemm_packed_split(prev)
        assert L.cvc_packed_linear_bf16w_fwd(wb.data_ptr(), xq.data_ptr(), K, b.data_ptr(), M, N, 1, None, N, rec_b.data_ptr(), st) == 0
        assert same_up_to_zero_sign(rec_b[:, :M], rec_p[:, :M])
        assert float(rec_b[:, M:].abs().sum()) == 0.0                       # rows beyond M are not written
        word = torch.zeros(M, dtype=torch.int64, device=dev)
        lp = torch.zeros(M, device=dev)
        assert L.cvc_top2_final(rec_b.data_ptr(), nblk, M, synth.UNK_IDX, word.data_ptr(), 1, lp.data_ptr(), None, 0, None, 0, st) == 0
        z = ref.clone()
        z[:, synth.UNK_IDX] = -float("inf")
        top = z.topk(2, 1)
        clear = (top.values[:, 0] - top.values[:, 1]) > 1e-3 * top.values[:, 0].abs().clamp(min=1.0)
        assert clear.any() and torch.equal(word[clear].cpu(), top.indices[clear, 0].cpu())


@pytest.mark.parametrize("M,R,K", [(64, 64, 160), (20, 128, 416), (3, 40, 96), (64, 1024, 3072), (64, 2048, 4096)])
def test_bf16w_lstm_kernel_vs_fp64_cell_and_the_fp32_kernel(dev, lib, M, R, K):
    """cvc_packed_lstm_bf16w_fwd against an fp64 LSTM cell on the rounded weights and against cvc_packed_lstm_embgate_ex_fwd on a
    pack of them: with the embedding-gate gather and the per-row gate term, M < 64 (rows beyond M stay zero), a contraction that
    stops short of the pack, and w_cached on / off."""
    from cvc.decode import bf16_round, from_quad, pack_weights, pack_weights_bf16, to_quad
    g = torch.Generator().manual_seed(M * 13 + R + K)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    V = 50
    w = rnd(4 * R, K) / K ** 0.5
    b_ih, b_hh = rnd(4 * R) * 0.1, rnd(4 * R) * 0.1
    x, c_prev = rnd(M, K), rnd(M, R)
    gate_bias, table = rnd(M, 4 * R) * 0.2, rnd(V, 4 * R) * 0.2
    word = torch.randint(0, V, (M,), generator=g).to(dev)
    wr = bf16_round(w)
    wb, wp, xq, cq = pack_weights_bf16(w, R), pack_weights(wr, R), to_quad(x), to_quad(c_prev)
    st = torch.cuda.current_stream().cuda_stream
    L = lib.lib()
    zq = lambda: torch.zeros(R // 4, 64, 4, device=dev)

    def cell64(Kc, with_bias, with_rows):
        pre = x[:, :Kc].double() @ wr[:, :Kc].double().t()
        if with_bias:
            pre = pre + b_ih.double() + b_hh.double()
        if with_rows:
            pre = pre + gate_bias.double() + table.double()[word]
        i, f, gg, o = pre.chunk(4, 1)
        c64 = torch.sigmoid(f) * c_prev.double() + torch.sigmoid(i) * torch.tanh(gg)
        return torch.sigmoid(o) * torch.tanh(c64), c64

    def bf16w(Kc, with_bias, with_rows, cached):
        h1, h2, c = zq(), zq(), zq()
        rc = L.cvc_packed_lstm_bf16w_fwd(wb.data_ptr(), K * 32, xq.data_ptr(), Kc, b_ih.data_ptr() if with_bias else None,
                                         b_hh.data_ptr() if with_bias else None, gate_bias.data_ptr() if with_rows else None,
                                         table.data_ptr() if with_rows else None, word.data_ptr() if with_rows else None,
                                         cq.data_ptr(), M, R, h1.data_ptr(), h2.data_ptr(), c.data_ptr(), 1 if cached else 0, st)
        assert rc == 0
        return h1, h2, c

    def fp32(Kc, with_bias, cached):
        h1, h2, c = zq(), zq(), zq()
        prev = lib.gemm_packed_split(-1)
        try:
            lib.gemm_packed_split(2)
            rc = L.cvc_packed_lstm_embgate_ex_fwd(wp.data_ptr(), (K // 4) * 128, xq.data_ptr(), Kc, b_ih.data_ptr() if with_bias else None,
                                                  b_hh.data_ptr() if with_bias else None, gate_bias.data_ptr(), table.data_ptr(),
                                                  word.data_ptr(), cq.data_ptr(), M, R, h1.data_ptr(), h2.data_ptr(), c.data_ptr(),
                                                  1 if cached else 0, st)
        finally:
            lib.gemm_packed_split(prev)
        assert rc == 0
        return h1, h2, c

    for Kc in sorted({K, K - 32, 32}):
        for with_bias in (True, False):
            h64, c64 = cell64(Kc, with_bias, True)
            h1, h2, c = bf16w(Kc, with_bias, True, False)
            assert torch.equal(h1, h2)
            close(from_quad(h1, M), h64.float(), **OP_TOL)
            close(from_quad(c, M), c64.float(), **OP_TOL)
            assert float(h1[:, M:].abs().sum()) == 0.0 and float(c[:, M:].abs().sum()) == 0.0           # rows beyond M stay zero
            h1c, _, cc = bf16w(Kc, with_bias, True, True)
            assert torch.equal(h1c, h1) and torch.equal(cc, c)                                          # w_cached: same bits
            hp, _, cp = fp32(Kc, with_bias, False)
            close(from_quad(h1, M), from_quad(hp, M), **OP_TOL)
            close(from_quad(c, M), from_quad(cp, M), **OP_TOL)
            bitwise = same_up_to_zero_sign(h1, hp) and same_up_to_zero_sign(c, cp)
            print(f"[bf16w lstm] M={M} R={R} K={Kc}/{K} bias={with_bias}: max |h - h64| {(from_quad(h1, M).double() - h64).abs().max().item():.2e}, "
                  f"max |h - fp32 kernel| {(h1 - hp).abs().max().item():.2e}, bitwise equal: {bitwise}")
            assert bitwise                                                                              # the summation order is kept
    # no gather, no per-row term (the language cell's form)
    h64, c64 = cell64(K, True, False)
    h1, _, c = bf16w(K, True, False, False)
    close(from_quad(h1, M), h64.float(), **OP_TOL)
    close(from_quad(c, M), c64.float(), **OP_TOL)


# ------------------------------------------------------------------ 2. / 3. the engine
def check_against_oracle(seq, att, lp, seq_o, att_o, logp_o, B, T, label):
    from helpers import tie_aware_seq_equal
    stats = {}
    n_exact = tie_aware_seq_equal(seq.cpu().numpy(), seq_o.numpy(), logp_o.numpy(), stats=stats)
    print(f"[bf16 engine vs oracle] {label}: n_exact {n_exact} / {B * T}, {stats}")
    assert n_exact >= 0.95 * B * T
    same = (seq.cpu() == seq_o).all(1)
    close(att.cpu()[same], att_o[same], **SEQ_TOL)
    lp_o = logp_o.gather(2, seq_o.unsqueeze(2)).squeeze(2)
    assert float((lp.cpu()[same] - lp_o[same]).abs().max()) <= LOGPROB_TOL
    assert not (seq == synth.UNK_IDX).any()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("key", ["w128", "w256", "cfg1"])
def test_bf16_engine_vs_oracle_on_the_rounded_checkpoint(dev, lib, key, graph):
    """The engine bound to the UNROUNDED checkpoint with weights_dtype="bf16" computes what the oracle computes on the rounded one;
    and what the fp32 engine computes on rounded weights (same words wherever the oracle's margins are clear, attention and
    log-probs within the fp32 tolerances -- bit for bit, in fact: the kernels keep the fp32 kernels' summation order)."""
    from helpers import to_dev, deciding_gaps
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, sd_r, f_np, seq_o, att_o, logp_o = case(key)
    W = DecodeWeights(to_dev(sd, dev))
    f = to_dev(f_np, dev)
    eng = DecodeEngine(W, f, d.T, synth.UNK_IDX, weights_dtype="bf16")
    assert eng.packed and eng.embgate and eng.bf16w and eng._plan is None
    if graph:
        eng.capture()
    seq, att, lp = run_clone(eng)
    check_against_oracle(seq, att, lp, seq_o, att_o, logp_o, d.B, d.T, f"{key} graph={graph}")
    # the fp32 engine (the parent's path) on the rounded weights
    e32 = DecodeEngine(DecodeWeights(to_dev(sd_r, dev)), f, d.T, synth.UNK_IDX)
    seq32, att32, lp32 = run_clone(e32)
    clear = torch.from_numpy(deciding_gaps(logp_o.numpy()).min(1) > 1e-3).to(dev)
    assert torch.equal(seq[clear], seq32[clear])
    same = (seq == seq32).all(1)
    close(att[same], att32[same], **SEQ_TOL)
    assert float((lp[same] - lp32[same]).abs().max()) <= LOGPROB_TOL
    bitwise = torch.equal(seq, seq32) and same_up_to_zero_sign(att, att32) and same_up_to_zero_sign(lp, lp32)
    print(f"[bf16 engine vs fp32 engine on rounded weights] {key}: clips with equal words {int(same.sum())} / {d.B}, max |att diff| "
          f"{(att - att32).abs().max().item():.2e}, max |logprob diff| {(lp - lp32).abs().max().item():.2e}, bitwise equal: {bitwise}")
    if lib.gemm_packed_split(-1) == 2:
        assert bitwise


def test_bf16_engine_cfg2_vs_the_fp64_referee(dev, lib):
    """Config 2 (the benchmarked size): the oracle's smallest margin on the rounded checkpoint is 1.7 x the tie tolerance, so the
    words are held to the fp64 referee with its measured tolerance (helpers.referee_seq_check), as the fp32 engine's are."""
    from helpers import to_dev, referee_seq_check
    import fullsize_oracle as FO
    from cvc.decode import DecodeEngine, DecodeWeights
    d = synth.CONFIGS["cfg2"]
    sd, f_np = synth.hot_path_state_dict(d, 1236), synth.clip_features(d, 1236)
    sd_r = rounded(sd)
    ref, _src = FO.greedy("cfg2_bf16w", 1236, d, sd_r, f_np)       # no stored fixture under this name: the oracle and the referee run now
    W = DecodeWeights(to_dev(sd, dev))
    f = to_dev(f_np, dev)
    eager = run_clone(DecodeEngine(W, f, d.T, synth.UNK_IDX, weights_dtype="bf16"))
    eng = DecodeEngine(W, f, d.T, synth.UNK_IDX, weights_dtype="bf16").capture()
    seq, att, lp = run_clone(eng)
    assert torch.equal(seq, eager[0]) and torch.equal(att, eager[1]) and torch.equal(lp, eager[2])
    st = referee_seq_check(seq.cpu().numpy(), lp.cpu().numpy(), ref, "cfg2 greedy, bf16 weights")
    same = (seq.cpu() == torch.from_numpy(ref["seq"])).all(1)
    assert int(same.sum()) >= 0.95 * d.B, st
    close(att.cpu()[same], torch.from_numpy(ref["att"])[same], **SEQ_TOL)
    close(att.sum(2), torch.ones(d.B, d.T), rtol=1e-5, atol=1e-5)
    # both gate matrices and the linear weights fit the cache plan together; 2-byte packs, and no fp32 pack on this binding
    assert eng.att_w_cached and eng.lang_w_cached
    for name in ("pb_att2", "pb_lang", "pb_h", "pb_o"):
        assert getattr(W, name).element_size() == 2
    assert not any(hasattr(W, n) for n in ("p_lang", "p_att2", "p_att", "p_h", "p_o"))
    # replay determinism
    seq2, att2, lp2 = run_clone(eng)
    assert torch.equal(seq, seq2) and torch.equal(att, att2) and torch.equal(lp, lp2)
    # the fp32 engine on the rounded weights
    seq32, att32, lp32 = run_clone(DecodeEngine(DecodeWeights(to_dev(sd_r, dev)), f, d.T, synth.UNK_IDX).capture())
    clear = torch.from_numpy(ref["gaps"].min(1) > 1e-3).to(dev)
    assert torch.equal(seq[clear], seq32[clear])
    eq = (seq == seq32).all(1)
    close(att[eq], att32[eq], **SEQ_TOL)
    assert float((lp[eq] - lp32[eq]).abs().max()) <= LOGPROB_TOL
    bitwise = torch.equal(seq, seq32) and same_up_to_zero_sign(att, att32) and same_up_to_zero_sign(lp, lp32)
    print(f"[bf16 engine vs fp32 engine on rounded weights] cfg2: equal clips {int(eq.sum())} / {d.B}, bitwise equal: {bitwise}")
    if lib.gemm_packed_split(-1) == 2:
        assert bitwise


# ------------------------------------------------------------------ 4. the mode really rounds
def test_bf16_mode_really_rounds(dev, lib):
    """At the first shape the oracles on the unrounded and on the rounded checkpoint differ by 2.5e-2 in the attention maps: the
    bf16 engine is on the rounded side (the test above) and far from the unrounded oracle."""
    from helpers import to_dev
    from oracle import ref_cpu as O
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, sd_r, f_np, seq_o, att_o, logp_o = case("w128")
    with torch.no_grad():
        att_u = O.greedy_sample(O.to_torch(sd), O.to_torch(f_np), d.T, synth.UNK_IDX, return_logprobs=True)[1]
    W = DecodeWeights(to_dev(sd, dev))
    eng = DecodeEngine(W, to_dev(f_np, dev), d.T, synth.UNK_IDX, weights_dtype="bf16")
    seq, att, lp = run_clone(eng)
    check_against_oracle(seq, att, lp, seq_o, att_o, logp_o, d.B, d.T, "w128 (rounding check)")
    diff = float((att.cpu() - att_u).abs().max())
    print(f"[bf16 mode] max |attention - unrounded oracle's| {diff:.3e}; oracle rounded vs unrounded {float((att_o - att_u).abs().max()):.3e}")
    assert diff > 10 * SEQ_TOL["atol"]
    for name in ("pb_att2", "pb_lang", "pb_h", "pb_o"):
        assert getattr(W, name).dtype == torch.bfloat16 and getattr(W, name).element_size() == 2
    assert not any(hasattr(W, n) for n in ("p_lang", "p_att2", "p_h", "p_o"))
    # the derived fp32 operands come from the rounded matrices
    from cvc.decode import bf16_round
    assert torch.equal(W.r_w_fc, bf16_round(W.w_ih_att[:, d.R:2 * d.R]))
    t64 = torch.relu(W.embed).double() @ bf16_round(W.w_ih_att[:, 2 * d.R:2 * d.R + d.E]).double().t()
    close(W.r_embgate, t64.float(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------ 5. idempotence, determinism, reuse
def test_bf16_engine_idempotent_deterministic_and_reusable(dev, lib):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, sd_r, f_np, *_ = case("w256")
    f = to_dev(f_np, dev)
    a = run_clone(DecodeEngine(DecodeWeights(to_dev(sd, dev)), f, d.T, synth.UNK_IDX, weights_dtype="bf16"))
    b = run_clone(DecodeEngine(DecodeWeights(to_dev(sd_r, dev)), f, d.T, synth.UNK_IDX, weights_dtype="bf16"))
    for x, y in zip(a, b):                                  # rounding an already rounded checkpoint changes nothing
        assert torch.equal(x, y)
    W = DecodeWeights(to_dev(sd, dev))
    eng = DecodeEngine(W, f, d.T, synth.UNK_IDX, weights_dtype="bf16", own_features=True).capture()
    r1, r2 = run_clone(eng), run_clone(eng)
    for x, y, z in zip(r1, r2, a):
        assert torch.equal(x, y) and torch.equal(x, z)
    f2 = to_dev(synth.clip_features(d, 99), dev)
    eng.load_features(f2)
    got = run_clone(eng)
    fresh = run_clone(DecodeEngine(W, f2, d.T, synth.UNK_IDX, weights_dtype="bf16"))
    for x, y in zip(got, fresh):
        assert torch.equal(x, y)
    assert not torch.equal(got[1], r1[1])
    # per-launch timing walks the same list, under the fp32 engine's launch names
    t = eng.run_timed()
    assert set(t) == {"gate_fc", "att_lstm", "h2attn", "attn_scores", "attn_wsum", "lang_lstm", "logits", "word_select"}
    assert all(len(v) == d.T for k, v in t.items() if k != "gate_fc")


@pytest.mark.parametrize("B,N,F", [(1, 1, 1), (33, 50, 17), (63, 129, 5)])
def test_bf16_engine_ragged_batch_and_region_counts(dev, lib, B, N, F):
    from helpers import to_dev
    from oracle import ref_cpu as O
    from cvc.decode import DecodeEngine, DecodeWeights
    d = dataclasses.replace(synth.CONFIGS["tiny"], B=B, N=N, F=F, R=64, A=32, E=32, V=97, T=6)
    sd, f_np = synth.hot_path_state_dict(d, 11), synth.clip_features(d, 11, full_mask_clip=0 if B > 1 else None)
    sd_r = rounded(sd)
    with torch.no_grad():
        seq_o, att_o, _, logp_o = O.greedy_sample(O.to_torch(sd_r), O.to_torch(f_np), d.T, synth.UNK_IDX, return_logprobs=True)
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, synth.UNK_IDX, weights_dtype="bf16")
    seq, att, lp = run_clone(eng)
    check_against_oracle(seq, att, lp, seq_o, att_o, logp_o, B, d.T, f"ragged B={B} N={N} F={F}")


# ------------------------------------------------------------------ 6. sampling, one caption per clip
def test_bf16_sampling_one_caption_per_clip_vs_the_reference_sampler(dev, lib):
    from helpers import to_dev
    from oracle import ref_cpu as O
    import sample_oracle as S
    import test_gpu_sampling as TS                       # its comparison and its tolerances
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np, _P, f = TS._inputs("cfg1")
    P_r = O.to_torch(rounded(sd))
    tau, seed = 0.8, 78
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, synth.UNK_IDX, sample_n=1, temperature=tau, seed=seed,
                       weights_dtype="bf16")
    assert eng.packed and eng.bf16w and eng.sampling
    for call in (1, 2):
        seq, att, lp = eng.run()
        with torch.no_grad():
            ref = S.sample(P_r, f, d.T, synth.UNK_IDX, 1, tau, seed, call)
        TS._compare(seq, att, lp, ref, f"cfg1 n=1 bf16 weights call {call}")


# ------------------------------------------------------------------ 7. plumbing
def sample_call(model, f, b, **kw):
    dummy = torch.zeros(f["fc_feats"].shape[0], 1, 1, device=f["fc_feats"].device)
    return model._sample(f, b["input_seq"], b["proposals"], b["gt_seq"], b["num"], b["box_mask"], b["gt_bboxs"], dummy, b["frm_mask"],
                         b["sample_idx"], f["pnt_mask"], **kw)


@pytest.mark.parametrize("graph", [False, True])
def test_model_decodes_with_bf16_weights_and_rebinds_on_a_switch(dev, lib, graph):
    from helpers import build_model, to_dev, model_call
    from cvc.decode import DecodeEngine, DecodeWeights
    d = dataclasses.replace(synth.CONFIGS["tiny"], B=5, R=64, A=32, E=32, V=97, T=6)
    sd = synth.hot_path_state_dict(d, 3)
    f, b = to_dev(synth.clip_features(d, 21), dev), to_dev(synth.label_glue_batch(d, 21), dev)
    model = build_model(d, sd, dev, hip_graph=graph, decode_weights="bf16")
    assert model.decode_weights_dtype == "bf16"
    with torch.no_grad():
        seq, att, none = model_call(model, f, b, True)
        assert none is None and model._engine_cache[1].weights_dtype == "bf16"
        want = run_clone(DecodeEngine(DecodeWeights(to_dev(sd, dev)), f, d.T, synth.UNK_IDX, weights_dtype="bf16"))
        assert torch.equal(seq, want[0]) and torch.equal(att, want[1])
        # the fp32 path before and after a bf16 decode on the same model: bit-identical, and every switch re-binds
        plain = build_model(d, sd, dev, hip_graph=graph)
        assert plain.decode_weights_dtype == "fp32"
        s0, a0, _ = model_call(plain, f, b, True)
        e0 = plain._engine_cache[1]
        assert e0.weights_dtype == "fp32"
        s1, a1, _ = sample_call(plain, f, b, decode_weights="bf16")
        e1 = plain._engine_cache[1]
        assert e1 is not e0 and e1.weights_dtype == "bf16"
        assert torch.equal(s1, seq) and torch.equal(a1, att)
        s2, a2, _ = sample_call(plain, f, b, decode_weights="fp32")
        assert plain._engine_cache[1] is not e1 and plain._engine_cache[1].weights_dtype == "fp32"
        assert torch.equal(s2, s0) and torch.equal(a2, a0)
        assert not torch.equal(a0, att)                   # (the two modes are different numbers)
        with pytest.raises(RuntimeError, match="weights_dtype"):
            sample_call(plain, f, b, decode_weights="fp16")
        with pytest.raises(RuntimeError, match="beam"):
            sample_call(plain, f, b, decode_weights="bf16", beam_size=3)


# ------------------------------------------------------------------ 8. refusals
def test_bf16_engine_refusals_launch_nothing(dev, lib):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d = dataclasses.replace(synth.CONFIGS["tiny"], B=5, R=64, A=32, E=32, V=97, T=6)
    W = DecodeWeights(to_dev(synth.hot_path_state_dict(d, 3), dev))
    f = to_dev(synth.clip_features(d, 21), dev)
    d65 = dataclasses.replace(d, B=65)
    f65 = to_dev(synth.clip_features(d65, 21), dev)
    d_odd = dataclasses.replace(d, R=40, A=16, E=16)
    W_odd = DecodeWeights(to_dev(synth.hot_path_state_dict(d_odd, 3), dev))
    f_odd = to_dev(synth.clip_features(d_odd, 21), dev)
    cases = [(W, f, dict(beam=3), "beam"), (W, f, dict(sample_n=2, temperature=1.0), "sample_n"), (W, f65, dict(), "64 rows"),
             (W, f, dict(path="tile"), "tile"), (W, f, dict(path="ring"), "ring"), (W, f, dict(embgate=False), "embgate"),
             (W_odd, f_odd, dict(), "multiples of 32")]
    for w, feats, kw, why in cases:
        eng = object.__new__(DecodeEngine)
        with pytest.raises(RuntimeError, match=why):
            eng.__init__(w, feats, d.T, synth.UNK_IDX, weights_dtype="bf16", **kw)
        assert not hasattr(eng, "_launches") and not hasattr(eng, "XA")          # refused before any buffer or launch list exists
    with pytest.raises(RuntimeError, match="weights_dtype"):
        DecodeEngine(W, f, d.T, synth.UNK_IDX, weights_dtype="fp8")
    for w in (W, W_odd):
        assert not any(hasattr(w, n) for n in ("pb_lang", "pb_att2", "p_lang", "p_att2"))   # and before any pack was built
