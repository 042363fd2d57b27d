"""CPU tests of what tests/test_gpu_packed_gemm.py relies on (no GPU): the fp64 restatements of tests/packed_gemm_cases.py against
torch.nn.LSTMCell in double and torch.log_softmax / topk, the record restatement merged on the host against the direct answer
(ties, UNK rule and the random cases' margin included), the K-loop sweep against the constants of csrc/gemm_packed.hip, and the
argument checks of the fp32 entry points, which answer CVC_E_BADARG before anything touches a device."""
import ctypes
import math

import pytest
import torch

import packed_gemm_cases as P
from packed_gemm_cases import E_BADARG, NO_INDEX


# ------------------------------------------------------------------ restatements
@pytest.mark.parametrize("M,R,K", [(5, 40, 96), (64, 64, 128)])
def test_lstm_restatement_is_nn_lstmcell_in_double(M, R, K):
    """lstm_ref with x = [input | h_prev], w = [W_ih | W_hh] and both biases is torch.nn.LSTMCell (gate order i, f, g, o); the
    per-row terms are plain additions to the pre-activations"""
    c = P.lstm_case(M + R, M, R, K)
    Ki = K - R
    cell = torch.nn.LSTMCell(Ki, R).double()
    with torch.no_grad():
        cell.weight_ih.copy_(c["w"][:, :Ki].double()); cell.weight_hh.copy_(c["w"][:, Ki:].double())
        cell.bias_ih.copy_(c["b_ih"].double()); cell.bias_hh.copy_(c["b_hh"].double())
        h, cc = cell(c["x"][:, :Ki].double(), (c["x"][:, Ki:].double(), c["c_prev"].double()))
    ref = P.lstm_ref(c["x"], c["w"], c["c_prev"], P.lstm_terms(c))
    torch.testing.assert_close(ref["h"], h, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["c"], cc, rtol=1e-12, atol=1e-12)
    # per-row terms: folding them into the bias of a one-row cell gives the same row
    full = P.lstm_ref(c["x"], c["w"], c["c_prev"], P.lstm_terms(c, True, True, True))
    m = M - 1
    extra = c["gate_bias"][m].double() + c["table"][c["word"][m]].double()
    one = P.lstm_ref(c["x"][m:m + 1], c["w"], c["c_prev"][m:m + 1], [c["b_ih"].double() + extra, c["b_hh"]])
    torch.testing.assert_close(full["h"][m:m + 1], one["h"], rtol=1e-12, atol=1e-12)
    assert full["gates"].shape == (M, 4 * R) and bool(((full["gates"][:, :2 * R] > 0) & (full["gates"][:, :2 * R] < 1)).all())
    assert c["word"][0] == 0 and c["word"][M - 1] == c["V"] - 1


@pytest.mark.parametrize("V", [33, 50, 300, 8190])
def test_record_restatement_merged_on_the_host_is_log_softmax_and_topk(V):
    """block_records + merge_records against torch.topk / log_softmax on the same fp64 logits, with and without UNK on top"""
    c = P.linear_case(V, 9, V, 64)
    y = P.linear_ref(c["x"], c["w"], c["b"])
    rec = P.block_records(y)
    nblk = (V + 31) // 32
    assert rec["v1"].shape == (9, nblk)
    top = y.topk(2, 1)
    lsm = torch.log_softmax(y, 1)
    word, lp, i1, i2 = P.merge_records(rec, -1)
    assert torch.equal(i1, top.indices[:, 0]) and torch.equal(i2, top.indices[:, 1]) and torch.equal(word, i1)
    torch.testing.assert_close(lp, lsm.gather(1, i1.view(-1, 1)).view(-1), rtol=1e-12, atol=1e-12)
    unk = int(top.indices[0, 0])
    word, lp, _, _ = P.merge_records(rec, unk)
    w_ref, lp_ref, _ = P.select_ref(y, unk)
    assert torch.equal(word, w_ref) and int(word[0]) == int(top.indices[0, 1])
    torch.testing.assert_close(lp, lp_ref, rtol=1e-12, atol=1e-12)
    if V % 32 == 1:                                            # one valid column in the last block
        assert bool((rec["i2"][:, -1] == NO_INDEX).all()) and bool((rec["v2"][:, -1] == -math.inf).all()) and bool((rec["se"][:, -1] == 1).all())
    # the sum of a block is over its valid columns only
    b0 = torch.exp(y[:, :32] - y[:, :32].max(1, keepdim=True).values).sum(1)
    torch.testing.assert_close(rec["se"][:, 0], b0, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("place,V,K,pair", P.TIE_PLACES)
def test_exact_cases_are_exact_and_their_ties_go_to_the_lowest_index(place, V, K, pair):
    """the integer cases: fp32 and fp64 products agree exactly, the planted scenarios give the stated top two, and the host merge of
    the records gives the direct answer with every planted column named UNK in turn"""
    c = P.exact_case(77, 8, V, K, pair)
    y = P.linear_ref(c["x"], c["w"], c["b"])
    assert torch.equal((c["x"] @ c["w"].t() + c["b"]).double(), y) and float(y.abs().max()) < 2 ** 24
    a, b, t = c["a"], c["b_col"], c["t"]
    assert c["top1"].tolist() == [a, t, b, a] * 2 and c["top2"].tolist() == [b, a, a, b] * 2
    assert bool((y[0::4, a] == y[0::4, b]).all()) and bool((y[1::4, a] == y[1::4, b]).all()) and bool((y[3::4, a] == y[3::4, t]).all())
    order = torch.sort(y, dim=1, descending=True, stable=True).indices
    assert torch.equal(order[:, 0], c["top1"]) and torch.equal(order[:, 1], c["top2"])
    rec = P.block_records(y.float())
    for unk in (-1, a, b, t):
        word, lp, i1, i2 = P.merge_records(rec, unk)
        assert torch.equal(i1, c["top1"]) and torch.equal(i2, c["top2"])
        w_ref, lp_ref, _ = P.select_ref(y, unk)
        assert torch.equal(word, w_ref) and torch.equal(word, torch.where(c["top1"] == unk, c["top2"], c["top1"]))
        torch.testing.assert_close(lp, lp_ref, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("unk", [0, 1, 99])
def test_unk_rule_of_the_restatements(unk):
    """UNK alone on top -> the runner-up and its log-prob; UNK tied with a higher index -> that index; UNK not on top -> no effect"""
    c = P.exact_case(78 + unk, 8, 100, 64, (5, 40), t=unk)
    y = P.linear_ref(c["x"], c["w"], c["b"])
    for word, lp in (P.select_ref(y, unk)[:2], P.merge_records(P.block_records(y), unk)[:2]):
        assert word.tolist() == [5, 5, 40, 5] * 2
        lsm = torch.log_softmax(y, 1)
        torch.testing.assert_close(lp, lsm.gather(1, word.view(-1, 1)).view(-1), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(lp[1::4], lsm[1::4, unk] - 1.0, rtol=1e-12, atol=1e-12)
    assert P.select_ref(y, -1)[0].tolist() == [5, unk, 40, min(5, unk)] * 2


@pytest.mark.parametrize("V,seed", P.MERGE_CASES)
def test_random_merge_cases_have_a_deciding_margin_on_every_row(V, seed):
    """what test_merged_word_and_logprob_on_random_rows asserts first, without a GPU: no row is excluded there"""
    c, unk = P.merge_case(V, seed)
    y = P.linear_ref(c["x"], c["w"], c["b"])
    word, _, margin = P.select_ref(y, unk)
    assert float(margin.min()) >= 1e-3
    on_top = int((y.argmax(1) == unk).sum())
    assert 0 < on_top < 64 and not bool((word == unk).any())
    w2, lp2, _, _ = P.merge_records(P.block_records(y), unk)
    assert torch.equal(w2, word)


def test_negative_vocabulary_cases_would_lose_to_a_padding_column():
    for V in (33, 50, 8190):
        c = P.negative_vocab_case(V + 5, 37, V)
        assert float(P.linear_ref(c["x"], c["w"], c["b"]).max()) < -1.0


# ------------------------------------------------------------------ the sweep reaches every branch of the register ring
def test_k_sweep_reaches_every_branch_of_the_ring_in_every_mode():
    """From CVC_PACKED_DEPTH / CVC_PACKED_DEPTH8 of the source: over the sweep, the waves of a launch take the short loop with 0, 1
    and DEPTH - 1 chunks, "prefill + drain only" at both of its ends, one pass of the steady loop with every drain length
    DEPTH - 1 .. 2 DEPTH - 2, and two passes; the ksplit = 1 launch with ten workgroups starts its walk at different chunks."""
    modes, rot = P.source_constants()
    assert modes == {0: (4, 4), 1: (4, 4), 2: (8, 3)} and rot == 5          # what the comments of the GPU file state
    for mode, (nw, depth) in modes.items():
        seen = set()
        for nchunk in P.SWEEP_CHUNKS:
            seen |= {P.ring_path(n, depth) for n in P.wave_counts(nchunk, nw)}
        want = {("short", 0, n) for n in (0, 1, depth - 1)} | {("ring", 0, depth), ("ring", 0, 2 * depth - 2)}
        want |= {("ring", 1, d) for d in range(depth - 1, 2 * depth - 1)} | {("ring", 2, depth - 1)}
        assert want <= seen, (mode, sorted(want - seen))
        n_max = max(P.wave_counts(max(P.SWEEP_CHUNKS), nw))
        assert len({(rot * b) % n_max for b in range(8)}) > 1
    # the thresholds as the issue lists them
    assert [P.ring_path(n, 3)[:2] for n in (2, 3, 4, 5, 7, 8)] == [("short", 0), ("ring", 0), ("ring", 0), ("ring", 1), ("ring", 1), ("ring", 2)]
    assert [P.ring_path(n, 4)[:2] for n in (3, 4, 6, 7, 10, 11)] == [("short", 0), ("ring", 0), ("ring", 0), ("ring", 1), ("ring", 1), ("ring", 2)]


# ------------------------------------------------------------------ argument checks, no device
def test_fp32_entry_points_refuse_bad_arguments_before_touching_a_device():
    """Never-dereferenced addresses: every call below is answered with CVC_E_BADARG."""
    import build_hip
    from cvc import hip
    build_hip.build(verbose=False)
    L = hip.lib()
    p = ctypes.c_void_p(4096)
    BAD = E_BADARG
    lstm = lambda wp=p, xq=p, K=64, c=p, M=4, R=16, co=p: L.cvc_packed_lstm_fwd(wp, xq, K, None, None, None, c, M, R, p, None, co, None)
    eg = lambda wp=p, xq=p, K=64, tab=p, word=p, c=p, M=4, R=16, co=p: L.cvc_packed_lstm_embgate_fwd(
        wp, xq, K, None, None, None, tab, word, c, M, R, p, None, co, None)
    ex = lambda wp=p, stride=0, xq=p, K=64, tab=p, word=p, c=p, M=4, R=16, co=p: L.cvc_packed_lstm_embgate_ex_fwd(
        wp, stride, xq, K, None, None, None, tab, word, c, M, R, p, None, co, 0, None)
    late = lambda wp=p, stride=16 * 128, xq=p, K=64, c=p, M=4, R=16, co=p: L.cvc_packed_lstm_late_fwd(
        wp, stride, xq, K, None, None, None, c, M, R, p, None, co, None, None)
    for f in (lstm, eg, ex, late):
        assert f(wp=None) == BAD and f(xq=None) == BAD and f(c=None) == BAD and f(co=None) == BAD, f
        assert f(K=48) == BAD and f(K=0) == BAD                            # K a multiple of 32, at least one chunk
        assert f(M=0) == BAD and f(M=65) == BAD
        assert f(R=0) == BAD and f(R=12) == BAD
    assert eg(tab=None) == BAD and eg(word=None) == BAD and ex(tab=None) == BAD and ex(word=None) == BAD
    # w_blk_stride: at least the contraction length's K / 4 * 128 floats, and a multiple of 4 (the late form takes no 0 = dense)
    assert ex(stride=16 * 128 - 4) == BAD and ex(stride=16 * 128 + 2) == BAD
    assert late(stride=16 * 128 - 4) == BAD and late(stride=16 * 128 + 2) == BAD and late(stride=0) == BAD

    def step(**kw):
        s = hip.LstmStep()
        s.wp = s.xq = s.c_prev = s.c_out = s.h_out = 4096
        s.K, s.M, s.R = 64, 4, 16
        for k, v in kw.items():
            setattr(s, k, v)
        return L.cvc_packed_lstm_step_fwd(s, None)
    assert L.cvc_packed_lstm_step_fwd(None, None) == BAD
    assert step(wp=None) == BAD and step(xq=None) == BAD and step(c_prev=None) == BAD and step(c_out=None) == BAD
    assert step(K=48) == BAD and step(K=0) == BAD and step(M=0) == BAD and step(M=65) == BAD and step(R=0) == BAD and step(R=12) == BAD
    assert step(row_bias=4096) == BAD and step(row_index=4096) == BAD      # table and index come together
    assert step(p=1.0) == BAD and step(p=-0.5) == BAD

    lin = lambda wp=p, xq=p, K=64, M=4, N=50, ks=1, y=p, ldy=50, top2=None: L.cvc_packed_linear_fwd(wp, xq, K, None, M, N, ks, y, ldy, top2, None)
    assert lin(wp=None) == BAD and lin(xq=None) == BAD
    assert lin(K=40) == BAD and lin(K=0) == BAD and lin(M=0) == BAD and lin(M=65) == BAD and lin(N=0) == BAD
    assert lin(ks=0) == BAD and lin(ks=2, top2=p) == BAD and lin(y=None) == BAD          # no slices; records need whole K; no output
    assert lin(ldy=49) == BAD and lin(ldy=49, top2=p) == BAD                             # rows of y would overlap

    fin = lambda part=p, nblk=2, M=4, word=p, ws=1, table=p, E=8, emb=p, ld=0: L.cvc_top2_final(part, nblk, M, 1, word, ws, None, table, E, emb, ld, None)
    assert fin(part=None) == BAD and fin(word=None) == BAD and fin(nblk=0) == BAD and fin(M=0) == BAD and fin(M=65) == BAD
    assert fin(ws=0) == BAD                                                              # word_stride >= 1
    assert fin(table=None) == BAD and fin(E=0) == BAD and fin(E=6) == BAD                # emb_out: a table and whole float4s
    assert fin(ld=6) == BAD and fin(ld=4) == BAD                                         # emb_ld: 0 (quad) or a multiple of 4 >= E
