"""The fused greedy tail (DecodeEngine(tail="fused"); csrc/sel_keys.h): the vocabulary head that posts its candidates as 64-bit keys
(cvc_packed_linear_keys_fwd), the attention cell that decodes its word from them (cvc_packed_lstm_embgate_keys_fwd) and the one
launch per decode that writes words and log-probs (cvc_keys_finalize).

  1. the head against fp64, element-wise: the kept (max, sum-exp) records, the chosen word (a planted winner whose fp64 margin is
     asserted to be far above the bound: no case needs a tie referee) and its log-prob;
  2. the selection corners on integer-exact logits: word and log-prob bits against the launch tail (cvc_packed_linear_fwd's records
     + cvc_top2_final) in every case, the word against cvc_top2_unk on the same launch's logits wherever that selection agrees with
     cvc_top2_final (it does not where a row's best word other than UNK is -inf or NaN);
  3. the attention cell's key form against the word form, bit for bit;
  4. the engine: fused against launch, both against the CPU oracle, launch against the stored outputs of the commit before the
     switch existed (tests/golden/fused_tail_parent.npz, written by parent_outputs() below on that commit's library);
  5. graph replays and a change of features: a missed key reset shows there.

The head keeps the 32-row block form of cvc_packed_linear_fwd (one block shape; there is no per-launch batch split to cover)."""
import dataclasses
import inspect
import math
import os

import numpy as np
import pytest
import torch

from cvc import synth
from packed_gemm_cases import OP_TOL, linear_case, linear_operands, linear_ref, lstm_case, lstm_operands, run_linear, run_lstm, QuadOut
from attn_step_cases import close, nan_buf, same_bits, stream_handle

pytestmark = pytest.mark.gpu

SEQ_TOL = dict(rtol=1e-4, atol=1e-4)      # attention maps after T recurrent steps (tests/test_gpu_parity.py)
LOGPROB_TOL = 1e-4                        # tests/helpers.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_tail_parent.npz")
NO_KEY = 0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from cvc import hip
    hip.lib()
    assert hip.gemm_packed_split(-1) == 2
    return hip


# ------------------------------------------------------------------ keys on the host
def host_key(v, n):
    """sel_key of csrc/sel_keys.h for a python float v (taken as fp32) and a word index n"""
    if math.isnan(v) or v == -math.inf:
        return 0
    u = int(np.float32(v).view(np.uint32))
    if u == 0x80000000:
        u = 0
    u = (~u & 0xFFFFFFFF) if u & 0x80000000 else (u | 0x80000000)
    return (u << 32) | (0x7FFFFFFF - n)


def as_i64(k):
    return k - (1 << 64) if k >= (1 << 63) else k


# ------------------------------------------------------------------ callers
def run_keys_head(hip, o, unk, bias=True):
    """cvc_packed_linear_keys_fwd + cvc_keys_finalize (T = 1) -> (word [M] int64, logprob [M], ms [nblk, 64, 2], keys [4, 64], key_unk [64])"""
    L = hip.lib()
    M, V, K = o["M"], o["V"], o["K"]
    dev = o["w"].device
    nblk = (V + 31) // 32
    kbuf = torch.zeros(64 * 5, dtype=torch.int64, device=dev)
    ms = nan_buf(nblk, 64, 2, dev=dev)
    kp, up = kbuf.data_ptr(), kbuf.data_ptr() + 64 * 4 * 8
    rc = L.cvc_packed_linear_keys_fwd(o["wp"].data_ptr(), o["xq"].data_ptr(), K, o["b"].data_ptr() if bias else None, M, V, unk, kp, up,
                                      ms.data_ptr(), stream_handle())
    assert rc == 0
    word = torch.full((M,), -7, dtype=torch.int64, device=dev)
    lp = nan_buf(M, dev=dev)
    assert L.cvc_keys_finalize(kp, up, ms.data_ptr(), nblk, 1, M, unk, word.data_ptr(), lp.data_ptr(), stream_handle()) == 0
    torch.cuda.synchronize()
    return word, lp, ms, kbuf[:256].view(4, 64), kbuf[256:]


def top2_unk_word(hip, y, unk):
    """cvc_top2_unk on row-major logits y [M, V]"""
    M, V = y.shape
    word = torch.full((M,), -7, dtype=torch.int64, device=y.device)
    assert hip.lib().cvc_top2_unk(y.data_ptr(), M, V, unk, word.data_ptr(), 1, None, stream_handle()) == 0
    torch.cuda.synchronize()
    return word


# ------------------------------------------------------------------ 1. the head against fp64
@pytest.mark.parametrize("K", [32, 96, 2048])
def test_keys_head_vs_fp64(dev, lib, K):
    """M in {1, 31, 33, 64} x V in {7, 40, 77, 1000}: (max, sum-exp) per block against fp64 within the bound of the packed GEMM pins
    (OP_TOL), rows >= M untouched; the word: a planted winner (bias + 8 on the last word, and UNK planted 16 above it, so the UNK rule
    decides every row) whose fp64 margin over the runner-up is asserted to be > 1; its log-prob within LOGPROB_TOL."""
    worst = 0.0
    for V in (7, 40, 77, 1000):
        for M in (1, 31, 33, 64):
            c = linear_case(1000 + V + M, M, V, K)
            unk, win = 1, V - 1
            c["b"][win] += 8.0
            c["b"][unk] += 24.0
            o = linear_operands(c, dev, pad_nan=True)
            y64 = linear_ref(c["x"], c["w"], c["b"])
            others = y64.clone()
            others[:, unk] = -math.inf
            top = torch.sort(others, dim=1, descending=True).values
            assert int(others.argmax(1).ne(win).sum()) == 0 and float((top[:, 0] - top[:, 1]).min()) > 1.0
            assert float((y64[:, unk] - top[:, 0]).min()) > 1.0                     # UNK on top of every row
            word, lp, ms, keys, kunk = run_keys_head(lib, o, unk)
            tag = f"keys head M={M} V={V} K={K}"
            assert torch.equal(word.cpu(), torch.full((M,), win, dtype=torch.int64)), tag
            nblk = (V + 31) // 32
            pad = torch.full((M, nblk * 32), -math.inf, dtype=torch.float64)
            pad[:, :V] = y64
            pad = pad.view(M, nblk, 32)
            mx64 = pad.max(2).values
            se64 = torch.exp(pad - mx64.unsqueeze(2)).sum(2)
            got = ms[:, :M].permute(1, 0, 2).cpu()
            assert bool(torch.isnan(ms[:, M:]).all()), (tag, "record rows >= M were written")
            err = max(float((got[..., 0].double() - mx64).abs().max()), float((got[..., 1].double() - se64).abs().max()))
            worst = max(worst, err)
            close(got[..., 0], mx64.float(), err_msg=tag + ": max", **OP_TOL)
            close(got[..., 1], se64.float(), err_msg=tag + ": sum-exp", **OP_TOL)
            lp64 = torch.log_softmax(y64, 1)[:, win]
            assert float((lp.cpu().double() - lp64).abs().max()) <= LOGPROB_TOL, tag
            # the posted keys: the winner in the slot of its block, UNK's own key apart, nothing in rows >= M
            assert bool((keys[:, M:] == 0).all()) and bool((kunk[M:] == 0).all()), tag
            assert bool((kunk[:M] != 0).all()) and bool((keys[(win // 32) % 4, :M] != 0).all()), tag
    print(f"fused_tail keys head K={K}: max |err| of (max, sum-exp) = {worst:.3e}")


# ------------------------------------------------------------------ 2. corners, exact
def exact_operands(logits, bias, dev):
    """K = 32, x = the unit rows e_m, w[n, m] = logits[m, n]: row m's logits are logits[m] + bias exactly (one non-zero product)"""
    M, V = logits.shape
    assert M <= 32
    w = torch.zeros(V, 32)
    w[:, :M] = logits.t()
    x = torch.zeros(M, 32)
    x[torch.arange(M), torch.arange(M)] = 1.0
    return linear_operands(dict(M=M, V=V, K=32, w=w, x=x, b=bias.clone()), dev)


def check_corner(lib, o, unk, tag, want=None, top2_unk=True):
    """The fused head + finalize against the launch tail on the same operands (cvc_packed_linear_fwd's records merged by
    cvc_top2_final): the same word and the same log-prob bits (NaN for NaN); with top2_unk also against cvc_top2_unk on the same
    launch's row-major logits -- off only where that selection is known to differ from cvc_top2_final (a row whose best word other
    than UNK is -inf or NaN: cvc_top2_unk takes -inf words as candidates and leaves the range on NaN)."""
    from packed_gemm_cases import run_top2_final
    M, V = o["M"], o["V"]
    word, lp, _, _, _ = run_keys_head(lib, o, unk)
    rc, y, rec = run_linear(lib, o, want_y=True, want_rec=True)
    assert rc == 0
    rc, wf, lpf, _ = run_top2_final(lib, o["w"].device, rec, (V + 31) // 32, M, unk)
    assert rc == 0
    assert torch.equal(word, wf.view(-1)), (tag, "fused != cvc_top2_final", word.tolist(), wf.view(-1).tolist())
    same = (lp.view(torch.int32) == lpf.view(torch.int32)) | (torch.isnan(lp) & torch.isnan(lpf))
    assert bool(same.all()), (tag, "log-prob bits", lp.tolist(), lpf.tolist())
    if top2_unk:
        ref = top2_unk_word(lib, y[0].contiguous(), unk)
        assert torch.equal(word, ref), (tag, "fused != cvc_top2_unk", word.tolist(), ref.tolist())
    if want is not None:
        assert word.cpu().tolist() == want, (tag, word.tolist(), want)
    return word


@pytest.mark.parametrize("unk_last", [False, True])
def test_corners_exact_ties_and_unk(dev, lib, unk_last):
    """V = 300 (ten blocks, the last ragged: 12 columns), small integer logits.  Rows: equal maxima in different blocks and slots;
    in two blocks that share a slot (blocks 0 and 8 of 4 slots); in one block; UNK strictly best; UNK tied with a lower-indexed word; UNK tied
    with a higher-indexed word; UNK tied on both sides; UNK in the first block (unk = 1) or in the last, ragged one (unk = V - 1)."""
    V = 300
    unk = V - 1 if unk_last else 1
    lo, hi = (290, None) if unk_last else (0, 50)         # a word below / above UNK (UNK as the last word has nothing above it)
    rows, want = [], []

    def row(pairs, w):
        r = torch.full((V,), -3.0)
        for n, v in pairs:
            r[n] = v
        rows.append(r)
        want.append(w)

    row([(3, 5.0), (69, 5.0)], 3)                          # blocks 0 and 2
    row([(261, 5.0), (5, 5.0)], 5)                         # blocks 8 and 0: the same slot
    row([(40, 5.0), (45, 5.0)], 40)                        # one block, two waves
    row([(unk, 7.0), (200, 4.0), (100, 4.0)], 100)         # UNK strictly best -> the best other word, lower index of two
    row([(unk, 6.0), (lo, 6.0)], lo)                       # UNK tied with a lower-indexed word
    if hi is not None:
        row([(unk, 6.0), (hi, 6.0)], hi)                   # UNK tied with a higher-indexed word
        row([(unk, 6.0), (lo, 6.0), (hi, 6.0)], lo)
    row([(unk, 9.0)], 0 if unk != 0 else 1)                # every other word ties at -3: the lowest index that is not UNK
    o = exact_operands(torch.stack(rows), torch.zeros(V), dev)
    check_corner(lib, o, unk, f"ties unk={unk}", want)


def test_corners_special_values(dev, lib):
    """-inf, NaN and -0 arrive through the bias (a per-column term): one launch per pattern, every row of it a different UNK /
    winner arrangement where that matters.  -inf and NaN are never candidates, as in the records of the launch tail."""
    V, unk = 77, 1
    base = torch.full((4, V), -3.0)
    base[0, 70] = 2.0
    base[1, unk] = 5.0
    base[1, 33] = 1.0
    base[2, 0] = 0.0
    base[3, 76] = 4.0
    # -inf on a set of columns (rows of mixed -inf and finite logits)
    b = torch.zeros(V)
    b[[0, 5, 33, 64, 76]] = -math.inf
    check_corner(lib, exact_operands(base, b, dev), unk, "-inf columns", [70, 2, 2, 2])
    # UNK -inf too: the best of the finite words
    b[unk] = -math.inf
    check_corner(lib, exact_operands(base, b, dev), unk, "-inf columns and UNK", [70, 2, 2, 2])
    # every word -inf but UNK ("only UNK finite") -> UNK (cvc_top2_unk: the lowest -inf word)
    b = torch.full((V,), -math.inf)
    b[unk] = 0.0
    check_corner(lib, exact_operands(base, b, dev), unk, "only UNK finite", [unk] * 4, top2_unk=False)
    # every word -inf: no candidate -> 0
    check_corner(lib, exact_operands(base, torch.full((V,), -math.inf), dev), unk, "all -inf", [0, 0, 0, 0])
    # an all-NaN row -> 0
    check_corner(lib, exact_operands(base, torch.full((V,), math.nan), dev), unk, "all NaN", [0, 0, 0, 0])
    # NaN on some columns: never candidates (row 0's winner 70 is NaN: the best of the rest)
    b = torch.zeros(V)
    b[[70, 2]] = math.nan
    check_corner(lib, exact_operands(base, b, dev), unk, "NaN columns")
    # UNK finite, every other word NaN -> UNK (cvc_top2_unk leaves the range and falls back to word 0)
    b = torch.full((V,), math.nan)
    b[unk] = 1.0
    check_corner(lib, exact_operands(base, b, dev), unk, "only UNK a number", [unk] * 4, top2_unk=False)
    # -0 against +0: logits 0 + bias; -0 on the lower or on the higher index ties with +0 -> the lower index
    z = torch.full((2, V), -3.0)
    z[0, 10] = z[0, 50] = 0.0
    z[1, 10] = z[1, 50] = 0.0
    for neg in (10, 50):
        b = torch.zeros(V)
        b[neg] = -0.0
        check_corner(lib, exact_operands(z, b, dev), unk, f"-0 at {neg}", [10, 10])


def test_corners_one_word(dev, lib):
    """V = 1: UNK = 0 is the only word -> UNK"""
    o1 = exact_operands(torch.tensor([[2.0], [-1.0]]), torch.zeros(1), dev)
    check_corner(lib, o1, 0, "V = 1", [0, 0])


# ------------------------------------------------------------------ 3. the attention cell's key form
@pytest.mark.parametrize("M,w_cached", [(33, 0), (64, 1), (5, 0)])
def test_embgate_keys_form_is_the_word_form(dev, lib, M, w_cached):
    """cvc_packed_lstm_embgate_keys_fwd on hand-made keys against cvc_packed_lstm_embgate_ex_fwd on the words they encode, bit for
    bit: the winner in any slot, below a UNK key (UNK best -> the best other word), only a UNK key (-> UNK), no key (-> 0)."""
    R, K, V, unk = 64, 128, 50, 1
    c = lstm_case(77, M, R, K, V)
    g = torch.Generator().manual_seed(5)
    keys = np.zeros((4, 64), dtype=np.int64)
    kunk = np.zeros(64, dtype=np.int64)
    word = torch.zeros(M, dtype=torch.int64)
    for m in range(M):
        kind = m % 4
        w = int(torch.randint(2, V, (1,), generator=g))
        if kind in (0, 1):                                 # a winner and losers in other slots; kind 1: UNK above all of them
            slot = m % 4
            keys[slot, m] = as_i64(host_key(1.5, w))
            keys[(slot + 1) % 4, m] = as_i64(host_key(1.5, w + 1) if w + 1 < V else NO_KEY)      # same value, higher index
            keys[(slot + 3) % 4, m] = as_i64(host_key(-2.0, 0))
            if kind == 1:
                kunk[m] = as_i64(host_key(9.0, unk))
            word[m] = w
        elif kind == 2:
            kunk[m] = as_i64(host_key(-1.0, unk))
            word[m] = unk
        else:
            word[m] = 0
    c["word"] = word
    o = lstm_operands(c, dev)
    rc, h1, h2, co = run_lstm(lib, o, entry="embgate_ex", gb=True, tab=True, w_cached=w_cached)
    assert rc == 0
    kd, ud = torch.from_numpy(keys).to(dev), torch.from_numpy(kunk).to(dev)
    g1, g2, gc = QuadOut(R, dev, 0), QuadOut(R, dev, 0), QuadOut(R, dev, 0)
    p = lambda t: t.data_ptr()
    rc = lib.lib().cvc_packed_lstm_embgate_keys_fwd(p(o["wp"]), 0, p(o["xq"]), K, p(o["b_ih"]), p(o["b_hh"]), p(o["gate_bias"]), p(o["table"]),
                                                    p(kd), p(ud), unk, p(o["cq"]), M, R, g1.ptr, g2.ptr, gc.ptr, w_cached, stream_handle())
    torch.cuda.synchronize()
    assert rc == 0
    assert same_bits(g1.rows(M), h1.rows(M)) and same_bits(g2.rows(M), h2.rows(M)) and same_bits(gc.rows(M), co.rows(M))
    assert g1.rest_is_nan(M) and gc.rest_is_nan(M)


# ------------------------------------------------------------------ 4. the engine
DIMS = dict(N=7, F=5, R=64, A=64, E=64, V=77, T=4)
SEED = 4311


def engine_inputs(B, twins=False):
    """random checkpoint + features at the tiny dimensions; twins: every vocabulary row n >= 3 of the first 40 has a bit-equal twin
    37 rows further (another 32-row block; K = 64 is one chunk per wave, so equal rows give bit-equal logits) and UNK = 1 has the
    twins 38 and 75 -- exact ties at the top of every row, between blocks and with UNK"""
    d = dataclasses.replace(synth.CONFIGS["tiny"], B=B, **DIMS)
    sd, f_np = synth.hot_path_state_dict(d, SEED), synth.clip_features(d, SEED)
    if twins:
        w, b = sd["logit.weight"].copy(), sd["logit.bias"].copy()
        w[40:77], b[40:77] = w[3:40], b[3:40]
        w[38], b[38] = w[1], b[1]
        w[75], b[75] = w[1], b[1]
        sd["logit.weight"], sd["logit.bias"] = w, b
    return d, sd, f_np


def run_engine(dev, B, tail, twins=False, **kw):
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np = engine_inputs(B, twins)
    if "tail" in inspect.signature(DecodeEngine.__init__).parameters:
        kw["tail"] = tail
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), to_dev(f_np, dev), d.T, synth.UNK_IDX, **kw)
    seq, att = eng.run()
    torch.cuda.synchronize()
    return eng, seq.clone(), att.clone(), eng.logprob.t().clone()


def parent_outputs(dev):
    """what the golden file holds: the launch schedule's outputs for B = 3 and 64 (run on the commit before the switch: every engine
    there is the launch schedule)"""
    out = {}
    for B in (3, 64):
        _, seq, att, lp = run_engine(dev, B, "launch")
        out[f"b{B}.seq"], out[f"b{B}.att"], out[f"b{B}.logprob"] = seq.cpu().numpy(), att.cpu().numpy(), lp.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def oracle_runs():
    from oracle import ref_cpu as O
    out = {}
    for B in (3, 64):
        d, sd, f_np = engine_inputs(B)
        with torch.no_grad():
            out[B] = O.greedy_sample(O.to_torch(sd), O.to_torch(f_np), d.T, synth.UNK_IDX, return_logprobs=True)
    return out


@pytest.mark.parametrize("B", [3, 64])
def test_engine_fused_vs_launch_vs_oracle(dev, lib, oracle_runs, B):
    from helpers import tie_aware_seq_equal
    e_l, seq_l, att_l, lp_l = run_engine(dev, B, "launch")
    e_f, seq_f, att_f, lp_f = run_engine(dev, B, "fused")
    assert e_f.fused_tail and not e_l.fused_tail
    names_f, names_l = [n for n, _, _ in e_f._python_launches()], [n for n, _, _ in e_l._python_launches()]
    assert "word_select" not in names_f and names_f.count("tail_finalize") == 1 and names_l.count("word_select") == e_l.T
    # the same logits bit for bit, the same rule: the same words, hence the same attention maps bit for bit
    assert torch.equal(seq_f, seq_l) and same_bits(att_f, att_l)
    assert same_bits(lp_f, lp_l)            # (cvc_keys_finalize sums the records as top2_final_kernel does)
    seq_o, att_o, _, logp_o = oracle_runs[B]
    for seq, att in ((seq_f, att_f), (seq_l, att_l)):
        n_exact = tie_aware_seq_equal(seq.cpu().numpy(), seq_o.numpy(), logp_o.numpy())
        assert n_exact >= 0.95 * B * e_f.T
        # at these dimensions and this seed every word equals the oracle's: the attention maps and the log-probs are compared on
        # every clip (a tie flip would make the clips after it incomparable -- then this has to fail and be looked at, not skip)
        assert n_exact == B * e_f.T, (n_exact, B * e_f.T)
        close(att, att_o, **SEQ_TOL)
        assert logp_o.dim() == 3
        close(lp_f, logp_o.gather(2, seq_o.unsqueeze(2)).squeeze(2), rtol=0, atol=LOGPROB_TOL)
    # driver and Python launch list agree
    e_p, seq_p, att_p, lp_p = run_engine(dev, B, "fused", driver=False)
    assert torch.equal(seq_p, seq_f) and same_bits(att_p, att_f) and same_bits(lp_p, lp_f)


@pytest.mark.parametrize("B", [3, 64])
def test_engine_fused_vs_launch_on_exact_ties(dev, lib, B):
    """twin vocabulary rows: the top of every row is an exact tie between two blocks (and, where UNK leads, between UNK and two
    words): both tails resolve it to the lower index"""
    _, seq_l, att_l, _ = run_engine(dev, B, "launch", twins=True)
    _, seq_f, att_f, _ = run_engine(dev, B, "fused", twins=True)
    assert torch.equal(seq_f, seq_l) and same_bits(att_f, att_l)
    assert int(seq_f.max()) < 40 and not bool((seq_f == synth.UNK_IDX).any())          # never the higher twin, never UNK


def test_engine_launch_is_the_parent_bit_for_bit(dev, lib):
    """tail="launch" against the stored outputs of the commit before the switch existed.  A pin of one moment: a later change that
    legitimately reorders a sum in any launch of the launch schedule changes these bits -- regenerate the file with
    parent_outputs() on that change (np.savez(GOLDEN, **parent_outputs(dev))) or retire this test then."""
    g = np.load(GOLDEN)
    got = parent_outputs(dev)
    for k in g.files:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(g[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


def test_engine_refusals(dev, lib):
    with pytest.raises(RuntimeError, match="tail"):
        run_engine(dev, 3, "fused", temperature=1.0)
    with pytest.raises(RuntimeError, match="tail"):
        run_engine(dev, 3, "fused", beam=2)
    with pytest.raises(RuntimeError, match="tail"):
        run_engine(dev, 3, "both")


# ------------------------------------------------------------------ 5. replay
def test_replay_and_new_features(dev, lib):
    """the captured graph three times, other features, the first features again: bitwise equal outputs for equal features (the keys
    of all T steps are cleared inside the graph: a missed reset would leave the previous decode's maxima in place)"""
    from helpers import to_dev
    from cvc.decode import DecodeEngine, DecodeWeights
    d, sd, f_np = engine_inputs(64)
    f1 = to_dev(f_np, dev)
    f2 = to_dev(synth.clip_features(d, SEED + 1), dev)
    eng = DecodeEngine(DecodeWeights(to_dev(sd, dev)), f1, d.T, synth.UNK_IDX, own_features=True, tail="fused").capture()
    outs = []
    for _ in range(3):
        seq, att = eng.run()
        outs.append((seq.clone(), att.clone(), eng.logprob.clone()))
    eng.load_features(f2)
    seq2, att2 = (t.clone() for t in eng.run())
    eng.load_features(f1)
    seq, att = eng.run()
    outs.append((seq.clone(), att.clone(), eng.logprob.clone()))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and same_bits(o[1], outs[0][1]) and same_bits(o[2], outs[0][2])
    assert not torch.equal(att2, outs[0][1])
    # ... and the other features' outputs are those of a fresh launch-tail engine on them
    ref = DecodeEngine(DecodeWeights(to_dev(sd, dev)), f2, d.T, synth.UNK_IDX, tail="launch")
    seq_r, att_r = ref.run()
    assert torch.equal(seq2, seq_r) and same_bits(att2, att_r)
