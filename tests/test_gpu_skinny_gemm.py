"""GPU tests (pytest -m gpu) of the skinny concat-GEMM's entry points (csrc/gemm_skinny.hip: cvc_linear_fwd,
cvc_linear_splitk_fwd, cvc_linear_top2_fwd, cvc_lstm_cell_fwd), each called through the C-ABI as cvc/decode/path_ring.py,
csrc/decode_driver.hip and csrc/train_driver.hip call it and compared ELEMENT-WISE with a torch fp64 restatement
(tests/packed_gemm_cases.py, tests/skinny_gemm_cases.py) on the same fp32 inputs cast up -- on BOTH kernels of the file: the LDS-DMA
ring kernel ("ring": the library's own choice wherever every width is a multiple of 32) and the direct-load kernel ("direct":
cvc_gemm_force_generic(1), and the library's choice for every other shape).

Every output buffer is pre-filled with NaN and is one row (plane, record block) larger than the contract writes: an element the
contract says is written is compared, every other one must still be NaN.  Tolerance: OP_TOL (rtol = atol = 2e-5), with weights
scaled by 1 / sqrt(K) and N(0, 1) activations, so pre-activations have unit scale at every K.  Every other comparison is bitwise
or exact; two launches of one case agree bit for bit."""
import math

import pytest
import torch

import packed_gemm_cases as P
import skinny_gemm_cases as S
from skinny_gemm_cases import E_BADARG, E_TOOBIG, OP_TOL, all_nan, close, nan_buf, same_bits

pytestmark = pytest.mark.gpu

KERNELS = ("ring", "direct")
ROWS = (1, 32, 33, 64)              # one row tile (MT = 1) and two (MT = 2): the tile boundary and its far ends


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from cvc import hip
    hip.lib()   # fails loudly if the extension is missing
    return hip


def on(dev, c, *names):
    return [c[n].to(dev) for n in names]


def assert_modes_agree(tag, kern, outs):
    """outs[mode] = list of output tensors.  The ring kernel has one template for modes 1 and 2 (SPLIT = true); the direct-load
    kernel has one arithmetic (fp32 MFMA) whatever the mode"""
    pairs = ((1, 2),) if kern == "ring" else ((0, 1), (1, 2))
    for a, b in pairs:
        assert all(same_bits(x, y) for x, y in zip(outs[a], outs[b])), (tag, kern, f"modes {a} and {b} differ")


def both_forms(lib, dev, tag, lstm, lin, kernels, rows, views=False, ldy_extra=4):
    """The comparisons of sections 1 and 2 on rows [0, M) of an LSTM case and a linear case, each (case, segments, x_eff), for
    M in rows: in modes 0, 1, 2 on every kernel of `kernels`, cvc_lstm_cell_fwd (b_ih, b_hh, gates_out) and cvc_linear_fwd (bias and
    a different bias2, as gate_fc passes them; ldy = Nout + ldy_extra) against fp64 within OP_TOL, two launches bitwise equal, the
    modes bitwise equal where they share a template.  -> {(kernel, form, M): outputs of mode 2}"""
    (cc, csegs, cx), (lc, lsegs, lx) = lstm, lin
    R, V = cc["R"], lc["V"]
    b2 = S.second_bias(lc)
    cref = P.lstm_ref(cx, cc["w"], cc["c_prev"], P.lstm_terms(cc))
    lref = P.linear_ref(lx, lc["w"], lc["b"]) + b2.double()
    b_ih, b_hh, c_prev = on(dev, cc, "b_ih", "b_hh", "c_prev")
    bias, bias2 = lc["b"].to(dev), b2.to(dev)
    kept = {}
    for M in rows:
        cds, lds = S.DevSegs(lib, cc, csegs, dev, (0, M), views), S.DevSegs(lib, lc, lsegs, dev, (0, M), views)
        cp = c_prev[:M].contiguous()
        for kern in kernels:
            couts, louts = {}, {}
            for mode in (0, 1, 2):
                t = f"{tag} {kern} mode={mode} M={M}"
                with P.split_mode(lib, mode), S.kernel(lib, kern):
                    rc, *outs = S.run_lstm(lib, cds, R, cp, b_ih, b_hh)
                    rc2, *again = S.run_lstm(lib, cds, R, cp, b_ih, b_hh)
                    rc3, y = S.run_linear(lib, lds, V, bias, bias2, ldy=V + ldy_extra)
                    rc4, y2 = S.run_linear(lib, lds, V, bias, bias2, ldy=V + ldy_extra)
                assert (rc, rc2, rc3, rc4) == (0, 0, 0, 0), (t, rc, rc2, rc3, rc4)
                S.check_lstm(t + " lstm", outs, {k: v[:M] for k, v in cref.items()}, M)
                S.check_linear(t + " linear", y, lref[:M], M, V)
                assert all(same_bits(a, b) for a, b in zip(outs, again)) and same_bits(y, y2), (t, "two launches of one case differ")
                couts[mode], louts[mode] = outs, [y]
            assert_modes_agree(tag + " lstm", kern, couts)
            assert_modes_agree(tag + " linear", kern, louts)
            kept[kern, "lstm", M], kept[kern, "linear", M] = couts[2], louts[2]
    return kept


# ------------------------------------------------------------------ 1. the K loop: every branch, both kernels, all three modes
# Wave w of NW takes chunks w, w + NW, ... of the K / 32 chunks of a segment: n_my = ceil((K / 32 - w) / NW).
# Ring kernel, NW = 4, RING = 3: n_my = 0 skips the segment; 1, 2, 3 run the drain alone; from 4 the steady loop (two chunks a pass)
# runs while c + 3 < n_my and leaves 2 (n_my even) or 3 (odd) chunks to the drain: one pass at 4 and 5, two at 6 and 7.
#   K / 32 -> n_my of waves 0..3:  1 (1,0,0,0)  3 (1,1,1,0)  6 (2,2,1,1)  11 (3,3,3,2)  14 (4,4,3,3)  18 (5,5,4,4)  23 (6,6,6,5)  27 (7,7,7,6)
# Direct-load kernel, NW = 8, two fragment sets: the same sweep gives n_my = 0 .. 4 (27 -> 4,4,4,3,3,3,3,3), odd counts leaving
# its two-step loop in the middle and even ones at its head.  tests/test_skinny_gemm_cpu.py checks both against the source.
# R = 40: five workgroups; Nout = 300: ten, the last with 12 columns.  A skipped or doubled chunk moves a pre-activation by
# about 1 / sqrt(K / 32) >= 0.19, four orders above OP_TOL.
@pytest.mark.parametrize("nchunk", S.SWEEP_CHUNKS)
def test_k_loop_every_branch_of_both_kernels_in_every_mode_vs_fp64(dev, lib, nchunk):
    K = nchunk * 32
    cc, lc = P.lstm_case(3000 + nchunk, 64, 40, K), P.linear_case(4000 + nchunk, 64, 300, K)
    both_forms(lib, dev, f"k_loop K/32={nchunk}", (cc, *S.split_segments(cc, (K,))), (lc, *S.split_segments(lc, (K,))), KERNELS, ROWS)


# ------------------------------------------------------------------ 2. segments
# (name, widths, gather segments, views, kernels).  Chunk counts (1, 6, 3, 11): wave 0 of the ring kernel restarts its pipeline with
# n_my = 1, 2, 1, 3 and wave 3 with 0 (skipped), 1, 0, 2.  Two gather segments and every width that is no multiple of 32 are the
# direct-load kernel's by the library's own choice: "ring" (no forcing) must then give the forced launch's bits.
SEGMENT_CASES = [
    ("four_segments", (32, 192, 96, 352), (), False, KERNELS),
    ("gather_first", (64, 96, 32), (0,), False, KERNELS),
    ("gather_middle", (64, 96, 32), (1,), False, KERNELS),
    ("gather_last", (64, 96, 32), (2,), False, KERNELS),
    ("column_views", (96, 64), (), True, KERNELS),
    ("column_views_gather", (64, 96, 32), (1,), True, KERNELS),
    ("two_gathers", (64, 96, 32), (0, 2), False, None),
    ("ragged_4", (4,), (), False, None), ("ragged_20", (20,), (), False, None), ("ragged_36", (36,), (), False, None),
    ("ragged_100", (100,), (), False, None), ("ragged_36_20", (36, 20), (), False, None), ("ragged_128_4_100", (128, 4, 100), (), False, None),
    ("ragged_views_gather", (36, 20), (1,), True, None),
]


@pytest.mark.parametrize("name,ks,gather,views,kernels", SEGMENT_CASES, ids=[c[0] for c in SEGMENT_CASES])
def test_segments_gathers_views_and_ragged_widths_vs_fp64(dev, lib, name, ks, gather, views, kernels):
    """the comparisons of section 1 on multi-segment calls: the table of a gather segment has 50 rows, indices 0 and 49 and
    negative entries; views: activations, table and weights are column blocks of wider NaN-filled tensors"""
    K = sum(ks)
    for M in ROWS:
        cc, lc = P.lstm_case(5000 + K + M, M, 40, K), P.linear_case(6000 + K + M, M, 300, K)
        csegs, cx = S.split_segments(cc, ks, gather)
        lsegs, lx = S.split_segments(lc, ks, gather)
        if gather:
            assert bool((csegs[gather[0]]["table"][csegs[gather[0]]["idx"]] < 0).any()), "the ReLU would not matter"
            assert 0 in lsegs[gather[0]]["idx"] or M == 1
            assert 49 in lsegs[gather[0]]["idx"]
        kept = both_forms(lib, dev, f"segments {name}", (cc, csegs, cx), (lc, lsegs, lx), kernels or KERNELS, (M,), views)
        if kernels is None:              # not a ring shape: the library's choice IS the direct-load kernel
            for form in ("lstm", "linear"):
                assert all(same_bits(a, b) for a, b in zip(kept["ring", form, M], kept["direct", form, M])), (name, form, M, "not the direct-load kernel's bits")


# ------------------------------------------------------------------ 3. split-K
# Slice s of ksplit takes chunks [nch s / ksplit, nch (s + 1) / ksplit) of EVERY segment, nch = k / 32 in the ring kernel and
# ceil(k / 32) with the tail clamped to k in the direct-load kernel.  K = 32 with ksplit = 8: only slice 7 owns a chunk; K = 96 with
# ksplit = 64: slices 21, 42, 63; (96, 160) with ksplit = 8: slice s owns chunks of segment 0 only for s = 2, 5, 7.  k = 100 over 3
# slices: nch = 4 -> chunks [0, 1), [1, 2), [2, 4): 32, 32 and 36 columns.
SPLITK = [(ks, ksplit, KERNELS) for ks in ((32,), (96,), (352,), (96, 160)) for ksplit in (1, 2, 3, 8, 64)] + [((100,), 3, ("direct",))]


@pytest.mark.parametrize("ks,ksplit,kernels", SPLITK)
def test_split_k_every_slice_vs_fp64_on_its_own_chunks(dev, lib, ks, ksplit, kernels):
    """every slice against the fp64 product over exactly its chunks of every segment, the bias in slice 0 only, a slice without a
    chunk written as exact zeros (slice 0: the bias itself), the fixed-order fp32 sum of the slices against the full product; plane
    `ksplit` of the buffer untouched; all three modes"""
    M, V, K = 33, 72, sum(ks)
    c = P.linear_case(7000 + K + ksplit, M, V, K)
    segs, x_eff = S.split_segments(c, ks)
    ds = S.DevSegs(lib, c, segs, dev)
    (bias,) = on(dev, c, "b")
    full = P.linear_ref(x_eff, c["w"], c["b"])
    for kern in kernels:
        refs, empty = S.slice_refs(c, segs, x_eff, ksplit, kern)
        if (ks, ksplit) == ((32,), 8):
            assert empty == [True] * 7 + [False]
        if (ks, ksplit) == ((96,), 64):
            assert [s for s in range(64) if not empty[s]] == [21, 42, 63]
        outs = {}
        for mode in (0, 1, 2):
            tag = f"split_k ks={ks} ksplit={ksplit} {kern} mode={mode}"
            with P.split_mode(lib, mode), S.kernel(lib, kern):
                rc, y = S.run_splitk(lib, ds, V, ksplit, bias)
                rc2, y2 = S.run_splitk(lib, ds, V, ksplit, bias)
            assert rc == 0 and rc2 == 0, (tag, rc, rc2)
            assert same_bits(y, y2), (tag, "two launches of one case differ")
            assert all_nan(y[ksplit]) and bool(torch.isfinite(y[:ksplit]).all()), (tag, "a plane was left unwritten, or one too many written")
            err = 0.0
            for s in range(ksplit):
                if empty[s]:
                    assert torch.equal(y[s], bias.expand(M, V) if s == 0 else torch.zeros(M, V, device=dev)), (tag, s, "empty slice")
                err = max(err, float((y[s].double().cpu() - refs[s]).abs().max()))
                close(y[s], refs[s].float(), err_msg=f"{tag} slice {s}", **OP_TOL)
            total = y[0].clone()
            for s in range(1, ksplit):
                total = total + y[s]
            print(f"skinny_gemm {tag}: slices max |err| = {err:.3e}, sum max |err| = {float((total.double().cpu() - full).abs().max()):.3e}")
            close(total, full.float(), err_msg=tag + " sum of the slices", **OP_TOL)
            outs[mode] = [y]
        assert_modes_agree(f"split_k ks={ks} ksplit={ksplit}", kern, outs)


# ------------------------------------------------------------------ 4. fused records
def records_of(lib, dev, c, kern, mode, want_y=True, ks=None):
    segs, x_eff = S.split_segments(c, ks or (c["K"],))
    ds = S.DevSegs(lib, c, segs, dev)
    (bias,) = on(dev, c, "b")
    with P.split_mode(lib, mode), S.kernel(lib, kern):
        rc, y, rec = S.run_top2(lib, ds, c["V"], bias, want_y=want_y)
    assert rc == 0, rc
    nblk = (c["V"] + 31) // 32
    assert all_nan(rec[nblk]), "a record block past the last one was written"
    if y is not None:
        assert all_nan(y[c["M"]:]), "row M of y was written"
        y = y[:c["M"]]
    return y, rec[:nblk]


@pytest.mark.parametrize("V", [50, 300, 1025])
@pytest.mark.parametrize("M", [1, 33, 64])
@pytest.mark.parametrize("kern", KERNELS)
def test_records_are_the_top_two_of_the_same_launchs_logits(dev, lib, kern, M, V):
    """y and top2_part from ONE call: per block and row (v1, i1, v2, i2) are the top two of that block's columns of y -- values by
    bits --, mx == v1, se against fp64, rows >= M untouched; y itself against fp64; the y = NULL form gives the same record bits; two
    launches agree.  V = 1025: the last block has one valid column, its second entry is (-inf, 0x7fffffff) and its sum is 1."""
    c = P.linear_case(8000 + V + M, M, V, 96)
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    for mode in (0, 1, 2):
        tag = f"records {kern} mode={mode} M={M} V={V}"
        y, rec = records_of(lib, dev, c, kern, mode)
        S.check_linear(tag, torch.cat([y, nan_buf(1, V, dev=dev)]), ref, M, V)
        P.check_records("skinny " + tag, rec, y, M, V)
        _, rec_only = records_of(lib, dev, c, kern, mode, want_y=False)
        assert same_bits(rec, rec_only), (tag, "the y = NULL form gives other records")
        _, again = records_of(lib, dev, c, kern, mode)
        assert same_bits(rec, again), (tag, "two launches of one case differ")
        if V % 32 == 1:
            last = P.decode_records(rec, M)
            assert bool((last["i2"][:, -1] == P.NO_INDEX).all()) and bool((last["v2"][:, -1] == -math.inf).all())
            assert bool((last["i1"][:, -1] == V - 1).all()) and bool((last["se"][:, -1] == 1.0).all())


@pytest.mark.parametrize("place,V,K,pair", P.TIE_PLACES)
@pytest.mark.parametrize("kern", KERNELS)
def test_exact_integer_cases_ties_go_to_the_lowest_index(dev, lib, kern, place, V, K, pair):
    """Integer operands make every sum exact in all three modes: y, the records' values and indices and the chosen word are asserted
    EXACTLY.  A wave scans columns 8w .. 8w + 7 of a block here, so (32, 33) tie inside one wave's scan, (33, 41) across waves 0 and 1
    of block 1 (the four-wave merge), (3, 69) across blocks 0 and 2, (7, 8195) across blocks 0 and 256.  i1 / i2 of the merged records
    per row scenario (exact_case); top-2 through cvc_top2_final by naming the top word UNK."""
    M = 8
    c = P.exact_case(77, M, V, K, pair)
    exact = P.linear_ref(c["x"], c["w"], c["b"])
    nblk = (V + 31) // 32
    for mode in (0, 1, 2):
        tag = f"exact {place} {kern} mode={mode}"
        y, rec = records_of(lib, dev, c, kern, mode)
        assert torch.equal(y.double().cpu(), exact), (tag, "y is not exact on integer operands")
        P.check_records("skinny " + tag, rec, y, M, V)
        got = P.decode_records(rec, M)
        _, _, i1, i2 = P.merge_records(got, -1)
        assert torch.equal(i1.cpu(), c["top1"]) and torch.equal(i2.cpu(), c["top2"]), (tag, i1.tolist(), i2.tolist())
        for unk in (-1, c["a"], c["b_col"], c["t"]):
            rc, word, lp, _ = P.run_top2_final(lib, dev, rec, nblk, M, unk)
            assert rc == 0, rc
            want = torch.where(c["top1"] == unk, c["top2"], c["top1"]).to(dev)
            assert torch.equal(word[:, 0], want), (tag, unk, word[:, 0].tolist(), want.tolist())
            w_ref, lp_ref, _ = P.select_ref(exact, unk)
            assert torch.equal(w_ref, want.cpu())
            close(lp, lp_ref.float(), **OP_TOL)


@pytest.mark.parametrize("M", [1, 33, 64])
@pytest.mark.parametrize("kern", KERNELS)
def test_last_valid_column_as_the_row_maximum_enters_once(dev, lib, kern, M):
    """V = 300: lanes of the last block past column 299 load clamped duplicates of weight row 299.  Column 299 is the row maximum
    on the even rows: it is the block's top-1 there, never its top-2, and the block's sum counts it once (check_records: se against
    fp64 over the 12 valid columns)."""
    V = 300
    c = S.last_column_case(8500 + M, M, V)
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    assert bool((ref[0::2].argmax(1) == V - 1).all()) and bool((ref[1::2].argmax(1) != V - 1).all() or M == 1)
    for mode in (0, 1, 2):
        tag = f"last column {kern} mode={mode} M={M}"
        y, rec = records_of(lib, dev, c, kern, mode)
        close(y, ref.float(), **OP_TOL)
        P.check_records("skinny " + tag, rec, y, M, V)
        last = P.decode_records(rec, M)
        assert bool((last["i1"][0::2, -1] == V - 1).all()) and bool((last["i2"][0::2, -1] != V - 1).all()), (tag, "column 299 twice, or not on top")
        assert bool((last["i2"][:, -1] < V).all())
        # the sum of the last block on an even row: 1 + 11 terms of exp(-20 + O(1)) -- a second copy of the maximum would make it 2
        assert bool((last["se"][0::2, -1] < 1.01).all())


@pytest.mark.parametrize("V,seed", S.NEGATIVE_VOCAB_CASES)
@pytest.mark.parametrize("kern", KERNELS)
def test_vocabulary_ending_inside_a_block_keeps_the_padding_out(dev, lib, kern, V, seed):
    """P.negative_vocab_case: every real logit is below -1, so a padding column (a zero, or a clamped duplicate) would win its
    block's record or enter its sum.  Records against the same launch's y; the merged word of EVERY row equal to the fp64 choice
    (the seeds give every row a deciding margin of at least 1e-3, asserted first), its log-prob against fp64."""
    M = 37
    c = P.negative_vocab_case(seed, M, V)
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    assert float(ref.max()) < -1.0
    w_ref, lp_ref, margin = P.select_ref(ref, -1)
    assert float(margin.min()) >= 1e-3
    for mode in (0, 1, 2):
        tag = f"negative vocabulary {kern} mode={mode} V={V}"
        y, rec = records_of(lib, dev, c, kern, mode)
        close(y, ref.float(), **OP_TOL)
        P.check_records("skinny " + tag, rec, y, M, V)
        rc, word, lp, _ = P.run_top2_final(lib, dev, rec, (V + 31) // 32, M, -1)
        assert rc == 0, rc
        assert bool((word[:, 0] < V).all()) and bool((word[:, 0] >= 0).all())
        assert torch.equal(word[:, 0].cpu(), w_ref), (tag, word[:, 0].tolist(), w_ref.tolist())
        print(f"skinny_gemm {tag}: logprob max |err| = {float((lp.double().cpu() - lp_ref).abs().max()):.3e}")
        close(lp, lp_ref.float(), **OP_TOL)


@pytest.mark.parametrize("V,seed", P.MERGE_CASES)
@pytest.mark.parametrize("kern", KERNELS)
def test_merged_word_and_logprob_on_random_rows(dev, lib, kern, V, seed):
    """M = 64, K = 256, records without y through cvc_top2_final: after asserting on the fp64 reference that EVERY row's deciding
    margin (after the UNK rule) is at least 1e-3 -- no row is left out --, the word is exact and its log-prob within OP_TOL."""
    c, unk = P.merge_case(V, seed)
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    w_ref, lp_ref, margin = P.select_ref(ref, unk)
    assert float(margin.min()) >= 1e-3
    for mode in (0, 1, 2):
        _, rec = records_of(lib, dev, c, kern, mode, want_y=False)
        rc, word, lp, _ = P.run_top2_final(lib, dev, rec, (V + 31) // 32, 64, unk)
        assert rc == 0, rc
        assert torch.equal(word[:, 0].cpu(), w_ref)
        print(f"skinny_gemm merge {kern} mode={mode} V={V}: logprob max |err| = {float((lp.double().cpu() - lp_ref).abs().max()):.3e}")
        close(lp, lp_ref.float(), **OP_TOL)


# ------------------------------------------------------------------ 5. the LSTM form
@pytest.mark.parametrize("R", [8, 40, 256])          # one workgroup, five, 32
@pytest.mark.parametrize("kern", KERNELS)
def test_lstm_form_every_bias_present_and_absent_gates_out_given_and_null(dev, lib, kern, R):
    """each of b_ih, b_hh and gate_bias (a different row per batch row) present and absent, gates_out given and NULL with h' and c'
    unchanged bit for bit by it; h', c' and the four activations against P.lstm_ref; M = 37 (two row tiles, the second with five
    rows), K = 96, modes 0 and 2"""
    M, K = 37, 96
    c = P.lstm_case(9000 + R, M, R, K)
    assert len({tuple(r.tolist()) for r in c["gate_bias"]}) == M
    segs, x_eff = S.split_segments(c, (K,))
    ds = S.DevSegs(lib, c, segs, dev)
    d = dict(zip(("b_ih", "b_hh", "gate_bias", "c_prev"), on(dev, c, "b_ih", "b_hh", "gate_bias", "c_prev")))
    for use in [(a, b, g) for a in (True, False) for b in (True, False) for g in (True, False)]:
        terms = [c[n] for n, u in zip(("b_ih", "b_hh", "gate_bias"), use) if u]
        ref = P.lstm_ref(x_eff, c["w"], c["c_prev"], terms)
        args = [d[n] if u else None for n, u in zip(("b_ih", "b_hh", "gate_bias"), use)]
        for mode in (0, 2):
            tag = f"lstm form {kern} mode={mode} R={R} b_ih={int(use[0])} b_hh={int(use[1])} gate_bias={int(use[2])}"
            with P.split_mode(lib, mode), S.kernel(lib, kern):
                rc, *outs = S.run_lstm(lib, ds, R, d["c_prev"], *args)
                rc2, *bare = S.run_lstm(lib, ds, R, d["c_prev"], *args, want_gates=False)
            assert rc == 0 and rc2 == 0, (tag, rc, rc2)
            S.check_lstm(tag, outs, ref, M)
            S.check_lstm(tag + " gates_out=NULL", bare, ref, M, want_gates=False)
            assert same_bits(outs[0], bare[0]) and same_bits(outs[1], bare[1]), (tag, "gates_out changes h' or c'")


@pytest.mark.parametrize("kern", KERNELS)
def test_linear_form_bias_and_bias2_present_and_absent(dev, lib, kern):
    """cvc_linear_fwd with each of bias and bias2 given and NULL (gate_fc of the decodes gives both, h2attn one, the ring path's
    projections none): y against linear_ref plus exactly the given vectors, which differ from each other and from zero by at least
    1e-2 on every column; M = 37, Nout = 300 (the last workgroup has 12 columns), K = 96, modes 0 and 2"""
    M, V, K = 37, 300, 96
    c = P.linear_case(9100, M, V, K)
    b2 = S.second_bias(c)
    ds = S.DevSegs(lib, c, S.split_segments(c, (K,))[0], dev)
    bias, bias2 = c["b"].to(dev), b2.to(dev)
    bare = P.linear_ref(c["x"], c["w"])
    for use in [(a, b) for a in (True, False) for b in (True, False)]:
        ref = bare + (c["b"].double() if use[0] else 0) + (b2.double() if use[1] else 0)
        for mode in (0, 2):
            tag = f"linear form {kern} mode={mode} bias={int(use[0])} bias2={int(use[1])}"
            with P.split_mode(lib, mode), S.kernel(lib, kern):
                rc, y = S.run_linear(lib, ds, V, bias if use[0] else None, bias2 if use[1] else None, ldy=V + 4)
            assert rc == 0, (tag, rc)
            S.check_linear(tag, y, ref, M, V)


# ------------------------------------------------------------------ 6. more than 64 rows: the slab walk
@pytest.mark.parametrize("M", [65, 129])             # the last slab has one row
@pytest.mark.parametrize("kern", KERNELS)
def test_more_than_64_rows_every_slab_is_its_own_64_row_call(dev, lib, kern, M):
    """cvc_linear_fwd (bias, bias2, ldy = Nout + 4) and cvc_lstm_cell_fwd (both biases, gate_bias, gates_out) with a gather segment
    in the middle: every row within OP_TOL of fp64, and rows [64 s, 64 s + 64) bitwise a call on that slab's own operands -- the
    offsets of idx, x, y, c_prev, gate_bias, h', c' and gates_out by m0.  Runs in the library's default split mode only (2): the
    slab walk is host code that never reads the mode, and each slab's launch is the 64-row launch of sections 1 and 2, which run
    every mode."""
    ks, R, V = (64, 96, 32), 40, 72
    cc, lc = P.lstm_case(9500 + M, M, R, sum(ks)), P.linear_case(9600 + M, M, V, sum(ks))
    csegs, cx = S.split_segments(cc, ks, (1,))
    lsegs, lx = S.split_segments(lc, ks, (1,))
    b2 = S.second_bias(lc)
    cref = P.lstm_ref(cx, cc["w"], cc["c_prev"], P.lstm_terms(cc, True, True))
    lref = P.linear_ref(lx, lc["w"], lc["b"]) + b2.double()
    b_ih, b_hh, gb, cp = on(dev, cc, "b_ih", "b_hh", "gate_bias", "c_prev")
    bias, bias2 = lc["b"].to(dev), b2.to(dev)
    with S.kernel(lib, kern):
        rc, *outs = S.run_lstm(lib, S.DevSegs(lib, cc, csegs, dev), R, cp, b_ih, b_hh, gb)
        rc2, y = S.run_linear(lib, S.DevSegs(lib, lc, lsegs, dev), V, bias, bias2, ldy=V + 4)
        assert rc == 0 and rc2 == 0, (rc, rc2)
        S.check_lstm(f"slabs {kern} M={M} lstm", outs, cref, M)
        S.check_linear(f"slabs {kern} M={M} linear", y, lref, M, V)
        for m0 in range(0, M, 64):
            m1 = min(m0 + 64, M)
            rc, *slab = S.run_lstm(lib, S.DevSegs(lib, cc, csegs, dev, (m0, m1)), R, cp[m0:m1].contiguous(), b_ih, b_hh, gb[m0:m1].contiguous())
            rc2, ys = S.run_linear(lib, S.DevSegs(lib, lc, lsegs, dev, (m0, m1)), V, bias, bias2, ldy=V + 4)
            assert rc == 0 and rc2 == 0, (rc, rc2)
            assert all(same_bits(a[m0:m1], b[:m1 - m0]) for a, b in zip(outs, slab)), (kern, M, m0, "lstm slab differs from its own 64-row call")
            assert same_bits(y[m0:m1], ys[:m1 - m0]), (kern, M, m0, "linear slab differs from its own 64-row call")


# ------------------------------------------------------------------ 7. the 32-bit offset bound of the ring kernel
def test_weight_rows_4_gib_apart_take_the_kernel_with_64_bit_offsets(dev, lib):
    """w is a [33, 32] view with ldw = 2^25 of one 4 GiB buffer, of which only the 33 viewed rows are written: row 32 lies 2^32 bytes
    after row 0.  The ring kernel forms per-lane byte offsets in 32 bits, where that row wraps to row 0 -- in bounds, so column 32
    would come out as column 0's product without a fault; the host has to send such a shape to the direct-load kernel.  All 33
    columns against fp64.  A refused allocation fails the test.
    Then the activation side in the same buffer: x is a [17, 32] view with ldx = 2^26, row 16 lying 2^32 bytes after row 0 (the
    kernel's xoff is 32-bit too); all 17 rows against fp64."""
    M, K, Nout, ldw = 4, 32, 33, 1 << 25
    c = P.linear_case(3232, M, Nout, K)
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    assert float((ref[:, 32] - ref[:, 0]).abs().min()) > 1e-2            # the wrapped answer is far outside OP_TOL on every row
    Mx, ldx = S.OFFSET_X_ROWS, 1 << 26
    cx = P.linear_case(S.OFFSET_X_SEED, Mx, 40, K)
    refx = P.linear_ref(cx["x"], cx["w"], cx["b"])
    assert float((refx[16] - refx[0]).abs().min()) > 1e-2                # row 0's answer in row 16 is far outside OP_TOL on every column
    big = w = x = None
    try:
        big = torch.empty((1 << 30) + 32, dtype=torch.float32, device=dev)
        w = big.as_strided((Nout, K), (ldw, 1))
        w.copy_(c["w"].to(dev))
        x, bias = c["x"].to(dev), c["b"].to(dev)
        arr = lib._segs([dict(x=x, w=w)], M)
        assert arr[0].ldw == ldw
        y = nan_buf(M + 1, Nout, dev=dev)
        rc = lib.lib().cvc_linear_fwd(arr, 1, bias.data_ptr(), None, M, Nout, y.data_ptr(), Nout, S.stream_handle())
        torch.cuda.synchronize()
        assert rc == 0, rc
        S.check_linear("offset bound ldw=2^25", y, ref, M, Nout)
        x = big.as_strided((Mx, K), (ldx, 1))
        x.copy_(cx["x"].to(dev))
        wx, bx = cx["w"].to(dev), cx["b"].to(dev)
        arr = lib._segs([dict(x=x, w=wx)], Mx)
        assert arr[0].ldx == ldx
        y = nan_buf(Mx + 1, 40, dev=dev)
        rc = lib.lib().cvc_linear_fwd(arr, 1, bx.data_ptr(), None, Mx, 40, y.data_ptr(), 40, S.stream_handle())
        torch.cuda.synchronize()
        assert rc == 0, rc
        S.check_linear("offset bound ldx=2^26", y, refx, Mx, 40)
    finally:
        big = w = x = None                   # the views hold the buffer too
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ 8. split arithmetic of the ring kernel
@pytest.mark.parametrize("M,K,N", [(17, 256, 96), (64, 1024, 520)])
def test_split_products_of_the_ring_kernel_are_fp32_grade(dev, lib, M, K, N):
    """the mixed-magnitude operands of test_split_product_gemm_is_fp32_grade through cvc_linear_fwd on the ring kernel: mode 0's rms
    error at most 1e-6 of the reference's rms, modes 1 and 2 (the three-way bf16 split) no worse than 1.25 x mode 0 in rms and max"""
    c = S.mixed_magnitude_case(M, K, N)
    segs, x_eff = S.split_segments(c, (K,))
    ds = S.DevSegs(lib, c, segs, dev)
    (bias,) = on(dev, c, "b")
    ref = P.linear_ref(c["x"], c["w"], c["b"])
    err = {}
    for mode in (0, 1, 2):
        with P.split_mode(lib, mode), S.kernel(lib, "ring"):
            rc, y = S.run_linear(lib, ds, N, bias)
        assert rc == 0 and all_nan(y[M:]) and bool(torch.isfinite(y[:M]).all()), (mode, rc)
        e = (y[:M].double().cpu() - ref).abs()
        err[mode] = (e.pow(2).mean().sqrt().item(), e.max().item())
        print(f"skinny_gemm split arithmetic M={M} K={K} N={N} mode={mode}: rms err = {err[mode][0]:.3e}, max |err| = {err[mode][1]:.3e}")
    assert err[0][0] <= 1e-6 * ref.pow(2).mean().sqrt().item(), err
    for mode in (1, 2):
        assert err[mode][0] <= 1.25 * err[0][0] and err[mode][1] <= 1.25 * err[0][1], err


# ------------------------------------------------------------------ 9. refusals
def test_refusals_launch_nothing_and_leave_every_output_nan(dev, lib):
    """every call below is answered before anything is launched: the return code is the stated one and every output buffer is
    still NaN throughout"""
    L = lib.lib()
    M, K, V, R = 4, 32, 40, 16
    g = torch.Generator().manual_seed(99)
    x = torch.randn(65, K + 8, generator=g).to(dev)                       # 65 rows: the M = 65 refusals name rows that exist
    w = torch.randn(4 * R, K + 8, generator=g).to(dev)
    table, idx = torch.randn(50, K, generator=g).to(dev), torch.randint(0, 50, (65,), generator=g).to(dev)
    bias, c_prev = torch.randn(4 * R, generator=g).to(dev), torch.randn(65, R, generator=g).to(dev)
    st = S.stream_handle()

    def segs(n=1, k=K, ldx=K + 8, ldw=K + 8, xoff=0, woff=0, gather=False):
        arr = (lib.GemmSeg * max(n, 1))()
        for i in range(max(n, 1)):
            if gather:
                arr[i] = lib.GemmSeg(table.data_ptr(), idx.data_ptr(), w.data_ptr() + woff, k, K, ldw, 1)
            else:
                arr[i] = lib.GemmSeg(x.data_ptr() + xoff, None, w.data_ptr() + woff, k, ldx, ldw, 0)
        return arr

    bad_segs = [dict(n=0), dict(n=5), dict(k=0), dict(k=2), dict(k=6), dict(ldx=K + 6), dict(ldw=K + 6), dict(xoff=4), dict(woff=8)]

    def linear(n=1, M=M, y=True, ldy=V, **kw):
        out = nan_buf(min(M, 65) + 1, V, dev=dev)
        rc = L.cvc_linear_fwd(segs(n, **kw), n, bias.data_ptr(), None, M, V, out.data_ptr() if y else None, ldy, st)
        return rc, [out]

    def splitk(n=1, M=M, ksplit=2, **kw):
        out = nan_buf(3, min(M, 65), V, dev=dev)
        rc = L.cvc_linear_splitk_fwd(segs(n, **kw), n, bias.data_ptr(), M, V, ksplit, out.data_ptr(), st)
        return rc, [out]

    def top2(n=1, M=M, y=True, rec=True, **kw):
        out, r = nan_buf(min(M, 65) + 1, V, dev=dev), nan_buf(3, 64, 6, dev=dev)
        rc = L.cvc_linear_top2_fwd(segs(n, **kw), n, bias.data_ptr(), M, V, out.data_ptr() if y else None, r.data_ptr() if rec else None, st)
        return rc, [out, r]

    def lstm(n=1, M=M, R=R, null=(), **kw):
        h, c, gates = nan_buf(M + 1, R, dev=dev), nan_buf(M + 1, R, dev=dev), nan_buf(M + 1, 4 * R, dev=dev)
        rc = L.cvc_lstm_cell_fwd(segs(n, **kw), n, bias.data_ptr(), None, None, None if "c_prev" in null else c_prev.data_ptr(), M, R,
                                 None if "h_out" in null else h.data_ptr(), None if "c_out" in null else c.data_ptr(), gates.data_ptr(), st)
        return rc, [h, c, gates]

    calls = [(f, kw, E_BADARG) for f in (linear, splitk, top2, lstm) for kw in bad_segs]
    calls += [(linear, dict(ldy=V - 1), E_BADARG), (linear, dict(y=False), E_BADARG),              # rows of y would overlap; no output at all
              (top2, dict(rec=False), E_BADARG), (top2, dict(rec=False, y=False), E_BADARG),       # the top-2 form without its records
              (splitk, dict(ksplit=0), E_BADARG), (splitk, dict(ksplit=65), E_BADARG),
              (splitk, dict(gather=True), E_BADARG),                                               # a K slice of gathered rows
              (splitk, dict(M=65), E_BADARG), (top2, dict(M=65), E_TOOBIG),                        # one slab only in these forms
              (lstm, dict(R=4), E_BADARG), (lstm, dict(R=12), E_BADARG),
              (lstm, dict(null=("c_prev",)), E_BADARG), (lstm, dict(null=("h_out",)), E_BADARG), (lstm, dict(null=("c_out",)), E_BADARG)]
    for f, kw, want in calls:
        rc, outs = f(**kw)
        torch.cuda.synchronize()
        assert rc == want, (f.__name__, kw, rc, want)
        assert all(all_nan(t) for t in outs), (f.__name__, kw, "an output was written by a refused call")
    # the same helpers with nothing wrong are accepted (the refusals above are not the helpers' own doing)
    for f in (linear, splitk, top2, lstm):
        rc, outs = f()
        torch.cuda.synchronize()
        assert rc == 0 and not all_nan(outs[0]), (f.__name__, rc)
    rc, outs = splitk(gather=True, ksplit=1)
    assert rc == 0, rc
