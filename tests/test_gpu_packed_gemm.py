"""GPU tests (pytest -m gpu) of the packed decode GEMM's entry points in the DEFAULT build (csrc/gemm_packed.hip:
cvc_packed_lstm_fwd, cvc_packed_lstm_embgate_fwd, cvc_packed_lstm_embgate_ex_fwd, cvc_packed_lstm_late_fwd with early = NULL,
cvc_packed_lstm_step_fwd, cvc_packed_linear_fwd) and of cvc_top2_final, each called through the C-ABI as cvc/decode/path_packed.py
and csrc/train_driver.hip call it and compared ELEMENT-WISE with a torch fp64 restatement (tests/packed_gemm_cases.py) on the same
fp32 inputs cast up.  Operands come from cvc.decode.pack_weights / to_quad / from_quad.

Every output buffer is pre-filled with NaN: an element the contract says is written is compared, every other one must still be
NaN (rows >= M of the quad outputs and of the records, columns >= Nout of y when ldy > Nout, the quads around a destination).
Tolerance: OP_TOL (rtol = atol = 2e-5), with weights scaled by 1 / sqrt(K) and N(0, 1) activations, so pre-activations have unit
scale at every K.  Forms that differ in layout, load policy or entry point only are BITWISE equal, and so are two launches of
one case.  Where a path is chosen by shape or mode, the arithmetic that chooses it stands beside the case; the constants are
CVC_PACKED_DEPTH = 4 (modes 0 / 1, NW = 4 waves) and CVC_PACKED_DEPTH8 = 3 (mode 2, NW = 8) of the source, which
tests/test_packed_gemm_cpu.py reads and checks the sweep against."""
import math

import pytest
import torch

import packed_gemm_cases as P
from packed_gemm_cases import E_BADARG, NO_INDEX, OP_TOL, all_nan, close, same_bits

pytestmark = pytest.mark.gpu


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


def sub_rows(o, M, pad_nan=False):
    """the first M rows of a 64-row LSTM / linear operand set (same weights, activations re-packed)"""
    from cvc.decode import to_quad
    s = dict(o, M=M, x=o["x"][:M], xq=to_quad(o["x"][:M].contiguous()))
    if "c_prev" in o:
        s.update(c_prev=o["c_prev"][:M].contiguous(), cq=to_quad(o["c_prev"][:M].contiguous()), gate_bias=o["gate_bias"][:M].contiguous(),
                 word=o["word"][:M].contiguous())
    if pad_nan:
        s["xq"][:, M:] = float("nan")
        if "cq" in s:
            s["cq"][:, M:] = float("nan")
    return s


# ------------------------------------------------------------------ 1. the K loop: every branch of the register ring
# Wave kw of NW takes chunks kw, kw + NW, ... of the K / 32 chunks: n_my = ceil((K / 32 - kw) / NW), and with DEPTH chunks in flight
#   n_my < DEPTH                       : the short loop (load, multiply)
#   DEPTH <= n_my < 2 DEPTH - 1        : prefill + drain only
#   n_my >= 2 DEPTH - 1                : passes of the steady loop while j + 2 DEPTH - 1 <= n_my (j += DEPTH), then a drain of n_my - j
# mode 2 (NW 8, DEPTH 3): short 0-2 | drain only 3-4 | one pass 5-7 (drain 2, 3, 4) | two passes 8 (drain 2)
# modes 0 / 1 (NW 4, DEPTH 4): short 0-3 | drain only 4-6 | one pass 7-10 (drain 3 .. 6) | two passes 11 (drain 3)
# K / 32 -> (largest, smallest n_my):  NW 8: 1 (1,0) 6 (1,0) 12 (2,1) 14 (2,1) 20 (3,2) 26 (4,3) 28 (4,3) 32 (4,4) 36 (5,4) 42 (6,5) 52 (7,6) 60 (8,7)
#                                      NW 4: 1 (1,0) 6 (2,1) 12 (3,3) 14 (4,3) 20 (5,5) 26 (7,6) 28 (7,7) 32 (8,8) 36 (9,9) 42 (11,10) 52 (13,13) 60 (15,15)
# The walk starts at chunk (5 blockIdx.x) mod n_my: with 8 (LSTM, R = 64) and 10 (linear, Nout = 300) workgroups the start differs
# between blocks.  M = 1 / 32 (MT = 1) and 33 / 64 (MT = 2) are the row-tile boundary and its far ends.
# A skipped or doubled chunk moves a pre-activation by about 1 / sqrt(K / 32) >= 0.13, four orders above OP_TOL.
@pytest.mark.parametrize("nchunk", P.SWEEP_CHUNKS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_k_loop_lstm_every_ring_branch_vs_fp64(dev, lib, mode, nchunk):
    """cvc_packed_lstm_fwd, R = 64 (eight workgroups), both biases, no per-row term: h_dst2 / h_dst1 and c' against fp64 at
    M = 1, 32, 33, 64; two launches agree bit for bit."""
    K, R = nchunk * 32, 64
    c = P.lstm_case(1000 + nchunk, 64, R, K)
    o = P.lstm_operands(c, dev)
    ref = P.lstm_ref(o["x"], o["w"], o["c_prev"], P.lstm_terms(o))
    with P.split_mode(lib, mode):
        for M in (1, 32, 33, 64):
            s = sub_rows(o, M)
            r = {k: v[:M] for k, v in ref.items()}
            rc, *outs = P.run_lstm(lib, s, "lstm")
            assert rc == 0, rc
            P.check_lstm(f"k_loop lstm mode={mode} K/32={nchunk} M={M}", outs, r, M)
            rc, *again = P.run_lstm(lib, s, "lstm")
            assert rc == 0, rc
            assert all(same_bits(a.buf, b.buf) for a, b in zip(outs, again)), "two launches of one case differ"


@pytest.mark.parametrize("nchunk", P.SWEEP_CHUNKS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_k_loop_linear_every_ring_branch_vs_fp64(dev, lib, mode, nchunk):
    """cvc_packed_linear_fwd, Nout = 300 (ten workgroups, the last with 12 columns), ksplit = 1, bias, y with ldy = 304."""
    K, V = nchunk * 32, 300
    o = P.linear_operands(P.linear_case(2000 + nchunk, 64, V, K), dev)
    ref = P.linear_ref(o["x"], o["w"], o["b"])
    with P.split_mode(lib, mode):
        for M in (1, 32, 33, 64):
            s = sub_rows(o, M)
            rc, y, _ = P.run_linear(lib, s, ldy=304)
            assert rc == 0, rc
            assert all_nan(y[0, :, V:]), "columns >= Nout of y were written"
            got = y[0, :, :V]
            assert bool(torch.isfinite(got).all())
            print(f"packed_gemm k_loop linear mode={mode} K/32={nchunk} M={M}: max |err| = {float((got.double() - ref[:M]).abs().max()):.3e}")
            close(got, ref[:M].float(), **OP_TOL)
            rc, y2, _ = P.run_linear(lib, s, ldy=304)
            assert rc == 0 and same_bits(y[0, :, :V], y2[0, :, :V])


# ------------------------------------------------------------------ 2. the decode cells as the default engine calls them
# R = 40: R / 8 = 5 workgroups.  The contraction length has to be a multiple of 32, so the "2 R" of the engine becomes the next one.
K_OF = {40: 96, 64: 128, 256: 512}
CELLS = [(M, R) for M in (5, 37, 64) for R in (40, 64, 256)]
# (biases, gate_bias, (h_dst1, h_dst2), K: "full" | "less" (K - 32) | "one" (32))
EX_VARIANTS = [(True, True, (True, True), "full"), (False, True, (True, False), "full"), (True, False, (False, True), "full"),
               (False, False, (True, True), "less"), (True, True, (True, True), "one"), (False, True, (False, True), "less")]


def k_of(kind, K):
    return {"full": K, "less": K - 32, "one": 32}[kind]


@pytest.mark.parametrize("M,R", CELLS)
def test_embgate_ex_the_default_attention_cell_vs_fp64(dev, lib, M, R):
    """cvc_packed_lstm_embgate_ex_fwd in mode 2: table [50, 4R] with words 0 and V - 1, gate_bias / biases set and null, one or both
    h' destinations at non-zero quad offsets inside larger NaN buffers, and the contraction stopping short of the packed K (step 0 of
    the engine: K = 32 with the full pack's block stride) -- against fp64 on w[:, :K], and bitwise a launch on a dense pack of
    w[:, :K].  w_cached = 1 is the same template with another load policy: bitwise.  cvc_packed_lstm_embgate_fwd is the _ex form
    with stride 0 and w_cached 0: bitwise."""
    from cvc.decode import pack_weights
    K = K_OF[R]
    o = P.lstm_operands(P.lstm_case(M * 1000 + R, M, R, K), dev)
    offs = (R // 4, 3)                                         # h_dst1 as qoff(XL_r, R); h_dst2 at another offset
    with P.split_mode(lib, 2):
        for b, gb, dst, kind in EX_VARIANTS:
            Kc = k_of(kind, K)
            tag = f"embgate_ex mode=2 M={M} R={R} K={Kc}/{K} b={int(b)} gb={int(gb)} dst={dst}"
            ref = P.lstm_ref(o["x"][:, :Kc], o["w"][:, :Kc], o["c_prev"], P.lstm_terms(o, b, gb, True))
            stride = 0 if kind == "full" and b else P.dense_stride(K)             # (0 = dense: both spellings of the full pack)
            rc, *outs = P.run_lstm(lib, o, "embgate_ex", K=Kc, b=b, gb=gb, tab=True, dst=dst, offs=offs, stride=stride)
            assert rc == 0, rc
            P.check_lstm(tag, outs, ref, M, dst)
            if kind != "full":
                rc, *dense = P.run_lstm(lib, o, "embgate_ex", K=Kc, b=b, gb=gb, tab=True, dst=dst, offs=offs,
                                        wp=pack_weights(o["w"][:, :Kc].contiguous(), R))
                assert rc == 0, rc
                assert all(same_bits(a.buf, d.buf) for a, d in zip(outs, dense)), (tag, "strided pack differs from the dense pack of w[:, :K]")
            rc, *cached = P.run_lstm(lib, o, "embgate_ex", K=Kc, b=b, gb=gb, tab=True, dst=dst, offs=offs, stride=stride, w_cached=1)
            assert rc == 0, rc
            assert all(same_bits(a.buf, d.buf) for a, d in zip(outs, cached)), (tag, "w_cached = 1 differs")
        rc, *ex = P.run_lstm(lib, o, "embgate_ex", gb=True, tab=True, offs=offs)
        rc2, *plain = P.run_lstm(lib, o, "embgate", gb=True, tab=True, offs=offs)
        assert rc == 0 and rc2 == 0
        assert all(same_bits(a.buf, d.buf) for a, d in zip(ex, plain)), "cvc_packed_lstm_embgate_fwd differs from the _ex form"
        P.check_lstm(f"embgate mode=2 M={M} R={R}", plain, P.lstm_ref(o["x"], o["w"], o["c_prev"], P.lstm_terms(o, True, True, True)), M)


@pytest.mark.parametrize("M,R", CELLS)
@pytest.mark.parametrize("mode", [0, 1])
def test_embgate_ex_in_the_four_wave_modes_ignores_w_cached(dev, lib, mode, M, R):
    """modes 0 / 1 have no cached-weights instantiation: w_cached = 1 runs the streaming kernel, bitwise, and both meet fp64"""
    K = K_OF[R]
    o = P.lstm_operands(P.lstm_case(M * 1000 + R + 7, M, R, K), dev)
    ref = P.lstm_ref(o["x"], o["w"], o["c_prev"], P.lstm_terms(o, True, True, True))
    with P.split_mode(lib, mode):
        rc, *outs = P.run_lstm(lib, o, "embgate_ex", gb=True, tab=True, offs=(R // 4, 3), w_cached=1)
        assert rc == 0, rc
        P.check_lstm(f"embgate_ex mode={mode} M={M} R={R}", outs, ref, M)
        rc, *plain = P.run_lstm(lib, o, "embgate_ex", gb=True, tab=True, offs=(R // 4, 3), w_cached=0)
        assert rc == 0 and all(same_bits(a.buf, d.buf) for a, d in zip(outs, plain))


@pytest.mark.parametrize("M,R", CELLS)
def test_late_form_without_early_tiles_is_the_language_cell_of_step_0(dev, lib, M, R):
    """cvc_packed_lstm_late_fwd(early = NULL) as path_packed.py's `first` step calls it -- the contraction 32 short of the pack's K,
    the pack's own block stride, biases, h_dst1 at offset 0 and h_dst2 at a quad offset -- against fp64 and bitwise
    cvc_packed_lstm_fwd on the same operands (the same instantiation); CVC_E_BADARG in modes 0 and 1, nothing written."""
    from cvc.decode import pack_weights
    K = K_OF[R]
    o = P.lstm_operands(P.lstm_case(M * 1000 + R + 13, M, R, K), dev)
    offs = (0, R // 2)
    with P.split_mode(lib, 2):
        for Kc in (K, K - 32):
            ref = P.lstm_ref(o["x"][:, :Kc], o["w"][:, :Kc], o["c_prev"], P.lstm_terms(o))
            rc, *late = P.run_lstm(lib, o, "late", K=Kc, offs=offs, stride=P.dense_stride(K))
            assert rc == 0, rc
            P.check_lstm(f"late mode=2 M={M} R={R} K={Kc}/{K}", late, ref, M)
            rc, *full = P.run_lstm(lib, o, "lstm", K=Kc, offs=offs, wp=pack_weights(o["w"][:, :Kc].contiguous(), R))
            assert rc == 0 and all(same_bits(a.buf, d.buf) for a, d in zip(late, full))
    for mode in (0, 1):
        with P.split_mode(lib, mode):
            rc, *outs = P.run_lstm(lib, o, "late", offs=offs, stride=P.dense_stride(K))
            assert rc == E_BADARG and all(all_nan(q.buf) for q in outs)


@pytest.mark.parametrize("M,R", CELLS)
def test_lstm_fwd_in_both_call_shapes_of_the_engine(dev, lib, M, R):
    """cvc_packed_lstm_fwd: the language cell (biases, no per-row term, h_dst1 at offset 0 of one buffer, h_dst2 at a quad offset
    of another) and the attention cell without the embedding-gate table (gate_bias only)."""
    K = K_OF[R]
    o = P.lstm_operands(P.lstm_case(M * 1000 + R + 29, M, R, K), dev)
    with P.split_mode(lib, 2):
        for name, b, gb, offs in (("lang", True, False, (0, R // 2)), ("att", False, True, (R // 4, (R + 32) // 4))):
            rc, *outs = P.run_lstm(lib, o, "lstm", b=b, gb=gb, offs=offs)
            assert rc == 0, rc
            P.check_lstm(f"lstm_fwd {name} mode=2 M={M} R={R}", outs, P.lstm_ref(o["x"], o["w"], o["c_prev"], P.lstm_terms(o, b, gb)), M)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_saturated_gates_and_huge_cell_states_stay_finite(dev, lib, mode):
    """gate_bias plants +-30 and +-100 on each of the four gates of 16 (row, unit) pairs and c_prev holds +-1e4 there and elsewhere:
    __expf overflows to inf (or underflows to 0) inside fast_sigmoid / fast_tanh, whose results must still be the saturated
    values -- every output finite and within OP_TOL of fp64."""
    M, R, K = 37, 64, 128
    c = P.lstm_case(31337, M, R, K)
    k = 0
    for g in range(4):
        for v in (30.0, -30.0, 100.0, -100.0):
            row, unit = (7 * k) % M, (11 * k + 3) % R
            c["gate_bias"][row, g * R + unit] = v
            c["c_prev"][row, unit] = 1e4 if k % 2 == 0 else -1e4
            k += 1
    c["c_prev"][1, 5], c["c_prev"][36, 63] = 1e4, -1e4
    o = P.lstm_operands(c, dev)
    with P.split_mode(lib, mode):
        for entry, tab in (("lstm", False), ("embgate_ex", True)):
            rc, *outs = P.run_lstm(lib, o, entry, gb=True, tab=tab, offs=(2, 0))
            assert rc == 0, rc
            P.check_lstm(f"saturation {entry} mode={mode}", outs, P.lstm_ref(o["x"], o["w"], o["c_prev"], P.lstm_terms(o, True, True, tab)), M)


@pytest.mark.parametrize("M", [5, 37])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_nan_in_the_padding_rows_reaches_no_output(dev, lib, mode, M):
    """rows >= M of xq and c_prev_q hold NaN instead of zero: a column of the product depends on its own row only, so rows < M are
    unchanged bit for bit and rows >= M of every output stay unwritten -- LSTM (embedding-gate form) and linear (y + records)."""
    R, K, V = 64, 128, 100
    c = P.lstm_case(4242 + M, M, R, K)
    lc = P.linear_case(4343 + M, M, V, K)
    with P.split_mode(lib, mode):
        rc, *clean = P.run_lstm(lib, P.lstm_operands(c, dev), "embgate_ex", gb=True, tab=True, offs=(1, 2))
        rc2, *dirty = P.run_lstm(lib, P.lstm_operands(c, dev, pad_nan=True), "embgate_ex", gb=True, tab=True, offs=(1, 2))
        assert rc == 0 and rc2 == 0
        assert all(bool(torch.isfinite(q.rows(M)).all()) and q.rest_is_nan(M) for q in dirty)
        assert all(same_bits(a.buf, d.buf) for a, d in zip(clean, dirty))
        rc, y, rec = P.run_linear(lib, P.linear_operands(lc, dev), want_rec=True)
        rc2, y2, rec2 = P.run_linear(lib, P.linear_operands(lc, dev, pad_nan=True), want_rec=True)
        assert rc == 0 and rc2 == 0
        assert bool(torch.isfinite(y2).all()) and same_bits(y, y2) and same_bits(rec, rec2) and all_nan(rec2[:, M:])
        assert bool(torch.isfinite(rec2[:, :M, [0, 4, 5]]).all())


# ------------------------------------------------------------------ 3. cvc_packed_lstm_step_fwd, the general training form
def check_step(tag, res, ref, M, outs=P.STEP_OUTS, mask=None):
    """c', h' and the activated gates against fp64; every row-major copy of h' and from_quad of the quad destinations bitwise h_out
    (or each other when h_out is null); h_drop_out == h' * mask exactly; a null output and row M of every row-major output unwritten"""
    err = 0.0
    for name, want in (("c_out", ref["c"]), ("gates_out", ref["gates"]), ("h_out", ref["h"])):
        if name != "c_out" and name not in outs:
            assert all_nan(res[name]), (tag, name, "written although null")
            continue
        got = res[name][:M]
        assert bool(torch.isfinite(got).all()) and all_nan(res[name][M:]), (tag, name)
        err = max(err, float((got.double() - want).abs().max()))
        close(got, want.float(), err_msg=f"{tag}: {name}", **OP_TOL)
    copies = []
    for name in ("h_out", "h_out2", "h_dst1_q", "h_dst2_q"):
        t = res[name]
        quad = isinstance(t, P.QuadOut)
        if name not in outs:
            assert all_nan(t.buf if quad else t), (tag, name, "written although null")
            continue
        assert t.rest_is_nan(M) if quad else all_nan(t[M:]), (tag, name)
        copies.append(t.rows(M) if quad else t[:M])
    for cpy in copies[1:]:
        assert same_bits(copies[0], cpy), (tag, "copies of h' differ")
    if copies:
        close(copies[0], ref["h"].float(), err_msg=f"{tag}: h'", **OP_TOL)
    if "h_drop_out" in outs:
        hd = res["h_drop_out"]
        assert all_nan(hd[M:]) and copies
        assert torch.equal(hd[:M], copies[0] * mask) if mask is not None else same_bits(hd[:M], copies[0]), (tag, "dropped copy")
    else:
        assert all_nan(res["h_drop_out"])
    print(f"packed_gemm {tag}: max |err| = {err:.3e}")


@pytest.mark.parametrize("K", [96, 416])              # K / 32 = 3, 13: mode 2 (NW 8) n_my <= 2: short; mode 0 (NW 4) n_my <= 1: short | 4, 3, 3, 3: drain only + short
@pytest.mark.parametrize("R", [40, 128])
@pytest.mark.parametrize("M", [3, 33, 64])
@pytest.mark.parametrize("mode", [2, 0])
def test_step_form_every_output_per_row_terms_and_dropped_copy(dev, lib, mode, M, R, K):
    """cvc_packed_lstm_step_fwd with a cvc.hip.LstmStep filled field by field: all seven outputs at once, then each nullable one null
    in turn; gate_pre and row_bias / row_index (with repeats) together and singly; h_drop_out == h_out * host_mask exactly for
    p = 0.3 and 0.5, and h' itself with rng_state = NULL or p = 0."""
    from cvc import dropout
    c = P.lstm_case(M * 100 + R + K, M, R, K, V=7)              # 7 table rows for up to 64 batch rows: the index vector repeats
    if M > 1:
        c["word"][1] = c["word"][0]
    o = P.lstm_operands(c, dev)
    rng, site = dropout.rng_state(dev), dropout.site_id("out_a.7")
    refs = {(gp, rb): P.lstm_ref(o["x"], o["w"], o["c_prev"], P.lstm_terms(o, True, gp, rb)) for gp in (True, False) for rb in (True, False)}
    with P.split_mode(lib, mode):
        masks = {p: dropout.host_mask("out_a.7", (M, R), p, dev).to(dev) for p in (0.3, 0.5)}
        for p, mask in masks.items():
            rc, res = P.run_step(lib, o, gate_pre=True, row_bias=True, rng=rng, site=site, p=p)
            assert rc == 0, rc
            assert 0 < int((mask == 0).sum()) < M * R
            check_step(f"step mode={mode} M={M} R={R} K={K} all outputs p={p}", res, refs[True, True], M, mask=mask)
        mask = masks[0.3]
        for null in P.STEP_OUTS:
            outs = tuple(n for n in P.STEP_OUTS if n != null)
            rc, res = P.run_step(lib, o, gate_pre=True, row_bias=True, outs=outs, rng=rng, site=site, p=0.3)
            assert rc == 0, rc
            check_step(f"step mode={mode} M={M} R={R} K={K} without {null}", res, refs[True, True], M, outs, mask)
        for gp, rb in ((True, False), (False, True), (False, False)):
            rc, res = P.run_step(lib, o, gate_pre=gp, row_bias=rb, rng=None, site=site, p=0.3)        # rng_state = NULL: h' itself
            assert rc == 0, rc
            check_step(f"step mode={mode} M={M} R={R} K={K} gate_pre={int(gp)} row_bias={int(rb)}", res, refs[gp, rb], M)
        rc, res = P.run_step(lib, o, gate_pre=True, row_bias=True, rng=rng, site=site, p=0.0, w_cached=1)   # p = 0: h' itself
        assert rc == 0, rc
        check_step(f"step mode={mode} M={M} R={R} K={K} p=0", res, refs[True, True], M)


def test_step_form_refusals(dev, lib):
    """row_bias without row_index, p = 1 and M = 65 are refused, nothing written"""
    from cvc import dropout
    o = P.lstm_operands(P.lstm_case(9, 64, 40, 96, V=7), dev)
    rng = dropout.rng_state(dev)
    for kw in (dict(row_bias=True, row_index=False), dict(rng=rng, p=1.0), dict(M=65)):
        rc, res = P.run_step(lib, o, **kw)
        assert rc == E_BADARG, (kw, rc)
        assert all(all_nan(t.buf if isinstance(t, P.QuadOut) else t) for t in res.values()), kw


# ------------------------------------------------------------------ 4. linear form: K slices, records, word selection
# Slice s of ksplit takes chunks [nchunk s / ksplit, nchunk (s + 1) / ksplit) (integer division): with K / 32 = 1 and ksplit = 8
# only slice 7 holds a chunk, with 6 slices 0 and 4 are empty; 12 gives 1 or 2 chunks per slice, 60 gives 7 or 8 (over 8 waves in
# mode 2: n_my <= 1), 20 over 3 slices 6 / 7 / 7 (modes 0 / 1: n_my <= 2).
@pytest.mark.parametrize("ld_extra", [0, 8])
@pytest.mark.parametrize("V", [96, 200])
@pytest.mark.parametrize("nchunk,ksplit", [(1, 8), (6, 8), (12, 8), (60, 8), (20, 3)])
def test_split_k_planes_vs_fp64_slice_by_slice(dev, lib, nchunk, ksplit, V, ld_extra):
    """every plane against fp64 on its own K slice, the bias in plane 0 only, a slice without a chunk written as exact zeros (plane 0:
    the bias itself), their sum against fp64; columns >= Nout untouched; all three modes"""
    M, K = 33, nchunk * 32
    o = P.linear_operands(P.linear_case(nchunk * 100 + V, M, V, K), dev)
    for mode in (0, 1, 2):
        with P.split_mode(lib, mode):
            rc, y, _ = P.run_linear(lib, o, ksplit=ksplit, ldy=V + ld_extra)
        assert rc == 0, rc
        assert all_nan(y[:, :, V:])
        y = y[:, :, :V]
        assert bool(torch.isfinite(y).all()), "a plane was left unwritten"
        for s in range(ksplit):
            lo, hi = nchunk * s // ksplit * 32, nchunk * (s + 1) // ksplit * 32
            want = P.linear_ref(o["x"][:, lo:hi], o["w"][:, lo:hi], o["b"] if s == 0 else None)
            if lo == hi:
                assert torch.equal(y[s], (o["b"].expand(M, V) if s == 0 else torch.zeros(M, V, device=dev))), (mode, s, "empty slice")
            close(y[s], want.float(), err_msg=f"mode {mode} plane {s}", **OP_TOL)
        ref = P.linear_ref(o["x"], o["w"], o["b"])
        print(f"packed_gemm split_k mode={mode} K/32={nchunk} ksplit={ksplit} V={V}: max |err| = {float((y.double().sum(0) - ref).abs().max()):.3e}")
        close(y.double().sum(0), ref, **OP_TOL)


@pytest.mark.parametrize("M,V,K", [(33, 300, 256), (5, 33, 64), (64, 1000, 128)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_records_are_the_top_two_of_the_same_launchs_logits(dev, lib, mode, M, V, K):
    """y and top2_part from ONE call: per block and row (v1, i1, v2, i2) are the top two of that block's columns of y -- values by
    bits, both being the same cross-wave sum plus bias --, mx == v1, se against fp64, rows >= M untouched; y itself against fp64.
    V = 33: the last block has one valid column, its second entry is (-inf, 0x7fffffff)."""
    o = P.linear_operands(P.linear_case(V * 10 + M, M, V, K), dev)
    with P.split_mode(lib, mode):
        rc, y, rec = P.run_linear(lib, o, want_rec=True)
    assert rc == 0, rc
    close(y[0], P.linear_ref(o["x"], o["w"], o["b"]).float(), **OP_TOL)
    P.check_records(f"records mode={mode} M={M} V={V}", rec, y[0], M, V)
    if V % 32 == 1:
        last = P.decode_records(rec, M)
        assert bool((last["i2"][:, -1] == NO_INDEX).all()) and bool((last["v2"][:, -1] == -math.inf).all())
        assert bool((last["i1"][:, -1] == V - 1).all()) and bool((last["se"][:, -1] == 1.0).all())


@pytest.mark.parametrize("V", [33, 50, 8190])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_vocabulary_ending_inside_a_block_keeps_the_padding_out(dev, lib, mode, V):
    """bias -5 on every word and small weights: every real logit is negative, so a zero row of the padded pack would win its block's
    record and enter its sum.  Records against the same launch's y, the merged word below V and its log-prob against fp64
    log_softmax over V columns."""
    M = 37
    o = P.linear_operands(P.negative_vocab_case(V + 5, M, V), dev)
    with P.split_mode(lib, mode):
        rc, y, rec = P.run_linear(lib, o, want_rec=True)
    assert rc == 0, rc
    ref = P.linear_ref(o["x"], o["w"], o["b"])
    assert float(ref.max()) < -1.0
    close(y[0], ref.float(), **OP_TOL)
    P.check_records(f"negative vocabulary mode={mode} V={V}", rec, y[0], M, V)
    rc, word, lp, _ = P.run_top2_final(lib, dev, rec, (V + 31) // 32, M, -1)
    assert rc == 0, rc
    w_ref, lp_ref, margin = P.select_ref(ref, -1)
    assert bool((word[:, 0] < V).all()) and bool((word[:, 0] >= 0).all())
    clear = margin > 1e-3
    assert torch.equal(word[:, 0][clear], w_ref[clear])
    # (on a row whose two best words are closer than the GEMM's error the other one may be chosen; its log-prob then differs by
    # less than that margin -- every row is compared with the log-prob of the word the device chose)
    lsm = torch.log_softmax(ref, 1).gather(1, word).view(-1)
    print(f"packed_gemm negative vocabulary mode={mode} V={V}: logprob max |err| = {float((lp.double() - lsm).abs().max()):.3e}")
    close(lp, lsm.float(), **OP_TOL)


@pytest.mark.parametrize("place,V,K,pair", P.TIE_PLACES)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_exact_integer_cases_ties_go_to_the_lowest_index(dev, lib, mode, place, V, K, pair):
    """Integer operands: y, the records' values and indices and the chosen word are asserted EXACTLY.  Ties at the row maximum and
    for second place (packed_gemm_cases.exact_case) inside one wave's share of a block, across two waves, across two blocks and
    across blocks b and b + 256 (one thread's stride in top2_final_kernel); top-2 is observed by naming the top word UNK."""
    M = 8
    c = P.exact_case(77, M, V, K, pair)
    o = P.linear_operands(c, dev)
    with P.split_mode(lib, mode):
        rc, y, rec = P.run_linear(lib, o, want_rec=True)
    assert rc == 0, rc
    exact = P.linear_ref(o["x"], o["w"], o["b"])
    assert torch.equal(y[0].double(), exact), "y is not exact on integer operands"
    P.check_records(f"exact {place} mode={mode}", rec, y[0], M, V)
    nblk = (V + 31) // 32
    for unk in (-1, c["a"], c["b_col"], c["t"]):
        rc, word, lp, _ = P.run_top2_final(lib, dev, rec, nblk, M, unk)
        assert rc == 0, rc
        want = torch.where(c["top1"] == unk, c["top2"], c["top1"]).to(dev)
        assert torch.equal(word[:, 0], want), (place, unk, word[:, 0].tolist(), want.tolist())
        w_ref, lp_ref, _ = P.select_ref(exact, unk)
        assert torch.equal(w_ref, want)
        close(lp, lp_ref.float(), **OP_TOL)


@pytest.mark.parametrize("unk", [0, 1, 99])
def test_unk_rule_on_exact_cases(dev, lib, unk):
    """the UNK column is the third planted column t of exact_case(a = 5, b = 40): row scenario 0: UNK not on top -> no effect (5);
    1: UNK alone on top -> the runner-up 5 and ITS log-prob; 2: 40 on top -> 40; 3: UNK tied on top with 5 and 40 -> the lowest index
    wins the top, so unk = 0 and 1 give the tied higher index 5, unk = V - 1 is not on top and changes nothing (5)."""
    M, V, K = 8, 100, 64
    c = P.exact_case(78 + unk, M, V, K, (5, 40), t=unk)
    o = P.linear_operands(c, dev)
    rc, y, rec = P.run_linear(lib, o, want_rec=True)
    assert rc == 0, rc
    exact = P.linear_ref(o["x"], o["w"], o["b"])
    assert torch.equal(y[0].double(), exact)
    rc, word, lp, _ = P.run_top2_final(lib, dev, rec, (V + 31) // 32, M, unk)
    assert rc == 0, rc
    assert word[:, 0].tolist() == [5, 5, 40, 5] * 2
    w_ref, lp_ref, _ = P.select_ref(exact, unk)
    assert torch.equal(w_ref, word[:, 0])
    close(lp, lp_ref.float(), **OP_TOL)
    # the runner-up's OWN log-prob on the rows where UNK was alone on top: one below the top logit there
    top_lp = torch.log_softmax(exact, 1)[:, unk]
    close(lp[1::4], (top_lp[1::4] - 1.0).float(), **OP_TOL)


# seeds chosen on the CPU (tests/test_packed_gemm_cpu.py asserts the margin without a GPU): bias[UNK] += 3 puts UNK on top of 39 of
# 64 rows at V = 300 and 9 at V = 5000
@pytest.mark.parametrize("V,seed", P.MERGE_CASES)
def test_merged_word_and_logprob_on_random_rows(dev, lib, V, seed):
    """M = 64, K = 256: after asserting on the fp64 reference that EVERY row's deciding margin (after the UNK rule) is at least
    1e-3 -- no row is excluded --, the word is exact and its log-prob within OP_TOL, in all three modes."""
    c, unk = P.merge_case(V, seed)
    o = P.linear_operands(c, dev)
    ref = P.linear_ref(o["x"], o["w"], o["b"])
    w_ref, lp_ref, margin = P.select_ref(ref, unk)
    assert float(margin.min()) >= 1e-3
    for mode in (0, 1, 2):
        with P.split_mode(lib, mode):
            rc, _, rec = P.run_linear(lib, o, want_y=False, want_rec=True)
        assert rc == 0, rc
        rc, word, lp, _ = P.run_top2_final(lib, dev, rec, (V + 31) // 32, 64, unk)
        assert rc == 0, rc
        assert torch.equal(word[:, 0], w_ref)
        print(f"packed_gemm merge mode={mode} V={V}: logprob max |err| = {float((lp.double() - lp_ref).abs().max()):.3e}")
        close(lp, lp_ref.float(), **OP_TOL)
        # the host merge of the device's records gives the device's answer
        w_host, lp_host, _, _ = P.merge_records(P.decode_records(rec, 64), unk)
        assert torch.equal(w_host, word[:, 0])
        close(lp, lp_host.float(), **OP_TOL)


@pytest.mark.parametrize("E", [4, 96, 1024])
def test_top2_final_word_slots_logprob_and_embedding_layouts(dev, lib, E):
    """cvc_top2_final: word_stride 1 and 3 with the other slots untouched, logprob null, emb_out in the quad layout (emb_ld = 0) at a
    quad offset and row-major with emb_ld = E and E + 4: relu(table[word]) exactly, rows >= M and everything around unwritten."""
    from cvc.decode import from_quad
    M, V, K = 37, 300, 64
    o = P.linear_operands(P.linear_case(555, M, V, K), dev)
    rc, _, rec = P.run_linear(lib, o, want_y=False, want_rec=True)
    assert rc == 0, rc
    nblk = (V + 31) // 32
    table = torch.randn(nblk * 32, E, generator=torch.Generator().manual_seed(E)).to(dev)     # (whole blocks of rows: any record index is a valid gather row)
    rc, word, lp, _ = P.run_top2_final(lib, dev, rec, nblk, M, 1)
    assert rc == 0 and bool(torch.isfinite(lp).all())
    want_emb = torch.relu(table[word[:, 0]])
    for stride in (1, 3):
        for emb in (None, "quad", E, E + 4):
            rc, w2, lp2, ebuf = P.run_top2_final(lib, dev, rec, nblk, M, 1, word_stride=stride, logprob=emb is None, table=table, emb=emb)
            assert rc == 0, (rc, stride, emb)
            assert torch.equal(w2[:, 0], word[:, 0]) and bool((w2[:, 1:] == -7).all())
            assert lp2 is None or same_bits(lp2, lp)
            if emb == "quad":
                assert torch.equal(from_quad(ebuf[2:2 + E // 4], M), want_emb)
                assert all_nan(ebuf[:2]) and all_nan(ebuf[2 + E // 4:]) and all_nan(ebuf[2:2 + E // 4, M:])
            elif emb is not None:
                assert torch.equal(ebuf[:M, :E], want_emb) and all_nan(ebuf[:M, E:]) and all_nan(ebuf[M:])
