"""GPU tests (pytest -m gpu) of the decode engine's TILE path and of the beam bookkeeping, every entry point called by name through
the C-ABI: cvc_tile_rows_alloc, cvc_tile_gemm, cvc_tile_linear_finish, cvc_tile_lstm_finish, cvc_tile_lstm_finish_embgate,
cvc_tile_pack_rows, cvc_tile_pack_rows_any, cvc_tile_pack_cols, cvc_tile_reorder_pack (csrc/gemm_tile.hip), cvc_beam_select,
cvc_beam_select_parts, cvc_beam_backtrack, cvc_gather_rows (csrc/beam.hip).  Cases and host references: tests/tile_path_cases.py;
what the tables reach is checked without a GPU in tests/test_tile_path_cpu.py; observed values: profiles/tile_path_pins.md.

Every output is pre-filled with NaN (fragment buffers with the bf16 NaN 0x7FC0, integer outputs with a sentinel): what the contract
says is written is compared, everything else must still hold the fill.  Every case runs twice and must repeat bit for bit.

  1. cvc_tile_gemm: an exact CENSUS.  The three term planes of both operands are independent integers in [-7, 7], so slab s must
     equal, exactly, the sum over the term pairs p + q <= 2 and over the k steps of slice s -- a dropped or doubled pair, a missed or
     repeated k step, a wrong slice boundary or lane / row mapping is off by integers.  In every form of the kernel.  One real-valued
     family through the packers is held element-wise against an fp32 GEMM's error (both against fp64).
  2. the finishing kernels: cvc_tile_linear_finish bitwise against the ordered fp32 host sum, the LSTM finish against fp64 at OP_TOL.
  3. packers and the beam-state reorder: bitwise against the host restatement of the fragment layout.
  4. beam bookkeeping: exact selection against a full fp64 scan on cases whose candidates are exactly tied by construction or at
     least 1e-3 apart; back-track and row gather against host indexing.
  5. refusals: CVC_E_BADARG before anything is launched."""
import pytest
import torch

import tile_path_cases as T
from tile_path_cases import E_BADARG, FILL16, KSTEP, OP_TOL, SCORE_TOL, all_nan, close, nan_buf, same_bits

pytestmark = pytest.mark.gpu
SENT = -7777                                     # fill of the integer outputs
DONE_FILL = 0xEE


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


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def frag_fill(nblk, ksteps, dev):
    return torch.full((nblk, ksteps, 3, 2, 32, 8), FILL16, dtype=torch.int16, device=dev)


def frag_at(xb, kstep):
    """(address of k step `kstep` of row block 0, row-block stride in bf16 elements)"""
    return xb.data_ptr() + kstep * KSTEP * 2, xb.shape[1] * KSTEP


def expect_planes(xb, rows, k0, want):
    """the buffer holds `want` [3, rows, K'] at rows [0, rows) and columns [k0, k0 + K') and the fill everywhere else"""
    got = T.frag_to_planes(xb)
    exp = T.fill_planes(got.shape[1], got.shape[2], xb.device)
    exp[:, :rows, k0:k0 + want.shape[2]] = want
    return torch.equal(got, exp)


# ------------------------------------------------------------------ 1. cvc_tile_gemm
def gemm(L, wb, xptr, xstride, K, M, N, ksplit, ld, dev):
    """-> (rc, slabs [ksplit, M, ld], the 7 floats behind every slab)"""
    buf = nan_buf(ksplit, M * ld + 7, dev=dev)
    rc = L.cvc_tile_gemm(wb.data_ptr(), xptr, xstride, K, M, N, ksplit, buf.data_ptr(), ld, M * ld + 7, st())
    return rc, buf[:, :M * ld].view(ksplit, M, ld), buf[:, M * ld:]


def check_census(what, out, ref, N):
    rc, slabs, tail = out
    assert rc == 0, (what, rc)
    assert all_nan(tail) and all_nan(slabs[:, :, N:]), f"{what}: columns >= N or the floats behind a slab were written"
    got = slabs[:, :, :N].double()
    assert bool(torch.isfinite(got).all()), f"{what}: a NaN of the rows >= M reached an output"
    bad = got != ref
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements differ, largest difference {float((got - ref).abs().max())}"


@pytest.mark.parametrize("M,N,K,ksplit", T.CENSUS)
def test_tile_gemm_exact_census_of_terms_and_k_steps(dev, lib, M, N, K, ksplit):
    """slab s == sum_{p + q <= 2} X_p[:, k range(s)] W_q[:, k range(s)]^T exactly, in forms 0, 1, 2, 4, the default and (whole tiles)
    the 256 x 256 form; ld > N and ld == N; as a K segment of a wider buffer; NaN patterns in every activation row >= M."""
    L = lib.lib()
    X, W = (t.to(dev) for t in T.census_case(M * 7 + N * 3 + K + ksplit, M, N, K))
    ref = T.census_ref(X, W, ksplit)
    xb, wb = T.census_frags(X, W)
    assert L.cvc_tile_rows_alloc(M) == T.rows_alloc(M) == xb.shape[0] * 32
    if M > 320:
        # The plan picks a ksplit of its own (printed); the launch below uses the case's, and its chunk height is
        # tile_rows_per_chunk(mblk, ntile * ksplit).  With grids this small (ntile * ksplit * chunks far below the CU count) both
        # come out at 3 accumulator tiles = 192 rows, which is asserted, so the dead-row-block check is about the launch made.
        # Chunk heights 4 and 5 are reached at or below ten row blocks only (M <= 320).
        ks_plan, chunk_rows, wgs = lib.tile_gemm_plan(M, N, K)
        assert chunk_rows == 192 and ((N + 127) // 128) * ksplit * ((M + 191) // 192) <= 64
        mblk, cb = (M + 31) // 32, chunk_rows // 32
        print(f"tile_path census M={M} N={N} K={K}: plan ksplit={ks_plan} chunk rows={chunk_rows} workgroups={wgs}")
        assert (mblk + cb - 1) // cb >= 2 and (mblk + cb - 1) // cb * cb > mblk, "the last row chunk has no dead row blocks"
    xp, xs = frag_at(xb, 0)
    ld = N + 3
    first = gemm(L, wb, xp, xs, K, M, N, ksplit, ld, dev)
    check_census("default form", first, ref, N)
    again = gemm(L, wb, xp, xs, K, M, N, ksplit, ld, dev)
    assert same_bits(first[1], again[1]), "two launches of one case differ"
    check_census("ld == N", gemm(L, wb, xp, xs, K, M, N, ksplit, N, dev), ref, N)
    prev = L.cvc_tile_gemm_loaders(-1)
    try:
        for form in (0, 1, 2, 4):
            L.cvc_tile_gemm_loaders(form)
            check_census(f"form {form}", gemm(L, wb, xp, xs, K, M, N, ksplit, ld, dev), ref, N)
    finally:
        L.cvc_tile_gemm_loaders(prev)
    if T.big_form(M, N):
        prev_big = L.cvc_tile_gemm_big(1, 1)
        try:
            check_census("256 x 256 form", gemm(L, wb, xp, xs, K, M, N, ksplit, ld, dev), ref, N)
        finally:
            L.cvc_tile_gemm_big(prev_big, 192)
    # a K segment of a wider activation buffer: pointer at k step 2, the row-block stride of the wide buffer; its other k steps are NaN
    xw = frag_fill(xb.shape[0], K // 16 + 3, dev)
    xw[:, 2:2 + K // 16] = xb
    wp, ws = frag_at(xw, 2)
    check_census("K segment", gemm(L, wb, wp, ws, K, M, N, ksplit, ld, dev), ref, N)


@pytest.mark.parametrize("M,N,K,ksplit", T.REAL)
def test_tile_gemm_real_values_element_wise_vs_fp64(dev, lib, M, N, K, ksplit):
    """through cvc_tile_pack_rows / cvc_tile_pack_rows_any: max |y - ref| / sum_k |x_ik| |w_jk| at most 4x the same quantity of the
    device's fp32 x @ w.t(), both against fp64 (observed values: profiles/tile_path_pins.md)"""
    L = lib.lib()
    x, w = (t.to(dev) for t in T.real_case(M + N + K, M, N, K))
    xb = torch.zeros(T.rows_alloc(M) // 32, K // 16, 3, 2, 32, 8, dtype=torch.int16, device=dev)
    wb = torch.zeros((N + 127) // 128 * 4, K // 16, 3, 2, 32, 8, dtype=torch.int16, device=dev)
    assert L.cvc_tile_pack_rows(x.data_ptr(), K, None, 0, M, K, *frag_at(xb, 0), st()) == 0
    assert L.cvc_tile_pack_rows_any(w.data_ptr(), K, N, K, *frag_at(wb, 0), st()) == 0
    rc, slabs, _ = gemm(L, wb, *frag_at(xb, 0), K, M, N, ksplit, N, dev)
    assert rc == 0
    y = T.ordered_sum(slabs)
    ref = x.double() @ w.double().t()
    scale = x.double().abs() @ w.double().abs().t()
    err = float(((y.double() - ref).abs() / scale).max())
    err32 = float((((x @ w.t()).double() - ref).abs() / scale).max())
    print(f"tile_path real M={M} N={N} K={K} ksplit={ksplit}: max |y - ref| / sum|x||w| = {err:.3e}, fp32 GEMM {err32:.3e}")
    assert err <= 4.0 * err32, (err, err32)
    assert same_bits(slabs, gemm(L, wb, *frag_at(xb, 0), K, M, N, ksplit, N, dev)[1])


# ------------------------------------------------------------------ 2. finishing kernels
@pytest.mark.parametrize("nparts", T.LIN_NPARTS)
def test_tile_linear_finish_is_the_ordered_fp32_sum_bitwise(dev, lib, nparts):
    """y == ((p0 + p1) + ...) + bias + bias2 in fp32, bit for bit; N = 1 .. 513, M = 1 / 321, ld > N, ldy > N, each bias null and set"""
    L = lib.lib()
    for c in (c for c in T.linear_cases() if c["nparts"] == nparts):
        M, N, ld, ldy = c["M"], c["N"], c["ld"], c["ldy"]
        parts, bias, bias2 = T.linear_inputs(c)
        want = T.ordered_sum(parts[:, :, :N], bias, bias2)
        dp, db, db2 = parts.to(dev), None if bias is None else bias.to(dev), None if bias2 is None else bias2.to(dev)
        ys = []
        for _ in range(2):
            y = nan_buf(M, ldy, dev=dev)
            assert L.cvc_tile_linear_finish(dp.data_ptr(), nparts, M * ld, ld, P(db), P(db2), M, N, y.data_ptr(), ldy, st()) == 0
            ys.append(y)
        assert all_nan(ys[0][:, N:]), (c, "columns >= N of y were written")
        assert same_bits(ys[0][:, :N].cpu(), want), c
        assert same_bits(ys[0][:, :N], ys[1][:, :N])


def lstm_call(L, c, d, dev, emb, null=None):
    """one launch of cvc_tile_lstm_finish / _embgate with every output pre-filled -> dict(rc, c_out, h_out [M + 1, R], f1, f2)"""
    M, R = c["M"], c["R"]
    nb = (M + 31) // 32 + 1                                        # one more row block than the rows need: it must stay untouched
    o = dict(c_out=nan_buf(M + 1, R, dev=dev), h_out=nan_buf(M + 1, R, dev=dev), f1=frag_fill(nb, R // 16 + 3, dev),
             f2=frag_fill(nb, R // 16 + 1, dev))
    p1, s1 = frag_at(o["f1"], 2) if null != "frag1" else (None, 0)
    p2, s2 = frag_at(o["f2"], 1) if null != "frag2" else (None, 0)
    g = lambda k: None if null == k else d[k].data_ptr()
    head = (d["parts"].data_ptr(), c["nparts"], M * 4 * R, g("b_ih"), g("b_hh"), g("gate_bias"), c["gb_div"])
    tail = (d["c_prev"].data_ptr(), M, R, o["c_out"].data_ptr(), None if null == "h_out" else o["h_out"].data_ptr(), p1, s1, p2, s2, st())
    if emb:
        o["rc"] = L.cvc_tile_lstm_finish_embgate(*head, d["emb_gate"].data_ptr(), d["word"].data_ptr(), T.LSTM_V, *tail)
    else:
        o["rc"] = L.cvc_tile_lstm_finish(*head, *tail)
    return o


def check_lstm(what, c, o, ref, h_bits, null=None):
    """c' / h' against fp64 at OP_TOL, finite; the row behind the last one untouched; both fragment destinations hold to_frag(h') at
    their k offset and the fill in every other k step, in rows >= M and in the extra row block"""
    M, R = c["M"], c["R"]
    assert o["rc"] == 0, (what, o["rc"])
    assert bool(torch.isfinite(o["c_out"][:M]).all()) and all_nan(o["c_out"][M:]), what
    cerr = float((o["c_out"][:M].double() - ref[0]).abs().max())
    close(o["c_out"][:M], ref[0].float(), **OP_TOL)
    if null == "h_out":
        assert all_nan(o["h_out"]), what
    else:
        assert bool(torch.isfinite(o["h_out"][:M]).all()) and all_nan(o["h_out"][M:]), what
        close(o["h_out"][:M], ref[1].float(), **OP_TOL)
    want = T.split3(h_bits)
    for key, k0 in (("f1", 32), ("f2", 16)):
        if null == ("frag1" if key == "f1" else "frag2"):
            assert bool((o[key] == FILL16).all()), (what, key)
        else:
            assert expect_planes(o[key], M, k0, want), f"{what}: {key} is not to_frag(h') inside the fill"
    return cerr


@pytest.mark.parametrize("nparts,R,M,gb_div", T.LSTM_CASES)
def test_tile_lstm_finish_and_embgate_vs_fp64(dev, lib, nparts, R, M, gb_div):
    """both entry points, every nullable argument null in turn, fragment destinations at a k offset inside wider buffers"""
    L = lib.lib()
    c = T.lstm_inputs(nparts * 1000 + R + M, nparts, R, M, gb_div)
    d = {k: v.to(dev) for k, v in c.items() if isinstance(v, torch.Tensor)}
    for emb in (False, True):
        name = "embgate" if emb else "finish"
        base = lstm_call(L, c, d, dev, emb)
        h = base["h_out"][:M]
        err = check_lstm(f"{name} base", c, base, [t.to(dev) for t in T.lstm_finish_ref(c, emb)], h)
        print(f"tile_path lstm_{name} nparts={nparts} R={R} M={M} gb_div={gb_div}: max |c' - ref| = {err:.3e}")
        again = lstm_call(L, c, d, dev, emb)
        assert all(torch.equal(base[k].view(torch.int16), again[k].view(torch.int16)) for k in ("c_out", "h_out", "f1", "f2"))
        for null in T.LSTM_NULLABLE:
            o = lstm_call(L, c, d, dev, emb, null)
            ref = [t.to(dev) for t in T.lstm_finish_ref(c, emb, null)]
            if null in ("h_out", "frag1", "frag2"):               # the other outputs are the base launch's, bit for bit
                check_lstm(f"{name} null {null}", c, o, ref, h, null)
                assert same_bits(o["c_out"][:M], base["c_out"][:M])
            else:
                check_lstm(f"{name} null {null}", c, o, ref, o["h_out"][:M], null)


@pytest.mark.parametrize("nparts,R,M", [(1, 16, 33), (8, 64, 70), (3, 48, 31)])
def test_tile_lstm_finish_saturated_gates_and_large_cell_states(dev, lib, nparts, R, M):
    """pre-activations of +-30 / +-100 with c = +-1e4: finite, c' within OP_TOL relative to |c'|"""
    L = lib.lib()
    c = T.lstm_inputs(77 + nparts, nparts, R, M, 1, saturated=True)
    d = {k: v.to(dev) for k, v in c.items() if isinstance(v, torch.Tensor)}
    for emb in (False, True):
        o = lstm_call(L, c, d, dev, emb)
        ref = [t.to(dev) for t in T.lstm_finish_ref(c, emb)]
        check_lstm(f"saturated emb={emb}", c, o, ref, o["h_out"][:M])
        rel = float(((o["c_out"][:M].double() - ref[0]).abs() / ref[0].abs().clamp_min(1.0)).max())
        print(f"tile_path lstm saturated nparts={nparts} R={R} M={M} emb={emb}: max |c' - ref| / max(|c'|, 1) = {rel:.3e}")
        again = lstm_call(L, c, d, dev, emb)
        assert all(torch.equal(o[k].view(torch.int16), again[k].view(torch.int16)) for k in ("c_out", "h_out", "f1", "f2"))


# ------------------------------------------------------------------ 3. packers and the beam-state reorder (bitwise)
@pytest.mark.parametrize("E,with_parent,beam,rows,R", T.REORDER_CASES)
def test_tile_reorder_pack_bitwise(dev, lib, E, with_parent, beam, rows, R):
    """xa = [h_lang[src] | relu(table[word]) | h_att[src]] (E = 0: no embedding segment, table NULL), xl's third segment, the two cell
    states; words outside [0, V) read row 0; the first two segments of xl, the k step behind xa and rows >= `rows` keep the fill"""
    L = lib.lib()
    c = T.reorder_inputs(E * 100 + rows + R + beam, E, with_parent, beam, rows, R)
    d = {k: v.to(dev) for k, v in c.items() if isinstance(v, torch.Tensor)}
    xa_ref, hl, ca, cl = (t.to(dev) for t in T.reorder_ref(c))
    nb = (rows + 31) // 32 + 1
    outs = []
    for _ in range(2):
        xa, xl = frag_fill(nb, (2 * R + E) // 16 + 1, dev), frag_fill(nb, 3 * R // 16, dev)
        cap, clp = nan_buf(rows + 1, R, dev=dev), nan_buf(rows + 1, R, dev=dev)
        rc = L.cvc_tile_reorder_pack(P(d.get("parent")), d["word"].data_ptr(), beam, d["h_att"].data_ptr(), d["c_att"].data_ptr(),
                                     d["h_lang"].data_ptr(), d["c_lang"].data_ptr(), P(d.get("table")), E, T.REORDER_V, cap.data_ptr(),
                                     clp.data_ptr(), *frag_at(xa, 0), *frag_at(xl, 2 * R // 16), rows, R, st())
        assert rc == 0
        outs.append((xa, xl, cap, clp))
    xa, xl, cap, clp = outs[0]
    assert expect_planes(xa, rows, 0, T.split3(xa_ref)), "xa"
    assert expect_planes(xl, rows, 2 * R, T.split3(hl)), "xl"
    assert same_bits(cap[:rows], ca) and same_bits(clp[:rows], cl) and all_nan(cap[rows:]) and all_nan(clp[rows:])
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(outs[0], outs[1]))


@pytest.mark.parametrize("M,K,ldx,koff", T.PACK_ROWS_CASES)
def test_tile_pack_rows_gather_and_relu_bitwise(dev, lib, M, K, ldx, koff):
    """plain, and with idx (repeated, out-of-order rows) + ReLU; ldx > K; a k offset inside a wider buffer; rows >= M keep the fill"""
    L = lib.lib()
    g = T.gen(M + K)
    x = torch.randn(M + 3, ldx, generator=g).to(dev)
    idx = torch.randint(0, M + 3, (M,), generator=g).to(dev)
    if M > 2:
        idx[0], idx[1], idx[2] = M + 2, 0, M + 2
    nb = (M + 31) // 32 + 1
    for ix, relu in ((None, 0), (idx, 1), (idx, 0), (None, 1)):
        xb, xb2 = frag_fill(nb, K // 16 + koff + 1, dev), frag_fill(nb, K // 16 + koff + 1, dev)
        for buf in (xb, xb2):
            assert L.cvc_tile_pack_rows(x.data_ptr(), ldx, P(ix), relu, M, K, *frag_at(buf, koff), st()) == 0
        assert torch.equal(xb, xb2), "two launches of one case differ"
        src = (x[:M] if ix is None else x[ix])[:, :K]
        assert expect_planes(xb, M, koff * 16, T.split3(torch.relu(src) if relu else src)), (ix is not None, relu)


def test_tile_pack_rows_any_both_forms_bitwise(dev, lib):
    """What is written, and by whom (include/cvc_hip.h): the fragment-shaped form (K % 16 == 0, 16-byte aligned, ldx % 4 == 0) writes
    whole fragments -- rows [M, 32 ceil(M / 32)) as zeros; the scalar form writes the ceil(K / 4) quads of rows < M -- zeros from K to the
    end of the last quad, the rest of the last k step and rows >= M are the CALLER's to clear"""
    L = lib.lib()
    for M, K, ldx in T.PACK_ANY_BLK:
        x = torch.randn(M, ldx, generator=T.gen(M + K)).to(dev)
        nb = (M + 31) // 32 + 1
        xb, xb2 = frag_fill(nb, K // 16 + 1, dev), frag_fill(nb, K // 16 + 1, dev)
        for buf in (xb, xb2):
            assert L.cvc_tile_pack_rows_any(x.data_ptr(), ldx, M, K, *frag_at(buf, 0), st()) == 0
        assert torch.equal(xb, xb2), "two launches of one case differ"
        want = torch.zeros(3, (nb - 1) * 32, K, dtype=torch.int16, device=dev)
        want[:, :M] = T.split3(x[:, :K])
        assert expect_planes(xb, (nb - 1) * 32, 0, want), ("fragment-shaped", M, K, ldx)
    for M, K, ldx, off in T.PACK_ANY_SCALAR:
        flat = torch.randn(M * ldx + 4, generator=T.gen(M + K + ldx)).to(dev)
        x = flat[off:off + M * ldx].view(M, ldx)
        assert K % 16 != 0 or ldx % 4 != 0 or x.data_ptr() % 16 != 0
        nb = (M + 31) // 32 + 1
        xb, xb2 = frag_fill(nb, (K + 15) // 16 + 1, dev), frag_fill(nb, (K + 15) // 16 + 1, dev)
        for buf in (xb, xb2):
            assert L.cvc_tile_pack_rows_any(x.data_ptr(), ldx, M, K, *frag_at(buf, 0), st()) == 0
        assert torch.equal(xb, xb2), "two launches of one case differ"
        xp = torch.zeros(M, (K + 3) // 4 * 4, device=dev)
        xp[:, :K] = x[:, :K]
        assert expect_planes(xb, M, 0, T.split3(xp)), ("scalar", M, K, ldx, off)


def test_tile_pack_cols_bitwise(dev, lib):
    """x [S, C] read as its transpose: every fragment of the ceil(C / 32) x ceil(S / 16) it touches is written whole, zero beyond C and
    S; ldx > C"""
    L = lib.lib()
    for S in T.PACK_COLS_S:
        for C in T.PACK_COLS_C:
            ldx = C + 3
            x = torch.randn(S, ldx, generator=T.gen(S * 131 + C)).to(dev)
            nb, ks = (C + 31) // 32, (S + 15) // 16
            xb, xb2 = frag_fill(nb + 1, ks + 1, dev), frag_fill(nb + 1, ks + 1, dev)
            for buf in (xb, xb2):
                assert L.cvc_tile_pack_cols(x.data_ptr(), ldx, S, C, *frag_at(buf, 0), st()) == 0
            assert torch.equal(xb, xb2), "two launches of one case differ"
            xp = torch.zeros(nb * 32, ks * 16, device=dev)
            xp[:C, :S] = x[:, :C].t()
            assert expect_planes(xb, nb * 32, 0, T.split3(xp)), (S, C)


# ------------------------------------------------------------------ 4. beam bookkeeping
def beam_run(L, c, dev, shift=0):
    """cvc_beam_select (one finished matrix) or cvc_beam_select_parts (slabs + bias); shift = 1: the logits start one float off
    alignment, which sends an aligned case to the general scan -> (rc, parent, word, score, done)"""
    rows, V, nparts, stride = c["B"] * c["beam"], c["V"], c["nparts"], c["part_stride"]
    buf = nan_buf(nparts * stride + 8, dev=dev)
    for p in range(nparts):
        buf[shift + p * stride:shift + p * stride + rows * V] = c["parts"][p].reshape(-1).to(dev)
    bias = None
    if c["bias_v"] is not None:
        bo = 1 if c["bias_shift"] else 0
        bias = nan_buf(V + 4, dev=dev)
        bias[bo:bo + V] = c["bias_v"].to(dev)
        bias = bias[bo:bo + V]
    score, done = c["score"].to(dev), c["done"].to(dev)
    parent = torch.full((rows,), SENT, dtype=torch.int64, device=dev)
    word = torch.full((rows,), SENT, dtype=torch.int64, device=dev)
    score_out = nan_buf(rows, dev=dev)
    done_out = torch.full((rows,), DONE_FILL, dtype=torch.uint8, device=dev)
    ws = nan_buf(17 * rows, dev=dev)
    lp = buf.data_ptr() + 4 * shift
    if nparts == 1 and bias is None:
        rc = L.cvc_beam_select(lp, score.data_ptr(), done.data_ptr(), c["B"], c["beam"], V, c["unk"], int(c["first"]), parent.data_ptr(),
                               word.data_ptr(), score_out.data_ptr(), done_out.data_ptr(), ws.data_ptr(), st())
    else:
        rc = L.cvc_beam_select_parts(lp, nparts, stride, P(bias), score.data_ptr(), done.data_ptr(), c["B"], c["beam"], V, c["unk"],
                                     int(c["first"]), parent.data_ptr(), word.data_ptr(), score_out.data_ptr(), done_out.data_ptr(),
                                     ws.data_ptr(), st())
    return rc, parent, word, score_out, done_out


def check_beam(what, c, out, dev):
    rc, parent, word, score, done = out
    B, beam, V = c["B"], c["beam"], c["V"]
    r = {k: v.to(dev) for k, v in c["ref"].items()}
    assert rc == 0, (what, rc)
    parent, word, score, done = parent.view(B, beam), word.view(B, beam), score.view(B, beam), done.view(B, beam)
    assert bool(((parent >= 0) & (parent < beam) & (word >= 0) & (word < V)).all()), f"{what}: parent / word out of range"
    live = r["live"]
    assert torch.equal(parent[live], r["parent"][live]), f"{what}: parent"
    assert torch.equal(word[live], r["word"][live]), f"{what}: word"
    assert torch.equal(done[live].bool(), r["done"][live]) and bool((done <= 1).all()), f"{what}: done"
    close(score[live], r["score"][live].float(), **SCORE_TOL)
    return float((score[live].double() - r["score"][live]).abs().max()) if bool(live.any()) else 0.0


@pytest.mark.parametrize("name", T.BEAM_NAMES)
def test_beam_select_exact_against_the_fp64_scan(dev, lib, name):
    """parent, word and done exact, scores at 1e-5 (fewer finite candidates than beam: on the live prefix, fillers in range); two
    launches bitwise equal; an integer case of the float4 scan also runs one float off alignment (the general scan on the same values)
    and must agree bit for bit in parent, word, score and done"""
    L = lib.lib()
    c = T.shared_beam_case(name)
    first = beam_run(L, c, dev)
    err = check_beam(name, c, first, dev)
    print(f"tile_path beam {name} fast={T.fast_form(c)}: max |score - ref| = {err:.3e}")
    again = beam_run(L, c, dev)
    assert all(torch.equal(a, b) or (a.dtype == torch.float32 and same_bits(a, b)) for a, b in zip(first[1:], again[1:]))
    if T.fast_form(c):                     # one float off alignment: the general scan on the same values
        check_beam(name + " (general scan)", c, beam_run(L, c, dev, shift=1), dev)


EXACT_FAST = [n for n in T.BEAM_NAMES if not n.startswith(("random", "general", "fallback"))]


@pytest.mark.parametrize("name", EXACT_FAST)
def test_beam_float4_and_general_scans_agree_bit_for_bit(dev, lib, name):
    """The integer cases of the float4 scan against the general scan on the same values (the logits one float off alignment):
    parent, word, score and done bit for bit, on the live prefix.  Both scans give a thread the same elements and share all code
    behind the loads (csrc/beam.hip::beam_rowtop4_kernel), so their log-sum-exp agree to the bit.  Before they did -- a general scan
    with its own element order and a block-wide max / sum -- 21 of these 31 cases failed here on the score (1 - 2 ulp, up to 9.5e-7;
    parent, word and done agreed): profiles/tile_path_pins.md."""
    L = lib.lib()
    c = T.shared_beam_case(name)
    assert T.fast_form(c)
    first, other = beam_run(L, c, dev), beam_run(L, c, dev, shift=1)
    assert first[0] == 0 and other[0] == 0
    live = c["ref"]["live"].view(-1).to(dev)
    d = (first[3][live].double() - other[3][live].double()).abs()
    print(f"tile_path beam {name} float4 vs general scan: scores differ in {int((d > 0).sum())} of {int(live.sum())}, largest {float(d.max()):.3e}")
    for a, b, what in zip(first[1:], other[1:], ("parent", "word", "score", "done")):
        a, b = a[live], b[live]
        assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b), f"{name}: {what} of the two scans differs"


@pytest.mark.parametrize("B,beam,T_,N", T.BACKTRACK_CASES)
def test_beam_backtrack_against_host_indexing(dev, lib, B, beam, T_, N):
    """seq and att_out bitwise; the attention row of step t is the PARENT row's; parents outside [0, beam) are clamped"""
    L = lib.lib()
    c = T.backtrack_inputs(B + beam + T_ + N, B, beam, T_, N)
    seq_ref, att_ref = T.backtrack_ref(c)
    words, parent, att = c["words"].to(dev), c["parent"].to(dev), c["att"].to(dev)
    outs = []
    for _ in range(2):
        seq = torch.full((B * T_ + 1,), SENT, dtype=torch.int64, device=dev)
        att_out = nan_buf(B * T_ * N + 1, dev=dev)
        assert L.cvc_beam_backtrack(words.data_ptr(), parent.data_ptr(), att.data_ptr(), B, beam, T_, N, seq.data_ptr(), att_out.data_ptr(), st()) == 0
        outs.append((seq, att_out))
    seq, att_out = outs[0]
    assert int(seq[-1]) == SENT and all_nan(att_out[-1:])
    assert torch.equal(seq[:-1].view(B, T_).cpu(), seq_ref)
    assert same_bits(att_out[:-1].view(B, T_, N).cpu(), att_ref)
    assert torch.equal(outs[1][0], seq) and same_bits(outs[1][1][:-1], att_out[:-1])


@pytest.mark.parametrize("width,beam", T.GATHER_CASES)
def test_gather_rows_bitwise(dev, lib, width, beam):
    L = lib.lib()
    rows = 3 * beam
    g = T.gen(width + beam)
    src = torch.randn(rows, width, generator=g).to(dev)
    parent = torch.randint(0, beam, (rows,), generator=g).to(dev)
    dst, dst2 = nan_buf(rows + 1, width, dev=dev), nan_buf(rows + 1, width, dev=dev)
    for buf in (dst, dst2):
        assert L.cvc_gather_rows(src.data_ptr(), parent.data_ptr(), rows, beam, width, buf.data_ptr(), st()) == 0
    assert same_bits(dst, dst2), "two launches of one case differ"
    want = src[(torch.arange(rows, device=dev) // beam) * beam + parent]
    assert same_bits(dst[:rows], want) and all_nan(dst[rows:])


# ------------------------------------------------------------------ 5. refusals: nothing is launched, outputs keep their fill
def test_refusals_leave_the_outputs_untouched(dev, lib):
    L = lib.lib()
    M, N, K = 33, 50, 64
    X, W = (t.to(dev) for t in T.census_case(5, M, N, K))
    xb, wb = T.census_frags(X, W)
    xp, xs = frag_at(xb, 0)
    out = nan_buf(2, M * N, dev=dev)
    g = lambda wptr, xptr, xstr, k, ks, ld: L.cvc_tile_gemm(wptr, xptr, xstr, k, M, N, ks, out.data_ptr(), ld, M * N, st())
    wp = wb.data_ptr()
    assert g(wp, xp, xs, K, 1, N) == 0                                            # (the arguments are good)
    out.fill_(float("nan"))
    for bad in ((wp, xp, xs, 0, 1, N), (wp, xp, xs, 24, 1, N), (wp, xp, xs, K, 5, N), (wp, xp, xs, K, 1, N - 1), (wp + 8, xp, xs, K, 1, N),
                (wp, xp + 8, xs, K, 1, N), (wp, xp, xs + 4, K, 1, N)):
        assert g(*bad) == E_BADARG, bad[2:]
    # finishers
    parts = torch.randn(2, 4, 64, device=dev)
    y = out[0, :4 * 16].view(4, 16)
    lf = lambda ld, ldy: L.cvc_tile_linear_finish(parts.data_ptr(), 2, 4 * 64, ld, None, None, 4, 16, y.data_ptr(), ldy, st())
    assert lf(15, 16) == E_BADARG and lf(16, 15) == E_BADARG
    c_prev, f1 = torch.randn(4, 32, device=dev), frag_fill(1, 2, dev)
    c_out, h_out = out[1, :128].view(4, 32), out[1, 128:256].view(4, 32)
    fin = lambda R, gb_div: L.cvc_tile_lstm_finish(parts.data_ptr(), 1, 4 * 64, None, None, None, gb_div, c_prev.data_ptr(), 4, R,
                                                   c_out.data_ptr(), h_out.data_ptr(), *frag_at(f1, 0), None, 0, st())
    assert fin(24, 1) == E_BADARG and fin(16, 0) == E_BADARG
    word = torch.zeros(4, dtype=torch.int64, device=dev)
    assert L.cvc_tile_lstm_finish_embgate(parts.data_ptr(), 1, 4 * 64, None, None, None, 0, parts.data_ptr(), word.data_ptr(), 1,
                                          c_prev.data_ptr(), 4, 16, c_out.data_ptr(), h_out.data_ptr(), *frag_at(f1, 0), None, 0, st()) == E_BADARG
    # reorder: E % 16 != 0, NULL table with E > 0
    h = torch.randn(4, 16, device=dev)
    ro = lambda table, E: L.cvc_tile_reorder_pack(None, word.data_ptr(), 1, h.data_ptr(), h.data_ptr(), h.data_ptr(), h.data_ptr(), table, E, 3,
                                                  c_out.data_ptr(), h_out.data_ptr(), *frag_at(f1, 0), *frag_at(f1, 1), 4, 16, st())
    assert ro(parts.data_ptr(), 8) == E_BADARG and ro(None, 16) == E_BADARG
    # beam select: beam 0 and 9, V = beam, V = 8193, nparts = 0
    logits = torch.randn(16, 16, device=dev)
    score, done = torch.zeros(16, device=dev), torch.zeros(16, dtype=torch.uint8, device=dev)
    parent = torch.full((16,), SENT, dtype=torch.int64, device=dev)
    wout = torch.full((16,), SENT, dtype=torch.int64, device=dev)
    dout = torch.full((16,), DONE_FILL, dtype=torch.uint8, device=dev)
    ws = out[0, 64:64 + 17 * 16]
    sel = lambda beam, V: L.cvc_beam_select(logits.data_ptr(), score.data_ptr(), done.data_ptr(), 1, beam, V, 1, 0, parent.data_ptr(),
                                            wout.data_ptr(), out[1, 256:272].data_ptr(), dout.data_ptr(), ws.data_ptr(), st())
    assert sel(0, 16) == E_BADARG and sel(9, 16) == E_BADARG and sel(4, 4) == E_BADARG and sel(2, 8193) == E_BADARG
    assert L.cvc_beam_select_parts(logits.data_ptr(), 0, 0, None, score.data_ptr(), done.data_ptr(), 1, 2, 16, 1, 0, parent.data_ptr(),
                                   wout.data_ptr(), out[1, 256:272].data_ptr(), dout.data_ptr(), ws.data_ptr(), st()) == E_BADARG
    # back-track: T = 0 and 257; gather: width % 4 != 0
    bt = lambda T_: L.cvc_beam_backtrack(word.data_ptr(), word.data_ptr(), logits.data_ptr(), 1, 1, T_, 1, wout.data_ptr(),
                                         out[1, 256:272].data_ptr(), st())
    assert bt(0) == E_BADARG and bt(257) == E_BADARG
    assert L.cvc_gather_rows(logits.data_ptr(), word.data_ptr(), 2, 1, 6, out.data_ptr(), st()) == E_BADARG
    torch.cuda.synchronize()
    assert all_nan(out) and bool((f1 == FILL16).all())
    assert bool((parent == SENT).all()) and bool((wout == SENT).all()) and bool((dout == DONE_FILL).all())
