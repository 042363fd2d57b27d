"""GPU tests (pytest -m gpu) of the decode attention step's entry points (csrc/attn_scores.h, csrc/attn_fwd.hip), each called
through the C-ABI as the decode and training paths call it and compared ELEMENT-WISE with a torch fp64 restatement
(tests/attn_step_cases.py): the split-K query planes of cvc_attn_scores_qparts, the query list split across launches, every width
instantiation, the `stream` bits, the quad / fragment / double-written layouts of the weighted sum, cvc_attn_weighted_rows and
its group step-down, and the forms that only an environment setting or a chip-sized launch selects.

Every output buffer is pre-filled with NaN (0x7FC0 for int16 fragments), so an element nobody wrote and an element written where
none belongs both fail.  Where a path is chosen by shape, the arithmetic that chooses it stands beside the case.

Tolerances: OP_TOL (rtol = atol = 2e-5) on scores and raw weighted rows, with alpha_net's weight scaled by 0.3 sqrt(256 / A) and dot
queries by 1 / sqrt(A) so that scores keep the magnitude they have at A = 256 (an fp32 restatement summed sequentially stays within
1.4e-5 of fp64 up to A = 4096 with 16 planes); attn rtol 2e-5 / atol 2e-6 and contexts rtol = atol = 2e-5 as in
test_gpu_parity.py::test_two_set_weighted_sum_at_the_edges_of_its_hoisted_forms.  Layout variants of one sum are BITWISE equal."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_step_cases as K
from attn_step_cases import E_BADARG, E_TOOBIG, all_nan, close, nan_buf, same_bits, stream_handle

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


# ------------------------------------------------------------------ 1. score pass: planes, bias, widths, masks, fills
# Width: launch_scores_q takes nch = ceil(A / 256) and the next compiled NCH of 1 / 2 / 4 / 8 / 16; the EXACT (guard-free) form of
# the factored loop needs A == NCH * 256.
#   A = 20 -> NCH 1 | 256 -> 1 exact | 260 -> 2 | 1024 -> 4 exact | 1028 -> nch 5 -> 8 | 2048 -> 8 exact | 2052 -> nch 9 -> 16
#   | 4096 -> 16 (one query per launch there: (1 + 1) * 4096 * 4 = 32 KiB fits, a padded group of 4 or 5 does not)
# Group: score_group(nq) = 1, 4 (3 padded), 5; for A <= 2052 all of nq <= 5 queries fit one launch
# ((5 + 1) * 2052 * 4 = 49 248 <= 65 536), so the group is that of nq.
# Chunk: one query scores 32 rows per workgroup (n = 31 / 32 / 33 around it, 130 = 5 chunks); several queries 8 (see section 5).
# sum_planes: fixed forms for 1 / 2 / 4 / 8 / 16 planes, the run-time loop for 3.
# (P, bias, A, nq, (n0, n1), stream, big)        big: (row, col) of a planted q = 12 > 10.4 -> that clip's workgroups go direct
SCORE_CASES = [
    (1, False, 20, 1, (1, 33), 0, None),
    (2, True, 256, 3, (31, 32), 1, None),
    (2, True, 256, 3, (31, 32), 1, (4, 17)),            # clip 1's workgroups take the direct form, the others the factored one
    (3, True, 260, 5, (33, 130), 4, None),
    (4, False, 1024, 1, (32, 31), 5, None),
    (8, True, 1028, 5, (130, 1), 0, None),
    (16, True, 2048, 3, (33, 32), 1, None),
    (3, False, 2052, 5, (31, 130), 4, None),
    (3, False, 2052, 5, (31, 130), 4, (2, 2051)),       # clip 0 direct at NCH 16, in the last (ragged) column group
    (16, False, 4096, 3, (130, 33), 5, None),
    (8, True, 2048, 1, (32, 1), 4, None),
    (2, False, 4096, 1, (33, 31), 0, None),
    (4, True, 1024, 5, (1, 130), 5, None),              # NCH 4 exact, group of 5
]


# (the direct / factored choice exists in the additive form only: the planted cases are not repeated for dot)
@pytest.mark.parametrize("kind,P,bias,A,nq,ns,stream,big", [(k,) + c for c in SCORE_CASES for k in ("additive", "dot")
                                                            if not (k == "dot" and c[6] is not None)])
def test_score_pass_planes_bias_widths_masks_and_fills_vs_fp64(dev, lib, kind, P, bias, A, nq, ns, stream, big):
    """cvc_attn_scores_qparts on two sets (set 0: region mask with clip 3 of 4 fully masked, frame mask; set 1: neither) against
    q = sum of planes + bias in fp64; then cvc_attn_scores on plane 0 alone, the P = 1 / no-bias baseline, on the same sets."""
    c = K.score_case(A * 131 + P * 7 + nq, kind, 4, nq, A, ns, P=P, bias=bias, big=None if big is None else (big[0], big[1], 12.0))
    rc, got, attns = K.run_scores(lib, dev, c, stream)
    assert rc == 0, rc
    K.check_scores(c, got, K.ref_scores(c, dev, stream), attns, stream)
    fill = -math.inf if stream & 4 else K.MIN_VALUE
    assert bool((got[0][0][3 * nq:] == fill).all())                      # the fully masked clip
    rc, got, attns = K.run_scores(lib, dev, c, stream, qparts=False)
    assert rc == 0, rc
    K.check_scores(c, got, K.ref_scores(c, dev, stream, planes=1), attns, stream)


def test_score_pass_exact_factored_form_at_2048_with_clamped_and_direct_clips(dev, lib):
    """A = 2048, nq = 5: NCH 8 with A == 8 * 256 -> the EXACT factored loop.  Planted as in
    test_gpu_parity.py::test_multi_query_additive_scores_large_values_take_the_direct_form: clip 0 holds q = -44 (direct form;
    p = 45 there is tanh(1)), clip 1 stays factored with p = 45, -60, 1e30 (C p clamped to +-62) and p = 21 (unclamped), clip 2
    holds a big query on another row; clip 3 is fully masked."""
    nq, A = 5, 2048
    c = K.score_case(2048, "additive", 4, nq, A, (33, 9), P=8, bias=True)
    q = c["qp"].double().sum(0) + c["qb"].double()
    for row, col, val in ((0, 5, -44.0), (2 * nq + 1, 2047, -44.0)):
        c["qp"][0, row, col] += val - float(q[row, col])
    P0 = c["proj"][0]
    P0[0, 3, 5], P0[0, 3, 6], P0[1, 20, 0] = 45.0, -60.0, 21.0
    P0[1, 21, 3], P0[1, 22, 4], P0[1, 22, 2047] = 45.0, -60.0, 1e30
    c["mask"][0, 3], c["mask"][1, 20:23] = 0, 0
    rc, got, attns = K.run_scores(lib, dev, c)
    assert rc == 0, rc
    K.check_scores(c, got, K.ref_scores(c, dev), attns)


@pytest.mark.parametrize("kind", ["additive", "dot"])
@pytest.mark.parametrize("A", [4100, 16384])
def test_score_pass_refuses_widths_beyond_its_templates(dev, lib, kind, A):
    """A = 4100: one query fits the LDS (2 * 4100 * 4 = 32 800) but nch = 17 > 16; A = 16384: 65 536 / (16384 * 4) - 1 = 0
    queries per launch.  Both CVC_E_TOOBIG, outputs untouched."""
    c = K.score_case(A, kind, 1, 2, A, (3,), P=2, bias=True)
    for qparts in (True, False):
        rc, got, attns = K.run_scores(lib, dev, c, qparts=qparts)
        assert rc == E_TOOBIG, rc
        assert all_nan(got[0][0]) and all_nan(got[0][1]) and all_nan(attns[0])


# ------------------------------------------------------------------ 2. query list split across launches
# run_scores: q_per_launch = 65 536 / (4 A) - 1, cut to whole groups of 5 when it is below nq, then lowered until the PADDED list
# plus alpha_net's weight fits: (pad(q) + 1) * A * 4 <= 65 536.
#   (20, 1024): 16 - 1 = 15 -> (15 + 1) * 4096 = 65 536 fits                       -> launches of 15 + 5, q0 = 0, 15
#   (7, 2048):  8 - 1 = 7 (not below nq): group 4 pads to 8, 9 * 8192 > 64 Ki; 6 -> 8, no; 5 -> 6 * 8192 fits -> 5 + 2, q0 = 0, 5
#   (5, 4096):  4 - 1 = 3: pads to 4, 5 * 16 384 no; 2 -> 4, no; 1 -> 2 * 16 384 fits    -> five launches of one query
#   (30, 2048): 7 -> whole groups: 5 -> 6 * 8192 fits                              -> six launches of 5, q0 = 0, 5, ..., 25
# (nq, A, n, index of the big query inside clip 0 -- in a launch after the first)
SPLIT_CASES = [(20, 1024, 37, 17), (7, 2048, 33, 6), (5, 4096, 33, 3), (30, 2048, 9, 27)]


@pytest.mark.parametrize("mode", ["additive", "additive_big_in_a_later_launch", "dot"])
@pytest.mark.parametrize("nq,A,n,big_q", SPLIT_CASES)
def test_query_list_split_across_launches_vs_fp64(dev, lib, mode, nq, A, n, big_q):
    """cvc_attn_scores, one masked set (clip 1 of 2 fully masked), every row of every launch against fp64: a wrong q0 offset on the
    read side scores another query, on the write side leaves NaN behind.  With the big query only the launch that stages it runs
    clip 0 in the direct form."""
    kind = "dot" if mode == "dot" else "additive"
    big = (big_q, 11, 12.0) if mode == "additive_big_in_a_later_launch" else None
    c = K.score_case(nq * 1000 + A, kind, 2, nq, A, (n,), big=big)
    rc, got, attns = K.run_scores(lib, dev, c, qparts=False)
    assert rc == 0, rc
    K.check_scores(c, got, K.ref_scores(c, dev), attns)


# ------------------------------------------------------------------ 3. weighted-sum layouts
def _rm(lib, dev, c, **kw):
    rc, attn, cout, tot, scs = K.run_wsum_rm(lib, dev, c, **kw)
    assert rc == 0, rc
    return attn, cout, tot, scs


def _same_attn_and_ctx(a, b):
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert (x is None) == (y is None)
        if x is not None:
            assert same_bits(x, y)


def _quad(lib, dev, c, R, **kw):
    """cvc_attn_wsum_quad into columns [R, 2R) of a [3R / 4][64][4] quad buffer (the packed path's XL holds three operands side by
    side) -> (rc, attn, ctx_out, the buffer)"""
    buf = nan_buf(3 * R // 4, 64, 4, dev=dev)
    L = lib.lib()
    dst = buf.data_ptr() + (R // 4) * 64 * 4 * 4
    rc, attn, cout, _ = K.run_wsum(lib, dev, c, lambda arr, ns, nclip, nq, R_, st: L.cvc_attn_wsum_quad(arr, ns, nclip, nq, R_, dst, st), **kw)
    return rc, attn, cout, buf


def _check_quad(buf, R, rows, tot):
    from cvc.decode.weights import from_quad
    mid = buf[R // 4:2 * R // 4]
    assert same_bits(from_quad(mid, rows).contiguous(), tot), "the quad layout must hold the row-major sum bit for bit"
    assert all_nan(buf[:R // 4]) and all_nan(buf[2 * R // 4:]) and all_nan(mid[:, rows:]), "written outside [0, R) x [0, rows)"


# rows = nclip * nq <= 64.  nq = 1: the one-query kernel (hoisted: n <= 512); nq = 5: attn_wsum_mq_kernel<5, 8, true> (QB 5,
# n_max <= 512, (R / 256 blocks) * nclip * 1 <= 512 workgroups -> 8 waves).  (rows of 37 or 1 cannot be had with nq = 5: 60 there.)
@pytest.mark.parametrize("ctx_out", [False, True])
@pytest.mark.parametrize("nclip,nq,R", [(1, 1, 64), (37, 1, 272), (64, 1, 64), (12, 5, 272), (1, 5, 64)])
def test_weighted_sum_quad_layout_equals_row_major_bitwise(dev, lib, nclip, nq, R, ctx_out):
    c = K.wsum_case(nclip * 10 + nq, nclip, nq, (70, 17), R)
    rows = nclip * nq
    attn, cout, tot, _ = _rm(lib, dev, c, ctx_out=ctx_out)
    K.check_wsum(c, dev, attn, cout, tot)
    rc, attn_q, cout_q, buf = _quad(lib, dev, c, R, ctx_out=ctx_out)             # ctx_out null: the decode call shape, sum only
    assert rc == 0, rc
    _same_attn_and_ctx((attn, cout), (attn_q, cout_q))
    _check_quad(buf, R, rows, tot)


@pytest.mark.parametrize("nclip,nq", [(65, 1), (13, 5)])
def test_weighted_sum_quad_refuses_more_than_64_rows(dev, lib, nclip, nq):
    c = K.wsum_case(65, nclip, nq, (9, 4), 64)
    rc, attn, cout, buf = _quad(lib, dev, c, 64)
    assert rc == E_BADARG, rc
    assert all_nan(buf) and all(all_nan(t) for t in attn + cout), "a refused call launched something"


# rows M = nclip * nq over one or two 32-row blocks; (5, 1): one-query kernel, (1, 5): QB 5, (11, 3): QB 4 (nq <= 4),
# (16, 4): QB 4, (32, 1) / (64, 1): exactly one / two blocks.  R = 272 = 256 + 16: a second column block of four lanes.
@pytest.mark.parametrize("k0", [0, 32])
@pytest.mark.parametrize("nclip,nq,R", [(5, 1, 64), (1, 5, 272), (32, 1, 272), (11, 3, 64), (16, 4, 272), (64, 1, 64)])
def test_weighted_sum_fragment_layout_equals_row_major_bitwise(dev, lib, nclip, nq, R, k0):
    """cvc_attn_wsum_frag at column k0 of a fragment tensor 64 columns wider than R with one row block to spare: from_frag of the
    written k steps equals the row-major sum bitwise, the three bf16 planes are to_frag's (hi, mid, lo in that order), rows >= M and
    the other k steps keep 0x7FC0."""
    from cvc.decode.weights import from_frag, to_frag
    M = nclip * nq
    c = K.wsum_case(M * 3 + R + k0, nclip, nq, (40, 17), R)
    attn, cout, tot, _ = _rm(lib, dev, c)
    K.check_wsum(c, dev, attn, cout, tot)
    nb, ks = (M + 31) // 32 + 1, (R + 64) // 16
    xb = torch.full((nb, ks, 3, 2, 32, 8), K.FRAG_PATTERN, dtype=torch.int16, device=dev)
    ptr, stride = lib._frag_ptr(xb, k0)
    L = lib.lib()
    rc, attn_f, cout_f, _ = K.run_wsum(lib, dev, c, lambda arr, ns, ncl, nq_, R_, st: L.cvc_attn_wsum_frag(arr, ns, ncl, nq_, R_, ptr, stride, st))
    assert rc == 0, rc
    _same_attn_and_ctx((attn, cout), (attn_f, cout_f))
    sub = xb[:, k0 // 16:k0 // 16 + R // 16]
    assert same_bits(from_frag(sub.contiguous(), M).contiguous(), tot)
    live = (torch.arange(nb * 32, device=dev) < M).view(nb, 1, 1, 1, 32, 1).expand_as(sub)
    assert torch.equal(sub[live], to_frag(tot, nb * 32)[live]), "the stored planes are not (hi, mid, lo) of the sum"
    assert bool((sub[~live] == K.FRAG_PATTERN).all()), "rows >= M were written"
    assert bool((xb[:, :k0 // 16] == K.FRAG_PATTERN).all()) and bool((xb[:, k0 // 16 + R // 16:] == K.FRAG_PATTERN).all()), "other k steps were written"


@pytest.mark.parametrize("R,stride_off", [(24, 0), (64, 2)])
def test_weighted_sum_fragment_refuses_bad_width_and_stride(dev, lib, R, stride_off):
    c = K.wsum_case(R, 2, 1, (9,), R)
    xb = torch.full((2, 8, 3, 2, 32, 8), K.FRAG_PATTERN, dtype=torch.int16, device=dev)
    ptr, stride = lib._frag_ptr(xb)
    L = lib.lib()
    rc, attn, cout, _ = K.run_wsum(lib, dev, c, lambda arr, ns, ncl, nq, R_, st: L.cvc_attn_wsum_frag(arr, ns, ncl, nq, R_, ptr, stride + stride_off, st))
    assert rc == E_BADARG, rc
    assert bool((xb == K.FRAG_PATTERN).all()) and all(all_nan(t) for t in attn + cout)


@pytest.mark.parametrize("nclip,R", [(1, 64), (37, 272), (64, 256)])
def test_weighted_sum_training_form_writes_quad_and_row_major_bitwise(dev, lib, nclip, R):
    from cvc.decode.weights import from_quad
    c = K.wsum_case(nclip + R, nclip, 1, (70, 17), R)
    attn, cout, tot, _ = _rm(lib, dev, c)
    K.check_wsum(c, dev, attn, cout, tot)
    q, rm = nan_buf(R // 4, 64, 4, dev=dev), nan_buf(nclip, R, dev=dev)
    L = lib.lib()
    rc, attn2, cout2, _ = K.run_wsum(lib, dev, c, lambda arr, ns, ncl, nq, R_, st: L.cvc_attn_wsum_quad_rm(arr, ns, ncl, R_, q.data_ptr(), rm.data_ptr(), st))
    assert rc == 0, rc
    _same_attn_and_ctx((attn, cout), (attn2, cout2))
    assert same_bits(rm, tot) and same_bits(from_quad(q, nclip).contiguous(), tot)
    assert all_nan(q[:, nclip:])


def test_weighted_sum_training_form_refuses_65_clips(dev, lib):
    c = K.wsum_case(65, 65, 1, (9,), 64)
    q, rm = nan_buf(16, 64, 4, dev=dev), nan_buf(65, 64, dev=dev)
    L = lib.lib()
    rc, attn, cout, _ = K.run_wsum(lib, dev, c, lambda arr, ns, ncl, nq, R_, st: L.cvc_attn_wsum_quad_rm(arr, ns, ncl, R_, q.data_ptr(), rm.data_ptr(), st))
    assert rc == E_BADARG, rc
    assert all_nan(q) and all_nan(rm) and all(all_nan(t) for t in attn + cout)


# One-query kernel: HOIST when n_max <= 512 (513 -> the per-set form); in the hoisted form set 0's first 16 context rows are
# requested ahead of the softmax when n0 >= 16 (15 / 16 / 17).  nq = 5: QB 5, attn_wsum_mq_kernel<5, 8, true> while n_max <= 512
# (3 or 6 workgroups <= 512 -> eight waves), the per-set 4-wave attn_wsum_mq_kernel<5> at 513.
# stream bit 1: context rows read non-temporally.
@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("n0,n1,R,stream", [(15, 512, 64, 0), (16, 513, 256, 2), (17, 16, 272, 2), (512, 15, 272, 0), (513, 17, 64, 2),
                                            (16, 512, 256, 0)])
def test_weighted_sum_at_the_sizes_its_forms_switch_on(dev, lib, nq, n0, n1, R, stream):
    c = K.wsum_case(n0 * 7 + n1 + R + nq, 3, nq, (n0, n1), R)
    attn, cout, tot, scs = _rm(lib, dev, c, stream=stream)
    K.check_wsum(c, dev, attn, cout, tot)
    for s in range(2):
        assert same_bits(scs[s], c["scores"][s].to(dev)), "the weighted sum changed its input scores"
    rc, attn_q, cout_q, buf = _quad(lib, dev, c, R, ctx_out=False, stream=stream)
    assert rc == 0, rc
    _same_attn_and_ctx((attn, [None, None]), (attn_q, cout_q))
    _check_quad(buf, R, 3 * nq, tot)


@pytest.mark.parametrize("nq", [1, 5])
def test_weighted_sum_fully_minus_inf_row_is_nan_on_exactly_that_row(dev, lib, nq):
    """with_sentinel fill: a row of -inf throughout has no softmax (exp(-inf - -inf)): NaN in attn and in both contexts on that row,
    every other row finite and inside the tolerances; the quad layout carries the same."""
    from cvc.decode.weights import from_quad
    bad, R = 2 * nq - 1, 64
    c = K.wsum_case(nq, 3, nq, (33, 17), R, neg_inf_row=bad)
    attn, cout, tot, _ = _rm(lib, dev, c)
    ok = torch.ones(3 * nq, dtype=torch.bool, device=dev)
    ok[bad] = False
    assert all_nan(attn[0][bad]) and all_nan(cout[0][bad]) and all_nan(tot[bad])
    close(attn[0][bad], torch.full((33,), float("nan")), equal_nan=True)
    for t in (attn[0], attn[1], cout[0], cout[1]):
        assert bool(torch.isfinite(t[ok]).all())
    assert bool(torch.isfinite(attn[1][bad]).all()) and bool(torch.isfinite(cout[1][bad]).all())
    K.check_wsum(c, dev, attn, cout, tot, skip_rows=(bad,))
    rc, attn_q, _, buf = _quad(lib, dev, c, R, ctx_out=False)
    assert rc == 0, rc
    got = from_quad(buf[R // 4:2 * R // 4], 3 * nq).contiguous()
    assert all_nan(got[bad]) and same_bits(got[ok], tot[ok]) and same_bits(attn_q[0][ok], attn[0][ok])


@pytest.mark.parametrize("nq,ns", [(1, (33, 17)), (5, (33, 17)), (3, (600,))])
def test_weighted_sum_attention_only_call_writes_attn_and_nothing_else(dev, lib, nq, ns):
    c = K.wsum_case(nq + len(ns), 3, nq, ns, 64)
    attn, cout, tot, scs = _rm(lib, dev, c, ctx_out=False, want_sum=False)
    ra, _, _ = K.ref_wsum(c, dev)
    for s in range(len(ns)):
        close(attn[s], ra[s].float(), **K.ATTN_TOL)
        assert same_bits(scs[s], c["scores"][s].to(dev))
    full, _, _, _ = _rm(lib, dev, c)
    for s in range(len(ns)):
        assert same_bits(attn[s], full[s])


def test_weighted_sum_four_wave_hoisted_group_form_vs_fp64(dev, lib):
    """nclip = 520, nq = 5, n = (8, 5), R = 256: QB = 5, n_max <= 512, grid (256 / 256) x 520 x (5 / 5) = 520 workgroups > 2 * 256
    -> not eight waves; lds_h(4) = (4 * 5 * 256 + 16 + 2 * 5 * 8) * 4 = 20 864 <= 64 KiB -> attn_wsum_mq_kernel<5, 4, true>."""
    c = K.wsum_case(520, 520, 5, (8, 5), 256)
    attn, cout, tot, _ = _rm(lib, dev, c)
    K.check_wsum(c, dev, attn, cout, tot)


def test_weighted_sum_falls_through_to_the_one_query_kernel_with_two_queries(dev, lib):
    """nq = 2, n = 7200, R = 4: lds_of(2) = (4 * 2 * 256 + 16 + 2 * 7200) * 4 = 65 856 > 65 536 -> QB steps down to 1; the one-query
    kernel's (1024 + 16 + 7200) * 4 = 32 960 fits, n > 512 -> attn_wsum_kernel<false>, one workgroup per row.  The raw-weights
    mode has no one-query form: CVC_E_TOOBIG, output untouched."""
    c = K.wsum_case(7200, 2, 2, (7200,), 4)
    attn, cout, tot, _ = _rm(lib, dev, c)
    K.check_wsum(c, dev, attn, cout, tot)
    w, X, out = c["scores"][0].to(dev), c["ctx"][0].to(dev), nan_buf(4, 4, dev=dev)
    w0 = w.clone()
    rc = lib.lib().cvc_attn_weighted_rows(w.data_ptr(), X.data_ptr(), 2, 2, 7200, 4, 0.5, out.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert rc == E_TOOBIG, rc
    assert all_nan(out) and same_bits(w, w0)


# ------------------------------------------------------------------ 4. cvc_attn_weighted_rows
# Group: QB = 2 (nq <= 2), 4 (<= 4), 5 (== 5), else 10 when ceil(nq / 10) < ceil(nq / 8), else 8; stepped down 10 -> 8 -> 5 -> 4 -> 2
# while lds_of(QB) = (4 * QB * 256 + 16 + QB * n) * 4 > 65 536:
#   (2, 1) QB 2 | (3, 70) QB 4, one slot unused | (5, 512), (5, 513) QB 5 (the raw mode runs in the hoisted form too:
#   512 takes <5, 8, true>, 513 the per-set <5>) | (7, 70) 1 < 1 is false -> QB 8, one unused | (20, 70) 2 < 3 -> QB 10
#   | (20, 700) QB 10 needs 69 024 -> 8: 60 992 fits, groups 8 + 8 + 4 | (20, 1100) 10: 85 024, 8: 68 032 -> 5: 42 544, four groups
#   | (23, 70) 3 < 3 is false -> QB 8, groups 8 + 8 + 7
@pytest.mark.parametrize("R,scale", [(8, 1 / 1.7), (260, -2.0)])
@pytest.mark.parametrize("nq,n", [(2, 1), (3, 70), (5, 512), (5, 513), (7, 70), (20, 70), (20, 700), (20, 1100), (23, 70)])
def test_weighted_rows_vs_fp64_through_every_group_size(dev, lib, nq, n, R, scale):
    """out = scale * w @ X per clip: raw weights (signed, 1 / sqrt(n)), no softmax; `attn` aliases w in this mode and must not be
    written."""
    g = torch.Generator().manual_seed(nq * 10000 + n + R)
    nclip = 2
    w = (torch.randn(nclip * nq, n, generator=g) / math.sqrt(n)).to(dev)
    X = torch.randn(nclip, n, R, generator=g).to(dev)
    w0, out = w.clone(), nan_buf(nclip * nq, R, dev=dev)
    rc = lib.lib().cvc_attn_weighted_rows(w.data_ptr(), X.data_ptr(), nclip, nq, n, R, scale, out.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert rc == 0, rc
    ref = scale * torch.bmm(w0.double().view(nclip, nq, n), X.double()).reshape(-1, R)
    close(out, ref.float(), **K.OP_TOL)
    assert same_bits(w, w0), "the raw-weights mode wrote its weights"


@pytest.mark.parametrize("scale,n", [(0.0, 9), (1.0, 0)])
def test_weighted_rows_refuses_zero_scale_and_empty_sets(dev, lib, scale, n):
    w, X, out = torch.randn(6, 9, device=dev), torch.randn(2, 9, 8, device=dev), nan_buf(6, 8, dev=dev)
    rc = lib.lib().cvc_attn_weighted_rows(w.data_ptr(), X.data_ptr(), 2, 3, n, 8, scale, out.data_ptr(), stream_handle())
    torch.cuda.synchronize()
    assert rc == E_BADARG, rc
    assert all_nan(out)


# ------------------------------------------------------------------ 5. forms chosen by the environment
ENV_KEYS = ("CVC_SCORE_ROWS_RT", "CVC_WSUM_HOIST", "CVC_WSUM_MQ_HOIST", "CVC_WSUM_MQ_WAVES")
# rows per workgroup r -> ceil(r / 4) rows per wave = mask-ballot bits 0 .. ceil(r / 4) - 1: 4 -> bit 0; 36 -> bits 0 .. 8;
# 128 -> all 32 (by default score_rows_per_wg picks 8 at these sizes: one round of workgroups, the smallest r is cheapest -> bits 0, 1)
CHILD_ENVS = [
    dict(CVC_SCORE_ROWS_RT="4", CVC_WSUM_HOIST="0", CVC_WSUM_MQ_HOIST="0"),      # attn_wsum_kernel<false>, attn_wsum_mq_kernel<5, 8>
    dict(CVC_SCORE_ROWS_RT="36", CVC_WSUM_MQ_WAVES="4"),                         # attn_wsum_mq_kernel<5, 4, true>
    dict(CVC_SCORE_ROWS_RT="128", CVC_WSUM_MQ_WAVES="8"),                        # attn_wsum_mq_kernel<5, 8, true>
]


def _child(env_add, path):
    """attn_step_cases.main in a fresh interpreter (the settings are read once per process); no retry"""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    paths = [root, os.path.join(root, "cyclical-visual-captioning_amd"), here]
    code = f"import sys; sys.path[:0] = {paths!r}; import attn_step_cases as k; k.main({str(path)!r})"
    env = {k: v for k, v in os.environ.items() if k not in ENV_KEYS}
    env.update(env_add)
    r = subprocess.run([sys.executable, "-X", "faulthandler", "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=root)
    report = f"child {env_add}: rc={r.returncode}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-8000:]}"
    assert r.returncode == 0, report
    assert "ATTN-STEP-CHILD-OK" in r.stdout and "libcvc_hip.so" in r.stdout, report
    return dict(np.load(path))


def test_forms_chosen_by_environment_agree_bitwise_where_the_kernels_say_so(dev, lib, tmp_path):
    """The same cases in this process (defaults) and in three children, one after another, each of which checks them against fp64
    itself.  Across all four: scores are bitwise equal (a row's arithmetic does not depend on how rows are dealt to workgroups and
    waves) and so are the softmax weights (the hoisted forms' claim: same partial sums in the same order); the one-query contexts
    are bitwise equal with and without the hoist; the group form's contexts with 4 and with 8 waves differ in summation order and
    agree to the context tolerance."""
    for k in ENV_KEYS:
        assert k not in os.environ, f"{k} is set: this test compares against the process's default forms"
    runs = [K.env_cases(lib, dev)] + [_child(e, tmp_path / f"child{i}.npz") for i, e in enumerate(CHILD_ENVS)]
    base = runs[0]
    bitwise = [k for k in base if k.startswith(("scores.", "fm.")) or ".attn" in k or k.startswith("w1.")]
    assert len(bitwise) == 6 + 4 + 3
    for i, r in enumerate(runs[1:]):
        assert sorted(r) == sorted(base)
        for k in bitwise:
            assert np.array_equal(base[k].view(np.int32), r[k].view(np.int32)), (k, CHILD_ENVS[i])
    four, eight = runs[2], runs[3]
    for k in ("w5.ctx0", "w5.ctx1", "w5.sum"):
        np.testing.assert_allclose(four[k], eight[k], err_msg=k, **K.CTX_TOL)
        assert np.array_equal(base[k].view(np.int32), eight[k].view(np.int32)), k      # the default here IS the 8-wave hoisted form
