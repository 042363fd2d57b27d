"""GPU tests (pytest -m gpu) of the backward-data GEMM's entry points (csrc/gemm_nn.hip: cvc_linear_nn_fwd,
cvc_linear_nn_planes_fwd, cvc_linear_nn_planes2_fwd, cvc_pack_quad), each called through the C-ABI as cvc/hip.py, csrc/train_driver.hip
and the GRU / LSTM sequence backwards call it and compared ELEMENT-WISE with a torch fp64 restatement dY.double() @ W.double()
(tests/nn_gemm_cases.py) on the same fp32 operands cast up -- on ALL THREE kernels of the file:

  skinny_gemm_nn_kernel<MT>        fp32 MFMA, NW = 4 waves, ring depth CVC_NN_DEPTH = 3 over a wave's 8-row groups; split mode 0
  skinny_gemm_nn_split_kernel<MT>  bf16x3 split products, NW = 4, ring depth CVC_NNS_DEPTH = 4 over DOUBLE groups, an odd last group
                                   on the fp32 MFMA; split modes 1 and 2 (one template: bit-equal), the default
  skinny_gemm_nn_split128_kernel   the same arithmetic on two 64-row operand groups (128 rows), dY through LDS-DMA, NW = 4, ring
                                   depth CVC_NN128_DEPTH = 3, hand-counted vmcnt waits; cvc_linear_nn_planes2_fwd, modes 1 and 2
  (MT = 1 for M <= 32, MT = 2 above; at most NN_MAX_SEG = 6 segments; tests/test_nn_gemm_cpu.py asserts these constants)

and on nn_reduce_kernel, nn_reduce128_kernel (the plane sums) and pack_quad_kernel.

  1. the K loop: every branch of the three register rings, every row tile, vs fp64; 128-row rows bit-equal to the 64-row kernel's
  2. K slices: the reduced form, the plane form [ksplit_eff][M][ntot] against the fp64 product of each slice's own K rows, the
     slab padding, the clamp of ksplit to K / 8, the plane order of the sum, the 128-row planes and their sum
  3. six segments on column views of two weight matrices (ldw > ncols) into dst views (ld_dst > ncols); the minimum shape
  4. cvc_pack_quad, exact
  5. the split product is fp32-grade here too, where an odd group mixes an fp32-MFMA step into it

Every output buffer is pre-filled with NaN and is one row and four columns (a workspace: one plane) larger than the contract
writes: an element the contract says is written is compared, every other one must still be NaN.  Operands: dY ~ N(0, 1),
W ~ N(0, 1) / sqrt(K), so outputs have unit scale at every K.  Tolerance: the project's OP_TOL (rtol = atol = 2e-5, the bound of
tests/test_gpu_parity.py for fp32 kernels against fp64); a skipped or doubled 8-row group moves an output by about sqrt(8 / K) >= 0.1
at the largest K here.  Every other comparison is bitwise or exact; two launches of one case agree bit for bit.

What this file does NOT prove: the 128-row kernel's hand-counted `s_waitcnt vmcnt` waits are exercised on every branch, but a read
of a weight register or a ring slot before its load has landed depends on timing and need not show at these sizes."""
import pytest
import torch

import nn_gemm_cases as N
from nn_gemm_cases import MODES, OP_TOL, ROWS, all_nan, all_same_bits, same_bits

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


def second_rows(M):
    """rows of the second operand group of the 128-row form: both groups together cross every row tile"""
    return 64 if M == 1 else 65 - M


def fwd_in_every_mode(lib, tag, dyq, ref, K, M, wts, ksplit=1):
    """cvc_linear_nn_fwd in modes 0, 1, 2: vs fp64 within OP_TOL, nothing written outside the views, two launches bit-equal,
    mode 1 bit-equal to mode 2 -> {mode: written values per segment}"""
    vals = {}
    for mode in MODES:
        t = f"{tag} mode={mode} M={M} ksplit={ksplit}"
        with N.split_mode(lib, mode):
            rc, dsts, ws = N.run_nn(lib, "fwd", dyq, K, M, wts, ksplit)
            rc2, again, _ = N.run_nn(lib, "fwd", dyq, K, M, wts, ksplit)
        assert (rc, rc2) == (0, 0), (t, rc, rc2)
        N.check_dsts(t, dsts, ref, M, wts)
        assert all_same_bits(dsts, again), (t, "two launches of one case differ")
        if ws is not None:
            eff = len(N.slice_groups(K // 8, ksplit))
            assert N.planes_rest_is_nan(ws, eff, M, N.plane_layout(wts.widths)[0]), (t, "wrote behind the planes of the workspace")
        vals[mode] = N.dst_values(dsts, wts, M)
    assert all_same_bits(vals[1], vals[2]), (tag, M, "modes 1 and 2 differ")
    return vals


def check_128(lib, tag, qa, qb, refa, refb, K, M, M2, wts, ksplit, want_a, want_b):
    """cvc_linear_nn_planes2_fwd (reduce = 1) in mode 2: rows 0 .. M and 64 .. 64 + M2 vs fp64 and bit-equal to the 64-row split
    kernel's values want_a / want_b; rows nobody owns still NaN; two launches bit-equal"""
    t = f"{tag} 128-row M={M} M2={M2} ksplit={ksplit}"
    with N.split_mode(lib, 2):
        rc, dsts, _ = N.run_nn(lib, "planes2", qa, K, M, wts, ksplit, dyq2=qb, M2=M2, reduce=1)
        rc2, again, _ = N.run_nn(lib, "planes2", qa, K, M, wts, ksplit, dyq2=qb, M2=M2, reduce=1)
    assert (rc, rc2) == (0, 0), (t, rc, rc2)
    N.check_dsts(t + " group A", dsts, refa, M, wts, rows_nan=(M, 64))
    N.check_dsts(t + " group B", dsts, refb, M2, wts, row0=64, rows_nan=(64 + M2, None))
    assert all_same_bits(N.dst_values(dsts, wts, M), want_a), (t, "group A: not the 64-row split kernel's bits")
    assert all_same_bits(N.dst_values(dsts, wts, M2, row0=64), want_b), (t, "group B: not the 64-row split kernel's bits")
    assert all_same_bits(dsts, again), (t, "two launches of one case differ")
    return dsts


# ------------------------------------------------------------------ 1. the K loop: every branch of all three kernels
# Wave w of NW = 4 takes the 8-row groups w, w + 4, ... of the K / 8 groups: n_my = ceil((K / 8 - w) / 4).
#   K / 8 -> n_my of waves 0..3:  1 (1,0,0,0)   8 n + 6 (2n+2, 2n+2, 2n+1, 2n+1) for n = 0 .. 11: every n_my in 0 .. 24
# fp32 kernel, depth 3 over n_my: n_my < 3 one group at a time; from 3 the ring, a steady pass of 3 while j + 5 <= n_my, tail of 2 .. 4.
# split kernel, depth 4 over n2 = n_my >> 1: n2 < 4 simple; ring from 4, a pass of 4 while j + 7 <= n2, tail of 3 .. 6; n_my & 1: one
#   more group on the fp32 MFMA.  128-row kernel: depth 3 over n2, its tail waits on counted vmcnt(32 / 16 / 0).
# The sweep reaches, in each kernel, the simple loop at every length, the ring without a pass at every tail, one pass at every tail
# and two passes -- in the split kernels with both parities of n_my (tests/test_nn_gemm_cpu.py, against the source's constants).
# One segment of 132 columns: two slabs, the second with 4 valid columns (31 lanes re-read the last quad, one lane stores).
@pytest.mark.parametrize("G", N.SWEEP_GROUPS)
def test_k_loop_every_branch_of_all_three_kernels_vs_fp64(dev, lib, G):
    K = 8 * G
    ca, cb = N.nn_case(1000 + G, 64, K, 132), N.nn_case(2000 + G, 64, K, 132)
    wa = N.Weights(dev, ca["w"], (132,))
    assert wa.mats[0].shape == (K, 148) and wa.views[0].data_ptr() == wa.mats[0].data_ptr() + 32
    # the second group is an operand of its own against the FIRST group's weights (one stream of the weights)
    ref_a, ref_b = N.nn_ref(ca["dy"], ca["w"]), N.nn_ref(cb["dy"], ca["w"])
    for M in ROWS:
        M2 = second_rows(M)
        qa, qb = N.device_quad(lib, ca["dy"][:M].to(dev)), N.device_quad(lib, cb["dy"][:M2].to(dev))
        tag = f"k_loop K/8={G}"
        vals = fwd_in_every_mode(lib, tag, qa, ref_a[:M], K, M, wa)
        with N.split_mode(lib, 2):
            rc, dsts_b, _ = N.run_nn(lib, "fwd", qb, K, M2, wa)
        assert rc == 0
        N.check_dsts(f"{tag} mode=2 group B M={M2}", dsts_b, ref_b[:M2], M2, wa)
        check_128(lib, tag, qa, qb, ref_a[:M], ref_b[:M2], K, M, M2, wa, 1, vals[2], N.dst_values(dsts_b, wa, M2))
    assert all_nan(wa.mats[0][:, :8]) and all_nan(wa.mats[0][:, 140:]) and not bool(torch.isnan(wa.views[0]).any())


# ------------------------------------------------------------------ 2. K slices and planes
# Slice s of ksplit_eff = min(ksplit, K / 8) owns the groups [G s / ksplit_eff, G (s + 1) / ksplit_eff): (5, 5) one group a slice
# (waves 1 .. 3 idle), (11, 3) 3 + 4 + 4, (23, 4) 5 + 6 + 6 + 6, (47, 2) 23 + 24, (94, 3) 31 + 31 + 32, (3, 64) clamped to three
# slices of one group.  Widths (132, 36): ntot = 384, segment 1 starts at plane column 256; columns 132 .. 256 and 292 .. 384 are
# slab padding.
@pytest.mark.parametrize("G,ksplit", N.SLICE_CASES)
def test_k_slices_reduced_planes_and_128_row_planes_vs_fp64(dev, lib, G, ksplit):
    K, widths = 8 * G, N.SLICE_WIDTHS
    eff = min(ksplit, G)
    ntot, _ = N.plane_layout(widths)
    ca, cb = N.nn_case(3000 + G, 64, K, sum(widths)), N.nn_case(4000 + G, 64, K, sum(widths))
    wts = N.Weights(dev, ca["w"], widths)
    for M in (33, 64):
        M2 = second_rows(M)
        dya, dyb = ca["dy"][:M], cb["dy"][:M2]
        qa, qb = N.host_quad(dya).to(dev), N.host_quad(dyb).to(dev)
        ref_a, ref_b = N.nn_ref(dya, ca["w"]), N.nn_ref(dyb, ca["w"])
        srefs_a, srefs_b = N.slice_refs(dya, ca["w"], ksplit), N.slice_refs(dyb, ca["w"], ksplit)
        assert len(srefs_a) == eff
        tag = f"k_slices K/8={G} ksplit={ksplit}"
        # (a) the reduced form
        reduced = fwd_in_every_mode(lib, tag, qa, ref_a, K, M, wts, ksplit)
        planes_by_mode = {}
        for mode in MODES:
            t = f"{tag} mode={mode} M={M}"
            with N.split_mode(lib, mode):
                rc, dsts, ws = N.run_nn(lib, "planes", qa, K, M, wts, ksplit)
                rc1, dsts1, _ = N.run_nn(lib, "planes", qa, K, M, wts, 1, null_ws=True)
                rc2, dsts2, _ = N.run_nn(lib, "fwd", qa, K, M, wts, 1)
            assert (rc, rc1, rc2) == (0, 0, 0), (t, rc, rc1, rc2)
            # (b) the plane form
            planes, _ = N.check_planes(t, ws, srefs_a, M, wts)
            assert N.planes_rest_is_nan(ws, eff, M, ntot), (t, "wrote behind plane ksplit_eff - 1")
            assert N.dsts_untouched(dsts), (t, "the plane form wrote a segment's dst")
            # (c) the plane order of the sum
            assert all_same_bits(N.plane_sum(planes, wts, M), reduced[mode]), (t, "the reduced form is not the planes summed in plane order")
            # (e) one slice through the plane entry point, NULL workspace: straight into dst
            N.check_dsts(t + " planes entry, ksplit=1", dsts1, ref_a, M, wts)
            assert all_same_bits(dsts1, dsts2), (t, "ksplit = 1: the plane entry point and cvc_linear_nn_fwd differ")
            planes_by_mode[mode] = planes
        assert same_bits(planes_by_mode[1], planes_by_mode[2]), (tag, M, "modes 1 and 2 differ")
        # (d) the 128-row planes
        t = f"{tag} 128-row M={M} M2={M2}"
        with N.split_mode(lib, 2):
            rcb, _, ws_b = N.run_nn(lib, "planes", qb, K, M2, wts, ksplit)
            rcr, dsts_br, _ = N.run_nn(lib, "fwd", qb, K, M2, wts, ksplit)
            rc, dsts, ws = N.run_nn(lib, "planes2", qa, K, M, wts, ksplit, dyq2=qb, M2=M2, reduce=0)
        assert (rcb, rcr, rc) == (0, 0, 0), (t, rcb, rcr, rc)
        planes_b, _ = N.check_planes(t + " group B alone", ws_b, srefs_b, M2, wts)
        N.check_dsts(t + " group B alone, reduced", dsts_br, ref_b, M2, wts)
        p128, _ = N.check_planes(t + " group A", ws, srefs_a, M, wts, rows=128)
        N.check_planes(t + " group B", ws, srefs_b, M2, wts, rows=128, row0=64)
        assert same_bits(p128[:, :M], planes_by_mode[2]) and same_bits(p128[:, 64:64 + M2], planes_b), (t, "not the 64-row planes' bits")
        assert all_nan(p128[:, M:64]) and all_nan(p128[:, 64 + M2:]), (t, "rows nobody owns were written")
        assert N.planes_rest_is_nan(ws, eff, 128, ntot) and N.dsts_untouched(dsts), (t, "wrote behind the planes, or a segment's dst")
        check_128(lib, tag, qa, qb, ref_a, ref_b, K, M, M2, wts, ksplit, reduced[2], N.dst_values(dsts_br, wts, M2))


# ------------------------------------------------------------------ 3. segments and views
# NN_MAX_SEG = 6 segments of widths (4, 128, 132, 256, 36, 260) -- 1, 1, 2, 2, 1, 3 slabs: the segment search of a workgroup runs
# over all six slab0 values -- alternating between two [K, 816 + 16] weight matrices that hold NaN wherever no segment of their
# own lies.  K = 376: 47 groups, waves (12, 12, 12, 11) at ksplit = 1, slices of 15 + 16 + 16 at ksplit = 3.
@pytest.mark.parametrize("M", [1, 33, 64])
def test_six_segments_on_column_views_vs_fp64(dev, lib, M):
    K, widths = 376, N.SIX_WIDTHS
    M2 = second_rows(M)
    ca, cb = N.nn_case(5000 + M, M, K, sum(widths)), N.nn_case(6000 + M, M2, K, sum(widths))
    wts = N.Weights(dev, ca["w"], widths, nmat=2)
    assert wts.ld == 832 and all(v.stride(0) == 832 and v.data_ptr() % 16 == 0 for v in wts.views)
    assert [v.data_ptr() == wts.mats[s % 2].data_ptr() + 4 * (8 + c0) for s, (v, c0) in enumerate(zip(wts.views, wts.c0))] == [True] * 6
    frames = [torch.isnan(m).sum().item() for m in wts.mats]
    qa, qb = N.host_quad(ca["dy"]).to(dev), N.host_quad(cb["dy"]).to(dev)
    ref_a, ref_b = N.nn_ref(ca["dy"], ca["w"]), N.nn_ref(cb["dy"], ca["w"])
    for ksplit in (1, 3):
        tag = "six_segments"
        vals = fwd_in_every_mode(lib, tag, qa, ref_a, K, M, wts, ksplit)
        with N.split_mode(lib, 2):
            rc, dsts_b, _ = N.run_nn(lib, "fwd", qb, K, M2, wts, ksplit)
        assert rc == 0
        N.check_dsts(f"{tag} mode=2 group B M={M2} ksplit={ksplit}", dsts_b, ref_b, M2, wts)
        check_128(lib, tag, qa, qb, ref_a, ref_b, K, M, M2, wts, ksplit, vals[2], N.dst_values(dsts_b, wts, M2))
    assert frames == [torch.isnan(m).sum().item() for m in wts.mats]


def test_minimum_shape_one_group_one_row_one_quad_vs_fp64(dev, lib):
    """K = 8, M = 1, ncols = 4: one wave has one group (the fp32-MFMA step alone in the split kernels), 31 lanes re-read the quad"""
    ca, cb = N.nn_case(77, 1, 8, 4), N.nn_case(78, 1, 8, 4)
    wts = N.Weights(dev, ca["w"], (4,))
    qa, qb = N.host_quad(ca["dy"]).to(dev), N.host_quad(cb["dy"]).to(dev)
    ref_a, ref_b = N.nn_ref(ca["dy"], ca["w"]), N.nn_ref(cb["dy"], ca["w"])
    vals = fwd_in_every_mode(lib, "minimum", qa, ref_a, 8, 1, wts)
    assert all_same_bits(vals[0], vals[2])                  # one group: every mode multiplies it on the fp32 MFMA
    with N.split_mode(lib, 2):
        rc, dsts_b, _ = N.run_nn(lib, "fwd", qb, 8, 1, wts)
        rc3, dsts_c, ws = N.run_nn(lib, "fwd", qa, 8, 1, wts, 3)           # ksplit clamped to 1: straight into dst, workspace untouched
    assert (rc, rc3) == (0, 0)
    N.check_dsts("minimum group B", dsts_b, ref_b, 1, wts)
    assert all_same_bits(N.dst_values(dsts_c, wts, 1), vals[2]) and all_nan(ws)
    check_128(lib, "minimum", qa, qb, ref_a, ref_b, 8, 1, 1, wts, 1, vals[2], N.dst_values(dsts_b, wts, 1))


# ------------------------------------------------------------------ 4. cvc_pack_quad, exact
@pytest.mark.parametrize("K", [4, 8, 376])
def test_pack_quad_is_the_host_built_layout_bit_for_bit(dev, lib, K):
    """row-major [M, K] read through ldx = K + 8 out of a NaN-filled tensor -> [K/4][64][4], rows >= M exactly +0.0, the quad
    behind the last one untouched; a GEMM fed from it gives the bits of a GEMM fed from the host-built quad (K >= 8: the GEMM's
    smallest K)"""
    for M in (1, 33, 64):
        c = N.nn_case(8000 + K + M, M, K, 36)
        c["dy"][0, 0] = -0.0                                 # a sign the copy has to keep
        rc, xq = N.run_pack_quad(lib, dev, c["dy"])
        assert rc == 0
        want = N.host_quad(c["dy"]).to(dev)
        assert same_bits(xq[:K // 4], want), (K, M, "not the host-built quad layout")
        assert not bool(xq[:K // 4, M:].contiguous().view(torch.int32).any()), (K, M, "rows >= M are not +0.0")
        assert all_nan(xq[K // 4:]), (K, M, "wrote behind the last quad")
        if K >= 8:
            wts = N.Weights(dev, c["w"], (36,))
            for mode in MODES:
                with N.split_mode(lib, mode):
                    rc1, d1, _ = N.run_nn(lib, "fwd", xq[:K // 4], K, M, wts)
                    rc2, d2, _ = N.run_nn(lib, "fwd", want, K, M, wts)
                assert (rc1, rc2) == (0, 0)
                N.check_dsts(f"pack_quad K={K} M={M} mode={mode}", d1, N.nn_ref(c["dy"], c["w"]), M, wts)
                assert all_same_bits(d1, d2), (K, M, mode)


# ------------------------------------------------------------------ 5. fp32 grade of the split product
@pytest.mark.parametrize("M,K,Ncols", [(64, 752, 132), (17, 376, 96)])
def test_split_product_is_fp32_grade_with_the_odd_group_step(dev, lib, M, K, Ncols):
    """The criterion of test_split_product_gemm_is_fp32_grade (tests/test_gpu_parity.py) on its mixed-magnitude operands -- 1e-3,
    64 and 1e18 / 1e-18 stripes on the K index of both operands, signed zeros, -2^-100 -- measured against fp64: the rms error is at
    most 1e-6 of the reference's rms in every mode, and the rms and max error of modes 1 and 2 are at most 1.25 times mode 0's, on the
    64-row entry and on the 128-row form.  K / 8 = 94 gives waves (24, 24, 23, 23) groups, 47 gives (12, 12, 12, 11): the split
    kernels add an fp32-MFMA step to their bf16x3 products in some waves."""
    c = N.mixed_nn_case(M, K, Ncols)
    wts = N.Weights(dev, c["w"], (Ncols,))
    dyb = c["dy"].flip(0).contiguous()                       # the 128-row form's second group: the same rows in reverse order
    qa, qb = N.host_quad(c["dy"]).to(dev), N.host_quad(dyb).to(dev)
    ref = N.nn_ref(c["dy"], c["w"]).to(dev)
    ref_rms = ref.pow(2).mean().sqrt().item()

    def errors(got, want):
        e = (got.double() - want).abs()
        return e.pow(2).mean().sqrt().item(), e.max().item()
    err = {}
    for mode in MODES:
        with N.split_mode(lib, mode):
            rc, dsts, _ = N.run_nn(lib, "fwd", qa, K, M, wts)
            assert rc == 0
            assert all_nan(dsts[0][M:]) and all_nan(dsts[0][:, Ncols:])
            err[mode] = errors(dsts[0][:M, :Ncols], ref)
            if mode:
                rc, d128, _ = N.run_nn(lib, "planes2", qa, K, M, wts, dyq2=qb, M2=M, reduce=1)
                assert rc == 0
                assert all_nan(d128[0][M:64]) and all_nan(d128[0][64 + M:]) and all_nan(d128[0][:, Ncols:])
                assert same_bits(d128[0][:M, :Ncols], dsts[0][:M, :Ncols])
                err[mode, 128] = errors(torch.cat([d128[0][:M, :Ncols], d128[0][64:64 + M, :Ncols]]), torch.cat([ref, ref.flip(0)]))
    print(f"nn_gemm fp32_grade M={M} K={K}: reference rms = {ref_rms:.3e}, (rms, max) errors = {err}")
    for k, (rms, _) in err.items():
        assert rms <= 1e-6 * ref_rms, (k, rms, ref_rms)
    for k in (1, 2, (1, 128), (2, 128)):
        assert err[k][0] <= 1.25 * err[0][0] and err[k][1] <= 1.25 * err[0][1], (k, err)
