"""The comparisons of tests/test_gpu_lstm_seq_kernels.py, proven on the CPU (no GPU here): fed the fp64 reference rounded to fp32 as
the "kernel result" they pass; fed a subtly wrong kernel's result they fail, at the smallest shapes of the case lists.  Two of the
mutations are shown to PASS the relative-norm check (< 1e-4) that was the only check of the LSTM's gradients before -- that is what
the element-wise comparisons are for.  Also: the case lists reach every kernel form of csrc/lstm_seq.hip (the forms restated in
tests/lstm_seq_cases.py from the cited lines of the source)."""
import os
import re

import pytest
import torch

import lstm_ref as R
import lstm_seq_cases as LC
from test_gpu_parity import GRAD_TOL
from test_gpu_train_kernels import red_tol

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cyclical-visual-captioning_amd", "csrc", "lstm_seq.hip")
FWD_CASE = (8, 33, 5, 2)            # the smallest per-step case with both directions, F >= 2 and a clip row 32
BWD_CASE = (8, 33, 5, 2)            # ... of the backward
# One row of dG is about 1 / sqrt(F * M) of the norm: scaled by 1 + 1e-3 it reads 1.04e-4 at 33 x 5 rows (step 0 is the forward
# direction's last processed step, its rows are larger than average) -- the norm check is blind to it from the next case up
BWD_ROWS_CASE = (256, 64, 5, 2)


def fails(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def as_kernel(t):
    """a correct kernel's result: the reference rounded to fp32"""
    return t.float()


# ---- the forward comparisons
def test_the_rounded_reference_passes_every_forward_check():
    for case in (FWD_CASE, (8, 1, 1, 1), (40, 32, 2, 2)):
        o = LC.ops(*case)
        LC.check_forward_results(o, as_kernel(o.y), as_kernel(o.gates), as_kernel(o.c), LC.case_id(case))


def test_swapped_f_and_o_gate_blocks_are_caught():
    o = LC.ops(*FWD_CASE)
    H = o.H
    gates = as_kernel(o.gates).clone()
    for d in range(o.ndir):
        f, og = slice(d * 4 * H + H, d * 4 * H + 2 * H), slice(d * 4 * H + 3 * H, d * 4 * H + 4 * H)
        gates[:, :, f], gates[:, :, og] = as_kernel(o.gates)[:, :, og], as_kernel(o.gates)[:, :, f]
    fails(LC.check_forward_results, o, as_kernel(o.y), gates, as_kernel(o.c), "f/o swapped")


@pytest.mark.parametrize("which", ["y", "gates", "c", "all"])
def test_reverse_direction_written_in_forward_time_order_is_caught(which):
    """the rows of direction 1 land at t = s (the step count), not at t = F - 1 - s"""
    o = LC.ops(*FWD_CASE)
    H = o.H
    res = dict(y=as_kernel(o.y).clone(), gates=as_kernel(o.gates).clone(), c=as_kernel(o.c).clone())
    for k, w in (("y", H), ("gates", 4 * H), ("c", H)):
        if which in (k, "all"):
            res[k][:, :, w:2 * w] = res[k][:, :, w:2 * w].flip(1)
    fails(LC.check_forward_results, o, res["y"], res["gates"], res["c"], "reverse rows in forward order")


# ---- the backward comparisons
def mutant_backward(dy, gates, c, w_hh, reverse, zero_c_prev=False, drop_dh_at=None):
    """lstm_ref.lstm_layer_backward's gate gradients written out again with two switches: c_prev taken as zero at every step (a
    kernel that never gets its c_prev pointer), the carried dh dropped at the step that works on time `drop_dh_at`"""
    M, F, H = c.shape
    g4 = gates.view(M, F, 4, H)
    dh_c, dc_c = dy.new_zeros(M, H), dy.new_zeros(M, H)
    dz = dy.new_zeros(M, F, 4 * H)
    for s in reversed(range(F)):
        t = F - 1 - s if reverse else s
        tp = t + 1 if reverse else t - 1
        i, f, g, og = g4[:, t, 0], g4[:, t, 1], g4[:, t, 2], g4[:, t, 3]
        c_prev = c[:, tp] if (0 <= tp < F and not zero_c_prev) else torch.zeros_like(c[:, t])
        tc = torch.tanh(c[:, t])
        dh = dy[:, t] + (0 if t == drop_dh_at else dh_c)
        dc = dh * og * (1 - tc * tc) + dc_c
        d = torch.cat((dc * g * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - g * g), dh * tc * og * (1 - og)), 1)
        dz[:, t] = d
        dh_c, dc_c = d @ w_hh, dc * f
    return dz


def mutant_dg(o, **kw):
    H = o.H
    return torch.cat([mutant_backward(o.dy[:, :, d * H:(d + 1) * H].double(), o.gates[:, :, d * 4 * H:(d + 1) * 4 * H].float().double(),
                                      o.c[:, :, d * H:(d + 1) * H].float().double(), o.w_hh[d].double(), d == 1, **kw)
                      for d in range(o.ndir)], 2)


def test_the_rounded_reference_passes_the_backward_check_and_the_mutant_without_switches_is_the_reference():
    for case in (BWD_CASE, (8, 1, 1, 1), (40, 64, 2, 2)):
        o = LC.ops(*case)
        LC.check_dg(o, as_kernel(o.dg), LC.case_id(case))
        assert torch.equal(mutant_dg(o), o.dg)


def test_c_prev_taken_as_zero_at_every_step_is_caught():
    o = LC.ops(*BWD_CASE)
    fails(LC.check_dg, o, as_kernel(mutant_dg(o, zero_c_prev=True)), "c_prev = 0")


@pytest.mark.parametrize("t", [1, 3])
def test_carried_dh_dropped_at_one_step_is_caught(t):
    o = LC.ops(*BWD_CASE)
    fails(LC.check_dg, o, as_kernel(mutant_dg(o, drop_dh_at=t)), "dh dropped at t = %d" % t)


def test_one_scaled_clip_row_of_dg_is_caught_where_the_norm_check_passed():
    """row 32 of dG [F * M, ndir * 4H] (step 0, the first clip of the second 32-row tile) times 1 + 1e-3"""
    o = LC.ops(*BWD_ROWS_CASE)
    assert BWD_ROWS_CASE in LC.E_CASES and o.M > 32
    dg = as_kernel(o.dg).clone()
    dg[32, 0] *= 1 + 1e-3                                        # [M, F, .]: clip 32, step 0 = row 0 * M + 32 of the kernel's dG
    H = o.H
    for d in range(o.ndir):
        sl = slice(d * 4 * H, (d + 1) * 4 * H)
        assert LC.rel_norm(dg[:, :, sl], o.dg[:, :, sl]) < 1e-4   # what tests/test_gpu_lstm_seq.py asserts of dG: passes
    fails(LC.check_dg, o, dg, "row 32 scaled")


def test_one_bias_gradient_element_off_is_caught_where_the_norm_check_passed():
    """one element of db_ih off by 10 atol + 10 rtol |ref|, at the smallest autograd case"""
    B, F, inp, H, layers, bidir = LC.G_CASES[0]
    lstm = R.make_lstm(inp, H, layers, bidir, 11, scale=1.5)
    g = LC._gen("lstm autograd", B, F, inp, H, layers, bidir)
    x, probe = torch.randn(B, F, inp, generator=g), torch.randn(B, F, 2 * H, generator=g)
    params = {k: v.detach().clone() for k, v in lstm.named_parameters()}
    _, saved = R.lstm_forward(x, params, layers, bidir)
    _, want = R.lstm_backward(probe, saved, params, layers, bidir)
    got = {k: as_kernel(v).clone() for k, v in want.items()}
    LC.check_param_grads(got, want, F * B, "rounded reference")
    tol = red_tol(F * B)
    k = "bias_ih_l0"
    j = int(want[k].abs().argmin())                              # (where the relative part of the allowance is smallest)
    got[k][j] += 10 * tol["atol"] + 10 * tol["rtol"] * float(want[k][j].abs())
    assert LC.rel_norm(got[k], want[k]) < 1e-4                   # the check of tests/test_gpu_lstm_seq.py: passes
    fails(LC.check_param_grads, got, want, F * B, "one db element off")


# ---- the case lists against the source
def test_the_restated_forms_are_the_sources():
    src = open(SRC).read()
    body = src[src.index("int bwd_ksplit(int H)"):src.index("bool aligned16")]
    assert "(H + 127) / 128" in body and "256 / slabs" in body and "4 * H / 8 / 16" in body and "ks < 1 ? 1 : ks" in body
    assert [LC.bwd_ksplit(H) for H in LC.E_WIDTHS] == [1, 1, 4, 6, 8, 32, 16]
    assert [LC.bwd_ntot(H) > H for H in LC.E_WIDTHS] == [True, True, False, True, False, False, False]
    impl = src[src.index("int persistent_impl"):src.index("int steps_impl")]
    assert "(H % 256) == 0" in impl and "w8 ? H / 256 : H / 128" in impl and "if (a.M <= 32) { CVC_LSTM_NC(1) }" in impl
    launched = {(int(nc), int(nw)) for nc, nw in re.findall(r"CVC_LSTM_P\(MT_, (\d), (\d)\)", impl)}
    assert "CVC_LSTM_NC(1)" in impl and "CVC_LSTM_NC(2)" in impl
    assert {(mt, nc, nw) for mt in (1, 2) for nc, nw in launched} == LC.ALL_INSTANTIATIONS and len(LC.ALL_INSTANTIATIONS) == 16
    steps = src[src.index("int steps_impl"):src.index("}  // namespace")]
    assert "if (a.M <= 32) hipLaunchKernelGGL(lstm_step_kernel<1>" in steps and "else hipLaunchKernelGGL(lstm_step_kernel<2>" in steps
    assert "const int Kp = (H + 31) / 32 * 32;" in src
    assert "ndir * ((long long)M * H + 4LL * H * 64 + (long long)bwd_ksplit(H) * M * ntot)" in src


def test_the_case_lists_reach_every_form():
    assert {LC.instantiation(H, M) for H, M, _, _ in LC.A_CASES} == LC.ALL_INSTANTIATIONS
    for axis, want in ((1, {1, 32, 33, 64}), (2, {1, 2, 3}), (3, {1, 2})):
        assert {c[axis] for c in LC.A_CASES} >= want, axis
    # per-step forward: every value of every axis, both tiles at every width, one direction at a padded K, F <= 3 at 2048
    for axis, want in ((0, {8, 40, 72, 128, 200, 2048}), (1, {1, 32, 33, 64}), (2, {1, 2, 5}), (3, {1, 2})):
        assert {c[axis] for c in LC.B_CASES} == want, axis
    for H in {c[0] for c in LC.B_CASES}:
        assert {LC.step_tile(M) for h, M, _, _ in LC.B_CASES if h == H} == {1, 2}, H
    assert any(nd == 1 and LC.kp(H) > H for H, _, _, nd in LC.B_CASES)
    assert any(LC.kp(H) == 32 for H, _, _, _ in LC.B_CASES)                         # a single k chunk
    assert all(F <= 3 for H, _, F, _ in LC.B_CASES if H == 2048)
    # backward: every distinct split count, padded and unpadded planes, F = 1 (null c_prev, no planes) in either direction count
    for axis, want in ((0, set(LC.E_WIDTHS)), (1, {1, 33, 64}), (2, {1, 2, 5}), (3, {1, 2})):
        assert {c[axis] for c in LC.E_CASES} == want, axis
    all_ks = {LC.bwd_ksplit(H) for H in range(8, 2049, 8)}
    assert {LC.bwd_ksplit(H) for H in LC.E_WIDTHS} == {1, 4, 6, 8, 16, 32} <= all_ks
    assert all(F <= 3 for H, _, F, _ in LC.E_CASES if H >= 1024)
    assert {nd for _, _, F, nd in LC.E_CASES if F == 1} == {1, 2}
    # layouts: both tiles of either forward form
    for cases in (LC.D_PERSISTENT, LC.D_STEPS):
        assert {LC.step_tile(M) for _, M, _, _ in cases} == {1, 2}
    assert {LC.bwd_ntot(H) > H for H, _, _, _ in LC.D_BWD} == {True, False}
    # autograd: two chunks of clips, one direction, a width the persistent form refuses
    assert any(B > 64 for B, *_ in LC.G_CASES) and any(not c[5] for c in LC.G_CASES) and any(c[3] % 128 for c in LC.G_CASES)
