"""Cases, operands, fp64 references and comparisons of tests/test_gpu_lstm_seq_kernels.py (the LSTM frame encoder's kernels of
csrc/lstm_seq.hip, every entry point by name).  Nothing here needs a GPU: tests/test_lstm_seq_cases_cpu.py feeds the comparisons
stand-in "kernel results" (the reference rounded to fp32 passes, every mutation of it fails) and checks that the case lists reach
every kernel form the source has.

The reference is tests/lstm_ref.py (proven against nn.LSTM in tests/test_lstm_seq_cpu.py).  The recurrence is isolated from the
tile GEMM: gi = x W_ih^T is made here in fp64 and rounded to fp32; the backward's reference reads `gates` and `c` of the forward
reference ROUNDED to fp32, which is what the kernel is handed.  Weights are nn.LSTM's initial range scaled by 1.5, so the gates
leave their linear region.  Tolerances are the project's; every comparison is element-wise."""
import functools
import types

import numpy as np
import torch

import lstm_ref as R
from test_gpu_parity import GRAD_TOL, OP_TOL
from test_gpu_train_kernels import _gen, red_tol

INP = 16           # width of the x behind gi
GATES = ("i", "f", "g", "o")


def close(got, want, what, tol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    print("%s: max |err| %.3g (max |ref| %.3g)" % (what, float((got - want).abs().max()), float(want.abs().max())))
    np.testing.assert_allclose(got.numpy(), want.numpy(), err_msg=what, **tol)


# ------------------------------------------------------------------------------------------------ the forms of csrc/lstm_seq.hip
def bwd_ksplit(H):
    """csrc/lstm_seq.hip:292-298 (bwd_ksplit): K slices of the backward-data product dgates W_hh"""
    slabs = (H + 127) // 128
    ks = min(256 // slabs, 4 * H // 8 // 16)
    return max(ks, 1)


def bwd_ntot(H):
    """csrc/lstm_seq.hip:410, :423: the plane row length, H rounded up to 128"""
    return (H + 127) // 128 * 128


def bwd_work_floats(M, H, ndir):
    """csrc/lstm_seq.hip:408-412 (cvc_lstm_seq_bwd_work): per direction dc [M, H], the quad operand [4H/4][64][4], ksplit planes"""
    return ndir * (M * H + 4 * H * 64 + bwd_ksplit(H) * M * bwd_ntot(H))


def instantiation(H, M):
    """csrc/lstm_seq.hip:326-341 (persistent_impl) -> (MT, NC, NW) of the lstm_persistent_kernel that runs: 8 waves with K / 8 each
    when H % 256 == 0, else 4 waves with K / 4 each; MT = 32-clip tiles"""
    assert H % 128 == 0 and 128 <= H <= 1024 and 1 <= M <= 64
    w8 = H % 256 == 0
    return (1 if M <= 32 else 2), (H // 256 if w8 else H // 128), (8 if w8 else 4)


ALL_INSTANTIATIONS = {(mt, nc, nw) for mt in (1, 2) for nc, nw in [(1, 8), (2, 8), (3, 8), (4, 8), (1, 4), (3, 4), (5, 4), (7, 4)]}


def step_tile(M):
    """csrc/lstm_seq.hip:357-358 (steps_impl): lstm_step_kernel<1> up to 32 clips, <2> above"""
    return 1 if M <= 32 else 2


def kp(H):
    """csrc/lstm_seq.hip:311: K of the packed tiles, H rounded up to 32"""
    return (H + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ the case lists: (H, M, F, ndir)
# persistent forward: every instantiation (H = 128 .. 1024 at 32 and 33 clips), then the edges M = 1, M = 64, F = 1, one direction
A_CASES = ([(H, M, 3, 2) for H in range(128, 1025, 128) for M in (32, 33)] +
           [(128, 1, 3, 2), (1024, 64, 3, 2), (256, 33, 1, 2), (384, 32, 3, 1), (512, 64, 2, 1)])
# per-step forward: Kp > H at 8, 40, 72, 200; a single k chunk at 8; config 5's width; every H at both tiles
B_CASES = [(8, 1, 1, 1), (8, 33, 5, 2), (40, 32, 2, 2), (40, 64, 5, 1), (72, 33, 5, 2), (72, 1, 2, 1), (128, 64, 1, 2), (128, 32, 5, 1),
           (200, 64, 2, 2), (200, 32, 5, 1), (2048, 33, 2, 2), (2048, 32, 1, 1)]
# backward: every distinct bwd_ksplit (1, 1, 4, 6, 8, 32, 16), ntot > H at 8, 40, 200
E_WIDTHS = (8, 40, 128, 200, 256, 1024, 2048)
E_CASES = [(8, 1, 1, 1), (8, 33, 5, 2), (40, 64, 2, 2), (40, 33, 5, 1), (128, 33, 5, 2), (128, 1, 2, 1), (200, 64, 1, 2), (200, 33, 2, 1),
           (256, 64, 5, 2), (256, 33, 1, 1), (1024, 33, 2, 2), (1024, 64, 1, 1), (2048, 33, 2, 2), (2048, 1, 2, 1)]
# layouts: one shape per kernel template (both tiles of either forward form; the backward at a padded and an unpadded ntot)
D_PERSISTENT = [(128, 5, 3, 2), (256, 37, 3, 2)]
D_STEPS = [(40, 5, 3, 2), (72, 37, 3, 2)]
D_BWD = [(40, 5, 3, 2), (128, 37, 3, 2)]
LAYOUTS = [("tm", 4), ("tm", 8), ("bm", 0)]          # padded time-major (ld_m = width + pad, one clip row more); clip-major
# autograd: (B, F, inp, H, layers, bidir); 70 clips are two chunks (parameter gradients summed over chunks)
G_CASES = [(5, 4, 48, 128, 2, True), (33, 3, 40, 200, 1, True), (9, 5, 24, 40, 1, False), (70, 3, 32, 128, 2, True)]


def case_id(c):
    return "H%d-M%d-F%d-ndir%d" % c


def a_id(c):
    return "H%d-M%d-F%d-ndir%d-MT%d-NC%d-NW%d" % (c + instantiation(c[0], c[1]))


# ------------------------------------------------------------------------------------------------ operands and references
@functools.lru_cache(maxsize=None)
def weights(H):
    """W_hh [2, 4H, H], b_ih, b_hh [2, 4H] of two directions at nn.LSTM's initialisation scaled by 1.5"""
    g = _gen("lstm weights", H)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * (1.5 / H ** 0.5)
    return u(2, 4 * H, H), u(2, 4 * H), u(2, 4 * H)


def reference_backward(dy, gates, c, w_hh, reverse):
    """dG [M, F, 4H] of one direction from the saved tensors (fp64): lstm_ref.lstm_layer_backward(...)[4] with no input side"""
    M, F, H = c.shape
    none = torch.zeros(M, F, 1, dtype=torch.float64), torch.zeros(4 * H, 1, dtype=torch.float64)
    return R.lstm_layer_backward(dy, none[0], torch.zeros_like(c), gates.view(M, F, 4, H), c, none[1], w_hh, reverse)[4]


@functools.lru_cache(maxsize=None)
def ops(H, M, F, ndir):
    """One case's host operands and its fp64 reference (made once, shared, never written to): gi [M, F, ndir * 4H] fp32; y, gates
    (activated i, f, g, o: columns [ndir][4][H]) and c of the forward; dg of the backward from a random dy and the forward's
    gates / c ROUNDED to fp32 (what the kernel reads).  Random in time, so a direction walked the wrong way is another result."""
    g = _gen("lstm case", H, M, F, ndir)
    w_hh, b_ih, b_hh = [t[:ndir] for t in weights(H)]
    x = torch.randn(M, F, INP, generator=g)
    w_ih = (torch.rand(ndir * 4 * H, INP, generator=g) * 2 - 1) * (1.5 / INP ** 0.5) * 2
    gi = (x.double() @ w_ih.double().T).float()
    dy = torch.randn(M, F, ndir * H, generator=g)
    ys, gs, cs, dgs = [], [], [], []
    for d in range(ndir):
        wd = w_hh[d].double()
        y, gates, c = R.lstm_recurrence(gi[:, :, d * 4 * H:(d + 1) * 4 * H].double(), wd, b_ih[d].double(), b_hh[d].double(), d == 1)
        gates = gates.reshape(M, F, 4 * H)
        ys.append(y)
        gs.append(gates)
        cs.append(c)
        dgs.append(reference_backward(dy[:, :, d * H:(d + 1) * H].double(), gates.float().double(), c.float().double(), wd, d == 1))
    cat = lambda ts: torch.cat(ts, 2)
    return types.SimpleNamespace(H=H, M=M, F=F, ndir=ndir, w_hh=w_hh.contiguous(), b_ih=b_ih.contiguous(), b_hh=b_hh.contiguous(), gi=gi,
                                 dy=dy, y=cat(ys), gates=cat(gs), c=cat(cs), dg=cat(dgs))


# ------------------------------------------------------------------------------------------------ the comparisons
def check_forward_results(o, y, gates, c, tag):
    """y, the four activated gate planes and c of every direction, [M, F, .], element-wise against fp64 within OP_TOL"""
    H = o.H
    close(y, o.y, "%s y" % tag, OP_TOL)
    for d in range(o.ndir):
        for p, nm in enumerate(GATES):
            sl = slice(d * 4 * H + p * H, d * 4 * H + (p + 1) * H)
            close(gates[:, :, sl], o.gates[:, :, sl], "%s gate %s dir %d" % (tag, nm, d), OP_TOL)
        close(c[:, :, d * H:(d + 1) * H], o.c[:, :, d * H:(d + 1) * H], "%s c dir %d" % (tag, d), OP_TOL)


def check_dg(o, dg, tag):
    """dG [M, F, ndir * 4H] of every direction element-wise within GRAD_TOL; with F >= 2 the first and the last time step -- each
    the first processed step of one direction (no carried planes, c_prev absent in the other) -- once more on their own"""
    H = o.H
    for d in range(o.ndir):
        sl = slice(d * 4 * H, (d + 1) * 4 * H)
        close(dg[:, :, sl], o.dg[:, :, sl], "%s dG dir %d" % (tag, d), GRAD_TOL)
        if o.F >= 2:
            for t in (0, o.F - 1):
                close(dg[:, t, sl], o.dg[:, t, sl], "%s dG dir %d step %d" % (tag, d, t), GRAD_TOL)


def check_param_grads(got, want, rows, tag):
    """every parameter gradient (name -> tensor) element-wise: sums over `rows` = F * B rows, red_tol(rows)"""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in sorted(want):
        close(got[k], want[k], "%s d%s" % (tag, k), red_tol(rows))


def rel_norm(a, b):
    """the relative norm the gradients were checked by before (tests/test_gpu_lstm_seq.py: rel(...) < 1e-4)"""
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))
