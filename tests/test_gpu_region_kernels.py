"""The small kernels around the region features and the grounding losses on the GPU, every C entry point called directly (hip.lib(),
hip._stream()), element-wise against the fp64 references and the bounds of tests/region_ref.py (proven against torch on the CPU in
tests/test_region_ref_cpu.py, which also shows that the bounds notice a wrong kernel):
    csrc/encoder_ops.hip   cvc_class_softmax_fwd, cvc_layernorm_cat_fwd, cvc_frame_embed_fwd (+ the wrapper cvc.encoder_ops.frame_embed)
    csrc/label_glue.hip    cvc_attn_nll_fwd, cvc_attn_nll_bwd
    csrc/attn_bwd.hip      cvc_grounder_fwd, cvc_grounder_bwd
    csrc/vocab.hip         cvc_embed_relu_fwd

Every operand is seeded here, never a GEMM's output (the wrapper test apart, which carries the GEMM's share u K sum |x| |w| per
element).  Every output lives in an arena with 64 sentinel floats on both sides, and the sentinels must survive; padding that an
argument declares unread (columns C .. ld - 1, the neighbours of a column view, the logits of padded regions, the tail of a
strided row) is NaN.  Every comparison prints its max |err| / (K x bound) (run with -s); the last test prints the worst per entry
point.

Measured on an MI355X, per entry point (K = 4; 1 = at the bound): the kernel's worst |err| / (K x bound) over every comparison of
this file; next to it the float32 restatement's own worst ratio over the tables, from the CPU (tests/test_region_ref_cpu.py: its
ratio WITHOUT K, and that over K); then the nearest wrong restatement, as its farthest case's |err| / (K x bound).
    cvc_class_softmax_fwd    0.188     restatement 0.750 (0.188)    bias dropped from class 64 on: 6.4e8 (the maximum or the sum of
                                                                    the first lane trip only, padding ignored: NaN or inf)
    cvc_layernorm_cat_fwd    0.0914    restatement 0.366 (0.091)    unbiased variance: 1.2e3 (eps outside the root 2.2e4, a shared
                                                                    mean 5.4e5, the first trip only 5.7e5)
    cvc_frame_embed_fwd      0.228     restatement 0.911 (0.228)    outer ReLU dropped: 4.2e6 (inner 5.6e8, scale from c - c0 2.3e9)
    cvc_attn_nll_fwd         0.0888    restatement 0.363 (0.091)    first trip only: 4.8e5 (lse without the maximum 2.2e6, the
                                                                    count per row 1.1e7)
    cvc_attn_nll_bwd         0.156     restatement 0.624 (0.156)    first trip only: 1.4e6 (count ignored 1.5e9, nt = 1: inf)
    cvc_grounder_fwd         0.0347    restatement 0.180 (0.045)    second 256-column chunk dropped: 1.2e4 (bias dropped 2.1e5, the
                                                                    last lane's columns 6.7e5, mask ignored: inf)
    cvc_grounder_bwd         0.237     restatement 0.948 (0.237)    fourth wave's rows dropped: 1.4e6 (the q >= 4 floor(nq / 4) tail
                                                                    4.2e6, d read with swapped strides 3.9e10)
    cvc_embed_relu_fwd       bitwise   (exact by construction; every wrong form differs in bits)
i.e. five of the seven kernels land on the restatement's own ratio to three digits (they ARE that arithmetic, FMAs included or
not), the two others within it (the dot product runs as FMAs: fewer roundings; the device's expf and logf are closer than the 2 u
they are allowed).  The fold of cvc.encoder_ops.frame_embed's scale and shift is within its three roundings of fp64.  The whole file
(126 tests) takes 2.6 s, most of it the first test's library load and the wrapper test's two GEMMs.

No defect was found: nothing in csrc/encoder_ops.hip, csrc/label_glue.hip, csrc/attn_bwd.hip's grounder or csrc/vocab.hip's
embedding, nor in the wrapper, was changed, and no bound had to be corrected after the first run on the device.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import region_ref as RR
from region_ref import BAND, K, SENTINEL, U

pytestmark = pytest.mark.gpu

F = np.float32
WORST = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    from cvc import hip
    return hip.lib()


def stream():
    from cvc import hip
    return hip._stream()


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def up(dev, a, dtype=None):
    """a host array on the device (bool -> uint8)"""
    a = np.ascontiguousarray(a)
    if a.dtype == bool:
        a = a.astype(np.uint8)
    return torch.from_numpy(a if dtype is None else a.astype(dtype)).to(dev)


class Arena:
    """n floats of output between two bands of 64 sentinels; the n floats start as sentinels too (what a kernel leaves unwritten,
    a declared gap for instance, must still hold them)"""

    def __init__(self, dev, n, fill=SENTINEL):
        self.n = n
        self.t = torch.full((n + 2 * BAND,), fill, dtype=torch.float32, device=dev)
        self.t[:BAND] = SENTINEL
        self.t[BAND + n:] = SENTINEL
        self.ptr = self.t.data_ptr() + 4 * BAND
        assert self.ptr % 16 == 0

    def host(self, what="arena"):
        """the n floats, after checking both bands"""
        torch.cuda.synchronize()
        a = self.t.cpu().numpy()
        assert (a[:BAND] == SENTINEL).all() and (a[BAND + self.n:] == SENTINEL).all(), "%s: a sentinel band was written" % what
        return a[BAND:BAND + self.n].copy()


def check(entry, what, got, want, bound):
    """got inside K x bound of want, element by element; prints and records the ratio |err| / (K x bound)"""
    r, err = RR.ratio(got, want, K * np.asarray(bound, dtype=np.float64))
    print("%s %s: max |err| / (K x bound) = %.3g, max |err| = %.3g" % (entry, what, r, err))
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    assert r <= 1.0, "%s %s leaves its bound: worst |err| / (K x bound) = %.4g" % (entry, what, r)
    return r


# ================================================================================================ cvc_class_softmax_fwd
def run_softmax(L, dev, x, bias, pad, B, N, C, ld, rows=True):
    """-> (return code, out [B, C, N], out_rows [B N, C] or None)"""
    xd = up(dev, x)
    bd = None if bias is None else up(dev, bias)
    pd = None if pad is None else up(dev, pad)
    out, out_rows = Arena(dev, B * C * N), Arena(dev, B * N * C) if rows else None
    rc = L.cvc_class_softmax_fwd(xd.data_ptr(), ld, None if bd is None else bd.data_ptr(), None if pd is None else pd.data_ptr(), B, N, C,
                                 out.ptr, out_rows.ptr if rows else None, stream())
    return rc, out.host("out").reshape(B, C, N), out_rows.host("out_rows").reshape(B * N, C) if rows else None


@pytest.mark.parametrize("case", RR.SOFTMAX_CASES, ids=str)
def test_class_softmax_elementwise_against_fp64(dev, L, case):
    """out within the bound; out_rows bitwise its transpose; a padded region bitwise float32(1) / float32(C) in every class; a -inf
    logit exactly 0 (its bound is 0).  The NaN of the unread columns and of the padded regions' logits reaches no output."""
    B, N, Cn, ld = case[:4]
    x, bias, pad = RR.softmax_values(case)
    want, bound = RR.softmax_fp64(x, bias, pad, Cn)
    rc, out, out_rows = run_softmax(L, dev, x, bias, pad, B, N, Cn, ld, case.rows)
    assert rc == 0
    got = out.transpose(0, 2, 1).reshape(B * N, Cn)
    check("cvc_class_softmax_fwd", str(tuple(case)), got, want, bound)
    if case.rows:
        assert same_bits(out_rows, got)
    if pad is not None and pad.any():
        assert (bits(got[pad]) == bits(F(1) / F(Cn))).all()
    assert (got[x[:, :Cn] == -np.inf] == 0).all()


@pytest.mark.parametrize("shape", [(2, 17, 65, 72), (1, 5, 1023, 1023)], ids=str)
def test_class_softmax_of_a_row_shifted_by_1e4(dev, L, shape):
    """logits that are multiples of 2^-8 (x + 1e4 is exact in float32), no bias: the shifted rows have the same probabilities, inside
    the bound of the shifted row (the rounding of x - max only: a maximum that was not subtracted overflows, one subtracted late
    loses 1e4 u)"""
    B, N, Cn, ld = shape
    rng = RR.rng_of("shift", shape)
    x = np.full((B * N, ld), np.nan, dtype=F)
    x[:, :Cn] = np.round(rng.standard_normal((B * N, Cn)) * 3.0 * 256) / 256
    shifted = (x + F(1e4)).astype(F)
    assert np.array_equal(shifted[:, :Cn].astype(np.float64), x[:, :Cn].astype(np.float64) + 1e4)
    want, _b = RR.softmax_fp64(x, None, None, Cn)
    _w, bound = RR.softmax_fp64(shifted, None, None, Cn)
    rc0, out0, _r = run_softmax(L, dev, x, None, None, B, N, Cn, ld, False)
    rc1, out1, _r = run_softmax(L, dev, shifted, None, None, B, N, Cn, ld, False)
    assert rc0 == 0 and rc1 == 0
    check("cvc_class_softmax_fwd", "%s shifted by 1e4" % (shape,), out1.transpose(0, 2, 1).reshape(B * N, Cn), want, bound)
    check("cvc_class_softmax_fwd", "%s unshifted" % (shape,), out0.transpose(0, 2, 1).reshape(B * N, Cn), want, bound)


def test_class_softmax_refuses_1024_classes(dev, L):
    """16 rows of 1025 floats do not fit the 64 KB of LDS: CVC_E_TOOBIG, and the outputs keep their bits"""
    x = np.zeros((2, 1024), dtype=F)
    rc, out, out_rows = run_softmax(L, dev, x, None, None, 1, 2, 1024, 1024, True)
    assert rc == RR.E_TOOBIG
    assert (out == SENTINEL).all() and (out_rows == SENTINEL).all()
    rc, out, out_rows = run_softmax(L, dev, x[:, :1023], None, None, 1, 2, 1023, 1023, True)
    assert rc == 0 and (bits(out) == bits(F(1) / F(1023))).all() and (bits(out_rows) == bits(F(1) / F(1023))).all()


# ================================================================================================ cvc_layernorm_cat_fwd
GAP = 5                                 # unread columns between the segments' column views; sentinel columns behind every output row


def run_layernorm(L, dev, xs, eps, nseg=None, rows=None, widths=None, ldx=None, ld_out=None):
    """the segments as column views of ONE wide NaN-filled matrix (ldx > width), the output with GAP sentinel columns behind every
    row (ld_out > total) -> (return code, out [rows, total], the whole output arena as [rows, ld_out])"""
    n_rows = xs[0].shape[0]
    ws = [x.shape[1] for x in xs]
    wide = sum(ws) + GAP * (len(ws) + 1)
    host = np.full((n_rows, wide), np.nan, dtype=F)
    offs, pos = [], GAP
    for x in xs:
        host[:, pos:pos + x.shape[1]] = x
        offs.append(pos)
        pos += x.shape[1] + GAP
    xd = up(dev, host)
    total = sum(ws)
    ldo = total + GAP
    out = Arena(dev, n_rows * ldo)
    n = len(xs)
    ptrs = (C.c_void_p * 3)(*([xd.data_ptr() + 4 * o for o in offs] + [None] * (3 - n)))
    lds = (C.c_longlong * 3)(*((list(ldx) if ldx is not None else [wide] * n) + [0] * (3 - n)))
    wid = (C.c_int * 3)(*((list(widths) if widths is not None else ws) + [0] * (3 - n)))
    rc = L.cvc_layernorm_cat_fwd(ptrs, lds, wid, n if nseg is None else nseg, n_rows if rows is None else rows, float(eps), out.ptr,
                                 ldo if ld_out is None else ld_out, stream())
    a = out.host("layernorm out").reshape(n_rows, ldo)
    return rc, a[:, :total], a


@pytest.mark.parametrize("case", RR.LN_CASES, ids=str)
def test_layernorm_cat_elementwise_against_fp64(dev, L, case):
    xs = RR.ln_values(case)
    want, bound = RR.ln_fp64(xs, case.eps)
    rc, got, whole = run_layernorm(L, dev, xs, case.eps)
    assert rc == 0
    check("cvc_layernorm_cat_fwd", str(tuple(case)), got, want, bound)
    assert (whole[:, want.shape[1]:] == SENTINEL).all(), "the gap columns of the output were written"


@pytest.mark.parametrize("widths", RR.LN_WIDTHS, ids=str)
def test_layernorm_cat_of_a_constant_row_is_bitwise_zero(dev, L, widths):
    """every partial sum of d copies of 0.375, -3 or 80 is exact, so is the mean, and (x - mean) rstd is +0; a width of 1 is its own
    mean whatever its value"""
    rng = RR.rng_of("const", widths)
    xs = [np.full((3, d), (0.375, -3.0, 80.0)[s], dtype=F) if d > 1 else rng.standard_normal((3, 1)).astype(F) for s, d in enumerate(widths)]
    for eps in RR.LN_EPS:
        rc, got, _whole = run_layernorm(L, dev, xs, eps)
        assert rc == 0 and not bits(got).any(), (widths, eps)


def test_layernorm_cat_refusals_leave_the_output_untouched(dev, L):
    xs = [np.ones((2, 7), dtype=F), np.ones((2, 4), dtype=F)]
    wide = 11 + 3 * GAP
    for over in (dict(nseg=0), dict(nseg=4), dict(widths=[7, 0]), dict(widths=[0, 4]), dict(ldx=[6, wide]), dict(ldx=[wide, 3]),
                 dict(ld_out=10), dict(rows=0)):
        rc, _got, whole = run_layernorm(L, dev, xs, 1e-5, **over)
        assert rc == RR.E_BADARG and (whole == SENTINEL).all(), over
    rc, got, _whole = run_layernorm(L, dev, xs, 1e-5)
    assert rc == 0 and not bits(got).any()


# ================================================================================================ cvc_frame_embed_fwd
@pytest.mark.parametrize("case", RR.FE_CASES, ids=str)
def test_frame_embed_elementwise_against_fp64(dev, L, case):
    """within the ABSOLUTE bound u (3 |t scale| + |shift|); where the value before the last ReLU is below -K x bound the output
    compares equal to 0 (the outer ReLU), and a channel of scale 0 gives max(shift, 0) exactly"""
    rows, c0, c1 = case
    y0, b0, y1, b1, scale, shift = v = RR.fe_values(case)
    want, z, bound = RR.fe_fp64(*v)
    d = [up(dev, a) for a in v]
    out = Arena(dev, rows * (c0 + c1))
    rc = L.cvc_frame_embed_fwd(d[0].data_ptr(), d[1].data_ptr(), c0, d[2].data_ptr(), d[3].data_ptr(), c1, d[4].data_ptr(), d[5].data_ptr(), rows,
                               out.ptr, stream())
    assert rc == 0
    got = out.host("frame_embed out").reshape(rows, c0 + c1)
    check("cvc_frame_embed_fwd", str(case), got, want, bound)
    neg = z < -K * bound
    assert neg.any() and (got[neg] == 0).all()
    assert (got >= 0).all()
    zero = scale == 0
    assert same_bits(got[:, zero], np.broadcast_to(np.maximum(shift[zero], F(0)), got[:, zero].shape))
    inner = np.concatenate([y0 + b0, y1 + b1], axis=1) < 0                      # the inner ReLU alone decides these: exactly max(shift, 0)
    assert same_bits(got[inner], np.broadcast_to(np.maximum(shift, F(0)), got.shape)[inner])


def test_frame_embed_wrapper_against_the_fp64_modules(dev):
    """cvc.encoder_ops.frame_embed on a stub encoder (two Linear, an eval-mode BatchNorm1d with negative and zero gamma channels and
    one running_var of 1e-6) against the same modules in float64.  The tolerance is K x the sum, per element, of
        the kernel's bound                                   u (3 |t scale| + |shift|)
        the two products' share, through the ReLU and scale  u K_dim sum |x| |w| |scale|
        the float32 fold of scale (3 roundings) and shift    3 u |scale| t + u (3 |mean scale| + |mean scale| + |shift|)
    and the cached fold itself is compared against fp64 within those three roundings"""
    from cvc import encoder_ops
    rng = RR.rng_of("fe-wrapper")
    rows, k0, k1, c0, c1 = 9, 24, 20, 8, 12
    l0, l1, bn = torch.nn.Linear(k0, c0), torch.nn.Linear(k1, c1), torch.nn.BatchNorm1d(c0 + c1)
    with torch.no_grad():
        for lin in (l0, l1):
            lin.weight.copy_(torch.from_numpy(rng.standard_normal(tuple(lin.weight.shape)).astype(F) * 0.3))
            lin.bias.copy_(torch.from_numpy(rng.standard_normal(lin.bias.shape[0]).astype(F) * 0.5))
        gamma = rng.standard_normal(c0 + c1).astype(F)
        gamma[1::4] = -np.abs(gamma[1::4])
        gamma[2] = 0.0
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(rng.standard_normal(c0 + c1).astype(F)))
        bn.running_mean.copy_(torch.from_numpy(rng.standard_normal(c0 + c1).astype(F) * 0.3))
        var = rng.uniform(0.2, 3.0, c0 + c1).astype(F)
        var[5] = 1e-6
        bn.running_var.copy_(torch.from_numpy(var))
    bn.eval()
    rgb, motion = rng.standard_normal((rows, k0)).astype(F), rng.standard_normal((rows, k1)).astype(F)
    # float64 twins, before the modules move
    import copy
    m0, m1, mbn = (copy.deepcopy(m).double() for m in (l0, l1, bn))
    with torch.no_grad():
        x0, x1 = torch.from_numpy(rgb).double(), torch.from_numpy(motion).double()
        t = torch.cat([torch.relu(m0(x0)), torch.relu(m1(x1))], dim=1)
        want = torch.relu(mbn(t)).numpy()
        scale64 = (mbn.weight / torch.sqrt(mbn.running_var + mbn.eps)).numpy()
        ms64 = (mbn.running_mean.numpy() * scale64)
        shift64 = mbn.bias.numpy() - ms64
        gemm = np.concatenate([(x0.abs() @ m0.weight.abs().T).numpy() * k0, (x1.abs() @ m1.weight.abs().T).numpy() * k1], axis=1) * U
        t = t.numpy()
    bound = (U * (3 * np.abs(t * scale64) + np.abs(shift64)) + gemm * np.abs(scale64) + 3 * U * np.abs(scale64) * t
             + U * (4 * np.abs(ms64) + np.abs(shift64)))
    enc = types.SimpleNamespace(att_embed=[[l0.to(dev)], [l1.to(dev)]], att_embed_aux=[bn.to(dev)])
    with torch.no_grad():
        got = encoder_ops.frame_embed(enc, torch.from_numpy(rgb).to(dev), torch.from_numpy(motion).to(dev))
    torch.cuda.synchronize()
    check("cvc_frame_embed_fwd", "wrapper", got.cpu().numpy(), want, bound)
    scale, shift = (a.cpu().numpy() for a in enc._cvc_bn_fold[1])
    assert scale[2] == 0 and (scale[1::4] < 0).all()
    assert (np.abs(scale - scale64) <= 3 * U * np.abs(scale64)).all(), np.abs(scale - scale64).max()
    assert (np.abs(shift - shift64) <= U * (4 * np.abs(ms64) + np.abs(shift64))).all(), np.abs(shift - shift64).max()
    assert (want == 0).any() and (want > 0).any()


# ================================================================================================ cvc_attn_nll_fwd / cvc_attn_nll_bwd
NLL_G = (0.7, -1.3)
TAIL = 3                                # NaN floats behind every row of x1 (stride_t = N + TAIL)


class NllRig:
    """x0 as [T, B, N] storage passed with swapped strides; x1 (two=True) as [B, T, N + TAIL] with NaN tails, or null"""

    def __init__(self, L, dev, case, x, tg, two):
        self.L, self.dev, self.case, self.two = L, dev, case, two
        B, T, N = case
        self.rows = B * T
        self.x0 = up(dev, x[0].transpose(1, 0, 2))
        self.a0 = (self.x0.data_ptr(), N, B * N)
        if two:
            host = np.full((B, T, N + TAIL), np.nan, dtype=F)
            host[:, :, :N] = x[1]
            self.x1 = up(dev, host)
            self.a1 = (self.x1.data_ptr(), T * (N + TAIL), N + TAIL)
        else:
            self.a1 = (None, 0, 0)
        self.tg = up(dev, tg)
        self.ws = Arena(dev, 5 * self.rows + 1)
        self.loss = Arena(dev, 2 if two else 1)

    def fwd(self):
        B, T, N = self.case
        rc = self.L.cvc_attn_nll_fwd(*self.a0, *self.a1, self.tg.data_ptr(), B, T, N, self.ws.ptr, self.loss.ptr, stream())
        assert rc == 0
        ws, r = self.ws.host("nll workspace"), self.rows
        return self.loss.host("nll loss"), ws[0:2 * r].reshape(2, r), ws[2 * r:4 * r].reshape(2, r), ws[4 * r:5 * r], ws[5 * r]

    def bwd(self, g0, g1, want0, want1):
        """-> (d_x0, d_x1), each [rows, N] or None"""
        B, T, N = self.case
        gd = [None if g is None else up(dev=self.dev, a=np.array([g], dtype=F)) for g in (g0, g1)]
        d = [Arena(self.dev, self.rows * N) if w else None for w in (want0, want1)]
        rc = self.L.cvc_attn_nll_bwd(*self.a0, *self.a1, self.tg.data_ptr(), B, T, N, self.ws.ptr, *[None if g is None else g.data_ptr() for g in gd],
                                     *[None if a is None else a.ptr for a in d], stream())
        assert rc == 0
        return [None if a is None else a.host("nll gradient").reshape(self.rows, N) for a in d]


@pytest.mark.parametrize("two,low", [(True, True), (False, True), (True, False)], ids=["two-tensors", "x1-null", "no-label-on-a-masked-slot"])
@pytest.mark.parametrize("case", RR.NLL_CASES, ids=str)
def test_attn_nll_forward_and_backward_elementwise_against_fp64(dev, L, case, two, low):
    """forward: both losses, row_lse and row_part inside the bounds of their summation structure, row_cnt and the count exact.
    backward: d_x0-only, d_x1-only and both give the same bits per tensor, element-wise inside the bound; a null g gives zeros.
    low: one target lies on a -1e8 slot (the issue's case; the loss is 1e8 / count there, and so is its bound's scale); without it
    the same loss is held to the bound of ordinary scores"""
    x, tg = RR.nll_values(case, low)
    nx = 2 if two else 1
    ref = RR.nll_fp64(x[:nx], tg)
    rig = NllRig(L, dev, case, x, tg, two)
    loss, part, lse, cnt, count = rig.fwd()
    e = "cvc_attn_nll_fwd"
    check(e, "%s loss" % (case,), loss, ref.loss, ref.e_loss)
    check(e, "%s row_lse" % (case,), lse[:nx], ref.lse, ref.e_lse)
    check(e, "%s row_part" % (case,), part[:nx], ref.part, ref.e_part)
    assert np.array_equal(cnt, ref.cnt) and count == ref.count
    if not two:
        assert (part[1] == SENTINEL).all() and (lse[1] == SENTINEL).all()
    # backward
    want, bound = RR.nll_bwd_fp64(x[:nx], tg, NLL_G[:nx], ref)
    e = "cvc_attn_nll_bwd"
    d0, _n = rig.bwd(NLL_G[0], NLL_G[1] if two else None, True, False)
    check(e, "%s d_x0" % (case,), d0, want[0], bound[0])
    if two:
        _n, d1 = rig.bwd(NLL_G[0], NLL_G[1], False, True)
        check(e, "%s d_x1" % (case,), d1, want[1], bound[1])
        b0, b1 = rig.bwd(NLL_G[0], NLL_G[1], True, True)
        assert same_bits(b0, d0) and same_bits(b1, d1)
        z0, z1 = rig.bwd(None, NLL_G[1], True, True)
        assert (z0 == 0).all() and same_bits(z1, d1)
        z0, z1 = rig.bwd(NLL_G[0], None, True, True)
        assert same_bits(z0, d0) and (z1 == 0).all()
    else:
        (z0, _n) = rig.bwd(None, None, True, False)
        assert (z0 == 0).all()


@pytest.mark.parametrize("case", [(2, 3, 7), (2, 3, 257)], ids=str)
def test_attn_nll_without_a_target(dev, L, case):
    """the losses are exactly 0, the count exactly 1 (clamped), the gradient all zeros"""
    x, tg = RR.nll_values(case)
    rig = NllRig(L, dev, case, x, np.zeros_like(tg), True)
    loss, part, _lse, cnt, count = rig.fwd()
    assert not bits(np.abs(loss)).any() and not part.any() and not cnt.any() and count == 1
    d0, d1 = rig.bwd(NLL_G[0], NLL_G[1], True, True)
    assert (d0 == 0).all() and (d1 == 0).all()


# ================================================================================================ cvc_grounder_fwd / cvc_grounder_bwd
def run_grounder_fwd(L, dev, xt, feats, bias, mask):
    B, T, G = xt.shape
    N = feats.shape[1]
    xd, fd = up(dev, xt), up(dev, feats)
    bd = None if bias is None else up(dev, bias)
    md = None if mask is None else up(dev, mask)
    out = Arena(dev, B * T * N)
    rc = L.cvc_grounder_fwd(xd.data_ptr(), fd.data_ptr(), None if bd is None else bd.data_ptr(), None if md is None else md.data_ptr(), B, T, N, G,
                            out.ptr, stream())
    assert rc == 0
    return out.host("grounder out").reshape(B, T, N)


GR_FWD = [(c, True, True) for c in RR.GR_CASES] + [(c, b, m) for c in RR.GR_OPTION_CASES for b, m in ((True, False), (False, True), (False, False))]


@pytest.mark.parametrize("case,with_bias,with_mask", GR_FWD, ids=str)
def test_grounder_forward_elementwise_against_fp64(dev, L, case, with_bias, with_mask):
    """inside the dot-product bound; masked slots bitwise -1e8; unmasked slots bitwise the mask-free run's"""
    xt, feats, bias, mask, _d = RR.gr_values(case)
    bias, mask = bias if with_bias else None, mask if with_mask else None
    want, bound = RR.gr_fwd_fp64(xt, feats, bias, mask)
    got = run_grounder_fwd(L, dev, xt, feats, bias, mask)
    check("cvc_grounder_fwd", "%s bias %s mask %s" % (case, with_bias, with_mask), got, want, bound)
    if with_mask:
        free = run_grounder_fwd(L, dev, xt, feats, bias, None)
        assert (bits(got[mask]) == bits(F(RR.MIN_VALUE))).all() and same_bits(got[~mask], free[~mask])


@pytest.mark.parametrize("case", RR.GR_CASES, ids=str)
def test_grounder_backward_elementwise_against_fp64(dev, L, case):
    """d_xt-only, d_feats-only and both: the same bits, element-wise inside u depth sum |d| |operand|"""
    B, T, N, G = case
    xt, feats, _bias, _mask, d = RR.gr_values(case)
    d_xt, e_xt, d_f, e_f = RR.gr_bwd_fp64(d, xt, feats)
    dd, xd, fd = up(dev, d), up(dev, xt), up(dev, feats)

    def run(want_xt, want_f):
        a = Arena(dev, B * T * G) if want_xt else None
        b = Arena(dev, B * N * G) if want_f else None
        rc = L.cvc_grounder_bwd(dd.data_ptr(), xd.data_ptr(), fd.data_ptr(), B, T, N, G, a.ptr if a else None, b.ptr if b else None, stream())
        assert rc == 0
        return (a.host("d_xt").reshape(B, T, G) if a else None), (b.host("d_feats").reshape(B, N, G) if b else None)
    gx, _n = run(True, False)
    _n, gf = run(False, True)
    bx, bf = run(True, True)
    assert same_bits(bx, gx) and same_bits(bf, gf)
    check("cvc_grounder_bwd", "%s d_xt" % (case,), gx, d_xt, e_xt)
    check("cvc_grounder_bwd", "%s d_feats" % (case,), gf, d_f, e_f)


# ================================================================================================ cvc_embed_relu_fwd
@pytest.mark.parametrize("with_drop", [False, True], ids=["no-drop", "drop"])
@pytest.mark.parametrize("case", RR.EMBED_CASES, ids=str)
def test_embed_relu_is_exact(dev, L, case, with_drop):
    """bitwise max(table[idx], 0) (x drop); the rows no index selects are NaN"""
    M, V, E = case
    table, idx, drop = RR.embed_values(case)
    drop = drop if with_drop else None
    td, idd = up(dev, table), up(dev, idx)
    dd = None if drop is None else up(dev, drop)
    out = Arena(dev, M * E)
    rc = L.cvc_embed_relu_fwd(td.data_ptr(), idd.data_ptr(), None if dd is None else dd.data_ptr(), M, E, out.ptr, stream())
    assert rc == 0
    got = out.host("embed out").reshape(M, E)
    want = RR.embed_ref(table, idx, drop)
    assert np.isfinite(want).all() and same_bits(got, want)
    WORST.setdefault("cvc_embed_relu_fwd", 0.0)


def test_zz_print_the_worst_ratio_per_entry_point():
    for e in sorted(WORST):
        print("worst |err| / (K x bound) of %s: %.3g" % (e, WORST[e]))
