"""The GRU frame encoder's kernels on the GPU, every entry point called by name, element-wise against the fp64 restatement of
tests/gru_ref.py (proven against nn.GRU in tests/test_gru_ref_cpu.py): cvc_gru_seq_fwd / cvc_gru_seq_train_fwd (per-step forms,
csrc/gemm_packed.hip), cvc_gru_seq_persistent_fwd / cvc_gru_seq_persistent_train_fwd (csrc/gru_persistent.hip, every instantiation),
cvc_gru_seq_bwd with cvc_gru_seq_bwd_ksplit (csrc/gru_bwd.hip), cvc_gru_seq_bwd_persistent (csrc/gru_bwd_persistent.hip, every NKS) and
the sync-word queries; then cvc.gru.gru_forward_train through autograd, with and without inter-layer dropout.

The recurrences are isolated: gi = x W_ih^T is made on the host in fp64 and rounded to fp32 (no tile GEMM), and the backward kernels
read `gates` / `y` of the fp64 reference rounded to fp32 (no forward kernel).  Padding of every strided operand is NaN (inputs) or
a sentinel (outputs) and must stay so.  Tolerances are the project's: OP_TOL on y and the saved gates, GRAD_TOL on dgi / dgh / dx,
red_tol(F * M) on the summed parameter gradients; all comparisons are element-wise.

Every comparison prints its max-abs error against fp64 and the reference's magnitude (run with -s); the ids and the printed lines
name H, M and the wave count / NKS of the instantiation that ran.  Measured on an MI355X, max-abs from fp64 over the shapes below
(|y|, |r|, |z|, |n| <= 1, |hn| <= 2.2, |dgi|, |dgh| <= 6):
  persistent forward (28 instantiations)   y 1.9e-7 .. 4.6e-7, r / z 0.8e-7 .. 2.2e-7, n 1.7e-7 .. 5.3e-7, hn 1.5e-7 .. 8.2e-7
  per-step forward (H = 8 .. 2048)         y 0.2e-7 .. 3.9e-7, r / z 0.3e-7 .. 1.8e-7, n 1.0e-7 .. 4.3e-7, hn 0 .. 5.7e-7
  the two forward forms from each other    y 4.2e-7, gates 2.4e-7; padded layouts give the bits of the dense call
  cvc_gru_seq_bwd                          dgi 0.2e-7 .. 6.7e-7, dgh 0.2e-7 .. 5.2e-7
  cvc_gru_seq_bwd_persistent (NKS 3..12)   dgi 1.3e-7 .. 7.8e-7, dgh 0.8e-7 .. 6.0e-7; 0 .. 7.2e-7 from the per-step form
  gru_forward_train, 2 and 3 layers        y 1.8e-7 .. 3.5e-7, dx 4.7e-7 .. 7.9e-7, dW_ih 1.0e-6 .. 1.4e-5 (|ref| <= 29), dW_hh 2.1e-7 ..
                                           2.6e-6 (<= 5.7), db_ih 0.7e-6 .. 1.1e-5 (<= 37), db_hh 0.4e-6 .. 6.5e-6 (<= 18), either backward
  ... under dropout 0.2                    y 3.0e-7, dx 8.8e-7, dW_ih 3.2e-6, dW_hh 8.5e-7, db_ih 2.9e-6, db_hh 1.7e-6; eval 2.4e-7
two orders inside OP_TOL / GRAD_TOL; the LSTM recurrence reads 1e-7 .. 1.9e-7 at the same tolerances (tests/test_gpu_lstm_seq.py).
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import gru_ref as R
from test_gpu_parity import GRAD_TOL, OP_TOL
from test_gpu_train_kernels import BADARG, SENTINEL, _gen, red_tol

pytestmark = pytest.mark.gpu

NAN = float("nan")
INP = 16           # width of the x behind gi


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    from cvc import hip
    return hip.lib()


def _stream():
    from cvc import hip
    return hip._stream()


def close(got, want, what, tol):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    print("%s: max |err| %.3g (max |ref| %.3g)" % (what, float((got - want).abs().max()), float(want.abs().max())))
    np.testing.assert_allclose(got.numpy(), want.numpy(), err_msg=what, **tol)


# ------------------------------------------------------------------------------------------------ operands and references
@functools.lru_cache(maxsize=None)
def weights(H):
    """W_hh, b_ih, b_hh of two directions at nn.GRU's initialisation scaled by 1.5 (the gates leave the linear region)"""
    g = _gen("gru weights", H)
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * (1.5 / H ** 0.5)
    return u(2, 3 * H, H), u(2, 3 * H), u(2, 3 * H)


@functools.lru_cache(maxsize=2)
def packed(H, dev):
    """the two packings of W_hh on the device: cvc_gru_seq_*fwd's and cvc_gru_seq_bwd_persistent's"""
    from cvc.gru import pack_gru_weights, pack_gru_weights_t
    w = weights(H)[0].to(dev)
    return torch.stack([pack_gru_weights(w[d], H) for d in range(2)]), torch.stack([pack_gru_weights_t(w[d], H) for d in range(2)])


@functools.lru_cache(maxsize=None)
def ops(H, M, F, ndir):
    """One case's host operands and its fp64 reference (made once, shared, never written to): gi [M, F, ndir * 3H] fp32, y / gates of
    the forward, and dgi / dgh of the backward from a random dy and the forward's results ROUNDED to fp32 (what the kernels read)."""
    g = _gen("gru case", H, M, F, ndir)
    w_hh, b_ih, b_hh = [t[:ndir] for t in weights(H)]
    x = torch.randn(M, F, INP, generator=g)
    w_ih = (torch.rand(ndir * 3 * H, INP, generator=g) * 2 - 1) * (1.5 / INP ** 0.5) * 2
    gi = (x.double() @ w_ih.double().T).float()
    dy = torch.randn(M, F, ndir * H, generator=g)
    ys, gs, dgis, dghs = [], [], [], []
    for d in range(ndir):
        wd = w_hh[d].double()
        y, gates = R.gru_recurrence(gi[:, :, d * 3 * H:(d + 1) * 3 * H].double(), wd, b_ih[d].double(), b_hh[d].double(), d == 1)
        ys.append(y)
        gs.append(gates.reshape(M, F, 4 * H))
        none = torch.zeros(M, F, 1, dtype=torch.float64), torch.zeros(3 * H, 1, dtype=torch.float64)      # no input side here
        dgi, dgh = R.gru_layer_backward(dy[:, :, d * H:(d + 1) * H].double(), none[0], y.float().double(),
                                        gates.float().double(), none[1], wd, d == 1)[5:]
        dgis.append(dgi)
        dghs.append(dgh)
    cat = lambda ts: torch.cat(ts, 2)
    return types.SimpleNamespace(H=H, M=M, F=F, ndir=ndir, w_hh=w_hh.contiguous(), b_ih=b_ih.contiguous(), b_hh=b_hh.contiguous(), gi=gi,
                                 dy=dy, y=cat(ys), gates=cat(gs), dgi=cat(dgis), dgh=cat(dghs))


class Lay:
    """A [M, F, W] operand in device memory: row of (clip m, step t) at m * ld_m + t * ld_t, time-major ("tm": [F][M + extra][W + pad])
    or batch-major ("bm": [M + extra][F][W + pad], as gru_forward's last layer writes); everything outside the [M, F, W] block -- pad
    columns, `extra` clip rows -- holds `fill`."""

    def __init__(self, dev, M, F, W, fill, data=None, layout="tm", pad=0, extra=0):
        self.M, self.W, self.fill, self.tm = M, W, fill, layout == "tm"
        self.buf = torch.full((F, M + extra, W + pad) if self.tm else (M + extra, F, W + pad), fill, device=dev, dtype=torch.float32)
        self.ld_m, self.ld_t = (W + pad, (M + extra) * (W + pad)) if self.tm else (F * (W + pad), W + pad)
        if data is not None:
            self.get().copy_(data.float())

    def get(self):
        v = self.buf[:, :self.M, :self.W]
        return v.transpose(0, 1) if self.tm else self.buf[:self.M, :, :self.W]

    def ptr(self):
        return self.buf.data_ptr()

    def outside_untouched(self):
        c = self.buf.clone()
        (c[:, :self.M, :self.W] if self.tm else c[:self.M, :, :self.W]).fill_(self.fill)
        return bool(torch.isnan(c).all()) if self.fill != self.fill else bool((c == self.fill).all())

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _train_fwd_block(L):
    """cvc_gru_seq_train_fwd is a building block: bound through cvc_block("name")"""
    P, LL, I = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    addr = L.cvc_block(b"cvc_gru_seq_train_fwd")
    assert addr, "cvc_gru_seq_train_fwd is not in the library's table"
    return ctypes.CFUNCTYPE(I, P, P, LL, LL, P, P, I, I, I, I, P, P, LL, LL, P, LL, LL, P)(addr)


FWD_BASE = ["wp", "gi", "gi_ld_m", "gi_ld_t", "b_ih", "b_hh", "M", "F", "H", "ndir", "hq", "y", "y_ld_m", "y_ld_t"]
FWD_GATES = ["gates", "g_ld_m", "g_ld_t"]
FWD_FORMS = ["cvc_gru_seq_fwd", "cvc_gru_seq_train_fwd", "cvc_gru_seq_persistent_fwd", "cvc_gru_seq_persistent_train_fwd"]


class Fwd:
    """One case's device operands for the four forward entry points; outputs pre-filled with SENTINEL, gi's padding with NaN."""

    def __init__(self, L, dev, o, layout="tm", pad=0, extra=0):
        H, M, F, ndir = o.H, o.M, o.F, o.ndir
        self.L, self.o = L, o
        self.gi = Lay(dev, M, F, ndir * 3 * H, NAN, o.gi, layout, pad, extra)
        self.y = Lay(dev, M, F, ndir * H, SENTINEL, None, layout, pad, extra)
        self.gates = Lay(dev, M, F, ndir * 4 * H, SENTINEL, None, layout, pad, extra)
        self.wp = packed(H, dev)[0][:ndir]
        self.b_ih, self.b_hh = o.b_ih.to(dev), o.b_hh.to(dev)
        Kp = (H + 31) // 32 * 32
        self.hq = torch.empty(max(2 * ndir * Kp * 64, (F + 1) * ndir * H * 64), device=dev)     # either form's workspace
        self.sync = torch.zeros(int(L.cvc_gru_persistent_sync_words()), dtype=torch.int32, device=dev)

    def call(self, name, **over):
        a = dict(wp=self.wp.data_ptr(), gi=self.gi.ptr(), gi_ld_m=self.gi.ld_m, gi_ld_t=self.gi.ld_t, b_ih=self.b_ih.data_ptr(),
                 b_hh=self.b_hh.data_ptr(), M=self.o.M, F=self.o.F, H=self.o.H, ndir=self.o.ndir, hq=self.hq.data_ptr(), y=self.y.ptr(),
                 y_ld_m=self.y.ld_m, y_ld_t=self.y.ld_t, gates=self.gates.ptr(), g_ld_m=self.gates.ld_m, g_ld_t=self.gates.ld_t,
                 sync=self.sync.data_ptr())
        assert set(over) <= set(a), over
        a.update(over)
        L, st = self.L, _stream()
        if name == "cvc_gru_seq_fwd":
            return L.cvc_gru_seq_fwd(*[a[k] for k in FWD_BASE], st)
        if name == "cvc_gru_seq_train_fwd":
            return _train_fwd_block(L)(*[a[k] for k in FWD_BASE + FWD_GATES], st)
        if name == "cvc_gru_seq_persistent_fwd":
            return L.cvc_gru_seq_persistent_fwd(*[a[k] for k in FWD_BASE], a["sync"], st)
        assert name == "cvc_gru_seq_persistent_train_fwd", name
        return L.cvc_gru_seq_persistent_train_fwd(*[a[k] for k in FWD_BASE + FWD_GATES], a["sync"], st)

    def run(self, name):
        """-> (y, gates or None) as [M, F, .] copies; a persistent form must launch and leave its error word clear"""
        self.y.buf.fill_(SENTINEL)
        self.gates.buf.fill_(SENTINEL)
        assert self.call(name) == 0, name
        torch.cuda.synchronize()
        if "persistent" in name:
            assert int(self.sync[4]) == 0, name + ": barrier time-out word set"
        return self.y.get().clone(), (self.gates.get().clone() if "train" in name else None)


def check_forward(f, train, infer, tag):
    """the training form against fp64 (y and the four gate planes of every direction), the inference form bit-equal to it, a second
    run of the training form bit-equal to the first"""
    o = f.o
    H = o.H
    y, gates = f.run(train)
    close(y, o.y, "%s y" % tag, OP_TOL)
    for d in range(o.ndir):
        for p, nm in enumerate(("r", "z", "n", "hn")):
            sl = slice(d * 4 * H + p * H, d * 4 * H + (p + 1) * H)
            close(gates[:, :, sl], o.gates[:, :, sl], "%s gate %s dir %d" % (tag, nm, d), OP_TOL)
    y2, gates2 = f.run(train)
    assert torch.equal(y, y2) and torch.equal(gates, gates2), tag + ": a second run gives other bits"
    yi, _ = f.run(infer)
    assert f.gates.untouched(), tag + ": the inference form wrote gates"
    assert torch.equal(y, yi), tag + ": training and inference form differ"
    return y, gates


# ------------------------------------------------------------------------------------------------ A: persistent forward
A_CASES = ([(H, M, 1) for H in (128, 256, 384, 512, 640, 768, 896, 1024) for M in (32, 33)] +
           [(H, M, 0) for H in (256, 512, 768, 1024) for M in (32, 33)] + [(H, M, 1) for H in (128, 1024) for M in (1, 64)])


@pytest.mark.parametrize("H,M,waves8", A_CASES, ids=["H%d-M%d-%dwaves" % (H, M, 8 if w and H % 256 == 0 else 4) for H, M, w in A_CASES])
def test_persistent_forward_every_instantiation_vs_fp64(dev, L, H, M, waves8):
    """gru_persistent_kernel<1, MT, NC, NW>: NC 1..8 at 4 waves (H = 128 .. 1024; H % 256 == 0 with the 8-wave form switched off),
    NC 1..4 at 8 waves, each at MT 1 (M <= 32) and MT 2"""
    prev = L.cvc_gru_persistent_waves8(waves8)
    try:
        f = Fwd(L, dev, ops(H, M, 3, 2))
        check_forward(f, "cvc_gru_seq_persistent_train_fwd", "cvc_gru_seq_persistent_fwd",
                      "persistent H=%d M=%d %d waves" % (H, M, 8 if waves8 and H % 256 == 0 else 4))
    finally:
        L.cvc_gru_persistent_waves8(prev)


# ------------------------------------------------------------------------------------------------ B: per-step forward
B_CASES = [(8, 1, 1, 1), (8, 33, 5, 2), (40, 32, 2, 2), (40, 64, 5, 1), (136, 33, 5, 2), (136, 1, 2, 1), (200, 64, 1, 2), (200, 32, 5, 1),
           (2048, 33, 2, 2)]


@pytest.mark.parametrize("H,M,F,ndir", B_CASES)
def test_per_step_forward_vs_fp64(dev, L, H, M, F, ndir):
    check_forward(Fwd(L, dev, ops(H, M, F, ndir)), "cvc_gru_seq_train_fwd", "cvc_gru_seq_fwd", "per-step H=%d M=%d F=%d ndir=%d" % (H, M, F, ndir))


def test_per_step_and_persistent_forward_agree(dev, L):
    f = Fwd(L, dev, ops(256, 37, 3, 2))
    ys, gs = check_forward(f, "cvc_gru_seq_train_fwd", "cvc_gru_seq_fwd", "per-step H=256 M=37")
    yp, gp = check_forward(f, "cvc_gru_seq_persistent_train_fwd", "cvc_gru_seq_persistent_fwd", "persistent H=256 M=37")
    close(ys, yp, "per-step vs persistent y", OP_TOL)
    close(gs, gp, "per-step vs persistent gates", OP_TOL)


# ------------------------------------------------------------------------------------------------ C: layouts
@pytest.mark.parametrize("pad", [4, 8])
@pytest.mark.parametrize("layout", ["tm", "bm"])
@pytest.mark.parametrize("H,train,infer", [(128, "cvc_gru_seq_persistent_train_fwd", "cvc_gru_seq_persistent_fwd"),
                                           (40, "cvc_gru_seq_train_fwd", "cvc_gru_seq_fwd")])
def test_forward_layouts_and_padding(dev, L, H, train, infer, layout, pad):
    """time-major and batch-major rows with leading dimensions `pad` floats wider than the used columns and one clip row more than M:
    same bits as the dense time-major call; NaN in gi's padding reaches nothing; y's and gates' padding keeps the sentinel"""
    o = ops(H, 5, 3, 2)
    y0, g0 = Fwd(L, dev, o).run(train)
    f = Fwd(L, dev, o, layout, pad, 1)
    y, gates = check_forward(f, train, infer, "%s %s pad %d" % (train, layout, pad))
    assert torch.equal(y, y0) and torch.equal(gates, g0)
    for name in (infer, train):
        f.run(name)
        assert f.y.outside_untouched() and f.gates.outside_untouched() and f.gi.outside_untouched(), name


# ------------------------------------------------------------------------------------------------ D, E: backward
BWD_HEAD = ["dy", "dy_ld_m", "dy_ld_t", "gates", "g_ld_m", "g_ld_t", "y", "y_ld_m", "y_ld_t"]
BWD_DIMS = ["M", "F", "H", "ndir", "dgi", "dgh"]


def work_floats(L, M, H, ndir):
    """include/cvc_hip.h: ndir * (2 M H + 192 H + ksplit * M * ceil(H/128) * 128)"""
    return ndir * (2 * M * H + 192 * H + int(L.cvc_gru_seq_bwd_ksplit(H)) * M * ((H + 127) // 128) * 128)


class Bwd:
    """One case's device operands for the two backward entry points: dy random, gates / y the fp64 reference's rounded to fp32, their
    padding NaN; work and slots NaN beforehand; dgi / dgh pre-filled with SENTINEL."""

    def __init__(self, L, dev, o, layout="tm", pad=0, extra=0):
        H, M, F, ndir = o.H, o.M, o.F, o.ndir
        self.L, self.o = L, o
        self.dy = Lay(dev, M, F, ndir * H, NAN, o.dy, layout, pad, extra)
        self.gates = Lay(dev, M, F, ndir * 4 * H, NAN, o.gates, layout, pad, extra)
        self.y = Lay(dev, M, F, ndir * H, NAN, o.y, layout, pad, extra)
        self.w_hh = o.w_hh.to(dev)
        self.dgi = torch.full((F * M, ndir * 3 * H), SENTINEL, device=dev)
        self.dgh = torch.full((F * M, ndir * 3 * H), SENTINEL, device=dev)
        self.work = torch.full((work_floats(L, M, H, ndir),), NAN, device=dev)
        self.persistent_ok = H % 256 == 0 and H <= 1024
        if self.persistent_ok:
            self.wt = packed(H, dev)[1][:ndir]
            self.slots = torch.full((F * ndir * 3 * H * 64,), NAN, device=dev)
            self.sync = torch.zeros(int(L.cvc_gru_bwd_persistent_sync_words()), dtype=torch.int32, device=dev)

    def call(self, name, **over):
        a = dict(dy=self.dy.ptr(), dy_ld_m=self.dy.ld_m, dy_ld_t=self.dy.ld_t, gates=self.gates.ptr(), g_ld_m=self.gates.ld_m,
                 g_ld_t=self.gates.ld_t, y=self.y.ptr(), y_ld_m=self.y.ld_m, y_ld_t=self.y.ld_t, w_hh=self.w_hh.data_ptr(), M=self.o.M,
                 F=self.o.F, H=self.o.H, ndir=self.o.ndir, dgi=self.dgi.data_ptr(), dgh=self.dgh.data_ptr(), work=self.work.data_ptr())
        if self.persistent_ok:
            a.update(wt=self.wt.data_ptr(), slots=self.slots.data_ptr(), sync=self.sync.data_ptr())
        assert set(over) <= set(a), over
        a.update(over)
        L, st = self.L, _stream()
        if name == "cvc_gru_seq_bwd":
            return L.cvc_gru_seq_bwd(*[a[k] for k in BWD_HEAD + ["w_hh"] + BWD_DIMS + ["work"]], st)
        assert name == "cvc_gru_seq_bwd_persistent", name
        return L.cvc_gru_seq_bwd_persistent(*[a[k] for k in BWD_HEAD + ["wt"] + BWD_DIMS + ["slots", "sync"]], st)

    def run(self, name):
        """-> dgi, dgh as [M, F, ndir * 3H] copies"""
        o = self.o
        self.dgi.fill_(SENTINEL)
        self.dgh.fill_(SENTINEL)
        self.work.fill_(NAN)
        if self.persistent_ok:
            self.slots.fill_(NAN)
        assert self.call(name) == 0, name
        torch.cuda.synchronize()
        if "persistent" in name:
            assert int(self.sync[4]) == 0, name + ": barrier time-out word set"
        rows = lambda t: t.view(o.F, o.M, -1).transpose(0, 1).clone()              # rows (t * M + m) -> [M, F, .]
        return rows(self.dgi), rows(self.dgh)


def check_backward(b, name, tag):
    o = b.o
    H = o.H
    dgi, dgh = b.run(name)
    for d in range(o.ndir):
        sl = slice(d * 3 * H, (d + 1) * 3 * H)
        close(dgi[:, :, sl], o.dgi[:, :, sl], "%s dgi dir %d" % (tag, d), GRAD_TOL)
        close(dgh[:, :, sl], o.dgh[:, :, sl], "%s dgh dir %d" % (tag, d), GRAD_TOL)
    dgi2, dgh2 = b.run(name)
    assert torch.equal(dgi, dgi2) and torch.equal(dgh, dgh2), tag + ": a second run gives other bits"
    assert b.dy.outside_untouched() and b.gates.outside_untouched() and b.y.outside_untouched()
    return dgi, dgh


D_CASES = [(8, 1, 1, 1, "tm", 0), (8, 37, 6, 2, "bm", 4), (40, 64, 2, 2, "tm", 8), (136, 37, 6, 2, "tm", 0), (136, 64, 2, 1, "bm", 8),
           (200, 37, 2, 2, "bm", 4), (200, 1, 6, 1, "tm", 4), (256, 64, 6, 2, "tm", 0), (256, 37, 1, 2, "bm", 0), (2048, 37, 2, 2, "tm", 0)]


@pytest.mark.parametrize("H,M,F,ndir,layout,pad", D_CASES)
def test_per_step_backward_vs_fp64(dev, L, H, M, F, ndir, layout, pad):
    """cvc_gru_seq_bwd from the reference's saved tensors: dgi and dgh of every direction, with `work` (sized as the header says) full
    of NaN beforehand -- the zero quad rows beyond M and the K-slice planes are the kernels' own"""
    o = ops(H, M, F, ndir)
    b = Bwd(L, dev, o, layout, pad, 1 if pad else 0)
    check_backward(b, "cvc_gru_seq_bwd", "per-step bwd H=%d M=%d F=%d ndir=%d %s pad %d ksplit %d" %
                   (H, M, F, ndir, layout, pad, int(L.cvc_gru_seq_bwd_ksplit(H))))
    per_dir = b.work.numel() // ndir
    for d in range(ndir):                 # the quad operand of dgh W_hh: [3H/4][64][4], rows beyond M zero
        q = b.work[d * per_dir + 2 * M * H:d * per_dir + 2 * M * H + 3 * H * 64].view(3 * H // 4, 64, 4)
        assert bool((q[:, M:] == 0).all()), "dgh_q rows beyond M, direction %d" % d
        want = o.dgh[:, (0 if d == 0 else F - 1), d * 3 * H:(d + 1) * 3 * H]       # the last processed step's dgh
        close(q[:, :M].permute(1, 0, 2).reshape(M, 3 * H), want, "dgh_q dir %d" % d, GRAD_TOL)


E_CASES = [(256, 1, 1, 1, "tm", 0), (256, 33, 5, 2, "bm", 4), (512, 64, 2, 2, "tm", 1), (512, 33, 5, 1, "tm", 0), (768, 33, 5, 2, "tm", 0),
           (768, 64, 1, 2, "bm", 3), (768, 1, 2, 1, "tm", 0), (1024, 64, 5, 2, "tm", 0), (1024, 1, 2, 2, "bm", 0), (1024, 33, 1, 1, "tm", 0)]


@pytest.mark.parametrize("H,M,F,ndir,layout,pad", E_CASES)
def test_persistent_backward_vs_fp64_and_per_step(dev, L, H, M, F, ndir, layout, pad):
    """gru_bwd_persistent_kernel<NKS>, NKS = 3, 6, 9, 12: exchange slots full of NaN beforehand (the rows of clips >= M are never
    written and must reach no output); it reads dy / gates / y one float at a time, so odd leading dimensions (pad 1, 3) are in range"""
    o = ops(H, M, F, ndir)
    b = Bwd(L, dev, o, layout, pad, 1 if pad else 0)
    dgi, dgh = check_backward(b, "cvc_gru_seq_bwd_persistent", "persistent bwd H=%d (NKS %d) M=%d F=%d ndir=%d %s pad %d" %
                              (H, 3 * H // 256, M, F, ndir, layout, pad))
    si, sh = Bwd(L, dev, o).run("cvc_gru_seq_bwd")
    close(dgi, si, "persistent vs per-step dgi", GRAD_TOL)
    close(dgh, sh, "persistent vs per-step dgh", GRAD_TOL)


# ------------------------------------------------------------------------------------------------ F, G: through autograd
def want_fwd_form(H):
    return "persistent" if (H % 128 == 0 and H <= 1024) else "steps"


def want_bwd_form(H):
    return "persistent" if (H % 256 == 0 and H <= 1024) else "steps"


def check_autograd(gd, x, probe, want_y, want_dx, want, tag, bwd_form):
    """one forward + backward of cvc.gru.gru_forward_train against the reference, element-wise"""
    from cvc import gru as G
    B, F, _ = x.shape
    for p in gd.parameters():
        p.grad = None
    xg = x.cuda().requires_grad_(True)
    assert G.supported_train(gd, xg)
    y = G.gru_forward_train(gd, xg)
    assert G.last_train_form == want_fwd_form(gd.hidden_size), G.last_train_form
    close(y, want_y, tag + " y", OP_TOL)
    (y * probe.cuda()).sum().backward()
    assert G.last_bwd_form == bwd_form, G.last_bwd_form
    close(xg.grad, want_dx, tag + " dx", GRAD_TOL)
    for k, p in gd.named_parameters():
        assert p.grad is not None, k
        close(p.grad, want[k], tag + " d" + k, red_tol(F * B))


@pytest.mark.parametrize("B,F,inp,H,layers", [(5, 4, 48, 128, 2), (37, 5, 80, 256, 3), (70, 3, 64, 768, 2), (6, 5, 24, 16, 3), (33, 2, 40, 200, 2)])
def test_gru_forward_train_elementwise_vs_fp64(dev, B, F, inp, H, layers):
    """tile-GEMM input projections + recurrence + backward + dense dW / dX products, bidirectional: output, input gradient and every
    parameter gradient element-wise; where the persistent backward ran, once more on the per-step backward"""
    from cvc import gru as G
    gru = R.make_gru(inp, H, layers, True, 11)
    g = _gen("gru autograd", B, F, inp, H, layers)
    x, probe = torch.randn(B, F, inp, generator=g), torch.randn(B, F, 2 * H, generator=g)
    params = {k: v.detach().clone() for k, v in gru.named_parameters()}
    want_y, saved = R.gru_forward(x, params, layers, True)
    want_dx, want = R.gru_backward(probe, saved, params, layers, True)
    gd = gru.to(dev)
    tag = "autograd B=%d F=%d H=%d layers=%d" % (B, F, H, layers)
    check_autograd(gd, x, probe, want_y, want_dx, want, tag, want_bwd_form(H))
    if want_bwd_form(H) == "persistent":
        G.BWD_PERSISTENT = False
        try:
            check_autograd(gd, x, probe, want_y, want_dx, want, tag + " (per-step backward)", "steps")
        finally:
            G.BWD_PERSISTENT = True


@pytest.mark.parametrize("B,F,inp,H", [(6, 5, 32, 128), (5, 4, 24, 40)])
def test_gru_train_mode_dropout_uses_the_kernel_mask(dev, B, F, inp, H):
    """train() with dropout 0.2 between three layers: output and every gradient equal the fp64 reference under the kernels' own masks
    (sites enc.gru.<l>) restated on the host; eval() afterwards is the undropped reference"""
    from cvc import dropout, gru as G
    layers = 3
    gru = R.make_gru(inp, H, layers, True, 17, dropout=0.2)
    g = _gen("gru dropout", B, F, inp, H)
    x, probe = torch.randn(B, F, inp, generator=g), torch.randn(B, F, 2 * H, generator=g)
    params = {k: v.detach().clone() for k, v in gru.named_parameters()}
    gd = gru.to(dev).train()
    dropout.seed(123)
    xg = x.cuda().requires_grad_(True)
    y = G.gru_forward_train(gd, xg)
    (y * probe.cuda()).sum().backward()
    # the masks act on time-major rows (t, clip): [F * B, 2H] -> [B, F, 2H]
    masks = [dropout.host_mask("enc.gru.%d" % l, (F * B, 2 * H), 0.2, dev).view(F, B, 2 * H).transpose(0, 1).double().cpu()
             for l in range(layers - 1)]
    assert all(0 < float((m == 0).double().mean()) < 0.5 for m in masks)
    want_y, saved = R.gru_forward(x, params, layers, True, masks)
    want_dx, want = R.gru_backward(probe, saved, params, layers, True, masks)
    tag = "dropout H=%d" % H
    close(y, want_y, tag + " y", OP_TOL)
    close(xg.grad, want_dx, tag + " dx", GRAD_TOL)
    for k, p in gd.named_parameters():
        close(p.grad, want[k], tag + " d" + k, red_tol(F * B))
    with torch.no_grad():
        gd.eval()
        close(G.gru_forward(gd, x.cuda()), R.gru_forward(x, params, layers, True)[0], tag + " eval", OP_TOL)


# ------------------------------------------------------------------------------------------------ H: contract
def test_sync_word_queries(L):
    """the error word of both persistent forms is word 4: the buffers the queries size must hold it"""
    assert int(L.cvc_gru_persistent_sync_words()) > 4 and int(L.cvc_gru_bwd_persistent_sync_words()) > 4


def test_bwd_ksplit_contract(L):
    for H in range(8, 2049, 8):
        assert int(L.cvc_gru_seq_bwd_ksplit(H)) >= 1, H
    assert int(L.cvc_gru_seq_bwd_ksplit(8)) == 1
    H, M, ndir = 200, 37, 2
    ks = int(L.cvc_gru_seq_bwd_ksplit(H))
    assert ks > 1 and work_floats(L, M, H, ndir) == ndir * (2 * M * H + 192 * H + ks * M * 256)


@pytest.mark.parametrize("name", FWD_FORMS)
def test_forward_entry_points_refuse_arguments_outside_the_contract(dev, L, name):
    """CVC_E_BADARG, and nothing launched: y and gates keep their sentinel"""
    persistent, train = "persistent" in name, "train" in name
    o = ops(256, 8, 2, 2)
    f = Fwd(L, dev, o)
    # buffers large enough for every refused shape below (M = 65, ndir = 3, H up to 1152), at the valid case's strides
    big = lambda n: torch.full((n,), SENTINEL, device=dev)
    Hx, room = 1152, 65 * 2 * 3
    zeros = lambda n: torch.zeros(n, device=dev)
    ins = dict(wp=zeros(3 * 4 * Hx * Hx), gi=zeros(room * 3 * Hx), b_ih=zeros(9 * Hx), b_hh=zeros(9 * Hx), hq=zeros(3 * 3 * Hx * 64))
    keep = [big(room * Hx), big(room * 4 * Hx)]
    over_ok = {k: t.data_ptr() for k, t in ins.items()}
    over_ok.update(y=keep[0].data_ptr(), gates=keep[1].data_ptr())
    bad = [dict(M=0), dict(M=65), dict(F=0), dict(ndir=0), dict(ndir=3)]
    bad += [{k: None} for k in ["wp", "gi", "b_ih", "b_hh", "hq", "y"] + (["sync"] if persistent else []) + (["gates"] if train else [])]
    bad += [dict(H=136), dict(H=1152)] if persistent else [dict(H=252), dict(H=4)]
    bad += [{k: v + off} for k, v in (("gi_ld_m", f.gi.ld_m), ("gi_ld_t", f.gi.ld_t), ("y_ld_m", f.y.ld_m), ("y_ld_t", f.y.ld_t)) for off in (1, 2)]
    if train:
        bad += [dict(g_ld_m=f.gates.ld_m + 2), dict(g_ld_t=f.gates.ld_t + 1)]
    for kw in bad:
        args = dict(over_ok)
        args.update(kw)
        assert f.call(name, **args) == BADARG, "%s accepted %r" % (name, kw)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in keep) and f.y.untouched() and f.gates.untouched(), name + " launched on a refused call"
    assert f.call(name) == 0                           # the same operands inside the contract run
    torch.cuda.synchronize()
    close(f.y.get(), o.y, name + " y", OP_TOL)


@pytest.mark.parametrize("name", ["cvc_gru_seq_bwd", "cvc_gru_seq_bwd_persistent"])
def test_backward_entry_points_refuse_arguments_outside_the_contract(dev, L, name):
    """CVC_E_BADARG, and nothing launched: dgi and dgh keep their sentinel.  cvc_gru_seq_bwd reads dy / gates / y four floats at a
    time and refuses strides that are no multiple of 4 floats; the persistent form takes any stride (test E runs odd ones)."""
    persistent = "persistent" in name
    o = ops(256, 8, 2, 2)
    b = Bwd(L, dev, o)
    Hx, room = 1280, 65 * 2 * 3
    zeros = lambda n: torch.zeros(n, device=dev)
    ins = [zeros(room * Hx), zeros(room * 4 * Hx), zeros(room * Hx), zeros(3 * 3 * Hx * Hx)]
    outs = [torch.full((room * 3 * Hx,), SENTINEL, device=dev) for _ in range(2)]
    scratch = torch.empty(max(3 * (2 * 65 * Hx + 192 * Hx + 32 * 65 * Hx), 2 * 3 * 3 * Hx * 64), device=dev)
    over_ok = dict(dy=ins[0].data_ptr(), gates=ins[1].data_ptr(), y=ins[2].data_ptr(), dgi=outs[0].data_ptr(), dgh=outs[1].data_ptr())
    over_ok.update(dict(wt=ins[3].data_ptr(), slots=scratch.data_ptr()) if persistent else dict(w_hh=ins[3].data_ptr(), work=scratch.data_ptr()))
    bad = [dict(M=0), dict(M=65), dict(F=0), dict(ndir=0), dict(ndir=3)]
    bad += [{k: None} for k in ["dy", "gates", "y", "dgi", "dgh"] + (["wt", "slots", "sync"] if persistent else ["w_hh", "work"])]
    if persistent:
        bad += [dict(H=128), dict(H=384), dict(H=1280)]
    else:
        bad += [dict(H=252), dict(H=4)]
        bad += [{k: v + off} for k, v in (("dy_ld_m", b.dy.ld_m), ("dy_ld_t", b.dy.ld_t), ("g_ld_m", b.gates.ld_m), ("g_ld_t", b.gates.ld_t),
                                          ("y_ld_m", b.y.ld_m), ("y_ld_t", b.y.ld_t)) for off in (1, 2)]
    for kw in bad:
        args = dict(over_ok)
        args.update(kw)
        assert b.call(name, **args) == BADARG, "%s accepted %r" % (name, kw)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs + [b.dgi, b.dgh]), name + " launched on a refused call"
    dgi, _ = b.run(name)                               # the same operands inside the contract run
    close(dgi, o.dgi, name + " dgi", GRAD_TOL)
