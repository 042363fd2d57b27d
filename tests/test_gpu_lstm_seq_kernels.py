"""The LSTM frame encoder's kernels on the GPU (csrc/lstm_seq.hip), every entry point called by name, element-wise against the fp64
restatement of tests/lstm_ref.py (proven against nn.LSTM in tests/test_lstm_seq_cpu.py): cvc_lstm_seq_fwd / cvc_lstm_seq_train_fwd
(per-step forms, both tiles), cvc_lstm_seq_persistent_fwd / cvc_lstm_seq_persistent_train_fwd (every instantiation, with
cvc_lstm_persistent_sync_words), cvc_lstm_seq_bwd with cvc_lstm_seq_bwd_work (every K-split count); then
cvc.lstm_seq.lstm_forward_train through autograd, with and without inter-layer dropout.  The twin of tests/test_gpu_gru_seq.py.

The recurrence is isolated: gi = x W_ih^T is made on the host in fp64 and rounded to fp32 (no tile GEMM), and the backward reads
`gates` / `c` of the fp64 reference rounded to fp32 (no forward kernel).  Padding of every strided operand is NaN (inputs) or a
sentinel (outputs) and must stay so; every float workspace (hq, slots, work) has exactly the size the product allocates, is full
of NaN before every call and carries a sentinel tail that must survive, as does dG.  Tolerances are the project's: OP_TOL on y, the
saved gates and c, GRAD_TOL on dG / dx, red_tol(F * B) on the summed parameter gradients, the ATOL / RTOL of
tests/test_gpu_lstm_seq.py on the y that went through the tile GEMM; all comparisons are element-wise.  The cases, operands and
comparisons are tests/lstm_seq_cases.py's; tests/test_lstm_seq_cases_cpu.py shows on the CPU that they notice a wrong kernel.

Every comparison prints its max-abs error against fp64 and the reference's magnitude (run with -s); the ids and the printed lines
name H, M and the (MT, NC, NW) of the instantiation that ran.  Measured on an MI355X, max-abs from fp64 over the shapes below
(|y| <= 0.98, gates <= 1, |c| <= 2.7, |dG| <= 3.2):
  persistent forward (16 instantiations)   y 2.1e-7 .. 3.4e-7, i / f / o 0.7e-7 .. 1.4e-7, g 1.7e-7 .. 3.6e-7, c 1.8e-7 .. 4.5e-7
  per-step forward (H = 8 .. 2048)         y 0.4e-7 .. 3.3e-7, i / f / o 0.6e-7 .. 1.6e-7, g 0.6e-7 .. 4.2e-7, c 0.4e-7 .. 3.9e-7
  the two forward forms from each other    y, gates, c 2.4e-7 .. 3.0e-7 at H = 256 (the same bits at H = 128: one k chunk per wave in
                                           either form); padded and clip-major layouts give the bits of the dense call
  cvc_lstm_seq_bwd (ksplit 1 .. 32)        dG 0.1e-7 .. 4.0e-7
  lstm_forward_train, 1 and 2 layers       y 1.3e-7 .. 1.6e-7, dx 1.7e-7 .. 3.4e-7, dW_ih 3.6e-7 .. 3.3e-6 (|ref| <= 11), dW_hh 1.1e-7 ..
                                           4.8e-7 (<= 1.4), db_ih = db_hh 3.4e-7 .. 3.0e-6 (<= 18), on either forward form
  ... under dropout 0.2, 3 layers          y 1.5e-7, dx 1.1e-7, dW_ih 5.3e-7, dW_hh 4.5e-7, db 1.2e-6 (<= 10)
two orders inside OP_TOL / GRAD_TOL / red_tol, as the GRU's kernels are (tests/test_gpu_gru_seq.py).  No case came near a tolerance
and none found a defect; the whole file takes 5 s.
"""
import functools

import pytest
import torch

import lstm_ref as R
import lstm_seq_cases as LC
from lstm_seq_cases import close
from test_gpu_lstm_seq import ATOL, RTOL
from test_gpu_parity import GRAD_TOL, OP_TOL
from test_gpu_train_kernels import BADARG, SENTINEL, _gen

pytestmark = pytest.mark.gpu

NAN = float("nan")
TAIL = 1024                                   # sentinel floats behind every workspace and behind dG
Y_TOL = dict(rtol=RTOL, atol=ATOL)            # y of lstm_forward_train: the tile GEMM's input projection is in the path
PERSISTENT = ("cvc_lstm_seq_persistent_train_fwd", "cvc_lstm_seq_persistent_fwd")
STEPS = ("cvc_lstm_seq_train_fwd", "cvc_lstm_seq_fwd")


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


@functools.lru_cache(maxsize=2)
def packed(H, dev):
    """W_hh of both directions in the packed gate tiles the forward entries read, on the device"""
    from cvc.lstm_seq import pack_lstm_weights
    w = LC.weights(H)[0]
    return torch.stack([pack_lstm_weights(w[d], H) for d in range(2)]).to(dev)


class Lay:
    """A [M, F, W] operand in device memory: row of (clip m, step t) at m * ld_m + t * ld_t, time-major ("tm": [F][M + extra][W + pad])
    or clip-major ("bm": [M + extra][F][W + pad], as lstm_forward's last layer writes); everything outside the [M, F, W] block -- pad
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


class Work:
    """n floats of workspace, NaN before every call, with TAIL sentinel floats behind them"""

    def __init__(self, dev, n, fill=NAN):
        self.n, self.fill = n, fill
        self.buf = torch.empty(n + TAIL, device=dev, dtype=torch.float32)
        self.poison()

    def poison(self):
        self.buf[:self.n].fill_(self.fill)
        self.buf[self.n:].fill_(SENTINEL)

    def ptr(self):
        return self.buf.data_ptr()

    def tail_intact(self):
        return bool((self.buf[self.n:] == SENTINEL).all())


FWD_BASE = ["wp", "gi", "gi_ld_m", "gi_ld_t", "b_ih", "b_hh", "M", "F", "H", "ndir", "hq", "y", "y_ld_m", "y_ld_t"]
FWD_SAVED = ["gates", "g_ld_m", "g_ld_t", "c", "c_ld_m", "c_ld_t"]
FWD_FORMS = STEPS + PERSISTENT


class Fwd:
    """One case's device operands for the four forward entry points; outputs pre-filled with SENTINEL, gi's padding with NaN."""

    def __init__(self, L, dev, o, layout="tm", pad=0, extra=0):
        H, M, F, ndir = o.H, o.M, o.F, o.ndir
        self.L, self.o = L, o
        self.gi = Lay(dev, M, F, ndir * 4 * H, NAN, o.gi, layout, pad, extra)
        self.y = Lay(dev, M, F, ndir * H, SENTINEL, None, layout, pad, extra)
        self.gates = Lay(dev, M, F, ndir * 4 * H, SENTINEL, None, layout, pad, extra)
        self.c = Lay(dev, M, F, ndir * H, SENTINEL, None, layout, pad, extra)
        self.wp = packed(H, dev)[:ndir]
        self.b_ih, self.b_hh = o.b_ih.to(dev), o.b_hh.to(dev)
        # the sizes cvc/lstm_seq.py allocates: per-step 3 * ndir * Kp * 64, persistent (F + 1) * ndir * H * 64
        self.hq = Work(dev, 3 * ndir * LC.kp(H) * 64)
        self.persistent_ok = H % 128 == 0 and H <= 1024
        if self.persistent_ok:
            self.slots = Work(dev, (F + 1) * ndir * H * 64)
        self.sync = torch.zeros(int(L.cvc_lstm_persistent_sync_words()), dtype=torch.int32, device=dev)

    def call(self, name, **over):
        ws = self.slots if "persistent" in name else self.hq
        a = dict(wp=self.wp.data_ptr(), gi=self.gi.ptr(), gi_ld_m=self.gi.ld_m, gi_ld_t=self.gi.ld_t, b_ih=self.b_ih.data_ptr(),
                 b_hh=self.b_hh.data_ptr(), M=self.o.M, F=self.o.F, H=self.o.H, ndir=self.o.ndir, hq=ws.ptr(), y=self.y.ptr(),
                 y_ld_m=self.y.ld_m, y_ld_t=self.y.ld_t, gates=self.gates.ptr(), g_ld_m=self.gates.ld_m, g_ld_t=self.gates.ld_t,
                 c=self.c.ptr(), c_ld_m=self.c.ld_m, c_ld_t=self.c.ld_t, sync=self.sync.data_ptr())
        assert set(over) <= set(a), over
        a.update(over)
        L, st = self.L, _stream()
        if name == "cvc_lstm_seq_fwd":
            return L.cvc_lstm_seq_fwd(*[a[k] for k in FWD_BASE], st)
        if name == "cvc_lstm_seq_train_fwd":
            return L.cvc_lstm_seq_train_fwd(*[a[k] for k in FWD_BASE + FWD_SAVED], st)
        if name == "cvc_lstm_seq_persistent_fwd":
            return L.cvc_lstm_seq_persistent_fwd(*[a[k] for k in FWD_BASE], a["sync"], st)
        assert name == "cvc_lstm_seq_persistent_train_fwd", name
        return L.cvc_lstm_seq_persistent_train_fwd(*[a[k] for k in FWD_BASE + FWD_SAVED], a["sync"], st)

    def run(self, name):
        """-> (y, gates or None, c or None) as [M, F, .] copies; a persistent form must launch and leave its error word clear (it is
        not retried)"""
        o = self.o
        for t in (self.y, self.gates, self.c):
            t.buf.fill_(SENTINEL)
        ws = self.slots if "persistent" in name else self.hq
        ws.poison()
        self.sync.zero_()
        assert self.call(name) == 0, name
        torch.cuda.synchronize()
        if "persistent" in name:
            assert int(self.sync[4]) == 0, "%s: barrier time-out word set, lstm_persistent_kernel<%d, %d, %d> at H=%d M=%d" % (
                (name,) + LC.instantiation(o.H, o.M) + (o.H, o.M))
        assert ws.tail_intact(), name + " wrote behind its workspace"
        train = "train" in name
        return self.y.get().clone(), (self.gates.get().clone() if train else None), (self.c.get().clone() if train else None)

    def padding_untouched(self):
        return all(t.outside_untouched() for t in (self.gi, self.y, self.gates, self.c))


def check_forward(f, names, tag):
    """the training entry against fp64 (y, the four gate planes and c of every direction); the inference entry bit-equal to it (one
    kernel, the stores of gates and c gated on a null pointer) and writing neither gates nor c; a second run of either entry
    bit-equal to the first; all padding as it was"""
    train, infer = names
    y, gates, c = f.run(train)
    assert f.padding_untouched(), tag + ": the training entry wrote padding"
    LC.check_forward_results(f.o, y, gates, c, tag)
    y2, gates2, c2 = f.run(train)
    assert torch.equal(y, y2) and torch.equal(gates, gates2) and torch.equal(c, c2), tag + ": a second run gives other bits"
    yi, _, _ = f.run(infer)
    assert f.gates.untouched() and f.c.untouched(), tag + ": the inference entry wrote gates or c"
    assert f.padding_untouched(), tag + ": the inference entry wrote padding"
    assert torch.equal(y, yi), tag + ": training and inference entry differ"
    assert torch.equal(yi, f.run(infer)[0]), tag + ": a second run of the inference entry gives other bits"
    return y, gates, c


# ------------------------------------------------------------------------------------------------ A: persistent forward
@pytest.mark.parametrize("case", LC.A_CASES, ids=LC.a_id)
def test_persistent_forward_every_instantiation_vs_fp64(dev, L, case):
    """lstm_persistent_kernel<MT, NC, NW>: NC 1..4 at 8 waves (H % 256 == 0), NC 1, 3, 5, 7 at 4 waves, each at MT 1 (32 clips) and
    MT 2 (33 clips); then 1 and 64 clips, one step, one direction"""
    check_forward(Fwd(L, dev, LC.ops(*case)), PERSISTENT, "persistent " + LC.a_id(case))


# ------------------------------------------------------------------------------------------------ B: per-step forward
@pytest.mark.parametrize("case", LC.B_CASES, ids=LC.case_id)
def test_per_step_forward_vs_fp64(dev, L, case):
    """lstm_step_kernel<1> / <2>: Kp > H at 8, 40, 72, 200 (the k padding of h and of the packed tiles), a single k chunk at 8,
    config 5's width"""
    check_forward(Fwd(L, dev, LC.ops(*case)), STEPS, "per-step %s tile %d" % (LC.case_id(case), LC.step_tile(case[1])))


# ------------------------------------------------------------------------------------------------ C: the forms from each other
@pytest.mark.parametrize("case", LC.D_PERSISTENT, ids=LC.a_id)
def test_per_step_and_persistent_forward_agree(dev, L, case):
    """the two forms sum k in different orders: y, gates and c within OP_TOL of each other"""
    f = Fwd(L, dev, LC.ops(*case))
    ys, gs, cs = f.run(STEPS[0])
    yp, gp, cp = f.run(PERSISTENT[0])
    close(ys, yp, "per-step vs persistent y " + LC.a_id(case), OP_TOL)
    close(gs, gp, "per-step vs persistent gates " + LC.a_id(case), OP_TOL)
    close(cs, cp, "per-step vs persistent c " + LC.a_id(case), OP_TOL)


# ------------------------------------------------------------------------------------------------ D: layouts
@pytest.mark.parametrize("layout,pad", LC.LAYOUTS, ids=["%s-pad%d" % lp for lp in LC.LAYOUTS])
@pytest.mark.parametrize("case,names", [(c, PERSISTENT) for c in LC.D_PERSISTENT] + [(c, STEPS) for c in LC.D_STEPS],
                         ids=["persistent-" + LC.case_id(c) for c in LC.D_PERSISTENT] + ["steps-" + LC.case_id(c) for c in LC.D_STEPS])
def test_forward_layouts_and_padding(dev, L, case, names, layout, pad):
    """time-major rows with leading dimensions `pad` floats wider than the used columns and one clip row more than M (ld_t > M ld_m),
    and clip-major rows (ld_t = width, ld_m = F width): the bits of the dense time-major call; NaN in gi's padding reaches nothing;
    the padding of y, gates and c keeps the sentinel"""
    o = LC.ops(*case)
    y0, g0, c0 = Fwd(L, dev, o).run(names[0])
    f = Fwd(L, dev, o, layout, pad, 1)
    if layout == "bm":
        assert (f.gi.ld_t, f.gi.ld_m) == (o.ndir * 4 * o.H, o.F * o.ndir * 4 * o.H)
    else:
        assert f.y.ld_m == o.ndir * o.H + pad and f.y.ld_t > o.M * f.y.ld_m
    y, gates, c = check_forward(f, names, "%s %s %s pad %d" % (names[0], LC.case_id(case), layout, pad))
    assert torch.equal(y, y0) and torch.equal(gates, g0) and torch.equal(c, c0)


# ------------------------------------------------------------------------------------------------ E: backward
BWD_ARGS = ["dy", "dy_ld_m", "dy_ld_t", "gates", "g_ld_m", "g_ld_t", "c", "c_ld_m", "c_ld_t", "w_hh", "M", "F", "H", "ndir", "dg", "work"]


class Bwd:
    """One case's device operands for cvc_lstm_seq_bwd: dy random, gates / c the fp64 reference's rounded to fp32, their padding NaN;
    work (cvc_lstm_seq_bwd_work floats) NaN beforehand; dG pre-filled with SENTINEL, tail included."""

    def __init__(self, L, dev, o, layout="tm", pad=0, extra=0):
        H, M, F, ndir = o.H, o.M, o.F, o.ndir
        self.L, self.o = L, o
        self.dy = Lay(dev, M, F, ndir * H, NAN, o.dy, layout, pad, extra)
        self.gates = Lay(dev, M, F, ndir * 4 * H, NAN, o.gates, layout, pad, extra)
        self.c = Lay(dev, M, F, ndir * H, NAN, o.c, layout, pad, extra)
        self.w_hh = o.w_hh.to(dev)
        self.dg = Work(dev, F * M * ndir * 4 * H, SENTINEL)
        n = int(L.cvc_lstm_seq_bwd_work(M, H, ndir))
        assert n == LC.bwd_work_floats(M, H, ndir), (n, LC.bwd_work_floats(M, H, ndir))
        self.work = Work(dev, n)

    def call(self, **over):
        a = dict(dy=self.dy.ptr(), dy_ld_m=self.dy.ld_m, dy_ld_t=self.dy.ld_t, gates=self.gates.ptr(), g_ld_m=self.gates.ld_m,
                 g_ld_t=self.gates.ld_t, c=self.c.ptr(), c_ld_m=self.c.ld_m, c_ld_t=self.c.ld_t, w_hh=self.w_hh.data_ptr(), M=self.o.M,
                 F=self.o.F, H=self.o.H, ndir=self.o.ndir, dg=self.dg.ptr(), work=self.work.ptr())
        assert set(over) <= set(a), over
        a.update(over)
        return self.L.cvc_lstm_seq_bwd(*[a[k] for k in BWD_ARGS], _stream())

    def run(self):
        """-> dG as a [M, F, ndir * 4H] copy"""
        o = self.o
        self.dg.poison()
        self.work.poison()
        assert self.call() == 0
        torch.cuda.synchronize()
        assert self.work.tail_intact(), "cvc_lstm_seq_bwd wrote behind its workspace"
        assert self.dg.tail_intact(), "cvc_lstm_seq_bwd wrote behind dG"
        assert self.dy.outside_untouched() and self.gates.outside_untouched() and self.c.outside_untouched()
        return self.dg.buf[:self.dg.n].view(o.F, o.M, -1).transpose(0, 1).clone()              # rows (t * M + m) -> [M, F, .]


def check_backward(b, tag):
    dg = b.run()
    LC.check_dg(b.o, dg, tag)
    assert torch.equal(dg, b.run()), tag + ": a second run gives other bits"
    return dg


@pytest.mark.parametrize("case", LC.E_CASES, ids=["%s-ksplit%d" % (LC.case_id(c), LC.bwd_ksplit(c[0])) for c in LC.E_CASES])
def test_backward_vs_fp64(dev, L, case):
    """cvc_lstm_seq_bwd from the reference's saved tensors: dG of every direction, every K-split count of the backward-data product,
    plane rows longer than H at 8, 40, 200; F = 1 has no c_prev and no carried planes at all, with F >= 2 the first and the last
    time step are each one direction's first processed step (checked on their own too)"""
    H = case[0]
    check_backward(Bwd(L, dev, LC.ops(*case)), "bwd %s ksplit %d ntot %d" % (LC.case_id(case), LC.bwd_ksplit(H), LC.bwd_ntot(H)))


@pytest.mark.parametrize("layout,pad", LC.LAYOUTS, ids=["%s-pad%d" % lp for lp in LC.LAYOUTS])
@pytest.mark.parametrize("case", LC.D_BWD, ids=LC.case_id)
def test_backward_layouts_and_padding(dev, L, case, layout, pad):
    """dy, gates and c in the padded and in the clip-major layout, their padding NaN: the bits of the dense call (dG has no stride)"""
    o = LC.ops(*case)
    dg0 = Bwd(L, dev, o).run()
    dg = check_backward(Bwd(L, dev, o, layout, pad, 1), "bwd %s %s pad %d" % (LC.case_id(case), layout, pad))
    assert torch.equal(dg, dg0)


# ------------------------------------------------------------------------------------------------ F: refusals
def test_sync_word_query(L):
    """the error word is word 4: the buffer the query sizes must hold it"""
    assert int(L.cvc_lstm_persistent_sync_words()) > 4


def test_bwd_work_refuses_arguments_outside_the_contract(L):
    for M, H, ndir in [(0, 128, 2), (65, 128, 2), (8, 4, 2), (8, 12, 2), (8, 128, 0), (8, 128, 3)]:
        assert int(L.cvc_lstm_seq_bwd_work(M, H, ndir)) == BADARG, (M, H, ndir)
    for H, M, ndir in [(8, 1, 1), (200, 37, 2), (2048, 64, 2)]:
        assert int(L.cvc_lstm_seq_bwd_work(M, H, ndir)) == LC.bwd_work_floats(M, H, ndir)


@pytest.mark.parametrize("name", FWD_FORMS)
def test_forward_entry_points_refuse_arguments_outside_the_contract(dev, L, name):
    """CVC_E_BADARG, and nothing launched: y, gates and c keep their sentinel"""
    persistent, train = "persistent" in name, "train" in name
    o = LC.ops(256, 8, 2, 2)
    f = Fwd(L, dev, o)
    # buffers large enough for every refused shape below (M = 65, ndir = 3, H up to 1152), at the valid case's strides
    Hx, room = 1152, 65 * 2 * 3
    zeros = lambda n: torch.zeros(n, device=dev)
    ins = dict(wp=zeros(3 * 4 * Hx * Hx), gi=zeros(room * 4 * Hx), b_ih=zeros(12 * Hx), b_hh=zeros(12 * Hx), hq=zeros(3 * 3 * Hx * 64))
    keep = dict(y=torch.full((room * Hx,), SENTINEL, device=dev), gates=torch.full((room * 4 * Hx,), SENTINEL, device=dev),
                c=torch.full((room * Hx,), SENTINEL, device=dev))
    over_ok = {k: t.data_ptr() for k, t in list(ins.items()) + list(keep.items())}
    pointers = ["wp", "gi", "b_ih", "b_hh", "hq", "y"] + (["gates", "c"] if train else [])
    strides = ["gi_ld_m", "gi_ld_t", "y_ld_m", "y_ld_t"] + (["g_ld_m", "g_ld_t", "c_ld_m", "c_ld_t"] if train else [])
    lds = dict(gi_ld_m=f.gi.ld_m, gi_ld_t=f.gi.ld_t, y_ld_m=f.y.ld_m, y_ld_t=f.y.ld_t, g_ld_m=f.gates.ld_m, g_ld_t=f.gates.ld_t,
               c_ld_m=f.c.ld_m, c_ld_t=f.c.ld_t)
    bad = [dict(H=4), dict(H=12), dict(M=0), dict(M=65), dict(F=0), dict(ndir=0), dict(ndir=3)]
    bad += [{k: lds[k] + off} for k in strides for off in (1, 2)]                  # no multiple of 4 floats
    bad += [{k: over_ok[k] + 4} for k in pointers]                                 # 4 bytes past a 16-byte boundary
    bad += [{k: None} for k in pointers]
    if persistent:
        bad += [dict(H=64), dict(H=136), dict(H=1152), dict(sync=None)]
    for kw in bad:
        args = dict(over_ok)
        args.update(kw)
        assert f.call(name, **args) == BADARG, "%s accepted %r" % (name, kw)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in keep.values()), name + " launched on a refused call"
    assert f.y.untouched() and f.gates.untouched() and f.c.untouched(), name + " launched on a refused call"
    y, _, _ = f.run(name)                              # the same operands inside the contract run
    close(y, o.y, name + " y", OP_TOL)


def test_backward_entry_point_refuses_arguments_outside_the_contract(dev, L):
    """CVC_E_BADARG, and nothing launched: dG keeps its sentinel"""
    o = LC.ops(256, 8, 2, 2)
    b = Bwd(L, dev, o)
    Hx, room = 1152, 65 * 2 * 3
    zeros = lambda n: torch.zeros(n, device=dev)
    ins = dict(dy=zeros(room * Hx), gates=zeros(room * 4 * Hx), c=zeros(room * Hx), w_hh=zeros(3 * 4 * Hx * Hx),
               work=zeros(3 * (65 * Hx + 256 * Hx + 32 * 65 * Hx)))
    keep = torch.full((room * 4 * Hx,), SENTINEL, device=dev)
    over_ok = {k: t.data_ptr() for k, t in ins.items()}
    over_ok["dg"] = keep.data_ptr()
    pointers = ["dy", "gates", "c", "w_hh", "dg", "work"]
    lds = dict(dy_ld_m=b.dy.ld_m, dy_ld_t=b.dy.ld_t, g_ld_m=b.gates.ld_m, g_ld_t=b.gates.ld_t, c_ld_m=b.c.ld_m, c_ld_t=b.c.ld_t)
    bad = [dict(H=4), dict(H=12), dict(M=0), dict(M=65), dict(F=0), dict(ndir=0), dict(ndir=3)]
    bad += [{k: v + off} for k, v in lds.items() for off in (1, 2)]
    bad += [{k: over_ok[k] + 4} for k in pointers]
    bad += [{k: None} for k in pointers]
    for kw in bad:
        args = dict(over_ok)
        args.update(kw)
        assert b.call(**args) == BADARG, "cvc_lstm_seq_bwd accepted %r" % (kw,)
    torch.cuda.synchronize()
    assert bool((keep == SENTINEL).all()) and bool((b.dg.buf == SENTINEL).all()), "cvc_lstm_seq_bwd launched on a refused call"
    LC.check_dg(o, b.run(), "cvc_lstm_seq_bwd after the refusals")     # the same operands inside the contract run


# ------------------------------------------------------------------------------------------------ G: through autograd
def want_form(H):
    return "persistent" if (H % 128 == 0 and H <= 1024) else "steps"


def check_autograd(ld, x, probe, want_y, want_dx, want, tag, form):
    """one forward + backward of cvc.lstm_seq.lstm_forward_train against the reference, element-wise"""
    from cvc import lstm_seq as LS
    B, F, _ = x.shape
    for p in ld.parameters():
        p.grad = None
    xg = x.cuda().requires_grad_(True)
    assert LS.supported_train(ld, xg)
    y = LS.lstm_forward_train(ld, xg)
    assert LS.last_train_form == form, LS.last_train_form
    close(y, want_y, tag + " y", Y_TOL)
    (y * probe.cuda()).sum().backward()
    close(xg.grad, want_dx, tag + " dx", GRAD_TOL)
    for k, p in ld.named_parameters():
        assert p.grad is not None, k
    LC.check_param_grads({k: p.grad for k, p in ld.named_parameters()}, want, F * B, tag)


@pytest.mark.parametrize("B,F,inp,H,layers,bidir", LC.G_CASES)
def test_lstm_forward_train_elementwise_vs_fp64(dev, B, F, inp, H, layers, bidir):
    """tile-GEMM input projections + recurrence + cvc_lstm_seq_bwd + dense dW / dX products: output, input gradient and every
    parameter gradient element-wise, in the form the shape selects and, where that is the persistent one, once more per step"""
    from cvc import lstm_seq as LS
    lstm = R.make_lstm(inp, H, layers, bidir, 11, scale=1.5)
    g = _gen("lstm autograd", B, F, inp, H, layers, bidir)
    x, probe = torch.randn(B, F, inp, generator=g), torch.randn(B, F, (2 if bidir else 1) * H, generator=g)
    params = {k: v.detach().clone() for k, v in lstm.named_parameters()}
    want_y, saved = R.lstm_forward(x, params, layers, bidir)
    want_dx, want = R.lstm_backward(probe, saved, params, layers, bidir)
    ld = lstm.to(dev)
    tag = "autograd B=%d F=%d H=%d layers=%d ndir=%d" % (B, F, H, layers, 2 if bidir else 1)
    check_autograd(ld, x, probe, want_y, want_dx, want, tag, want_form(H))
    if want_form(H) == "persistent":
        LS.PERSISTENT = False
        try:
            check_autograd(ld, x, probe, want_y, want_dx, want, tag + " (per-step forward)", "steps")
        finally:
            LS.PERSISTENT = True


def test_lstm_train_mode_dropout_elementwise_vs_fp64(dev):
    """train() with dropout 0.2 between three layers: output and every gradient equal the fp64 reference under the kernels' own masks
    (sites enc.lstm.<l>) restated on the host, element-wise"""
    from cvc import dropout, lstm_seq as LS
    B, F, inp, H, layers = 6, 5, 32, 128, 3
    lstm = R.make_lstm(inp, H, layers, True, 17, dropout=0.2, scale=1.5)
    g = _gen("lstm dropout", B, F, inp, H)
    x, probe = torch.randn(B, F, inp, generator=g), torch.randn(B, F, 2 * H, generator=g)
    params = {k: v.detach().clone() for k, v in lstm.named_parameters()}
    ld = lstm.to(dev).train()
    dropout.seed(123)
    xg = x.cuda().requires_grad_(True)
    y = LS.lstm_forward_train(ld, xg)
    (y * probe.cuda()).sum().backward()
    # the masks act on time-major rows (t, clip): [F * B, 2H] -> [B, F, 2H]
    masks = [dropout.host_mask("enc.lstm.%d" % l, (F * B, 2 * H), 0.2, dev).view(F, B, 2 * H).transpose(0, 1).double().cpu()
             for l in range(layers - 1)]
    assert all(0 < float((m == 0).double().mean()) < 0.5 for m in masks)
    want_y, saved = R.lstm_forward(x, params, layers, True, masks)
    want_dx, want = R.lstm_backward(probe, saved, params, layers, True, masks)
    tag = "dropout H=%d" % H
    close(y, want_y, tag + " y", Y_TOL)
    close(xg.grad, want_dx, tag + " dx", GRAD_TOL)
    LC.check_param_grads({k: p.grad for k, p in ld.named_parameters()}, want, F * B, tag)
