"""Element-wise tests of the training step's backward kernels (pytest -m gpu), each called by name through the C-ABI and compared
with fp64 autograd in torch of the operation it implements (the kernel's fp32 result cast to fp64 first):

  A. cvc_lstm_pointwise_bwd4 / cvc_lstm_pointwise_bwd4_pair  -- the gate gradients of the C-driven training loops
  B. cvc_attn_bwd_pair                                        -- the attention backward over both feature sets
  C. cvc_vocab_head_nll_fwd / cvc_scale_by_scalar             -- the vocabulary head's fused criterion and its backward
     (+ the unfused log_softmax / masked NLL path the captioner still uses)
  D. cvc_bn_relu_train_fwd/_bwd, cvc_layernorm_cat_bwd, cvc_class_softmax_bwd, cvc_relu_dropout_fwd/_bwd -- the encoder's
     train-mode pieces

Tolerances are test_gpu_parity.py's (OP_TOL on single-op outputs, GRAD_TOL on gradients); a reduction of length L gets its
atol grown as sqrt(L) (the random-walk growth of an fp32 sum's rounding error, `red_tol`).  Every kernel is also run twice on
the same inputs and must give the same bits: the captured training graph replays them and relies on that.

The CPU cross-checks of the references themselves (e.g. the gate-gradient reference against nn.LSTMCell autograd) live in
tests/test_train_kernel_refs.py.
"""
import ctypes as C
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import GRAD_TOL, OP_TOL

pytestmark = pytest.mark.gpu

BADARG = -1
SENTINEL = -777.0


def red_tol(L, base=GRAD_TOL):
    """`base`, with atol grown as sqrt(L / 64): the rounding error of a length-L fp32 sum walks like sqrt(L)"""
    return dict(rtol=base["rtol"], atol=base["atol"] * max(1.0, math.sqrt(L / 64.0)))


def close(a, b, **tol):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    np.testing.assert_allclose(a, b, **tol)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    from cvc import hip
    return hip.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    from cvc import hip
    return hip._stream()


def _gen(*key):
    """a CPU generator seeded from the case's parameters (stable across processes, unlike hash())"""
    return torch.Generator(device="cpu").manual_seed(zlib.crc32(repr(key).encode()))


def _misaligned(t):
    """a copy of t whose data pointer is one float past a 16-byte boundary (forces the kernels' scalar forms)"""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


# ================================================================================================ A. gate gradients
def lstm_gates_bwd_ref(z, c_prev, dh, dc):
    """fp64 autograd of one nn.LSTMCell update given its pre-activations z [M, 4R] (gate order i, f, g, o): the gradients with
    respect to z and c_prev of <h', dh> + <c', dc>, h' = o * tanh(c'), c' = f * c_prev + i * g"""
    z = z.detach().double().requires_grad_(True)
    cp = c_prev.detach().double().requires_grad_(True)
    R = cp.shape[1]
    i, f = torch.sigmoid(z[:, :R]), torch.sigmoid(z[:, R:2 * R])
    g, o = torch.tanh(z[:, 2 * R:3 * R]), torch.sigmoid(z[:, 3 * R:])
    c = f * cp + i * g
    h = o * torch.tanh(c)
    dz, dcp = torch.autograd.grad([h, c], [z, cp], [dh.double(), dc.double()])
    return dz, dcp


def lstm_cell_state(z, c_prev):
    """(activated gates [M, 4R], c' [M, R]) in fp64"""
    R = c_prev.shape[1]
    gates = torch.cat([torch.sigmoid(z[:, :2 * R]), torch.tanh(z[:, 2 * R:3 * R]), torch.sigmoid(z[:, 3 * R:])], 1)
    c = gates[:, R:2 * R] * c_prev + gates[:, :R] * gates[:, 2 * R:3 * R]
    return gates, c


class PwCase:
    """inputs of one gate-gradient launch: three gradient sources of h' as K-slice planes (None = NULL source), d_hd under the
    dropout mask of `site`, d_c; planes are [nplanes + 1, M, ld] with the extra plane and the columns past R poisoned with NaN,
    so a kernel that reads a plane or a column too many fails the comparison"""

    def __init__(self, dev, M, R, planes=(1, None, None), ld=None, p=0.0, site="out_a.3", d_hd=True, d_c=True, seed=0):
        from cvc import dropout
        gen = _gen("pw", M, R, planes, ld, p, site, d_hd, d_c, seed)
        ld = ld or R
        self.M, self.R, self.p, self.site = M, R, p, site
        self.z = torch.randn(M, 4 * R, generator=gen, dtype=torch.float64) * 1.5
        self.c_prev64 = torch.randn(M, R, generator=gen, dtype=torch.float64)
        gates, c_new = lstm_cell_state(self.z, self.c_prev64)
        self.gates, self.c_prev, self.c_new = (t.float().to(dev) for t in (gates, self.c_prev64, c_new))
        self.srcs = []
        dh = torch.zeros(M, R, dtype=torch.float64)
        for n in planes:
            if n is None:
                self.srcs.append(None)
                continue
            buf = torch.randn(n + 1, M, ld, generator=gen)
            dh += buf[:n, :, :R].double().sum(0)
            buf[n] = float("nan")
            buf[:, :, R:] = float("nan")
            self.srcs.append((buf.to(dev), n, ld))
        self.d_hd = torch.randn(M, R, generator=gen).to(dev) if d_hd else None
        self.site_id = dropout.site_id(site)
        self.state = dropout.rng_state(dev) if p > 0 else None
        if d_hd:
            mask = dropout.host_mask(site, (M, R), p, dev) if p > 0 else torch.ones(M, R)
            dh += self.d_hd.cpu().double() * mask.double()
        self.dh64 = dh
        self.d_c = torch.randn(M, R, generator=gen).to(dev) if d_c else None
        self.dc64 = self.d_c.cpu().double() if d_c else torch.zeros(M, R, dtype=torch.float64)

    def grad_srcs(self):
        from cvc import hip
        arr = (hip.GradSrc * 3)()
        for k, s in enumerate(self.srcs):
            if s is not None:
                buf, n, ld = s
                arr[k] = hip.GradSrc(buf.data_ptr(), ld, self.M * ld, n)
        return arr

    def ref(self):
        return lstm_gates_bwd_ref(self.z, self.c_prev64, self.dh64, self.dc64)

    def outputs(self, dev, quad=False, dg_sum=None):
        M, R = self.M, self.R
        o = dict(d_gates=torch.full((M, 4 * R), SENTINEL, device=dev), d_c_prev=torch.full((M, R), SENTINEL, device=dev),
                 d_gates_q=torch.full((R, 64, 4), SENTINEL, device=dev) if quad else None, dg_sum=dg_sum)
        return o

    def args(self, o, q_row0=0):
        """cvc_pw_bwd_args for the pair launch"""
        from cvc import hip
        a = hip.PwBwdArgs()
        a.d_h = self.grad_srcs()
        a.d_hd, a.rng_state, a.site, a.p = _ptr(self.d_hd), _ptr(self.state), self.site_id, self.p
        a.d_c, a.gates, a.c_prev, a.c_new, a.M = _ptr(self.d_c), _ptr(self.gates), _ptr(self.c_prev), _ptr(self.c_new), self.M
        a.d_gates, a.d_c_prev, a.d_gates_q, a.dg_sum = _ptr(o["d_gates"]), _ptr(o["d_c_prev"]), _ptr(o["d_gates_q"]), _ptr(o["dg_sum"])
        a.q_row0 = q_row0
        return a

    def launch(self, L, o, q_row0=0, gates=None, c_prev=None, c_new=None):
        return L.cvc_lstm_pointwise_bwd4(self.grad_srcs(), _ptr(self.d_hd), _ptr(self.state), self.site_id, self.p, _ptr(self.d_c),
                                         _ptr(self.gates if gates is None else gates), _ptr(self.c_prev if c_prev is None else c_prev),
                                         _ptr(self.c_new if c_new is None else c_new), self.M, self.R, _ptr(o["d_gates"]),
                                         _ptr(o["d_c_prev"]), _ptr(o["d_gates_q"]), _ptr(o["dg_sum"]), q_row0, _stream())


def quad_rows(q, R):
    """the [R][64][4] quad layout of a [rows <= 64, 4R] operand decoded back to [64, 4R]"""
    return q.view(R, 64, 4).permute(1, 0, 2).reshape(64, 4 * R)


def check_quad(q, R, *placed):
    """placed: (q_row0, d_gates) of every launch that wrote into q; every other row still holds the sentinel"""
    rows = quad_rows(q, R)
    free = torch.ones(64, dtype=torch.bool, device=q.device)
    for q_row0, d_gates in placed:
        assert torch.equal(rows[q_row0:q_row0 + d_gates.shape[0]], d_gates)
        free[q_row0:q_row0 + d_gates.shape[0]] = False
    assert bool((rows[free] == SENTINEL).all())


# (planes of the three sources, ld - R, dropout p, d_hd given, d_c given): every source as planes, NULL sources, ld > R (aligned:
# vector form; ld - R odd: scalar form), no d_hd / d_c
PW_SOURCES = [((1, 2, 4), 0, 0.0, True, True), ((5, 7, 8), 4, 0.3, True, False), ((None, 5, None), 1, 0.3, True, True),
              ((None, None, None), 0, 0.3, True, True), ((6, None, 1), 8, 0.0, False, True)]


@pytest.mark.parametrize("R", [4, 130, 2048])
@pytest.mark.parametrize("M", [1, 37, 64])
def test_lstm_pointwise_bwd4_vs_fp64(dev, L, M, R):
    """cvc_lstm_pointwise_bwd4: d_gates, d_c_prev (and d_gates_q at q_row0 0 / 13, the rows around it untouched) against fp64
    autograd of the cell update, the upstream dh being the three plane-summed sources + d_hd * dropout mask"""
    for k, (planes, pad, p, hd, dc) in enumerate(PW_SOURCES):
        case = PwCase(dev, M, R, planes, R + pad, p, "out_a.%d" % k, hd, dc, seed=k)
        quad = R % 4 == 0
        q_row0 = 13 if (quad and M + 13 <= 64 and k % 2 == 0) else 0
        o = case.outputs(dev, quad)
        assert case.launch(L, o, q_row0) == 0
        o2 = case.outputs(dev, quad)
        assert case.launch(L, o2, q_row0) == 0
        dz, dcp = case.ref()
        close(o["d_gates"], dz, **GRAD_TOL)
        close(o["d_c_prev"], dcp, **GRAD_TOL)
        assert torch.equal(o["d_gates"], o2["d_gates"]) and torch.equal(o["d_c_prev"], o2["d_c_prev"])      # same bits re-run
        if quad:
            check_quad(o["d_gates_q"], R, (q_row0, o["d_gates"]))
            assert torch.equal(o["d_gates_q"], o2["d_gates_q"])


def test_lstm_pointwise_bwd4_dg_sum_accumulates(dev, L):
    """dg_sum += d_gates over three successive launches (the loop's bias / fc_feats gradient): the launches' own d_gates summed in
    launch order, bit for bit, and the fp64 sum of the three steps' gate gradients"""
    M, R = 37, 256
    dg = torch.zeros(M, 4 * R, device=dev)
    own, refs = [], []
    for t in range(3):
        case = PwCase(dev, M, R, (5, 1, None), R, 0.3, "out_c.%d" % t, seed=10 + t)
        o = case.outputs(dev, dg_sum=dg)
        assert case.launch(L, o) == 0
        own.append(o["d_gates"].clone())
        refs.append(case.ref()[0])
    assert torch.equal(dg, ((torch.zeros_like(dg) + own[0]) + own[1]) + own[2])
    close(dg, refs[0] + refs[1] + refs[2], **GRAD_TOL)


def test_lstm_pointwise_bwd4_vector_and_scalar_forms_agree(dev, L):
    """The vector form (every operand 16-byte aligned) and the scalar form (forced by operands one float off) give the same bits:
    planes 5 / 7 / 8, dropout, dg_sum and d_gates_q at q_row0 = 13"""
    M, R = 37, 2048
    case = PwCase(dev, M, R, (5, 7, 8), R, 0.3, "out_a.7", seed=3)
    outs = []
    for form in ("vector", "scalar"):
        o = case.outputs(dev, quad=True, dg_sum=torch.full((M, 4 * R), 0.5, device=dev))
        if form == "vector":
            assert case.launch(L, o, 13) == 0
        else:
            assert case.launch(L, o, 13, gates=_misaligned(case.gates), c_prev=_misaligned(case.c_prev),
                               c_new=_misaligned(case.c_new)) == 0
        outs.append(o)
    for k in ("d_gates", "d_c_prev", "d_gates_q", "dg_sum"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    check_quad(outs[1]["d_gates_q"], R, (13, outs[1]["d_gates"]))
    close(outs[1]["d_gates"], case.ref()[0], **GRAD_TOL)


def test_lstm_pointwise_bwd4_rejects_bad_quad_rows(dev, L):
    """q_row0 + M > 64 (and a negative q_row0, and R % 4 != 0 with a quad destination) return CVC_E_BADARG and launch nothing"""
    for M, R, q_row0 in ((37, 64, 28), (64, 64, 1), (1, 64, -1), (5, 130, 0)):
        case = PwCase(dev, M, R, (2, None, None), R, seed=4)
        o = case.outputs(dev, quad=True, dg_sum=torch.full((M, 4 * R), SENTINEL, device=dev))
        assert case.launch(L, o, q_row0) == BADARG
        torch.cuda.synchronize()
        for k in ("d_gates", "d_c_prev", "d_gates_q", "dg_sum"):
            assert bool((o[k] == SENTINEL).all()), k


@pytest.mark.parametrize("Ma,Mb,R", [(64, 64, 2048), (64, 37, 256), (1, 64, 132), (27, 37, 512)])
def test_lstm_pointwise_bwd4_pair_equals_two_launches(dev, L, Ma, Mb, R):
    """cvc_lstm_pointwise_bwd4_pair == two cvc_lstm_pointwise_bwd4 launches, bit for bit (two dropout sites, dg_sum, quad rows;
    the second set at q_row0 = Ma of the same quad operand when Ma + Mb <= 64)"""
    from cvc import hip
    a = PwCase(dev, Ma, R, (5, 2, None), R, 0.3, "out_a.1", seed=5)
    b = PwCase(dev, Mb, R, (8, None, 1), R + 4, 0.3, "out_c.1", seed=6)
    joint = Ma + Mb <= 64
    qb_row0 = Ma if joint else 0

    def outs():
        oa = a.outputs(dev, quad=True, dg_sum=torch.full((Ma, 4 * R), 0.25, device=dev))
        ob = b.outputs(dev, quad=not joint, dg_sum=torch.full((Mb, 4 * R), -0.5, device=dev))
        if joint:
            ob["d_gates_q"] = oa["d_gates_q"]
        return oa, ob
    pa, pb = outs()
    assert hip.lib().cvc_lstm_pointwise_bwd4_pair(C.byref(a.args(pa)), C.byref(b.args(pb, qb_row0)), R, _stream()) == 0
    sa, sb = outs()
    assert a.launch(L, sa) == 0 and b.launch(L, sb, qb_row0) == 0
    for k in ("d_gates", "d_c_prev", "d_gates_q", "dg_sum"):
        assert torch.equal(pa[k], sa[k]) and torch.equal(pb[k], sb[k]), k
    close(pa["d_gates"], a.ref()[0], **GRAD_TOL)
    close(pb["d_gates"], b.ref()[0], **GRAD_TOL)
    if joint:
        check_quad(pa["d_gates_q"], R, (0, pa["d_gates"]), (Ma, pb["d_gates"]))
    else:
        check_quad(pa["d_gates_q"], R, (0, pa["d_gates"]))
        check_quad(pb["d_gates_q"], R, (0, pb["d_gates"]))
    # re-run: same bits
    pa2, pb2 = outs()
    assert hip.lib().cvc_lstm_pointwise_bwd4_pair(C.byref(a.args(pa2)), C.byref(b.args(pb2, qb_row0)), R, _stream()) == 0
    for k in ("d_gates", "d_c_prev", "d_gates_q", "dg_sum"):
        assert torch.equal(pa[k], pa2[k]) and torch.equal(pb[k], pb2[k]), k


def test_lstm_pointwise_bwd4_pair_rejects(dev, L):
    """the pair form is vector-only and keeps the quad-row bound: a misaligned operand or q_row0 + M > 64 -> CVC_E_BADARG"""
    from cvc import hip
    a, b = PwCase(dev, 37, 64, seed=7), PwCase(dev, 37, 64, seed=8)
    oa, ob = a.outputs(dev, quad=True), b.outputs(dev, quad=True)
    ob["d_c_prev"] = _misaligned(ob["d_c_prev"])
    assert hip.lib().cvc_lstm_pointwise_bwd4_pair(C.byref(a.args(oa)), C.byref(b.args(ob)), 64, _stream()) == BADARG
    ob = b.outputs(dev, quad=True)
    assert hip.lib().cvc_lstm_pointwise_bwd4_pair(C.byref(a.args(oa)), C.byref(b.args(ob, 28)), 64, _stream()) == BADARG
    torch.cuda.synchronize()
    for o in (oa, ob):
        assert bool((o["d_gates"] == SENTINEL).all()) and bool((o["d_gates_q"] == SENTINEL).all())


# ================================================================================================ B. attention backward pair
def attn_fwd_ref(kind, q, w_a, inv_temp, sets):
    """fp64 forward of cvc_attn_fwd without masks (cvc_hip.h): per set s = w_a . tanh(proj_n + q) (additive) or (proj_n . q) *
    inv_temp (dot), attn = softmax_n(s); the summed context sum_sets attn @ ctx.  q [nclip, nq, A]; sets: (proj [nclip, n, A],
    ctx [nclip, n, R]).  -> (scores per set, attn per set, ctx_sum [nclip, nq, R])"""
    scores, attns, ctx = [], [], 0
    for proj, cf in sets:
        if kind == 0:
            s = torch.einsum("cqna,a->cqn", torch.tanh(proj[:, None, :, :] + q[:, :, None, :]), w_a)
        else:
            s = torch.einsum("cna,cqa->cqn", proj, q) * inv_temp
        a = torch.softmax(s, -1)
        scores.append(s)
        attns.append(a)
        ctx = ctx + torch.einsum("cqn,cnr->cqr", a, cf)
    return scores, attns, ctx


class AttnCase:
    def __init__(self, dev, kind, nclip, nq, ns, A, R, q_planes, dctx_planes=1, seed=0):
        g = _gen("attn", kind, nclip, nq, ns, A, R, q_planes, dctx_planes, seed)
        rows = nclip * nq
        self.kind, self.nclip, self.nq, self.ns, self.A, self.R, self.rows = kind, nclip, nq, ns, A, R, rows
        self.inv_temp = 0.7
        self.q_planes = torch.randn(q_planes, rows, A, generator=g) * 0.4
        self.q_bias = torch.randn(A, generator=g) * 0.2 if q_planes > 1 else None
        q = self.q_planes.double().sum(0) + (self.q_bias.double() if self.q_bias is not None else 0)
        self.q64 = q.view(nclip, nq, A)
        self.w_a64 = (torch.randn(A, generator=g) * 0.5).float().double()
        self.proj64 = [(torch.randn(nclip, n, A, generator=g) * 0.6).float().double() for n in ns]
        self.ctx64 = [torch.randn(nclip, n, R, generator=g).float().double() for n in ns]
        _, attns, _ = attn_fwd_ref(kind, self.q64, self.w_a64, self.inv_temp, list(zip(self.proj64, self.ctx64)))
        self.attn = [a.float().reshape(rows, -1).to(dev) for a in attns]
        # d_ctx: None (the context had no consumer), a finished tensor (1 plane) or k planes [k, rows, R + 4] (padding NaN)
        self.dctx_planes = dctx_planes
        self.d_ctx = None
        if dctx_planes is not None:
            self.dctx_ld = R if dctx_planes == 1 else R + 4
            pl = torch.full((dctx_planes, rows, self.dctx_ld), float("nan"))
            pl[:, :, :R] = torch.randn(dctx_planes, rows, R, generator=g) / math.sqrt(dctx_planes)
            self.dctx_buf = pl
            self.d_ctx = pl[:, :, :R].double().sum(0)
        self.d_fm = [torch.randn(rows, n, generator=g) for n in ns]
        self.dev = dev

    def ref(self, nsets, with_fm):
        """fp64 autograd: gradients of <ctx_sum, d_ctx> + sum_s <scores_s, d_fm_s> (the frame-masked copy's gradient reaches the
        scores unchanged) with respect to the scores, q, w_a, proj and ctx"""
        q = self.q64.clone().requires_grad_(True)
        w = self.w_a64.clone().requires_grad_(True)
        proj = [p.clone().requires_grad_(True) for p in self.proj64[:nsets]]
        cf = [c.clone().requires_grad_(True) for c in self.ctx64[:nsets]]
        scores, _, ctx = attn_fwd_ref(self.kind, q, w, self.inv_temp, list(zip(proj, cf)))
        for s in scores:
            s.retain_grad()
        loss = (ctx * self.d_ctx.view(ctx.shape)).sum() if self.d_ctx is not None else 0
        if with_fm:
            loss = loss + sum((s * fm.double().view(s.shape)).sum() for s, fm in zip(scores, self.d_fm))
        loss.backward()
        return dict(d_scores=[s.grad.reshape(self.rows, -1) for s in scores], d_q=q.grad.reshape(self.rows, -1),
                    d_w=w.grad if self.kind == 0 else None, d_proj=[p.grad for p in proj], d_ctxfeat=[c.grad for c in cf])

    def run(self, nsets, with_fm, want_ctxfeat, quad):
        """one cvc_attn_bwd_pair launch"""
        from cvc import hip
        dev, rows, A, R = self.dev, self.rows, self.A, self.R
        qbuf = self.q_planes.to(dev)
        qsrc = hip.GradSrc(qbuf.data_ptr(), A, rows * A, self.q_planes.shape[0])
        qb = self.q_bias.to(dev) if self.q_bias is not None else None
        w_a = self.w_a64.float().to(dev)
        proj = [p.float().to(dev) for p in self.proj64[:nsets]]
        cf = [c.float().to(dev) for c in self.ctx64[:nsets]]
        fm = [f.to(dev) for f in self.d_fm[:nsets]] if with_fm else [None] * nsets
        d_scores = [torch.full((rows, n), SENTINEL, device=dev) for n in self.ns[:nsets]]
        sets = (hip.AttnSet * nsets)()
        for s in range(nsets):
            sets[s] = hip.AttnSet(proj[s].data_ptr(), cf[s].data_ptr(), None, None, d_scores[s].data_ptr(), _ptr(fm[s]),
                                  self.attn[s].data_ptr(), None, self.ns[s], 0)
        dsrc = None
        if self.dctx_planes is not None:
            pl = self.dctx_buf.to(dev)
            dsrc = C.byref(hip.GradSrc(pl.data_ptr(), self.dctx_ld, rows * self.dctx_ld, self.dctx_planes))
        d_q = torch.full((rows, A), SENTINEL, device=dev)
        d_q_q = torch.full((A // 4, 64, 4), SENTINEL, device=dev) if quad else None
        d_w_part = torch.full((rows, A), SENTINEL, device=dev) if self.kind == 0 else None
        g = _gen("acc", rows, A, R)
        d_proj = [torch.randn(p.shape, generator=g).to(dev) for p in proj]
        d_proj0 = [t.clone() for t in d_proj]
        d_cf = [torch.randn(c.shape, generator=g).to(dev) for c in cf] if want_ctxfeat else None
        d_cf0 = [t.clone() for t in d_cf] if want_ctxfeat else None
        dp_arr = (C.c_void_p * 2)(*[t.data_ptr() for t in d_proj])
        dc_arr = (C.c_void_p * 2)(*[t.data_ptr() for t in d_cf]) if want_ctxfeat else None
        rc = hip.lib().cvc_attn_bwd_pair(self.kind, C.byref(qsrc), _ptr(qb), w_a.data_ptr(), self.inv_temp, sets, nsets, dsrc,
                                         self.nclip, self.nq, A, R, d_q.data_ptr(), _ptr(d_q_q), _ptr(d_w_part), dp_arr, dc_arr,
                                         _stream())
        assert rc == 0
        torch.cuda.synchronize()
        return dict(d_scores=d_scores, d_q=d_q, d_q_q=d_q_q, d_w_part=d_w_part, d_proj=d_proj, d_proj0=d_proj0, d_ctxfeat=d_cf,
                    d_ctxfeat0=d_cf0)


def _check_attn(case, got, ref, nsets, tol_n):
    A, R = case.A, case.R
    for s in range(nsets):
        close(got["d_scores"][s], ref["d_scores"][s], **red_tol(R))
        close(got["d_proj"][s] - got["d_proj0"][s], ref["d_proj"][s], **red_tol(case.nq))
        if got["d_ctxfeat"] is not None:
            close(got["d_ctxfeat"][s] - got["d_ctxfeat0"][s], ref["d_ctxfeat"][s], **red_tol(case.nq))
    close(got["d_q"], ref["d_q"], **red_tol(tol_n))
    if got["d_q_q"] is not None:
        rows = got["d_q_q"].view(A // 4, 64, 4).permute(1, 0, 2).reshape(64, A)
        assert torch.equal(rows[:case.rows], got["d_q"]) and bool((rows[case.rows:] == SENTINEL).all())
    if case.kind == 0:
        close(got["d_w_part"].double().sum(0), ref["d_w"], **red_tol(tol_n * case.rows))


ATTN_SHAPES = [(3, 2, 7, 16, 32), (5, 1, 1, 64, 64), (4, 1, 257, 64, 128), (64, 1, 100, 1024, 2048)]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("nclip,nq,n,A,R", ATTN_SHAPES)
def test_attn_bwd_pair_vs_fp64(dev, L, kind, nclip, nq, n, A, R):
    """cvc_attn_bwd_pair over two sets (and one): d_scores, d_q (+ its quad copy when rows <= 64), d w_a as the row sum of
    d_w_part, d_proj[s] and d_ctxfeat[s] accumulated into (+=) -- q as 1 or 5 planes (+ q_bias), d_ctx as planes (no
    d_ctxfeat) or as a finished tensor (with d_ctxfeat), frame-masked gradients"""
    ns = (n, max(1, n // 2 + 3))
    big = A >= 1024
    variants = [(2, 5, 1, True, True), (2, 1, 3, False, True), (1, 5, 1, True, False)]
    if big:
        variants = variants[:1]           # the config-3 size once
    for nsets, q_planes, dctx, want_cf, with_fm in variants:
        case = AttnCase(dev, kind, nclip, nq, ns, A, R, q_planes, dctx, seed=nsets)
        quad = case.rows <= 64
        got = case.run(nsets, with_fm, want_cf, quad)
        ref = case.ref(nsets, with_fm)
        _check_attn(case, got, ref, nsets, sum(ns[:nsets]))
        again = case.run(nsets, with_fm, want_cf, quad)
        for k in ("d_q", "d_q_q", "d_w_part"):
            if got[k] is not None:
                assert torch.equal(got[k], again[k]), k
        for k in ("d_scores", "d_proj", "d_ctxfeat"):
            if got[k] is not None:
                assert all(torch.equal(x, y) for x, y in zip(got[k], again[k])), k


@pytest.mark.parametrize("kind", [0, 1])
def test_attn_bwd_pair_frame_mask_only(dev, L, kind):
    """no d_ctx (the context was not used downstream): the gradient reaches the scores only through the frame-masked copy"""
    case = AttnCase(dev, kind, 4, 1, (9, 6), 32, 16, 1, None, seed=9)
    got = case.run(2, True, False, True)
    ref = case.ref(2, True)
    _check_attn(case, got, ref, 2, 15)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("nclip,nq,n,A,R", ATTN_SHAPES[:3])
def test_attn_bwd_pair_one_set_equals_attn_bwd(dev, L, kind, nclip, nq, n, A, R):
    """with one set, cvc_attn_bwd_pair == cvc_attn_bwd (within GRAD_TOL: the pair sums q's planes, the single form takes q whole)"""
    from cvc import hip
    case = AttnCase(dev, kind, nclip, nq, (n, 1), A, R, 1, 1, seed=11)
    got = case.run(1, True, True, case.rows <= 64)
    q = case.q64.float().reshape(case.rows, A).to(dev)
    proj, cf = case.proj64[0].float().to(dev), case.ctx64[0].float().to(dev)
    ds, dq, dw, dp, dcf = hip.attn_bwd(kind, q, case.w_a64.float().to(dev), case.inv_temp, proj, cf, case.attn[0],
                                       case.d_ctx.float().to(dev), case.d_fm[0].to(dev), nclip, nq, True, True, kind == 0)
    close(got["d_scores"][0], ds, **GRAD_TOL)
    close(got["d_q"], dq, **GRAD_TOL)
    close(got["d_proj"][0] - got["d_proj0"][0], dp, **GRAD_TOL)
    close(got["d_ctxfeat"][0] - got["d_ctxfeat0"][0], dcf, **GRAD_TOL)
    if kind == 0:
        close(got["d_w_part"], dw, **GRAD_TOL)


# ================================================================================================ C. vocabulary head criterion
def _quantised(shape, g, scale=16.0):
    """values k / 16, |k| < 48: any sum of up to 8 of them (+ a shift of +-90) is exact in fp32, so the fp32 slab sum the kernel
    takes its argmax over equals the fp64 one and ties are exact"""
    return torch.randint(-47, 48, shape, generator=g).float() / scale


def nll_head_ref(logits64, target, w):
    """fp64: (loss, argmax with ties to the lowest index, pre = w * (softmax - onehot))"""
    lp = torch.log_softmax(logits64, 1)
    loss = -(lp.gather(1, target[:, None]).squeeze(1) * w.double()).sum()
    mx = logits64.max(1, keepdim=True)[0]
    V = logits64.shape[1]
    amax = torch.where(logits64 == mx, torch.arange(V, dtype=torch.int64)[None], torch.full((1, V), V, dtype=torch.int64)).min(1)[0]
    pre = w.double()[:, None] * (lp.exp() - F.one_hot(target, V).double())
    return loss, amax, pre


def _head_inputs(M, V, nparts, ld, g, with_bias=True):
    parts = torch.full((nparts, M, ld), float("nan"))
    parts[:, :, :V] = _quantised((nparts, M, V), g)
    shift = torch.zeros(M)
    shift[1::3], shift[2::3] = 90.0, -90.0                          # exp without the max subtraction would overflow
    parts[0, :, :V] += shift[:, None]
    bias = _quantised((V,), g) if with_bias else None
    if V >= 6:                                                      # an exact tie across the slab sum in row 0: index 2 must win
        if bias is not None:
            bias[5] = bias[2]
        row0 = parts[:, 0, :V].sum(0) + (bias if bias is not None else 0)
        parts[0, 0, 2] += float(row0.max()) + 1.0 - float(row0[2])
        parts[:, 0, 5] = parts[:, 0, 2].flip(0)                     # the same slab values in the other order
    target = torch.randint(0, V, (M,), generator=g)
    w = (torch.rand(M, generator=g) < 0.7).float()
    target[3::4] = 0                                                # padding rows: target 0 and w = 0
    w[3::4] = 0.0
    w[:min(M, 3)] = 1.0
    logits = parts[:, :, :V].double().sum(0) + (bias.double() if bias is not None else 0)
    return parts, bias, target, w, logits


@pytest.mark.parametrize("V,nparts,M", [(1, 1, 7), (2, 3, 7), (255, 8, 7), (256, 1, 7), (257, 3, 7), (5000, 8, 7), (8191, 3, 7),
                                        (8192, 1, 7), (5000, 3, 1), (8192, 8, 1), (5000, 3, 1280)])
def test_vocab_head_nll_fwd_vs_fp64(dev, L, V, nparts, M):
    """cvc_vocab_head_nll_fwd through raw calls: ld > V, pre NOT aliasing its input with ld_pre != ld (columns past V and rows'
    padding untouched), with and without bias; loss, argmax (exact ties across the slab sum -> lowest index), pre (exactly 0 on
    w = 0 rows, including target-0 padding rows); rows shifted by +-90"""
    for with_bias in (True, False):
        g = _gen("head", V, nparts, M, with_bias)
        ld, ld_pre = V + 4, V + 9
        parts, bias, target, w, logits = _head_inputs(M, V, nparts, ld, g, with_bias)
        pd, bd, td, wd = parts.to(dev), (bias.to(dev) if bias is not None else None), target.to(dev), w.to(dev)
        outs = []
        for _ in range(2):
            pre = torch.full((M, ld_pre), SENTINEL, device=dev)
            amax = torch.full((M,), -5, dtype=torch.int64, device=dev)
            row_loss, loss = torch.full((M,), SENTINEL, device=dev), torch.full((1,), SENTINEL, device=dev)
            rc = L.cvc_vocab_head_nll_fwd(pd.data_ptr(), nparts, M * ld, ld, _ptr(bd), td.data_ptr(), wd.data_ptr(), M, V, pre.data_ptr(),
                                          ld_pre, amax.data_ptr(), row_loss.data_ptr(), loss.data_ptr(), _stream())
            assert rc == 0
            outs.append((pre, amax, loss))
        pre, amax, loss = outs[0]
        rl, ra, rp = nll_head_ref(logits, target, w)
        close(loss, rl.reshape(1), rtol=2e-6 * max(M, 8), atol=1e-5)
        assert torch.equal(amax.cpu(), ra)
        if V >= 6:
            assert int(amax[0]) == 2
        close(pre[:, :V], rp, **OP_TOL)
        assert bool((pre[w.to(dev) == 0, :V] == 0).all())
        assert bool((pre[:, V:] == SENTINEL).all())
        assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))


def test_vocab_head_nll_fwd_wrapper_and_bounds(dev, L):
    """hip.vocab_head_nll_fwd (pre aliasing slab 0) against fp64; V = 8193 (past the register cache) and bad leading dimensions
    return CVC_E_BADARG"""
    from cvc import hip
    M, V, nparts = 300, 5000, 3
    g = _gen("headw")
    parts, bias, target, w, logits = _head_inputs(M, V, nparts, V, g)
    pd = parts.contiguous().to(dev)
    loss, amax, pre = hip.vocab_head_nll_fwd(pd, bias.to(dev), target.to(dev), w.to(dev))
    assert pre.data_ptr() == pd.data_ptr()
    rl, ra, rp = nll_head_ref(logits, target, w)
    close(loss, rl.reshape(1), rtol=2e-6 * M, atol=1e-5)
    assert torch.equal(amax.cpu(), ra) and int(amax[0]) == 2
    close(pre, rp, **OP_TOL)
    assert bool((pre[w.to(dev) == 0] == 0).all())
    t1, w1 = torch.zeros(2, dtype=torch.int64, device=dev), torch.ones(2, device=dev)
    buf = torch.zeros(2, 8200, device=dev)
    out = torch.full((2, 8200), SENTINEL, device=dev)
    ws = torch.zeros(4, device=dev)
    a1 = torch.zeros(2, dtype=torch.int64, device=dev)
    for V_, ld, ld_pre in ((8193, 8200, 8200), (64, 63, 64), (64, 64, 63)):
        rc = L.cvc_vocab_head_nll_fwd(buf.data_ptr(), 1, 0, ld, None, t1.data_ptr(), w1.data_ptr(), 2, V_, out.data_ptr(), ld_pre,
                                      a1.data_ptr(), ws.data_ptr(), ws[2:].data_ptr(), _stream())
        assert rc == BADARG, (V_, ld, ld_pre)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_scale_by_scalar_bitwise(dev, L):
    """cvc_scale_by_scalar == g * pre bit for bit (device scalar g); n % 4 != 0 and n < 4 are rejected"""
    from cvc import hip
    g = _gen("scale")
    x = torch.randn(1283, 4 * 37, generator=g).to(dev)
    s = torch.tensor([-0.37], device=dev)
    y = hip.scale_by_scalar(x, s)
    assert torch.equal(y, x * s) and torch.equal(y, hip.scale_by_scalar(x, s))
    close(y, x.double() * -0.37, **OP_TOL)
    out = torch.full((16,), SENTINEL, device=dev)
    for n in (6, 2, 15):
        assert L.cvc_scale_by_scalar(x.data_ptr(), s.data_ptr(), n, out.data_ptr(), _stream()) == BADARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_vocab_head_nll_end_to_end_vs_fp64(dev, L):
    """F.vocab_head_nll under autograd at the config-3 head size (M = 1280, K = 2048, V = 5000): loss, argmax and the gradients of
    x, W and b (cvc_vocab_head_nll_fwd's pre scaled by cvc_scale_by_scalar, through nn.Linear's backward products)"""
    from cvc import functional as F_
    M, K, V = 1280, 2048, 5000
    g = _gen("head_e2e")
    x0, W0, b0 = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g) * 0.02, torch.randn(V, generator=g) * 0.1
    target = torch.randint(0, V, (M,), generator=g)
    target[::9] = 0
    w = (torch.rand(M, generator=g) < 0.7).float()
    w[::9] = 0.0
    assert F_.vocab_head_nll_ok(x0.to(dev), W0.to(dev))
    x, W, b = (t.to(dev).requires_grad_(True) for t in (x0, W0, b0))
    loss, amax = F_.vocab_head_nll(x, W, b, target.to(dev), w.to(dev))
    (loss * 0.37).sum().backward()
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x0, W0, b0))
    logits = xr @ Wr.t() + br
    lp = torch.log_softmax(logits, 1)
    ref = -(lp.gather(1, target[:, None]).squeeze(1) * w.double()).sum()
    (ref * 0.37).backward()
    close(loss, ref.reshape(1), rtol=2e-6 * M, atol=1e-5)
    # argmax over fp32 logits of a K = 2048 product: compared where the fp64 top-2 gap is clear of the products' rounding
    top2 = logits.detach().topk(2, 1)[0]
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert torch.equal(amax.cpu()[clear], logits.detach().argmax(1)[clear]) and int(clear.sum()) > M * 0.9
    close(x.grad, xr.grad, **GRAD_TOL)
    close(W.grad, Wr.grad, **red_tol(M))
    close(b.grad, br.grad, **red_tol(M))


@pytest.mark.parametrize("M,V", [(1, 1), (7, 9), (64, 5000), (300, 257)])
def test_unfused_log_softmax_masked_nll_vs_fp64(dev, L, M, V):
    """the captioner's unfused criterion: F.log_softmax (cvc_log_softmax_fwd/_bwd) + F.masked_nll_sum (cvc_nll_fwd/_bwd) under
    autograd against fp64, rows holding -inf entries (masked words) included"""
    from cvc import functional as F_
    g = _gen("unfused", M, V)
    logits = torch.randn(M, V, generator=g) * 3
    if V > 1:
        logits[::2, V // 2:] = -float("inf")
    target = torch.randint(0, max(1, V // 2), (M,), generator=g)
    w = (torch.rand(M, generator=g) < 0.7).float()
    w[0] = 1.0
    x = logits.to(dev).requires_grad_(True)
    lp = F_.log_softmax(x)
    loss = F_.masked_nll_sum(lp, target.to(dev), w.to(dev))
    (loss * 0.37).sum().backward()
    xr = logits.double().requires_grad_(True)
    lpr = torch.log_softmax(xr, 1)
    ref = -(lpr.gather(1, target[:, None]).squeeze(1) * w.double()).sum()
    (ref * 0.37).backward()
    close(lp, lpr, **OP_TOL)
    close(loss, ref.reshape(1), rtol=2e-6 * max(M, 8), atol=1e-5)
    close(x.grad, xr.grad, **GRAD_TOL)
    assert bool(torch.isfinite(x.grad).all())
    x2 = logits.to(dev).requires_grad_(True)
    lp2 = F_.log_softmax(x2)
    (F_.masked_nll_sum(lp2, target.to(dev), w.to(dev)) * 0.37).sum().backward()
    assert torch.equal(lp2, lp) and torch.equal(x2.grad, x.grad)


# ================================================================================================ D. encoder train-mode kernels
@pytest.mark.parametrize("rows,Cn", [(2, 4), (255, 260), (256, 1024), (257, 260), (6400, 1024), (48000, 260)])
def test_bn_relu_train_vs_fp64(dev, L, rows, Cn):
    """cvc_bn_relu_train_fwd/_bwd against fp64 autograd of relu(F.batch_norm(training=True, momentum=0.1)): y, mean, invstd,
    running statistics (unbiased variance), dx, dgamma, dbeta; rows around the 256-row chunks of the column sums"""
    g = _gen("bn", rows, Cn)
    eps, mom = 1e-5, 0.1
    x0 = torch.randn(rows, Cn, generator=g) * 2 + 3                 # a non-zero mean: a row missed by the sums shows in the mean
    gamma0, beta0 = torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g) * 0.5
    rm0, rv0 = torch.randn(Cn, generator=g), torch.rand(Cn, generator=g) + 0.5
    dy0 = torch.randn(rows, Cn, generator=g)
    x, gamma, beta, dy = (t.to(dev) for t in (x0, gamma0, beta0, dy0))
    nws = int(L.cvc_bn_workspace(rows, Cn))
    res = []
    for _ in range(2):
        rm, rv = rm0.to(dev), rv0.to(dev)
        y = torch.full((rows, Cn), SENTINEL, device=dev)
        mean, invstd = torch.full((Cn,), SENTINEL, device=dev), torch.full((Cn,), SENTINEL, device=dev)
        ws = torch.full((nws,), float("nan"), device=dev)
        assert L.cvc_bn_relu_train_fwd(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, mom, rm.data_ptr(), rv.data_ptr(), rows,
                                       Cn, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), _stream()) == 0
        dx = torch.full((rows, Cn), SENTINEL, device=dev)
        dgam, dbet = torch.full((Cn,), SENTINEL, device=dev), torch.full((Cn,), SENTINEL, device=dev)
        ws.fill_(float("nan"))
        assert L.cvc_bn_relu_train_bwd(x.data_ptr(), dy.data_ptr(), y.data_ptr(), gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                       rows, Cn, dx.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), ws.data_ptr(), _stream()) == 0
        res.append((y, mean, invstd, rm, rv, dx, dgam, dbet))
    y, mean, invstd, rm, rv, dx, dgam, dbet = res[0]
    xr, gr, br = (t.double().requires_grad_(True) for t in (x0, gamma0, beta0))
    rmr, rvr = rm0.double(), rv0.double()
    zr = F.batch_norm(xr, rmr, rvr, gr, br, training=True, momentum=mom, eps=eps)
    yr = F.relu(zr)
    # the ReLU's gate as the kernel's forward decided it: an fp32 pre-activation within rounding of 0 may fall either way (one in
    # ~10^7 elements does at 48000 x 260), and its whole dy then moves dbeta / dgamma; away from 0 the gates must agree
    gate = (y > 0).cpu()
    assert torch.equal(gate[zr.detach().abs() > 1e-4], (zr.detach() > 0)[zr.detach().abs() > 1e-4])
    (zr * gate).backward(dy0.double())
    xd = x0.double()
    close(mean, xd.mean(0), **OP_TOL)
    close(invstd, 1.0 / torch.sqrt(xd.var(0, unbiased=False) + eps), **OP_TOL)
    close(rm, rmr, **OP_TOL)
    close(rv, rvr, **OP_TOL)
    close(y, yr, **OP_TOL)
    close(dx, xr.grad, **GRAD_TOL)
    close(dgam, gr.grad, **red_tol(rows))
    close(dbet, br.grad, **red_tol(rows))
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


LN_WIDTHS = [(2048, 300, 432), (3072, 4), (7,), (24, 300, 7)]


@pytest.mark.parametrize("widths", LN_WIDTHS)
@pytest.mark.parametrize("rows", [1, 6400])
def test_layernorm_cat_bwd_vs_fp64(dev, L, widths, rows):
    """cvc_layernorm_cat_bwd against fp64 autograd of cat(layer_norm(x_i)): inputs as column views of a wider tensor (ldx > width),
    d_out with ld_out > total, the dx's as column views of one wider buffer, one dx NULL (its columns and the padding untouched)"""
    g = _gen("ln", widths, rows)
    eps = 1e-5
    tot = sum(widths)
    xw = torch.randn(rows, tot + 5, generator=g) * 1.7 + 0.3
    offs = np.cumsum((0,) + widths[:-1]).tolist()
    xs = [xw[:, o + 2:o + 2 + d] for o, d in zip(offs, widths)]
    d_out = torch.full((rows, tot + 3), float("nan"))
    d_out[:, :tot] = torch.randn(rows, tot, generator=g)
    skip = len(widths) - 1 if len(widths) > 1 else None             # the NULL dx (the last segment when there are several)
    xd, dod = xw.to(dev), d_out.to(dev)
    xs_d = [xd[:, o + 2:o + 2 + d] for o, d in zip(offs, widths)]
    res = []
    for _ in range(2):
        dxw = torch.full((rows, tot + 6), SENTINEL, device=dev)
        dxs = [None if s == skip else dxw[:, o + 1:o + 1 + d] for s, (o, d) in enumerate(zip(offs, widths))]
        n = len(widths)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in xs_d])
        lds = (C.c_longlong * n)(*[t.stride(0) for t in xs_d])
        ws = (C.c_int * n)(*widths)
        dptrs = (C.c_void_p * n)(*[None if t is None else t.data_ptr() for t in dxs])
        dlds = (C.c_longlong * n)(*[0 if t is None else t.stride(0) for t in dxs])
        assert L.cvc_layernorm_cat_bwd(ptrs, lds, ws, n, rows, eps, dod.data_ptr(), dod.stride(0), dptrs, dlds, _stream()) == 0
        res.append(dxw)
    assert torch.equal(res[0], res[1])
    dxw = res[0]
    xr = [x.double().requires_grad_(True) for x in xs]
    out = torch.cat([F.layer_norm(x, (x.shape[1],), eps=eps) for x in xr], 1)
    out.backward(d_out[:, :tot].double())
    for s, (o, d) in enumerate(zip(offs, widths)):
        got = dxw[:, o + 1:o + 1 + d]
        if s == skip:
            assert bool((got == SENTINEL).all())
        else:
            close(got, xr[s].grad, **GRAD_TOL)
    assert bool((dxw[:, :1] == SENTINEL).all()) and bool((dxw[:, tot + 1:] == SENTINEL).all())


@pytest.mark.parametrize("Cn", [7, 64, 65, 432])
def test_class_softmax_bwd_vs_fp64(dev, L, Cn):
    """cvc_class_softmax_bwd against fp64 autograd of p = softmax(logits) feeding sim_rows [B, N, C] and sim [B, C, N]: gradients
    from d_rows only, d_sim only and both; padded regions give exact zeros"""
    B, N = 3, 37
    g = _gen("cls", Cn)
    logits = torch.randn(B * N, Cn, generator=g) * 2
    p32 = torch.softmax(logits.double(), 1).float()
    d_rows, d_sim = torch.randn(B, N, Cn, generator=g), torch.randn(B, Cn, N, generator=g)
    pad = torch.rand(B * N, generator=g) < 0.25
    pd, padd = p32.to(dev), pad.to(torch.uint8).to(dev)
    for use_rows, use_sim in ((True, False), (False, True), (True, True)):
        dr, ds = (d_rows.to(dev) if use_rows else None), (d_sim.to(dev) if use_sim else None)
        outs = []
        for _ in range(2):
            out = torch.full((B * N, Cn), SENTINEL, device=dev)
            assert L.cvc_class_softmax_bwd(pd.data_ptr(), _ptr(dr), _ptr(ds), padd.data_ptr(), B, N, Cn, out.data_ptr(), _stream()) == 0
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        lr = logits.double().requires_grad_(True)
        p = torch.softmax(lr, 1).view(B, N, Cn)
        loss = 0
        if use_rows:
            loss = loss + (p * d_rows.double()).sum()
        if use_sim:
            loss = loss + (p.transpose(1, 2) * d_sim.double()).sum()
        loss.backward()
        ref = torch.where(pad[:, None], torch.zeros(()), lr.grad)
        close(outs[0], ref, **GRAD_TOL)
        assert bool((outs[0][padd.bool()] == 0).all())


@pytest.mark.parametrize("rows,N", [(37, 132), (5, 4), (129, 2052)])
def test_relu_dropout_fwd_bwd_vs_fp64(dev, L, rows, N):
    """cvc_relu_dropout_fwd/_bwd against fp64 autograd of relu(x + bias) * keep-mask (cvc.dropout.host_mask): with and without
    bias, p = 0 (generator NULL) and 0.5; rows * N not a multiple of the 1024 elements a workgroup covers"""
    from cvc import dropout
    g = _gen("relu_drop", rows, N)
    x0, b0, dy0 = torch.randn(rows, N, generator=g), torch.randn(N, generator=g) * 0.3, torch.randn(rows, N, generator=g)
    x, b, dy = x0.to(dev), b0.to(dev), dy0.to(dev)
    site = "enc.att1"
    for p in (0.0, 0.5):
        st = dropout.rng_state(dev) if p > 0 else None
        mask = dropout.host_mask(site, (rows, N), p, dev).double() if p > 0 else torch.ones(rows, N, dtype=torch.float64)
        for with_bias in (True, False):
            outs = []
            for _ in range(2):
                y = torch.full((rows, N), SENTINEL, device=dev)
                assert L.cvc_relu_dropout_fwd(x.data_ptr(), _ptr(b if with_bias else None), rows, N, _ptr(st), dropout.site_id(site),
                                              p, y.data_ptr(), _stream()) == 0
                dx = torch.full((rows, N), SENTINEL, device=dev)
                assert L.cvc_relu_dropout_bwd(dy.data_ptr(), y.data_ptr(), rows * N, _ptr(st), dropout.site_id(site), p, dx.data_ptr(),
                                              _stream()) == 0
                outs.append((y, dx))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
            y, dx = outs[0]
            xr = x0.double().requires_grad_(True)
            yr = F.relu(xr + (b0.double() if with_bias else 0)) * mask
            yr.backward(dy0.double())
            close(y, yr, **OP_TOL)
            close(dx, xr.grad, **GRAD_TOL)
            if p > 0 and mask.numel() >= 4096:
                assert abs(float((mask == 0).double().mean()) - p) < 0.05
