"""Shared pieces of tests/test_gpu_attn_step.py (not collected: no test_ prefix): input builders, torch fp64 restatements and
C-ABI callers of the decode attention step (csrc/attn_scores.h, csrc/attn_fwd.hip), and the fixed case list that the test runs in
its own process AND in child processes under other CVC_SCORE_ROWS_RT / CVC_WSUM_* settings (those are read once per process).

Run as a program (`python tests/attn_step_cases.py OUT.npz`) it runs env_cases(), which checks every output against fp64 itself,
and writes the raw outputs to OUT.npz for the parent's bitwise comparisons."""
import math
import os
import sys

import numpy as np
import torch

OP_TOL = dict(rtol=2e-5, atol=2e-5)              # tests/test_gpu_parity.py
ATTN_TOL = dict(rtol=2e-5, atol=2e-6)            # test_two_set_weighted_sum_at_the_edges_of_its_hoisted_forms
CTX_TOL = dict(rtol=2e-5, atol=2e-5)
E_BADARG, E_TOOBIG = -1, -2                      # include/cvc_hip.h
MIN_VALUE = -1e8
FRAG_PATTERN = 0x7FC0


def stream_handle():
    return torch.cuda.current_stream().cuda_stream


def nan_buf(*shape, dev):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def all_nan(t):
    return bool(torch.isnan(t).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def close(a, b, **tol):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, **tol)


# ------------------------------------------------------------------ score pass
def score_case(seed, kind, nclip, nq, A, ns, P=1, bias=False, mask="set0", big=None):
    """Inputs of one score-pass call.  kind: "additive" | "dot".  ns: feature rows of each set (1 or 2 sets).  Set 0 carries a region
    mask (clip nclip - 1 fully masked when nclip > 1) and a frame mask unless mask is None; set 1 carries neither.  The query is
    P planes (+ q_bias) whose sum has unit scale (1 / sqrt(A) for dot); big = (row, col, value): added to plane 0."""
    g = torch.Generator().manual_seed(seed)
    rows = nclip * nq
    qp = torch.randn(P, rows, A, generator=g) / math.sqrt(P)
    qb = torch.randn(A, generator=g) * 0.5 if bias else None
    if kind == "dot":
        qp /= math.sqrt(A)
        if qb is not None:
            qb /= math.sqrt(A)
    if big is not None:
        qp[0, big[0], big[1]] += big[2]
    c = dict(kind=kind, nclip=nclip, nq=nq, A=A, ns=list(ns), P=P, qp=qp, qb=qb,
             w=torch.randn(A, generator=g) * (0.3 * math.sqrt(256.0 / A)), b=torch.randn(1, generator=g), inv_temp=1.0 / 1.7,
             proj=[torch.randn(nclip, n, A, generator=g) for n in ns], mask=None, fmask=None)
    if mask is not None:
        m = torch.rand(nclip, ns[0], generator=g) < 0.3
        if nclip > 1:
            m[nclip - 1] = True
        c["mask"] = m.to(torch.uint8)
        c["fmask"] = (torch.rand(rows, ns[0], generator=g) < 0.3).to(torch.uint8)
    return c


def ref_scores(c, dev, stream=0, planes=None):
    """torch fp64: [(scores, frame_masked or None)] per set, on `dev`.  planes: how many of the query planes enter (None: all + bias)."""
    fill = -math.inf if stream & 4 else MIN_VALUE
    nclip, nq, A = c["nclip"], c["nq"], c["A"]
    q = c["qp"].to(dev).double()
    q = q.sum(0) + (c["qb"].to(dev).double() if c["qb"] is not None else 0.0) if planes is None else q[:planes].sum(0)
    q = q.view(nclip, nq, A)
    out = []
    for s, p in enumerate(c["proj"]):
        p = p.to(dev).double()
        if c["kind"] == "additive":
            sc = torch.stack([(torch.tanh(p + q[:, u, None, :]) * c["w"].to(dev).double()).sum(-1) for u in range(nq)], 1) + c["b"].to(dev).double()
        else:
            sc = torch.einsum("cna,cua->cun", p, q) * c["inv_temp"]
        fm = None
        if s == 0 and c["mask"] is not None:
            sc = sc.masked_fill(c["mask"].to(dev).bool()[:, None, :], fill)
            fm = sc.reshape(nclip * nq, -1).masked_fill(c["fmask"].to(dev).bool(), fill)
        out.append((sc.reshape(nclip * nq, -1), fm))
    return out


def run_scores(hip, dev, c, stream=0, qparts=True):
    """cvc_attn_scores_qparts (all planes + bias) or cvc_attn_scores (plane 0 alone) into NaN-filled outputs.
    -> (rc, [(scores, frame_masked or None)], [attn buffers, which the score pass must not touch])"""
    L = hip.lib()
    nclip, nq, A = c["nclip"], c["nq"], c["A"]
    rows = nclip * nq
    keep = [c["qp"].to(dev).contiguous(), c["qb"].to(dev) if c["qb"] is not None else None, c["w"].to(dev), c["b"].to(dev)]
    qp, qb, w, b = keep
    arr = (hip.AttnSet * len(c["ns"]))()
    outs, attns = [], []
    for s, n in enumerate(c["ns"]):
        p = c["proj"][s].to(dev).contiguous()
        m = c["mask"].to(dev) if s == 0 and c["mask"] is not None else None
        fmk = c["fmask"].to(dev) if m is not None else None
        sc, at = nan_buf(rows, n, dev=dev), nan_buf(rows, n, dev=dev)
        fm = nan_buf(rows, n, dev=dev) if fmk is not None else None
        ptr = lambda t: None if t is None else t.data_ptr()
        arr[s] = hip.AttnSet(p.data_ptr(), p.data_ptr(), ptr(m), ptr(fmk), sc.data_ptr(), ptr(fm), at.data_ptr(), None, n, stream)
        keep += [p, m, fmk]
        outs.append((sc, fm)); attns.append(at)
    k = hip.ATTN_ADDITIVE if c["kind"] == "additive" else hip.ATTN_DOT
    if qparts:
        rc = L.cvc_attn_scores_qparts(k, qp.data_ptr(), c["P"], None if qb is None else qb.data_ptr(), w.data_ptr(), b.data_ptr(),
                                      c["inv_temp"], arr, len(c["ns"]), nclip, nq, A, stream_handle())
    else:
        rc = L.cvc_attn_scores(k, qp.data_ptr(), w.data_ptr(), b.data_ptr(), c["inv_temp"], arr, len(c["ns"]), nclip, nq, A, stream_handle())
    torch.cuda.synchronize()
    return rc, outs, attns


def check_scores(c, got, want, attns, stream=0):
    """every element: exactly the fill where the reference holds it, inside OP_TOL elsewhere; nothing else written"""
    fill = -math.inf if stream & 4 else MIN_VALUE
    for s, ((sc, fm), (rsc, rfm)) in enumerate(zip(got, want)):
        for name, a, r in (("scores", sc, rsc), ("frame_masked", fm, rfm)):
            if r is None:
                assert a is None
                continue
            filled = r == fill
            assert bool((a[filled] == fill).all()), (name, s, "masked positions must hold the fill exactly")
            assert bool(torch.isfinite(a[~filled]).all()), (name, s, "unwritten or non-finite element")
            err = float((a[~filled].double() - r[~filled]).abs().max()) if bool((~filled).any()) else 0.0
            print(f"attn_step scores kind={c['kind']} A={c['A']} nq={c['nq']} P={c['P']} set={s} {name}: max |err| = {err:.3e}")
            close(a[~filled], r[~filled].float(), err_msg=f"{name} of set {s}", **OP_TOL)
        assert all_nan(attns[s]), "the score pass wrote attn"


# ------------------------------------------------------------------ weighted sums
def wsum_case(seed, nclip, nq, ns, R, neg_inf_row=None):
    """scores per set: uniform in [-10, 10], a tenth of the entries at -1e8, row rows // 2 of set 0 fully -1e8 (rows > 1).
    neg_inf_row: that row of set 0 is -inf throughout instead."""
    g = torch.Generator().manual_seed(seed)
    rows = nclip * nq
    sc = []
    for n in ns:
        s = torch.rand(rows, n, generator=g) * 20 - 10
        s[torch.rand(rows, n, generator=g) < 0.1] = MIN_VALUE
        sc.append(s)
    if rows > 1:
        sc[0][rows // 2] = MIN_VALUE
    if neg_inf_row is not None:
        sc[0][neg_inf_row] = -math.inf
    return dict(nclip=nclip, nq=nq, ns=list(ns), R=R, scores=sc, ctx=[torch.randn(nclip, n, R, generator=g) for n in ns])


def ref_wsum(c, dev):
    """torch fp64 softmax + bmm -> ([attn], [ctx], ctx summed over the sets)"""
    at, cx = [], []
    for s, n in enumerate(c["ns"]):
        a = torch.softmax(c["scores"][s].to(dev).double(), 1)
        at.append(a)
        cx.append(torch.bmm(a.view(c["nclip"], c["nq"], n), c["ctx"][s].to(dev).double()).reshape(-1, c["R"]))
    return at, cx, sum(cx)


def run_wsum(hip, dev, c, call, ctx_out=True, stream=0):
    """call(arr, nsets, nclip, nq, R, stream_handle) -> rc launches one of the cvc_attn_wsum* entry points on the sets built here.
    -> (rc, [attn], [ctx_out or None], [scores as the device holds them afterwards])"""
    rows = c["nclip"] * c["nq"]
    arr = (hip.AttnSet * len(c["ns"]))()
    keep, attn, cout, scs = [], [], [], []
    for s, n in enumerate(c["ns"]):
        x, sc = c["ctx"][s].to(dev).contiguous(), c["scores"][s].to(dev).contiguous()
        a = nan_buf(rows, n, dev=dev)
        o = nan_buf(rows, c["R"], dev=dev) if ctx_out else None
        arr[s] = hip.AttnSet(x.data_ptr(), x.data_ptr(), None, None, sc.data_ptr(), None, a.data_ptr(), None if o is None else o.data_ptr(), n, stream)
        keep.append(x); attn.append(a); cout.append(o); scs.append(sc)
    rc = call(arr, len(c["ns"]), c["nclip"], c["nq"], c["R"], stream_handle())
    torch.cuda.synchronize()
    return rc, attn, cout, scs


def run_wsum_rm(hip, dev, c, ctx_out=True, stream=0, want_sum=True):
    """cvc_attn_wsum -> (rc, attn, ctx_out, ctx_sum [rows, R] or None, scores)"""
    tot = nan_buf(c["nclip"] * c["nq"], c["R"], dev=dev) if want_sum else None
    L = hip.lib()
    rc, attn, cout, scs = run_wsum(hip, dev, c, lambda arr, ns, nclip, nq, R, st: L.cvc_attn_wsum(arr, ns, nclip, nq, R, None if tot is None else tot.data_ptr(), st),
                                   ctx_out, stream)
    return rc, attn, cout, tot, scs


def check_wsum(c, dev, attn, cout, tot, skip_rows=()):
    """attn, per-set contexts and their sum against fp64 on every row but skip_rows"""
    ra, rc_, rt = ref_wsum(c, dev)
    rows = c["nclip"] * c["nq"]
    keep = torch.ones(rows, dtype=torch.bool, device=dev)
    for r in skip_rows:
        keep[r] = False
    for s in range(len(c["ns"])):
        close(attn[s][keep], ra[s][keep].float(), err_msg=f"attn of set {s}", **ATTN_TOL)
        if cout[s] is not None:
            close(cout[s][keep], rc_[s][keep].float(), err_msg=f"context of set {s}", **CTX_TOL)
    if tot is not None:
        close(tot[keep], rt[keep].float(), err_msg="summed context", **CTX_TOL)


# ------------------------------------------------------------------ the cases run under every environment
def env_cases(hip, dev):
    """Fixed cases whose kernels' FORM depends on the process environment; every output is checked against fp64 here and returned
    (numpy, by name) for the bitwise comparisons between processes.

    * multi-query scores, n = 130 region rows and 40 frame rows, A = 260, nq = 5, additive (factored) and dot.  CVC_SCORE_ROWS_RT=r
      gives ceil(r / 4) rows per wave: wave w of chunk 0 takes rows w, w + 4, ..., and the mask ballot's bit k is its k-th row.  The
      region mask is random (about half set) and has rows 124 .. 127 -- bit 31 of every wave at r = 128 -- and 129 set in clip 0.
    * two-set weighted sums, nq = 1 and nq = 5, n = (130, 40) <= 512: the hoisted forms by default."""
    out = {}
    for kind in ("additive", "dot"):
        c = score_case(501, kind, 3, 5, 260, (130, 40), P=8, bias=True)
        g = torch.Generator().manual_seed(77)
        m = (torch.rand(3, 130, generator=g) < 0.5).to(torch.uint8)
        m[0, 124:128] = 1
        m[0, 129] = 1
        m[0, 120:124] = 0
        m[2] = 1
        c["mask"] = m
        rc, got, attns = run_scores(hip, dev, c)
        assert rc == 0, rc
        check_scores(c, got, ref_scores(c, dev), attns)
        out[f"scores.{kind}.0"], out[f"fm.{kind}.0"], out[f"scores.{kind}.1"] = got[0][0], got[0][1], got[1][0]
    for nq in (1, 5):
        c = wsum_case(600 + nq, 3, nq, (130, 40), 272)
        rc, attn, cout, tot, _ = run_wsum_rm(hip, dev, c)
        assert rc == 0, rc
        check_wsum(c, dev, attn, cout, tot)
        out[f"w{nq}.attn0"], out[f"w{nq}.attn1"], out[f"w{nq}.ctx0"], out[f"w{nq}.ctx1"], out[f"w{nq}.sum"] = attn[0], attn[1], cout[0], cout[1], tot
    return {k: v.cpu().numpy() for k, v in out.items()}


def main(path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "cyclical-visual-captioning_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from cvc import hip
    hip.lib()
    assert torch.cuda.is_available()
    np.savez(path, **env_cases(hip, torch.device("cuda:0")))
    print("ATTN-STEP-CHILD-OK", hip.LIB_PATH)


if __name__ == "__main__":
    main(sys.argv[1])
