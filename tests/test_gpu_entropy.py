"""The entropy regulariser of the vocabulary criterion on the GPU (csrc/vocab.hip: cvc_vocab_head_nll_ent_fwd, cvc_vocab_nll_ent_fwd /
_bwd) and through the layers above it, against the fp64 restatement of tests/entropy_ref.py.

Tolerance of the kernels: the rule of tests/test_gpu_label_smoothing.py -- the reference is the restatement in fp64; the yardstick is
the SAME restatement in fp32 on the CPU, on the same case; a kernel's largest error may be 4 x the yardstick's largest error with a
floor of 2^-20.  Where the reference itself is not finite (a label-smoothed loss over a column at -inf) the kernel must give the same
infinity or a NaN too.  Every test prints its figures before it asserts."""
import dataclasses

import pytest
import torch

from cvc import synth
import entropy_ref as R

pytestmark = pytest.mark.gpu

BADARG = -1
SENTINEL = -777.0
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from cvc import hip
    return hip.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(a, b):
    """bit for bit (NaNs and the sign of zero included)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and (torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b))


def _check(label, got, ref64, ref32):
    """one output against fp64 under the 4 x yardstick rule -> (error, bound)"""
    got, ref64, ref32 = got.detach().cpu().double().reshape(-1), ref64.reshape(-1), ref32.double().reshape(-1)
    odd = ~torch.isfinite(ref64)
    if bool(odd.any()):
        g, r = got[odd], ref64[odd]
        assert torch.equal(g.isnan(), r.isnan()) and torch.equal(g[~g.isnan()], r[~r.isnan()]), (label, g, r)
    fin = ~odd
    err = float((got[fin] - ref64[fin]).abs().max()) if bool(fin.any()) else 0.0
    yard = float((ref32[fin] - ref64[fin]).abs().max()) if bool(fin.any()) else 0.0
    bound = max(4.0 * yard, R.FLOOR)
    print(f"[entropy] {label}: kernel max |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e})")
    assert err <= bound, (label, err, yard, bound)
    return err, bound


def _head_case(M, V, nparts, with_bias, minus_inf=False, seed=3):
    """K-slice slabs [nparts, M, V] and a bias whose fp32 sum, in the kernel's order (slab 0, 1, ..., then the bias), is the logits of
    R.case up to rounding; the reference takes THAT fp32 sum as its input.  minus_inf: two columns of the bias are -inf (no row's
    target among them) -> (parts, bias, logits32, target, w, m, the -inf columns)"""
    logits, target, w, m = R.case(M, V, seed)
    g = torch.Generator().manual_seed(77 * V + M + nparts)
    bias = torch.randn(V, generator=g) if with_bias else None
    rest = [torch.randn(M, V, generator=g) for _ in range(nparts - 1)]
    first = logits - (bias if with_bias else 0)
    for r in rest:
        first = first - r
    parts = torch.stack([first] + rest)
    cols = R.minus_inf_columns(V, target) if with_bias and minus_inf else []
    if cols:
        bias[cols] = -INF
    x = parts[0].clone()
    for p in range(1, nparts):
        x = x + parts[p]
    if with_bias:
        x = x + bias
    return parts, bias, x, target, w, m, cols


VARIANTS = [(False, False), (True, False), (True, True)]            # (with a bias, two of its columns at -inf)


def _run_head(L, dev, parts, bias, target, w, m, eps, beta, alias, entry="ent"):
    """a raw call -> dict(pre [M, V], argmax, row_loss, loss_sum, row_nll, nll_sum, row_ent, ent_sum).  alias: pre = slab 0 (ld = ld_pre
    = V), else ld = V + 4 and ld_pre = V + 9 with sentinels around (checked here).  entry "ls": cvc_vocab_head_nll_ls_fwd"""
    nparts, M, V = parts.shape
    ld, ld_pre = (V, V) if alias else (V + 4, V + 9)
    pd = torch.full((nparts, M, ld), float("nan"), device=dev)
    pd[:, :, :V] = parts.to(dev)
    pre = pd[0] if alias else torch.full((M, ld_pre), SENTINEL, device=dev)
    bd, td, wd, md = (None if bias is None else bias.to(dev)), target.to(dev), w.to(dev), m.to(dev)
    amax = torch.full((M,), -5, dtype=torch.int64, device=dev)
    rows = torch.full((3, M), SENTINEL, device=dev)
    sums = torch.full((3,), SENTINEL, device=dev)
    lo = torch.full((3, M), SENTINEL, device=dev)                     # (the workspace of the rows' fp32 remainders)
    if entry == "ent":
        rc = L.cvc_vocab_head_nll_ent_fwd(pd.data_ptr(), nparts, M * ld, ld, _ptr(bd), td.data_ptr(), wd.data_ptr(), md.data_ptr(), M, V,
                                          float(eps), float(beta), pre.data_ptr(), ld_pre, amax.data_ptr(), rows[0].data_ptr(),
                                          sums[0:].data_ptr(), rows[1].data_ptr(), sums[1:].data_ptr(), rows[2].data_ptr(),
                                          sums[2:].data_ptr(), lo.data_ptr(), _stream())
    else:
        rc = L.cvc_vocab_head_nll_ls_fwd(pd.data_ptr(), nparts, M * ld, ld, _ptr(bd), td.data_ptr(), wd.data_ptr(), M, V, float(eps),
                                         pre.data_ptr(), ld_pre, amax.data_ptr(), rows[0].data_ptr(), sums[0:].data_ptr(),
                                         rows[1].data_ptr(), sums[1:].data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if not alias:
        assert bool((pre[:, V:] == SENTINEL).all())
    return dict(pre=pre[:, :V].clone(), argmax=amax, row_loss=rows[0], loss_sum=sums[0], row_nll=rows[1], nll_sum=sums[1], row_ent=rows[2],
                ent_sum=sums[2])


def _run_two_step(L, dev, logits, target, w, m, eps, beta, g, entry="ent"):
    M, V = logits.shape
    x, t, wd, md = logits.to(dev), target.to(dev), w.to(dev), m.to(dev)
    lse = torch.full((M,), SENTINEL, device=dev)
    amax = torch.full((M,), -5, dtype=torch.int64, device=dev)
    rows, sums = torch.full((3, M), SENTINEL, device=dev), torch.full((3,), SENTINEL, device=dev)
    lo = torch.full((3, M), SENTINEL, device=dev)
    d = torch.full((M, V), SENTINEL, device=dev)
    gd = torch.tensor([g], device=dev)
    if entry == "ent":
        rc = L.cvc_vocab_nll_ent_fwd(x.data_ptr(), t.data_ptr(), wd.data_ptr(), md.data_ptr(), M, V, float(eps), float(beta), lse.data_ptr(),
                                     amax.data_ptr(), rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(), sums[1:].data_ptr(),
                                     rows[2].data_ptr(), sums[2:].data_ptr(), lo.data_ptr(), _stream())
        assert rc == 0, rc
        rc = L.cvc_vocab_nll_ent_bwd(x.data_ptr(), lse.data_ptr(), t.data_ptr(), wd.data_ptr(), md.data_ptr(), rows[2].data_ptr(),
                                     gd.data_ptr(), M, V, float(eps), float(beta), d.data_ptr(), _stream())
    else:
        rc = L.cvc_vocab_nll_ls_fwd(x.data_ptr(), t.data_ptr(), wd.data_ptr(), M, V, float(eps), lse.data_ptr(), amax.data_ptr(),
                                    rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(), sums[1:].data_ptr(), _stream())
        assert rc == 0, rc
        rc = L.cvc_vocab_nll_ls_bwd(x.data_ptr(), lse.data_ptr(), t.data_ptr(), wd.data_ptr(), gd.data_ptr(), M, V, float(eps), d.data_ptr(),
                                    _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(d_logits=d, argmax=amax, row_loss=rows[0], loss_sum=sums[0], row_nll=rows[1], nll_sum=sums[1], row_ent=rows[2],
                ent_sum=sums[2], lse=lse)


VALUES = ("row_loss", "row_nll", "row_ent", "loss_sum", "nll_sum", "ent_sum")


# ------------------------------------------------------------------------------------------------ the fused head kernel
@pytest.mark.parametrize("eps,beta", R.SETTINGS)
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_fused_head_vs_fp64(dev, L, M, V, nparts, eps, beta):
    """cvc_vocab_head_nll_ent_fwd: the row values, the three sums and pre against fp64, argmax exact; without a bias, with one, with
    two of its columns at -inf; pre aliasing slab 0 and not (then ld > V, ld_pre != ld, columns past V untouched); NLL weights 0, 1,
    negative and others, entropy weights 0 and 1; two runs bit-identical.
    The sums meet the bound because the entries form the row values in fp64 and add value + remainder in fp64: a sum is the fp64
    result rounded once (fp32 rows summed in fp32, or in fp64, miss it where the restatement's own fp32 sum happens to land on the
    nearest fp32 number)."""
    for with_bias, minus_inf in VARIANTS:
        parts, bias, logits32, target, w, m, cols = _head_case(M, V, nparts, with_bias, minus_inf)
        r64, r32 = R.restate(logits32, target, w, m, eps, beta), R.restate(logits32, target, w, m, eps, beta, torch.float32)
        outs = [_run_head(L, dev, parts, bias, target, w, m, eps, beta, alias) for alias in (False, True, True)]
        for k in outs[0]:
            assert _bits(outs[0][k], outs[1][k]) and _bits(outs[1][k], outs[2][k]), k
        o = outs[1]
        tag = f"head M {M} V {V} parts {nparts} eps {eps} beta {beta} bias {with_bias} -inf {cols}"
        for k in VALUES + ("pre",):
            _check(f"{tag} {k}", o[k], r64[k], r32[k])
        assert torch.equal(o["argmax"].cpu(), r64["argmax"])
        dead = ((w == 0) & (m == 0)).to(dev)
        assert bool((o["pre"][dead] == 0).all()) and bool((o["row_loss"][dead] == 0).all()) and bool((o["row_ent"][dead] == 0).all())
        assert bool((o["row_ent"][(m == 0).to(dev)] == 0).all()) and bool((o["row_ent"][(m != 0).to(dev)] > 0).all())
        if cols and eps == 0:
            assert bool((o["pre"][:, cols] == 0).all()) and bool(torch.isfinite(o["pre"]).all()) and bool(torch.isfinite(o["row_loss"]).all())


@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_beta_zero_has_the_bits_of_the_label_smoothing_entries(dev, L, M, V, nparts):
    """beta = 0 (the monitor mode) through the new entries == cvc_vocab_head_nll_ls_fwd / cvc_vocab_nll_ls_fwd / _bwd bit for bit in
    loss, pre, NLL, argmax and lse, rows that hold -inf logits included; the entropy is reported all the same"""
    for eps in (0.0, 0.1):
        for with_bias, minus_inf in VARIANTS:
            parts, bias, logits32, target, w, m, cols = _head_case(M, V, nparts, with_bias, minus_inf)
            r64, r32 = R.restate(logits32, target, w, m, eps, 0.0), R.restate(logits32, target, w, m, eps, 0.0, torch.float32)
            for alias in (False, True):
                new = _run_head(L, dev, parts, bias, target, w, m, eps, 0.0, alias)
                old = _run_head(L, dev, parts, bias, target, w, m, eps, 0.0, alias, entry="ls")
                for k in ("pre", "row_loss", "loss_sum", "row_nll", "nll_sum", "argmax"):
                    assert _bits(new[k], old[k]), (k, eps, alias, with_bias, cols)
            _check(f"monitor head M {M} V {V} eps {eps} -inf {cols} row_ent", new["row_ent"], r64["row_ent"], r32["row_ent"])
            _check(f"monitor head M {M} V {V} eps {eps} -inf {cols} ent_sum", new["ent_sum"], r64["ent_sum"], r32["ent_sum"])
            new = _run_two_step(L, dev, logits32, target, w, m, eps, 0.0, -0.37)
            old = _run_two_step(L, dev, logits32, target, w, m, eps, 0.0, -0.37, entry="ls")
            for k in ("d_logits", "row_loss", "loss_sum", "row_nll", "nll_sum", "argmax", "lse"):
                assert _bits(new[k], old[k]), (k, eps, with_bias, cols)
            _check(f"monitor two-step M {M} V {V} eps {eps} -inf {cols} row_ent", new["row_ent"], r64["row_ent"], r32["row_ent"])


# ------------------------------------------------------------------------------------------------ the two-step form
@pytest.mark.parametrize("eps,beta", R.SETTINGS)
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_two_step_form_vs_fp64(dev, L, M, V, nparts, eps, beta):
    """cvc_vocab_nll_ent_fwd (forward values) and cvc_vocab_nll_ent_bwd (d_logits = g x the restatement's pre) against fp64 under the
    same rule, on logits without and with columns at -inf; the gradient's yardstick is g x the restatement's pre in fp32"""
    g = -0.37
    for minus_inf in (False, True):
        _parts, _bias, logits, target, w, m, cols = _head_case(M, V, 1, True, minus_inf, seed=5)
        r64, r32 = R.restate(logits, target, w, m, eps, beta), R.restate(logits, target, w, m, eps, beta, torch.float32)
        o = _run_two_step(L, dev, logits, target, w, m, eps, beta, g)
        again = _run_two_step(L, dev, logits, target, w, m, eps, beta, g)
        assert all(_bits(o[k], again[k]) for k in o)
        tag = f"two-step M {M} V {V} eps {eps} beta {beta} -inf {cols}"
        for k in VALUES:
            _check(f"{tag} {k}", o[k], r64[k], r32[k])
        _check(f"{tag} lse", o["lse"], torch.logsumexp(logits.double(), 1), torch.logsumexp(logits, 1))
        _check(f"{tag} d_logits", o["d_logits"], g * r64["pre"], torch.tensor(g) * r32["pre"])
        assert torch.equal(o["argmax"].cpu(), r64["argmax"])
        dead = ((w == 0) & (m == 0)).to(dev)
        assert bool((o["d_logits"][dead] == 0).all()) and bool((o["row_loss"][dead] == 0).all()) and bool((o["row_ent"][dead] == 0).all())
        if cols and eps == 0:
            assert bool((o["d_logits"][:, cols] == 0).all()) and bool(torch.isfinite(o["d_logits"]).all())


@pytest.mark.parametrize("eps,beta", R.SETTINGS)
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_fused_form_and_two_step_form_agree_bit_for_bit(dev, L, M, V, nparts, eps, beta):
    """both kernels on equal logits (one slab, no bias; g = 1), columns at -inf included: every value, pre against d_logits and the
    argmax have the same bits"""
    for minus_inf in (False, True):
        _parts, _bias, logits, target, w, m, cols = _head_case(M, V, 1, True, minus_inf, seed=7)
        a = _run_head(L, dev, logits[None], None, target, w, m, eps, beta, alias=True)
        b = _run_two_step(L, dev, logits, target, w, m, eps, beta, 1.0)
        for ka, kb in [(k, k) for k in VALUES + ("argmax",)] + [("pre", "d_logits")]:
            same = _bits(a[ka], b[kb])
            if not same:
                diff = (a[ka].double() - b[kb].double()).abs()
                print(f"[entropy] fused vs two-step M {M} V {V} eps {eps} beta {beta} -inf {cols} {ka}: max |diff| {float(diff.max()):.3e}")
            assert same, (ka, cols)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev, L):
    """a beta that is not finite is refused before a launch (the Python layers raise, the raw entries return CVC_E_BADARG and write
    nothing); a `done` made with another beta is refused"""
    from cvc import functional as F_
    M, K, V = 72, 64, 100
    g = torch.Generator().manual_seed(11)
    x, W, b = torch.randn(M, K, generator=g).to(dev), (torch.randn(V, K, generator=g) * 0.1).to(dev), torch.randn(V, generator=g).to(dev)
    t, w = torch.randint(0, V, (M,), generator=g).to(dev), torch.ones(M, device=dev)
    assert F_.vocab_head_nll_ok(x, W)
    F_.new_step()
    lg = (x @ W.t()).contiguous()
    for bad in (float("nan"), INF, -INF):
        for call in (lambda: F_.vocab_head_nll(x, W, b, t, w, entropy_beta=bad, entropy_weight=w),
                     lambda: F_.vocab_nll(lg, t, w, entropy_beta=bad, entropy_weight=w),
                     lambda: F_.vocab_head_nll_compute(x, W, b, t, w, entropy_beta=bad, entropy_weight=w)):
            with pytest.raises(ValueError, match="entropy_beta"):
                call()
        out = torch.full((M, V), SENTINEL, device=dev)
        rows, sums = torch.full((3, M), SENTINEL, device=dev), torch.full((3,), SENTINEL, device=dev)
        assert L.cvc_vocab_head_nll_ent_fwd(lg.data_ptr(), 1, 0, V, None, t.data_ptr(), w.data_ptr(), w.data_ptr(), M, V, 0.0, bad,
                                            out.data_ptr(), V, None, rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(),
                                            sums[1:].data_ptr(), rows[2].data_ptr(), sums[2:].data_ptr(), out.data_ptr(), _stream()) == BADARG
        assert L.cvc_vocab_nll_ent_fwd(lg.data_ptr(), t.data_ptr(), w.data_ptr(), w.data_ptr(), M, V, 0.0, bad, rows[1].data_ptr(), None,
                                       rows[0].data_ptr(), sums[0:].data_ptr(), None, None, rows[2].data_ptr(), sums[2:].data_ptr(),
                                       out.data_ptr(), _stream()) == BADARG
        assert L.cvc_vocab_nll_ent_bwd(lg.data_ptr(), rows[0].data_ptr(), t.data_ptr(), w.data_ptr(), w.data_ptr(), rows[2].data_ptr(),
                                       sums.data_ptr(), M, V, 0.0, bad, out.data_ptr(), _stream()) == BADARG
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((rows == SENTINEL).all()) and bool((sums == SENTINEL).all())
    for made, asked in ((0.05, 0.02), (0.05, 0.0), (0.0, 0.05), (0.05, None), (None, 0.05)):
        mk = {} if made is None else dict(entropy_beta=made, entropy_weight=w)
        ak = {} if asked is None else dict(entropy_beta=asked, entropy_weight=w)
        done = F_.vocab_head_nll_compute(x, W, b, t, w, **mk)
        with pytest.raises(RuntimeError, match="entropy_beta"):
            F_.vocab_head_nll(x, W, b, t, w, done, **ak)
    done = F_.vocab_head_nll_compute(x, W, b, t, w, label_smoothing=0.1, entropy_beta=0.05, entropy_weight=w)
    loss, amax, nll, ent = F_.vocab_head_nll(x, W, b, t, w, done, label_smoothing=0.1, return_nll=True, entropy_beta=0.05, entropy_weight=w,
                                             return_entropy=True)
    assert torch.equal(loss, done[0]) and torch.equal(amax, done[1]) and torch.equal(nll, done[3]) and torch.equal(ent, done[5])
    assert not nll.requires_grad and not ent.requires_grad


# ------------------------------------------------------------------------------------------------ the functional layer under autograd
@pytest.mark.parametrize("V", [100, 97])
def test_functional_forms_under_autograd(dev, V):
    """F.vocab_head_nll (V = 100; V = 97 is a width it refuses) and F.vocab_nll with eps = 0.1, beta = 0.05, signed weights, on the same
    x W^T + b: loss, unsmoothed loss, entropy and the gradients of x, W and b against fp64 autograd.  The bound of the gradients is
    the one tests/test_gpu_train.py holds the training pass to: |err| <= 5e-4 |want| in norm."""
    from cvc import functional as F_
    M, K, eps, beta = 72, 64, 0.1, 0.05
    g = torch.Generator().manual_seed(V)
    x0, W0, b0 = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g) * 0.3, torch.randn(V, generator=g)
    target = torch.randint(0, V, (M,), generator=g)
    m = (torch.rand(M, generator=g) < 0.7).float()
    m[::9], target[::9] = 0.0, 0
    w = m * (torch.rand(M, generator=g) - 0.4)                                # advantages of either sign on the mask
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x0, W0, b0))
    z64 = xr @ Wr.t() + br
    logp = torch.log_softmax(z64, 1)
    H64 = -(logp.exp() * logp).sum(1)
    ref = (w.double() * torch.nn.functional.cross_entropy(z64, target, reduction="none", label_smoothing=eps)).sum() - beta * (m.double() * H64).sum()
    ref_nll = (w.double() * torch.nn.functional.cross_entropy(z64, target, reduction="none")).sum().detach()
    ref_ent = (m.double() * H64).sum().detach()
    (ref * 0.37).backward()
    z32 = x0 @ W0.t() + b0
    r32 = R.restate(z32, target, w, m, eps, beta, torch.float32)
    r64 = R.restate(z32, target, w, m, eps, beta)
    scale = float(r64["row_loss"].abs().sum())                                # (the loss itself is a sum of signed terms)
    kw = dict(label_smoothing=eps, return_nll=True, entropy_beta=beta, entropy_weight=m.to(dev), return_entropy=True)
    forms = {"two-step": lambda x, W, b: F_.vocab_nll(F_.linear(x, W, b), target.to(dev), w.to(dev), **kw)}
    if V % 4 == 0:
        forms["fused"] = lambda x, W, b: F_.vocab_head_nll(x, W, b, target.to(dev), w.to(dev), **kw)
    else:
        assert not F_.vocab_head_nll_ok(x0.to(dev), W0.to(dev))
    for name, form in forms.items():
        F_.new_step()            # (operands derived from weights are kept per step and address: fresh tensors, fresh step)
        x, W, b = (t.to(dev).requires_grad_(True) for t in (x0, W0, b0))
        loss, _amax, nll, ent = form(x, W, b)
        (loss * 0.37).sum().backward()
        for what, got, want, key in (("loss", loss, ref.detach(), "loss_sum"), ("nll", nll, ref_nll, "nll_sum"), ("entropy", ent, ref_ent, "ent_sum")):
            err = abs(float(got.detach().cpu().double() - want))
            yard = abs(float(r32[key].double() - r64[key]))
            bound = max(4.0 * yard, 4.0 * (scale if what != "entropy" else float(ref_ent)) * 2.0 ** -23)   # (floor: 4 fp32 ulps of the summed magnitudes)
            print(f"[entropy] functional {name} V {V}: {what} |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e})")
            assert err <= bound, (name, what, err, bound)
        assert not nll.requires_grad and not ent.requires_grad
        for got, want, what in ((x.grad, xr.grad, "x"), (W.grad, Wr.grad, "W"), (b.grad, br.grad, "b")):
            rel = float((got.cpu().double() - want).norm() / want.norm())
            print(f"[entropy] functional {name} V {V}: d{what} relative error {rel:.3e}")
            assert rel <= 5e-4, (name, what, rel)


# ------------------------------------------------------------------------------------------------ the model
def _dims(V):
    return dataclasses.replace(synth.CONFIGS["tiny"], B=12, R=64, A=32, E=32, V=V, T=6)


def _model(dev, d, seed=5, **over):
    from helpers import build_model, to_dev
    model = build_model(d, synth.hot_path_state_dict(d, seed), dev, **over).train()
    f, b = to_dev(synth.clip_features(d, seed), dev), to_dev(synth.label_glue_batch(d, seed), dev)
    return model, f, b


def _tap(obj, names, store):
    for name in names:
        orig = getattr(obj, name)

        def f(*a, _orig=orig, _name=name, **k):
            store.append((obj, _name, a, k))
            return _orig(*a, **k)
        setattr(obj, name, f)


def _one_pass(model, f, b, seed=31):
    """one training pass on the dropout masks of `seed` -> (losses, the criteria's tapped calls)"""
    from cvc import dropout
    from helpers import model_call
    calls = []
    _tap(model.critLM, ("from_head", "from_logits"), calls)
    _tap(model.xe_criterion, ("from_head", "from_logits"), calls)
    try:
        dropout.seed(seed)
        model.zero_grad(set_to_none=True)
        out = model_call(model, f, b, False)
    finally:
        for crit in (model.critLM, model.xe_criterion):
            for n in ("from_head", "from_logits"):
                crit.__dict__.pop(n, None)
    return out, calls


def _head_logits(model, x):
    """the head's product on x [rows, R] (fp32, from the device) -> (fp64 product of the fp32 operands, the fp32 product)"""
    x = x.detach().cpu()
    W, bias = model.logit.weight.detach().cpu(), model.logit.bias.detach().cpu()
    return x.double() @ W.double().t() + bias.double(), x @ W.t() + bias


def _expected_xe(model, call, eps, beta):
    """the restatement on the logits a tapped criterion call saw -> (loss64, nll64, entropy64, fp32 yardstick of the loss)"""
    obj, name, a, k = call
    lm = obj is model.critLM
    target = ((a[4] if name == "from_head" else a[3]) if lm else (a[2] if name == "from_head" else a[1])).cpu()
    mask = R.text_mask(target)
    tf, mf = (target.t().reshape(-1), mask.t().reshape(-1)) if k.get("t_major", False) else (target.reshape(-1), mask.reshape(-1))
    z64, z32 = _head_logits(model, a[0]) if name == "from_head" else (a[0].detach().cpu().double(), a[0].detach().cpu())
    loss, nll, ent = R.masked_mean(z64, tf, mf, mf, eps, beta)
    yard = abs(float(R.masked_mean(z32, tf, mf, mf, eps, beta, torch.float32)[0].double() - loss))
    return float(loss), float(nll), float(ent), yard


@pytest.mark.parametrize("V", [100, 97])
def test_model_xe_pass_with_a_confidence_penalty(dev, V):
    """A small synthetic model in training mode (dropout on, in-kernel masks of a fixed seed) at a width the fused head takes
    (V = 100, 72 rows) and at one it refuses (V = 97: the two-step fallback), eps = 0.1 and beta = 0.05: lm_loss and lm_recon_loss are
    the restatement on the model's own logits, model.last_entropy its mean masked entropy, and model.last_nll is that of a pass
    without the penalty on the same masks (4 fp32 ulps: the same rows, summed in fp64 here).  Bounds: the label-smoothing model test's -- 4 x the fp32 yardstick with a floor of 4 fp32
    ulps of the value."""
    from cvc import functional as F_
    eps, beta = 0.1, 0.05
    d = _dims(V)
    model, f, b = _model(dev, d, label_smoothing=eps, confidence_penalty=beta)
    assert model.confidence_penalty == beta and model.xe_criterion.confidence_penalty == beta and model.critLM.confidence_penalty == beta
    out, calls = _one_pass(model, f, b)
    assert [c[1] for c in calls] == ["from_head", "from_head"] and len(out) == 5
    assert F_.vocab_head_nll_ok(calls[0][2][0], model.logit.weight) == (V % 4 == 0)
    for i, name in ((0, "lm_loss"), (1, "lm_recon_loss")):
        got = float(out[0 if i == 0 else 4])
        want, want_nll, want_ent, yard = _expected_xe(model, calls[i], eps, beta)
        bound = max(4.0 * yard, 4.0 * want * 2.0 ** -23)
        print(f"[entropy] model V {V} {name}: {got:.6f} vs {want:.6f}, |err| {abs(got - want):.3e} (yardstick {yard:.3e}, bound {bound:.3e}); "
              f"NLL {want_nll:.6f}, entropy {want_ent:.6f}")
        assert abs(got - want) <= bound, (name, got, want, bound)
        if i == 0:
            ent = float(model.last_entropy)
            print(f"[entropy] model V {V}: last_entropy {ent:.6f} vs {want_ent:.6f}")
            assert abs(ent - want_ent) <= max(4.0 * yard, 4.0 * want_ent * 2.0 ** -23), (ent, want_ent)
            assert model.last_entropy.dim() == 0 and not model.last_entropy.requires_grad and 0 < ent <= torch.log(torch.tensor(float(V)))
            assert abs(float(model.last_nll) - want_nll) <= max(4.0 * yard, 4.0 * want_nll * 2.0 ** -23)
    last_nll, lm_with = model.last_nll.clone(), out[0].detach().clone()
    (0.5 * out[0].mean() + 0.5 * out[4].mean()).backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    # a pass without the penalty on the same masks: last_nll unchanged, no entropy kept, and the loss differs by beta x the entropy
    model.confidence_penalty = None
    out0, _ = _one_pass(model, f, b)
    assert model.last_entropy is None and model.critLM.last_entropy is None
    diff = abs(float(model.last_nll) - float(last_nll))
    print(f"[entropy] model V {V}: last_nll with the penalty {float(last_nll):.7f}, without {float(model.last_nll):.7f}, |diff| {diff:.3e}")
    assert diff <= 4.0 * float(last_nll) * 2.0 ** -23            # (the same rows; with beta != 0 their sum is accumulated in fp64)
    assert float(out0[0]) > float(lm_with)
    # the monitor mode: beta = 0 has the bits of the pass without it and reports the entropy
    model.confidence_penalty = 0.0
    out1, _ = _one_pass(model, f, b)
    assert _bits(out1[0].detach(), out0[0].detach()) and _bits(out1[4].detach(), out0[4].detach()) and float(model.last_entropy) > 0


@pytest.mark.parametrize("V", [100, 97])
def test_scst_loss_with_an_entropy_bonus(dev, V):
    """model.scst_loss(entropy_beta=beta) == model.scst_loss() - beta x the restatement's mean masked entropy on the model's own
    logits (debug_collect["scst_out"] through the head in fp64), within the label-smoothing model test's bound (4 x the fp32 yardstick
    of the loss, floor 4 fp32 ulps of the value); the gradient of logit.weight is the restatement's head-only gradient
    (5e-4 of the norm); entropy_beta = None and = 0 have the bits of today's scst_loss in loss, advantage and gradient"""
    beta = 0.05
    d = _dims(V)
    model, f, b = _model(dev, d)
    model.eval()
    P = dict(model.named_parameters())
    dummy = torch.zeros(d.B, 1, 1, device=dev)
    g = torch.Generator().manual_seed(3)
    words = torch.randint(0, V, (d.B, d.T), generator=g).to(dev)
    reward, base = torch.rand(d.B, generator=g).to(dev), torch.rand(d.B, generator=g).to(dev)
    with torch.no_grad():
        enc = model.encode_clips(f, b["proposals"], b["num"], b["box_mask"], dummy, b["gt_bboxs"], b["frm_mask"], b["sample_idx"], f["pnt_mask"])
    res = {}
    for key, kw in (("today", {}), ("none", dict(entropy_beta=None)), ("zero", dict(entropy_beta=0.0)), ("beta", dict(entropy_beta=beta))):
        model.zero_grad(set_to_none=True)
        model.debug_collect = {}
        loss, adv = model.scst_loss(enc, words, reward, base, 1, **kw)
        loss.backward()
        res[key] = dict(loss=loss.detach().clone(), adv=adv.clone(), grad=P["logit.weight"].grad.clone(), ent=model.last_entropy,
                        collect=model.debug_collect)
    model.debug_collect = None
    for key in ("none", "zero"):
        for k in ("loss", "adv", "grad"):
            assert _bits(res[key][k].reshape(-1), res["today"][k].reshape(-1)), (key, k)
    assert res["today"]["ent"] is None and res["none"]["ent"] is None and float(res["zero"]["ent"]) > 0
    c = res["beta"]["collect"]
    z64, z32 = _head_logits(model, c["scst_out"])
    target = words.masked_fill((words == 0).cumsum(1) > 0, 0).cpu()
    mask = R.text_mask(target)
    tf, mf = (target.t().reshape(-1), mask.t().reshape(-1)) if c["scst_t_major"] else (target.reshape(-1), mask.reshape(-1))
    w = c["scst_w"].detach().cpu().reshape(-1)
    assert bool((w < 0).any()) and bool((w > 0).any()) and bool((w[~mf] == 0).all())
    r64, r32 = R.restate(z64, tf, w, mf, 0.0, beta), R.restate(z32, tf, w, mf, 0.0, beta, torch.float32)
    count = float(mf.sum())
    ent64 = float(r64["ent_sum"]) / count
    want = float(res["today"]["loss"]) - beta * ent64
    got = float(res["beta"]["loss"])
    yard = abs(float(r32["loss_sum"].double() - r64["loss_sum"])) / count
    bound = max(4.0 * yard, 4.0 * abs(want) * 2.0 ** -23)
    print(f"[entropy] scst V {V}: loss {got:.7f} vs scst_loss() - beta H = {want:.7f}, |err| {abs(got - want):.3e} (yardstick {yard:.3e}, "
          f"bound {bound:.3e}); H {ent64:.6f}, last_entropy {float(res['beta']['ent']):.6f}, fp64 loss {float(r64['loss_sum']) / count:.7f}")
    assert abs(got - want) <= bound, (got, want, bound)
    assert abs(float(res["beta"]["ent"]) - ent64) <= max(4.0 * abs(float(r32["ent_sum"].double() - r64["ent_sum"])) / count, 4.0 * ent64 * 2.0 ** -23)
    assert _bits(res["zero"]["ent"].reshape(1), res["beta"]["ent"].reshape(1))
    dW = (r64["pre"].t() @ c["scst_out"].detach().cpu().double()) / count
    rel = float((res["beta"]["grad"].cpu().double() - dW).norm() / dW.norm())
    moved = float((res["beta"]["grad"] - res["today"]["grad"]).norm() / res["today"]["grad"].norm())
    print(f"[entropy] scst V {V}: d logit.weight relative error {rel:.3e}; the bonus moved the gradient by {moved:.3e} of its norm")
    assert rel <= 5e-4 and moved > 10 * 5e-4


# ------------------------------------------------------------------------------------------------ the captured step
def test_captured_step_equals_eager_step(dev):
    """train_step_graphed with beta = 0.05 (3 warm-up steps, a capture, 3 replays) against 6 eager steps of a twin: the loss vectors
    [loss, lm, att2, cls, recon, mean entropy] of steps 4 .. 6 and the parameters after them are equal (eval-mode dropout: both
    deterministic; the same launches on the same kind of buffers)"""
    from helpers import make_opts, to_dev
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    from cvc import opts as cvc_opts
    d, seed, beta = _dims(100), 5, 0.05
    vecs, finals = {}, {}
    for mode in ("eager", "graph"):
        o = cvc_opts.parse_opt([])
        for k, v in vars(make_opts(d, train_decoder_only=False, confidence_penalty=beta)).items():
            setattr(o, k, v)
        o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 2e-3, d.B
        model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed).items()}, strict=False)
        model = model.to(dev).eval()
        f, b = to_dev(synth.clip_features(d, seed), dev), to_dev(synth.label_glue_batch(d, seed), dev)
        batch = (f, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
                 ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], f["pnt_mask"][:, 1:])
        tr = Trainer(o, None, model, build_optimizer(model, o, capturable=True), None, None)
        assert tr.confidence_penalty == beta and tr.scst_entropy is None
        if mode == "eager":
            seq = [tr._core_step(tr._prepare(batch, True)).clone() for _ in range(6)]
            vecs[mode] = seq[3:]
        else:
            vecs[mode] = [tr.train_step_graphed(batch).clone() for _ in range(3)]
        torch.cuda.synchronize()
        finals[mode] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for i, (e, g) in enumerate(zip(vecs["eager"], vecs["graph"])):
        print(f"[entropy] captured step {i + 4}: eager {e.tolist()} graph {g.tolist()}")
        assert e.numel() == 6 and g.numel() == 6
        assert torch.equal(e, g), (e, g)
        assert 0 < float(g[5]) <= 4.61                                # the mean entropy, at most log(100)
    for k in finals["eager"]:
        assert torch.equal(finals["eager"][k], finals["graph"][k]), k
    # a model whose beta was changed afterwards: the trainer refuses the step
    model.confidence_penalty = 0.1
    with pytest.raises(RuntimeError, match="confidence_penalty"):
        tr._ent_tail()


# ------------------------------------------------------------------------------------------------ the trainer's self-critical step
@pytest.mark.parametrize("wor", [False, True])
def test_trainer_scst_step_reports_the_entropy(dev, wor):
    """Trainer.scst_step with scst_entropy, with and without rollouts drawn without replacement: last_scst["entropy"] is a finite
    device scalar >= 0 (at most log V); a trainer without the option keeps no such key"""
    import math
    import test_gpu_scst as TS
    d = _dims(100)
    for beta in (0.05, None):
        over = {} if beta is None else dict(scst_entropy=beta)
        o, model, tr = TS._trainer(dev, d, seed=5, S=3, lr=1e-4, **over)
        if wor:
            o.scst_wor = tr.scst_wor = True
        assert tr.scst_entropy == beta and tr.confidence_penalty is None
        _f, _b, batch = TS._batch(dev, d, 5)
        res = tr.scst_step(batch)
        assert len(res) == 4 and all(bool(torch.isfinite(x)) for x in res)
        if beta is None:
            assert "entropy" not in tr.last_scst and model.last_entropy is None
            continue
        ent = tr.last_scst["entropy"]
        print(f"[entropy] scst_step wor {wor}: entropy {float(ent):.6f}, loss {float(res[0]):.6f}")
        assert ent.is_cuda and ent.dim() == 0 and not ent.requires_grad
        assert math.isfinite(float(ent)) and 0 <= float(ent) <= math.log(d.V)


# ------------------------------------------------------------------------------------------------ the entry point
def test_main_entry_point_logs_the_entropy(tmp_path, capsys):
    """python -m cvc.main --log_entropy --scst_entropy 0.05: a cross-entropy epoch (beta = 0: measured only) and a self-critical epoch;
    the display line and the histories carry the mean entropy per display interval"""
    import math
    import os
    import pickle
    from cvc import main as cvc_main
    rc = cvc_main.main(["--no_cfg", "--max_epochs", "2", "--batch_size", "4", "--synthetic_clips", "12", "--num_prop_per_frm", "7",
                        "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "4",
                        "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "1", "--exp_name", "e", "--learning_rate", "0.001",
                        "--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/", "--id", "e1",
                        "--log_entropy", "--scst_entropy", "0.05", "--scst_after", "1", "--scst_samples", "3"])
    assert rc == 0
    tr = cvc_main.LAST_TRAINER
    model = getattr(tr.model, "module", tr.model)
    assert tr.confidence_penalty == 0.0 and model.confidence_penalty == 0.0 and tr.scst_entropy == pytest.approx(0.05)
    assert sorted(tr.entropy_history) == [0, 1] and all(len(v) == 2 for v in tr.entropy_history.values())   # 12 clips / 4 per batch, the last dropped
    assert all(math.isfinite(x) and x > 0 for v in tr.entropy_history.values() for x in v)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Epoch: [")]
    assert len(lines) == 4 and all("\tH " in l for l in lines) and sum("\tReward " in l for l in lines) == 2
    for l in lines:
        assert 0 < float(l.split("\tH ")[1].split()[0]) < 10
    hist = pickle.load(open(os.path.join(tmp_path, "e", "histories_e1.pkl"), "rb"))
    assert hist["entropy_history"] == tr.entropy_history
