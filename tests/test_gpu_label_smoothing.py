"""Label smoothing in the vocabulary criterion on the GPU (csrc/vocab.hip: cvc_vocab_head_nll_ls_fwd, cvc_vocab_nll_ls_fwd / _bwd) and
through the layers above it, against the fp64 restatement of tests/label_smoothing_ref.py.

Tolerance of the kernels: the reference is the restatement in fp64; the yardstick is the SAME restatement in fp32 on the CPU, on the
same case; a kernel's largest error may be 4 x the yardstick's largest error with a floor of 2^-20 (tests/test_gpu_cider.py's
convention).  Every test prints its figures before it asserts."""
import dataclasses

import pytest
import torch

from cvc import synth
import label_smoothing_ref as R

pytestmark = pytest.mark.gpu

BADARG = -1
SENTINEL = -777.0
HEAD_CASES = [(1, 5, 1), (7, 97, 3), (9, 257, 2), (33, 1000, 2), (5, 8192, 1)]          # (M, V, nparts)
EPS = [0.1, 0.5]


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


def _check(label, got, ref64, ref32):
    """one output against fp64 under the 4 x yardstick rule -> (error, bound)"""
    err = float((got.detach().cpu().double() - ref64).abs().max())
    yard = float((ref32.double() - ref64).abs().max())
    bound = max(4.0 * yard, R.FLOOR)
    print(f"[label smoothing] {label}: kernel max |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e})")
    assert err <= bound, (label, err, yard, bound)
    return err, bound


def _head_case(M, V, nparts, with_bias, seed=3):
    """K-slice slabs [nparts, M, V] and a bias whose fp32 sum, in the kernel's order (slab 0, 1, ..., then the bias), is the logits of
    R.case up to rounding; the reference takes THAT fp32 sum as its input -> (parts, bias, logits32, target, w)"""
    logits, target, w = R.case(M, V, seed)
    g = torch.Generator().manual_seed(77 * V + M + nparts)
    bias = torch.randn(V, generator=g) if with_bias else None
    rest = [torch.randn(M, V, generator=g) for _ in range(nparts - 1)]
    first = logits - (bias if with_bias else 0)
    for r in rest:
        first = first - r
    parts = torch.stack([first] + rest)
    x = parts[0].clone()
    for p in range(1, nparts):
        x = x + parts[p]
    if with_bias:
        x = x + bias
    return parts, bias, x, target, w


def _run_head(L, dev, parts, bias, target, w, eps, alias, entry="ls"):
    """a raw call -> dict(pre [M, V], argmax, row_loss, loss_sum, row_nll, nll_sum).  alias: pre = slab 0 (ld = ld_pre = V), else
    ld = V + 4 and ld_pre = V + 9 with sentinels around (checked here)"""
    nparts, M, V = parts.shape
    ld, ld_pre = (V, V) if alias else (V + 4, V + 9)
    pd = torch.full((nparts, M, ld), float("nan"), device=dev)
    pd[:, :, :V] = parts.to(dev)
    pre = pd[0] if alias else torch.full((M, ld_pre), SENTINEL, device=dev)
    bd, td, wd = (None if bias is None else bias.to(dev)), target.to(dev), w.to(dev)
    amax = torch.full((M,), -5, dtype=torch.int64, device=dev)
    rows = torch.full((2, M), SENTINEL, device=dev)
    sums = torch.full((2,), SENTINEL, device=dev)
    if entry == "ls":
        rc = L.cvc_vocab_head_nll_ls_fwd(pd.data_ptr(), nparts, M * ld, ld, _ptr(bd), td.data_ptr(), wd.data_ptr(), M, V, float(eps),
                                         pre.data_ptr(), ld_pre, amax.data_ptr(), rows[0].data_ptr(), sums[0:].data_ptr(),
                                         rows[1].data_ptr(), sums[1:].data_ptr(), _stream())
    else:
        rc = L.cvc_vocab_head_nll_fwd(pd.data_ptr(), nparts, M * ld, ld, _ptr(bd), td.data_ptr(), wd.data_ptr(), M, V, pre.data_ptr(), ld_pre,
                                      amax.data_ptr(), rows[0].data_ptr(), sums[0:].data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if not alias:
        assert bool((pre[:, V:] == SENTINEL).all())
    return dict(pre=pre[:, :V].clone(), argmax=amax, row_loss=rows[0], loss_sum=sums[0], row_nll=rows[1], nll_sum=sums[1])


# ------------------------------------------------------------------------------------------------ the fused head kernel
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("M,V,nparts", HEAD_CASES)
def test_fused_head_vs_fp64(dev, L, M, V, nparts, eps):
    """cvc_vocab_head_nll_ls_fwd: row_loss, row_nll, loss_sum, nll_sum and pre against fp64, argmax exact; with and without a bias;
    pre aliasing slab 0 and not (then ld > V, ld_pre != ld, columns past V untouched); weights 0, 1 and others; targets in the last
    column and in the first column of the last register slot; two runs bit-identical"""
    for with_bias in (True, False):
        parts, bias, logits32, target, w = _head_case(M, V, nparts, with_bias)
        r64, r32 = R.restate(logits32, target, w, eps), R.restate(logits32, target, w, eps, torch.float32)
        outs = [_run_head(L, dev, parts, bias, target, w, eps, alias) for alias in (False, True, True)]
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]) and torch.equal(outs[1][k], outs[2][k]), k
        o = outs[1]
        tag = f"head M {M} V {V} parts {nparts} eps {eps} bias {with_bias}"
        for k in ("row_loss", "row_nll", "loss_sum", "nll_sum", "pre"):
            _check(f"{tag} {k}", o[k], r64[k], r32[k])
        assert torch.equal(o["argmax"].cpu(), r64["argmax"])
        dead = (w == 0).to(dev)
        assert bool((o["pre"][dead] == 0).all()) and bool((o["row_loss"][dead] == 0).all()) and bool((o["row_nll"][dead] == 0).all())


@pytest.mark.parametrize("M,V,nparts", HEAD_CASES)
def test_eps_zero_has_the_bits_of_the_unsmoothed_entries(dev, L, M, V, nparts):
    """eps = 0 through the new entries == cvc_vocab_head_nll_fwd / cvc_vocab_nll_fwd / cvc_vocab_nll_bwd bit for bit; row_nll then is
    row_loss"""
    from cvc import hip
    parts, bias, logits32, target, w = _head_case(M, V, nparts, True)
    for alias in (False, True):
        new = _run_head(L, dev, parts, bias, target, w, 0.0, alias)
        old = _run_head(L, dev, parts, bias, target, w, 0.0, alias, entry="plain")
        for k in ("pre", "row_loss", "argmax", "loss_sum"):
            assert torch.equal(new[k], old[k]), (k, alias)
        assert torch.equal(new["row_nll"], new["row_loss"]) and torch.equal(new["nll_sum"], new["loss_sum"])
    x, t, wd = logits32.to(dev), target.to(dev), w.to(dev)
    loss0, lse0, amax0 = hip.vocab_nll_fwd(x, t, wd)
    loss1, lse1, amax1, nll1 = hip.vocab_nll_ls_fwd(x, t, wd, 0.0)
    assert torch.equal(loss0, loss1) and torch.equal(lse0, lse1) and torch.equal(amax0, amax1) and torch.equal(nll1, loss1)
    g = torch.tensor([-0.37], device=dev)
    assert torch.equal(hip.vocab_nll_bwd(x, lse0, t, wd, g), hip.vocab_nll_ls_bwd(x, lse0, t, wd, g, 0.0))


# ------------------------------------------------------------------------------------------------ the two-step form
def _run_two_step(L, dev, logits, target, w, eps, g):
    M, V = logits.shape
    x, t, wd = logits.to(dev), target.to(dev), w.to(dev)
    lse = torch.full((M,), SENTINEL, device=dev)
    amax = torch.full((M,), -5, dtype=torch.int64, device=dev)
    rows, sums = torch.full((2, M), SENTINEL, device=dev), torch.full((2,), SENTINEL, device=dev)
    rc = L.cvc_vocab_nll_ls_fwd(x.data_ptr(), t.data_ptr(), wd.data_ptr(), M, V, float(eps), lse.data_ptr(), amax.data_ptr(),
                                rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(), sums[1:].data_ptr(), _stream())
    assert rc == 0, rc
    d = torch.full((M, V), SENTINEL, device=dev)
    gd = torch.tensor([g], device=dev)
    rc = L.cvc_vocab_nll_ls_bwd(x.data_ptr(), lse.data_ptr(), t.data_ptr(), wd.data_ptr(), gd.data_ptr(), M, V, float(eps), d.data_ptr(),
                                _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(d_logits=d, argmax=amax, row_loss=rows[0], loss_sum=sums[0], row_nll=rows[1], nll_sum=sums[1], lse=lse)


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("M,V,nparts", HEAD_CASES)
def test_two_step_form_vs_fp64(dev, L, M, V, nparts, eps):
    """cvc_vocab_nll_ls_fwd (forward values) and cvc_vocab_nll_ls_bwd (d_logits = g w (softmax - (1 - eps) onehot - eps / V))
    against fp64 under the same rule; the gradient's yardstick is g x the restatement's pre in fp32"""
    logits, target, w = R.case(M, V, 5)
    g = -0.37
    r64, r32 = R.restate(logits, target, w, eps), R.restate(logits, target, w, eps, torch.float32)
    o = _run_two_step(L, dev, logits, target, w, eps, g)
    again = _run_two_step(L, dev, logits, target, w, eps, g)
    assert all(torch.equal(o[k], again[k]) for k in o)
    tag = f"two-step M {M} V {V} eps {eps}"
    for k in ("row_loss", "row_nll", "loss_sum", "nll_sum"):
        _check(f"{tag} {k}", o[k], r64[k], r32[k])
    _check(f"{tag} lse", o["lse"], torch.logsumexp(logits.double(), 1), torch.logsumexp(logits, 1))
    _check(f"{tag} d_logits", o["d_logits"], g * r64["pre"], torch.tensor(g) * r32["pre"])
    assert torch.equal(o["argmax"].cpu(), r64["argmax"])
    dead = (w == 0).to(dev)
    assert bool((o["d_logits"][dead] == 0).all()) and bool((o["row_loss"][dead] == 0).all())


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("M,V,nparts", HEAD_CASES)
def test_fused_form_against_two_step_form(dev, L, M, V, nparts, eps):
    """both kernels on the same logits (one slab, no bias; g = 1): two independent kernels agree within the sum of their bounds"""
    logits, target, w = R.case(M, V, 7)
    r64, r32 = R.restate(logits, target, w, eps), R.restate(logits, target, w, eps, torch.float32)
    a = _run_head(L, dev, logits[None], None, target, w, eps, alias=True)
    b = _run_two_step(L, dev, logits, target, w, eps, 1.0)
    for ka, kb, kr in (("row_loss", "row_loss", "row_loss"), ("row_nll", "row_nll", "row_nll"), ("loss_sum", "loss_sum", "loss_sum"),
                       ("pre", "d_logits", "pre")):
        bound = 2.0 * max(4.0 * float((r32[kr].double() - r64[kr]).abs().max()), R.FLOOR)
        diff = float((a[ka].double() - b[kb].double()).abs().max())
        print(f"[label smoothing] fused vs two-step M {M} V {V} eps {eps} {kr}: max |diff| {diff:.3e} (sum of bounds {bound:.3e})")
        assert diff <= bound, (kr, diff, bound)
    assert torch.equal(a["argmax"], b["argmax"])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev, L):
    """eps = 1, -0.1 and nan are refused before a launch (the Python layers raise, the raw entries return CVC_E_BADARG and write
    nothing); a `done` made with another eps is refused"""
    from cvc import functional as F_
    M, K, V = 72, 64, 100
    g = torch.Generator().manual_seed(11)
    x, W, b = torch.randn(M, K, generator=g).to(dev), (torch.randn(V, K, generator=g) * 0.1).to(dev), torch.randn(V, generator=g).to(dev)
    t, w = torch.randint(0, V, (M,), generator=g).to(dev), torch.ones(M, device=dev)
    assert F_.vocab_head_nll_ok(x, W)
    F_.new_step()
    for bad in (1.0, -0.1, float("nan")):
        for call in (lambda: F_.vocab_head_nll(x, W, b, t, w, label_smoothing=bad), lambda: F_.vocab_nll(x @ W.t(), t, w, label_smoothing=bad),
                     lambda: F_.vocab_head_nll_compute(x, W, b, t, w, label_smoothing=bad),
                     lambda: F_.masked_nll_sum(torch.log_softmax(x @ W.t(), 1), t, w, label_smoothing=bad)):
            with pytest.raises(ValueError, match="label_smoothing"):
                call()
        out = torch.full((M, V), SENTINEL, device=dev)
        rows, sums = torch.full((2, M), SENTINEL, device=dev), torch.full((2,), SENTINEL, device=dev)
        lg = (x @ W.t()).contiguous()
        assert L.cvc_vocab_head_nll_ls_fwd(lg.data_ptr(), 1, 0, V, None, t.data_ptr(), w.data_ptr(), M, V, bad, out.data_ptr(), V, None,
                                           rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(), sums[1:].data_ptr(), _stream()) == BADARG
        assert L.cvc_vocab_nll_ls_fwd(lg.data_ptr(), t.data_ptr(), w.data_ptr(), M, V, bad, rows[1].data_ptr(), None, rows[0].data_ptr(),
                                      sums[0:].data_ptr(), None, None, _stream()) == BADARG
        assert L.cvc_vocab_nll_ls_bwd(lg.data_ptr(), rows[0].data_ptr(), t.data_ptr(), w.data_ptr(), sums.data_ptr(), M, V, bad,
                                      out.data_ptr(), _stream()) == BADARG
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((rows == SENTINEL).all()) and bool((sums == SENTINEL).all())
    for made, asked in ((0.1, 0.2), (0.1, 0.0), (0.0, 0.1)):
        done = F_.vocab_head_nll_compute(x, W, b, t, w, label_smoothing=made)
        with pytest.raises(RuntimeError, match="label_smoothing"):
            F_.vocab_head_nll(x, W, b, t, w, done, label_smoothing=asked)
    done = F_.vocab_head_nll_compute(x, W, b, t, w, label_smoothing=0.1)
    loss, amax, nll = F_.vocab_head_nll(x, W, b, t, w, done, label_smoothing=0.1, return_nll=True)
    assert torch.equal(loss, done[0]) and torch.equal(amax, done[1]) and torch.equal(nll, done[3])


# ------------------------------------------------------------------------------------------------ the functional layer under autograd
@pytest.mark.parametrize("V", [100, 97])
def test_functional_forms_under_autograd(dev, V):
    """F.vocab_head_nll (V = 100; V = 97 is a width it refuses), F.vocab_nll and log_softmax + F.masked_nll_sum with eps = 0.1 on the
    same x W^T + b: loss, unsmoothed loss and the gradients of x, W and b against fp64 autograd of the restatement.  The bound of
    the gradients is the one tests/test_gpu_train.py holds the training pass to: |err| <= 5e-4 |want| in norm."""
    from cvc import functional as F_
    M, K, eps = 72, 64, 0.1
    g = torch.Generator().manual_seed(V)
    x0, W0, b0 = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g) * 0.3, torch.randn(V, generator=g)
    target = torch.randint(0, V, (M,), generator=g)
    w = (torch.rand(M, generator=g) < 0.7).float()
    w[::9], target[::9] = 0.0, 0
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x0, W0, b0))
    z64 = xr @ Wr.t() + br
    lse = torch.logsumexp(z64, 1)
    ref = (w.double() * (lse - (1 - eps) * z64.gather(1, target[:, None]).squeeze(1) - (eps / V) * z64.sum(1))).sum()
    ref_nll = (w.double() * (lse - z64.gather(1, target[:, None]).squeeze(1))).sum().detach()
    (ref * 0.37).backward()
    z32 = x0 @ W0.t() + b0
    yard = abs(float(R.restate(z32, target, w, eps, torch.float32)["loss_sum"].double() - ref.detach()))
    bound = max(4.0 * yard, 4.0 * float(ref.detach()) * 2.0 ** -23)          # (floor: 4 fp32 ulps of the sum itself)
    forms = {"two-step": lambda x, W, b: F_.vocab_nll(F_.linear(x, W, b), target.to(dev), w.to(dev), label_smoothing=eps, return_nll=True),
             "log-prob": lambda x, W, b: (F_.masked_nll_sum(F_.log_softmax(F_.linear(x, W, b)), target.to(dev), w.to(dev), label_smoothing=eps),
                                          None, None)}
    if V % 4 == 0:
        forms["fused"] = lambda x, W, b: F_.vocab_head_nll(x, W, b, target.to(dev), w.to(dev), label_smoothing=eps, return_nll=True)
    else:
        assert not F_.vocab_head_nll_ok(x0.to(dev), W0.to(dev))
    for name, form in forms.items():
        F_.new_step()            # (operands derived from weights are kept per step and address: fresh tensors, fresh step)
        x, W, b = (t.to(dev).requires_grad_(True) for t in (x0, W0, b0))
        loss, _amax, nll = form(x, W, b)
        (loss * 0.37).sum().backward()
        err = abs(float(loss.detach().cpu().double() - ref.detach()))
        print(f"[label smoothing] functional {name} V {V}: loss |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e})")
        assert err <= bound, (name, err, bound)
        if nll is not None:
            assert abs(float(nll.cpu().double() - ref_nll)) <= max(4.0 * yard, 4.0 * float(ref_nll) * 2.0 ** -23) and not nll.requires_grad
        for got, want, what in ((x.grad, xr.grad, "x"), (W.grad, Wr.grad, "W"), (b.grad, br.grad, "b")):
            rel = float((got.cpu().double() - want).norm() / want.norm())
            print(f"[label smoothing] functional {name} V {V}: d{what} relative error {rel:.3e}")
            assert rel <= 5e-4, (name, what, rel)


# ------------------------------------------------------------------------------------------------ the model
def _dims(V):
    return dataclasses.replace(synth.CONFIGS["tiny"], B=12, R=64, A=32, E=32, V=V, T=6)


def _model(dev, d, eps, seed=5):
    from helpers import build_model, to_dev
    model = build_model(d, synth.hot_path_state_dict(d, seed), dev, label_smoothing=eps).train()
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
        for m in (model.critLM, model.xe_criterion):
            for n in ("from_head", "from_logits"):
                m.__dict__.pop(n, None)
    return out, calls


def _expected(model, call, eps):
    """the restatement on the logits a tapped criterion call saw (fp64 from its fp32 input; the head's product in fp64 when the call
    got the head's input) -> (loss64, nll64, fp32 yardstick of the loss)"""
    obj, name, a, k = call
    lm = obj is model.critLM
    target = (a[4] if name == "from_head" else a[3]) if lm else (a[2] if name == "from_head" else a[1])
    target = target.cpu()
    mask = R.text_mask(target)
    if k.get("t_major", False):
        tf, mf = target.t().reshape(-1), mask.t().reshape(-1)
    else:
        tf, mf = target.reshape(-1), mask.reshape(-1)
    x = a[0].detach().cpu()
    if name == "from_head":
        W, bias = model.logit.weight.detach().cpu(), model.logit.bias.detach().cpu()
        z64, z32 = x.double() @ W.double().t() + bias.double(), x @ W.t() + bias
    else:
        z64, z32 = x.double(), x
    loss, nll = R.masked_mean(z64, tf, mf, eps)
    yard = abs(float(R.masked_mean(z32, tf, mf, eps, torch.float32)[0].double() - loss))
    return float(loss), float(nll), yard


@pytest.mark.parametrize("V", [100, 97])
def test_model_losses_last_nll_routes_and_scst(dev, V):
    """A small synthetic model in training mode (dropout on, in-kernel masks of a fixed seed) at a width the fused head takes
    (V = 100, 72 rows) and at one it refuses (V = 97: the two-step fallback), eps = 0.1:
    lm_loss and lm_recon_loss are the restatement on the model's own logits; model.last_nll is the unsmoothed loss of a second pass
    with eps = 0 on the same masks; the gradients of logit.weight and of the attention LSTM's input matrix agree between the C-driven
    route (head_words -> from_head) and the eager route (from_logits); scst_loss has the same bits for eps = 0 and 0.1.
    Bounds: the losses 4 x the fp32 yardstick (the restatement in fp32 on the fp32 product) with a floor of 4 fp32 ulps of the value;
    last_nll against the second pass 4 ulps (the same logits, the same expression); the routes' gradients 5e-4 of the norm, the
    bound tests/test_gpu_train.py holds either route to against the oracle."""
    from cvc import train_loops, functional as F_
    eps = 0.1
    d = _dims(V)
    model, f, b = _model(dev, d, eps)
    assert model.label_smoothing == eps and model.xe_criterion.label_smoothing == eps
    out, calls = _one_pass(model, f, b)
    assert [c[1] for c in calls] == ["from_head", "from_head"] and len(out) == 5
    fused = F_.vocab_head_nll_ok(calls[0][2][0], model.logit.weight)
    assert fused == (V % 4 == 0)
    for i, name in ((0, "lm_loss"), (1, "lm_recon_loss")):
        got = float(out[0 if i == 0 else 4])
        want, want_nll, yard = _expected(model, calls[i], eps)
        bound = max(4.0 * yard, 4.0 * want * 2.0 ** -23)
        print(f"[label smoothing] model V {V} {name}: {got:.6f} vs {want:.6f}, |err| {abs(got - want):.3e} (yardstick {yard:.3e}, bound {bound:.3e}); "
              f"unsmoothed {want_nll:.6f}")
        assert abs(got - want) <= bound, (name, got, want, bound)
        if i == 0:
            nll = float(model.last_nll)
            assert abs(nll - want_nll) <= max(4.0 * yard, 4.0 * want_nll * 2.0 ** -23), (nll, want_nll)
            assert model.last_nll.dim() == 0 and not model.last_nll.requires_grad
    last_nll = model.last_nll.clone()
    (0.5 * out[0].mean() + 0.5 * out[4].mean()).backward()
    names = ("logit.weight", "decoder_core.att_lstm.weight_ih")
    P = dict(model.named_parameters())
    grads_c = {n: P[n].grad.clone() for n in names}
    # the eager route on the same masks
    train_loops.ENABLED = False
    try:
        out_e, calls_e = _one_pass(model, f, b)
    finally:
        train_loops.ENABLED = True
    assert [c[1] for c in calls_e] == ["from_logits", "from_logits"]
    (0.5 * out_e[0].mean() + 0.5 * out_e[4].mean()).backward()
    for n in names:
        rel = float((P[n].grad - grads_c[n]).norm() / grads_c[n].norm())
        print(f"[label smoothing] model V {V} d {n}: C-driven vs eager route relative difference {rel:.3e}")
        assert rel <= 5e-4, (n, rel)
    for i in (0, 4):
        assert float(out_e[i]) == pytest.approx(float(out[i]), rel=2e-5)
    # a second pass without smoothing on the same masks: its LM loss is what the smoothed pass left in last_nll
    model.label_smoothing = 0.0
    out0, _ = _one_pass(model, f, b)
    assert model.last_nll is None
    diff = abs(float(out0[0]) - float(last_nll))
    print(f"[label smoothing] model V {V}: last_nll {float(last_nll):.7f}, eps = 0 pass {float(out0[0]):.7f}, |diff| {diff:.3e}")
    assert diff <= 4.0 * float(out0[0]) * 2.0 ** -23
    # the self-critical loss ignores smoothing
    model.eval()
    dummy = torch.zeros(d.B, 1, 1, device=dev)
    g = torch.Generator().manual_seed(3)
    words = torch.randint(0, V, (d.B, d.T), generator=g).to(dev)
    reward, base = torch.rand(d.B, generator=g).to(dev), torch.rand(d.B, generator=g).to(dev)
    res = []
    for e in (0.0, eps):
        model.label_smoothing = e
        model.zero_grad(set_to_none=True)
        with torch.no_grad():
            enc = model.encode_clips(f, b["proposals"], b["num"], b["box_mask"], dummy, b["gt_bboxs"], b["frm_mask"], b["sample_idx"], f["pnt_mask"])
        loss, adv = model.scst_loss(enc, words, reward, base, 1)
        loss.backward()
        res.append((loss.detach().clone(), adv.clone(), P["logit.weight"].grad.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*res))


# ------------------------------------------------------------------------------------------------ the captured step
def test_captured_step_equals_eager_step(dev):
    """train_step_graphed with eps = 0.1 (3 warm-up steps, a capture, 3 replays) against 6 eager steps of a twin: the loss vectors
    [loss, lm, att2, cls, recon, unsmoothed NLL] of steps 4 .. 6 and the parameters after them are equal (eval-mode dropout: both
    deterministic; the same launches on the same kind of buffers)"""
    from helpers import make_opts, to_dev
    from cvc.model.captioner import DecodeAndGroundCaptionerGVDROI, PrecomputedRegionFeatures
    from cvc.trainer import Trainer, build_optimizer
    from cvc import opts as cvc_opts
    d, seed, eps = _dims(100), 5, 0.1
    vecs, finals = {}, {}
    for mode in ("eager", "graph"):
        o = cvc_opts.parse_opt([])
        for k, v in vars(make_opts(d, train_decoder_only=False, label_smoothing=eps)).items():
            setattr(o, k, v)
        o.xe_loss_weight, o.caption_consistency_loss_weight, o.learning_rate, o.batch_size = 0.5, 0.5, 2e-3, d.B
        model = DecodeAndGroundCaptionerGVDROI(o, roi_extractor=PrecomputedRegionFeatures(d.DET, d.G))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.hot_path_state_dict(d, seed).items()}, strict=False)
        model = model.to(dev).eval()
        f, b = to_dev(synth.clip_features(d, seed), dev), to_dev(synth.label_glue_batch(d, seed), dev)
        batch = (f, b["input_seq"], b["gt_seq"], b["num"].cpu(), b["proposals"], b["gt_bboxs"], b["box_mask"],
                 ["v_x_segment_%02d" % i for i in range(d.B)], torch.zeros(d.B, d.N, 1), b["frm_mask"], b["sample_idx"], f["pnt_mask"][:, 1:])
        tr = Trainer(o, None, model, build_optimizer(model, o, capturable=True), None, None)
        assert tr.label_smoothing == eps
        if mode == "eager":
            seq = [tr._core_step(tr._prepare(batch, True)).clone() for _ in range(6)]
            vecs[mode] = seq[3:]
        else:
            vecs[mode] = [tr.train_step_graphed(batch).clone() for _ in range(3)]
        torch.cuda.synchronize()
        finals[mode] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for i, (e, g) in enumerate(zip(vecs["eager"], vecs["graph"])):
        print(f"[label smoothing] captured step {i + 4}: eager {e.tolist()} graph {g.tolist()}")
        assert e.numel() == 6 and g.numel() == 6
        assert torch.equal(e, g), (e, g)
        assert float(g[5]) > 0 and float(g[5]) != float(g[1])   # the unsmoothed NLL beside the smoothed LM loss
    for k in finals["eager"]:
        assert torch.equal(finals["eager"][k], finals["graph"][k]), k


# ------------------------------------------------------------------------------------------------ the entry point
def test_main_entry_point_logs_the_unsmoothed_nll(tmp_path, capsys):
    """python -m cvc.main --label_smoothing 0.1: a cross-entropy epoch and a scheduled-sampling epoch (both smoothed); the display
    line and the histories carry the unsmoothed NLL per display interval, which differs from the smoothed LM loss"""
    import math
    import os
    import pickle
    from cvc import main as cvc_main
    rc = cvc_main.main(["--no_cfg", "--max_epochs", "2", "--batch_size", "4", "--synthetic_clips", "12", "--num_prop_per_frm", "7",
                        "--t_attn_size", "5", "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "4",
                        "--vis_encoding_size", "24", "--tensorboard", "0", "--disp_interval", "1", "--exp_name", "l", "--learning_rate", "0.001",
                        "--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/", "--id", "l1",
                        "--label_smoothing", "0.1", "--scheduled_sampling_start", "0", "--scheduled_sampling_increase_every", "1",
                        "--scheduled_sampling_increase_prob", "0.25"])
    assert rc == 0
    tr = cvc_main.LAST_TRAINER
    model = getattr(tr.model, "module", tr.model)
    assert tr.label_smoothing == pytest.approx(0.1) and model.label_smoothing == pytest.approx(0.1)
    assert sorted(tr.nll_history) == [0, 1] and all(len(v) == 2 for v in tr.nll_history.values())      # 12 clips / 4 per batch, the last dropped
    assert all(math.isfinite(x) and x > 0 for v in tr.nll_history.values() for x in v)
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Epoch: [")]
    assert len(lines) == 4 and all("\tNLL " in l for l in lines) and any("\tSampled " in l for l in lines)
    for l in lines:                                                # "LM Loss v (avg)" is the smoothed loss, "NLL v (avg)" the unsmoothed one
        lm = float(l.split("LM Loss ")[1].split()[0])
        nll = float(l.split("\tNLL ")[1].split()[0])
        assert lm != nll and abs(lm - nll) < 1.0
    hist = pickle.load(open(os.path.join(tmp_path, "l", "histories_l1.pkl"), "rb"))
    assert hist["nll_history"] == tr.nll_history
