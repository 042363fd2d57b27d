"""Word-level distillation in the vocabulary criterion on the GPU (csrc/distill.hip: cvc_vocab_head_nll_kd_fwd,
cvc_vocab_nll_kd_fwd / _bwd), against the fp64 restatement of tests/distill_ref.py.

Tolerance of the kernels: the reference is the restatement in fp64; the yardstick is the SAME restatement in fp32 on the CPU, on the
same case; a kernel's largest error may be 4 x the yardstick's largest error with a floor of 2^-20 (the convention of
tests/test_gpu_label_smoothing.py and tests/test_gpu_cider.py).  Every test prints its figures before it asserts."""
import pytest
import torch

import distill_ref as R
import label_smoothing_ref as LS

pytestmark = pytest.mark.gpu

SENTINEL = -777.0
KEYS = ("row_loss", "row_nll", "row_kd", "loss_sum", "nll_sum", "kd_sum", "pre")


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
    print(f"[distill] {label}: kernel max |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e})")
    assert err <= bound, (label, err, yard, bound)
    return err, bound


_CASES = {}


def _head_case(M, V, nparts, with_bias, seed=3):
    """K-slice slabs [nparts, M, V] and a bias whose fp32 sum, in the kernel's order (slab 0, 1, ..., then the bias), is the logits of
    R.case up to rounding; the references take THAT fp32 sum as their input.  The teacher rows of the w = 0 rows are NaN.  Made once
    per shape and shared -> (parts, bias, logits32, teacher, target, w)"""
    key = (M, V, nparts, with_bias, seed)
    if key not in _CASES:
        logits, teacher, target, w = R.case(M, V, seed)
        teacher[w == 0] = float("nan")
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
        _CASES[key] = (parts, bias, x, teacher, target, w)
    return _CASES[key]


_REFS = {}


def _refs(key, logits32, teacher, target, w, alpha, tau):
    k = (key, alpha, tau)
    if k not in _REFS:
        _REFS[k] = (R.restate(logits32, teacher, target, w, alpha, tau), R.restate(logits32, teacher, target, w, alpha, tau, torch.float32))
    return _REFS[k]


def _teacher_store(dev, teacher, pad, use_map):
    """the teacher rows as the entry points take them -> (storage on the device, ld_t, row map or None, rows in the storage).
    use_map: the rows are stored permuted among three more (filled with a value that would show), and an int32 map finds them"""
    M, V = teacher.shape
    ld_t = V + pad
    if not use_map:
        st = torch.full((M, ld_t), SENTINEL, device=dev)
        st[:, :V] = teacher.to(dev)
        return st, ld_t, None, M
    perm = torch.randperm(M + 3, generator=torch.Generator().manual_seed(M + V))[:M]
    st = torch.full((M + 3, ld_t), 55.0, device=dev)
    st[perm.to(dev), :V] = teacher.to(dev)
    return st, ld_t, perm.to(torch.int32).to(dev), M + 3


def _run_head(L, dev, parts, bias, target, w, teacher, alpha, tau, alias, use_map, graph=False):
    """a raw call of the fused form -> dict(pre [M, V], argmax, the three rows, the three sums).  alias: pre = slab 0 (ld = ld_pre = V,
    teacher ld_t = V), else ld = V + 4, ld_pre = V + 9, ld_t = V + 5 with sentinels around (checked here)"""
    nparts, M, V = parts.shape
    ld, ld_pre = (V, V) if alias else (V + 4, V + 9)
    pd = torch.full((nparts, M, ld), float("nan"), device=dev)
    pd[:, :, :V] = parts.to(dev)
    pre = pd[0] if alias else torch.full((M, ld_pre), SENTINEL, device=dev)
    bd, td, wd = (None if bias is None else bias.to(dev)), target.to(dev), w.to(dev)
    st, ld_t, rmap, t_rows = _teacher_store(dev, teacher, 0 if alias else 5, use_map)
    amax = torch.full((M,), -5, dtype=torch.int64, device=dev)
    rows = torch.full((3, M), SENTINEL, device=dev)
    sums = torch.full((3,), SENTINEL, device=dev)

    def call():
        return L.cvc_vocab_head_nll_kd_fwd(pd.data_ptr(), nparts, M * ld, ld, _ptr(bd), td.data_ptr(), wd.data_ptr(), st.data_ptr(), ld_t,
                                           _ptr(rmap), t_rows, M, V, float(alpha), float(tau), pre.data_ptr(), ld_pre, amax.data_ptr(),
                                           rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(), sums[1:].data_ptr(),
                                           rows[2].data_ptr(), sums[2:].data_ptr(), _stream())
    if graph:
        assert not alias                         # (a replay reads the slabs again)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            assert call() == 0
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            rc = call()
        assert rc == 0
        for t in (pre, rows, sums):
            t.fill_(SENTINEL)
        amax.fill_(-5)
        g.replay()
    else:
        assert call() == 0
    torch.cuda.synchronize()
    if not alias:
        assert bool((pre[:, V:] == SENTINEL).all())
        assert bool((st[:, V:] == (55.0 if use_map else SENTINEL)).all())
    return dict(pre=pre[:, :V].clone(), argmax=amax, row_loss=rows[0], row_nll=rows[1], row_kd=rows[2], loss_sum=sums[0], nll_sum=sums[1],
                kd_sum=sums[2])


def _run_two_step(L, dev, logits, target, w, teacher, alpha, tau, g, use_map=False):
    M, V = logits.shape
    x, t, wd = logits.to(dev), target.to(dev), w.to(dev)
    st, ld_t, rmap, t_rows = _teacher_store(dev, teacher, 3 if use_map else 0, use_map)
    stats = torch.full((5, M), SENTINEL, device=dev)
    amax = torch.full((M,), -5, dtype=torch.int64, device=dev)
    rows, sums = torch.full((3, M), SENTINEL, device=dev), torch.full((3,), SENTINEL, device=dev)
    rc = L.cvc_vocab_nll_kd_fwd(x.data_ptr(), t.data_ptr(), wd.data_ptr(), st.data_ptr(), ld_t, _ptr(rmap), t_rows, M, V, float(alpha),
                                float(tau), stats.data_ptr(), amax.data_ptr(), rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(),
                                sums[1:].data_ptr(), rows[2].data_ptr(), sums[2:].data_ptr(), _stream())
    assert rc == 0, rc
    d = torch.full((M, V), SENTINEL, device=dev)
    gd = torch.tensor([g], device=dev)
    rc = L.cvc_vocab_nll_kd_bwd(x.data_ptr(), stats.data_ptr(), t.data_ptr(), wd.data_ptr(), st.data_ptr(), ld_t, _ptr(rmap), t_rows,
                                gd.data_ptr(), M, V, float(alpha), float(tau), d.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(pre=d, argmax=amax, row_loss=rows[0], row_nll=rows[1], row_kd=rows[2], loss_sum=sums[0], nll_sum=sums[1], kd_sum=sums[2])


# ------------------------------------------------------------------------------------------------ the fused head kernel
@pytest.mark.parametrize("alpha,tau", R.SETTINGS)
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_fused_head_vs_fp64(dev, L, M, V, nparts, alpha, tau):
    """cvc_vocab_head_nll_kd_fwd: the three rows, the three sums and pre against fp64, argmax exact; with and without a bias; pre
    aliasing slab 0 and not (then ld > V, ld_pre != ld, ld_t > V, columns past V untouched); with and without a row map; weights 0
    (under a NaN teacher row: exact zeros), 1 and others; targets in the last column and in the first column of the last register
    slot; three runs bit-identical, and every variant has the bits of the first"""
    for with_bias in (True, False):
        parts, bias, logits32, teacher, target, w = _head_case(M, V, nparts, with_bias)
        r64, r32 = _refs((M, V, nparts, with_bias), logits32, teacher, target, w, alpha, tau)
        outs = [_run_head(L, dev, parts, bias, target, w, teacher, alpha, tau, alias, use_map)
                for alias, use_map in ((False, False), (True, False), (True, False), (True, True), (False, True))]
        for o in outs[1:]:
            for k in outs[0]:
                assert torch.equal(outs[0][k], o[k]), k
        o = outs[1]
        tag = f"head M {M} V {V} parts {nparts} alpha {alpha} tau {tau} bias {with_bias}"
        for k in KEYS:
            _check(f"{tag} {k}", o[k], r64[k], r32[k])
        assert torch.equal(o["argmax"].cpu(), r64["argmax"])
        dead = (w == 0).to(dev)
        for k in ("pre", "row_loss", "row_nll", "row_kd"):
            assert bool((o[k][dead] == 0).all()), k
        assert not bool(torch.isnan(o["pre"]).any())


@pytest.mark.parametrize("alpha,tau", R.SETTINGS)
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_two_step_form_vs_fp64_and_bit_equal_to_the_fused_form(dev, L, M, V, nparts, alpha, tau):
    """cvc_vocab_nll_kd_fwd / _bwd on materialised logits: forward values against fp64, d_logits = g pre against fp64 (g = -0.37; the
    yardstick is g x the restatement's pre in fp32), with a row map and without (the same bits); with g = 1 every output has the bits
    of the fused form on the same fp32 logits (one slab, no bias)"""
    logits, teacher, target, w = R.case(M, V, 5)
    teacher[w == 0] = float("nan")
    g = -0.37
    r64, r32 = R.restate(logits, teacher, target, w, alpha, tau), R.restate(logits, teacher, target, w, alpha, tau, torch.float32)
    o = _run_two_step(L, dev, logits, target, w, teacher, alpha, tau, g)
    again = _run_two_step(L, dev, logits, target, w, teacher, alpha, tau, g, use_map=True)
    assert all(torch.equal(o[k], again[k]) for k in o)
    tag = f"two-step M {M} V {V} alpha {alpha} tau {tau}"
    for k in KEYS[:-1]:
        _check(f"{tag} {k}", o[k], r64[k], r32[k])
    _check(f"{tag} d_logits", o["pre"], g * r64["pre"], torch.tensor(g) * r32["pre"])
    assert torch.equal(o["argmax"].cpu(), r64["argmax"])
    dead = (w == 0).to(dev)
    assert bool((o["pre"][dead] == 0).all()) and bool((o["row_loss"][dead] == 0).all()) and bool((o["row_kd"][dead] == 0).all())
    a = _run_head(L, dev, logits[None], None, target, w, teacher, alpha, tau, alias=True, use_map=False)
    b = _run_two_step(L, dev, logits, target, w, teacher, alpha, tau, 1.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("V", [97, 8192, 8197, 20000])
def test_two_step_form_takes_widths_the_fused_form_refuses(dev, L, V):
    """the fallback has no register cache: any V (odd, past 8192) against fp64"""
    logits, teacher, target, w = R.case(3, V, 9)
    r64, r32 = R.restate(logits, teacher, target, w, 0.3, 2.0), R.restate(logits, teacher, target, w, 0.3, 2.0, torch.float32)
    o = _run_two_step(L, dev, logits, target, w, teacher, 0.3, 2.0, 1.0)
    for k in KEYS:
        _check(f"two-step V {V} {k}", o[k], r64[k], r32[k])
    assert torch.equal(o["argmax"].cpu(), r64["argmax"])


# ------------------------------------------------------------------------------------------------ edge rows
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES[1:])
def test_teacher_entries_at_minus_inf(dev, L, M, V, nparts):
    """teacher columns at -inf (the first, one in the middle, the last; in one row the target's too): q = 0 there, no NaN anywhere,
    every value within the bound; pre at those columns is w ((1 - alpha) (p - hit) + alpha tau p_tau), which the reference states"""
    parts, bias, logits32, teacher, target, w = _head_case(M, V, nparts, True)
    teacher = teacher.clone()
    cols = [0, V // 2, V - 1]
    teacher[:, cols] = float("-inf")
    teacher[0, int(target[0])] = float("-inf")
    for alpha, tau in ((0.3, 2.0), (1.0, 1.0)):
        r64, r32 = R.restate(logits32, teacher, target, w, alpha, tau), R.restate(logits32, teacher, target, w, alpha, tau, torch.float32)
        o = _run_head(L, dev, parts, bias, target, w, teacher, alpha, tau, alias=True, use_map=False)
        t = _run_two_step(L, dev, logits32, target, w, teacher, alpha, tau, 1.0)
        for k in KEYS:
            assert not bool(torch.isnan(o[k]).any()) and bool(torch.isfinite(o[k]).all()), k
            _check(f"-inf teacher M {M} V {V} alpha {alpha} tau {tau} {k}", o[k], r64[k], r32[k])
            _check(f"-inf teacher two-step M {M} V {V} alpha {alpha} tau {tau} {k}", t[k], r64[k], r32[k])


@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_teacher_equal_to_the_student_has_no_kd(dev, L, M, V, nparts, tau):
    """s = z: the kd row is within the floor of 0 and pre is (1 - alpha) x the one-hot criterion's"""
    parts, bias, logits32, _teacher, target, w = _head_case(M, V, nparts, False)
    o = _run_head(L, dev, parts, bias, target, w, logits32, 0.3, tau, alias=True, use_map=False)
    worst = float(o["row_kd"].abs().max())
    print(f"[distill] s = z M {M} V {V} tau {tau}: max |row_kd| {worst:.3e} (floor {R.FLOOR:.3e})")
    assert worst <= R.FLOOR
    r64, r32 = R.restate(logits32, logits32, target, w, 0.3, tau), R.restate(logits32, logits32, target, w, 0.3, tau, torch.float32)
    _check(f"s = z M {M} V {V} tau {tau} pre", o["pre"], r64["pre"], r32["pre"])


@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("M,V,nparts", R.HEAD_CASES)
def test_label_smoothing_identity_against_the_smoothing_kernel(dev, L, M, V, nparts, eps):
    """s = log((1 - eps) onehot + eps / V), alpha = 1, tau = 1: the kd kernel's row_loss + w H(q) is cvc_vocab_head_nll_ls_fwd's row
    loss.  s is rounded to fp32, so the kernel distils from q' = softmax(fp32(s)); the identity is stated for what it was given:
    ls = row_loss + w H(q') + w sum_v (q' - q) log p, the last term (about 1e-8) evaluated in fp64.  Two independent kernels: the
    bound is the sum of their bounds (the 4 x yardstick rule of each on this case)."""
    parts, bias, logits32, _teacher, target, w = _head_case(M, V, nparts, True)
    s64, q = R.smoothed_teacher(target, V, eps)
    s32 = s64.float()
    qr = torch.softmax(s32.double(), 1)
    a = _run_head(L, dev, parts, bias, target, w, s32, 1.0, 1.0, alias=True, use_map=False)
    pd, bd, td, wd = parts.to(dev).contiguous(), bias.to(dev), target.to(dev), w.to(dev)
    rows, sums = torch.full((2, M), SENTINEL, device=dev), torch.full((2,), SENTINEL, device=dev)
    rc = L.cvc_vocab_head_nll_ls_fwd(pd.data_ptr(), nparts, M * V, V, bd.data_ptr(), td.data_ptr(), wd.data_ptr(), M, V, float(eps),
                                     pd.data_ptr(), V, None, rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(),
                                     sums[1:].data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    logp = torch.log_softmax(logits32.double(), 1)
    got = a["row_loss"].cpu().double() + w.double() * R.entropy(qr) + w.double() * ((qr - q) * logp).sum(1)
    kd64, kd32 = R.restate(logits32, s32, target, w, 1.0, 1.0), R.restate(logits32, s32, target, w, 1.0, 1.0, torch.float32)
    ls64, ls32 = LS.restate(logits32, target, w, eps), LS.restate(logits32, target, w, eps, torch.float32)
    bound = (max(4.0 * float((kd32["row_loss"].double() - kd64["row_loss"]).abs().max()), R.FLOOR) +
             max(4.0 * float((ls32["row_loss"].double() - ls64["row_loss"]).abs().max()), LS.FLOOR))
    diff = float((got - rows[0].cpu().double()).abs().max())
    print(f"[distill] label-smoothing identity M {M} V {V} eps {eps}: max |diff| {diff:.3e} (sum of bounds {bound:.3e})")
    assert diff <= bound, (diff, bound)
    # and each side against its own fp64 value
    _check(f"identity M {M} V {V} eps {eps} kd row_loss", a["row_loss"], kd64["row_loss"], kd32["row_loss"])
    _check(f"identity M {M} V {V} eps {eps} pre", a["pre"], ls64["pre"], ls32["pre"])


def test_a_mapped_row_outside_the_teacher_is_not_read(dev, L):
    """a row map entry outside [0, t_rows): that row's loss, kd and pre are NaN (nothing is read), the other rows keep their bits"""
    M, V = 7, 97
    logits, teacher, target, w = R.case(M, V, 4)
    teacher[w == 0] = 0.0
    good = _run_two_step(L, dev, logits, target, w, teacher, 0.3, 2.0, 1.0)
    x, t, wd, st = logits.to(dev), target.to(dev), w.to(dev), teacher.to(dev)
    rmap = torch.arange(M, dtype=torch.int32, device=dev)
    rmap[1], rmap[5] = -1, M
    pre = x.clone()
    rows, sums = torch.full((3, M), SENTINEL, device=dev), torch.full((3,), SENTINEL, device=dev)
    rc = L.cvc_vocab_head_nll_kd_fwd(pre.data_ptr(), 1, 0, V, None, t.data_ptr(), wd.data_ptr(), st.data_ptr(), V, rmap.data_ptr(), M, M, V, 0.3,
                                     2.0, pre.data_ptr(), V, None, rows[0].data_ptr(), sums[0:].data_ptr(), rows[1].data_ptr(),
                                     sums[1:].data_ptr(), rows[2].data_ptr(), sums[2:].data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    bad = torch.zeros(M, dtype=torch.bool, device=dev)
    bad[1] = bad[5] = True
    assert bool(torch.isnan(rows[0][bad]).all()) and bool(torch.isnan(rows[2][bad]).all()) and bool(torch.isnan(pre[bad]).all())
    assert torch.equal(rows[:, ~bad], torch.stack([good["row_loss"], good["row_nll"], good["row_kd"]])[:, ~bad])
    assert torch.equal(pre[~bad], good["pre"][~bad])


# ------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("M,V,nparts", [(7, 97, 3), (5, 8192, 1)])
def test_a_captured_call_replays_the_eager_bits(dev, L, M, V, nparts):
    parts, bias, logits32, teacher, target, w = _head_case(M, V, nparts, True)
    eager = _run_head(L, dev, parts, bias, target, w, teacher, 0.3, 2.0, alias=False, use_map=True)
    replay = _run_head(L, dev, parts, bias, target, w, teacher, 0.3, 2.0, alias=False, use_map=True, graph=True)
    for k in eager:
        assert torch.equal(eager[k], replay[k]), k


# ------------------------------------------------------------------------------------------------ the functional layer under autograd
@pytest.mark.parametrize("V", [100, 97])
def test_functional_forms_under_autograd(dev, V):
    """F.vocab_head_nll (V = 100; V = 97 is a width it refuses) and F.vocab_nll with distill= on the same x W^T + b: the mixed loss,
    the unmixed NLL and KD and the gradients of x, W and b against fp64 autograd of the restatement; the teacher rows as [M, V] and as
    the engine's [T, B, V].  The bound of the gradients is the one tests/test_gpu_train.py holds the training pass to: |err| <= 5e-4
    |want| in norm.  distill=None has the bits of a call without the argument."""
    from cvc import functional as F_
    M, K, alpha, tau = 72, 64, 0.3, 2.0
    g = torch.Generator().manual_seed(V)
    x0, W0, b0 = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g) * 0.3, torch.randn(V, generator=g)
    teacher = torch.randn(M, V, generator=g) * 2.0
    target = torch.randint(0, V, (M,), generator=g)
    w = (torch.rand(M, generator=g) < 0.7).float()
    w[::9], target[::9] = 0.0, 0
    xr, Wr, br = (t.double().requires_grad_(True) for t in (x0, W0, b0))
    z64 = xr @ Wr.t() + br
    q = torch.softmax(teacher.double() / tau, 1)
    kl = (q * (q.log() - torch.log_softmax(z64 / tau, 1))).sum(1)
    nll = torch.logsumexp(z64, 1) - z64.gather(1, target[:, None]).squeeze(1)
    ref = (w.double() * ((1 - alpha) * nll + alpha * tau * tau * kl)).sum()
    ref_nll, ref_kd = (w.double() * nll).sum().detach(), (w.double() * tau * tau * kl).sum().detach()
    (ref * 0.37).backward()
    z32 = x0 @ W0.t() + b0
    r32 = R.restate(z32, teacher, target, w, alpha, tau, torch.float32)
    yard = abs(float(r32["loss_sum"].double() - ref.detach()))
    bound = max(4.0 * yard, 4.0 * float(ref.detach()) * 2.0 ** -23)          # (floor: 4 fp32 ulps of the sum itself)
    td = teacher.to(dev)
    forms = {"two-step": lambda x, W, b, t: F_.vocab_nll(F_.linear(x, W, b), target.to(dev), w.to(dev), distill=(t, alpha, tau), return_nll=True,
                                                        return_kd=True)}
    if V % 4 == 0:
        forms["fused"] = lambda x, W, b, t: F_.vocab_head_nll(x, W, b, target.to(dev), w.to(dev), distill=(t, alpha, tau), return_nll=True,
                                                              return_kd=True)
    else:
        assert not F_.vocab_head_nll_ok(x0.to(dev), W0.to(dev))
    for name, form in forms.items():
        for rows in (td, td.view(6, 12, V)):
            F_.new_step()
            x, W, b = (t.to(dev).requires_grad_(True) for t in (x0, W0, b0))
            loss, _amax, nll_sum, kd_sum = form(x, W, b, rows)
            assert not nll_sum.requires_grad and not kd_sum.requires_grad
            (loss * 0.37).sum().backward()
            err = abs(float(loss.detach().cpu().double() - ref.detach()))
            print(f"[distill] functional {name} V {V}: loss |err| {err:.3e} (fp32 yardstick {yard:.3e}, bound {bound:.3e})")
            assert err <= bound, (name, err, bound)
            assert abs(float(nll_sum.cpu().double() - ref_nll)) <= max(4.0 * yard, 4.0 * float(ref_nll) * 2.0 ** -23)
            assert abs(float(kd_sum.cpu().double() - ref_kd)) <= max(4.0 * yard, 4.0 * float(ref_kd) * 2.0 ** -23)
            for got, want, what in ((x.grad, xr.grad, "x"), (W.grad, Wr.grad, "W"), (b.grad, br.grad, "b")):
                rel = float((got.cpu().double() - want).norm() / want.norm())
                print(f"[distill] functional {name} V {V}: d{what} relative error {rel:.3e}")
                assert rel <= 5e-4, (name, what, rel)
    # distill=None: the call of a caller that does not know the argument
    F_.new_step()
    xd, Wd, bd, t_, w_ = x0.to(dev), W0.to(dev), b0.to(dev), target.to(dev), w.to(dev)
    a = F_.vocab_nll(F_.linear(xd, Wd, bd), t_, w_)
    b_ = F_.vocab_nll(F_.linear(xd, Wd, bd), t_, w_, distill=None)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]) and len(a) == len(b_) == 2
    if V % 4 == 0:
        done = F_.vocab_head_nll_compute(xd, Wd, bd, t_, w_, distill=(td, alpha, tau))
        for other in ((td, 0.5, tau), (td, alpha, 1.0)):
            with pytest.raises(RuntimeError, match="distill"):
                F_.vocab_head_nll(xd, Wd, bd, t_, w_, done, distill=other)
        with pytest.raises(RuntimeError, match="distill"):
            F_.vocab_head_nll(xd, Wd, bd, t_, w_, done)
        loss, amax, nll_sum, kd_sum = F_.vocab_head_nll(xd, Wd, bd, t_, w_, done, distill=(td, alpha, tau), return_nll=True, return_kd=True)
        assert torch.equal(loss, done[0]) and torch.equal(amax, done[1]) and torch.equal(nll_sum, done[3]) and torch.equal(kd_sum, done[5])
