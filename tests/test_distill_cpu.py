"""Word-level distillation in the vocabulary criterion, the parts a machine without a GPU can check: the restatement of
tests/distill_ref.py against torch autograd, the label-smoothing identity, flag parsing, the refusals that happen before any launch
(host-side argument checks of the three entry points included), the `done` tuple, keep_rows outside the forced mode and the block
table.  The criteria themselves run on the GPU only (the package has no CPU path): tests/test_gpu_distill.py,
tests/test_gpu_distill_train.py."""
import argparse
import ctypes
import os
import re

import pytest
import torch

import distill_ref as R
import label_smoothing_ref as LS

BADARG = -1
NAMES = ("cvc_vocab_head_nll_kd_fwd", "cvc_vocab_nll_kd_fwd", "cvc_vocab_nll_kd_bwd")


@pytest.mark.parametrize("alpha,tau", R.SETTINGS + [(0.0, 1.5), (0.6, 0.5)])
@pytest.mark.parametrize("V", [5, 97, 257, 1000])
def test_restatement_pre_equals_torch_autograd(V, alpha, tau):
    """distill_ref's pre is torch autograd's fp64 gradient of its own row_loss, written out independently here (F.kl_div and
    F.cross_entropy); the values agree too.  Bound 1e-12."""
    import torch.nn.functional as F
    logits, teacher, target, w = R.case(9, V, 1)
    z = logits.double().requires_grad_(True)
    q = F.softmax(teacher.double() / tau, 1)
    kl = F.kl_div(F.log_softmax(z / tau, 1), q, reduction="none").sum(1)
    rows = w.double() * ((1 - alpha) * F.cross_entropy(z, target, reduction="none") + alpha * tau * tau * kl)
    rows.sum().backward()
    r = R.restate(logits, teacher, target, w, alpha, tau)
    errs = dict(row_loss=float((r["row_loss"] - rows.detach()).abs().max()), pre=float((r["pre"] - z.grad).abs().max()),
                row_kd=float((r["row_kd"] - (w.double() * tau * tau * kl.detach())).abs().max()),
                loss_sum=abs(float(r["loss_sum"] - rows.detach().sum())))
    print(f"[distill ref] V {V} alpha {alpha} tau {tau}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1e-12 for v in errs.values()), errs
    assert torch.equal(r["argmax"], logits.double().argmax(1))
    dead = w == 0
    assert bool(dead.any()) and bool((r["pre"][dead] == 0).all()) and bool((r["row_loss"][dead] == 0).all())
    assert bool((r["row_kd"][~dead] > 0).all())


@pytest.mark.parametrize("eps", [0.1, 0.5])
@pytest.mark.parametrize("V", LS.SIZES)
def test_label_smoothing_is_distillation_from_the_smoothed_one_hot(V, eps):
    """s = log((1 - eps) onehot + eps / V), alpha = 1, tau = 1: row_loss + w H(q) is label_smoothing_ref's row loss and pre is its pre
    (fp64, bound 1e-11: sums over up to 8192 columns)"""
    logits, target, w = LS.case(9, V, 2)
    s, q = R.smoothed_teacher(target, V, eps)
    r = R.restate(logits, s, target, w, 1.0, 1.0)
    want = LS.restate(logits, target, w, eps)
    got = r["row_loss"] + w.double() * R.entropy(q)
    err = float((got - want["row_loss"]).abs().max())
    err_pre = float((r["pre"] - want["pre"]).abs().max())
    print(f"[distill ref] V {V} eps {eps}: row_loss + w H(q) vs label smoothing {err:.2e}, pre {err_pre:.2e}")
    assert err <= 1e-11 and err_pre <= 1e-12
    assert float((r["row_nll"] - want["row_nll"]).abs().max()) <= 1e-12


def test_edge_rows_of_the_restatement():
    """a teacher entry at -inf is q = 0 and adds an exact 0; a w = 0 row is exact zeros under a NaN teacher row; s = z gives kd = 0"""
    logits, teacher, target, w = R.case(9, 97, 3)
    t2 = teacher.clone()
    t2[:, [0, 40, 96]] = float("-inf")
    t2[2] = float("nan")                                     # (row 2 has w = 0)
    for dtype in (torch.float64, torch.float32):
        r = R.restate(logits, t2, target, w, 0.3, 2.0, dtype)
        for k in ("row_loss", "row_kd", "pre"):
            assert bool(torch.isfinite(r[k]).all()), (k, dtype)
        assert bool((r["pre"][2] == 0).all()) and float(r["row_kd"][2]) == 0.0
        same = R.restate(logits, logits, target, w, 1.0, 2.0, dtype)
        assert float(same["row_kd"].abs().max()) <= (1e-12 if dtype == torch.float64 else R.FLOOR)


def test_fp32_yardstick_is_of_the_size_the_bound_assumes():
    """the CPU guard of the GPU cases: the restatement alone, in fp32, on the kernel cases -- a few fp32 ulps of the values, so that
    4 x it (floor 2^-20) is a bound a correct fp32 kernel meets and a wrong one does not"""
    for (M, V, _), (alpha, tau) in ((c, s) for c in R.HEAD_CASES for s in R.SETTINGS):
        logits, teacher, target, w = R.case(M, V, 3)
        r64, r32 = R.restate(logits, teacher, target, w, alpha, tau), R.restate(logits, teacher, target, w, alpha, tau, torch.float32)
        for k, cap in (("row_loss", 1e-4), ("row_kd", 1e-4), ("pre", 4e-6), ("row_nll", 2e-5)):
            yard = float((r32[k].double() - r64[k]).abs().max())
            print(f"[distill ref] M {M} V {V} alpha {alpha} tau {tau} {k}: fp32 yardstick {yard:.2e}, bound {max(4 * yard, R.FLOOR):.2e}")
            assert yard < cap, (k, yard)


# ------------------------------------------------------------------------------------------------ refusals before any launch
def _flag_opts(argv):
    from cvc import main as cvc_main
    return cvc_main.build_parser().parse_args(argv)


def test_flags_absent_add_no_option_key():
    o = _flag_opts([])
    assert not any(k.startswith("distill") for k in vars(o))
    from cvc import main as cvc_main
    assert cvc_main.check_distill_flags(o) is None


def test_flag_parsing_and_refusals(tmp_path):
    from cvc import main as cvc_main
    a, b = tmp_path / "a.pth", tmp_path / "b.pth"
    a.write_bytes(b"")
    b.write_bytes(b"")
    both = "%s,%s" % (a, b)
    got = cvc_main.check_distill_flags(_flag_opts(["--distill_from", both]))
    assert got == dict(paths=[str(a), str(b)], weights=None, combine="prob", alpha=0.5, tau=1.0)
    got = cvc_main.check_distill_flags(_flag_opts(["--distill_from", str(a), "--distill_weights", "2", "--distill_combine", "logprob",
                                                   "--distill_alpha", "1", "--distill_temperature", "2.5"]))
    assert got == dict(paths=[str(a)], weights=[2.0], combine="logprob", alpha=1.0, tau=2.5)
    # every refusal ends the run through main() before any set-up (no GPU is asked for)
    base = ["--no_cfg", "--distill_from", both]
    for extra, word in ((["--distill_alpha", "1.5"], "distill_alpha"), (["--distill_alpha", "-0.1"], "distill_alpha"),
                        (["--distill_alpha", "nan"], "distill_alpha"), (["--distill_temperature", "0"], "distill_temperature"),
                        (["--distill_temperature", "-1"], "distill_temperature"), (["--distill_temperature", "inf"], "distill_temperature"),
                        (["--distill_temperature", "nan"], "distill_temperature"), (["--label_smoothing", "0.1"], "label_smoothing"),
                        (["--confidence_penalty", "0.05"], "confidence_penalty"), (["--scheduled_sampling_start", "0"], "scheduled sampling"),
                        (["--distill_weights", "1"], "distill_weights"), (["--distill_weights", "1,x"], "distill_weights"),
                        (["--distill_weights", "1,-1"], "distill_weights")):
        with pytest.raises(SystemExit, match=word):
            cvc_main.main(base + extra)
    for lone in (["--distill_weights", "1,1"], ["--distill_combine", "prob"], ["--distill_alpha", "0.5"], ["--distill_temperature", "1"]):
        with pytest.raises(SystemExit, match="need --distill_from"):
            cvc_main.main(["--no_cfg"] + lone)
    with pytest.raises(SystemExit, match="no such checkpoint file"):
        cvc_main.main(["--no_cfg", "--distill_from", str(tmp_path / "missing.pth")])
    with pytest.raises(SystemExit, match="at most 8 members"):
        cvc_main.main(["--no_cfg", "--distill_from", ",".join([str(a)] * 9)])
    with pytest.raises(SystemExit, match="names no checkpoint"):
        cvc_main.main(["--no_cfg", "--distill_from", ","])
    # a teacher of another vocabulary: the member check of --ensemble under this flag's name
    ref = {"embed.0.weight": torch.zeros(10, 4), "logit.weight": torch.zeros(10, 4)}
    with pytest.raises(SystemExit, match="--distill_from: .* different vocabulary"):
        cvc_main.check_member_state("t.pth", {"embed.0.weight": torch.zeros(11, 4), "logit.weight": torch.zeros(11, 4)}, ref,
                                    flag="--distill_from")


def test_python_layers_refuse_before_touching_a_tensor():
    from cvc import functional as F_, hip
    from cvc.misc import utils
    x, W = torch.zeros(3, 8), torch.zeros(8, 8)
    t, w = torch.zeros(3, dtype=torch.int64), torch.ones(3)
    rows = torch.zeros(3, 8)
    for bad in (-0.1, 1.5, float("nan"), "x", None):
        with pytest.raises(ValueError, match="alpha"):
            hip.check_distill_scalars(bad, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="tau"):
            hip.check_distill_scalars(0.5, bad)
    assert hip.check_distill_scalars(0, 2) == (0.0, 2.0) and hip.check_distill_scalars(1, 0.5) == (1.0, 0.5)
    for call in (lambda **kw: F_.vocab_head_nll(x, W, None, t, w, **kw), lambda **kw: F_.vocab_nll(x, t, w, **kw),
                 lambda **kw: F_.vocab_head_nll_compute(x, W, None, t, w, **kw)):
        with pytest.raises(ValueError, match="alpha"):
            call(distill=(rows, 1.5, 1.0))
        with pytest.raises(ValueError, match="tau"):
            call(distill=(rows, 0.5, 0.0))
        with pytest.raises(ValueError, match="label_smoothing"):
            call(distill=(rows, 0.5, 1.0), label_smoothing=0.1)
        with pytest.raises(ValueError, match="entropy_beta"):
            call(distill=(rows, 0.5, 1.0), entropy_beta=0.05, entropy_weight=w)
        with pytest.raises(ValueError, match="teacher_rows"):
            call(distill=(torch.zeros(3, 9), 0.5, 1.0))
        with pytest.raises(ValueError, match="teacher rows"):
            call(distill=(torch.zeros(2, 8), 0.5, 1.0))
        with pytest.raises(ValueError, match="row_map"):
            call(distill=(rows, 0.5, 1.0, torch.zeros(3, dtype=torch.int64)))
    with pytest.raises(ValueError, match="return_kd"):
        F_.vocab_head_nll(x, W, None, t, w, return_kd=True)
    with pytest.raises(ValueError, match="return_kd"):
        F_.vocab_nll(x, t, w, return_kd=True)
    # the criteria: a self-critical call (row_weight) is not distilled; the teacher rows are [T, B, V]
    target = torch.zeros(3, 2, dtype=torch.int64)
    xs = torch.zeros(6, 8)
    head = torch.nn.Linear(8, 8)
    kd = (torch.zeros(2, 3, 8), 0.5, 1.0)
    with pytest.raises(ValueError, match="row_weight"):
        utils._masked_nll_mean_from_head(xs, head.weight, head.bias, target, row_weight=torch.ones(6), distill=kd)
    with pytest.raises(ValueError, match="row_weight"):
        utils._masked_nll_mean_from_logits(xs, target, row_weight=torch.ones(6), distill=kd)
    with pytest.raises(ValueError, match="teacher_rows"):
        utils._masked_nll_mean_from_logits(xs, target, distill=(torch.zeros(3, 2, 8), 0.5, 1.0))
    with pytest.raises(ValueError, match="label_smoothing"):
        utils._masked_nll_mean_from_logits(xs, target, label_smoothing=0.1, distill=kd)
    with pytest.raises(ValueError, match="entropy_beta"):
        utils._masked_nll_mean_from_logits(xs, target, entropy_beta=0.05, distill=kd)
    assert utils.LMCriterion(argparse.Namespace(vocab_size=8)).last_kd is None
    # with or without a teacher, CPU tensors are refused as ever: there is no library fall-back
    with pytest.raises(RuntimeError, match="GPU"):
        F_.vocab_nll(x, t, w, distill=(rows, 0.5, 1.0), return_kd=True)


def test_a_done_made_with_another_alpha_or_tau_is_refused():
    """the opaque `done` carries alpha and tau: (loss, argmax, pre, nll, 0.0, kd, None, alpha, tau); one made with other values, or
    without a teacher, is refused before anything is launched -- and a distilled `done` is refused by a call without a teacher"""
    from cvc import functional as F_
    x, W = torch.zeros(3, 8), torch.zeros(8, 8)
    t, w = torch.zeros(3, dtype=torch.int64), torch.ones(3)
    rows, one = torch.zeros(3, 8), torch.zeros(1)
    kd_done = (one, t, torch.zeros(3, 8), one, 0.0, one, None, 0.5, 2.0)
    plain, smoothed = (one, t, torch.zeros(3, 8)), (one, t, torch.zeros(3, 8), one, 0.1)
    with_beta = (one, t, torch.zeros(3, 8), one, 0.0, one, 0.05)
    for done, kw in ((kd_done, dict(distill=(rows, 0.3, 2.0))), (kd_done, dict(distill=(rows, 0.5, 1.0))), (kd_done, {}),
                     (kd_done, dict(label_smoothing=0.1)), (plain, dict(distill=(rows, 0.5, 2.0))), (smoothed, dict(distill=(rows, 0.5, 2.0))),
                     (with_beta, dict(distill=(rows, 0.5, 2.0)))):
        with pytest.raises(RuntimeError, match="distill"):
            F_.vocab_head_nll(x, W, None, t, w, done, **kw)


def test_keep_rows_is_refused_outside_the_forced_mode():
    from cvc.decode import EnsembleOptions
    o = EnsembleOptions.resolve(2, 6, 100, forced_n=2, keep_rows=True)
    assert o.keep_rows is True and o.mode.forced
    assert EnsembleOptions.resolve(2, 6, 100, forced_n=2).keep_rows is False
    assert EnsembleOptions.resolve(1, 6, 100, forced_n=1, keep_rows=True).M == 1           # a single-checkpoint teacher
    for kw in ({}, dict(beam=3), dict(sample_n=2, temperature=1.0)):
        with pytest.raises(RuntimeError, match="keep_rows"):
            EnsembleOptions.resolve(2, 6, 100, keep_rows=True, **kw)
    with pytest.raises(RuntimeError, match="keep_rows"):
        EnsembleOptions.resolve(2, 6, 100, forced_n=2, keep_rows=1)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_blocks_are_declared_resolve_and_are_not_exported():
    from cvc import hip
    lib = hip.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cvc_hip_blocks.h")).read()
    for n, nargs in zip(NAMES, (25, 20, 15)):
        assert n in hip.BLOCKS and n in hip.SIGNATURES and len(hip.SIGNATURES[n]) == nargs
        decl = re.search(r"\bint %s\(([^;]*)\);" % n, header)
        assert decl is not None, f"{n} is not declared in include/cvc_hip_blocks.h"
        assert len(decl.group(1).split(",")) == nargs, n
        assert lib.cvc_block(n.encode()), n
    raw = ctypes.CDLL(hip.LIB_PATH)
    for n in NAMES:
        assert not hasattr(raw, n), f"{n} is a building block: not an exported symbol"


def test_entry_points_refuse_on_the_host():
    """null pointers, alpha outside [0, 1], tau not finite or <= 0, V past the register cache of the fused form, a teacher leading
    dimension < V (and ld, ld_pre), no teacher rows: CVC_E_BADARG before any launch (no GPU here: a launch attempt would not return -1)"""
    from cvc import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(parts=p, nparts=1, stride=0, ld=8, bias=None, target=p, w=p, teacher=p, ld_t=8, row_map=None, t_rows=2, M=2, V=8, alpha=0.5,
              tau=2.0, pre=p, ld_pre=8, amax=None, row_loss=p, loss_sum=p, row_nll=p, nll_sum=p, row_kd=p, kd_sum=p, stats=p, g=p, d=p)

    def head(**kw):
        a = {**ok, **kw}
        return lib.cvc_vocab_head_nll_kd_fwd(a["parts"], a["nparts"], a["stride"], a["ld"], a["bias"], a["target"], a["w"], a["teacher"],
                                             a["ld_t"], a["row_map"], a["t_rows"], a["M"], a["V"], a["alpha"], a["tau"], a["pre"], a["ld_pre"],
                                             a["amax"], a["row_loss"], a["loss_sum"], a["row_nll"], a["nll_sum"], a["row_kd"], a["kd_sum"], None)

    def fwd(**kw):
        a = {**ok, **kw}
        return lib.cvc_vocab_nll_kd_fwd(a["parts"], a["target"], a["w"], a["teacher"], a["ld_t"], a["row_map"], a["t_rows"], a["M"], a["V"],
                                        a["alpha"], a["tau"], a["stats"], a["amax"], a["row_loss"], a["loss_sum"], a["row_nll"], a["nll_sum"],
                                        a["row_kd"], a["kd_sum"], None)

    def bwd(**kw):
        a = {**ok, **kw}
        return lib.cvc_vocab_nll_kd_bwd(a["parts"], a["stats"], a["target"], a["w"], a["teacher"], a["ld_t"], a["row_map"], a["t_rows"],
                                        a["g"], a["M"], a["V"], a["alpha"], a["tau"], a["d"], None)
    for call in (head, fwd, bwd):
        for al in (-0.1, 1.5, float("nan"), float("inf")):
            assert call(alpha=al) == BADARG, (call.__name__, al)
        for ta in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            assert call(tau=ta) == BADARG, (call.__name__, ta)
        for kw in (dict(parts=None), dict(target=None), dict(w=None), dict(teacher=None), dict(ld_t=7), dict(t_rows=0), dict(M=0), dict(V=0)):
            assert call(**kw) == BADARG, (call.__name__, kw)
    for kw in (dict(pre=None), dict(row_loss=None), dict(loss_sum=None), dict(row_nll=None), dict(nll_sum=None), dict(row_kd=None),
               dict(kd_sum=None), dict(V=8193, ld=8200, ld_pre=8200, ld_t=8200), dict(ld=7), dict(ld_pre=7), dict(nparts=0),
               dict(nparts=2, stride=8)):
        assert head(**kw) == BADARG, kw
    for kw in (dict(stats=None), dict(row_loss=None), dict(loss_sum=None), dict(row_nll=None), dict(nll_sum=None), dict(row_kd=None),
               dict(kd_sum=None)):
        assert fwd(**kw) == BADARG, kw
    for kw in (dict(stats=None), dict(g=None), dict(d=None)):
        assert bwd(**kw) == BADARG, kw
