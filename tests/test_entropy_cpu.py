"""The entropy regulariser of the vocabulary criterion, the parts a machine without a GPU can check: the restatement of
tests/entropy_ref.py against torch autograd, its edge cases, flag parsing, the refusals that happen before any launch (host-side
argument checks of the three entry points included) and the block table.  The criteria themselves run on the GPU only (the package
has no CPU path), so their values are checked in tests/test_gpu_entropy.py."""
import argparse
import ctypes
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import entropy_ref as R

BADARG = -1
NAMES = ("cvc_vocab_head_nll_ent_fwd", "cvc_vocab_nll_ent_fwd", "cvc_vocab_nll_ent_bwd")


@pytest.mark.parametrize("V", R.SIZES)
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("beta", [0.05, -0.02])
def test_restatement_equals_torch_autograd(V, eps, beta):
    """values and gradients in fp64 against autograd of sum w CE(label_smoothing = eps) - beta sum m H, H = -sum p log p from
    log_softmax; bound 1e-12"""
    logits, target, w, m = R.case(9, V, 1)
    z = logits.double().requires_grad_(True)
    logp = F.log_softmax(z, 1)
    H = -(logp.exp() * logp).sum(1)
    rows = F.cross_entropy(z, target, reduction="none", label_smoothing=eps) * w.double() - beta * m.double() * H
    rows.sum().backward()
    r = R.restate(logits, target, w, m, eps, beta)
    errs = dict(row_loss=float((r["row_loss"] - rows.detach()).abs().max()), pre=float((r["pre"] - z.grad).abs().max()),
                H=float((r["H"] - H.detach()).abs().max()), loss_sum=abs(float(r["loss_sum"] - rows.detach().sum())),
                row_ent=float((r["row_ent"] - (m.double() * H.detach())).abs().max()))
    print(f"[entropy ref] V {V} eps {eps} beta {beta}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= 1e-12 for v in errs.values()), errs
    plain = F.cross_entropy(logits.double(), target, reduction="none") * w.double()
    assert float((r["row_nll"] - plain).abs().max()) <= 1e-12
    assert torch.equal(r["argmax"], logits.double().argmax(1))
    dead = (w == 0) & (m == 0)
    assert bool(dead.any()) and bool((r["pre"][dead] == 0).all()) and bool((r["row_loss"][dead] == 0).all()) and bool((r["row_ent"][dead] == 0).all())
    only_entropy = (w == 0) & (m != 0)                     # advantage 0 on a step that counts: the entropy term alone
    assert bool(only_entropy.any()) and bool((r["row_nll"][only_entropy] == 0).all()) and bool((r["row_loss"][only_entropy] != 0).all())


def test_rows_with_minus_inf_logits_stay_finite():
    """columns at -inf add exactly 0 to H and get an exactly zero gradient; everything else equals the row without those columns"""
    for V in (97, 1000):
        logits, target, w, m = R.case(9, V, 2)
        cols = R.minus_inf_columns(V, target)
        assert len(cols) == 2
        z = logits.clone()
        z[:, cols] = float("-inf")
        keep = [c for c in range(V) if c not in cols]
        tmap = torch.full((V,), -1, dtype=torch.int64)
        tmap[keep] = torch.arange(len(keep))
        for dtype in (torch.float64, torch.float32):
            r = R.restate(z, target, w, m, 0.0, 0.05, dtype)
            q = R.restate(z[:, keep], tmap[target], w, m, 0.0, 0.05, dtype)
            for k in ("H", "row_loss", "row_ent", "row_nll", "pre", "loss_sum", "ent_sum"):
                assert bool(torch.isfinite(r[k]).all()), (k, dtype)
            assert bool((r["pre"][:, cols] == 0).all())
            tol = 1e-12 if dtype == torch.float64 else 1e-5
            assert float((r["H"] - q["H"]).abs().max()) <= tol and float((r["pre"][:, keep] - q["pre"]).abs().max()) <= tol
            assert float((r["row_loss"] - q["row_loss"]).abs().max()) <= tol


def test_uniform_and_one_hot_rows():
    for V in R.SIZES:
        t, one = torch.zeros(2, dtype=torch.int64), torch.ones(2)
        H = R.restate(torch.full((2, V), 0.37), t, one, one, 0.0, 0.05)["H"]
        assert float((H - math.log(V)).abs().max()) <= 1e-12
        z = torch.zeros(2, V)
        z[0, 0], z[1, V - 1] = 60.0, 1000.0                # nearly and (in floating point) exactly one-hot
        for dtype in (torch.float64, torch.float32):
            r = R.restate(z, t, one, one, 0.0, 0.05, dtype)
            assert bool((r["H"] >= 0).all()) and float(r["H"].max()) < 1e-19 and bool(torch.isfinite(r["pre"]).all())


def test_fp32_yardstick_is_of_the_size_the_bound_assumes():
    """the CPU guard of the GPU cases: the restatement alone, in fp32, on the kernel cases -- a few fp32 ulps of the values, never 0
    where the values are not, so that 4 x it (floor 2^-20) is a bound a correct fp32 kernel meets and a wrong one does not"""
    for (M, V, _), (eps, beta) in ((c, s) for c in R.HEAD_CASES for s in R.SETTINGS):
        logits, target, w, m = R.case(M, V, 3)
        r64, r32 = R.restate(logits, target, w, m, eps, beta), R.restate(logits, target, w, m, eps, beta, torch.float32)
        for k, cap in (("row_loss", 2e-5), ("row_ent", 2e-5), ("pre", 2e-6), ("row_nll", 2e-5)):
            yard = float((r32[k].double() - r64[k]).abs().max())
            bound = max(4.0 * yard, R.FLOOR)
            print(f"[entropy ref] M {M} V {V} eps {eps} beta {beta} {k}: fp32 yardstick {yard:.2e}, bound {bound:.2e}")
            assert yard < cap and yard <= bound
        assert float((r32["row_loss"].double() - r64["row_loss"]).abs().max()) > 0


def test_flag_parsing_and_refusals():
    from cvc import main as cvc_main
    p = cvc_main.build_parser()
    o = p.parse_args([])
    assert not any(hasattr(o, k) for k in ("confidence_penalty", "scst_entropy", "log_entropy"))      # off: no key at all
    o = p.parse_args(["--confidence_penalty", "0.05", "--scst_entropy", "-0.02", "--log_entropy"])
    assert o.confidence_penalty == pytest.approx(0.05) and o.scst_entropy == pytest.approx(-0.02) and o.log_entropy is True
    cvc_main.check_entropy_flags(o)
    cvc_main.check_entropy_flags(p.parse_args([]))
    for flag in ("--confidence_penalty", "--scst_entropy"):
        for bad in ("nan", "inf", "-inf"):
            with pytest.raises(SystemExit, match=flag[2:]):
                cvc_main.main([flag + "=" + bad, "--no_cfg"])   # (ends before any set-up: no GPU is asked for)


def test_python_layers_refuse_bad_values_before_touching_a_tensor():
    from cvc import functional as F_, hip
    from cvc.misc import utils
    x, W = torch.zeros(3, 8), torch.zeros(8, 8)
    t, w = torch.zeros(3, dtype=torch.int64), torch.ones(3)
    for bad in (float("nan"), float("inf"), float("-inf"), "x", None):
        with pytest.raises(ValueError, match="entropy_beta"):
            hip.check_entropy_beta(bad)
    assert hip.check_entropy_beta(0) == 0.0 and hip.check_entropy_beta(-0.02) == -0.02 and hip.check_entropy_beta(3) == 3.0
    for bad in (float("nan"), float("inf")):
        # (CPU tensors: a launch attempt would raise RuntimeError "must live on the GPU" instead)
        with pytest.raises(ValueError, match="entropy_beta"):
            F_.vocab_nll(x, t, w, entropy_beta=bad, entropy_weight=w)
        with pytest.raises(ValueError, match="entropy_beta"):
            F_.vocab_head_nll(x, W, None, t, w, entropy_beta=bad, entropy_weight=w)
        with pytest.raises(ValueError, match="entropy_beta"):
            F_.vocab_head_nll_compute(x, W, None, t, w, entropy_beta=bad, entropy_weight=w)
        with pytest.raises(ValueError, match="confidence_penalty"):
            utils.LanguageCriterion(confidence_penalty=bad)
        with pytest.raises(ValueError, match="confidence_penalty"):
            utils.LMCriterion(argparse.Namespace(vocab_size=8, confidence_penalty=bad))
    # the entropy needs its weight, one per row
    with pytest.raises(ValueError, match="entropy_weight"):
        F_.vocab_nll(x, t, w, entropy_beta=0.05)
    with pytest.raises(ValueError, match="entropy_weight"):
        F_.vocab_head_nll(x, W, None, t, w, return_entropy=True)
    with pytest.raises(ValueError, match="entropy_weight"):
        F_.vocab_nll(x, t, w, entropy_beta=0.05, entropy_weight=torch.ones(4))
    # the criteria read opt.confidence_penalty; a constructor argument wins; no option = None (off)
    o = argparse.Namespace(vocab_size=8, confidence_penalty=0.2)
    assert utils.LMCriterion(o).confidence_penalty == 0.2 and utils.LMCriterion(o, confidence_penalty=0.0).confidence_penalty == 0.0
    assert utils.LanguageCriterion(o).confidence_penalty == 0.2 and utils.LanguageCriterion().confidence_penalty is None
    assert utils.LMCriterion(argparse.Namespace(vocab_size=8)).confidence_penalty is None
    assert utils.LMCriterion(o).last_entropy is None and utils.LanguageCriterion(o).last_entropy is None
    # with or without the term, CPU tensors are refused as ever: there is no library fall-back
    for kw in ({}, dict(entropy_beta=0.05, entropy_weight=w), dict(entropy_weight=w, return_entropy=True)):
        with pytest.raises(RuntimeError, match="GPU"):
            F_.vocab_nll(x, t, w, **kw)


def test_a_done_made_with_another_beta_is_refused():
    """the opaque `done` carries beta next to eps: (loss, argmax, pre, nll, eps, entropy, beta); one made with another value of
    either, or without the entropy form, is refused before anything is launched"""
    from cvc import functional as F_
    x, W = torch.zeros(3, 8), torch.zeros(8, 8)
    t, w = torch.zeros(3, dtype=torch.int64), torch.ones(3)
    one = torch.zeros(1)
    with_beta = (one, t, torch.zeros(3, 8), one, 0.0, one, 0.05)
    plain, smoothed = (one, t, torch.zeros(3, 8)), (one, t, torch.zeros(3, 8), one, 0.1)
    for done, kw in ((with_beta, dict(entropy_beta=0.02, entropy_weight=w)), (with_beta, dict(entropy_beta=0.0, entropy_weight=w)),
                     (with_beta, {}), (plain, dict(entropy_beta=0.05, entropy_weight=w)),
                     (smoothed, dict(label_smoothing=0.1, entropy_beta=0.05, entropy_weight=w)),
                     (plain, dict(entropy_weight=w, return_entropy=True))):
        with pytest.raises(RuntimeError, match="entropy_beta"):
            F_.vocab_head_nll(x, W, None, t, w, done, **kw)
    with pytest.raises(RuntimeError, match="label_smoothing"):
        F_.vocab_head_nll(x, W, None, t, w, with_beta, label_smoothing=0.1, entropy_beta=0.05, entropy_weight=w)


def test_blocks_are_declared_resolve_and_are_not_exported():
    from cvc import hip, ops
    lib = hip.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "cvc_hip_blocks.h")).read()
    for n, nargs in zip(NAMES, (23, 18, 13)):
        assert n in hip.BLOCKS and n in hip.SIGNATURES and len(hip.SIGNATURES[n]) == nargs
        decl = re.search(r"\bint %s\(([^;]*)\);" % n, header)
        assert decl is not None, f"{n} is not declared in include/cvc_hip_blocks.h"
        assert len(decl.group(1).split(",")) == nargs, n
        assert lib.cvc_block(n.encode()), n
    raw = ctypes.CDLL(hip.LIB_PATH)
    for n in NAMES:
        assert not hasattr(raw, n), f"{n} is a building block: not an exported symbol"
    assert len(ops.REGISTERED) == 13 and not any("ent" in n.split("_") for n in ops.REGISTERED)


def test_entry_points_refuse_on_the_host():
    """null pointers, beta not finite, eps outside [0, 1), V past the register cache, short leading dimensions, one of row_nll /
    nll_sum without the other: CVC_E_BADARG before any launch (no GPU here: a launch attempt would not return -1)"""
    from cvc import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok = dict(parts=p, nparts=1, stride=0, ld=8, bias=None, target=p, w=p, m=p, M=2, V=8, eps=0.1, beta=0.05, pre=p, ld_pre=8, amax=None,
              row_loss=p, loss_sum=p, row_nll=None, nll_sum=None, row_ent=p, ent_sum=p, row_lo=p)

    def head(**kw):
        a = {**ok, **kw}
        return lib.cvc_vocab_head_nll_ent_fwd(a["parts"], a["nparts"], a["stride"], a["ld"], a["bias"], a["target"], a["w"], a["m"], a["M"],
                                              a["V"], a["eps"], a["beta"], a["pre"], a["ld_pre"], a["amax"], a["row_loss"], a["loss_sum"],
                                              a["row_nll"], a["nll_sum"], a["row_ent"], a["ent_sum"], a["row_lo"], None)

    def fwd(**kw):
        a = {**ok, "lse": p, **kw}
        return lib.cvc_vocab_nll_ent_fwd(a["parts"], a["target"], a["w"], a["m"], a["M"], a["V"], a["eps"], a["beta"], a["lse"], a["amax"],
                                         a["row_loss"], a["loss_sum"], a["row_nll"], a["nll_sum"], a["row_ent"], a["ent_sum"], a["row_lo"], None)

    def bwd(**kw):
        a = {**ok, "lse": p, "g": p, "d": p, **kw}
        return lib.cvc_vocab_nll_ent_bwd(a["parts"], a["lse"], a["target"], a["w"], a["m"], a["row_ent"], a["g"], a["M"], a["V"], a["eps"],
                                         a["beta"], a["d"], None)
    for call in (head, fwd, bwd):
        for b in (float("nan"), float("inf"), float("-inf")):
            assert call(beta=b) == BADARG, (call.__name__, b)
        for e in (1.0, -0.1, float("nan"), 1.5):
            assert call(eps=e) == BADARG, (call.__name__, e)
        for kw in (dict(parts=None), dict(target=None), dict(w=None), dict(m=None), dict(row_ent=None), dict(M=0), dict(V=0)):
            assert call(**kw) == BADARG, (call.__name__, kw)
    for kw in (dict(pre=None), dict(row_loss=None), dict(loss_sum=None), dict(ent_sum=None), dict(row_lo=None), dict(V=8193, ld=8200, ld_pre=8200), dict(ld=7),
               dict(ld_pre=7), dict(nparts=0), dict(row_nll=p), dict(nll_sum=p)):
        assert head(**kw) == BADARG, kw
    for kw in (dict(lse=None), dict(row_loss=None), dict(loss_sum=None), dict(ent_sum=None), dict(row_lo=None), dict(row_nll=p), dict(nll_sum=p)):
        assert fwd(**kw) == BADARG, kw
    for kw in (dict(lse=None), dict(g=None), dict(d=None)):
        assert bwd(**kw) == BADARG, kw
