"""Label smoothing, the parts a machine without a GPU can check: the restatement of tests/label_smoothing_ref.py against
torch.nn.functional.cross_entropy(label_smoothing=), flag parsing, the refusals that happen before any launch (host-side argument
checks of the three entry points included), and the block table.  The criteria themselves run on the GPU only (the package has no
CPU path: tests/test_cabi.py::test_product_ops_refuse_cpu_tensors), so their values are checked in tests/test_gpu_label_smoothing.py."""
import argparse
import ctypes

import pytest
import torch
import torch.nn.functional as F

import label_smoothing_ref as R

BADARG = -1


@pytest.mark.parametrize("V", R.SIZES)
@pytest.mark.parametrize("eps", [0.0, 0.1, 0.5])
def test_restatement_equals_torch_cross_entropy(V, eps):
    """values and gradients in fp64: per-row losses (weights applied after), the sum, and d loss_sum / d logits = pre"""
    M = 9
    logits, target, w = R.case(M, V, 1)
    z = logits.double().requires_grad_(True)
    rows = F.cross_entropy(z, target, reduction="none", label_smoothing=eps)
    want = (rows * w.double()).sum()
    want.backward()
    r = R.restate(logits, target, w, eps)
    err = float((r["row_loss"] - (rows.detach() * w.double())).abs().max())
    err_g = float((r["pre"] - z.grad).abs().max())
    print(f"[label smoothing ref] V {V} eps {eps}: row_loss {err:.2e}, gradient {err_g:.2e}")
    assert err <= 1e-13 and err_g <= 1e-14 and abs(float(r["loss_sum"] - want.detach())) <= 1e-12
    plain = F.cross_entropy(logits.double(), target, reduction="none") * w.double()
    assert float((r["row_nll"] - plain).abs().max()) <= 1e-13
    assert torch.equal(r["argmax"], logits.double().argmax(1))
    assert bool((r["pre"][w == 0] == 0).all()) and bool((r["row_loss"][w == 0] == 0).all())


def test_fp32_yardstick_is_of_the_size_the_bound_assumes():
    """the yardstick (the restatement in fp32) on row_loss at logits of scale 4: a few fp32 ulps of the loss, never 0 at these sizes"""
    for V in R.SIZES:
        logits, target, w = R.case(9, V, 2)
        r64, r32 = R.restate(logits, target, w, 0.1), R.restate(logits, target, w, 0.1, torch.float32)
        yard = float((r32["row_loss"].double() - r64["row_loss"]).abs().max())
        print(f"[label smoothing ref] V {V}: fp32 yardstick on row_loss {yard:.2e}")
        assert 0 < yard < 2e-5


def test_flag_parsing_and_refusals():
    from cvc import main as cvc_main
    p = cvc_main.build_parser()
    assert p.parse_args([]).label_smoothing == 0.0
    assert p.parse_args(["--label_smoothing", "0.1"]).label_smoothing == pytest.approx(0.1)
    for bad in ("1", "1.5", "-0.1", "nan", "inf"):
        with pytest.raises(SystemExit, match="label_smoothing"):
            cvc_main.main(["--label_smoothing", bad, "--no_cfg"])          # (ends before any set-up: no GPU is asked for)
    cvc_main.check_label_smoothing_flag(0.0)
    cvc_main.check_label_smoothing_flag(0.999)


def test_python_layers_refuse_bad_values_before_touching_a_tensor():
    from cvc import functional as F_, hip
    from cvc.misc import utils
    x = torch.zeros(3, 8)
    t, w = torch.zeros(3, dtype=torch.int64), torch.ones(3)
    for bad in (1.0, -0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="label_smoothing"):
            hip.check_label_smoothing(bad)
    for bad in (1.0, -0.1, float("nan")):
        # (CPU tensors: a launch attempt would raise RuntimeError "must live on the GPU" instead)
        with pytest.raises(ValueError, match="label_smoothing"):
            F_.vocab_nll(x, t, w, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            F_.vocab_head_nll(x, torch.zeros(8, 8), None, t, w, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            F_.vocab_head_nll_compute(x, torch.zeros(8, 8), None, t, w, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            F_.masked_nll_sum(x, t, w, label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            utils.LanguageCriterion(label_smoothing=bad)
        with pytest.raises(ValueError, match="label_smoothing"):
            utils.LMCriterion(argparse.Namespace(vocab_size=8, label_smoothing=bad))
    assert hip.check_label_smoothing(0) == 0.0 and hip.check_label_smoothing(0.25) == 0.25
    # the criteria read opt.label_smoothing; a constructor argument wins; no option = 0
    o = argparse.Namespace(vocab_size=8, label_smoothing=0.2)
    assert utils.LMCriterion(o).label_smoothing == 0.2 and utils.LMCriterion(o, label_smoothing=0.3).label_smoothing == 0.3
    assert utils.LanguageCriterion(o).label_smoothing == 0.2 and utils.LanguageCriterion().label_smoothing == 0.0
    assert utils.LMCriterion(argparse.Namespace(vocab_size=8)).label_smoothing == 0.0
    # smoothed or not, CPU tensors are refused as ever: there is no library fall-back
    for eps in (0.0, 0.1):
        with pytest.raises(RuntimeError, match="GPU"):
            F_.vocab_nll(x, t, w, label_smoothing=eps)
        with pytest.raises(RuntimeError, match="GPU"):
            F_.masked_nll_sum(x, t, w, label_smoothing=eps)


def test_blocks_resolve_and_are_not_exported():
    from cvc import hip
    lib = hip.lib()
    names = ("cvc_vocab_head_nll_ls_fwd", "cvc_vocab_nll_ls_fwd", "cvc_vocab_nll_ls_bwd")
    for n in names:
        assert n in hip.BLOCKS and n in hip.SIGNATURES
        assert lib.cvc_block(n.encode()), n
    raw = ctypes.CDLL(hip.LIB_PATH)
    for n in names:
        assert not hasattr(raw, n), f"{n} is a building block: not an exported symbol"
    from cvc import ops
    assert len(ops.REGISTERED) == 13 and not any("ls" in n.split("_") for n in ops.REGISTERED)


def test_entry_points_refuse_on_the_host():
    """null pointers, eps outside [0, 1) or not finite, V past the register cache, short leading dimensions, one of row_nll /
    nll_sum without the other: CVC_E_BADARG before any launch (no GPU here: a launch attempt would not return -1)"""
    from cvc import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ok_head = dict(parts=p, nparts=1, stride=0, ld=8, bias=None, target=p, w=p, M=2, V=8, eps=0.1, pre=p, ld_pre=8, amax=None,
                   row_loss=p, loss_sum=p, row_nll=None, nll_sum=None)

    def head(**kw):
        a = {**ok_head, **kw}
        return lib.cvc_vocab_head_nll_ls_fwd(a["parts"], a["nparts"], a["stride"], a["ld"], a["bias"], a["target"], a["w"], a["M"], a["V"],
                                             a["eps"], a["pre"], a["ld_pre"], a["amax"], a["row_loss"], a["loss_sum"], a["row_nll"],
                                             a["nll_sum"], None)
    bad_eps = (1.0, -0.1, float("nan"), float("inf"), 1.5)
    for e in bad_eps:
        assert head(eps=e) == BADARG, e
    for kw in (dict(parts=None), dict(target=None), dict(w=None), dict(pre=None), dict(row_loss=None), dict(loss_sum=None), dict(V=8193, ld=8200, ld_pre=8200),
               dict(ld=7), dict(ld_pre=7), dict(M=0), dict(nparts=0), dict(row_nll=p), dict(nll_sum=p)):
        assert head(**kw) == BADARG, kw
    for e in bad_eps:
        assert lib.cvc_vocab_nll_ls_fwd(p, p, p, 2, 8, e, p, None, p, p, None, None, None) == BADARG
        assert lib.cvc_vocab_nll_ls_bwd(p, p, p, p, p, 2, 8, e, p, None) == BADARG
    assert lib.cvc_vocab_nll_ls_fwd(None, p, p, 2, 8, 0.1, p, None, p, p, None, None, None) == BADARG
    assert lib.cvc_vocab_nll_ls_fwd(p, p, p, 2, 8, 0.1, None, None, p, p, None, None, None) == BADARG
    assert lib.cvc_vocab_nll_ls_fwd(p, p, p, 2, 8, 0.1, p, None, p, p, p, None, None) == BADARG
    assert lib.cvc_vocab_nll_ls_fwd(p, p, p, 2, 0, 0.1, p, None, p, p, None, None, None) == BADARG
    assert lib.cvc_vocab_nll_ls_bwd(p, p, p, p, None, 2, 8, 0.1, p, None) == BADARG
    assert lib.cvc_vocab_nll_ls_bwd(p, p, p, p, p, 2, 8, 0.1, None, None) == BADARG
