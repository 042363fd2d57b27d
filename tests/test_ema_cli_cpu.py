"""The weight-averaging flags of cvc.main (no GPU here): absent they add no key to the options namespace, a bad value or a lone
--ema_warmup ends the run with a message before any set-up, so does --ema_decay without the native optimizer step; the trainer and
the optimizers refuse an average they cannot keep instead of emulating it."""
import argparse
import inspect

import pytest
import torch


def test_absent_flags_add_no_key_and_live_in_cvc_main():
    from cvc import main as cvc_main, opts
    o = cvc_main.build_parser().parse_args([])
    assert not [k for k in vars(o) if "ema" in k]
    cvc_main.check_ema_flags(o)
    assert "ema_decay" in inspect.getsource(cvc_main) and "ema" not in inspect.getsource(opts)
    o = cvc_main.build_parser().parse_args(["--ema_decay", "0.999", "--ema_warmup"])
    assert o.ema_decay == 0.999 and o.ema_warmup is True
    cvc_main.check_ema_flags(o)
    o = cvc_main.build_parser().parse_args(["--ema_decay", "0"])             # 0 = off, said explicitly
    cvc_main.check_ema_flags(o)
    assert o.ema_decay == 0 and not hasattr(o, "ema_warmup")


@pytest.mark.parametrize("bad", ["1", "1.5", "-0.1", "nan", "inf", "-inf"])
def test_a_decay_outside_the_unit_interval_ends_the_run(bad):
    from cvc import main as cvc_main
    with pytest.raises(SystemExit, match=r"--ema_decay must lie in \[0, 1\)"):
        cvc_main.main(["--no_cfg", "--ema_decay=" + bad])                    # (ends before any set-up: no GPU is asked for)


@pytest.mark.parametrize("argv", [["--ema_warmup"], ["--ema_warmup", "--ema_decay", "0"]])
def test_warmup_alone_ends_the_run(argv):
    from cvc import main as cvc_main
    with pytest.raises(SystemExit, match="--ema_warmup shapes the decay of --ema_decay"):
        cvc_main.main(["--no_cfg"] + argv)


def test_the_flag_without_the_native_step_ends_the_run(monkeypatch):
    from cvc import main as cvc_main, trainer
    monkeypatch.setattr(trainer, "CLIP_ADAM", False)
    with pytest.raises(SystemExit, match="--ema_decay needs the native optimizer step"):
        cvc_main.main(["--no_cfg", "--ema_decay", "0.9"])
    cvc_main.check_ema_flags(cvc_main.build_parser().parse_args(["--ema_decay", "0"]))      # off: nothing to refuse


def test_the_trainer_refuses_a_library_optimizer_and_the_optimizer_cpu_parameters():
    from cvc.optim import ClipAdam, ClipAdamax, ClipSGD
    from cvc.trainer import Trainer
    lin = torch.nn.Linear(2, 2)
    for ema in ((0.9, False), None):
        o = argparse.Namespace(**({} if ema else dict(ema_decay=0.9, ema_warmup=True)))
        with pytest.raises(RuntimeError, match="library optimizer .* not emulated"):
            Trainer(o, None, lin, torch.optim.SGD(lin.parameters(), lr=0.1), None, None, **(dict(ema=ema) if ema else {}))
    tr = Trainer(argparse.Namespace(), None, lin, torch.optim.SGD(lin.parameters(), lr=0.1), None, None)
    assert not tr.ema_active
    with pytest.raises(RuntimeError, match="no weight average is attached"):
        tr.eval(0, weights="ema")
    with pytest.raises(ValueError, match="'ema' or 'live'"):
        tr.eval(0, weights="mean")
    for cls in (ClipAdam, ClipSGD, ClipAdamax):
        opt = cls(lin.parameters(), lr=0.1)
        assert not opt.ema_active
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.attach_ema(0.9)
        with pytest.raises(ValueError, match=r"decay must lie in \[0, 1\)"):
            opt.attach_ema(float("nan"))
        assert not opt.ema_active
