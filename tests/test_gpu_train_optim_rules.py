"""--optim sgd / adamax on the training path: build_optimizer hands out cvc.optim.ClipSGD / ClipAdamax, which gives these two of the
reference's three optimizers (main.py:182-191) what Adam had alone -- captured steps (--hip_graph) and deferred error words -- and
three graphed training steps equal three eager ones bit for bit.  The tiny configuration of the captured-step tests of
tests/test_gpu_train.py."""
import pytest
import torch

from cvc import synth
from test_gpu_train import _setup

pytestmark = pytest.mark.gpu

STATE = {"sgd": ("momentum_buffer",), "adamax": ("step", "exp_avg", "exp_inf")}


def _trainer(optim):
    dev = torch.device("cuda:0")
    o, model, batch, Trainer, build_optimizer = _setup(dev, synth.CONFIGS["tiny"], train_decoder_only=False)
    o.optim, o.hip_graph = optim, 1
    model.eval()                                  # dropout off: the eager and the graphed sequence are deterministic
    return o, model, batch, Trainer(o, None, model, build_optimizer(model, o), None, None)


@pytest.mark.parametrize("optim", ["sgd", "adamax"])
def test_build_optimizer_returns_the_native_step_and_the_trainer_can_capture_and_defer(optim, monkeypatch):
    from cvc import optim as cvc_optim, trainer as cvc_trainer
    o, model, _batch, tr = _trainer(optim)
    cls, base = {"sgd": (cvc_optim.ClipSGD, torch.optim.SGD), "adamax": (cvc_optim.ClipAdamax, torch.optim.Adamax)}[optim]
    assert type(tr.optimizer) is cls and isinstance(tr.optimizer, base)
    assert tr.graph_capable() and tr._can_defer()
    groups = tr.optimizer.param_groups
    assert len(groups) == sum(1 for p in model.parameters() if p.requires_grad) and all(len(g["params"]) == 1 for g in groups)
    assert {g["lr"] for g in groups} <= {o.learning_rate, o.learning_rate * 0.1}
    if optim == "sgd":
        assert all(g["momentum"] == 0.9 and "betas" not in g for g in groups)
    else:
        assert all(tuple(g["betas"]) == (o.optim_alpha, o.optim_beta) for g in groups)
    # the A/B switch and CPU parameters keep the library optimizers; Adamax's can now be captured too
    monkeypatch.setattr(cvc_trainer, "CLIP_ADAM", False)
    lib = cvc_trainer.build_optimizer(model, o, capturable=True)
    assert type(lib) is base
    if optim == "adamax":
        assert all(g["capturable"] for g in lib.param_groups)
    monkeypatch.setattr(cvc_trainer, "CLIP_ADAM", True)
    assert type(cvc_trainer.build_optimizer(model.cpu(), o)) is base


@pytest.mark.parametrize("optim", ["sgd", "adamax"])
def test_three_graphed_training_steps_equal_three_eager_ones_bit_for_bit(optim):
    """(train_step_graphed takes 3 warm-up steps before its capture: 3 + 3 replays against 6 eager steps)"""
    finals = []
    for graphed in (False, True):
        o, model, batch, tr = _trainer(optim)
        for _ in range(3 if graphed else 6):
            res = tr.train_step_graphed(batch) if graphed else tr._core_step(tr._prepare(batch, True))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(res[0]).all())
        assert (tr._graph is not None) == graphed
        out = {"p." + k: v.detach().clone() for k, v in model.state_dict().items()}
        named = dict(model.named_parameters())
        stepped = 0
        for k, p in named.items():
            st = tr.optimizer.state[p]
            if p.grad is None:
                assert len(st) == 0, k
                continue
            stepped += 1
            assert set(st) == set(STATE[optim]), k
            for n in STATE[optim]:
                out["s.%s.%s" % (k, n)] = st[n].detach().clone()
            if optim == "adamax":
                assert float(st["step"]) == 6
        assert stepped > 10
        finals.append(out)
        tr._graph = None
    assert finals[0].keys() == finals[1].keys()
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]), k
    moved = [k for k in finals[0] if k.startswith("s.") and k.endswith(STATE[optim][-1]) and bool(finals[0][k].any())]
    assert len(moved) > 10
