"""The weight average on the training path: Trainer(ema=...) attaches it before any capture, captured and eager steps keep the same
shadows bit for bit, a void step keeps none, Trainer.eval / score run on the averaged weights in the parameters' own storage and
hand the live ones back bit for bit, and cvc.main --ema_decay writes model.pth (live), model-ema.pth and a model-best.pth that holds
the averaged weights, and resumes the shadows.  The tiny configuration of the captured-step tests of tests/test_gpu_train.py."""
import pickle

import numpy as np
import pytest
import torch

import ema_ref as ER
from cvc import synth
from test_gpu_train import _setup

pytestmark = pytest.mark.gpu


def _trainer(optim, ema=(0.9, True)):
    dev = torch.device("cuda:0")
    o, model, batch, Trainer, build_optimizer = _setup(dev, synth.CONFIGS["tiny"], train_decoder_only=False)
    o.optim, o.hip_graph = optim, 1
    model.eval()                                  # dropout off: the eager and the graphed sequence are deterministic
    return o, model, batch, Trainer(o, None, model, build_optimizer(model, o), None, None, ema=ema)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _snapshot(tr, model):
    out = {"p." + k: v.detach().clone() for k, v in model.state_dict().items()}
    for k, p in model.state_dict(keep_vars=True).items():          # (every name of a shared parameter, as in the checkpoints)
        if not isinstance(p, torch.nn.Parameter):
            continue
        e = tr.optimizer._ema_shadow.get(p)
        assert (e is None) == (p.grad is None), k          # a shadow for exactly the stepped parameters
        if e is not None:
            out["e." + k] = e.detach().clone()
    return out


@pytest.mark.parametrize("optim", ["adam", "sgd"])
def test_graphed_steps_equal_eager_ones_in_the_shadows_bits_and_the_swap_gives_the_live_bits_back(optim):
    """3 warm-up + 3 replayed steps against 6 eager ones; then the graphed trainer swaps the averages in and out
    (averaged_weights) and replays once more: equal to the eager trainer's seventh step, which saw no swap"""
    finals = []
    for graphed in (False, True):
        o, model, batch, tr = _trainer(optim)
        assert tr.ema_active and tr.optimizer.ema_active
        for _ in range(3 if graphed else 6):
            res = tr.train_step_graphed(batch) if graphed else tr._core_step(tr._prepare(batch, True))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(res[0]).all()) and (tr._graph is not None) == graphed
        assert tr.optimizer.ema_updates == 6
        six = _snapshot(tr, model)
        if graphed:
            with tr.averaged_weights():
                torch.cuda.synchronize()
                inside = _snapshot(tr, model)
                with tr.averaged_weights():                    # re-entrant: nothing moves
                    pass
                with pytest.raises(RuntimeError, match="inside averaged_weights"):
                    tr._core_step(tr._prepare(batch, True))
            torch.cuda.synchronize()
            back = _snapshot(tr, model)
            swapped = 0
            for k in six:
                assert np.array_equal(_bits(back[k]), _bits(six[k])), k
                if k.startswith("e."):                         # inside: p held the average, the shadow the live value
                    assert np.array_equal(_bits(inside["p." + k[2:]]), _bits(six[k])) and np.array_equal(_bits(inside[k]), _bits(six["p." + k[2:]]))
                    swapped += int(not torch.equal(six[k], six["p." + k[2:]]))
                elif "e." + k[2:] not in six:
                    assert np.array_equal(_bits(inside[k]), _bits(six[k])), k
            assert swapped > 10
            res = tr.train_step_graphed(batch)
        else:
            res = tr._core_step(tr._prepare(batch, True))
        torch.cuda.synchronize()
        assert tr.optimizer.ema_updates == 7
        finals.append((six, _snapshot(tr, model)))
        tr._graph = None
    for a, b in zip(finals[0], finals[1]):
        assert a.keys() == b.keys() and sum(k.startswith("e.") for k in a) > 10
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_a_void_step_is_not_averaged_and_its_eager_rerun_is():
    from cvc import hip
    o, model, batch, tr = _trainer("adam", ema=(0.5, False))
    b = tr._prepare(batch, True)
    for _ in range(2):
        tr._core_step(b)
    before = _snapshot(tr, model)
    st = hip.step_status(tr.device)
    tr._status = st
    st.fill_(1)                                              # whoever sets the word before a step voids that step
    res = tr._core_step(b)
    torch.cuda.synchronize()
    assert float(res[5]) == 1 and int(st) == 0
    after = _snapshot(tr, model)
    for k in before:
        assert np.array_equal(_bits(after[k]), _bits(before[k])), k
    assert tr.optimizer.ema_updates == 2
    tr._status = None
    tr.rerun_void_steps([b])
    torch.cuda.synchronize()
    rerun = _snapshot(tr, model)
    assert tr.optimizer.ema_updates == 3
    moved = [k for k in before if k.startswith("e.") and not torch.equal(rerun[k], before[k])]
    assert len(moved) > 10
    for k in moved:                                          # ... by the rule, from the re-run's own p_new
        ER.check_shadow(rerun[k].cpu().numpy(), rerun["p." + k[2:]].cpu().numpy(), before[k].cpu().numpy(), np.float32(0.5), k)


MAIN = ["--no_cfg", "--max_epochs", "1", "--batch_size", "4", "--synthetic_clips", "16", "--num_prop_per_frm", "7", "--t_attn_size", "5",
        "--rnn_size", "32", "--att_hid_size", "16", "--input_encoding_size", "16", "--seq_length", "6", "--vis_encoding_size", "24",
        "--tensorboard", "0", "--disp_interval", "100", "--exp_name", "e", "--learning_rate", "0.01", "--id", "e1",
        "--ema_decay", "0.9", "--ema_warmup"]


def test_main_writes_live_averaged_and_best_checkpoints_evaluates_on_the_average_and_resumes_it(tmp_path, capsys, monkeypatch):
    from cvc import main as cvc_main
    from cvc.model.create_model import build_model
    from cvc.trainer import Trainer, build_optimizer
    argv = MAIN + ["--results_dir", str(tmp_path / "results"), "--checkpoint_path", str(tmp_path) + "/"]
    assert cvc_main.main(argv) == 0
    tr = cvc_main.LAST_TRAINER
    dev = tr.device
    d = tmp_path / "e"
    live, ema, best = (torch.load(d / n, map_location=dev) for n in ("model.pth", "model-ema.pth", "model-best.pth"))
    infos = pickle.load(open(d / "infos_e1.pkl", "rb"))
    steps = len(tr.train_loader) - 1
    assert steps == 3 and ema.pop("updates") == steps == tr.optimizer.ema_updates
    assert infos["ema_updates"] == steps and infos["ema_decay"] == 0.9 and infos["ema_warmup"] is True
    assert live.keys() == ema.keys() == best.keys()
    named = {k: v for k, v in tr.model.state_dict(keep_vars=True).items() if isinstance(v, torch.nn.Parameter)}
    differ = 0
    for k in live:
        assert np.array_equal(_bits(best[k]), _bits(ema[k])), k                     # the weights that were scored
        assert np.array_equal(_bits(live[k]), _bits(tr.model.state_dict()[k])), k   # the live ones are back in the model
        shadow = tr.optimizer._ema_shadow.get(named.get(k))
        if shadow is not None:
            assert np.array_equal(_bits(ema[k]), _bits(shadow)), k
            differ += int(not torch.equal(ema[k], live[k]))
        else:
            assert np.array_equal(_bits(ema[k]), _bits(live[k])), k
    assert differ > 10
    # eval / score on the average == a fresh model loaded from model-ema.pth, bit for bit; and not the live weights'
    tr.eval(0, weights="ema")
    pred_ema = tr.predictions
    tr.score(weights="ema")
    score_ema = tr.scores
    tr.score()
    assert tr.scores == score_ema                                                   # the default, with an average attached
    tr.score(weights="live")
    score_live = tr.scores
    tr.eval(0, weights="live")
    pred_live = tr.predictions
    for k in live:
        assert np.array_equal(_bits(live[k]), _bits(tr.model.state_dict()[k])), k
    fresh = build_model(tr.opts, dev)
    fresh.load_state_dict(ema)
    o2 = type(tr.opts)(**{k: v for k, v in vars(tr.opts).items() if not k.startswith("ema_")})
    tr2 = Trainer(o2, tr.dataset, fresh, build_optimizer(fresh, o2), tr.train_loader, tr.val_loader)
    assert not tr2.ema_active
    tr2.eval(0)
    tr2.score()
    assert tr2.predictions == pred_ema and tr2.scores == score_ema
    assert score_live != score_ema
    fresh.load_state_dict(live)
    tr2._weights_changed()
    tr2.eval(0)
    tr2.score()
    assert tr2.predictions == pred_live and tr2.scores == score_live
    # --resume True: the shadows and their count come from model-ema.pth (the epoch's training is stubbed out: what was loaded stays)
    capsys.readouterr()
    monkeypatch.setattr(Trainer, "train", lambda self, epoch, tb=None: None)
    assert cvc_main.main(argv + ["--resume", "True"]) == 0
    out = capsys.readouterr().out
    assert "model-ema.pth (3 averaged steps)" in out
    tr3 = cvc_main.LAST_TRAINER
    assert tr3 is not tr and tr3.optimizer.ema_updates == 3
    named3 = dict(tr3.model.named_parameters())
    assert len(tr3.optimizer._ema_shadow) == len(tr3.optimizer.param_groups) > 10
    for k, p in named3.items():
        e = tr3.optimizer._ema_shadow.get(p)
        assert (e is None or np.array_equal(_bits(e), _bits(ema[k]))) and np.array_equal(_bits(p), _bits(live[k])), k
    assert tr3.predictions == pred_ema                                              # its evaluation ran on the restored average
    again = torch.load(d / "model-ema.pth", map_location=dev)
    assert again.pop("updates") == 3 and all(np.array_equal(_bits(again[k]), _bits(ema[k])) for k in ema)
    # a run directory without model-ema.pth: the average starts from the resumed weights, said once
    (d / "model-ema.pth").unlink()
    assert cvc_main.main(argv + ["--resume", "True"]) == 0
    out = capsys.readouterr().out
    assert out.count("the weight average starts from the resumed weights") == 1
    # --inference_only on a run directory that has a model-ema.pth: as without the flags
    assert cvc_main.main(argv + ["--resume", "True", "--inference_only"]) == 0
    tr4 = cvc_main.LAST_TRAINER
    assert not tr4.ema_active and tr4.predictions == pred_live
