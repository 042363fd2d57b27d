"""Reward mixes of self-critical training (opts.scst_reward_weights; cvc.metrics.reward_mix) at the tiny shape of tests/test_gpu_scst.py:
the default stays bit for bit what it was, a mix is the fixed-order fp32 combination of the separately evaluated metrics."""
import pytest
import torch

from test_gpu_scst import _batch, _dims, _trainer

pytestmark = pytest.mark.gpu

MIX = {"cider": 1.0, "bleu4": 2.0, "rougel": 0.5}


def _with_weights(dev, d, seed, S, weights):
    """test_gpu_scst's trainer, rebuilt so that the Trainer reads opts.scst_reward_weights as cvc.main leaves it"""
    from cvc.trainer import Trainer, build_optimizer
    o, model, tr0 = _trainer(dev, d, seed=seed, S=S, lr=1e-3)
    o.scst_reward_weights = weights
    tr = Trainer(o, None, model, build_optimizer(model, o), None, None)
    tr._cider = tr0._cider
    return model, tr


def test_default_weights_are_todays_step_bit_for_bit():
    dev = torch.device("cuda:0")
    d, seed, S = _dims(), 5, 3
    _f, _b, batch = _batch(dev, d, seed)
    _o, model_a, tr_a = _trainer(dev, d, seed=seed, S=S, lr=1e-3)
    assert not hasattr(tr_a.opts, "scst_reward_weights")
    res_a = tr_a.scst_step(batch)
    model_b, tr_b = _with_weights(dev, d, seed, S, {"cider": 1.0})
    res_b = tr_b.scst_step(batch)
    ra, rb = tr_a.last_scst["reward"], tr_b.last_scst["reward"]
    print(f"[scst reward] default: reward max |a - b| {float((ra - rb).abs().max()):.3e}, mean reward {float(ra.mean()):.5f}, "
          f"loss {float(res_a[0]):.6f} / {float(res_b[0]):.6f}")
    assert torch.equal(ra, rb) and torch.equal(tr_a.last_scst["seq"], tr_b.last_scst["seq"]) and torch.equal(tr_a.last_scst["adv"], tr_b.last_scst["adv"])
    assert "reward_parts" not in tr_a.last_scst and "reward_parts" not in tr_b.last_scst
    for x, y in zip(res_a, res_b):
        assert torch.equal(x, y)
    for (k, v), (k2, v2) in zip(model_a.state_dict().items(), model_b.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k


def _combine(table, seq, refs, nref):
    """the mix added in the fixed order cider, bleu4, rougel from the metrics evaluated on their own"""
    from cvc import metrics
    c = table.score(seq, refs, nref)
    ov = metrics.overlap(seq, refs, nref)
    parts = {"cider": c, "bleu4": ov["bleu"][:, 3].contiguous(), "rougel": ov["rouge"]}
    return (parts["cider"] * MIX["cider"] + parts["bleu4"] * MIX["bleu4"]) + parts["rougel"] * MIX["rougel"], parts


@pytest.mark.parametrize("S", [3, 1])
def test_mixed_reward_is_the_fixed_order_combination(S):
    from cvc import hip
    dev = torch.device("cuda:0")
    d, seed = _dims(), 5
    _f, b, batch = _batch(dev, d, seed)
    model, tr = _with_weights(dev, d, seed, S, dict(MIX))
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    res = tr.scst_step(batch)
    last = tr.last_scst
    seq = last["seq"]
    refs, nref = b["gt_seq"][:, :, :d.T].contiguous(), b["num"][:, 0].to(torch.int32)
    want, parts = _combine(tr.cider(), seq, refs, nref)
    print(f"[scst reward] S={S}: mix {MIX}: mean reward {float(last['reward'].mean()):.5f} (cider {float(parts['cider'].mean()):.5f}, bleu4 "
          f"{float(parts['bleu4'].mean()):.3e}, rougel {float(parts['rougel'].mean()):.5f}), max |reward - combination| "
          f"{float((last['reward'] - want).abs().max()):.3e}, loss {float(res[0]):.6f}, non-zero advantages {int((last['adv'] != 0).sum())}/{d.B * S}")
    assert seq.shape == (d.B * S, d.T)
    assert torch.equal(last["reward"], want)
    assert list(last["reward_parts"]) == ["cider", "bleu4", "rougel"]
    for k, v in parts.items():
        assert torch.equal(last["reward_parts"][k], v), k
    assert float(parts["rougel"].abs().sum()) > 0 and not torch.equal(last["reward"], parts["cider"])      # the mix is no plain CIDEr-D
    base = None
    if S == 1:
        base, _ = _combine(tr.cider(), last["greedy"], refs, nref)
        assert torch.equal(last["base"], base)
    adv, _w = hip.scst_weights(last["reward"], base, S, seq)
    assert torch.equal(last["adv"], adv)
    assert all(bool(torch.isfinite(x)) for x in res) and float(res[1]) == float(last["reward"].mean())
    moved = sum(int(not torch.equal(v, sd0[k])) for k, v in model.state_dict().items()
                if k.startswith(("decoder_core.att_lstm", "decoder_core.lang_lstm", "embed", "logit")))
    assert int((last["adv"] != 0).sum()) >= 1 and moved >= 8, moved
