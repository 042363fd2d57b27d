"""cvc.optim.ClipAdam / ClipSGD / ClipAdamax with the weight average attached (attach_ema), six steps on the GPU.

Reference: nn.utils.clip_grad_norm_ + the torch optimizer for the parameters, and an fp64 lerp on the CPU over the TORCH parameters
for the shadows, e_k = e_{k-1} + (p_k - e_{k-1}) (1 - d_k), d_k the warm-up's fp64 value.  The tolerance of a shadow element is
carried through the same recursion:
    tol_k = d_k tol_{k-1} + (1 - d_k) (2e-6 |p_k| + 1e-6) + K x bound_k + u |p_k - e_{k-1}|
-- the parameters are held to torch within rtol 2e-6 / atol 1e-6 (the tolerance of the six-step tests of
tests/test_gpu_optim_rules.py, asserted here too), an average is a convex combination of them, every step adds its own rounding
(K x the bound of tests/ema_ref.py), and the device's d_k is one float32 division (u d_k on the weight of the difference).
Besides: parameters, gradients, state and step counts are BIT-equal to the same optimizer without the average; optimizer.state holds
torch's keys only; the shadows survive a scheduler and a state_dict round trip.

Measured on an MI355X, the worst per-step |err| / (K x bound) of a shadow: 0.25 without the warm-up (all three rules), 0.39 / 0.25 /
0.40 under it (Adam / SGD / Adamax: at d_eff = 0.1 the difference's weight 0.9 carries its own rounding).  The file takes 4 s."""
import numpy as np
import pytest
import torch

import ema_ref as ER
from optim_ref import CHUNK, K, U

pytestmark = pytest.mark.gpu

SIZES = (7, 1024, CHUNK + 1)
STATE_KEYS = {"adam": {"step", "exp_avg", "exp_avg_sq"}, "sgd": {"momentum_buffer"}, "adamax": {"step", "exp_avg", "exp_inf"}}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a visible MI355X (torch.cuda.is_available() is False)")
    return torch.device("cuda:0")


def make(dev, rule, seed=3, ours=True):
    from cvc.optim import ClipAdam, ClipAdamax, ClipSGD
    rng = np.random.default_rng(seed)
    ps = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)) for n in SIZES]
    late = torch.nn.Parameter(torch.from_numpy(rng.standard_normal(33).astype(np.float32)).to(dev))      # no gradient at first
    groups = [{"params": [q], "lr": (1e-2, 1e-3)[i % 2], "weight_decay": (0.0, 0.01)[i % 2]} for i, q in enumerate(ps + [late])]
    if rule == "adam":
        opt = (ClipAdam if ours else torch.optim.Adam)(groups, betas=(0.8, 0.99))
    elif rule == "sgd":
        opt = (ClipSGD if ours else torch.optim.SGD)(groups, lr=1e-3, momentum=0.9)
    else:
        opt = (ClipAdamax if ours else torch.optim.Adamax)(groups, betas=(0.8, 0.99))
    return ps, late, opt


def grads(ps, it, late=None):
    """fresh values IN PLACE where a gradient tensor exists (new tensors would be new addresses, hence a new step table every step)"""
    rng = np.random.default_rng(100 + it)
    vals = [(rng.standard_normal(q.numel()) * (3.0 if it % 2 else 0.05)).astype(np.float32) for q in ps]
    if late is not None:
        ps, vals = ps + [late], vals + [rng.standard_normal(late.numel()).astype(np.float32)]
    for q, v in zip(ps, vals):
        v = torch.from_numpy(v).to(q.device)
        if q.grad is None:
            q.grad = v
        else:
            q.grad.copy_(v)


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("rule", ["adam", "sgd", "adamax"])
def test_six_steps_with_the_average_attached(dev, rule, warmup):
    d = 0.9
    pa, late_a, ref = make(dev, rule, ours=False)
    pb, late_b, opt = make(dev, rule)
    pc, late_c, plain = make(dev, rule)
    opt.attach_ema(d, warmup)
    assert opt.ema_active and not plain.ema_active and opt.ema_updates == 0
    e_ref = tol = None
    worst = 0.0
    for it in range(6):
        late = it >= 3                                  # the fourth parameter's gradient appears at step four
        for ps, l in ((pa, late_a), (pb, late_b), (pc, late_c)):
            grads(ps, it, l if late else None)
        act_a, act_b, act_c = (ps + ([l] if late else []) for ps, l in ((pa, late_a), (pb, late_b), (pc, late_c)))
        torch.nn.utils.clip_grad_norm_(act_a, 0.5)
        ref.step()
        before = [opt._ema_shadow[q].detach().cpu().numpy().copy() if q in opt._ema_shadow else q.detach().cpu().numpy().copy() for q in act_b]
        if it == 3:
            assert late_b not in opt._ema_shadow
        opt.clip_and_step(0.5, 1.0)
        plain.clip_and_step(0.5, 1.0)
        torch.cuda.synchronize()
        if it == 2:
            old = (opt._table, opt._ema_ptrs)
        if it == 3:
            tables = (opt._table, opt._ema_ptrs)        # rebuilt for the new parameter; the old table and pointer array kept alive
            assert tables[0] is not old[0] and len(opt._retired) == 2 and all(any(r is o for r in opt._retired) for o in old)
        d_dev = float(opt._ema_state[1])
        d_k = ER.d_eff_fp64(d, it, warmup)
        assert abs(d_dev - d_k) <= U * d_k and opt.ema_updates == it + 1
        for q, r in zip(act_b, act_c):                 # the average does not touch the step: bits of the plain optimizer
            assert np.array_equal(bits(q), bits(r)) and np.array_equal(bits(q.grad), bits(r.grad))
            assert set(opt.state[q].keys()) == STATE_KEYS[rule]
            for k in STATE_KEYS[rule]:
                assert np.array_equal(bits(opt.state[q][k]), bits(plain.state[r][k])), k
        for q, p in zip(act_b, act_a):
            assert torch.allclose(q, p, rtol=2e-6, atol=1e-6), it
        # per step, under the device's own p_new and d_eff (a shadow created this step was a copy of the value BEFORE the step)
        for j, (q, e0) in enumerate(zip(act_b, before)):
            worst = max(worst, ER.check_shadow(opt._ema_shadow[q].cpu().numpy(), q.detach().cpu().numpy(), e0, np.float32(d_dev),
                                               "%s step %d param %d" % (rule, it + 1, j)))
        # against torch + the fp64 lerp, the first three parameters from step one on
        p64 = [p.detach().cpu().numpy().astype(np.float64) for p in pa]
        if e_ref is None:
            rng = np.random.default_rng(3)
            e_ref = [rng.standard_normal(n).astype(np.float32).astype(np.float64) for n in SIZES]       # = the initial parameters
            tol = [np.zeros(n) for n in SIZES]
        for j in range(3):
            diff = p64[j] - e_ref[j]
            e1, bound = ER.ema_fp64(p64[j], e_ref[j], np.float32(d_k))
            e1 = e_ref[j] + diff * (1.0 - d_k)
            tol[j] = d_k * tol[j] + (1.0 - d_k) * (2e-6 * np.abs(p64[j]) + 1e-6) + K * bound + U * np.abs(diff)
            e_ref[j] = e1
            err = np.abs(opt._ema_shadow[pb[j]].cpu().numpy().astype(np.float64) - e1)
            assert (err <= tol[j]).all(), (it, j, float((err / tol[j]).max()))
    print("%s warmup %s: worst per-step e ratio %.3g of K x bound" % (rule, warmup, worst))
    assert opt._table is tables[0] and opt._ema_ptrs is tables[1] and len(opt._retired) == 2
    assert set(opt._ema_shadow) == set(pb + [late_b]) and len(opt.state[late_b]) == len(STATE_KEYS[rule])
    # state_dict() is torch's and loads into the torch optimizer
    sd = opt.state_dict()
    assert all(set(s.keys()) == STATE_KEYS[rule] for s in sd["state"].values()) and set(sd.keys()) == {"state", "param_groups"}
    ref.load_state_dict(sd)


@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_a_scheduler_keeps_the_table_and_the_shadows(dev, rule):
    ps, late, opt = make(dev, rule)
    opt.attach_ema(0.5)
    grads(ps, 0)
    opt.clip_and_step(0.5, 1.0)
    t0, ptrs, shadows = opt._table, opt._ema_ptrs, dict(opt._ema_shadow)
    for it in (1, 2):
        for g in opt.param_groups:
            g["lr"] *= 0.5
        grads(ps, it)
        before = [opt._ema_shadow[q].clone() for q in ps]
        opt.clip_and_step(0.5, 1.0)
        torch.cuda.synchronize()
        assert opt._table is t0 and opt._ema_ptrs is ptrs and not opt._retired
        assert all(opt._ema_shadow[q] is shadows[q] for q in ps) and opt.ema_updates == it + 1
        for q, e0 in zip(ps, before):
            ER.check_shadow(opt._ema_shadow[q].cpu().numpy(), q.detach().cpu().numpy(), e0.cpu().numpy(), np.float32(0.5),
                            "%s after the scheduler, step %d" % (rule, it + 1))
    assert late not in opt._ema_shadow


def test_ema_state_dict_round_trip_swap_and_refusals(dev):
    from cvc.optim import ClipAdam

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Linear(5, 3)
            self.b = torch.nn.Linear(3, 2)             # never gets a gradient: no shadow
            self.register_buffer("count", torch.arange(4.0))

    torch.manual_seed(0)
    m = M().to(dev)
    opt = ClipAdam(m.parameters(), lr=1e-2)
    with pytest.raises(RuntimeError, match="no average is attached"):
        opt.swap_ema()
    for bad in (1.0, -0.1, float("nan"), 2.0):
        with pytest.raises(ValueError, match=r"decay must lie in \[0, 1\)"):
            opt.attach_ema(bad)
    cpu = ClipAdam([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpu.attach_ema(0.9)
    opt.attach_ema(0.5, warmup=True)
    for it in range(3):
        m.a(torch.ones(2, 5, device=dev)).sum().backward() if it == 0 else [p.grad.add_(0.1) for p in m.a.parameters()]
        opt.clip_and_step(1.0)
    assert set(opt._ema_shadow) == set(m.a.parameters()) and opt.ema_updates == 3
    sd = opt.ema_state_dict(m)
    assert set(sd) == set(m.state_dict()) | {"updates"} and sd["updates"] == 3
    assert torch.equal(sd["a.weight"], opt._ema_shadow[m.a.weight]) and not torch.equal(sd["a.weight"], m.a.weight)
    assert torch.equal(sd["b.weight"], m.b.weight) and torch.equal(sd["count"], m.count)
    assert sd["a.weight"].data_ptr() != opt._ema_shadow[m.a.weight].data_ptr()
    # the swap: averaged weights in the parameters' own storage, and back bit for bit
    live = {n: p.detach().clone() for n, p in m.named_parameters()}
    ptrs = {n: p.data_ptr() for n, p in m.named_parameters()}
    with opt.averaged():
        torch.cuda.synchronize()
        for n, p in m.named_parameters():
            assert torch.equal(p, sd[n]) and p.data_ptr() == ptrs[n]
        assert torch.equal(opt._ema_shadow[m.a.weight], live["a.weight"])
    for n, p in m.named_parameters():
        assert np.array_equal(bits(p), bits(live[n]))
    assert torch.equal(opt._ema_shadow[m.a.bias], sd["a.bias"])
    # into a fresh optimizer over a fresh model, before its first step
    torch.manual_seed(1)
    m2 = M().to(dev)
    opt2 = ClipAdam(m2.parameters(), lr=1e-2)
    with pytest.raises(RuntimeError, match="no average is attached"):
        opt2.load_ema_state_dict(m2, sd)
    opt2.attach_ema(0.5, warmup=True)
    opt2.load_ema_state_dict(m2, sd)
    assert opt2.ema_updates == 3
    sd2 = opt2.ema_state_dict(m2)
    assert sd2["updates"] == 3 and all(np.array_equal(bits(sd2[n]), bits(sd[n])) for n in ("a.weight", "a.bias"))
    m2.a(torch.ones(2, 5, device=dev)).sum().backward()
    e0 = opt2._ema_shadow[m2.a.weight].clone()
    opt2.clip_and_step(1.0)
    assert opt2.ema_updates == 4 and abs(float(opt2._ema_state[1]) - 4.0 / 13.0) <= U      # the warm-up goes on from the loaded count
    ER.check_shadow(opt2._ema_shadow[m2.a.weight].cpu().numpy(), m2.a.weight.detach().cpu().numpy(), e0.cpu().numpy(),
                    opt2._ema_state[1].cpu().numpy(), "after load_ema_state_dict")
    # ... and into one that has stepped
    opt.load_ema_state_dict(m, dict(sd, updates=7))
    assert opt.ema_updates == 7 and torch.equal(opt._ema_shadow[m.a.weight], sd["a.weight"])
    opt.detach_ema()
    assert not opt.ema_active and not opt._ema_shadow
    m.a(torch.ones(2, 5, device=dev)).sum().backward()
    opt.clip_and_step(1.0)                             # the plain entry again
    assert opt._ema_ptrs is None
