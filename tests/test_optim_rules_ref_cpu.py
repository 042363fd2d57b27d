"""tests/optim_rules_ref.py proven on the CPU (no GPU here): sgd_step_fp64 / adamax_step_fp64 + optim_ref.norm_coef_fp64 are
nn.utils.clip_grad_norm_ + torch.optim.SGD(momentum=...) / torch.optim.Adamax on float64 tensors over four steps, NaN gradients
included; the float32 restatements of optim_sgd_kernel's and optim_adamax_kernel's `upd` stay inside the bounds on every table (the
worst ratios are printed, and each K is 4 x its ratio); every subtly wrong kernel leaves the bounds by a wide margin (printed); and
the case lists hold what they promise."""
import numpy as np
import pytest
import torch

import optim_ref as OR
import optim_rules_ref as RR


def _r32(x):
    return float(np.float32(x))


SIZES, LRS, WDS = (5, 37, 130, 1), (1e-3, 1e-4, 1e-3, 0.0), (0.0, 0.01, 0.01, 0.0)


def _four_steps(make_opt, step_ref, state_names, kind, max_norm, inv):
    """four steps of clip_grad_norm_ + a torch optimizer on float64 CPU tensors against norm_coef_fp64 + step_ref, per-group lr and
    weight decay; gradients that are sums over 4 ranks are handed to torch divided by 4 (exact).  step_ref(i, it, p, g, state, coef)
    -> (Step, new state list); state_names: torch's state keys in that list's order"""
    rng = np.random.default_rng(5)
    ps = [rng.standard_normal(n).astype(np.float32).astype(np.float64) for n in SIZES]
    states = [[np.zeros(n) for _ in state_names] for n in SIZES]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = make_opt([{"params": [q], "lr": _r32(lr), "weight_decay": _r32(wd)} for q, lr, wd in zip(tp, LRS, WDS)])
    worst = 0.0
    for it in range(4):
        gs = [(rng.standard_normal(n) * (30.0 if it == 1 else 1.0)).astype(np.float32).astype(np.float64) for n in SIZES]
        if it == 0 and kind == "nan":
            gs[1][7] = float("nan")
        for q, g in zip(tp, gs):
            q.grad = torch.from_numpy(g * inv)
        if max_norm > 0:                                                # (max_norm <= 0: the clip is off, torch takes its step alone)
            n_t = torch.nn.utils.clip_grad_norm_(tp, _r32(max_norm))
        opt.step()
        norm, coef = OR.norm_coef_fp64(gs, max_norm, inv)
        if max_norm > 0:
            np.testing.assert_allclose(norm, float(n_t), rtol=1e-12)
        for i, (q, g) in enumerate(zip(tp, gs)):
            r, states[i] = step_ref(i, it, ps[i], g, states[i], coef)
            ps[i] = r.p
            np.testing.assert_allclose(r.g, q.grad.numpy(), rtol=1e-12, atol=0, equal_nan=True)
            np.testing.assert_allclose(r.p, q.detach().numpy(), rtol=1e-12, atol=0, equal_nan=True)
            fin = np.isfinite(r.p)
            if fin.any():
                worst = max(worst, float(np.max(np.abs(r.p[fin] - q.detach().numpy()[fin]))))
            for name, mine in zip(state_names, states[i]):
                np.testing.assert_allclose(mine, opt.state[q][name].numpy(), rtol=1e-12, atol=0, equal_nan=True)
            if "step" in opt.state[q]:
                assert float(opt.state[q]["step"]) == it + 1
    print("worst |reference - torch| of a parameter over four steps: %.3g" % worst)
    return ps, states


# ---- the references against torch
@pytest.mark.parametrize("kind", ["finite", "nan"])
@pytest.mark.parametrize("mom,max_norm,inv", [(0.9, 1.5, 1.0), (0.5, 40.0, 0.25), (0.0, 0.7, 1.0), (0.9, 1e9, 0.25)])
def test_sgd_reference_equals_clip_grad_norm_plus_torch_sgd_in_float64(kind, mom, max_norm, inv):
    m32 = _r32(mom)

    def step_ref(i, it, p, g, state, coef):
        r = RR.sgd_step_fp64(p, g, state[0] if mom else np.zeros_like(p), LRS[i], WDS[i], m32, coef)
        return r, [r.m] if mom else []
    ps, _ = _four_steps(lambda groups: torch.optim.SGD(groups, lr=1e-3, momentum=m32, foreach=False), step_ref,
                        ["momentum_buffer"] if mom else [], kind, max_norm, inv)
    if kind == "nan":
        assert all(np.isnan(p).all() for p in ps)                          # through the norm (a bound never reached included)


@pytest.mark.parametrize("kind", ["finite", "nan"])
@pytest.mark.parametrize("betas,max_norm,inv", [((0.9, 0.999), 1.5, 1.0), ((0.8, 0.99), 40.0, 0.25), ((0.0, 0.0), 1e9, 1.0),
                                                ((0.5, 0.5), 0.7, 0.25), ((0.9, 0.0), 0.0, 1.0)])
def test_adamax_reference_equals_clip_grad_norm_plus_torch_adamax_in_float64(kind, betas, max_norm, inv):
    b1, b2, eps = _r32(betas[0]), _r32(betas[1]), _r32(OR.EPS)

    def step_ref(i, it, p, g, state, coef):
        r = RR.adamax_step_fp64(p, g, state[0], state[1], it, LRS[i], WDS[i], b1, b2, eps, coef)
        return r, [r.m, r.v]
    ps, states = _four_steps(lambda groups: torch.optim.Adamax(groups, betas=(b1, b2), eps=eps, foreach=False), step_ref,
                             ["exp_avg", "exp_inf"], kind, max_norm, inv)
    if kind == "nan" and max_norm > 0:
        assert all(np.isnan(p).all() for p in ps)                          # through the norm: every parameter
    elif kind == "nan":
        # without a clip the NaN stays where it is: NaN exp_inf (torch.maximum hands it on) and NaN p at that element only
        bad = np.zeros(SIZES[1], dtype=bool)
        bad[7] = True
        assert np.array_equal(np.isnan(ps[1]), bad) and np.array_equal(np.isnan(states[1][1]), bad)
        assert all(np.isfinite(ps[i]).all() for i in (0, 2, 3))


# ---- the float32 restatements inside the bounds
def _restated(table, variant=None):
    vals = RR.values(table)
    gs = [vals.g[a:b] for a, b in zip(vals.off[:-1], vals.off[1:])]
    _norm, coef = OR.norm_coef_f32(gs, table.max_norm, table.inv)
    return vals, coef, RR.restated(table, vals, coef, variant), RR.reference(table, vals, coef)


def _ratios(table, got, ref):
    keys = {"sgd": "pmg" if table.mom != 0 else "pg", "adamax": "pmvg"}[table.rule]
    every = dict(p=(got[0], ref.p, ref.ep), m=(got[1], ref.m, ref.em), v=(got[2], ref.v, ref.ev), g=(got[3], ref.g, ref.eg))
    return {k: OR.ratio(*every[k])[0] for k in keys}


@pytest.mark.parametrize("rule", ["sgd", "adamax"])
def test_restatement_stays_inside_the_bounds_and_k_is_four_times_its_worst_ratio(rule):
    worst = {}
    for table in RR.RULE_TABLES[rule]:
        _vals, _coef, got, ref = _restated(table)
        for k, r in _ratios(table, got, ref).items():
            if r > worst.get(k, (0.0, ""))[0]:
                worst[k] = (r, table.name)
    print("%s: worst |float32 restatement - fp64| / bound (without K): " % rule + ", ".join("%s %.4f (%s)" % ((k,) + w) for k, w in worst.items()))
    top = max(w[0] for k, w in worst.items() if k != "g")
    print("%s: worst ratio %.4f -> K = 4 x = %.3f (optim_rules_ref.K = %g)" % (rule, top, 4 * top, RR.K[rule]))
    assert worst["g"][0] <= 1.0                                        # one rounding: no constant
    assert abs(top - RR.WORST_RATIO[rule]) < 5e-4, (top, RR.WORST_RATIO[rule])
    assert 4 * RR.WORST_RATIO[rule] <= RR.K[rule] < 4 * RR.WORST_RATIO[rule] + 0.05


def test_a_nan_gradient_element_stays_one_element_without_a_clip_and_is_everything_with_one():
    for name in ("adamax-shape-300", "sgd-shape-300"):
        table = RR.TABLES[name]
        v = RR.values(table)
        g = v.g.copy()
        at = int(v.off[123]) + 2
        g[at] = np.nan
        v = v._replace(g=g)
        bad = np.zeros(len(g), dtype=bool)
        bad[at] = True
        for ref in (RR.reference(table, v, 0.25), RR.restated(table, v, np.float32(0.25))):
            p, m, u = ref[0], ref[1], ref[2]
            assert np.array_equal(np.isnan(p), bad) and np.array_equal(np.isnan(m), bad)
            if table.rule == "adamax":
                assert np.array_equal(np.isnan(u), bad)                    # (fmax would have dropped it)
        _norm, coef = OR.norm_coef_fp64([g], 5.0, 0.25)
        assert coef != coef and np.isnan(RR.reference(table, v, coef).p).all()


# ---- the bounds notice a wrong kernel
WIDE = 10.0            # x (K x bound)


@pytest.mark.parametrize("rule,variant", [("sgd", v) for v in RR.SGD_VARIANTS] + [("adamax", v) for v in RR.ADAMAX_VARIANTS])
def test_wrong_kernel_leaves_the_bounds_by_a_wide_margin(rule, variant):
    caught = []
    for table in RR.HYPER_TABLES[rule] + RR.SHAPE_TABLES[rule]:
        _vals, _coef, got, ref = _restated(table, variant)
        try:
            r = _ratios(table, got, ref)
        except AssertionError:                                        # an Inf / NaN where the reference has a number, or the reverse
            r = {"nonfinite": float("inf")}
        out = {k: x / RR.K[rule] for k, x in r.items() if x > WIDE * RR.K[rule]}
        if out:
            caught.append((table.name, out))
    assert caught, variant
    top = max(caught, key=lambda c: max(c[1].values()))
    print("%s %s: %d tables more than %g x outside, the widest %s: %s" % (rule, variant, len(caught), WIDE, top[0],
                                                                        ", ".join("%s at %.3g x the bound" % kv for kv in top[1].items())))


def test_wrong_bias_correction_is_invisible_at_a_large_step_count():
    """why the small step counts are in the case list"""
    table = RR.TABLES["adamax-hyper-b0.9-0.999-wd0"]
    for variant in ("t_minus_1", "no_bias_correction"):
        vals, _coef, got, ref = _restated(table, variant)
        late, early = vals.t == 99999, (vals.t >= 1) & (vals.t <= 9) & (vals.lr > 0)
        assert late.any() and early.any()
        assert OR.ratio(got[0][late], ref.p[late], ref.ep[late])[0] <= RR.K_ADAMAX
        assert OR.ratio(got[0][early], ref.p[early], ref.ep[early])[0] > RR.K_ADAMAX


# ---- the tables
def test_case_lists_hold_what_they_should():
    C_ = OR.CHUNK
    assert set(OR.SIZES) == {1, 2, 3, 4, 5, 7, 8, 255, 256, 1023, 1024, 1025, 1027, C_ - 1, C_, C_ + 1, C_ + 4, 2 * C_ + 3, 3 * C_ + 1025}
    assert [len(RR.forms_of(*a)) for a in (("adamax",), ("sgd", 0.9), ("sgd", 0.0))] == [13, 10, 7]
    for rule, moms in (("adamax", (None,)), ("sgd", (0.9, 0.0))):
        for mom in moms:
            forms = [f for f, _ in RR.forms_of(rule, 0.9 if mom is None else mom)]
            seen = {(s.n, s.offs) for t in RR.SIZE_TABLES[rule] if t.mom == mom for s in t.segs}
            for n in OR.SMALL_N + OR.MID_N:
                assert all((n, f) in seen for f in forms), (rule, mom, n)
            for n in OR.LARGE_N:
                got = {f for (k, f) in seen if k == n}
                assert OR.ALIGNED in got and len(got) == 1 + len(forms) // 3
                assert {j for f in got for j in range(4) if f[j]} == set(range(len(forms) // 3))          # every operand of the rule
                assert {f[j] for f in got for j in range(4) if f[j]} == ({1, 2, 3} if len(forms) > 7 else {1, 2})
    for t in RR.HYPER_TABLES["sgd"] + RR.HYPER_TABLES["adamax"]:
        assert {(s.t, s.lr) for s in t.segs} == {(a, b) for a in RR.T_BEFORE for b in OR.LRS}
    assert {(t.mom, t.segs[0].wd) for t in RR.HYPER_TABLES["sgd"]} == {(m, w) for m in (0.9, 0.5, 0.0) for w in (0.0, 0.01)}
    assert {(t.betas, t.segs[0].wd) for t in RR.HYPER_TABLES["adamax"]} == {(b, w) for b in OR.BETAS for w in OR.WDS}
    assert RR.T_BEFORE == (0, 1, 9, 99999)
    for rule in ("sgd", "adamax"):
        hy = RR.HYPER_TABLES[rule]
        assert {t.max_norm for t in hy} == {5.0, 0.0, 1e9} and {t.inv for t in hy} == {1.0, 0.25}
        assert [len(t.segs) for t in RR.SHAPE_TABLES[rule]] == [1, 256, 257, 300]
        for t in RR.RULE_TABLES[rule]:
            assert sum(s.n for s in t.segs) < 700000, t.name
            assert {s.lr for s in t.segs} <= set(OR.LRS) and {s.wd for s in t.segs} <= set(OR.WDS)
            v = RR.values(t)
            assert (v.g == 0).any() or len(v.g) < 20
            assert not v.m[v.t == 0].any() and not v.v[v.t == 0].any()
            if rule == "adamax":
                assert (v.v >= 0).all() and (np.abs(v.m) <= v.v * (1 + 1e-6)).all()
            else:
                assert not v.v.any() and (t.mom != 0 or not v.m.any())


def test_slots_do_not_overlap():
    for t in RR.ALL_TABLES:
        starts, size = OR.layout(t.segs)
        for s, a, b in zip(t.segs, starts, starts[1:] + [size - OR.BAND]):
            assert a % 4 == 0 and a >= OR.BAND and a + 3 + s.n <= b - 1
