"""tests/optim_ref.py proven on the CPU (no GPU here): step_fp64 + norm_coef_fp64 are nn.utils.clip_grad_norm_ +
torch.optim.Adam(foreach=False) on float64 tensors, NaN and Inf gradients included; the float32 restatement of optim_adam_kernel's
arithmetic stays inside the bounds on every table of the case lists (the worst ratio is printed, and K is 4 x it); every subtly
wrong kernel leaves the bounds on a committed case (printed), while the other correct order of the first moment's update stays
inside; and the tables as cvc.optim.ClipAdam._build_table lays them out tile every segment exactly once."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as OR


def _r32(x):
    return float(np.float32(x))


# ---- the reference against torch
@pytest.mark.parametrize("kind", ["finite", "nan", "inf"])
@pytest.mark.parametrize("betas,max_norm,inv", [((0.9, 0.999), 1.5, 1.0), ((0.8, 0.99), 40.0, 0.25), ((0.0, 0.0), 1e9, 1.0),
                                                ((0.5, 0.5), 0.7, 0.25)])
def test_reference_equals_clip_grad_norm_plus_torch_adam_in_float64(kind, betas, max_norm, inv):
    """three steps, per-group lr and weight decay; gradients that are sums over 4 ranks are handed to torch divided by 4 (exact)"""
    rng = np.random.default_rng(5)
    sizes, lrs, wds = (5, 37, 130, 1), (1e-3, 1e-4, 1e-3, 0.0), (0.0, 0.01, 0.01, 0.0)
    b1, b2, eps = _r32(betas[0]), _r32(betas[1]), _r32(OR.EPS)
    ps = [rng.standard_normal(n).astype(np.float32).astype(np.float64) for n in sizes]
    ms = [np.zeros(n) for n in sizes]
    vs = [np.zeros(n) for n in sizes]
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in ps]
    opt = torch.optim.Adam([{"params": [q], "lr": _r32(lr), "weight_decay": _r32(wd)} for q, lr, wd in zip(tp, lrs, wds)],
                           betas=(b1, b2), eps=eps, foreach=False)
    for it in range(3):
        gs = [(rng.standard_normal(n) * (30.0 if it == 1 else 1.0)).astype(np.float32).astype(np.float64) for n in sizes]
        if it == 0 and kind != "finite":
            gs[1][7] = float(kind)
        for q, g in zip(tp, gs):
            q.grad = torch.from_numpy(g * inv)
        n_t = torch.nn.utils.clip_grad_norm_(tp, _r32(max_norm))
        opt.step()
        norm, coef = OR.norm_coef_fp64(gs, max_norm, inv)
        np.testing.assert_allclose(norm, float(n_t), rtol=1e-12)
        for i, (q, g) in enumerate(zip(tp, gs)):
            r = OR.step_fp64(ps[i], g, ms[i], vs[i], it, lrs[i], wds[i], b1, b2, eps, coef)
            ps[i], ms[i], vs[i] = r.p, r.m, r.v
            st = opt.state[q]
            np.testing.assert_allclose(r.g, q.grad.numpy(), rtol=1e-12, atol=0, equal_nan=True)
            np.testing.assert_allclose(r.p, q.detach().numpy(), rtol=1e-12, atol=0, equal_nan=True)
            np.testing.assert_allclose(r.m, st["exp_avg"].numpy(), rtol=1e-12, atol=0, equal_nan=True)
            np.testing.assert_allclose(r.v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0, equal_nan=True)
            assert float(st["step"]) == it + 1
    if kind == "nan":
        assert all(np.isnan(p).all() for p in ps)                      # one NaN element poisons every parameter
    if kind == "inf":
        assert np.isnan(ps[1][7]) and np.isfinite(np.delete(ps[1], 7)).all() and np.isfinite(ps[0]).all()


def test_norm_coef_edges():
    g = [np.array([3.0, 0.0]), np.array([4.0])]
    assert OR.norm_coef_fp64(g, 0.0, 0.25) == (1.25, 0.25)
    assert OR.norm_coef_fp64(g, -1.0, 1.0) == (5.0, 1.0)
    assert OR.norm_coef_fp64(g, 10.0, 0.5) == (2.5, 0.5)                # below max_norm: inv
    n, c = OR.norm_coef_fp64(g, 1.0, 1.0)
    assert n == 5.0 and c == 1.0 / (5.0 + OR.TINY)
    n, c = OR.norm_coef_fp64([np.array([1.0, float("nan")])], 1.0, 1.0)
    assert n != n and c != c
    n, c = OR.norm_coef_fp64([np.array([1.0, float("nan")])], 0.0, 0.5)
    assert n != n and c == 0.5
    n, c = OR.norm_coef_fp64([np.array([1.0, float("inf")])], 1.0, 1.0)
    assert n == float("inf") and c == 0.0


# ---- the float32 restatement of the kernel inside the bounds
def _restated(table, variant=None, coef_variant=None):
    vals = OR.values(table)
    gs = [vals.g[a:b] for a, b in zip(vals.off[:-1], vals.off[1:])]
    norm, coef = OR.norm_coef_f32(gs, table.max_norm, table.inv, coef_variant)
    got = OR.step_f32(vals.p, vals.g, vals.m, vals.v, vals.t, vals.lr, vals.wd, table.betas[0], table.betas[1], OR.EPS, coef, variant)
    return vals, norm, coef, got, OR.reference(table, vals, coef)


def _ratios(got, ref):
    return {k: OR.ratio(g, w, b)[0] for k, g, w, b in (("p", got[0], ref.p, ref.ep), ("m", got[1], ref.m, ref.em),
                                                       ("v", got[2], ref.v, ref.ev), ("g", got[3], ref.g, ref.eg))}


def test_restatement_stays_inside_the_bounds_and_k_is_four_times_its_worst_ratio():
    worst = dict(p=(0.0, ""), m=(0.0, ""), v=(0.0, ""), g=(0.0, ""))
    for table in OR.ADAM_TABLES:
        _vals, _norm, _coef, got, ref = _restated(table)
        for k, r in _ratios(got, ref).items():
            if r > worst[k][0]:
                worst[k] = (r, table.name)
    print("worst |float32 restatement - fp64| / bound (without K): " + ", ".join("%s %.4f (%s)" % ((k,) + w) for k, w in worst.items()))
    top = max(worst[k][0] for k in "pmv")
    print("worst ratio %.4f -> K = 4 x = %.3f (optim_ref.K = %g)" % (top, 4 * top, OR.K))
    assert worst["g"][0] <= 1.0                                        # one rounding: no constant
    assert abs(top - OR.WORST_RATIO) < 5e-4, (top, OR.WORST_RATIO)
    assert 4 * OR.WORST_RATIO <= OR.K < 4 * OR.WORST_RATIO + 0.05
    for k in "pmv":
        assert worst[k][0] * 4 <= OR.K


def test_a_rounded_reference_passes_and_nonfinite_results_are_compared_exactly():
    table = OR.TABLES["shape-257"]
    vals = OR.values(table)
    ref = OR.reference(table, vals, 0.01)
    f = np.float32
    OR.check_elements(ref.p.astype(f), ref.m.astype(f), ref.v.astype(f), ref.g.astype(f), ref, "rounded reference", k=1.0)
    bad = ref.p.astype(f).copy()
    bad[3] = np.nan
    with pytest.raises(AssertionError):
        OR.check_elements(bad, ref.m.astype(f), ref.v.astype(f), None, ref, "a NaN where a number belongs")
    nan_ref = OR.reference(table, vals, float("nan"))
    assert np.isnan(nan_ref.p).all() and np.isnan(nan_ref.m).all() and np.isnan(nan_ref.v).all()
    with pytest.raises(AssertionError):
        OR.check_elements(ref.p.astype(f), nan_ref.m.astype(f), nan_ref.v.astype(f), None, nan_ref, "a number where NaN belongs")


# ---- the bounds notice a wrong kernel
@pytest.mark.parametrize("variant", OR.VARIANTS)
def test_wrong_kernel_leaves_the_bounds(variant):
    caught = []
    for table in OR.HYPER_TABLES + OR.SHAPE_TABLES[:2]:
        _vals, _norm, _coef, got, ref = _restated(table, variant)
        try:
            r = _ratios(got, ref)
        except AssertionError:                                        # an Inf / NaN where the reference has a number, or the reverse
            r = {"nonfinite": float("inf")}
        out = {k: x for k, x in r.items() if x > OR.K}
        if out:
            caught.append((table.name, out))
    assert caught, variant
    print("%s: caught by %d tables, first %s: %s" % (variant, len(caught), caught[0][0],
                                                      ", ".join("%s at %.3g x the bound" % (k, x / OR.K) for k, x in caught[0][1].items())))


def test_wrong_bias_corrections_are_invisible_at_large_step_counts():
    """why the small step counts are in the case list: with t - 1 in place of t, or without bc2, a segment at t_before = 99999 stays
    inside the bounds (beta^t underflowed long ago), and one at t_before <= 9 does not"""
    table = OR.TABLES["hyper-b0.9-0.999-wd0"]
    for variant in ("t_minus_1", "no_bc2"):
        vals, _norm, _coef, got, ref = _restated(table, variant)
        late, early = vals.t == 99999, (vals.t >= 1) & (vals.t <= 9) & (vals.lr > 0)
        assert late.any() and early.any()
        assert OR.ratio(got[0][late], ref.p[late], ref.ep[late])[0] <= OR.K
        assert OR.ratio(got[0][early], ref.p[early], ref.ep[early])[0] > OR.K


@pytest.mark.parametrize("variant", OR.ALLOWED)
def test_another_correct_kernel_stays_inside(variant):
    """m = beta1 m + (1 - beta1) g is Adam too: the bound must not be so tight that it singles out one operation order"""
    top = 0.0
    for table in OR.HYPER_TABLES + OR.SHAPE_TABLES[:5] + OR.SIZE_TABLES[:1]:
        _vals, _norm, _coef, got, ref = _restated(table, variant)
        top = max(top, max(_ratios(got, ref)[k] for k in "pmv"))
    print("%s: worst ratio %.3f of the bound without K, %.3f with" % (variant, top, top / OR.K))
    assert top <= OR.K


def test_coefficient_without_inv_is_caught():
    caught = []
    for table in OR.HYPER_TABLES:
        _vals, norm, coef, _got, _ref = _restated(table)
        OR.check_coef(norm, coef, table.max_norm, table.inv, table.name)            # the right one passes
        _vals, norm, coef, _got, _ref = _restated(table, coef_variant="coef_no_inv")
        try:
            OR.check_coef(norm, coef, table.max_norm, table.inv, table.name)
        except AssertionError:
            caught.append(table.name)
    assert caught
    print("coef without inv: caught by", ", ".join(caught))


def test_norm_bound_is_tight_enough_to_mean_something():
    """small tables: well inside the 2e-6 of tests/test_gpu_train.py; a full chunk's 256-term sequential sums: below 1e-5"""
    t = OR.TABLES["shape-300"]
    assert OR.norm_rel_bound([s.n for s in t.segs], 300) < 1e-6
    t = OR.TABLES["shape-513-chunks"]
    assert OR.norm_rel_bound([s.n for s in t.segs], 513) < 1e-5
    # the float32 restatement's norm (numpy's pairwise sums: another order, fewer roundings on a path) is inside
    for table in OR.ADAM_TABLES[:12]:
        vals, norm, _coef, _got, _ref = _restated(table)
        gs = [vals.g[a:b] for a, b in zip(vals.off[:-1], vals.off[1:])]
        ns = [s.n for s in table.segs]
        OR.check_norm(float(norm), gs, table.inv, ns, len(OR.chunk_table(ns)[0]), table.name)
    with pytest.raises(AssertionError):
        OR.check_norm(float(norm) * (1 + 2e-5), gs, table.inv, ns, len(OR.chunk_table(ns)[0]), "a norm 2e-5 off")


# ---- the tables
def test_table_records_have_the_layout_of_the_c_structs():
    from cvc import hip
    from cvc.optim import _CHUNK_DT, _SEG_DT
    assert _SEG_DT.itemsize == C.sizeof(hip.OptimSeg) == 56 and _CHUNK_DT.itemsize == C.sizeof(hip.OptimChunk) == 16
    for dt, st in ((_SEG_DT, hip.OptimSeg), (_CHUNK_DT, hip.OptimChunk)):
        for (name, _ctype), np_name in zip(st._fields_, dt.names):
            assert dt.fields[np_name][1] == getattr(st, name).offset and dt.fields[np_name][0].itemsize == getattr(st, name).size


def test_case_lists_hold_what_they_should():
    C_ = OR.CHUNK
    assert set(OR.SIZES) == {1, 2, 3, 4, 5, 7, 8, 255, 256, 1023, 1024, 1025, 1027, C_ - 1, C_, C_ + 1, C_ + 4, 2 * C_ + 3, 3 * C_ + 1025}
    assert len(OR.FORMS) == 13 and len(set(OR.FORMS)) == 13 and all(sum(1 for o in f if o) <= 1 and max(f) <= 3 for f in OR.FORMS)
    seen = {(s.n, s.offs) for t in OR.SIZE_TABLES for s in t.segs}
    for n in OR.SMALL_N + OR.MID_N:
        assert all((n, f) in seen for f in OR.FORMS), n
    for n in OR.LARGE_N:
        assert {f for (k, f) in seen if k == n} >= {OR.ALIGNED, (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1)}
    for t in OR.HYPER_TABLES:
        assert {(s.t, s.lr) for s in t.segs} == {(a, b) for a in OR.T_BEFORE for b in OR.LRS}
    assert {(t.betas, t.segs[0].wd) for t in OR.HYPER_TABLES} == {(b, w) for b in OR.BETAS for w in OR.WDS}
    shapes = {t.name: (len(t.segs), len(OR.chunk_table([s.n for s in t.segs])[0])) for t in OR.SHAPE_TABLES}
    assert shapes == {"shape-1-1": (1, 1), "shape-255": (255, 255), "shape-256": (256, 256), "shape-257": (257, 257),
                      "shape-300": (300, 300), "shape-300+2": (302, 305), "shape-513-chunks": (511, 513)}
    for t in OR.ADAM_TABLES:
        assert sum(s.n for s in t.segs) < 700000, t.name               # a few hundred thousand elements at the most
        v = OR.values(t)
        assert (v.g == 0).any() or len(v.g) < 20
        assert (v.v >= 0).all() and (np.abs(v.m) <= np.sqrt(v.v) * (1 + 1e-6)).all()
        assert not v.m[v.t == 0].any() and not v.v[v.t == 0].any()


def test_chunks_tile_every_segment_exactly_once_and_slots_do_not_overlap():
    for t in OR.ADAM_TABLES:
        ns = [s.n for s in t.segs]
        seg, start = OR.chunk_table(ns)
        # the kernels' range of a chunk: [start, min(start + CHUNK, n))
        cover = [np.zeros(n, dtype=np.int32) for n in ns]
        for s, a in zip(seg, start):
            assert 0 <= a < ns[s] and a % OR.CHUNK == 0
            cover[s][a:min(a + OR.CHUNK, ns[s])] += 1
        assert all((c == 1).all() for c in cover), t.name
        assert (np.diff(seg) >= 0).all() and set(seg) == set(range(len(ns)))
        # ClipAdam._build_table's own arithmetic, restated
        counts = np.array([(n + OR.CHUNK - 1) // OR.CHUNK for n in ns], dtype=np.int64)
        first = np.concatenate(([0], np.cumsum(counts)[:-1]))
        assert np.array_equal(np.repeat(np.arange(len(ns)), counts), seg)
        assert np.array_equal((np.arange(int(counts.sum())) - np.repeat(first, counts)) * OR.CHUNK, start)
        starts, size = OR.layout(t.segs)
        used = np.zeros(size, dtype=np.int32)
        for s, a in zip(t.segs, starts):
            assert a % 4 == 0
            for o in s.offs:
                used[a + o:a + o + s.n] += 1
        assert used.max() <= 4 and not used[:OR.BAND].any() and not used[-OR.BAND:].any()
        for s, a, b in zip(t.segs, starts, starts[1:] + [size - OR.BAND]):
            assert a + 3 + s.n <= b - 1                                # at least one sentinel float between two segments, any offset
