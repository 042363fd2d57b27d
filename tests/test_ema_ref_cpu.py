"""tests/ema_ref.py proven on the CPU (no GPU here): the float32 restatement of the weight average stays inside the bound on every
table (the worst ratio is printed and pinned), every subtly wrong kernel leaves it -- or breaks the exact void-step rules -- on a
committed case, the other correct form d e + (1 - d) p stays inside but moves a converged weight's average, and the warm-up's
effective decay follows its fp64 statement."""
import numpy as np
import pytest

import ema_ref as ER
from optim_ref import K, U

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _run(table, variant=None, void=False):
    v = ER.values(table)
    e1, n1, de = ER.ema_f32(v.p_old, v.p_new, v.e, table.d, table.n, table.warmup, void, variant)
    return v, e1, n1, de


def _ratio(table, variant=None):
    """worst |restatement - fp64| / bound (WITHOUT K) under the CORRECT effective decay"""
    v, e1, _n1, _de = _run(table, variant)
    want, bound = ER.ema_fp64(v.p_new, v.e, ER.d_eff_f32(table.d, table.n, table.warmup))
    return ER.ratio(e1, want, bound)[0]


def test_restatement_stays_inside_the_bound_and_the_worst_ratio_is_pinned():
    worst, where = 0.0, ""
    for table in ER.EMA_TABLES:
        r = _ratio(table)
        if r > worst:
            worst, where = r, table.name
        v, e1, n1, de = _run(table)
        ER.check_shadow(e1, v.p_new, v.e, de, table.name, same=v.same)
        assert n1 == table.n + 1
    print("worst |ema_f32 - ema_fp64| / bound over %d tables: %.4g at %s (K = %g)" % (len(ER.EMA_TABLES), worst, where, K))
    assert worst <= K
    assert abs(worst - ER.WORST_RATIO) <= 0.005, worst


@pytest.mark.parametrize("variant", ["p_old", "d_exchanged", "warmup_n_plus_1"])
def test_a_wrong_average_leaves_the_bound(variant):
    left = {}
    for table in ER.EMA_TABLES:
        r = _ratio(table, variant) / K
        if r > 1.0:
            left[table.name] = r
    print("%s leaves K x bound on %d of %d tables, e.g. %s" % (variant, len(left), len(ER.EMA_TABLES), sorted(left.items())[:2]))
    assert left
    if variant == "p_old":
        assert len(left) == len([t for t in ER.EMA_TABLES if ER.d_eff_f32(t.d, t.n, t.warmup) < 1])
    if variant == "warmup_n_plus_1":               # only where the warm-up, not d, decides; never without it
        assert all(ER.TABLES[n].warmup for n in left) and "ema-d0.9999-n0-warm" in left and "ema-d0.9999-n9-warm" in left
    if variant == "d_exchanged":                   # (d = 0.5 is its own exchange)
        assert "ema-d0.5-n0-flat" not in left and "ema-d0.999-n0-flat" in left and "ema-d0-n1-flat" in left


@pytest.mark.parametrize("variant", ["void_updates", "void_counts"])
def test_a_void_step_moves_neither_the_average_nor_the_counter(variant):
    table = ER.TABLES["ema-d0.9-n9-flat"]
    v, e1, n1, _de = _run(table, void=True)
    assert np.array_equal(_bits(e1), _bits(v.e)) and n1 == 9
    v, e1, n1, _de = _run(table, variant, void=True)
    assert not (np.array_equal(_bits(e1), _bits(v.e)) and n1 == 9)


def test_two_products_is_inside_the_bound_but_moves_a_converged_average():
    moved = 0
    for table in ER.EMA_TABLES:
        assert _ratio(table, "two_products") <= K, table.name
        v, e1, _n1, _de = _run(table, "two_products")
        moved += int((_bits(e1)[v.same] != _bits(v.e)[v.same]).sum())
        v, e1, _n1, _de = _run(table)
        assert v.same.sum() > 1000 and np.array_equal(_bits(e1)[v.same], _bits(v.e)[v.same])
    print("d e + (1 - d) p moved %d converged elements" % moved)
    assert moved > 0
    with pytest.raises(AssertionError, match="moved e"):
        table = ER.TABLES["ema-d0.9-n9-flat"]
        v, e1, _n1, de = _run(table, "two_products")
        ER.check_shadow(e1, v.p_new, v.e, de, "two_products", same=v.same)


@pytest.mark.parametrize("d", [0.9, 0.9999])
def test_warmup_sequence_against_fp64(d):
    for n in ER.N_BEFORE:
        got, want = float(ER.d_eff_f32(d, n, True)), ER.d_eff_fp64(d, n, True)
        print("d %g n %d: d_eff %.9g (fp64 %.12g)" % (d, n, got, want))
        assert abs(got - want) <= U * want
        assert float(ER.d_eff_f32(d, n, False)) == float(F(d)) == ER.d_eff_fp64(d, n, False)
    assert ER.d_eff_fp64(0.9999, 0, True) == 0.1 and ER.d_eff_fp64(0.9999, 1, True) == 2.0 / 11.0
    assert ER.d_eff_fp64(0.9999, 9, True) == 10.0 / 19.0 and ER.d_eff_fp64(0.9, 10 ** 5, True) == float(F(0.9))
    # (after 10^5 steps the warm-up no longer binds even d = 0.9999: 100001 / 100010 = 0.99991)
    assert ER.d_eff_fp64(0.9999, 10 ** 5, True) == float(F(0.9999)) < 100001.0 / 100010.0
    assert ER.d_eff_fp64(0.9999, 1000, True) == 1001.0 / 1010.0
