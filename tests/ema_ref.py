"""Reference, error bound, case lists and comparisons of the weight average kept inside the optimizer step (csrc/optim.hip: the
EMA forms of the three update kernels behind cvc_adam / sgd / adamax_clip_step_ema, optim_finalize_ema_kernel, ema_swap_kernel).
Nothing here needs a GPU: tests/test_ema_ref_cpu.py shows that a float32 restatement stays inside the bound and that wrong kernels
leave it; tests/test_gpu_ema_kernels.py holds the kernels to it.

The rule, per element, from the p the update has just produced:
    d_eff = warmup ? min(d, (1 + n) / (10 + n)) : d         n = averaged (non-void) steps BEFORE this one; then n += 1
    e     = fma(p_new - e, 1 - d_eff, e)                    (1 - d_eff formed in float32)
A void step moves neither e nor n.  ema_fp64 is that in numpy float64, FED the device's own p_new and d_eff (as optim_ref feeds the
device's clip coefficient): the parameter's rounding is tests/optim_ref.py's business, the decay's is checked on its own against
d_eff_fp64 -- one correctly rounded division, so within u d_eff.  Next to e it returns the bound WITHOUT the constant,
    u (|p_new - e| (1 - d_eff) + |e_new|)                   u = 2^-24
-- the difference's rounding and (1 - d_eff)'s, u |p_new - e| (1 - d_eff) each to first order, and the fma's own u |e_new| -- and the
comparisons multiply it by the project's K = 4 (tests/optim_ref.py).  The float32 restatement ema_f32 rounds the product as well
(numpy has no fma): its worst |ema_f32 - ema_fp64| / bound over EMA_TABLES is WORST_RATIO, printed and pinned by the CPU test.
    measured worst ratio: 1.92 (without K)  ->  0.48 of K x bound
p_new == e gives p_new - e = +0 and e = fma(0, x, e) = e: the average of a frozen or converged weight keeps its BITS, which the
other correct form d e + (1 - d) p does not (ALLOWED below: inside the bound, but it fails the property)."""
import collections
import zlib

import numpy as np

from optim_ref import BAND, CHUNK, K, SENTINEL, U, f32, ratio       # noqa: F401 -- the GPU file takes them from here

WORST_RATIO = 1.92                  # of ema_f32 against the bound WITHOUT K over EMA_TABLES (test_ema_ref_cpu.py keeps it honest)

F = np.float32


# ------------------------------------------------------------------------------------------------ the reference
def d_eff_fp64(d, n, warmup):
    """the effective decay of the step that follows n averaged steps, in float64 (d rounded to float32 first: what the entry is handed)"""
    d = float(f32(d))
    return min(d, (1.0 + n) / (10.0 + n)) if warmup else d


def ema_fp64(p_new, e, d_eff):
    """-> (e_new, bound without K).  d_eff: the float32 value the step used (a scalar or per element)"""
    p_new, e = np.asarray(p_new, dtype=np.float64), np.asarray(e, dtype=np.float64)
    omd = 1.0 - f32(d_eff)
    with np.errstate(all="ignore"):
        diff = p_new - e
        e1 = e + diff * omd
        return e1, U * (np.abs(diff) * omd + np.abs(e1))


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in float32
VARIANTS = ("p_old", "d_exchanged", "warmup_n_plus_1", "void_updates", "void_counts")        # wrong kernels
ALLOWED = ("two_products",)                                                                 # numerically fine, fails the property


def d_eff_f32(d, n, warmup, variant=None):
    n = F(n) + (F(1) if variant == "warmup_n_plus_1" else F(0))
    return np.minimum(F(d), (F(1) + n) / (F(10) + n)) if warmup else F(d)


def ema_f32(p_old, p_new, e, d, n, warmup, void=False, variant=None):
    """one step of the average in numpy float32, one rounding per operation -> (e_new, n_new, d_eff).  p_old: the parameter before
    the step, which only the wrong variant "p_old" reads."""
    p_old, p_new, e = (np.asarray(x, dtype=F) for x in (p_old, p_new, e))
    if void and variant not in ("void_updates", "void_counts"):
        return e.copy(), F(n), None
    de = d_eff_f32(d, n, warmup, variant)
    n1 = F(n) if (void and variant == "void_updates") else F(n) + F(1)
    if void and variant == "void_counts":
        return e.copy(), n1, de
    omd = F(1) - de
    src = p_old if variant == "p_old" else p_new
    with np.errstate(all="ignore"):
        if variant == "d_exchanged":
            e1 = e + (src - e) * de
        elif variant == "two_products":
            e1 = de * e + omd * src
        else:
            e1 = e + (src - e) * omd
    return e1, n1, de


# ------------------------------------------------------------------------------------------------ the cases
DECAYS = (0.0, 0.5, 0.9, 0.999, 0.9999)
N_BEFORE = (0, 1, 9, 10 ** 5)
Table = collections.namedtuple("Table", "name size d n warmup")
EMA_TABLES = [Table("ema-d%g-n%d-%s" % (d, n, "warm" if w else "flat"), 4099, d, n, w) for d in DECAYS for n in N_BEFORE for w in (False, True)]
TABLES = {t.name: t for t in EMA_TABLES}

Values = collections.namedtuple("Values", "p_old p_new e same")


def shadow_values(p_new, p_old, seed):
    """a shadow for every element of one step: a third exactly p_new (`same`: the average of a weight that has stopped moving), a
    third a trailing average (between the old value and a little behind it), the rest far away at scales 1e-3, 1, 30; signs mixed"""
    rng = np.random.default_rng(seed)
    p_new, p_old = np.asarray(p_new, dtype=F), np.asarray(p_old, dtype=F)
    n = p_new.size
    kind = rng.integers(0, 3, n)
    trail = p_old + (p_old - p_new) * rng.uniform(0.0, 50.0, n).astype(F)
    far = (rng.standard_normal(n) * np.array([1e-3, 1.0, 30.0])[rng.integers(0, 3, n)]).astype(F)
    e = np.where(kind == 0, p_new, np.where(kind == 1, trail, far)).astype(F)
    return e, (kind == 0) & np.isfinite(p_new)


def values(table):
    """seeded operands of one table: parameters of scale 1 that an update of relative size 1e-3 .. 1e-1 has just moved"""
    rng = np.random.default_rng(zlib.crc32(table.name.encode()))
    p_old = rng.standard_normal(table.size).astype(F)
    p_new = (p_old - p_old * (10.0 ** rng.uniform(-3, -1, table.size)) * rng.choice([-1.0, 1.0], table.size)).astype(F)
    p_new[rng.random(table.size) < 0.05] = 0.0
    e, same = shadow_values(p_new, p_old, zlib.crc32(table.name.encode()) + 1)
    return Values(p_old, p_new, e, same)


# ------------------------------------------------------------------------------------------------ the comparisons
def check_shadow(got_e, p_new, e_before, d_eff, what, same=None, k=None):
    """e of one step inside K x the bound under the step's own p_new and d_eff; where p_new == e_before (bitwise, `same` or every
    such element) e keeps its bits.  Prints and returns the max ratio (of K x bound)."""
    k = K if k is None else k
    want, bound = ema_fp64(p_new, e_before, d_eff)
    r, err = ratio(got_e, want, k * bound)
    print("%s: e ratio %.3g max |err| %.3g" % (what, r, err))
    assert r <= 1.0, "%s: e leaves its bound, worst |err| / (K x bound) = %.4g" % (what, r)
    pb, eb = (np.ascontiguousarray(x, dtype=F).ravel().view(np.uint32) for x in (p_new, e_before))
    still = (pb == eb) & np.isfinite(np.asarray(p_new, dtype=F).ravel())
    if same is not None:
        assert still[np.asarray(same).ravel()].all()
    gb = np.ascontiguousarray(got_e, dtype=F).ravel().view(np.uint32)
    assert np.array_equal(gb[still], eb[still]), "%s: p_new == e moved e" % what
    return r
