"""Reference, error bounds, case lists and comparisons of tests/test_gpu_optim_kernels.py (the optimizer step of csrc/optim.hip:
optim_sumsq_kernel, optim_finalize_kernel, optim_adam_kernel behind cvc_adam_clip_step, driven by cvc.optim.ClipAdam).  Nothing
here needs a GPU: tests/test_optim_ref_cpu.py proves the reference against torch.optim.Adam on float64 CPU tensors, shows that a
float32 restatement of the kernel's arithmetic stays inside the bounds, and that wrong kernels leave them.

step_fp64 is ONE Adam step in numpy float64 with the arithmetic of csrc/optim.hip's header comment (torch.optim.Adam, no amsgrad,
no maximize); the scalar hyper-parameters are rounded to float32 first, which is what the kernel is handed, and the clip
coefficient is an INPUT (the GPU file feeds it the device's own coefficient, so the norm's rounding does not leak into the
element-wise comparison).  Next to every value it returns a first-order bound of the float32 evaluation's error: every float32
rounding contributes u = 2^-24 times the magnitude of its result, and the contributions are carried through the later operations
with those operations' derivatives.  The bound therefore carries the conditioning of
    g coef + wd p                      u (|g coef| + |wd p| + |sum|): large against the sum under cancellation
    m + (ge - m) (1 - beta1)           u (|ge - m| (1 - beta1) ...) + u |m'|: cancellation against a large old m
    1 - beta^t                         the error of pow (2 u beta^t: powf is not correctly rounded) and of the subtraction, divided by
                                       bc (step_size = lr / bc1) and by 2 bc2 (1 / sqrt(bc2)): the factor 1 / bc at small t
    m' / (sqrt(v') / sqrt(bc2) + eps)  the errors of m' and of the denominator over den and den^2
and is multiplied by ONE constant K.  K is measured, not derived, and never from a kernel's output: step_f32 restates `upd` of
optim_adam_kernel in numpy float32, operation by operation in the kernel's order (wd != 0 ? g + wd p : g, step_size = lr / bc1,
inv_sqrt_bc2 = 1 / sqrtf(bc2)), and K = 4 x the worst |step_f32 - step_fp64| / bound over every table of ADAM_TABLES.  The margin
of 4 is for what the device may legitimately do differently from numpy: FMAs (the kernel spells g + wd p, the two moments' updates,
the denominator and p's update as fmaf: one rounding where numpy has two) and a powf a couple of ulp off.
    measured worst ratio: 0.999 (p 0.9992, m 0.9646, v 0.9863: a rounding next to a power of two fills its u |x|)  ->  K = 4.0
(tests/test_optim_ref_cpu.py prints the ratio and asserts that K is 4 x it, to the digits given.)  The written gradient g coef is a
single rounding: its bound is u |g coef| with no constant.

The norm's bound comes from the summation structure of the two reduction kernels, see norm_depth()."""
import collections
import itertools
import math
import zlib

import numpy as np

U = 2.0 ** -24
K = 4.0
WORST_RATIO = 0.999                 # of step_f32 against the bounds over ADAM_TABLES (test_optim_ref_cpu.py keeps it honest)
CHUNK = 65536                       # cvc_optim_chunk_elems(); the GPU file asserts that the library agrees
WG = 256                            # OPT_WG of csrc/optim.hip
BAND = 64                           # sentinel floats on both sides of every arena
SENTINEL = -777.0
EPS = 1e-8
TINY = float(np.float32(1e-6))      # the 1e-6f of the clip coefficient


def f32(x):
    """x rounded to float32, as float64"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the reference
def norm_coef_fp64(gs, max_norm, inv):
    """(sqrt(sum g^2) inv, min(1, max_norm / (norm + 1e-6)) inv) in float64; the coefficient is inv when max_norm <= 0 and NaN when
    the norm is NaN (torch's clamp(NaN, max=1))"""
    max_norm, inv = float(f32(max_norm)), float(f32(inv))
    s = 0.0
    with np.errstate(all="ignore"):
        for g in gs:
            g = np.asarray(g, dtype=np.float64).ravel()
            s += float(np.sum(g * g))
        norm = math.sqrt(s) * inv if s == s else float("nan")
    if max_norm <= 0:
        return norm, inv
    if norm != norm:
        return norm, float("nan")
    return norm, min(1.0, max_norm / (norm + TINY)) * inv


Step = collections.namedtuple("Step", "p m v g ep em ev eg")


def step_fp64(p, g, m, v, t_before, lr, wd, beta1, beta2, eps, coef):
    """One Adam step in float64 -> Step(p, m, v, written gradient, and the bound of each WITHOUT the constant K).  t_before, lr and
    wd may be per-element arrays (one table's segments side by side)."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    lr, wd, b1, b2, eps, coef = f32(lr), f32(wd), float(f32(beta1)), float(f32(beta2)), float(f32(eps)), float(coef)
    t = np.asarray(t_before, dtype=np.float64) + 1.0
    with np.errstate(all="ignore"):
        gc = g * coef;                      e_gc = U * np.abs(gc)
        wdp = wd * p
        ge = gc + wdp
        e_ge = np.where(wd != 0, e_gc + U * np.abs(wdp) + U * np.abs(ge), e_gc)
        # m' = m + (ge - m) (1 - beta1)
        d = ge - m;                         e_d = e_ge + U * np.abs(d)
        dm = d * (1.0 - b1);                e_dm = e_d * (1.0 - b1) + U * np.abs(dm)
        m1 = m + dm;                        e_m = e_dm + U * np.abs(m1)
        # v' = beta2 v + ((1 - beta2) ge) ge
        og = (1.0 - b2) * ge;               e_og = (1.0 - b2) * e_ge + U * np.abs(og)
        gg = og * ge;                       e_gg = e_og * np.abs(ge) + np.abs(og) * e_ge + U * np.abs(gg)
        bv = b2 * v;                        e_bv = U * np.abs(bv)
        v1 = bv + gg;                       e_v = e_bv + e_gg + U * np.abs(v1)
        # bias corrections: pow within 2 ulp, then 1 - pow
        pw1, pw2 = np.power(b1, t), np.power(b2, t)
        bc1 = 1.0 - pw1;                    e_bc1 = 2 * U * pw1 + U * bc1
        bc2 = 1.0 - pw2;                    e_bc2 = 2 * U * pw2 + U * bc2
        ss = lr / bc1;                      e_ss = np.abs(lr) * e_bc1 / (bc1 * bc1) + U * np.abs(ss)
        sq2 = np.sqrt(bc2);                 e_sq2 = e_bc2 / (2 * sq2) + U * sq2
        isb = 1.0 / sq2;                    e_isb = e_sq2 / (sq2 * sq2) + U * isb
        sv = np.sqrt(v1);                   e_sv = np.where(v1 > 0, e_v / (2 * np.where(v1 > 0, sv, 1.0)), 0.0) + U * sv
        sc = sv * isb;                      e_sc = e_sv * isb + sv * e_isb + U * sc
        den = sc + eps;                     e_den = e_sc + U * den
        q = m1 / den;                       e_q = e_m / den + np.abs(m1) * e_den / (den * den) + U * np.abs(q)
        up = ss * q;                        e_up = e_ss * np.abs(q) + np.abs(ss) * e_q + U * np.abs(up)
        p1 = p - up;                        e_p = e_up + U * np.abs(p1)
    return Step(p1, m1, v1, gc, e_p, e_m, e_v, e_gc)


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in float32
VARIANTS = ("t_minus_1", "no_bc2", "eps_in_sqrt", "adamw", "wd_unclipped", "v_from_g")       # wrong kernels (elements)
ALLOWED = ("m_two_products",)                                                               # another correct kernel


def step_f32(p, g, m, v, t_before, lr, wd, beta1, beta2, eps, coef, variant=None):
    """`upd` of optim_adam_kernel (csrc/optim.hip) in numpy float32, one rounding per operation, in the kernel's order ->
    (p, m, v, written gradient).  variant: one of VARIANTS (a subtly wrong kernel) or ALLOWED."""
    F = np.float32
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    lr, wd = np.asarray(lr, dtype=F), np.asarray(wd, dtype=F)
    b1, b2, eps, coef, one = F(beta1), F(beta2), F(eps), F(coef), F(1)
    t = (np.asarray(t_before, dtype=np.float64) + 1.0).astype(F)         # the step count after the finalize launch's += 1
    with np.errstate(all="ignore"):
        tp = t - one if variant == "t_minus_1" else t
        bc1, bc2 = one - np.power(b1, tp).astype(F), one - np.power(b2, tp).astype(F)
        step_size = lr / bc1
        inv_sqrt_bc2 = np.ones_like(bc2) if variant == "no_bc2" else one / np.sqrt(bc2)
        omb1, omb2 = one - b1, one - b2
        if variant == "adamw":
            p = p - (lr * wd) * p
        gc = g * coef
        if variant == "adamw":
            ge = gc
        elif variant == "wd_unclipped":
            ge = np.where(wd != 0, (g + wd * p) * coef, gc)
        else:
            ge = np.where(wd != 0, gc + wd * p, gc)
        if variant == "m_two_products":
            m1 = b1 * m + omb1 * ge
        else:
            m1 = m + (ge - m) * omb1
        gv = gc if variant == "v_from_g" else ge
        v1 = b2 * v + omb2 * gv * gv
        if variant == "eps_in_sqrt":
            den = np.sqrt(v1 * inv_sqrt_bc2 * inv_sqrt_bc2 + eps)
        else:
            den = np.sqrt(v1) * inv_sqrt_bc2 + eps
        p1 = p - step_size * (m1 / den)
    return p1, m1, v1, gc


def norm_coef_f32(gs, max_norm, inv, variant=None):
    """optim_finalize_kernel's norm and coefficient in float32 (the sums in numpy's order).  variant "coef_no_inv": the wrong
    kernel that forgets the 1 / ranks in the clipped coefficient."""
    F = np.float32
    max_norm, inv = F(max_norm), F(inv)
    with np.errstate(all="ignore"):
        s = F(0)
        for g in gs:
            g = np.asarray(g, dtype=F).ravel()
            s = F(s + np.sum(g * g, dtype=F))
        total = F(np.sqrt(s) * inv)
        if not max_norm > 0:
            return total, inv
        if total != total:
            return total, total
        c = np.minimum(F(max_norm / F(total + F(1e-6))), F(1))
        return total, (c if variant == "coef_no_inv" else F(c * inv))


# ------------------------------------------------------------------------------------------------ the comparisons
def ratio(got, want, bound):
    """max |got - want| / bound over the elements whose reference is finite, after asserting that the others agree exactly (NaN
    where the reference is NaN, the same infinity where it is infinite).  A zero bound asks for the exact value."""
    got, want, bound = (np.asarray(x, dtype=np.float64).ravel() for x in (got, want, bound))
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    if got.size == 0:
        return 0.0, 0.0
    fin = np.isfinite(want)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), "a NaN of the reference is a number in the result"
    inf = ~fin & ~nan
    assert np.array_equal(got[inf], want[inf]), "an infinity of the reference is not the result's"
    with np.errstate(all="ignore"):
        err = np.abs(got[fin] - want[fin])
        r = np.where(err == 0, 0.0, err / bound[fin])
    if r.size == 0:
        return 0.0, 0.0
    r = np.where(np.isnan(r), np.inf, r)                     # a finite reference, a NaN result (or bound)
    err = np.where(np.isnan(err), np.inf, err)
    return float(r.max()), float(err.max())


def check_elements(got_p, got_m, got_v, got_g, ref, what, k=None):
    """p, m, v of one step inside K x the bounds of `ref` (a Step); the written gradient (None: not written) inside its single
    rounding.  Prints and returns the max ratios (of K x bound)."""
    k = K if k is None else k
    out = {}
    for name, got, want, bound in (("p", got_p, ref.p, k * ref.ep), ("m", got_m, ref.m, k * ref.em), ("v", got_v, ref.v, k * ref.ev),
                                   ("g", got_g, ref.g, ref.eg)):
        if got is None:
            continue
        out[name] = ratio(got, want, bound)
    print("%s: %s" % (what, ", ".join("%s ratio %.3g max |err| %.3g" % (n, r, e) for n, (r, e) in out.items())))
    for n, (r, _e) in out.items():
        assert r <= 1.0, "%s: %s leaves its bound, worst |err| / bound = %.4g" % (what, n, r)
    return {n: r for n, (r, _e) in out.items()}


def norm_depth(ns, nchunk):
    """Roundings on the longest path from one square to the sum of squares, as optim_sumsq_kernel and optim_finalize_kernel add:
        a thread's sequential sum over its share of one chunk   ceil(min(n, CHUNK) / 256) adds in the scalar form; the vector form
                                                                adds 4 squares as a tree (2 levels) per 1024 elements and up to 3
                                                                tail elements in one thread: fewer, bounded by the same + 5
        the square itself                                       1
        wave_sum                                                6 levels
        4 wave partials in thread 0                             3 adds
        thread t of the finalize launch: partial[t], [t + 256]  ceil(nchunk / 256) adds
        the same tree again                                     6 + 3
    Every term is >= 0, so the sum's relative error is at most depth x u (first order)."""
    longest = max(min(n, CHUNK) for n in ns)
    return (-(-longest // WG) + 5 + 1) + 6 + 3 + -(-nchunk // WG) + 6 + 3


def norm_rel_bound(ns, nchunk):
    """relative bound of the norm: half the sum's (the square root), + u for sqrtf's rounding, + u for the product with inv"""
    return (norm_depth(ns, nchunk) / 2 + 2) * U


def check_norm(norm_dev, gs, inv, ns, nchunk, what):
    want, _ = norm_coef_fp64(gs, 0.0, inv)
    rel = norm_rel_bound(ns, nchunk)
    if want != want or math.isinf(want):
        assert (norm_dev != norm_dev) if want != want else norm_dev == want, (what, norm_dev, want)
        return 0.0
    err = abs(float(norm_dev) - want)
    r = 0.0 if err == 0 else err / (rel * want)
    print("%s: norm %.9g, fp64 %.9g, rel err %.3g, bound %.3g (ratio %.3g)" % (what, norm_dev, want, err / want if want else 0, rel, r))
    assert r <= 1.0, "%s: the norm leaves its bound: %r against %r, relative bound %.3g" % (what, norm_dev, want, rel)
    return r


def check_coef(norm_dev, coef_dev, max_norm, inv, what="coef"):
    """the coefficient from the DEVICE's norm: an add, a division and a product, each rounded once -> within 4 u; inv exactly when
    max_norm <= 0 or the norm is clearly below max_norm; NaN from a NaN norm"""
    max_norm, inv = float(f32(max_norm)), float(f32(inv))
    norm_dev, coef_dev = float(norm_dev), float(coef_dev)
    if max_norm <= 0:
        assert coef_dev == inv, (what, coef_dev, inv)
        return
    if norm_dev != norm_dev:
        assert coef_dev != coef_dev, (what, coef_dev)
        return
    r = max_norm / (norm_dev + TINY)
    if r >= 1 + 4 * U:
        assert coef_dev == inv, (what, "unclipped", coef_dev, inv)
    elif r <= 1 - 4 * U:
        assert abs(coef_dev - r * inv) <= 4 * U * r * inv, (what, coef_dev, r * inv)
    else:
        assert abs(coef_dev - inv) <= 8 * U * inv, (what, coef_dev, inv)


# ------------------------------------------------------------------------------------------------ tables: layout
def chunk_table(ns, chunk=CHUNK):
    """(seg, start) of every chunk as cvc.optim.ClipAdam._build_table lays them out: segment by segment, ceil(n / chunk) each"""
    seg, start = [], []
    for i, n in enumerate(ns):
        for c in range(-(-n // chunk)):
            seg.append(i)
            start.append(c * chunk)
    return np.array(seg, dtype=np.int64), np.array(start, dtype=np.int64)


def layout(segs):
    """-> (slot starts, arena floats).  Each segment has a 16-byte-aligned slot in every arena (p, g, m, v place it at slot +
    offs[k]); BAND sentinel floats before the first and after the last slot and at least 4 between two slots."""
    pos, starts = BAND, []
    for s in segs:
        starts.append(pos)
        pos += (s.n + 3 + 3) // 4 * 4 + 4
    return starts, pos + BAND


# ------------------------------------------------------------------------------------------------ tables: the cases
Seg = collections.namedtuple("Seg", "n offs lr wd t")                 # offs: element offsets of (p, g, m, v) inside their slots
Table = collections.namedtuple("Table", "name segs betas max_norm inv")

ALIGNED = (0, 0, 0, 0)
FORMS = (ALIGNED,) + tuple(tuple(k if j == i else 0 for j in range(4)) for i in range(4) for k in (1, 2, 3))
FORM_NAMES = ("aligned",) + tuple("%s+%d" % (o, k) for o in "pgmv" for k in (1, 2, 3))
SMALL_N = (1, 2, 3, 4, 5, 7, 8, 255, 256, 1023, 1024, 1025, 1027)
MID_N = (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 4)
LARGE_N = (2 * CHUNK + 3, 3 * CHUNK + 1023 + 2)
SIZES = SMALL_N + MID_N + LARGE_N
BETAS = ((0.9, 0.999), (0.8, 0.99), (0.5, 0.5), (0.0, 0.0), (0.9, 0.0))
T_BEFORE = (0, 1, 2, 9, 999, 99999)
WDS = (0.0, 0.01)
LRS = (1e-3, 1e-4, 0.0)
DEFAULT_BETAS = BETAS[0]


def _cycle(i):
    """the lr / weight decay / step count of the i-th segment of a size or shape table: every value of each list, out of phase"""
    return LRS[i % 3], WDS[(i // 3) % 2], T_BEFORE[(i + i // 6) % 6]


def hyper_tables():
    """betas x weight decay; inside each, every t_before x every lr as segments of the small sizes, every alignment form.  The clip:
    active (max_norm 5), off (max_norm 0) and not reached (1e9); gradients as sums over 4 ranks (inv 0.25) on every other table."""
    out = []
    for bi, betas in enumerate(BETAS):
        for wi, wd in enumerate(WDS):
            segs = [Seg(SMALL_N[(i + bi) % 13], FORMS[(i + 2 * bi + wi) % 13], lr, wd, t)
                    for i, (t, lr) in enumerate(itertools.product(T_BEFORE, LRS))]
            out.append(Table("hyper-b%g-%g-wd%g" % (betas + (wd,)), segs, betas, (5.0, 0.0, 1e9)[(bi + wi) % 3], (1.0, 0.25)[(bi + wi) % 2]))
    return out


def size_tables():
    """every size x every alignment form.  The small sizes share one table; CHUNK - 1 .. CHUNK + 4 one table per form.  The two
    multi-chunk sizes take the aligned form and every operand alone off by 1, 2 or 3: the scalar forms of both kernels do not
    read the offset (i = start + thread, stride 256), the three values are one code path there, and each value occurs."""
    out = [Table("small-sizes-x-forms", [Seg(n, f, *_cycle(i)) for i, (n, f) in enumerate(itertools.product(SMALL_N, FORMS))],
                 DEFAULT_BETAS, 5.0, 1.0)]
    for fi, f in enumerate(FORMS):
        out.append(Table("chunk-sizes-%s" % FORM_NAMES[fi], [Seg(n, f, *_cycle(i + fi)) for i, n in enumerate(MID_N)], DEFAULT_BETAS,
                         5.0, 1.0 if fi % 2 else 0.5))
    for fi in (0, 1, 5, 9, 10):
        out.append(Table("multi-chunk-%s" % FORM_NAMES[fi], [Seg(n, FORMS[fi], *_cycle(i + fi)) for i, n in enumerate(LARGE_N)],
                         DEFAULT_BETAS, 5.0, 1.0))
    return out


def _small_segs(k):
    return [Seg(1 + i % 13, FORMS[i % 13], *_cycle(i)) for i in range(k)]


def shape_tables():
    """nseg / nchunk of 1 / 1; 255, 256, 257, 300 one-chunk segments of 1 .. 13 elements; 300 of them and two multi-chunk segments
    (nchunk 305 > nseg 302 > 256); 513 chunks (510 + a 3-chunk segment)"""
    out = [Table("shape-1-1", [Seg(5, ALIGNED, 1e-3, 0.01, 2)], DEFAULT_BETAS, 1.0, 1.0)]
    for k in (255, 256, 257, 300):
        out.append(Table("shape-%d" % k, _small_segs(k), DEFAULT_BETAS, 5.0, 1.0))
    out.append(Table("shape-300+2", _small_segs(300) + [Seg(CHUNK + 4, ALIGNED, 1e-3, 0.01, 9), Seg(2 * CHUNK + 3, FORMS[4], 1e-4, 0.0, 0)],
                     DEFAULT_BETAS, 5.0, 1.0))
    out.append(Table("shape-513-chunks", _small_segs(510) + [Seg(2 * CHUNK + 3, ALIGNED, 1e-3, 0.01, 1)], DEFAULT_BETAS, 5.0, 0.25))
    return out


HYPER_TABLES, SIZE_TABLES, SHAPE_TABLES = hyper_tables(), size_tables(), shape_tables()
ADAM_TABLES = HYPER_TABLES + SIZE_TABLES + SHAPE_TABLES
TABLES = {t.name: t for t in ADAM_TABLES}
assert len(TABLES) == len(ADAM_TABLES)


# ------------------------------------------------------------------------------------------------ tables: the values
Values = collections.namedtuple("Values", "p g m v lr wd t off")      # flat float32, segment after segment; off[i] : off[i + 1]


def per_element(segs):
    ns = np.array([s.n for s in segs], dtype=np.int64)
    return (np.repeat(np.array([s.lr for s in segs], dtype=np.float32), ns), np.repeat(np.array([s.wd for s in segs], dtype=np.float32), ns),
            np.repeat(np.array([s.t for s in segs], dtype=np.float32), ns), np.concatenate(([0], np.cumsum(ns))))


def values(table):
    """Seeded operands of one table.  Gradients of scales 1e-3, 1 and 30 mixed element by element, one in ten exactly zero; fresh
    (zero) moments where the step count is 0, else moments an Adam run could have left: v >= 0 at the scales of the gradients
    squared, |m| <= sqrt(v), so that (ge - m) cancels against a large old m where the new gradient is small."""
    rng = np.random.default_rng(zlib.crc32(table.name.encode()))
    lr, wd, t, off = per_element(table.segs)
    n = int(off[-1])
    scales = np.array([1e-3, 1.0, 30.0])
    g = rng.standard_normal(n) * scales[rng.integers(0, 3, n)]
    g[rng.random(n) < 0.1] = 0.0
    p = rng.standard_normal(n)
    v = (np.abs(rng.standard_normal(n)) * scales[rng.integers(0, 3, n)]) ** 2
    m = np.sqrt(v) * rng.uniform(-1.0, 1.0, n)
    m[t == 0] = 0.0
    v[t == 0] = 0.0
    return Values(p.astype(np.float32), g.astype(np.float32), m.astype(np.float32), v.astype(np.float32), lr, wd, t, off)


def reference(table, vals, coef):
    return step_fp64(vals.p, vals.g, vals.m, vals.v, vals.t, vals.lr, vals.wd, table.betas[0], table.betas[1], EPS, coef)
