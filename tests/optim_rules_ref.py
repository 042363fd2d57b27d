"""Reference, error bounds and case lists of tests/test_gpu_optim_rules.py: the SGD-with-momentum and Adamax steps of
csrc/optim.hip (optim_sgd_kernel behind cvc_sgd_clip_step, optim_adamax_kernel behind cvc_adamax_clip_step, driven by
cvc.optim.ClipSGD / ClipAdamax).  The method is tests/optim_ref.py's, whose Seg / layout / values / ratio / norm machinery is
imported, not copied; nothing here needs a GPU.  tests/test_optim_rules_ref_cpu.py proves the references against torch.optim.SGD and
torch.optim.Adamax on float64 CPU tensors, shows that a float32 restatement of each kernel's `upd` stays inside the bounds, and that
wrong kernels leave them.

sgd_step_fp64 / adamax_step_fp64 are ONE step in numpy float64 (torch.optim.SGD with dampening 0 and no Nesterov;
torch.optim.Adamax); the scalar hyper-parameters are rounded to float32 first, the clip coefficient is an INPUT (the GPU file feeds
the device's own).  Next to every value stands a first-order bound of a float32 evaluation's error, built as in optim_ref: every
float32 rounding adds u = 2^-24 times the magnitude of its result, carried through the later operations with their derivatives:
    SGD      ge = g coef + wd p              u (|g coef| + |wd p| + |sum|)
             buf' = mom buf + ge             u |mom buf| + e(ge) + u |buf'|: cancellation of the new gradient against the old buffer
             p' = p - lr buf'                |lr| e(buf') + u |lr buf'| + u |p'|
    Adamax   m' = m + (ge - m) (1 - beta1)   as Adam's
             u' = max(beta2 u, |ge| + eps)   the larger of the two sides' errors (|max(a', b') - max(a, b)| <= max(|a' - a|, |b' - b|))
             lr / (1 - beta1^t)              pow within 2 ulp, the subtraction, the division: the factor 1 / bc at small t
             p' = p - clr m' / u'            e(m') / u' + |m'| e(u') / u'^2, times clr; u' >= eps > 0
and is multiplied by ONE constant K per rule.  K is measured, never from a kernel's output: sgd_step_f32 / adamax_step_f32 restate
`upd` in numpy float32, operation by operation in the kernels' order, and K = 4 x the worst |f32 - fp64| / bound over every table
of the rule.  The 4 is the project's margin for what the device may do differently from numpy: FMAs (one rounding where numpy has
two) and a powf a couple of ulp off.
    measured worst ratio, SGD:    0.9993 (p 0.9993, buffer 0.9747)  ->  K_SGD = 4.0
    measured worst ratio, Adamax: 0.9993 (p 0.9981, exp_avg 0.9643, exp_inf 0.9993)  ->  K_ADAMAX = 4.0
(a rounding next to a power of two fills its u |x|)
(tests/test_optim_rules_ref_cpu.py prints the ratios and asserts that each K is 4 x its ratio, to the digits given.)  The written
gradient g coef is a single rounding: its bound is u |g coef| with no constant."""
import collections
import itertools

import numpy as np

import optim_ref as OR
from optim_ref import ALIGNED, BETAS, CHUNK, EPS, FORM_NAMES, FORMS, LARGE_N, LRS, MID_N, SMALL_N, U, WDS, Seg, Step, f32

K_SGD = 4.0
K_ADAMAX = 4.0
WORST_RATIO = {"sgd": 0.9993, "adamax": 0.9993}    # of the float32 restatements against the bounds (test_optim_rules_ref_cpu.py)
K = {"sgd": K_SGD, "adamax": K_ADAMAX}
MOMENTA = (0.9, 0.5, 0.0)
T_BEFORE = (0, 1, 9, 99999)         # Adamax: the step count before the step.  SGD keeps none: 0 = a fresh (zero) buffer


# ------------------------------------------------------------------------------------------------ the references
def _ge(p, g, wd, coef):
    gc = g * coef;                          e_gc = U * np.abs(gc)
    wdp = wd * p
    ge = gc + wdp
    e_ge = np.where(wd != 0, e_gc + U * np.abs(wdp) + U * np.abs(ge), e_gc)
    return gc, e_gc, np.where(wd != 0, ge, gc), e_ge


def sgd_step_fp64(p, g, buf, lr, wd, mom, coef):
    """One torch.optim.SGD(momentum=mom) step in float64 -> optim_ref.Step(p, buffer, 0, written gradient, and the bound of each
    WITHOUT the constant K).  mom == 0: no buffer (the returned one is `buf` unchanged, bound 0).  lr and wd may be per-element."""
    p, g, buf = (np.asarray(x, dtype=np.float64) for x in (p, g, buf))
    lr, wd, mom, coef = f32(lr), f32(wd), float(f32(mom)), float(coef)
    with np.errstate(all="ignore"):
        gc, e_gc, ge, e_ge = _ge(p, g, wd, coef)
        if mom != 0:
            mb = mom * buf;                 e_mb = U * np.abs(mb)
            b1 = mb + ge;                   e_b = e_mb + e_ge + U * np.abs(b1)
            d, e_d = b1, e_b
        else:
            b1, e_b = buf, np.zeros_like(buf)
            d, e_d = ge, e_ge
        up = lr * d;                        e_up = np.abs(lr) * e_d + U * np.abs(up)
        p1 = p - up;                        e_p = e_up + U * np.abs(p1)
    z = np.zeros_like(p)
    return Step(p1, b1, z, gc, e_p, e_b, z, e_gc)


def adamax_step_fp64(p, g, m, u, t_before, lr, wd, beta1, beta2, eps, coef):
    """One torch.optim.Adamax step in float64 -> optim_ref.Step(p, exp_avg, exp_inf, written gradient, and the bound of each WITHOUT
    the constant K).  t_before, lr and wd may be per-element arrays."""
    p, g, m, u = (np.asarray(x, dtype=np.float64) for x in (p, g, m, u))
    lr, wd, b1, b2, eps, coef = f32(lr), f32(wd), float(f32(beta1)), float(f32(beta2)), float(f32(eps)), float(coef)
    t = np.asarray(t_before, dtype=np.float64) + 1.0
    with np.errstate(all="ignore"):
        gc, e_gc, ge, e_ge = _ge(p, g, wd, coef)
        d = ge - m;                         e_d = e_ge + U * np.abs(d)
        dm = d * (1.0 - b1);                e_dm = e_d * (1.0 - b1) + U * np.abs(dm)
        m1 = m + dm;                        e_m = e_dm + U * np.abs(m1)
        a = b2 * u;                         e_a = U * np.abs(a)
        b = np.abs(ge) + eps;               e_b = e_ge + U * np.abs(b)
        u1 = np.maximum(a, b);              e_u = np.maximum(e_a, e_b)               # (np.maximum hands a NaN on, as torch.maximum)
        pw = np.power(b1, t)
        bc = 1.0 - pw;                      e_bc = 2 * U * pw + U * bc
        clr = lr / bc;                      e_clr = np.abs(lr) * e_bc / (bc * bc) + U * np.abs(clr)
        q = m1 / u1;                        e_q = e_m / u1 + np.abs(m1) * e_u / (u1 * u1) + U * np.abs(q)
        up = clr * q;                       e_up = e_clr * np.abs(q) + np.abs(clr) * e_q + U * np.abs(up)
        p1 = p - up;                        e_p = e_up + U * np.abs(p1)
    return Step(p1, m1, u1, gc, e_p, e_m, e_u, e_gc)


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in float32
SGD_VARIANTS = ("dampening", "nesterov", "wd_unclipped", "buf_not_updated")                           # wrong kernels
ADAMAX_VARIANTS = ("t_minus_1", "no_bias_correction", "eps_outside_max", "u_from_unclipped", "u_decayed_after_max")


def _ge32(p, g, wd, coef, unclipped=False):
    gc = g * coef
    if unclipped:
        return gc, np.where(wd != 0, (g + wd * p) * coef, gc)
    return gc, np.where(wd != 0, gc + wd * p, gc)


def sgd_step_f32(p, g, buf, lr, wd, mom, coef, variant=None):
    """`upd` of optim_sgd_kernel in numpy float32, one rounding per operation, in the kernel's order -> (p, buffer, written gradient).
    variant: one of SGD_VARIANTS, a subtly wrong kernel."""
    F = np.float32
    p, g, buf = (np.asarray(x, dtype=F) for x in (p, g, buf))
    lr, wd, mom, coef, one = np.asarray(lr, dtype=F), np.asarray(wd, dtype=F), F(mom), F(coef), F(1)
    with np.errstate(all="ignore"):
        gc, ge = _ge32(p, g, wd, coef, variant == "wd_unclipped")
        if mom == 0:
            return p - lr * ge, buf, gc
        b1 = mom * buf + ((one - mom) * ge if variant == "dampening" else ge)
        d = ge + mom * b1 if variant == "nesterov" else b1
        p1 = p - lr * d
    return p1, (buf if variant == "buf_not_updated" else b1), gc


def adamax_step_f32(p, g, m, u, t_before, lr, wd, beta1, beta2, eps, coef, variant=None):
    """`upd` of optim_adamax_kernel in numpy float32, one rounding per operation, in the kernel's order -> (p, exp_avg, exp_inf,
    written gradient).  variant: one of ADAMAX_VARIANTS."""
    F = np.float32
    p, g, m, u = (np.asarray(x, dtype=F) for x in (p, g, m, u))
    lr, wd = np.asarray(lr, dtype=F), np.asarray(wd, dtype=F)
    b1, b2, eps, coef, one = F(beta1), F(beta2), F(eps), F(coef), F(1)
    t = (np.asarray(t_before, dtype=np.float64) + 1.0).astype(F)         # the step count after the finalize launch's += 1
    with np.errstate(all="ignore"):
        tp = t - one if variant == "t_minus_1" else t
        bc = np.ones_like(tp) if variant == "no_bias_correction" else one - np.power(b1, tp).astype(F)
        clr = lr / bc
        gc, ge = _ge32(p, g, wd, coef)
        m1 = m + (ge - m) * (one - b1)
        gu = _ge32(p, g, wd, one)[1] if variant == "u_from_unclipped" else ge
        if variant == "eps_outside_max":
            u1 = np.maximum(b2 * u, np.abs(gu)) + eps
        elif variant == "u_decayed_after_max":
            u1 = b2 * np.maximum(u, np.abs(gu) + eps)
        else:
            u1 = np.maximum(b2 * u, np.abs(gu) + eps)
        p1 = p - clr * (m1 / u1)
    return p1, m1, u1, gc


# ------------------------------------------------------------------------------------------------ tables: the cases
# rule: "sgd" / "adamax"; segs: optim_ref.Seg (offs: element offsets of (p, g, m, v) in their slots -- SGD has no v, and no m at
# momentum 0); betas: Adamax's; mom: SGD's
Table = collections.namedtuple("Table", "name rule segs betas mom max_norm inv")


def forms_of(rule, mom=0.9):
    """the alignment forms of optim_ref.FORMS that differ in an operand the rule has -> [(form, its name)]"""
    nop = 4 if rule == "adamax" else (3 if mom != 0 else 2)
    return [(f, FORM_NAMES[i]) for i, f in enumerate(FORMS) if not any(f[nop:])]


def _cycle(i):
    """the lr / weight decay / step count of the i-th segment of a size or shape table: every value of each list, out of phase"""
    return LRS[i % 3], WDS[(i // 3) % 2], T_BEFORE[(i + i // 6) % 4]


def _clip(i):
    """the clip active (max_norm 5), off (0), not reached (1e9); gradients as sums over 4 ranks (inv 0.25) on every other table"""
    return (5.0, 0.0, 1e9)[i % 3], (1.0, 0.25)[i % 2]


def hyper_tables(rule):
    """SGD: momentum x weight decay; Adamax: betas x weight decay.  Inside each table every t_before x every lr as segments of the
    small sizes, in the rule's alignment forms; the clip's three states and both inv go round the tables."""
    out = []
    for hi, h in enumerate(MOMENTA if rule == "sgd" else BETAS):
        forms = forms_of(rule, h if rule == "sgd" else 0.9)
        for wi, wd in enumerate(WDS):
            segs = [Seg(SMALL_N[(i + hi) % 13], forms[(i + 2 * hi + wi) % len(forms)][0], lr, wd, t)
                    for i, (t, lr) in enumerate(itertools.product(T_BEFORE, LRS))]
            if rule == "sgd":
                out.append(Table("sgd-hyper-mom%g-wd%g" % (h, wd), rule, segs, None, h, *_clip(hi + wi)))
            else:
                out.append(Table("adamax-hyper-b%g-%g-wd%g" % (h + (wd,)), rule, segs, h, None, *_clip(hi + wi)))
    return out


def size_tables(rule):
    """every size x every alignment form of the rule, laid out as optim_ref.size_tables: the small sizes in one table, CHUNK - 1 ..
    CHUNK + 4 one table per form, the two multi-chunk sizes aligned and with every operand alone off by 1, 2 or 3 (the scalar form
    does not read the offset: i = start + thread, stride 256).  SGD at momentum 0.9, and its buffer-less form (momentum 0: p and g
    only) over the small sizes, the chunk sizes and the multi-chunk sizes again."""
    out = []
    for mom in ((0.9, 0.0) if rule == "sgd" else (None,)):
        forms = forms_of(rule, 0.9 if mom is None else mom)
        tag = rule + ("-mom0" if mom == 0 else "")
        mk = lambda name, segs, mn, inv: Table("%s-%s" % (tag, name), rule, segs, OR.DEFAULT_BETAS if rule == "adamax" else None, mom, mn, inv)
        out.append(mk("small-sizes-x-forms", [Seg(n, f, *_cycle(i)) for i, (n, (f, _)) in enumerate(itertools.product(SMALL_N, forms))],
                      5.0, 1.0))
        for fi, (f, fname) in enumerate(forms):
            out.append(mk("chunk-sizes-%s" % fname, [Seg(n, f, *_cycle(i + fi)) for i, n in enumerate(MID_N)], 5.0, 1.0 if fi % 2 else 0.5))
        # (forms: aligned, then operand j off by 1, 2, 3 at 1 + 3 j ..: aligned, p+1, g+2, m+3, v+1 as far as the rule has them)
        one_each = [forms[0]] + [forms[1 + 3 * j + j % 3] for j in range(len(forms) // 3)]
        for fi, (f, fname) in enumerate(one_each):
            out.append(mk("multi-chunk-%s" % fname, [Seg(n, f, *_cycle(i + fi)) for i, n in enumerate(LARGE_N)], 5.0, 1.0))
    return out


def shape_tables(rule):
    """nseg = nchunk = 1, 256, 257, 300: one-chunk segments of 1 .. 13 elements in the rule's forms"""
    forms = forms_of(rule)
    mk = lambda name, segs, mn, inv: Table("%s-%s" % (rule, name), rule, segs, OR.DEFAULT_BETAS if rule == "adamax" else None,
                                           0.9 if rule == "sgd" else None, mn, inv)
    out = [mk("shape-1", [Seg(5, ALIGNED, 1e-3, 0.01, 1)], 1.0, 1.0)]
    for k in (256, 257, 300):
        out.append(mk("shape-%d" % k, [Seg(1 + i % 13, forms[i % len(forms)][0], *_cycle(i)) for i in range(k)], 5.0, 0.25 if k == 300 else 1.0))
    return out


HYPER_TABLES = {r: hyper_tables(r) for r in ("sgd", "adamax")}
SIZE_TABLES = {r: size_tables(r) for r in ("sgd", "adamax")}
SHAPE_TABLES = {r: shape_tables(r) for r in ("sgd", "adamax")}
RULE_TABLES = {r: HYPER_TABLES[r] + SIZE_TABLES[r] + SHAPE_TABLES[r] for r in ("sgd", "adamax")}
ALL_TABLES = RULE_TABLES["sgd"] + RULE_TABLES["adamax"]
TABLES = {t.name: t for t in ALL_TABLES}
assert len(TABLES) == len(ALL_TABLES)


# ------------------------------------------------------------------------------------------------ tables: the values
def values(table):
    """optim_ref.values' seeded operands (gradients of scales 1e-3, 1 and 30, one in ten zero; a fresh state where t is 0), with the
    second state array at the scale of the rule: Adamax's exp_inf is a running max of |g|, so u = sqrt(v) >= |m|; SGD has none, and
    at momentum 0 no buffer either"""
    v = OR.values(table)
    if table.rule == "adamax":
        return v._replace(v=np.sqrt(v.v))
    return v._replace(v=np.zeros_like(v.v), m=v.m if table.mom != 0 else np.zeros_like(v.m))


def reference(table, vals, coef):
    if table.rule == "sgd":
        return sgd_step_fp64(vals.p, vals.g, vals.m, vals.lr, vals.wd, table.mom, coef)
    return adamax_step_fp64(vals.p, vals.g, vals.m, vals.v, vals.t, vals.lr, vals.wd, table.betas[0], table.betas[1], EPS, coef)


def restated(table, vals, coef, variant=None):
    """the float32 restatement of the table's rule -> (p, m, v, written gradient); SGD's v is its (unused) input"""
    if table.rule == "sgd":
        p, b, g = sgd_step_f32(vals.p, vals.g, vals.m, vals.lr, vals.wd, table.mom, coef, variant)
        return p, b, vals.v, g
    return adamax_step_f32(vals.p, vals.g, vals.m, vals.v, vals.t, vals.lr, vals.wd, table.betas[0], table.betas[1], EPS, coef, variant)
