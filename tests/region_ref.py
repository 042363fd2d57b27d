"""References, float32 restatements, error bounds and case tables of tests/test_gpu_region_kernels.py: the small kernels around the
region features and the grounding losses,
    csrc/encoder_ops.hip   cvc_class_softmax_fwd, cvc_layernorm_cat_fwd, cvc_frame_embed_fwd
    csrc/label_glue.hip    cvc_attn_nll_fwd, cvc_attn_nll_bwd
    csrc/attn_bwd.hip      cvc_grounder_fwd (the dot form of attn_scores.h), cvc_grounder_bwd (weighted_rows_kernel)
    csrc/vocab.hip         cvc_embed_relu_fwd
Nothing here needs a GPU.  tests/test_region_ref_cpu.py proves every *_fp64 against the torch formulation in float64, shows that
every *_f32 (the kernel's arithmetic in numpy float32, one rounding per operation, in the kernel's order) stays within 1.0 of its
bound WITHOUT the constant K on every case of every table, and that every wrong restatement (`variant`) leaves K x bound somewhere.

Every *_fp64 returns its values in float64 next to a first-order bound of the float32 evaluation's error: each rounding contributes
u = 2^-24 times the magnitude of its result (2 u for expf, logf and rsqrtf, which are within one ulp but not correctly rounded), and
a contribution is carried through the later operations with those operations' derivatives.  The GPU file allows K = 4 x the bound
(optim_ref.K), for what the device may do differently from numpy: fused multiply-adds, another library's expf.

All sums here have ONE shape: a thread adds every width-th element one after the other (`trips` of them), and the `width` partial
sums are added as a balanced tree of neighbours.  wave_sum's DPP network is that tree over 64 lanes; block_sum4 / block_sum_all
continue it over 4 waves with (r0 + r1) + (r2 + r3); weighted_rows_kernel is the same with width 4 (its four waves).  The longest
chain of roundings from a term to the total is depth(n, width); a sum of terms t_i is within u depth sum |t_i| (first order).
Where fewer than `width` terms exist the tree adds exact zeros, which depth() does not count."""
import collections
import itertools
import math
import zlib

import numpy as np

from optim_ref import BAND, K, SENTINEL, U, f32, ratio                      # noqa: F401  (re-exported to the two test files)

F = np.float32
MIN_VALUE = -1e8                                 # CVC_MIN_VALUE
TINY = 2.0 ** -126                               # below the normal range a result may be flushed: an absolute floor of every bound
E_TOOBIG, E_BADARG = -2, -1


def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ the one summation shape
def tree32(v):
    """balanced tree of neighbours over the last axis (a power of two), float32"""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def strided_sum32(x, width, trips=None):
    """thread k of `width` adds x[k], x[k + width], ... in float32; the partial sums are added by tree32.  trips: stop after that
    many (a wrong kernel)"""
    x = np.asarray(x, dtype=F)
    n = x.shape[-1]
    t = -(-n // width)
    pad = np.zeros(x.shape[:-1] + (t * width,), dtype=F)
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (t, width))
    acc = np.zeros(x.shape[:-1] + (width,), dtype=F)
    for k in range(t if trips is None else min(t, trips)):
        acc = acc + pad[..., k, :]
    return tree32(acc)


def depth(n, width):
    """roundings on the longest path of strided_sum32: trips - 1 sequential adds (the first adds to 0), then the tree's levels"""
    return (-(-n // width) - 1) + int(math.ceil(math.log2(min(n, width)))) if n > 1 else 0


def exp32(x):
    """float32 exp, rounded once from float64 (numpy's own float32 exp is a vector routine of a few ulp)"""
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, dtype=np.float64)).astype(F)


# ================================================================================================ class_softmax
# (B, N, C, ld, bias, pad, out_rows, family).  The full cross of bias / pad / out_rows at two shapes, each toggled once elsewhere.
# family "steep": logits that grow by 0.5 per class on top of the noise, so that the row's maximum lies far beyond its first 64
# classes (a maximum taken there overflows expf) and most probabilities underflow.
SOFTMAX_SHAPES = ((1, 1, 1, 1), (2, 15, 7, 7), (3, 16, 64, 64), (2, 17, 65, 72), (1, 33, 100, 100), (2, 48, 432, 440), (1, 5, 1023, 1023))
SoftmaxCase = collections.namedtuple("SoftmaxCase", "B N C ld bias pad rows family")


def _softmax_cases():
    out = []
    for shape in ((2, 15, 7, 7), (2, 17, 65, 72)):
        out += [SoftmaxCase(*shape, *flags, "normal") for flags in itertools.product((True, False), repeat=3)]
    out += [SoftmaxCase(1, 1, 1, 1, True, True, True, "normal"), SoftmaxCase(1, 1, 1, 1, False, False, False, "normal"),
            SoftmaxCase(3, 16, 64, 64, True, True, True, "normal"), SoftmaxCase(3, 16, 64, 64, False, True, True, "normal"),
            SoftmaxCase(1, 33, 100, 100, True, False, True, "normal"), SoftmaxCase(1, 33, 100, 100, True, True, False, "steep"),
            SoftmaxCase(2, 48, 432, 440, True, True, True, "normal"), SoftmaxCase(2, 48, 432, 440, True, False, False, "steep"),
            SoftmaxCase(1, 5, 1023, 1023, True, True, True, "normal"), SoftmaxCase(1, 5, 1023, 1023, False, False, True, "steep")]
    return out


SOFTMAX_CASES = _softmax_cases()


def pad_mask(B, N, key):
    """clip 0 fully padded and clip 1 free of padding when there are two clips; a random third elsewhere"""
    pad = rng_of("pad", key).random((B, N)) < 1 / 3
    if B >= 2:
        pad[0], pad[1] = True, False
    return pad


def softmax_values(case):
    """-> (logits [B N, ld] float32, bias [C] or None, pad [B N] bool or None).  Columns C .. ld - 1 and the logits of padded regions
    are NaN (declared unread).  One logit of every third row is -inf where C >= 2."""
    B, N, C, ld = case[:4]
    rng = rng_of("softmax", tuple(case))
    x = np.full((B * N, ld), np.nan, dtype=F)
    x[:, :C] = rng.standard_normal((B * N, C)) * 3.0
    if case.family == "steep":
        x[:, :C] += 0.5 * np.arange(C, dtype=F)
    if C >= 2:
        rows = np.arange(0, B * N, 3)
        x[rows, (rows * 7) % C] = -np.inf
    bias = (rng.standard_normal(C) * 2.0).astype(F) if case.bias else None
    pad = pad_mask(B, N, tuple(case)).reshape(-1) if case.pad else None
    if pad is not None:
        x[pad] = np.nan
    return x, bias, pad


def softmax_fp64(x, bias, pad, C):
    """softmax over the C classes of (x + bias), padded rows filled with -1e8 -> (p [rows, C], bound).
        v = x + b             u |v| (none without a bias: x + 0 is exact)
        d = v - m             m is one of the v: its rounding too, and u |d| for the subtraction
        e = expf(d)           relative: the absolute error of d, + 2 u
        s = sum e             the errors of the e, + u depth(C, 64) s (all terms >= 0)
        p = e (1 / s)         + 2 u
    a padded row is exact: every e is 1, s = C, p = float32(1) / float32(C) (the bound keeps the u of that division)"""
    x = np.asarray(x, dtype=np.float64)[:, :C]
    with np.errstate(all="ignore"):
        v = x + (0.0 if bias is None else np.asarray(bias, dtype=np.float64))
        if pad is not None:
            v = np.where(np.asarray(pad, dtype=bool)[:, None], MIN_VALUE, v)
        m = v.max(axis=1, keepdims=True)
        d = v - m
        e = np.exp(d)
        s = e.sum(axis=1, keepdims=True)
        p = e / s
        ev = U * np.abs(v) if bias is not None else np.zeros_like(v)
        ed = ev + (U * np.abs(m) if bias is not None else 0.0) + U * np.abs(d)
        rel_e = np.where(e > 0, ed + 2 * U, 0.0)                        # (-inf: exactly 0, no error)
        rel_s = (e * rel_e).sum(axis=1, keepdims=True) / s + U * depth(C, 64)
        bound = p * (rel_e + rel_s + 2 * U) + np.where(p > 0, TINY, 0.0)
        if pad is not None:
            bound = np.where(np.asarray(pad, dtype=bool)[:, None], U * p, bound)
    return p, bound


SOFTMAX_MUTANTS = ("bias_dropped_from_64", "max_of_first_trip", "sum_of_first_trip", "pad_ignored")


def softmax_f32(x, bias, pad, C, variant=None):
    """class_softmax_kernel's row in float32: lane-strided maximum, expf, lane-strided sum + wave tree, one reciprocal, one product"""
    x = np.asarray(x, dtype=F)[:, :C]
    with np.errstate(all="ignore"):
        b = np.zeros(C, dtype=F) if bias is None else np.asarray(bias, dtype=F).copy()
        if variant == "bias_dropped_from_64":
            b[64:] = 0
        v = x + b
        if pad is not None and variant != "pad_ignored":
            v = np.where(np.asarray(pad, dtype=bool)[:, None], F(MIN_VALUE), v)
        m = (v[:, :64] if variant == "max_of_first_trip" else v).max(axis=1, keepdims=True)
        e = exp32(v - m)
        s = strided_sum32(e, 64, 1 if variant == "sum_of_first_trip" else None)[:, None]
        return e * (F(1) / s)


# ================================================================================================ layernorm_cat
LN_WIDTHS = ((1,), (7,), (255, 256, 257), (4, 3072), (2048, 300, 432))
LN_ROWS = (1, 5)
LN_EPS = (1e-5, 1e-3)
LN_FAMILIES = ("scaled", "offset")
LnCase = collections.namedtuple("LnCase", "widths rows eps family")
LN_CASES = [LnCase(*c) for c in itertools.product(LN_WIDTHS, LN_ROWS, LN_EPS, LN_FAMILIES)]
LN_SCALES, LN_OFFSETS = (0.01, 1.0, 30.0), (-2.0, 0.5, 3.0)
LN_BIG_OFFSET = 1000.0              # family "offset": mean = 1000 std.  u |mean| rstd depth is 5e-4 there: still first order


def ln_values(case):
    """one [rows, width] float32 array per segment.  "scaled": segment s has std LN_SCALES[s] around LN_OFFSETS[s]; "offset": std 1
    around +-1000"""
    rng = rng_of("ln", tuple(case))
    out = []
    for s, d in enumerate(case.widths):
        if case.family == "scaled":
            out.append((rng.standard_normal((case.rows, d)) * LN_SCALES[s] + LN_OFFSETS[s]).astype(F))
        else:
            out.append((rng.standard_normal((case.rows, d)) + LN_BIG_OFFSET * (-1) ** s).astype(F))
    return out


def ln_fp64(xs, eps):
    """F.layer_norm(x_s, [d_s], eps=eps) of every segment, side by side -> (out [rows, total], bound).
        mean = block_sum(x) / d            u depth(d, 256) sum |x| / d + u |mean|
        c = x - mean                       the mean's error, + u |c|
        var = block_sum(c c) / d + eps     the mean's error enters at second order only (sum c = 0); 2 |c| u |c| from the c, u per
                                           product, u depth for the sum, u each for the division and the sum with eps
        rstd = rsqrtf(var)                 half the relative error of var, + 2 u
        out = c rstd                       (error of c) rstd + |c| (error of rstd) + u |out|
    the first term is u depth |mean| rstd where the mean is large against the spread"""
    eps = float(F(eps))
    outs, bounds = [], []
    for x in xs:
        x = np.asarray(x, dtype=np.float64)
        d = x.shape[1]
        dep = depth(d, 256)
        mean = x.mean(axis=1, keepdims=True)
        e_mean = U * dep * np.abs(x).sum(axis=1, keepdims=True) / d + U * np.abs(mean)
        c = x - mean
        e_c = e_mean + U * np.abs(c)
        sq = (c * c).sum(axis=1, keepdims=True)
        e_sq = (2 * np.abs(c) * U * np.abs(c)).sum(axis=1, keepdims=True) + d * e_mean ** 2 + U * (dep + 1) * sq
        var = sq / d + eps
        e_var = e_sq / d + U * sq / d + U * var
        rstd = 1.0 / np.sqrt(var)
        e_rstd = rstd * (e_var / (2 * var) + 2 * U)
        out = c * rstd
        outs.append(out)
        bounds.append(e_c * rstd + np.abs(c) * e_rstd + U * np.abs(out))
    return np.concatenate(outs, axis=1), np.concatenate(bounds, axis=1)


LN_MUTANTS = ("unbiased_variance", "eps_outside_sqrt", "mean_shared", "sum_of_first_trip")


def ln_f32(xs, eps, variant=None):
    eps = F(eps)
    outs = []
    first_mean = None
    for x in xs:
        x = np.asarray(x, dtype=F)
        d = x.shape[1]
        trips = 1 if variant == "sum_of_first_trip" else None
        mean = (strided_sum32(x, 256, trips) / F(d))[:, None]
        if variant == "mean_shared":
            first_mean = mean if first_mean is None else first_mean
            mean = first_mean
        c = x - mean
        sq = strided_sum32(c * c, 256, trips)[:, None]
        with np.errstate(all="ignore"):
            if variant == "unbiased_variance":
                var = sq / F(max(d - 1, 1)) + eps
            else:
                var = sq / F(d) + eps
            if variant == "eps_outside_sqrt":
                rstd = (1.0 / (np.sqrt((sq / F(d)).astype(np.float64)) + float(eps))).astype(F)
            else:
                rstd = (1.0 / np.sqrt(var.astype(np.float64))).astype(F)
        outs.append((x - mean) * rstd)
    return np.concatenate(outs, axis=1)


# ================================================================================================ frame_embed
FE_CASES = ((1, 4, 4), (3, 8, 4), (5, 4, 12), (33, 64, 36), (257, 128, 128))        # (rows, c0, c1)


def fe_values(case):
    """-> y0 [rows, c0], b0, y1 [rows, c1], b1, scale [c0 + c1], shift.  scale runs through (negative, zero, positive) channel by
    channel, starting so that both sides of c0 see all three; shift and y + b take both signs"""
    rows, c0, c1 = case
    rng = rng_of("fe", tuple(case))
    C = c0 + c1
    y0, y1 = rng.standard_normal((rows, c0)).astype(F), rng.standard_normal((rows, c1)).astype(F)
    b0, b1 = (rng.standard_normal(c0) * 0.5).astype(F), (rng.standard_normal(c1) * 0.5).astype(F)
    sign = np.array([-1.0, 0.0, 1.0])[(np.arange(C) + (c0 % 3)) % 3]
    scale = (sign * rng.uniform(0.5, 2.0, C)).astype(F)
    shift = (rng.standard_normal(C) * 0.7).astype(F)
    return y0, b0, y1, b1, scale, shift


def fe_fp64(y0, b0, y1, b1, scale, shift):
    """relu(bn(cat(relu(y0 + b0), relu(y1 + b1)))) with the folded scale / shift -> (out, z = the value before the last ReLU, bound).
        t = max(y + b, 0)        u t (a rounded sum keeps its sign)
        z = t scale + shift      u |t scale| from t, u |t scale| for the product (absent under an FMA), u |z| <= u (|t scale| +
                                 |shift|) for the sum: ABSOLUTE, the sum cancels near zero
    -> u (3 |t scale| + |shift|), contracted or not.  The last ReLU is 1-Lipschitz."""
    y = np.concatenate([np.asarray(y0, np.float64) + np.asarray(b0, np.float64), np.asarray(y1, np.float64) + np.asarray(b1, np.float64)], axis=1)
    t = np.maximum(y, 0.0)
    ts = t * np.asarray(scale, np.float64)
    z = ts + np.asarray(shift, np.float64)
    return np.maximum(z, 0.0), z, U * (3 * np.abs(ts) + np.abs(np.asarray(shift, np.float64)))


FE_MUTANTS = ("inner_relu_dropped", "outer_relu_dropped", "scale_indexed_from_c0")


def fe_f32(y0, b0, y1, b1, scale, shift, variant=None):
    c0 = y0.shape[1]
    y = np.concatenate([np.asarray(y0, F) + np.asarray(b0, F), np.asarray(y1, F) + np.asarray(b1, F)], axis=1)
    t = y if variant == "inner_relu_dropped" else np.maximum(y, F(0))
    sc = np.asarray(scale, F)
    if variant == "scale_indexed_from_c0":
        sc = np.concatenate([sc[:c0], sc[:y.shape[1] - c0]])
    z = t * sc + np.asarray(shift, F)
    return z if variant == "outer_relu_dropped" else np.maximum(z, F(0))


# ================================================================================================ attn_nll
NLL_CASES = ((1, 1, 1), (2, 3, 7), (3, 1, 255), (2, 2, 256), (2, 3, 257), (1, 2, 1000))         # (B, T, N)


def nll_values(case, low=True):
    """-> (x [2, B, T, N] float32: the two score tensors, target [B, T, N] bool).  Scores of std 2 with a fifth of the slots at -1e8
    (masked proposals); targets 5 % dense.  With three or more rows: row 0 has no target, row 1 every proposal (and no -1e8 slot);
    the last row has one target on a -1e8 slot.  With two rows: row 0 has the target on a -1e8 slot, row 1 every proposal.
    low=False: no target lies on a -1e8 slot (that one label puts 1e8 / count into the loss, and 1e8 u into its bound: the same
    case without it holds the loss and every row_part to the bound of ordinary scores)."""
    B, T, N = case
    rng = rng_of("nll", tuple(case))
    x = (rng.standard_normal((2, B * T, N)) * 2.0).astype(F)
    masked = rng.random((B * T, N)) < 0.2
    tg = rng.random((B * T, N)) < 0.05
    rows = B * T
    if rows == 1:
        tg[0, 0], masked[0] = True, False
    else:
        full, lrow = (1, rows - 1) if rows >= 3 else (1, 0)
        if rows >= 3:
            tg[0] = False
        tg[full], masked[full] = True, False
        masked[lrow, N // 2], tg[lrow, N // 2] = True, True
        if N > 1:
            masked[lrow, 0] = False
    if not low:
        masked &= ~tg
    x[:, masked] = MIN_VALUE
    return x.reshape(2, B, T, N), tg.reshape(B, T, N)


Nll = collections.namedtuple("Nll", "loss count lse part cnt e_loss e_lse e_part")


def nll_fp64(x, target):
    """-sum(log_softmax(x, -1)[target]) / max(count, 1) of every tensor of x [nx, B, T, N] -> Nll, rows flattened.
        lse = m + logf(sum expf(x - m))     d = x - m: u |d| (m is one of the x); expf: + 2 u relative; the sum: u depth(N, 256) s;
                                            logf: the sum's relative error + 2 u |log s|; + u |lse|
        part = tx - c lse                   tx = the sum of the labelled x: u depth sum |x|; c (a count) is exact; c x the error of
                                            lse, u |c lse|, u |part|
        loss = -block_sum(part) / count     the parts' errors, u depth(rows, 256) sum |part|, both over count, + u |loss|"""
    x = np.asarray(x, dtype=np.float64)
    nx, N = x.shape[0], x.shape[-1]
    x = x.reshape(nx, -1, N)
    tg = np.asarray(target, dtype=bool).reshape(-1, N)
    rows = tg.shape[0]
    dep = depth(N, 256)
    with np.errstate(all="ignore"):
        m = x.max(axis=2, keepdims=True)
        d = x - m
        e = np.exp(d)
        s = e.sum(axis=2, keepdims=True)
        logs = np.log(s)
        lse = (m + logs)[..., 0]
        e_lse = ((e * (U * np.abs(d) + 2 * U)).sum(axis=2) / s[..., 0] + U * dep + 2 * U * np.abs(logs[..., 0]) + U * np.abs(lse))
        cnt = tg.sum(axis=1).astype(np.float64)
        tx = np.where(tg, x, 0.0).sum(axis=2)
        part = tx - cnt * lse
        e_part = U * dep * np.where(tg, np.abs(x), 0.0).sum(axis=2) + cnt * e_lse + U * np.abs(cnt * lse) + U * np.abs(part)
        count = max(cnt.sum(), 1.0)
        loss = -part.sum(axis=1) / count
        e_loss = (e_part.sum(axis=1) + U * depth(rows, 256) * np.abs(part).sum(axis=1)) / count + U * np.abs(loss)
    return Nll(loss, count, lse, part, cnt, e_loss, e_lse, e_part)


NLL_FWD_MUTANTS = ("count_per_row", "sum_of_first_trip", "max_not_added_back")


def nll_fwd_f32(x, target, variant=None):
    """attn_nll_rows_kernel + attn_nll_final_kernel -> (loss [nx], count, lse [nx, rows], part [nx, rows], cnt [rows])"""
    x = np.asarray(x, dtype=F)
    nx, N = x.shape[0], x.shape[-1]
    x = x.reshape(nx, -1, N)
    tg = np.asarray(target, dtype=bool).reshape(-1, N)
    trips = 1 if variant == "sum_of_first_trip" else None
    with np.errstate(all="ignore"):
        m = x.max(axis=2, keepdims=True)
        s = strided_sum32(exp32(x - m), 256, trips)
        tx = strided_sum32(np.where(tg, x, F(0)), 256, trips)
        c = strided_sum32(tg.astype(F), 256, trips)
        logs = np.log(s.astype(np.float64)).astype(F)
        lse = logs if variant == "max_not_added_back" else m[..., 0] + logs
        part = tx - c * lse
        count = np.maximum(strided_sum32(c, 256), F(1))
        if variant == "count_per_row":
            loss = -strided_sum32(part / np.maximum(c, F(1)), 256)
        else:
            loss = -strided_sum32(part, 256) / count
    return loss, count, lse, part, c


def nll_bwd_fp64(x, target, g, fwd=None):
    """d loss_w / d x scaled by g[w]: g / count (softmax(x) nt - target), nt = the row's labelled proposals -> (d [nx, rows, N],
    bound).  The kernel reads lse back from the forward's workspace:
        a = x - lse               the error of lse (nll_fp64), + u |a|
        p = expf(a)               relative: the error of a, + 2 u
        q = p nt - target         u |p nt|, u |q|
        d = (g / count) q         2 u more"""
    fwd = nll_fp64(x, target) if fwd is None else fwd
    x = np.asarray(x, dtype=np.float64)
    nx, N = x.shape[0], x.shape[-1]
    x = x.reshape(nx, -1, N)
    tg = np.asarray(target, dtype=bool).reshape(-1, N).astype(np.float64)
    g = np.asarray(g, dtype=np.float64).reshape(nx, 1, 1)
    with np.errstate(all="ignore"):
        a = x - fwd.lse[..., None]
        p = np.exp(a)
        nt = fwd.cnt[None, :, None]
        q = p * nt - tg
        d = g / fwd.count * q
        e_q = p * nt * (fwd.e_lse[..., None] + U * np.abs(a) + 2 * U) + U * p * nt + U * np.abs(q)
        bound = np.abs(g) / fwd.count * e_q + 2 * U * np.abs(d) + np.where(d != 0, TINY, 0.0)
    return d, bound


NLL_BWD_MUTANTS = ("nt_is_one", "first_trip_only", "count_ignored")


def nll_bwd_f32(x, target, g, variant=None):
    x = np.asarray(x, dtype=F)
    nx, N = x.shape[0], x.shape[-1]
    _loss, count, lse, _part, c = nll_fwd_f32(x, target)
    x = x.reshape(nx, -1, N)
    tg = np.asarray(target, dtype=bool).reshape(-1, N).astype(F)
    with np.errstate(all="ignore"):
        scale = np.asarray(g, dtype=F).reshape(nx, 1, 1) / (F(1) if variant == "count_ignored" else count)
        nt = F(1) if variant == "nt_is_one" else c[None, :, None]
        d = scale * (exp32(x - lse[..., None]) * nt - tg)
    if variant == "first_trip_only":
        d[..., 256:] = 0
    return d


# ================================================================================================ grounder
GR_CASES = ((1, 1, 1, 4), (2, 3, 7, 24), (2, 5, 17, 252), (1, 4, 64, 256), (2, 2, 65, 260), (1, 6, 130, 36))    # (B, T, N, G)
GR_OPTION_CASES = ((2, 3, 7, 24), (2, 2, 65, 260))           # bias and mask each present or null here; both present elsewhere


def gr_values(case):
    """-> xt [B, T, G], feats [B, N, G], bias [B, T, N], mask [B, T, N] bool (a quarter set), d [B, T, N] (the backward's operand)"""
    B, T, N, G = case
    rng = rng_of("gr", tuple(case))
    xt, feats = rng.standard_normal((B, T, G)).astype(F), rng.standard_normal((B, N, G)).astype(F)
    bias = rng.standard_normal((B, T, N)).astype(F)
    mask = rng.random((B, T, N)) < 0.25
    d = (rng.standard_normal((B, T, N)) * 10.0 ** rng.integers(-2, 2, (B, T, N))).astype(F)
    return xt, feats, bias, mask, d


def gr_lane_levels(G):
    return int(math.ceil(math.log2(min(-(-G // 4), 64)))) if G > 4 else 0


def gr_fwd_fp64(xt, feats, bias, mask):
    """einsum('btg,bng->btn') + bias, masked slots -1e8 -> (out, bound).  The dot form of attn_scores_kernel: lane l owns 4
    columns of every 256-column chunk and adds their 4 products and the running sum (4 adds per chunk, as written or as FMAs), then
    wave_sum: depth = 1 (the product) + 4 chunks + the tree's levels; u depth sum |x| |f|.  The bias is one more rounded sum."""
    xt, feats = np.asarray(xt, np.float64), np.asarray(feats, np.float64)
    G = xt.shape[-1]
    out = np.einsum("btg,bng->btn", xt, feats)
    mag = np.einsum("btg,bng->btn", np.abs(xt), np.abs(feats))
    bound = U * (1 + 4 * (-(-G // 256)) + gr_lane_levels(G)) * mag
    if bias is not None:
        out = out + np.asarray(bias, np.float64)
        bound = bound + U * np.abs(out)
    if mask is not None:
        m = np.asarray(mask, dtype=bool)
        out, bound = np.where(m, MIN_VALUE, out), np.where(m, 0.0, bound)
    return out, bound


GR_FWD_MUTANTS = ("second_chunk_dropped", "last_lane_dropped", "bias_dropped", "mask_ignored")


def gr_fwd_f32(xt, feats, bias, mask, variant=None):
    xt, feats = np.asarray(xt, F), np.asarray(feats, F)
    B, T, G = xt.shape
    N = feats.shape[1]
    nch = -(-G // 256)
    prod = np.zeros((B, T, N, nch * 256), dtype=F)
    prod[..., :G] = xt[:, :, None, :] * feats[:, None, :, :]
    prod = prod.reshape(B, T, N, nch, 64, 4)
    if variant == "second_chunk_dropped":
        prod[:, :, :, 1:] = 0
    if variant == "last_lane_dropped":                        # the lane that holds the last 4 columns
        last = (G - 4) // 4
        prod[:, :, :, last // 64, last % 64] = 0
    acc = np.zeros((B, T, N, 64), dtype=F)
    for j in range(nch):
        p = prod[:, :, :, j]
        acc = acc + (((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3])
    out = tree32(acc)
    if bias is not None and variant != "bias_dropped":
        out = out + np.asarray(bias, F)
    if mask is not None and variant != "mask_ignored":
        out = np.where(np.asarray(mask, dtype=bool), F(MIN_VALUE), out)
    return out


def gr_bwd_fp64(d, xt, feats):
    """d_xt = einsum('btn,bng->btg'), d_feats = einsum('btn,btg->bng') -> (d_xt, bound, d_feats, bound).  weighted_rows_kernel: wave
    w adds the rows q = w, w + 4, ... one after the other (a product and a sum each, or one FMA), thread 0's wave adds the four
    partial sums as (p0 + p1) + (p2 + p3): depth = 1 + depth(nq, 4), nq = N for d_xt and T for d_feats; u depth sum |d| |operand|"""
    d, xt, feats = np.asarray(d, np.float64), np.asarray(xt, np.float64), np.asarray(feats, np.float64)
    T, N = d.shape[1], d.shape[2]
    d_xt = np.einsum("btn,bng->btg", d, feats)
    d_f = np.einsum("btn,btg->bng", d, xt)
    e_xt = U * (1 + depth(N, 4)) * np.einsum("btn,bng->btg", np.abs(d), np.abs(feats))
    e_f = U * (1 + depth(T, 4)) * np.einsum("btn,btg->bng", np.abs(d), np.abs(xt))
    return d_xt, e_xt, d_f, e_f


GR_BWD_MUTANTS = ("tail_dropped", "fourth_wave_dropped", "d_transposed_strides")


def _split4(terms, variant):
    """terms [..., nq, R] -> [..., R]: strided_sum32 of width 4 over q"""
    nq = terms.shape[-2]
    if variant == "tail_dropped":
        terms = terms[..., :nq // 4 * 4, :]
        if terms.shape[-2] == 0:
            return np.zeros(terms.shape[:-2] + terms.shape[-1:], dtype=F)
    t = np.swapaxes(terms, -1, -2)
    if variant == "fourth_wave_dropped":
        t = t.copy()
        t[..., 3::4] = 0
    return strided_sum32(t, 4)


def gr_bwd_f32(d, xt, feats, variant=None):
    d, xt, feats = np.asarray(d, F), np.asarray(xt, F), np.asarray(feats, F)
    B, T, N = d.shape
    if variant == "d_transposed_strides":
        d = np.ascontiguousarray(d.reshape(B, N, T).swapaxes(1, 2))
    d_xt = _split4(d[:, :, :, None] * feats[:, None, :, :], variant)                          # [B, T, N, G] over n
    d_f = _split4(d.swapaxes(1, 2)[:, :, :, None] * xt[:, None, :, :], variant)               # [B, N, T, G] over t
    return d_xt, d_f


# ================================================================================================ embed_relu (exact)
EMBED_CASES = ((1, 3, 4), (37, 11, 16), (5, 50, 1028))                 # (M, V, E)
POISON = float("nan")


def embed_values(case):
    """-> (table [V, E] with the rows no index selects poisoned, idx [M] int64 with repeats and V - 1, drop [M, E] of 0 / 2)"""
    M, V, E = case
    rng = rng_of("embed", tuple(case))
    table = rng.standard_normal((V, E)).astype(F)
    idx = rng.integers(0, V, M).astype(np.int64)
    idx[-1] = V - 1
    if M >= 3:
        idx[1] = idx[0]
    unused = np.setdiff1d(np.arange(V), idx)
    table[unused] = POISON
    drop = (rng.random((M, E)) < 0.5).astype(F) * F(2)
    return table, idx, drop


EMBED_MUTANTS = ("relu_dropped", "drop_ignored", "previous_row")


def embed_ref(table, idx, drop, variant=None):
    """max(table[idx], 0) (x drop): float32, exact"""
    rows = table[idx - 1] if variant == "previous_row" else table[idx]
    v = rows if variant == "relu_dropped" else np.maximum(rows, F(0))
    return v * drop if drop is not None and variant != "drop_ignored" else v
