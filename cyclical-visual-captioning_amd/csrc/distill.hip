// Word-level distillation in the vocabulary criterion ("Distillation"): the head's finishing pass against a DENSE
// target row, the teacher's next-word distribution, mixed with the one-hot loss.  Per row with student logits z [V] (the K-slice slabs
// summed by the selection blocks' row loader, csrc/select_row.h: slab 0 + slab 1 + ... + bias, vocab_head_nll_kernel's order), teacher
// scores s [V] (any log-scale row, normalised or not), target t, weight w, alpha in [0, 1] and tau > 0:
//
//   p = softmax(z),  p_tau = softmax(z / tau),  q = softmax(s / tau)
//   row_nll  = w (lse(z) - z[t])                                     (unmixed, for logging)
//   row_kd   = w tau^2 sum_v q[v] (log q[v] - log p_tau[v])          (unmixed, for logging)
//   row_loss = (1 - alpha) row_nll + alpha row_kd
//   pre[v]   = w ((1 - alpha) (p[v] - [v == t]) + alpha tau (p_tau[v] - q[v]))          = d row_loss / d z[v]
//
// The row values.  A row's KL is a small difference of sums of terms up to 30 in size, and a row value of 17 has an fp32 ulp of
// 2e-6: plain fp32 sums and logf leave an error of several ulps of the result.  With e_s[v] = exp((s[v] - max s) / tau),
// S_q = sum e_s, S_tau = sum exp((z - max z) / tau), S_1 = sum exp(z - max z) and d[v] = (s[v] - max s) - (z[v] - max z),
//     sum_v q (log q - log p_tau) = (1 / tau) (sum_v e_s[v] d[v]) / S_q + log S_tau - log S_q        (sum q = 1 taken exactly)
//     lse(z) - z[t]               = log S_1 - (z[t] - max z)
// are evaluated in TWO-FLOAT arithmetic (an fp32 value and an fp32 remainder, error-free sums and fma products: Dekker 1971, Knuth):
// the differences d[v], the sums over the row (each thread's columns in ascending order, the four waves in a fixed order), the
// quotient, the logarithms (log S = k ln 2 + log m with S = m 2^k, m in [0.71, 1.42), ln 2 as a pair) and the mix; one rounding at
// the end.  No fp64 anywhere.  The exponentials themselves are fp32 expf of fp32 arguments.  A teacher entry of -inf has e_s = 0: its
// term is an exact 0 (selected, not multiplied).  A row with w == 0 writes exact zeros whatever its teacher row holds.  tau == 1 takes
// S_tau = S_1 in a uniform branch (the same bits).
// pre is plain fp32 around the row maxima: p = expf((z - max z) - log S_1) and so on, with the logarithms rounded to fp32.
//
// One workgroup per row.  The fused form keeps the student's and the teacher's row in registers (two NC-arrays, NC chosen from V as
// the selection blocks choose it; the build refuses scratch: build_hip.py), so the teacher row is read once; `pre` may alias slab 0
// (a thread reads its columns of every slab before it writes them).  The two-step form (shapes the fused head refuses: any V, any
// row count) streams both rows from memory with the same column-to-thread assignment, the same expressions and the same fixed-order
// reductions: on equal fp32 logits the two forms agree bit for bit.  Its forward leaves five numbers per row for its backward
// (stats [5, M]: max z, log S_1, log S_tau, max s, log S_q).
// contract(off), no atomics, no workspace allocation: capturable, bitwise deterministic.
// The teacher row of row m is teacher + map[m] * ld_t (map NULL: m); a mapped row outside [0, t_rows) is not read: that row's loss,
// kd and pre are NaN.
#include "select_row.h"
#include <math.h>

namespace {

// ---- two-float arithmetic: the value hi + lo, |lo| <= ulp(hi) / 2 after a normalising step
struct df { float hi, lo; };

__device__ __forceinline__ df two_sum(float a, float b) {                 // a + b exactly
#pragma clang fp contract(off)
    const float s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ df fast_two_sum(float a, float b) {            // a + b exactly when |a| >= |b| (or a == 0)
#pragma clang fp contract(off)
    const float s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ df two_prod(float a, float b) {                // a * b exactly
#pragma clang fp contract(off)
    const float p = a * b;
    return {p, fmaf(a, b, -p)};
}
__device__ __forceinline__ df df_add(df x, df y) {
#pragma clang fp contract(off)
    const df s = two_sum(x.hi, y.hi);
    return fast_two_sum(s.hi, s.lo + (x.lo + y.lo));
}
__device__ __forceinline__ df df_add_f(df x, float y) {
#pragma clang fp contract(off)
    const df s = two_sum(x.hi, y);
    return fast_two_sum(s.hi, s.lo + x.lo);
}
__device__ __forceinline__ df df_neg(df x) { return {-x.hi, -x.lo}; }
__device__ __forceinline__ df df_mul_f(df x, float y) {
#pragma clang fp contract(off)
    const df p = two_prod(x.hi, y);
    return fast_two_sum(p.hi, fmaf(x.lo, y, p.lo));
}
__device__ __forceinline__ df df_div(df a, df b) {
#pragma clang fp contract(off)
    const float r = a.hi / b.hi;
    const df p = two_prod(r, b.hi);
    const float rem = (((a.hi - p.hi) - p.lo) + a.lo) - r * b.lo;
    return fast_two_sum(r, rem / b.hi);
}
// log(S) for S >= 1: S.hi = m 2^k with m in [0.71, 1.42), k ln 2 from a pair whose first part has 16 bits (k * LN2_HI is exact)
__device__ __forceinline__ df df_log(df S) {
#pragma clang fp contract(off)
    int k;
    float m = frexpf(S.hi, &k);
    if (m < 0.70710678f) { m = m * 2.f; k -= 1; }
    const float kf = (float)k;
    return fast_two_sum(kf * 0.693138123f, logf(m) + (kf * 9.0580006145e-06f + S.lo / S.hi));
}
// the sum of a two-float value over the workgroup: the lanes of a wave by exchange, the four waves in the order (0 + 1) + (2 + 3)
__device__ __forceinline__ df block_sum_df(df v, float* red8) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = df_add(v, df{__shfl_xor(v.hi, o, 64), __shfl_xor(v.lo, o, 64)});
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        red8[2 * (threadIdx.x >> 6)] = v.hi;
        red8[2 * (threadIdx.x >> 6) + 1] = v.lo;
    }
    __syncthreads();
    return df_add(df_add(df{red8[0], red8[1]}, df{red8[2], red8[3]}), df_add(df{red8[4], red8[5]}, df{red8[6], red8[7]}));
}

__device__ __forceinline__ float kd_log_prob(float x, float mx, float it, float ls) {
#pragma clang fp contract(off)
    return (x - mx) * it - ls;
}

// gw: the row's weight (times the upstream scalar in the two-step backward); zc = z - max z; q: the teacher's probability; hit: 1 at
// the target's column
__device__ __forceinline__ float kd_pre(float gw, float alpha, float tau, float it, float zc, float ls1, float lst, float q, float hit) {
#pragma clang fp contract(off)
    const float p = expf(zc - ls1);
    const float pt = tau == 1.f ? p : expf(zc * it - lst);
    return gw * ((1.f - alpha) * (p - hit) + (alpha * tau) * (pt - q));
}

// the columns of a thread in ascending order: register slot u holds column v = tid + u * WG (NC > 0: NC slots, unrolled; NC == 0: the
// streaming form, as many as the row has).  Every column is tested against its OWN opaque copy of V (an empty volatile statement per
// column): the NC column tests are otherwise hoisted out of the passes as NC lane masks held in scalar registers and the columns'
// exponentials interleaved across the whole pass -- at NC = 32 that spills scalar registers (csrc/ensemble.hip has the same remedy
// per member)
__device__ __forceinline__ int kd_opaque(int v) {
    asm volatile("" : "+s"(v));
    return v;
}
#define KD_COLS(u, v) _Pragma("unroll KD_UNROLL") for (int u = 0, v = tid; u < (NC > 0 ? NC : nu); ++u, v += WG)
#define KD_IN(v) (v < kd_opaque(V))

template <int NC, bool FUSED>
__global__ __launch_bounds__(WG) void vocab_kd_fwd_kernel(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                                                          const int64_t* target, const float* w, const float* teacher, int ld_t,
                                                          const int* row_map, int t_rows, int V, float alpha, float tau, float it,
                                                          float* pre, int ld_pre, float* stats, int64_t* argmax, float* row_loss,
                                                          float* row_nll, float* row_kd) {
#pragma clang fp contract(off)
    static_assert(NC > 0 || !FUSED, "the streaming form reads materialised logits");
    constexpr int KD_UNROLL = NC > 0 ? NC : 1;            // (the streaming form's loops have a run-time length: not unrolled)
    __shared__ float red[4];
    __shared__ float red8[8];
    __shared__ int ired[4];
    __shared__ float xt_s;
    const int row = blockIdx.x, tid = threadIdx.x, M = gridDim.x;
    const int nu = (V + WG - 1) / WG;
    const float* x = parts + (size_t)row * ld;
    const int tgt = (int)target[row];
    const float wm = w[row];
    const int trow = row_map != nullptr ? row_map[row] : row;
    const bool t_ok = trow >= 0 && trow < t_rows;
    const float* s = teacher + (size_t)(t_ok ? trow : 0) * ld_t;
    float zr[NC > 0 ? NC : 1], sr[NC > 0 ? NC : 1];
    if constexpr (NC > 0) {
        load_logit_row<NC, 0, false>(x, nparts, part_stride, bias, kd_opaque(V), tid, zr);
        const int Vt = kd_opaque(V);
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int v = col<false>(tid, u);
            sr[u] = v < Vt ? s[v] : -INFINITY;
        }
    }
    auto Z = [&](int u, int v) { if constexpr (NC > 0) return zr[u]; else return x[v]; };
    auto S = [&](int u, int v) { if constexpr (NC > 0) return sr[u]; else return s[v]; };

    float m = -INFINITY, ms = -INFINITY;
    int mi = 0x7fffffff;
    KD_COLS(u, v) {
        if (KD_IN(v)) {
            const float xv = Z(u, v);
            if (xv > m) { m = xv; mi = v; }                       // ascending v per thread: first occurrence wins
            if (v == tgt) xt_s = xv;
            ms = fmaxf(ms, S(u, v));
        }
    }
    const float bm = block_max(m, red);
    int cand = m == bm ? mi : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    __syncthreads();
    if ((tid & 63) == 0) ired[tid >> 6] = cand;
    __syncthreads();
    const int best = min(min(ired[0], ired[1]), min(ired[2], ired[3]));
    const float bms = block_max(ms, red);

    // one pass: S_1, S_q, S_tau and sum e_s d, each a two-float sum of this thread's columns in ascending order
    df s1 = {0.f, 0.f}, sq = {0.f, 0.f}, st = {0.f, 0.f}, sa = {0.f, 0.f};
    KD_COLS(u, v) {
        if (KD_IN(v)) {
            const float zv = Z(u, v), sv = S(u, v);
            const df zc = two_sum(zv, -bm), sc = two_sum(sv, -bms);
            s1 = df_add_f(s1, expf(zc.hi));
            if (tau != 1.f) st = df_add_f(st, expf(zc.hi * it));
            const float es = expf(sc.hi * it);
            sq = df_add_f(sq, es);
            const df d = two_sum(sc.hi, -zc.hi);
            df term = two_prod(es, d.hi);
            term.lo = fmaf(es, d.lo + (sc.lo - zc.lo), term.lo);
            if (es > 0.f) sa = df_add(sa, term);                  // (a teacher entry at -inf: an exact 0, not 0 x inf)
        }
    }
    s1 = block_sum_df(s1, red8);
    sq = block_sum_df(sq, red8);
    sa = block_sum_df(sa, red8);
    const df l1 = df_log(s1), lq = df_log(sq);
    df lt = l1;
    if (tau != 1.f) lt = df_log(block_sum_df(st, red8));
    const float ls1 = l1.hi, lsq = lq.hi, lst = lt.hi;
    if (tid == 0) {
        if (argmax != nullptr) argmax[row] = best == 0x7fffffff ? 0 : best;      // all-NaN row: keep the index in range
        const bool live = wm != 0.f;
        const df nll = df_add(l1, df_neg(two_sum(xt_s, -bm)));
        df kd = df_add(df_mul_f(df_div(sa, sq), it), df_add(lt, df_neg(lq)));
        kd = df_mul_f(df_mul_f(kd, tau), tau);
        const df mix = df_add(df_mul_f(nll, 1.f - alpha), df_mul_f(kd, alpha));
        float loss = live ? df_mul_f(mix, wm).hi : 0.f;
        float kdr = live ? df_mul_f(kd, wm).hi : 0.f;
        if (live && !t_ok) kdr = loss = NAN;
        row_loss[row] = loss;
        row_nll[row] = live ? df_mul_f(nll, wm).hi : 0.f;
        row_kd[row] = kdr;
        if constexpr (!FUSED) {
            stats[row] = bm;
            stats[(size_t)M + row] = ls1;
            stats[2 * (size_t)M + row] = lst;
            stats[3 * (size_t)M + row] = bms;
            stats[4 * (size_t)M + row] = lsq;
        }
    }
    if constexpr (FUSED) {
        float* out = pre + (size_t)row * ld_pre;
        const int Vp = kd_opaque(V);
        KD_COLS(u, v) {
            if (v < Vp) {
                const float q = expf(kd_log_prob(S(u, v), bms, it, lsq));
                const float d = kd_pre(wm, alpha, tau, it, Z(u, v) - bm, ls1, lst, q, v == tgt ? 1.f : 0.f);
                out[v] = wm == 0.f ? 0.f : t_ok ? d : NAN;
            }
        }
    }
}

// d_logits[m, v] = g[0] * pre[m, v], pre formed from the forward's stats with the fused kernel's expressions
__global__ __launch_bounds__(WG) void vocab_kd_bwd_kernel(const float* logits, const float* stats, const int64_t* target, const float* w,
                                                          const float* teacher, int ld_t, const int* row_map, int t_rows, const float* g,
                                                          int V, float alpha, float tau, float it, float* d_logits) {
#pragma clang fp contract(off)
    const int m = blockIdx.x, M = gridDim.x;
    const int v = blockIdx.y * WG + threadIdx.x;
    if (v >= V) return;
    const size_t o = (size_t)m * V + v;
    const float gw = g[0] * w[m];
    const int trow = row_map != nullptr ? row_map[m] : m;
    const bool t_ok = trow >= 0 && trow < t_rows;
    if (gw == 0.f || !t_ok) {
        d_logits[o] = gw == 0.f ? 0.f : NAN;
        return;
    }
    const float sv = teacher[(size_t)trow * ld_t + v];
    const float q = expf(kd_log_prob(sv, stats[3 * (size_t)M + m], it, stats[4 * (size_t)M + m]));
    d_logits[o] = kd_pre(gw, alpha, tau, it, logits[o] - stats[m], stats[(size_t)M + m], stats[2 * (size_t)M + m], q,
                         v == (int)target[m] ? 1.f : 0.f);
}

// loss_sum, nll_sum, kd_sum: block b adds row vector b -- a two-float sum (thread t its rows t, t + 256, ... in ascending order, then
// the workgroup in block_sum_df's fixed order), rounded once: the exact sum of the fp32 row values unless they span more than 2^24
__global__ __launch_bounds__(WG) void kd_row_sums_kernel(const float* r0, float* s0, const float* r1, float* s1, const float* r2, float* s2,
                                                         int M) {
    __shared__ float red8[8];
    const float* r = blockIdx.x == 0 ? r0 : blockIdx.x == 1 ? r1 : r2;
    float* out = blockIdx.x == 0 ? s0 : blockIdx.x == 1 ? s1 : s2;
    df s = {0.f, 0.f};
    for (int m = threadIdx.x; m < M; m += WG) s = df_add_f(s, r[m]);
    s = block_sum_df(s, red8);
    if (threadIdx.x == 0) out[0] = s.hi;
}

// alpha in [0, 1], tau finite and > 0 (a NaN fails the comparisons)
bool kd_scalars_ok(float alpha, float tau) { return alpha >= 0.f && alpha <= 1.f && tau > 0.f && tau - tau == 0.f; }

}  // namespace

extern "C" int cvc_vocab_head_nll_kd_fwd(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                                         const int64_t* target, const float* w, const float* teacher, int ld_t, const int* row_map,
                                         int t_rows, int M, int V, float alpha, float tau, float* pre, int ld_pre, int64_t* argmax,
                                         float* row_loss, float* loss_sum, float* row_nll, float* nll_sum, float* row_kd, float* kd_sum,
                                         cvc_stream_t stream) {
    if (!parts || nparts < 1 || !target || !w || !teacher || !pre || !row_loss || !loss_sum || !row_nll || !nll_sum || !row_kd || !kd_sum ||
        M < 1 || V < 1 || V > WG * NC_MAX || ld < V || ld_pre < V || ld_t < V || t_rows < 1 || !kd_scalars_ok(alpha, tau))
        return CVC_E_BADARG;
    if (nparts > 1 && part_stride < (long long)(M - 1) * ld + V) return CVC_E_BADARG;
    // NC as the selection blocks choose it, in the loader's scalar form (select_dispatch decides from the operand it is shown, never
    // dereferenced there: a misaligned address)
    select_dispatch(reinterpret_cast<const float*>(uintptr_t(4)), 1, 0, nullptr, V, [&](auto nc, auto, auto) {
        hipLaunchKernelGGL((vocab_kd_fwd_kernel<decltype(nc)::value, true>), dim3(M), dim3(WG), 0, (hipStream_t)stream, parts, nparts,
                           part_stride, ld, bias, target, w, teacher, ld_t, row_map, t_rows, V, alpha, tau, 1.f / tau, pre, ld_pre,
                           (float*)nullptr, argmax, row_loss, row_nll, row_kd);
    });
    hipLaunchKernelGGL(kd_row_sums_kernel, dim3(3), dim3(WG), 0, (hipStream_t)stream, (const float*)row_loss, loss_sum,
                       (const float*)row_nll, nll_sum, (const float*)row_kd, kd_sum, M);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_nll_kd_fwd(const float* logits, const int64_t* target, const float* w, const float* teacher, int ld_t,
                                    const int* row_map, int t_rows, int M, int V, float alpha, float tau, float* stats, int64_t* argmax,
                                    float* row_loss, float* loss_sum, float* row_nll, float* nll_sum, float* row_kd, float* kd_sum,
                                    cvc_stream_t stream) {
    if (!logits || !target || !w || !teacher || !stats || !row_loss || !loss_sum || !row_nll || !nll_sum || !row_kd || !kd_sum || M < 1 ||
        V < 1 || ld_t < V || t_rows < 1 || !kd_scalars_ok(alpha, tau))
        return CVC_E_BADARG;
    hipLaunchKernelGGL((vocab_kd_fwd_kernel<0, false>), dim3(M), dim3(WG), 0, (hipStream_t)stream, logits, 1, 0LL, V, (const float*)nullptr,
                       target, w, teacher, ld_t, row_map, t_rows, V, alpha, tau, 1.f / tau, (float*)nullptr, 0, stats, argmax, row_loss,
                       row_nll, row_kd);
    hipLaunchKernelGGL(kd_row_sums_kernel, dim3(3), dim3(WG), 0, (hipStream_t)stream, (const float*)row_loss, loss_sum,
                       (const float*)row_nll, nll_sum, (const float*)row_kd, kd_sum, M);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_nll_kd_bwd(const float* logits, const float* stats, const int64_t* target, const float* w, const float* teacher,
                                    int ld_t, const int* row_map, int t_rows, const float* g, int M, int V, float alpha, float tau,
                                    float* d_logits, cvc_stream_t stream) {
    if (!logits || !stats || !target || !w || !teacher || !g || !d_logits || M < 1 || V < 1 || ld_t < V || t_rows < 1 ||
        (V + WG - 1) / WG > 65535 || !kd_scalars_ok(alpha, tau))
        return CVC_E_BADARG;
    hipLaunchKernelGGL(vocab_kd_bwd_kernel, dim3(M, (V + WG - 1) / WG), dim3(WG), 0, (hipStream_t)stream, logits, stats, target, w, teacher,
                       ld_t, row_map, t_rows, g, V, alpha, tau, 1.f / tau, d_logits);
    return cvc_launch_status();
}
