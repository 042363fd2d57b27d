// The training step's pointwise kernels: the gate gradients of the LSTM cells (cvc_lstm_pointwise_bwd, _bwd3, _bwd3_drop, _bwd4,
// _bwd4_pair) and the small deterministic helpers beside them -- the scaling by the upstream scalar (cvc_scale_by_scalar), the stable
// order of the word indices (cvc_stable_order) and the column sums of the bias gradients (cvc_col_sum).  Pinned to fp64 references
// by tests/test_gpu_train_kernels.py.  Nothing here runs in decoding.
#include "row_block.h"
#include "dropout_rng.h"
#include <math.h>

namespace {

// y[i] = g[0] * x[i] (the backward of the fused head criterion: d_logits = upstream scalar x pre), float4 granules
__global__ __launch_bounds__(WG) void scale_by_scalar_kernel(const float* x, const float* g, long long n4, float* y) {
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i >= n4) return;
    const float s = g[0];
    const f32x4 v = ld4(x + i * 4);
    st4(y + i * 4, f32x4{v.x * s, v.y * s, v.z * s, v.w * s});
}

// ------------------------------------------------------------------ LSTM pointwise backward
__global__ __launch_bounds__(WG) void lstm_pointwise_bwd_kernel(const float* d_h, const float* d_h2, const float* d_h3, const float* d_c,
                                                                const float* gates, const float* c_prev, const float* c_new, int M,
                                                                int R, float* d_gates, float* d_c_prev, float* d_gates_q,
                                                                DropSpec rng3) {
    const int j = blockIdx.x * WG + threadIdx.x;
    const int m = blockIdx.y;
    if (j >= R) return;
    const size_t o = (size_t)m * R + j, g0 = (size_t)m * 4 * R + j;
    const float ig = gates[g0], fg = gates[g0 + R], gg = gates[g0 + 2 * R], og = gates[g0 + 3 * R];
    const float tc = tanhf(c_new[o]);
    // h' may have gone out as up to three tensors (one per consumer): their gradients are summed here, not by autograd
    // (rng3: the third tensor went out through nn.Dropout fused into the cell's launch -- its gradient takes the same mask)
    float dh3 = d_h3 != nullptr ? d_h3[o] : 0.f;
    if (rng3.state != nullptr) dh3 *= cvc_drop_mult(rng3, rng3.state[0], rng3.state[1], rng3.state[2], (uint32_t)o);
    const float dh = ((d_h != nullptr ? d_h[o] : 0.f) + (d_h2 != nullptr ? d_h2[o] : 0.f)) + dh3;
    const float dcn = (d_c != nullptr ? d_c[o] : 0.f) + dh * og * (1.f - tc * tc);
    const float d0 = dcn * gg * ig * (1.f - ig), d1 = dcn * c_prev[o] * fg * (1.f - fg);
    const float d2 = dcn * ig * (1.f - gg * gg), d3 = dh * tc * og * (1.f - og);
    d_gates[g0] = d0;
    d_gates[g0 + R] = d1;
    d_gates[g0 + 2 * R] = d2;
    d_gates[g0 + 3 * R] = d3;
    d_c_prev[o] = dcn * fg;
    if (d_gates_q != nullptr) {                      // column g*R + j -> quad (g*R + j)/4, element j&3 (R % 4 == 0)
        const size_t q0 = ((size_t)(j >> 2) * 64 + m) * 4 + (j & 3), qs = (size_t)(R >> 2) * 256;
        d_gates_q[q0] = d0;
        d_gates_q[q0 + qs] = d1;
        d_gates_q[q0 + 2 * qs] = d2;
        d_gates_q[q0 + 3 * qs] = d3;
    }
}

// four gradients of h' (the C-driven training loops: this step's other consumers, the next step's two cells, the dropped output),
// summed in the order d_h[0], d_h[1], d_h[2], d_hd * mask.  Each d_h[i] may arrive as the K-slice planes of the backward-data
// product that produced it: summed here, in plane order, instead of by a launch of their own.
struct HSrc3 { cvc_grad_src s[3]; };
__device__ __forceinline__ float hsrc_load(const cvc_grad_src& g, int m, int j) {
    if (g.p == nullptr) return 0.f;
    const float* p = g.p + (size_t)m * g.ld + j;
    float v = p[0];
    for (int k = 1; k < g.nplanes; ++k) v += p[(size_t)k * g.plane_stride];
    return v;
}
__global__ __launch_bounds__(WG) void lstm_pointwise_bwd4_kernel(HSrc3 src, const float* d_hd, DropSpec rng, const float* d_c,
                                                                 const float* gates, const float* c_prev, const float* c_new, int M,
                                                                 int R, float* d_gates, float* d_c_prev, float* d_gates_q, float* dg_sum,
                                                                 int q_row0) {
#pragma clang fp contract(off)          // (every operation rounds on its own: the same bits as the vector form, see below)
    const int j = blockIdx.x * WG + threadIdx.x;
    const int m = blockIdx.y;
    if (j >= R) return;
    const size_t o = (size_t)m * R + j, g0 = (size_t)m * 4 * R + j;
    const float ig = gates[g0], fg = gates[g0 + R], gg = gates[g0 + 2 * R], og = gates[g0 + 3 * R];
    const float tc = tanhf(c_new[o]);
    // running sum over the steps of the loop (dg_sum [M, 4R], zero before the last step's launch): the bias gradients and the dY of
    // the step-invariant fc_feats columns, accumulated by the same thread launch after launch (stream-ordered: deterministic)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (dg_sum != nullptr) { s0 = dg_sum[g0]; s1 = dg_sum[g0 + R]; s2 = dg_sum[g0 + 2 * R]; s3 = dg_sum[g0 + 3 * R]; }
    float dhd = d_hd != nullptr ? d_hd[o] : 0.f;
    if (rng.state != nullptr) dhd *= cvc_drop_mult(rng, rng.state[0], rng.state[1], rng.state[2], (uint32_t)o);
    const float dh = ((hsrc_load(src.s[0], m, j) + hsrc_load(src.s[1], m, j)) + hsrc_load(src.s[2], m, j)) + dhd;
    const float dcn = (d_c != nullptr ? d_c[o] : 0.f) + dh * og * (1.f - tc * tc);
    const float d0 = dcn * gg * ig * (1.f - ig), d1 = dcn * c_prev[o] * fg * (1.f - fg);
    const float d2 = dcn * ig * (1.f - gg * gg), d3 = dh * tc * og * (1.f - og);
    d_gates[g0] = d0;
    d_gates[g0 + R] = d1;
    d_gates[g0 + 2 * R] = d2;
    d_gates[g0 + 3 * R] = d3;
    d_c_prev[o] = dcn * fg;
    if (dg_sum != nullptr) { dg_sum[g0] = s0 + d0; dg_sum[g0 + R] = s1 + d1; dg_sum[g0 + 2 * R] = s2 + d2; dg_sum[g0 + 3 * R] = s3 + d3; }
    if (d_gates_q != nullptr) {        // (q_row0: this launch's rows sit behind another loop's in a joint 64-row operand)
        const size_t q0 = ((size_t)(j >> 2) * 64 + q_row0 + m) * 4 + (j & 3), qs = (size_t)(R >> 2) * 256;
        d_gates_q[q0] = d0;
        d_gates_q[q0 + qs] = d1;
        d_gates_q[q0 + 2 * qs] = d2;
        d_gates_q[q0 + 3 * qs] = d3;
    }
}

// The same arithmetic, four hidden units per thread: every operand as one 16-byte load, and the K-slice planes of a gradient source
// requested four at a time before the first is added (the scalar form above walks a source's planes one dependent load after the
// other -- three sources x 5-8 planes of memory latency in an 11 us launch).  Sums in the same order, and contraction into fused
// multiply-adds switched OFF in both forms (hipcc's device default, -ffp-contract=fast, fused the two forms' dcn differently: 1-2 ulp
// apart in d_gates i/f/g and d_c_prev): same bits.
__device__ __forceinline__ f32x4 hsrc_load4(const cvc_grad_src& g, int m, int j) {
    if (g.p == nullptr) return f32x4{0.f, 0.f, 0.f, 0.f};
    const float* p = g.p + (size_t)m * g.ld + j;
    f32x4 v = ld4(p);
    int k = 1;
    for (; k + 3 < g.nplanes; k += 4) {
        const f32x4 a = ld4(p + (size_t)k * g.plane_stride), b = ld4(p + (size_t)(k + 1) * g.plane_stride);
        const f32x4 c = ld4(p + (size_t)(k + 2) * g.plane_stride), d = ld4(p + (size_t)(k + 3) * g.plane_stride);
        v += a; v += b; v += c; v += d;
    }
    for (; k < g.nplanes; ++k) v += ld4(p + (size_t)k * g.plane_stride);
    return v;
}
__device__ __forceinline__ void lstm_pointwise_bwd4v_body(const HSrc3& src, const float* d_hd, const DropSpec& rng, const float* d_c,
                                                          const float* gates, const float* c_prev, const float* c_new, int M,
                                                          int R, float* d_gates, float* d_c_prev, float* d_gates_q, float* dg_sum,
                                                          int q_row0) {
#pragma clang fp contract(off)
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) * 4;      // (64-thread workgroups: 8 x M of them at R = 2048)
    const int m = blockIdx.y;
    if (j >= R || m >= M) return;
    const size_t o = (size_t)m * R + j, g0 = (size_t)m * 4 * R + j;
    const f32x4 ig = ld4(gates + g0), fg = ld4(gates + g0 + R), gg = ld4(gates + g0 + 2 * R), og = ld4(gates + g0 + 3 * R);
    const f32x4 cn = ld4(c_new + o), cp = ld4(c_prev + o);
    f32x4 s0 = {0, 0, 0, 0}, s1 = s0, s2 = s0, s3 = s0;
    if (dg_sum != nullptr) { s0 = ld4(dg_sum + g0); s1 = ld4(dg_sum + g0 + R); s2 = ld4(dg_sum + g0 + 2 * R); s3 = ld4(dg_sum + g0 + 3 * R); }
    f32x4 dhd = d_hd != nullptr ? ld4(d_hd + o) : f32x4{0, 0, 0, 0};
    const f32x4 dcin = d_c != nullptr ? ld4(d_c + o) : f32x4{0, 0, 0, 0};
    const f32x4 h0 = hsrc_load4(src.s[0], m, j), h1 = hsrc_load4(src.s[1], m, j), h2 = hsrc_load4(src.s[2], m, j);
    if (rng.state != nullptr) {
        const uint32_t r0 = rng.state[0], r1 = rng.state[1], r2 = rng.state[2];
#pragma unroll
        for (int e = 0; e < 4; ++e) dhd[e] *= cvc_drop_mult(rng, r0, r1, r2, (uint32_t)(o + e));
    }
    f32x4 d0, d1, d2, d3, dcp;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float tc = tanhf(cn[e]);
        const float dh = ((h0[e] + h1[e]) + h2[e]) + dhd[e];
        const float dcn = dcin[e] + dh * og[e] * (1.f - tc * tc);
        d0[e] = dcn * gg[e] * ig[e] * (1.f - ig[e]);
        d1[e] = dcn * cp[e] * fg[e] * (1.f - fg[e]);
        d2[e] = dcn * ig[e] * (1.f - gg[e] * gg[e]);
        d3[e] = dh * tc * og[e] * (1.f - og[e]);
        dcp[e] = dcn * fg[e];
    }
    st4(d_gates + g0, d0); st4(d_gates + g0 + R, d1); st4(d_gates + g0 + 2 * R, d2); st4(d_gates + g0 + 3 * R, d3);
    st4(d_c_prev + o, dcp);
    if (dg_sum != nullptr) { st4(dg_sum + g0, s0 + d0); st4(dg_sum + g0 + R, s1 + d1); st4(dg_sum + g0 + 2 * R, s2 + d2); st4(dg_sum + g0 + 3 * R, s3 + d3); }
    if (d_gates_q != nullptr) {
        float* q = d_gates_q + ((size_t)(j >> 2) * 64 + q_row0 + m) * 4;
        const size_t qs = (size_t)(R >> 2) * 256;
        st4(q, d0); st4(q + qs, d1); st4(q + 2 * qs, d2); st4(q + 3 * qs, d3);
    }
}
__global__ __launch_bounds__(WG) void lstm_pointwise_bwd4v_kernel(HSrc3 src, const float* d_hd, DropSpec rng, const float* d_c,
                                                                  const float* gates, const float* c_prev, const float* c_new, int M,
                                                                  int R, float* d_gates, float* d_c_prev, float* d_gates_q, float* dg_sum,
                                                                  int q_row0) {
    lstm_pointwise_bwd4v_body(src, d_hd, rng, d_c, gates, c_prev, c_new, M, R, d_gates, d_c_prev, d_gates_q, dg_sum, q_row0);
}
// Two independent gate-gradient launches as ONE (blockIdx.z picks the argument set): the two loops of the cyclical pass share the
// LSTM cells, and in the joint back-propagation their gate-gradient kernels of a step are two ~10 us, latency-bound launches of the
// same shape -- 80 launches per training step become 40.
struct PwOne {
    HSrc3 src; const float* d_hd; DropSpec rng; const float *d_c, *gates, *c_prev, *c_new; int M; float *d_gates, *d_c_prev, *d_gates_q, *dg_sum;
    int q_row0;
};
__global__ __launch_bounds__(WG) void lstm_pointwise_bwd4v_pair_kernel(PwOne a, PwOne b, int R) {
    // (uniform branch, not an indexed argument array: indexing kernel arguments makes hipcc copy them to scratch)
    if (blockIdx.z == 0) lstm_pointwise_bwd4v_body(a.src, a.d_hd, a.rng, a.d_c, a.gates, a.c_prev, a.c_new, a.M, R, a.d_gates, a.d_c_prev, a.d_gates_q, a.dg_sum, a.q_row0);
    else lstm_pointwise_bwd4v_body(b.src, b.d_hd, b.rng, b.d_c, b.gates, b.c_prev, b.c_new, b.M, R, b.d_gates, b.d_c_prev, b.d_gates_q, b.dg_sum, b.q_row0);
}

}  // namespace

// ---- small dense helpers of the training step that used to be library launches (a radix sort of 1 280 keys is three launches; a
// bias gradient is a generic reduction): both deterministic, fixed summation order.
//
// Stable order of n int64 keys by counting: rank(i) = #{j : key[j] < key[i]} + #{j < i : key[j] == key[i]}; order[rank(i)] = i.
// A workgroup ranks 32 keys: it holds all n keys in LDS, thread (key il, segment sg) counts over an eighth of the j range (all
// lanes of a segment read the same LDS word: broadcast), the eight counts are added through LDS.
__global__ __launch_bounds__(WG) void stable_order_kernel(const int64_t* key, int n, int64_t* order) {
    extern __shared__ int64_t keys[];
    __shared__ int cnt[8][32];
    for (int j = threadIdx.x; j < n; j += WG) keys[j] = key[j];
    __syncthreads();
    const int il = threadIdx.x & 31, sg = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + il;
    const int per = (n + 7) / 8;
    const int j0 = sg * per, j1 = min(n, j0 + per);
    int r = 0;
    if (i < n) {
        const int64_t k = keys[i];
        // j < i: ties count; j > i: strictly smaller only.  Split at i so that the loops carry no per-element branch.
        const int m = min(max(i, j0), j1);
#pragma unroll 8
        for (int j = j0; j < m; ++j) r += keys[j] <= k ? 1 : 0;
#pragma unroll 8
        for (int j = max(m, i + 1); j < j1; ++j) r += keys[j] < k ? 1 : 0;
    }
    cnt[sg][il] = r;
    __syncthreads();
    if (sg == 0 && i < n) {
        int t = 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) t += cnt[g][il];
        order[t] = i;
    }
}

// out[c] (and out2[c]) = sum over the S rows of x[s, c].  One column per lane (a wave reads 256 contiguous bytes of a row); a
// workgroup owns 64 columns x one chunk of rows, its 4 waves take rows w, w + 4, ... with 8 loads in flight each and are combined
// in wave order.  More than one chunk: the chunks' sums go to a [chunks, n] workspace and a second launch of the same kernel adds
// them, again in a fixed order.
__global__ __launch_bounds__(WG) void col_sum_kernel(const float* x, long long ld, int S, int rows_per_chunk, int n, float* out, long long ld_out,
                                                     float* out2) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int r0 = blockIdx.y * rows_per_chunk, r1 = min(S, r0 + rows_per_chunk);
    float acc[8], tail = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.f;
    if (c < n) {
        const float* p = x + c;
        int r = r0 + wave;
        for (; r + 28 < r1; r += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += p[(size_t)(r + 4 * u) * ld];
        }
        for (; r < r1; r += 4) tail += p[(size_t)r * ld];
    }
    part[wave][lane] = (((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]))) + tail;
    __syncthreads();
    if (wave == 0 && c < n) {
        const float v = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        out[(size_t)blockIdx.y * ld_out + c] = v;
        if (out2 != nullptr) out2[c] = v;
    }
}

extern "C" int cvc_stable_order(const int64_t* key, int n, int64_t* order, cvc_stream_t stream) {
    if (!key || !order || n < 1 || n > 7168) return CVC_E_BADARG;      // keys + counters within the 64 KB a workgroup may take
    hipLaunchKernelGGL(stable_order_kernel, dim3((n + 31) / 32), dim3(WG), (size_t)n * 8, (hipStream_t)stream, key, n, order);
    return cvc_launch_status();
}

static int col_sum_chunks(int S) { return S <= 128 ? 1 : (S + 63) / 64 < 64 ? (S + 63) / 64 : 64; }

extern "C" long long cvc_col_sum_ws(int S, int n) {
    const int ch = col_sum_chunks(S);
    return ch > 1 ? (long long)ch * n : 0;
}

extern "C" int cvc_col_sum(const float* x, long long ld, int S, int n, float* out, float* out2, float* ws, cvc_stream_t stream) {
    if (!x || !out || S < 1 || n < 1 || ld < n) return CVC_E_BADARG;
    const int ch = col_sum_chunks(S);
    if (ch == 1) {
        hipLaunchKernelGGL(col_sum_kernel, dim3((n + 63) / 64, 1), dim3(WG), 0, (hipStream_t)stream, x, ld, S, S, n, out, 0, out2);
        return cvc_launch_status();
    }
    if (!ws) return CVC_E_BADARG;
    const int rpc = (S + ch - 1) / ch;
    hipLaunchKernelGGL(col_sum_kernel, dim3((n + 63) / 64, ch), dim3(WG), 0, (hipStream_t)stream, x, ld, S, rpc, n, ws, (long long)n, nullptr);
    hipLaunchKernelGGL(col_sum_kernel, dim3((n + 63) / 64, 1), dim3(WG), 0, (hipStream_t)stream, ws, (long long)n, ch, ch, n, out, 0, out2);
    return cvc_launch_status();
}

extern "C" int cvc_scale_by_scalar(const float* x, const float* g, long long n, float* y, cvc_stream_t stream) {
    if (!x || !g || !y || n < 4 || (n & 3) || ((uintptr_t)x & 15) || ((uintptr_t)y & 15)) return CVC_E_BADARG;
    const long long n4 = n / 4;
    hipLaunchKernelGGL(scale_by_scalar_kernel, dim3((unsigned)((n4 + WG - 1) / WG)), dim3(WG), 0, (hipStream_t)stream, x, g, n4, y);
    return cvc_launch_status();
}

extern "C" int cvc_lstm_pointwise_bwd(const float* d_h, const float* d_c, const float* gates, const float* c_prev,
                                      const float* c_new, int M, int R, float* d_gates, float* d_c_prev,
                                      float* d_gates_q, cvc_stream_t stream) {
    if (!gates || !c_prev || !c_new || !d_gates || !d_c_prev || M < 1 || R < 1) return CVC_E_BADARG;
    if (d_gates_q != nullptr && (M > 64 || (R & 3))) return CVC_E_BADARG;
    hipLaunchKernelGGL(lstm_pointwise_bwd_kernel, dim3((R + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, d_h, nullptr, nullptr,
                       d_c, gates, c_prev, c_new, M, R, d_gates, d_c_prev, d_gates_q, cvc_drop_spec(nullptr, 0, 0.f));
    return cvc_launch_status();
}

// the same with the gradients of up to three copies of h' (cvc_packed_lstm_train_fwd's h_out, h_out2, h_out3), summed in order
extern "C" int cvc_lstm_pointwise_bwd3(const float* d_h, const float* d_h2, const float* d_h3, const float* d_c, const float* gates,
                                       const float* c_prev, const float* c_new, int M, int R, float* d_gates, float* d_c_prev,
                                       float* d_gates_q, cvc_stream_t stream) {
    if (!gates || !c_prev || !c_new || !d_gates || !d_c_prev || M < 1 || R < 1) return CVC_E_BADARG;
    if (d_gates_q != nullptr && (M > 64 || (R & 3))) return CVC_E_BADARG;
    hipLaunchKernelGGL(lstm_pointwise_bwd_kernel, dim3((R + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, d_h, d_h2, d_h3, d_c,
                       gates, c_prev, c_new, M, R, d_gates, d_c_prev, d_gates_q, cvc_drop_spec(nullptr, 0, 0.f));
    return cvc_launch_status();
}

// ... where the third copy of h' went out through the dropout fused into cvc_packed_lstm_train_drop_fwd: d_h3 takes that mask
extern "C" int cvc_lstm_pointwise_bwd3_drop(const float* d_h, const float* d_h2, const float* d_h3, const uint32_t* rng_state,
                                            unsigned site, float p, const float* d_c, const float* gates, const float* c_prev,
                                            const float* c_new, int M, int R, float* d_gates, float* d_c_prev, float* d_gates_q,
                                            cvc_stream_t stream) {
    if (!gates || !c_prev || !c_new || !d_gates || !d_c_prev || M < 1 || R < 1 || !rng_state || p < 0.f || p >= 1.f) return CVC_E_BADARG;
    if (d_gates_q != nullptr && (M > 64 || (R & 3))) return CVC_E_BADARG;
    hipLaunchKernelGGL(lstm_pointwise_bwd_kernel, dim3((R + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, d_h, d_h2, d_h3, d_c,
                       gates, c_prev, c_new, M, R, d_gates, d_c_prev, d_gates_q, cvc_drop_spec(rng_state, site, p));
    return cvc_launch_status();
}

extern "C" int cvc_lstm_pointwise_bwd4(const cvc_grad_src* d_h, const float* d_hd, const uint32_t* rng_state, unsigned site, float p,
                                       const float* d_c, const float* gates, const float* c_prev, const float* c_new, int M, int R,
                                       float* d_gates, float* d_c_prev, float* d_gates_q, float* dg_sum, int q_row0, cvc_stream_t stream) {
    if (!d_h || !gates || !c_prev || !c_new || !d_gates || !d_c_prev || M < 1 || R < 1 || p < 0.f || p >= 1.f) return CVC_E_BADARG;
    if (d_gates_q != nullptr && (q_row0 < 0 || q_row0 + M > 64 || (R & 3))) return CVC_E_BADARG;
    HSrc3 src;
    for (int i = 0; i < 3; ++i) {
        src.s[i] = d_h[i];
        if (src.s[i].p != nullptr && (src.s[i].nplanes < 1 || src.s[i].ld < R)) return CVC_E_BADARG;
    }
    // four hidden units per thread when every operand allows 16-byte accesses (the training loops' buffers all do)
    bool vec = (R & 3) == 0;
    auto al = [&](const void* q) { return q == nullptr || ((uintptr_t)q & 15) == 0; };
    vec = vec && al(d_hd) && al(d_c) && al(gates) && al(c_prev) && al(c_new) && al(d_gates) && al(d_c_prev) && al(d_gates_q) && al(dg_sum);
    for (int i = 0; i < 3; ++i)
        if (src.s[i].p != nullptr) vec = vec && al(src.s[i].p) && (src.s[i].ld & 3) == 0 && (src.s[i].plane_stride & 3) == 0;
    if (vec)
        hipLaunchKernelGGL(lstm_pointwise_bwd4v_kernel, dim3((R / 4 + 63) / 64, M), dim3(64), 0, (hipStream_t)stream, src, d_hd,
                           cvc_drop_spec(rng_state, site, p), d_c, gates, c_prev, c_new, M, R, d_gates, d_c_prev, d_gates_q, dg_sum, q_row0);
    else
        hipLaunchKernelGGL(lstm_pointwise_bwd4_kernel, dim3((R + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, src, d_hd,
                           cvc_drop_spec(rng_state, site, p), d_c, gates, c_prev, c_new, M, R, d_gates, d_c_prev, d_gates_q, dg_sum, q_row0);
    return cvc_launch_status();
}

// cvc_lstm_pointwise_bwd4 for two argument sets in one launch (vector form only: every operand 16-byte aligned, R % 4 == 0)
extern "C" int cvc_lstm_pointwise_bwd4_pair(const cvc_pw_bwd_args* x, const cvc_pw_bwd_args* y, int R, cvc_stream_t stream) {
    if (!x || !y || R < 4 || (R & 3)) return CVC_E_BADARG;
    PwOne o[2];
    const cvc_pw_bwd_args* in[2] = {x, y};
    auto al = [&](const void* q) { return q == nullptr || ((uintptr_t)q & 15) == 0; };
    for (int k = 0; k < 2; ++k) {
        const cvc_pw_bwd_args& a = *in[k];
        if (!a.gates || !a.c_prev || !a.c_new || !a.d_gates || !a.d_c_prev || a.M < 1 || a.p < 0.f || a.p >= 1.f) return CVC_E_BADARG;
        if (a.d_gates_q != nullptr && (a.q_row0 < 0 || a.q_row0 + a.M > 64)) return CVC_E_BADARG;
        bool vec = al(a.d_hd) && al(a.d_c) && al(a.gates) && al(a.c_prev) && al(a.c_new) && al(a.d_gates) && al(a.d_c_prev) && al(a.d_gates_q) && al(a.dg_sum);
        for (int i = 0; i < 3; ++i) {
            o[k].src.s[i] = a.d_h[i];
            if (a.d_h[i].p != nullptr) {
                if (a.d_h[i].nplanes < 1 || a.d_h[i].ld < R) return CVC_E_BADARG;
                vec = vec && al(a.d_h[i].p) && (a.d_h[i].ld & 3) == 0 && (a.d_h[i].plane_stride & 3) == 0;
            }
        }
        if (!vec) return CVC_E_BADARG;
        o[k].d_hd = a.d_hd; o[k].rng = cvc_drop_spec(a.rng_state, a.site, a.p); o[k].d_c = a.d_c; o[k].gates = a.gates; o[k].c_prev = a.c_prev;
        o[k].c_new = a.c_new; o[k].M = a.M; o[k].d_gates = a.d_gates; o[k].d_c_prev = a.d_c_prev; o[k].d_gates_q = a.d_gates_q;
        o[k].dg_sum = a.dg_sum; o[k].q_row0 = a.q_row0;
    }
    const int Mmax = x->M > y->M ? x->M : y->M;
    hipLaunchKernelGGL(lstm_pointwise_bwd4v_pair_kernel, dim3((R / 4 + 63) / 64, Mmax, 2), dim3(64), 0, (hipStream_t)stream, o[0], o[1], R);
    return cvc_launch_status();
}
