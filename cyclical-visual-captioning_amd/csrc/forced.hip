// Teacher-forced decoding: the log-prob and the rank of a GIVEN next word, one workgroup per row.
// The selection block of the decode engine's forced mode (cvc/decode/engine.py, forced_n): it sums the K-slice slabs of the
// vocabulary GEMM (+ bias) in the finishing pass's order (cvc_tile_linear_finish: slab 0 + slab 1 + ... + bias, so the logits are
// bit for bit what the greedy / beam / sampling selection sees), reads the row's word and writes two numbers; it writes no word.
//
//   w          = word[r * word_stride]                    outside [0, V): logprob = NaN, rank = -1, nothing is read at w
//   logprob[r] = z[r, w] - logsumexp_v z[r, v]            full V, UNK included: the definition of csrc/sample.hip
//   rank[r]    = #{v : z[v] > z[w]} + #{v < w : z[v] == z[w]}        0 <=> w is the arg-max under the lower-index tie rule;
//                                                                    NaN logits compare false
//
// The row's logits stay in registers, loaded by the row loader all selection blocks share (csrc/select_row.h: column map, order of
// the slab sum, argument checks and the NC / NP / VEC dispatch).  The thread that owns column w publishes z[w] through LDS; max and
// sum-exp go through the DPP wave reductions and the four wave partials through LDS in the fixed order (w0 + w1) + (w2 + w3); the
// count is an integer DPP wave sum and the same merge.  No atomics: bitwise deterministic.
#include "select_row.h"
#include <math.h>

namespace {

// NC / NP / VEC: the loader form (csrc/select_row.h)
template <int NC, int NP, bool VEC>
__global__ __launch_bounds__(WG) void forced_select_kernel(const float* parts, int nparts, long long part_stride, const float* bias,
                                                           int V, const int64_t* word, int wstride, float* logprob, int32_t* rank) {
#pragma clang fp contract(off)
    __shared__ float red_m[4], red_s[4], zw_pub;
    __shared__ int red_c[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float z[NC];
    load_logit_row<NC, NP, VEC>(parts + (size_t)row * V, nparts, part_stride, bias, V, tid, z);
    const int64_t w64 = word[(size_t)row * wstride];
    const bool valid = w64 >= 0 && w64 < (int64_t)V;      // uniform over the workgroup
    const int w = valid ? (int)w64 : -1;                  // -1: no column matches, nothing is published
    // the row's maximum (padding is -inf); the owner of column w publishes its logit
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        m = fmaxf(m, z[u]);
        if (col<VEC>(tid, u) == w) zw_pub = z[u];
    }
    m = wave_max(m);
    if (lane == 0) red_m[wave] = m;
    __syncthreads();
    if (!valid) {
        if (tid == 0) {
            if (logprob != nullptr) logprob[row] = __builtin_nanf("");
            if (rank != nullptr) rank[row] = -1;
        }
        return;
    }
    m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    const float zw = zw_pub;
    float se = 0.f;
    int cnt = 0;
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        if (m != -INFINITY) se += expf(z[u] - m);          // padding: exp(-inf) = 0
        cnt += ((z[u] > zw) | ((z[u] == zw) & (col<VEC>(tid, u) < w))) ? 1 : 0;       // padding: -inf > zw never, and its column is >= V > w
    }
    se = wave_sum(se);
    cnt = wave_sum_int(cnt);
    if (lane == 0) { red_s[wave] = se; red_c[wave] = cnt; }
    __syncthreads();
    if (tid == 0) {
        const float S = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        if (logprob != nullptr) logprob[row] = zw - (m + logf(S));
        if (rank != nullptr) rank[row] = (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]);
    }
}

}  // namespace

extern "C" int cvc_forced_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                                       const int64_t* word, int word_stride, float* logprob, int32_t* rank, cvc_stream_t stream) {
    const int rc = select_row_check(parts, nparts, part_stride, M, V, word, word_stride);
    if (rc != 0) return rc;
    select_dispatch(parts, nparts, part_stride, bias, V, [&](auto nc, auto np, auto vec) {
        hipLaunchKernelGGL((forced_select_kernel<decltype(nc)::value, decltype(np)::value, decltype(vec)::value>), dim3(M), dim3(WG), 0,
                           (hipStream_t)stream, parts, nparts, part_stride, bias, V, word, word_stride, logprob, rank);
    });
    return cvc_launch_status();
}
