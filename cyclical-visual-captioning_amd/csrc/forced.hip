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
// The row's logits stay in registers (NC per thread, V <= 256 * FORCED_NC_MAX), loaded as float4 where V % 4 == 0 -- the row loader
// is the one of sample_select_kernel (same column map, same order of the slab sum).  The thread that owns column w publishes z[w]
// through LDS; max and sum-exp go through the DPP wave reductions and the four wave partials through LDS in the fixed order
// (w0 + w1) + (w2 + w3); the count is an integer DPP wave sum and the same merge.  No atomics: bitwise deterministic.
#include "cvc_common.h"
#include <math.h>

namespace {

constexpr int WG = 256;
constexpr int FORCED_NC_MAX = 32;              // logits per thread: V <= 8192, the bound of the other selection blocks

// wave_sum of cvc_common.h over integers (the DPP network moves 32-bit words: same steps, same masks)
__device__ __forceinline__ int wave_sum_int(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);        // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);       // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);       // row_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);       // row_bcast15 -> rows 1, 3 (rows 0, 2 add 0)
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);       // row_bcast31 -> rows 2, 3
    return __builtin_amdgcn_readlane(v, 63);
}

// NC logits per thread; NP > 0: that many slabs summed with an unrolled loop, NP == 0: nparts at run time.  VEC (V % 4 == 0,
// 16-byte aligned operands): NC / 4 float4 groups, element u at column (tid + (u / 4) * WG) * 4 + u % 4; otherwise column tid + u * WG.
// Both sum a column's slabs in the same order (same bits); only the loads differ.
template <int NC, int NP, bool VEC>
__global__ __launch_bounds__(WG) void forced_select_kernel(const float* parts, int nparts, long long part_stride, const float* bias,
                                                           int V, const int64_t* word, int wstride, float* logprob, int32_t* rank) {
#pragma clang fp contract(off)
    __shared__ float red_m[4], red_s[4], zw_pub;
    __shared__ int red_c[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = parts + (size_t)row * V;
    float z[NC];
    auto col = [&](int u) { return VEC ? (tid + (u >> 2) * WG) * 4 + (u & 3) : tid + u * WG; };
    if constexpr (VEC) {
#pragma unroll
        for (int g = 0; g < NC / 4; ++g) {
            const int e = (tid + g * WG) * 4;
            f32x4 s = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (e < V) {                                  // V % 4 == 0: the whole group is inside the row
                if constexpr (NP > 0) {
                    f32x4 p[NP];
#pragma unroll
                    for (int k = 0; k < NP; ++k) p[k] = ld4(x + (size_t)k * part_stride + e);
                    s = p[0];
#pragma unroll
                    for (int k = 1; k < NP; ++k) s += p[k];
                } else {
                    s = ld4(x + e);
                    for (int k = 1; k < nparts; ++k) s += ld4(x + (size_t)k * part_stride + e);
                }
                if (bias != nullptr) s += ld4(bias + e);
            }
            z[4 * g] = s.x; z[4 * g + 1] = s.y; z[4 * g + 2] = s.z; z[4 * g + 3] = s.w;
        }
    } else {
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int v = col(u);
            float s = -INFINITY;
            if (v < V) {
                s = x[v];
                for (int k = 1; k < nparts; ++k) s += x[(size_t)k * part_stride + v];
                if (bias != nullptr) s += bias[v];
            }
            z[u] = s;
        }
    }
    const int64_t w64 = word[(size_t)row * wstride];
    const bool valid = w64 >= 0 && w64 < (int64_t)V;      // uniform over the workgroup
    const int w = valid ? (int)w64 : -1;                  // -1: no column matches, nothing is published
    // the row's maximum (padding is -inf); the owner of column w publishes its logit
    float m = -INFINITY;
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        m = fmaxf(m, z[u]);
        if (col(u) == w) zw_pub = z[u];
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
        cnt += ((z[u] > zw) | ((z[u] == zw) & (col(u) < w))) ? 1 : 0;       // padding: -inf > zw never, and its column is >= V > w
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
    // the argument checks of the sampling blocks (csrc/sample.hip::select_check), without their temperature / generator state
    if (!parts || !word || nparts < 1 || M < 1 || V < 2 || word_stride < 1) return CVC_E_BADARG;
    if (nparts > 1 && part_stride < (long long)M * V) return CVC_E_BADARG;
    if ((long long)M * V > 0xffffffffLL) return CVC_E_TOOBIG;
    if ((V + WG - 1) / WG > FORCED_NC_MAX) return CVC_E_TOOBIG;
    const int nc = (V + WG - 1) / WG;
    const bool vec = (V & 3) == 0 && ((uintptr_t)parts & 15) == 0 && (nparts == 1 || (part_stride & 3) == 0) &&
                     ((uintptr_t)bias & 15) == 0;
#define CVC_FS(NC_, NP_, VEC_) hipLaunchKernelGGL((forced_select_kernel<NC_, NP_, VEC_>), dim3(M), dim3(WG), 0, (hipStream_t)stream, \
                                                  parts, nparts, part_stride, bias, V, word, word_stride, logprob, rank)
#define CVC_FS_NP(NG_) do { switch (nparts) { case 1: CVC_FS(4 * NG_, 1, true); break; case 2: CVC_FS(4 * NG_, 2, true); break; \
                                              case 4: CVC_FS(4 * NG_, 4, true); break; case 6: CVC_FS(4 * NG_, 6, true); break; \
                                              case 8: CVC_FS(4 * NG_, 8, true); break; default: CVC_FS(4 * NG_, 0, true); break; } \
                           } while (0)
    if (vec) {                                             // float4 groups: V <= NG * 1024
        const int ng = (V + 4 * WG - 1) / (4 * WG);
        if (ng <= 1) CVC_FS_NP(1);
        else if (ng <= 2) CVC_FS_NP(2);
        else if (ng <= 4) CVC_FS_NP(4);
        else if (ng <= 5) CVC_FS_NP(5);
        else CVC_FS_NP(8);
    } else if (nc <= 1) CVC_FS(1, 0, false);
    else if (nc <= 2) CVC_FS(2, 0, false);
    else if (nc <= 4) CVC_FS(4, 0, false);
    else if (nc <= 8) CVC_FS(8, 0, false);
    else if (nc <= 16) CVC_FS(16, 0, false);
    else if (nc <= 20) CVC_FS(20, 0, false);
    else CVC_FS(32, 0, false);
#undef CVC_FS_NP
#undef CVC_FS
    return cvc_launch_status();
}
