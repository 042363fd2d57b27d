// What the word-selection blocks over the vocabulary logits share (csrc/sample_select.h: sampling, truncation, constraints;
// csrc/forced.hip: teacher forcing): one workgroup of WG threads per row keeps the row's logits in registers, NC per thread.
// The row loader sums the K-slice slabs of the vocabulary GEMM (+ bias) in the finishing pass's order (cvc_tile_linear_finish:
// slab 0 + slab 1 + ... + bias), so every block sees the logits of the greedy / beam selection bit for bit; the argument checks and
// the NC / NP / VEC choice of the entry points are here too, once.
#pragma once
#include "row_block.h"
#include <type_traits>

namespace {

constexpr int NC_MAX = 32;                     // logits per thread: V <= 8192, the bound of cvc_beam_select_parts

// the column of register slot u.  VEC: NC / 4 float4 groups, slot u at column (tid + (u / 4) * WG) * 4 + u % 4; otherwise tid + u * WG
template <bool VEC>
__device__ __forceinline__ int col(int tid, int u) { return VEC ? (tid + (u >> 2) * WG) * 4 + (u & 3) : tid + u * WG; }

// the inverse: the bit of the register slot of thread tid that holds column v (0: another thread's column, or v outside [0, V))
template <bool VEC>
__device__ __forceinline__ uint32_t slot_bit(int tid, int v, int V) {
    if (v < 0 || v >= V) return 0u;
    const int owner = VEC ? (v >> 2) % WG : v % WG, u = VEC ? ((v >> 2) / WG) * 4 + (v & 3) : v / WG;
    return tid == owner ? 1u << u : 0u;
}

// z[u] = the logit at col<VEC>(tid, u) of the row that starts at x, -inf past V.  NP > 0: that many slabs summed with an unrolled
// loop, NP == 0: nparts at run time.  VEC needs V % 4 == 0 and 16-byte aligned operands.  Both forms sum a column's slabs in the same
// order (same bits); only the loads differ.
template <int NC, int NP, bool VEC>
__device__ __forceinline__ void load_logit_row(const float* x, int nparts, long long part_stride, const float* bias, int V, int tid,
                                               float (&z)[NC]) {
#pragma clang fp contract(off)
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
            const int v = col<false>(tid, u);
            float s = -INFINITY;
            if (v < V) {
                s = x[v];
                for (int k = 1; k < nparts; ++k) s += x[(size_t)k * part_stride + v];
                if (bias != nullptr) s += bias[v];
            }
            z[u] = s;
        }
    }
}

}  // namespace

// the argument checks every selection block shares
static int select_row_check(const float* parts, int nparts, long long part_stride, int M, int V, const int64_t* word, int word_stride) {
    if (!parts || !word || nparts < 1 || M < 1 || V < 2 || word_stride < 1) return CVC_E_BADARG;
    if (nparts > 1 && part_stride < (long long)M * V) return CVC_E_BADARG;
    if ((long long)M * V > 0xffffffffLL) return CVC_E_TOOBIG;          // the hash counter r * V + v is one 32-bit word
    if ((V + WG - 1) / WG > NC_MAX) return CVC_E_TOOBIG;
    return 0;
}

// the loader form of a call: f(integral_constant<int, NC>, integral_constant<int, NP>, bool_constant<VEC>), called once
template <class F>
static void select_dispatch(const float* parts, int nparts, long long part_stride, const float* bias, int V, F f) {
    using std::integral_constant;
    const bool vec = (V & 3) == 0 && ((uintptr_t)parts & 15) == 0 && (nparts == 1 || (part_stride & 3) == 0) &&
                     ((uintptr_t)bias & 15) == 0;
    if (vec) {                                             // float4 groups: V <= NG * 1024
        auto groups = [&](auto ng_) {
            constexpr int NC = 4 * decltype(ng_)::value;
            auto slabs = [&](auto np_) { f(integral_constant<int, NC>{}, np_, std::true_type{}); };
            switch (nparts) {
                case 1: slabs(integral_constant<int, 1>{}); break;
                case 2: slabs(integral_constant<int, 2>{}); break;
                case 4: slabs(integral_constant<int, 4>{}); break;
                case 6: slabs(integral_constant<int, 6>{}); break;
                case 8: slabs(integral_constant<int, 8>{}); break;
                default: slabs(integral_constant<int, 0>{}); break;
            }
        };
        const int ng = (V + 4 * WG - 1) / (4 * WG);
        if (ng <= 1) groups(integral_constant<int, 1>{});
        else if (ng <= 2) groups(integral_constant<int, 2>{});
        else if (ng <= 4) groups(integral_constant<int, 4>{});
        else if (ng <= 5) groups(integral_constant<int, 5>{});
        else groups(integral_constant<int, 8>{});
    } else {
        auto scalar = [&](auto nc_) { f(nc_, integral_constant<int, 0>{}, std::false_type{}); };
        const int nc = (V + WG - 1) / WG;
        if (nc <= 1) scalar(integral_constant<int, 1>{});
        else if (nc <= 2) scalar(integral_constant<int, 2>{});
        else if (nc <= 4) scalar(integral_constant<int, 4>{});
        else if (nc <= 8) scalar(integral_constant<int, 8>{});
        else if (nc <= 16) scalar(integral_constant<int, 16>{});
        else if (nc <= 20) scalar(integral_constant<int, 20>{});
        else scalar(integral_constant<int, 32>{});
    }
}
