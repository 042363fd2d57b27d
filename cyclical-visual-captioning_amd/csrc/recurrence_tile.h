// The per-step tile product of the persistent forward recurrences (gru_persistent.hip, lstm_seq.hip): a workgroup's 32 gate
// rows of W_hh times the previous state of up to MT 32-clip tiles.  NW waves split K chunk by chunk (a chunk = 32 k; wave w
// owns chunks w, w + NW, ...; NC chunks per wave), keep their weights in registers as the three bf16 terms of the split
// product (gemm_split.h), and sum their partial tiles through LDS in a fixed order.
#pragma once
#include "gemm_split.h"

namespace {

// This wave's share of the weights, split once: register slot c holds chunk wave + NW * c.  `wl` = the lane's address within
// chunk 0 of the packed tile ([Kp/4][32][4]).
template <int NC, int NW>
__device__ __forceinline__ void load_weights(Split3 (&W)[NC][2], const float* wl, const int wave) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float* w = wl + (size_t)(wave + NW * c) * 8 * 128;
        const f32x4 q0 = ld4(w), q1 = ld4(w + 128), q2 = ld4(w + 256), q3 = ld4(w + 384);
        W[c][0] = split8(q0, q1);
        W[c][1] = split8(q2, q3);
    }
}

// acc[mt] = this wave's K slice of W x (clip tile mt).  `xl` = the lane's address within chunk 0 of the state (quad layout
// [Kp/4][64][4]).  The activations are requested in phases of (half of the wave's chunks) x (one 32-clip tile), two phases in
// flight (128 registers next to the 192 of the weights); the schedule is pinned, otherwise the compiler requests the later
// phases one load at a time with a full wait behind each.  `after_first_loads` runs between the first two phases' loads and
// the first multiply: the place for a caller's own load of the step (an unconditional load there keeps the waits counted).
template <int MT, int NC, int NW, typename AfterFirstLoads>
__device__ __forceinline__ void tile_product(f32x16 (&acc)[MT], const Split3 (&W)[NC][2], const float* xl, const int wave,
                                             AfterFirstLoads&& after_first_loads) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    constexpr int HC = (NC + 1) / 2;                                  // chunks per phase
    f32x4 xb[2][HC][4];
    auto load_phase = [&](f32x4 (&buf)[HC][4], const int half, const int mt) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < HC; ++j) {
            const int c = half * HC + j;
            if (c < NC) {
#pragma unroll
                for (int q = 0; q < 4; ++q) buf[j][q] = ld4(xl + (size_t)(wave + NW * c) * 8 * 256 + q * 256 + mt * 128);
            }
        }
    };
    auto mma_phase = [&](const f32x4 (&buf)[HC][4], const int half, f32x16& d) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < HC; ++j) {
            const int c = half * HC + j;
            if (c < NC) {
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) split_mma6(W[c][s2], split8(buf[j][2 * s2], buf[j][2 * s2 + 1]), d);
            }
        }
    };
    load_phase(xb[0], 0, 0);
    load_phase(xb[1], 1, 0);
    after_first_loads();
    __builtin_amdgcn_sched_barrier(0);
    mma_phase(xb[0], 0, acc[0]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (MT == 2) load_phase(xb[0], 0, 1);
    __builtin_amdgcn_sched_barrier(0);
    mma_phase(xb[1], 1, acc[0]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (MT == 2) {
        load_phase(xb[1], 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma_phase(xb[0], 0, acc[1]);
        __builtin_amdgcn_sched_barrier(0);
        mma_phase(xb[1], 1, acc[1]);
    }
}

// The LDS operand of the two helpers below is typed as LDS: through a generic float* the optimizer orders the accesses as
// if they could alias the global loads around them, and the persistent kernels' register allocation moves.
using lds_float = __attribute__((address_space(3))) float;

// red: [wave][32 gate rows][MT * 32 clips + 1]
template <int MT>
__device__ __forceinline__ void spill_tiles(lds_float* red, const f32x16 (&acc)[MT], const int wave, const int lane) {
    constexpr int LDM = MT * 32 + 1;
    const int i = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
            red[(wave * 32 + row) * LDM + mt * 32 + i] = acc[mt][r];
        }
}

// the waves' partial sums of (gate row, clip em), added pairwise in a fixed order
template <int MT, int NW>
__device__ __forceinline__ float sum_waves(const lds_float* red, const int row, const int em) {
    constexpr int LDM = MT * 32 + 1;
    float p = (red[(0 * 32 + row) * LDM + em] + red[(1 * 32 + row) * LDM + em]) +
              (red[(2 * 32 + row) * LDM + em] + red[(3 * 32 + row) * LDM + em]);
    if constexpr (NW == 8)
        p += (red[(4 * 32 + row) * LDM + em] + red[(5 * 32 + row) * LDM + em]) +
             (red[(6 * 32 + row) * LDM + em] + red[(7 * 32 + row) * LDM + em]);
    return p;
}

}  // namespace
