// What the kernels that give a row (or a slice of an elementwise range) to one workgroup of WG threads share, once: the workgroup
// size, the sum / max over its four waves, and the order in which two (value, index) candidates rank.  Used by the vocabulary head
// (csrc/vocab.hip), the beam blocks (csrc/beam.hip), the training step's pointwise kernels (csrc/lstm_pointwise_bwd.hip) and, through
// csrc/select_row.h, every word-selection block.
#pragma once
#include "cvc_common.h"

namespace {

constexpr int WG = 256;

__device__ __forceinline__ float block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ float block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// candidate a ranks before candidate b: the larger value, ties -> the lower index
// (bitwise, not short-circuit: three compares and two mask operations instead of branches)
__device__ __forceinline__ bool better(float va, int ia, float vb, int ib) { return (va > vb) | ((va == vb) & (ia < ib)); }

}  // namespace
