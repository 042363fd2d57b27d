// Packed GEMM of the decode engine with bf16-STORED weights (DecodeEngine(weights_dtype="bf16"); building blocks
// cvc_packed_lstm_bf16w_fwd / cvc_packed_linear_bf16w_fwd of include/cvc_hip_blocks.h).
//
// The weight operand is ONE bf16 term, rounded once when the engine binds the checkpoint; the activations stay fp32 in the quad
// layout XQ[quad][64][4] of gemm_packed.hip (their producers are unchanged) and keep the exact three-way split of gemm_split.h.
// A product w~ * x is w~ * x.lo + w~ * x.mid + w~ * x.hi -- all three cross terms, so it is fp32-grade -- on three
// v_mfma_f32_32x32x16_bf16 instead of the fp32 path's six, with no VALU work on the weights and half their bytes.
//
// Weight layout  Wb[blk][K/8][32 rows][8 k]  (bf16, cvc.decode.pack_weights_bf16): blk = 32 output rows in the row order of the
// fp32 pack (LSTM: the 4 gates x 8 hidden units of workgroup blk).  Lane (i = l & 31, kh = l >> 5) of the wave that handles chunk c
// (32 k) loads k-octets 4c + 2kh + {0, 1} of row i: 16 bytes each, its A operand of one K = 16 MFMA step as stored, 512 contiguous
// bytes per half-wave and instruction.  Octet 4c + 2kh + s holds the k of activation quads 8c + 4kh + 2s and + 2s + 1: W and X
// sit on the same k-slot map as in split8.
//
// Work split: the one of skinny_gemm_packed_kernel's 8-wave split-product form -- chunk c0 + wave + 8 j to wave `wave`, the same
// rotated start chunk, the same ordered cross-wave sum -- and the three MFMAs are issued in the order lo, mid, hi, the order in
// which that kernel issues the three products a bf16-exact weight leaves non-zero (its split is (w~, 0, 0)).  The result is
// therefore bitwise the fp32 kernel's on a pack of the rounded weights, up to the sign of zero (tests/test_gpu_decode_bf16.py).
// The epilogues (LSTM cell update, row-major / K-slice store, per-block top-2 records) are copies of gemm_packed.hip's: that file
// is not touched, so the fp32 kernels cannot move.
#include "cvc_common.h"
#include "gemm_split.h"

namespace {

struct Bf16wArgs {
    const uint16_t* wp;       // packed bf16 weights
    const float* xq;          // packed activations, first quad of this GEMM's K range
    int nquad;                // K / 4 (multiple of 8)
    int M, Nout, R;
    const float* bias;        // linear: [Nout]; lstm: b_ih [4R] (nullable)
    const float* bias2;       // lstm: b_hh (nullable)
    const float* gate_bias;   // lstm: [M, 4R] row-major (nullable)
    const float* emb_gate;    // lstm: [V][4R] table, checkpoint gate order (nullable, with word)
    const int64_t* word;      // lstm: [M]
    const float* c_prev_q;    // lstm: cell state, quad layout [R/4][64][4]
    float* c_out_q;
    float* h_dst1_q;          // lstm: h' in quad layout (quad offset baked into the pointer); nullable
    float* h_dst2_q;
    float* y;                 // linear: row-major [M, ldy] (+ K-slice copies), nullable
    int ldy;
    int ksplit;
    long long split_stride;
    float* top2_part;         // linear: [Nout/32][64][6] records of cvc_top2_final, nullable
    long long wstride;        // bf16 elements between consecutive 32-row blocks of wp
};

template <int MT>
struct BFrag {
    u32x4 w[2];               // 2 x 8 bf16: the lane's A operands of the chunk's two K = 16 steps
    f32x4 x[MT][4];
};

__device__ __forceinline__ float sum_partials8(const float* red, int row, int ldm, int m) {
    float v = (red[(0 * 32 + row) * ldm + m] + red[(1 * 32 + row) * ldm + m]) +
              (red[(2 * 32 + row) * ldm + m] + red[(3 * 32 + row) * ldm + m]);
    v += (red[(4 * 32 + row) * ldm + m] + red[(5 * 32 + row) * ldm + m]) +
         (red[(6 * 32 + row) * ldm + m] + red[(7 * 32 + row) * ldm + m]);
    return v;
}

// WC: the gate weights keep the default cache policy (Infinity-Cache resident by the engine's cache plan) instead of streaming
template <int MT, bool LSTM, int DEPTH, bool WC>
__global__ __launch_bounds__(512) void packed_bf16w_kernel(Bf16wArgs a) {
    constexpr int NW = 8;
    constexpr int LDM = MT * 32 + 1;
    __shared__ float red[NW * 32 * LDM + NW * 64 * 6];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, kh = lane >> 5;
    const int M = a.M, R = a.R;

    int nchunk = a.nquad >> 3, c0 = 0;
    if (!LSTM && a.ksplit > 1) {                              // K slice of this workgroup (whole chunks)
        const int lo = nchunk * (int)blockIdx.y / a.ksplit, hi = nchunk * ((int)blockIdx.y + 1) / a.ksplit;
        c0 = lo;
        nchunk = hi - lo;
    }
    const int n_my = nchunk > wave ? (nchunk - wave + NW - 1) / NW : 0;     // chunks c0 + wave + NW * j
    // per-lane bases: k-octet o of this block lives at wp + blk * wstride + (o * 32 + i) * 8
    const uint16_t* wl = a.wp + (size_t)blockIdx.x * a.wstride + (size_t)i * 8 + (size_t)(c0 + wave) * 4 * 256 + kh * 2 * 256;
    const float* xl = a.xq + (size_t)i * 4 + (size_t)(c0 + wave) * 8 * 256 + kh * 4 * 256;
    constexpr size_t WSTEP = (size_t)NW * 4 * 256, XSTEP = (size_t)NW * 8 * 256;   // bf16 / floats per wave-chunk step
    const int rot = n_my > 0 ? (int)((blockIdx.x * 5) % (unsigned)n_my) : 0;

    auto load = [&](BFrag<MT>& f, int j) __attribute__((always_inline)) {
        // every workgroup walks K from a different starting chunk (see skinny_gemm_packed_kernel)
        int jr = j + rot;
        jr = jr >= n_my ? jr - n_my : jr;
        const uint16_t* w = wl + (size_t)jr * WSTEP;
        const float* x = xl + (size_t)jr * XSTEP;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            if constexpr (LSTM && !WC) f.w[s2] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(w + s2 * 256));
            else f.w[s2] = *reinterpret_cast<const u32x4*>(w + s2 * 256);
#pragma unroll
            for (int q = 2 * s2; q < 2 * s2 + 2; ++q)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) f.x[mt][q] = ld4(x + q * 256 + mt * 128);
        }
    };

    // embedding-gate form: the table row of this thread's epilogue work item, requested before the K loop
    f32x4 eadd4[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    if constexpr (LSTM) {
        if (a.emb_gate != nullptr && tid < 2 * 64) {
            const int em0 = tid & 63;
            const long long eword = a.word[em0 < a.M ? em0 : a.M - 1];
            const float* trow = a.emb_gate + (size_t)eword * 4 * a.R + (size_t)blockIdx.x * 8 + ((tid >> 6) & 1) * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g) eadd4[g] = ld4(trow + (size_t)g * a.R);
        }
    }

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

    auto mma = [&](const BFrag<MT>& f) __attribute__((always_inline)) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const Split3 X = split8(f.x[mt][2 * s2], f.x[mt][2 * s2 + 1]);
                acc[mt] = mfma_bf16(f.w[s2], X.lo, acc[mt]);
                acc[mt] = mfma_bf16(f.w[s2], X.mid, acc[mt]);
                acc[mt] = mfma_bf16(f.w[s2], X.hi, acc[mt]);
            }
        }
    };

    // register ring, DEPTH chunks in flight, fully unrolled; the steady-state loop issues its loads unconditionally
    BFrag<MT> ring[DEPTH];
    if (n_my >= DEPTH) {
#pragma unroll
        for (int s = 0; s < DEPTH - 1; ++s) load(ring[s], s);
        int j = 0;
        for (; j + 2 * DEPTH - 1 <= n_my; j += DEPTH) {
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                load(ring[(s + DEPTH - 1) % DEPTH], j + s + DEPTH - 1);
                mma(ring[s]);
                // 2 + 4 MT loads, 6 MT MFMAs and the activation split (~36 VALU per split8) of one slot, interleaved
#pragma unroll
                for (int g = 0; g < 2 * MT - 2; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x002, 15, 0);   // VALU (operand split + addresses)
                    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);    // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // VMEM read
                }
#pragma unroll
                for (int g = 2 * MT - 2; g < 2 + 4 * MT; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x002, 15, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // drain: chunks j .. n_my-1 (fewer than 2*DEPTH-1 left); slots 0..DEPTH-2 hold chunks j..j+DEPTH-2
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) {
            if (j + s + DEPTH - 1 < n_my) load(ring[(s + DEPTH - 1) % DEPTH], j + s + DEPTH - 1);
            if (j + s < n_my) mma(ring[s]);
        }
#pragma unroll
        for (int s = 0; s < DEPTH - 1; ++s)
            if (j + DEPTH + s < n_my) mma(ring[s]);
    } else {
        for (int j = 0; j < n_my; ++j) {                       // short K: no pipeline
            load(ring[0], j);
            mma(ring[0]);
        }
    }

    // LSTM: the cell update's global operands (one work item per thread: batch row m, 4 hidden units) are requested before the
    // cross-wave LDS stage
    const int em = tid & 63, eqd = (tid >> 6) & 1;
    const bool ework = LSTM && tid < 2 * 64 && em < M && em < MT * 32;
    const int ejq = (int)blockIdx.x * 8 + eqd * 4;                      // first of this thread's 4 hidden units
    const size_t eqoff = ((size_t)(ejq / 4) * 64 + em) * 4;
    f32x4 ecp = {0, 0, 0, 0}, eadd[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    f32x4 eadd2[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, eadd3[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    if (ework) {
        ecp = ld4(a.c_prev_q + eqoff);
        if (a.bias != nullptr) {
#pragma unroll
            for (int g = 0; g < 4; ++g) eadd[g] = ld4(a.bias + g * R + ejq);
        }
        if (a.bias2 != nullptr) {
#pragma unroll
            for (int g = 0; g < 4; ++g) eadd2[g] = ld4(a.bias2 + g * R + ejq);
        }
        if (a.gate_bias != nullptr) {
#pragma unroll
            for (int g = 0; g < 4; ++g) eadd3[g] = ld4(a.gate_bias + (size_t)em * 4 * R + g * R + ejq);
        }
    }

    // linear form with the top-2 epilogue: the biases of the columns this wave scans
    constexpr int ECPW = 32 / NW;
    float ebias[ECPW];
#pragma unroll
    for (int c = 0; c < ECPW; ++c) {
        const int n = (int)blockIdx.x * 32 + wave * ECPW + c;
        ebias[c] = (!LSTM && a.top2_part != nullptr && a.bias != nullptr) ? a.bias[n < a.Nout ? n : a.Nout - 1] : 0.f;
    }

    // ---- ordered cross-wave reduction
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;
            red[(wave * 32 + row) * LDM + mt * 32 + i] = acc[mt][r];
        }
    __syncthreads();

    if constexpr (LSTM) {
        if (ework) {
            f32x4 hv, cv;
#pragma unroll
            for (int g = 0; g < 4; ++g) eadd[g] = ((eadd[g] + eadd2[g]) + eadd3[g]) + eadd4[g];      // (an absent term is an exact zero)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int jj = eqd * 4 + e;
                float pre[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) pre[g] = sum_partials8(red, g * 8 + jj, LDM, em) + eadd[g][e];
                const float ig = fast_sigmoid(pre[0]), fg = fast_sigmoid(pre[1]);
                const float gg = fast_tanh(pre[2]), og = fast_sigmoid(pre[3]);
                const float c2 = fg * ecp[e] + ig * gg;
                cv[e] = c2;
                hv[e] = og * fast_tanh(c2);
            }
            st4(a.c_out_q + eqoff, cv);
            if (a.h_dst1_q != nullptr) st4(a.h_dst1_q + eqoff, hv);
            if (a.h_dst2_q != nullptr) st4(a.h_dst2_q + eqoff, hv);
        }
    } else {
        const int n0 = blockIdx.x * 32;
        const bool lead = blockIdx.y == 0;
        float* y = a.y != nullptr ? a.y + (long long)blockIdx.y * a.split_stride : nullptr;
        if (y != nullptr) {
            for (int u = tid; u < 32 * MT * 32; u += NW * 64) {
                const int nl = u & 31, m = u >> 5;
                const int n = n0 + nl;
                if (m >= M || n >= a.Nout) continue;
                float v = sum_partials8(red, nl, LDM, m);
                if (lead && a.bias != nullptr) v += a.bias[n];
                y[(size_t)m * a.ldy + n] = v;
            }
        }
        if (a.top2_part != nullptr) {
            float* scratch = red + NW * 32 * LDM;
            float v1 = -__builtin_inff(), v2 = -__builtin_inff(), mx = -__builtin_inff(), se = 0.f;
            int i1 = 0x7fffffff, i2 = 0x7fffffff;
            const int m = lane < MT * 32 ? lane : MT * 32 - 1;
#pragma unroll
            for (int c = 0; c < ECPW; ++c) {
                const int nl = wave * ECPW + c, n = n0 + nl;
                if (n >= a.Nout) break;
                const float v = sum_partials8(red, nl, LDM, m) + ebias[c];
                if (v > v1) { v2 = v1; i2 = i1; v1 = v; i1 = n; }
                else if (v > v2) { v2 = v; i2 = n; }
                const float nm = fmaxf(mx, v);
                se = se * __expf(mx - nm) + __expf(v - nm);
                mx = nm;
            }
            float* r4 = scratch + ((size_t)wave * 64 + lane) * 6;
            r4[0] = v1; r4[1] = __int_as_float(i1); r4[2] = v2; r4[3] = __int_as_float(i2); r4[4] = mx; r4[5] = se;
            __syncthreads();
            if (wave == 0 && lane < M) {
                for (int w = 1; w < NW; ++w) {
                    const float* q4 = scratch + ((size_t)w * 64 + lane) * 6;
                    const float u1 = q4[0], u2 = q4[2];
                    const int k1 = __float_as_int(q4[1]), k2 = __float_as_int(q4[3]);
                    if (u1 > v1) { if (v1 >= u2) { v2 = v1; i2 = i1; } else { v2 = u2; i2 = k2; } v1 = u1; i1 = k1; }
                    else if (u1 > v2) { v2 = u1; i2 = k1; }
                    const float nm = fmaxf(mx, q4[4]);
                    se = (nm == -__builtin_inff()) ? 0.f : se * __expf(mx - nm) + q4[5] * __expf(q4[4] - nm);
                    mx = nm;
                }
                float* rec = a.top2_part + ((size_t)blockIdx.x * 64 + lane) * 6;
                rec[0] = v1; rec[1] = __int_as_float(i1); rec[2] = v2; rec[3] = __int_as_float(i2); rec[4] = mx; rec[5] = se;
            }
        }
    }
}

#ifndef CVC_BF16W_DEPTH
#define CVC_BF16W_DEPTH 4       // chunks in flight per wave: 2 KB of weights + 4 / 8 KB of activations each (M <= 32 / 64 rows)
#endif

template <bool LSTM>
int launch_bf16w(Bf16wArgs a, int blocks, bool w_cached, hipStream_t st) {
    if (a.wstride == 0) a.wstride = (long long)a.nquad * 4 * 32;
    const dim3 grid(blocks, LSTM || a.ksplit < 1 ? 1 : a.ksplit);
    if (LSTM && w_cached) {
        if (a.M <= 32) hipLaunchKernelGGL((packed_bf16w_kernel<1, LSTM, CVC_BF16W_DEPTH, true>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((packed_bf16w_kernel<2, LSTM, CVC_BF16W_DEPTH, true>), grid, dim3(512), 0, st, a);
    } else {
        if (a.M <= 32) hipLaunchKernelGGL((packed_bf16w_kernel<1, LSTM, CVC_BF16W_DEPTH, false>), grid, dim3(512), 0, st, a);
        else hipLaunchKernelGGL((packed_bf16w_kernel<2, LSTM, CVC_BF16W_DEPTH, false>), grid, dim3(512), 0, st, a);
    }
    return cvc_launch_status();
}

}  // namespace

extern "C" int cvc_packed_lstm_bf16w_fwd(const uint16_t* wp, long long w_blk_stride, const float* xq, int K, const float* b_ih,
                                         const float* b_hh, const float* gate_bias, const float* emb_gate, const int64_t* word,
                                         const float* c_prev_q, int M, int R, float* h_dst1_q, float* h_dst2_q, float* c_out_q,
                                         int w_cached, cvc_stream_t stream) {
    if (!wp || !xq || !c_prev_q || !c_out_q || (K & 31) || K < 32 || R < 8 || (R & 7) || M < 1 || M > 64) return CVC_E_BADARG;
    if ((emb_gate != nullptr) != (word != nullptr)) return CVC_E_BADARG;
    if (w_blk_stride != 0 && (w_blk_stride < (long long)K * 32 || (w_blk_stride & 7))) return CVC_E_BADARG;
    if (((uintptr_t)wp & 15) || ((uintptr_t)xq & 15)) return CVC_E_BADARG;
    Bf16wArgs a{};
    a.wp = wp; a.xq = xq; a.nquad = K / 4; a.M = M; a.Nout = 4 * R; a.R = R; a.wstride = w_blk_stride;
    a.bias = b_ih; a.bias2 = b_hh; a.gate_bias = gate_bias; a.emb_gate = emb_gate; a.word = word;
    a.c_prev_q = c_prev_q; a.c_out_q = c_out_q; a.h_dst1_q = h_dst1_q; a.h_dst2_q = h_dst2_q; a.ksplit = 1;
    return launch_bf16w<true>(a, R / 8, w_cached != 0, (hipStream_t)stream);
}

extern "C" int cvc_packed_linear_bf16w_fwd(const uint16_t* wp, const float* xq, int K, const float* bias, int M, int Nout,
                                           int ksplit, float* y, int ldy, float* top2_part, cvc_stream_t stream) {
    if (!wp || !xq || (K & 31) || K < 32 || Nout < 1 || ksplit < 1 || (!y && !top2_part) || M < 1 || M > 64) return CVC_E_BADARG;
    if (ksplit > 1 && top2_part != nullptr) return CVC_E_BADARG;
    if (y != nullptr && ldy < Nout) return CVC_E_BADARG;
    if (((uintptr_t)wp & 15) || ((uintptr_t)xq & 15)) return CVC_E_BADARG;
    Bf16wArgs a{};
    a.wp = wp; a.xq = xq; a.nquad = K / 4; a.M = M; a.Nout = Nout; a.R = 0;
    a.bias = bias; a.y = y; a.ldy = ldy; a.ksplit = ksplit; a.split_stride = (long long)M * ldy; a.top2_part = top2_part;
    return launch_bf16w<false>(a, (Nout + 31) / 32, false, (hipStream_t)stream);
}
