// Persistent form of the GRU backward recurrence (cvc_gru_seq_bwd launches three kernels per time step; 70 of the 93 ms of a
// config-2 forward + backward are those 1 440 launches per layer).  One launch per layer (recurrence_sync.h), built like the
// forward (gru_persistent.hip): a workgroup owns 8 hidden units of one direction for all F steps.
//   per step s (the forward direction walks t = F-1 .. 0, the reverse direction t = 0 .. F-1):
//     1. wait until every workgroup of the direction has published dgh of step s - 1 (spread arrival counters);
//     2. dh_mm[m, j] = sum_k dgh_{s-1}[m, k] W_hh[k, j] for its 8 units j: the 3H x 8 weight columns live in registers as split
//        bf16 terms (A operand of v_mfma_f32_16x16x32_bf16: 8 units + 8 zero rows), dgh_{s-1} of ALL units is read from its
//        exchange slot ([3H/8][64 clips][8], written once, read after the barrier: no cache can hold a stale copy), 8 waves split K;
//     3. thread (clip m, unit j): dh = dY_t + z-carried part (a register) + dh_mm; gate gradients; dgi_t, dgh_t rows to global
//        memory (the dense dW / dX products of the host side read them), dgh_t of the own units to the step's exchange slot
//        with write-through stores; arrival.
#include "cvc_common.h"
#include "gemm_split.h"
#include "recurrence_sync.h"

namespace {

constexpr int SYNC_GROUPS = 2;                    // arrival counter groups (recurrence_sync.h): one per direction

struct GruBArgs {
    const float* wt;                              // W_hh^T packed [ndir][H/8][3H/8][8 units][8 k]
    const float* dy; long long dy_ld_m, dy_ld_t;  // dL/dh rows: (m, t) at + m * ld_m + t * ld_t, columns [ndir][H]
    const float* gates; long long g_ld_m, g_ld_t; // (r, z, n, hn): columns [ndir][4][H]
    const float* y; long long y_ld_m, y_ld_t;     // forward outputs h_t: columns [ndir][H]
    float* dgi; float* dgh;                       // [F * M rows (t * M + m), ndir * 3H]
    float* slots;                                 // exchange: [F][ndir][3H/8][64][8]
    unsigned* sync;
    int M, F, H;
    unsigned spin_limit;
};

using f32x4v = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f32x4v mfma16(const u32x4 a, const u32x4 b, const f32x4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// split_mma6 (gemm_split.h) on a 16x16x32 tile
__device__ __forceinline__ void split_mma6_16(const Split3& W, const Split3& X, f32x4v& d) {
    d = mfma16(W.mid, X.mid, d);
    d = mfma16(W.lo, X.hi, d);
    d = mfma16(W.hi, X.lo, d);
    d = mfma16(W.mid, X.hi, d);
    d = mfma16(W.hi, X.mid, d);
    d = mfma16(W.hi, X.hi, d);
}

// NKS = 32-k steps per wave: 3H = 256 * NKS
template <int NKS>
__global__ __launch_bounds__(512, 1) void gru_bwd_persistent_kernel(GruBArgs a) {
    __shared__ float red[8][8][64];               // [wave][unit][clip]
    __shared__ int gave_up;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int dir = blockIdx.y, blk = blockIdx.x, ndir = gridDim.y, H = a.H, M = a.M, F = a.F;
    const int K = 3 * H, ngrp = K >> 3;
    const unsigned nblk = gridDim.x;
    unsigned* counter = counter_group(a.sync, dir);

    // ---- weights: lane (row r = lane & 15, k group = lane >> 4) of k step ks holds 8 consecutive k of unit r (rows 8..15 zero)
    const int wr = lane & 15, wg = lane >> 4;
    Split3 W[NKS];
    {
        const float* wl = a.wt + ((size_t)dir * (H / 8) + blk) * (size_t)ngrp * 64;
#pragma unroll
        for (int j = 0; j < NKS; ++j) {
            const int ks = wave + 8 * j;
            f32x4 q0 = {0, 0, 0, 0}, q1 = {0, 0, 0, 0};
            if (wr < 8) {
                const float* p = wl + ((size_t)(ks * 4 + wg) * 8 + wr) * 8;
                q0 = ld4(p); q1 = ld4(p + 4);
            }
            W[j] = split8(q0, q1);
        }
    }

    // ---- elementwise role: thread <-> (clip em, unit ej of this block), fixed for the whole sequence
    const int em = tid >> 3, ejr = tid & 7;
    const int ej = blk * 8 + ejr;
    const bool ework = em < M;
    float dh_part = 0.f;                           // dh z of the previous processed step (own unit): never leaves the thread
    const long long row_ld = (long long)ndir * 3 * H;

    if (tid == 0) gave_up = 0;
    __syncthreads();
    for (int s = 0; s < F; ++s) {
        const long long t = dir == 0 ? F - 1 - s : s;
        const long long tp = dir == 0 ? t - 1 : t + 1;
        // operands of the gate arithmetic: independent of the other workgroups, requested before the wait
        float dyv = 0.f, rg = 0.f, zg = 0.f, ng = 0.f, hn = 0.f, hp = 0.f;
        if (ework) {
            dyv = a.dy[(size_t)em * a.dy_ld_m + t * a.dy_ld_t + (size_t)dir * H + ej];
            const float* gp = a.gates + (size_t)em * a.g_ld_m + t * a.g_ld_t + (size_t)dir * 4 * H + ej;
            rg = gp[0]; zg = gp[H]; ng = gp[2 * H]; hn = gp[3 * H];
            if (tp >= 0 && tp < F) hp = a.y[(size_t)em * a.y_ld_m + tp * a.y_ld_t + (size_t)dir * H + ej];
        }
        float dh_mm = 0.f;
        if (s > 0) {
            // ---- wait for dgh of step s - 1
            if (wave == 0 && wait_arrivals(a.sync, counter, nblk * (unsigned)s, a.spin_limit, lane) && lane == 0)
                gave_up = 1;                              // tell the workgroup
            __syncthreads();
            if (gave_up) return;
            // ---- dh_mm = dgh_{s-1} W_hh[:, own units]: this wave's k steps, 4 tiles of 16 clips
            const float* X = a.slots + ((size_t)(s - 1) * ndir + dir) * (size_t)ngrp * 512 + ((size_t)wg * 64 + (lane & 15)) * 8;
            f32x4v acc[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4v{0, 0, 0, 0};
            // phases of (k step, two clip tiles), two in flight: 32 registers next to the 144 of the weights
            f32x4 xb[2][2][2];
            auto loadx = [&](f32x4 (&buf)[2][2], const int ph) __attribute__((always_inline)) {
                const float* p = X + (size_t)(wave + 8 * (ph >> 1)) * 4 * 512 + (ph & 1) * 256;
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) { buf[c2][0] = ld4(p + c2 * 128); buf[c2][1] = ld4(p + c2 * 128 + 4); }
            };
            loadx(xb[0], 0);
#pragma unroll
            for (int ph = 0; ph < 2 * NKS; ++ph) {
                if (ph + 1 < 2 * NKS) loadx(xb[(ph + 1) & 1], ph + 1);
                __builtin_amdgcn_sched_barrier(0);
                const int j = ph >> 1;
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    split_mma6_16(W[j], split8(xb[ph & 1][c2][0], xb[ph & 1][c2][1]), acc[(ph & 1) * 2 + c2]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // D[unit = 4 * (lane >> 4) + r][clip = ct * 16 + (lane & 15)]: units 0..7 live in lanes 0..31
            if (wg < 2) {
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[wave][4 * wg + r][ct * 16 + (lane & 15)] = acc[ct][r];
            }
            __syncthreads();
            dh_mm = ((red[0][ejr][em] + red[1][ejr][em]) + (red[2][ejr][em] + red[3][ejr][em])) +
                    ((red[4][ejr][em] + red[5][ejr][em]) + (red[6][ejr][em] + red[7][ejr][em]));
        }
        // ---- gate gradients of step s for (clip em, unit ej)
        if (ework) {
            const float dh = (dyv + dh_part) + dh_mm;
            const float dn = dh * (1.f - zg) * (1.f - ng * ng);
            const float dz = dh * (hp - ng) * zg * (1.f - zg);
            const float dr = dn * hn * rg * (1.f - rg);
            const float dnr = dn * rg;
            dh_part = dh * zg;
            float* gi = a.dgi + (size_t)(t * M + em) * row_ld + (size_t)dir * 3 * H + ej;
            gi[0] = dr; gi[H] = dz; gi[2 * H] = dn;
            float* gh = a.dgh + (size_t)(t * M + em) * row_ld + (size_t)dir * 3 * H + ej;
            gh[0] = dr; gh[H] = dz; gh[2 * H] = dnr;
            if (s + 1 < F) {
                // own units of the exchange slot: group (g H + 8 blk) / 8 of gate g, element (clip, unit); straight to memory
                float* sl = a.slots + ((size_t)s * ndir + dir) * (size_t)ngrp * 512 + ((size_t)blk * 64 + em) * 8 + ejr;
                const size_t gs = (size_t)(H / 8) * 512;
                store_through1(sl, dr);
                store_through1(sl + gs, dz);
                store_through1(sl + 2 * gs, dnr);
            }
        }
        if (s + 1 < F) {
            drain_stores();
            __syncthreads();                              // every wave's slot stores are acknowledged; `red` may be rewritten
            if (tid == 0) arrive(counter, blk);
        }
    }
}

}  // namespace

extern "C" int cvc_gru_bwd_persistent_sync_words(void) { return (int)sync_words(SYNC_GROUPS); }

// Same inputs and outputs as cvc_gru_seq_bwd except: wt = W_hh^T packed [ndir][H/8][3H/8][8][8] (cvc.gru.pack_gru_weights_t),
// slots = F * ndir * 3H * 64 floats of exchange memory, sync = cvc_gru_bwd_persistent_sync_words() words (word 4 non-zero
// afterwards = barrier time-out, outputs invalid: use cvc_gru_seq_bwd).  H % 256 == 0, H <= 1024, M <= 64; CVC_E_BADARG
// without launching otherwise.
extern "C" int cvc_gru_seq_bwd_persistent(const float* dy, long long dy_ld_m, long long dy_ld_t, const float* gates, long long g_ld_m,
                                          long long g_ld_t, const float* y, long long y_ld_m, long long y_ld_t, const float* wt,
                                          int M, int F, int H, int ndir, float* dgi, float* dgh, float* slots, unsigned* sync,
                                          cvc_stream_t stream) {
    if (!dy || !gates || !y || !wt || !dgi || !dgh || !slots || !sync || M < 1 || M > 64 || F < 1 || H < 256 || (H & 255) ||
        H > 1024 || ndir < 1 || ndir > 2)
        return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    GruBArgs a{};
    a.wt = wt; a.dy = dy; a.dy_ld_m = dy_ld_m; a.dy_ld_t = dy_ld_t; a.gates = gates; a.g_ld_m = g_ld_m; a.g_ld_t = g_ld_t;
    a.y = y; a.y_ld_m = y_ld_m; a.y_ld_t = y_ld_t; a.dgi = dgi; a.dgh = dgh; a.slots = slots; a.sync = sync;
    a.M = M; a.F = F; a.H = H; a.spin_limit = 1u << 20;
#define CVC_GRU_B(NKS_) \
    return launch_resident(gru_bwd_persistent_kernel<NKS_>, dim3(H / 8, ndir), 512, a, nullptr, 0, sync, SYNC_GROUPS, st)
    switch (3 * H / 256) {
        case 3: CVC_GRU_B(3);
        case 6: CVC_GRU_B(6);
        case 9: CVC_GRU_B(9);
        case 12: CVC_GRU_B(12);
        default: return CVC_E_BADARG;
    }
#undef CVC_GRU_B
}
