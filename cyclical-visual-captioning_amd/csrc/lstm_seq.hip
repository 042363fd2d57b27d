// LSTM recurrence of the encoder's frame context in its `bilstm` mode (reference backbone.py:94-106 builds
// nn.LSTM(R, R/2, 2, dropout=0.2, bidirectional=True, batch_first=True); :335-338 runs it over the F sampled frames):
//     z = W_ih x + b_ih + W_hh h + b_hh          gate order i, f, g, o;  h0 = c0 = 0
//     c' = sig(f) c + sig(i) tanh(g),   h' = sig(o) tanh(c')
// The input projections of all steps and both directions are one dense product on the tile GEMM (cvc/lstm_seq.py); this file is
// the recurrence, in the two forms the GRU has (gru_persistent.hip, gemm_packed.hip) plus the walk backwards:
//   * persistent (cvc_lstm_seq_persistent_fwd / _train_fwd; H % 128 == 0, H <= 1024, M <= 64): ONE launch for the whole sequence.
//     A workgroup owns 8 hidden units of one direction for all F steps: 32 rows of W_hh (4 gates x 8 units -- the packed gate
//     tile of cvc/decode/weights.py::pack_weights, with no zero rows where the GRU pads its fourth gate), held in registers as the
//     three bf16 terms of the split product (gemm_split.h).  Per step it reads the direction's previous h from that step's own
//     slot ([F + 1][ndir][H/4][64][4]: an address is written once, before the arrival, and first read after it, so no cache holds a
//     stale copy and nobody invalidates), multiplies on v_mfma_f32_32x32x16_bf16 with the six cross terms, sums the waves' partial
//     tiles through LDS in a fixed order and applies the cell arithmetic.  THE CELL STATE NEVER LEAVES THE WORKGROUP: an epilogue
//     thread keeps the c of its (clip, 4 units) in registers across the steps -- where the GRU reads its previous h back from the
//     slot for the z blend, the LSTM's epilogue has no global operand that another step wrote.  Steps are separated by
//     per-direction arrival counters; the state stores are write-through (sc0 sc1) and drained before the arrival; every spin is
//     bounded and ends in the error word (sync word 4) instead of a hung GPU.
//   * per step (cvc_lstm_seq_fwd / _train_fwd; any H % 8 == 0, M <= 64): F launches from one C call, W_hh re-read every step, h
//     and c exchanged through a small workspace.  Same packed tile, same split product, same cell arithmetic as the LSTM form of
//     the packed gate-GEMM kernel (gemm_packed.hip), with the strided row operands of a sequence (that kernel's row operands have
//     the fixed strides of the decode step).  The fallback when the persistent form refuses a shape or reports a time-out, and the
//     only form for config 5's width (H = 2048).  The two forms sum k in different orders: equal within rounding, not in bits.
//   * backward (cvc_lstm_seq_bwd): per step and direction the gate gradients (the arithmetic of cvc_lstm_pointwise_bwd4:
//     dh = dY_t + carried dh, dc carried through f) and dgates_t W_hh on the backward-data kernel (cvc_linear_nn_planes_fwd), as
//     cvc_gru_seq_bwd does.  b_ih and b_hh enter the same sum, so ONE dG serves the input-side and the hidden-side products.
#include "cvc_common.h"
#include "recurrence_sync.h"
#include "recurrence_tile.h"

namespace {

constexpr int SYNC_GROUPS = 2;                    // arrival counter groups (recurrence_sync.h): one per direction

struct LstmArgs {
    const float* wp; long long w_stride;          // packed W_hh [ndir][H/8][Kp/4][32][4]
    const float* gi; long long gi_ld_m, gi_ld_t;  // input projections (no bias), columns [ndir][4H]
    const float* b_ih; const float* b_hh;         // [ndir][4H]
    int M, F, H, Kp;
    float* hq; long long h_stride;                // persistent: state slots [F + 1][ndir][Kp/4][64][4], slot 0 = h0
    float* y; long long y_ld_m, y_ld_t;
    float* gates; long long g_ld_m, g_ld_t;       // training: activated (i, f, g, o) of every step, columns [ndir][4][H]; nullable
    float* c; long long c_ld_m, c_ld_t;           // training: c_t of every step, columns [ndir][H]; nullable
    unsigned* sync;                               // sync_words(SYNC_GROUPS) words: error word + arrival counters
    unsigned spin_limit;
    // per-step form: this step's operands
    const float* h_in; float* h_out; float* c_q;  // quad layout [ndir][Kp/4][64][4] each
    long long t_of[2];                            // the time index direction d works on
};

// the cell of one (clip, 4 hidden units): pre-activations `pre` (i, f, g, o) -> c (updated in place), h, activated gates
__device__ __forceinline__ void lstm_cell4(const f32x4 (&pre)[4], f32x4& c, f32x4& h, f32x4 (&act)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ig = fast_sigmoid(pre[0][e]), fg = fast_sigmoid(pre[1][e]);
        const float gg = fast_tanh(pre[2][e]), og = fast_sigmoid(pre[3][e]);
        const float c2 = fg * c[e] + ig * gg;
        c[e] = c2;
        h[e] = og * fast_tanh(c2);
        act[0][e] = ig; act[1][e] = fg; act[2][e] = gg; act[3][e] = og;
    }
}

// NC = 32-k chunks per wave (K = 32 * NW * NC), MT = 32-clip tiles, NW = 4 waves (K / 4 each) or 8 (K / 8 each).
template <int MT, int NC, int NW>
__global__ __launch_bounds__(NW * 64, 1) void lstm_persistent_kernel(LstmArgs a) {
    constexpr int LDM = MT * 32 + 1;
    __shared__ float red[NW * 32 * LDM];
    __shared__ float sbias[32];
    __shared__ float sgi[32 * LDM];                                    // this step's x-projections + bias, [gate row][clip]
    __shared__ int gave_up;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, kh = lane >> 5;
    const int dir = blockIdx.y, blk = blockIdx.x, H = a.H, M = a.M;
    const int nquad = a.Kp >> 2;
    const unsigned nblk = gridDim.x;

    // ---- this wave's share of the weights (chunks wave, wave + NW, ...), split once
    Split3 W[NC][2];
    load_weights<NC, NW>(W, a.wp + (size_t)dir * a.w_stride + ((size_t)blk * nquad * 32 + i) * 4 + kh * 4 * 128, wave);

    // ---- epilogue role: thread (em = clip, eqd = which 4 of the 8 hidden units); its cell state lives in `ecell` for all steps
    constexpr int ET = MT * 32, NT = NW * 64, NGI = (ET * 8 + NT - 1) / NT;
    const int em = tid % ET, eqd = tid / ET;
    const int ejq = blk * 8 + (eqd & 1) * 4;
    const bool ework = eqd < 2 && em < M;
    const size_t eqoff = ((size_t)(ejq / 4) * 64 + em) * 4;
    f32x4 ecell = {0, 0, 0, 0};                                        // c0 = 0
    // b_ih + b_hh of the workgroup's 32 gate rows: in LDS, not in 16 registers per lane next to the weights
    if (tid < 32) {
        const size_t col = (size_t)dir * 4 * H + (size_t)(tid >> 3) * H + blk * 8 + (tid & 7);
        sbias[tid] = a.b_ih[col] + a.b_hh[col];
    }
    unsigned* counter = counter_group(a.sync, dir);

    if (tid == 0) gave_up = 0;
    __syncthreads();
    for (int s = 0; s < a.F; ++s) {
        const long long t = dir == 0 ? s : a.F - 1 - s;
        const float* hprev = a.hq + ((size_t)s * gridDim.y + dir) * a.h_stride;
        float* hnext = a.hq + ((size_t)(s + 1) * gridDim.y + dir) * a.h_stride;

        // x-projections of this step: independent of the other workgroups, requested before the wait
        // (ALL threads share the ET x 32 values, one or two float4 each, and pass them through LDS: four float4 held by the
        // epilogue threads alone would be 16 registers per lane next to the weights)
        f32x4 egi[NGI];
#pragma unroll
        for (int k = 0; k < NGI; ++k) {
            const int it = tid + k * NT, gm = it % ET, gq = it / ET;       // item = (clip gm, gate gq >> 1, quad gq & 1)
            egi[k] = f32x4{0, 0, 0, 0};
            if (it < ET * 8 && gm < M)
                egi[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(
                    a.gi + (size_t)gm * a.gi_ld_m + t * a.gi_ld_t + (size_t)dir * 4 * H + (size_t)(gq >> 1) * H + blk * 8 + (gq & 1) * 4));
        }

        // ---- wait until every workgroup of this direction has published step s - 1
        if (s > 0) {
            if (wave == 0 && wait_arrivals(a.sync, counter, nblk * (unsigned)s, a.spin_limit, lane) && lane == 0)
                gave_up = 1;                                           // tell the workgroup
            __syncthreads();                                           // (also: the previous step's readers of `red` are done)
            if (gave_up) return;                                       // no invalidate: slot s has never been read before
        }

        // ---- partial tiles: this wave's K slice of the clip tiles
        f32x16 acc[MT];
        tile_product<MT, NC, NW>(acc, W, hprev + (size_t)i * 4 + kh * 4 * 256, wave, [] {});

        // ---- ordered cross-wave sum, cell arithmetic
        spill_tiles<MT>((lds_float*)red, acc, wave, lane);
#pragma unroll
        for (int k = 0; k < NGI; ++k) {
            const int it = tid + k * NT, gm = it % ET, gq = it / ET;
            if (it < ET * 8) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sgi[(gq * 4 + e) * LDM + gm] = egi[k][e] + sbias[gq * 4 + e];
            }
        }
        __syncthreads();
        if (ework) {
            f32x4 pre[4], hv, act[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = g * 8 + eqd * 4 + e;
                    pre[g][e] = sum_waves<MT, NW>((const lds_float*)red, row, em) + sgi[row * LDM + em];
                }
            lstm_cell4(pre, ecell, hv, act);
            if (a.gates != nullptr) {
                float* gp = a.gates + (size_t)em * a.g_ld_m + t * a.g_ld_t + (size_t)dir * 4 * H + ejq;
#pragma unroll
                for (int g = 0; g < 4; ++g) st4(gp + g * H, act[g]);
                st4(a.c + (size_t)em * a.c_ld_m + t * a.c_ld_t + (size_t)dir * H + ejq, ecell);
            }
            store_through4(hnext + eqoff, hv);
            st4(a.y + (size_t)em * a.y_ld_m + t * a.y_ld_t + (size_t)dir * H + ejq, hv);
            drain_stores();
        }
        // ---- publish: one arrival per workgroup, after all of its state stores have been acknowledged
        __syncthreads();
        if (tid == 0) arrive(counter, blk);
    }
}

// ---- per-step form: one launch per time step, grid (H / 8, ndir), 4 waves splitting K chunk by chunk (wave, wave + 4, ...)
template <int MT>
__global__ __launch_bounds__(256) void lstm_step_kernel(LstmArgs a) {
    constexpr int LDM = MT * 32 + 1, NW = 4;
    __shared__ float red[NW * 32 * LDM];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, kh = lane >> 5;
    const int dir = blockIdx.y, blk = blockIdx.x, H = a.H, M = a.M;
    const int nquad = a.Kp >> 2, nchunk = a.Kp >> 5;
    const long long t = dir == 0 ? a.t_of[0] : a.t_of[1];
    const float* hprev = a.h_in + (size_t)dir * a.h_stride;

    constexpr int ET = MT * 32;
    const int em = tid % ET, eqd = tid / ET;
    const int ejq = blk * 8 + (eqd & 1) * 4;
    const bool ework = eqd < 2 && em < M;
    const size_t eqoff = ((size_t)(ejq / 4) * 64 + em) * 4;
    f32x4 pre[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}}, ecell = {0, 0, 0, 0};
    float* cq = a.c_q + (size_t)dir * a.h_stride + eqoff;
    if (ework) {
        const float* gi = a.gi + (size_t)em * a.gi_ld_m + t * a.gi_ld_t + (size_t)dir * 4 * H + ejq;
        const float* bi = a.b_ih + (size_t)dir * 4 * H + ejq;
        const float* bh = a.b_hh + (size_t)dir * 4 * H + ejq;
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g] = ld4(gi + g * H) + (ld4(bi + g * H) + ld4(bh + g * H));
        ecell = ld4(cq);
    }

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    const float* wl = a.wp + (size_t)dir * a.w_stride + ((size_t)blk * nquad * 32 + i) * 4 + kh * 4 * 128;
    const float* xl = hprev + (size_t)i * 4 + kh * 4 * 256;
    for (int c = wave; c < nchunk; c += NW) {
        const float* w = wl + (size_t)c * 8 * 128;
        const f32x4 w0 = ld4(w), w1 = ld4(w + 128), w2 = ld4(w + 256), w3 = ld4(w + 384);
        const Split3 Ws[2] = {split8(w0, w1), split8(w2, w3)};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const float* x = xl + (size_t)c * 8 * 256 + mt * 128;
            const f32x4 x0 = ld4(x), x1 = ld4(x + 256), x2 = ld4(x + 512), x3 = ld4(x + 768);
            const Split3 Xs[2] = {split8(x0, x1), split8(x2, x3)};
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) split_mma6(Ws[s2], Xs[s2], acc[mt]);
        }
    }
    spill_tiles<MT>((lds_float*)red, acc, wave, lane);
    __syncthreads();
    if (ework) {
        f32x4 hv, act[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) pre[g][e] += sum_waves<MT, NW>((const lds_float*)red, g * 8 + eqd * 4 + e, em);
        lstm_cell4(pre, ecell, hv, act);
        st4(cq, ecell);
        st4(a.h_out + (size_t)dir * a.h_stride + eqoff, hv);
        st4(a.y + (size_t)em * a.y_ld_m + t * a.y_ld_t + (size_t)dir * H + ejq, hv);
        if (a.gates != nullptr) {
            float* gp = a.gates + (size_t)em * a.g_ld_m + t * a.g_ld_t + (size_t)dir * 4 * H + ejq;
#pragma unroll
            for (int g = 0; g < 4; ++g) st4(gp + g * H, act[g]);
            st4(a.c + (size_t)em * a.c_ld_m + t * a.c_ld_t + (size_t)dir * H + ejq, ecell);
        }
    }
}

// ---- backward: the gate gradients of one step, both directions in one launch (blockIdx.y)
struct LstmStepBwd {
    const float* dy; long long dy_ld;          // dL/dh_t rows (row m at + m * dy_ld), H columns of this direction
    const float* dh_planes; int nplanes;       // dgates W_hh of the previously processed step as K-slice planes, nullable
    long long plane_stride, plane_ld;
    const float* gates; long long g_ld;        // activated (i, f, g, o) of this step: row m at + m * g_ld, columns [4][H]
    const float* c; long long c_ld;            // c_t rows
    const float* c_prev;                       // c_{t-1} rows (stride c_ld), nullable (= 0)
    float* dc;                                 // [M, H] carried dL/dc (read unless first, written), own element per thread
    int first;
    float* dg; long long dg_ld;                // [M, 4H] at + m * dg_ld
    float* dg_q;                               // [4H/4][64][4]
    int M, H;
};
struct LstmStepBwd2 { LstmStepBwd d[2]; };

__global__ __launch_bounds__(256) void lstm_pointwise_bwd_kernel(LstmStepBwd2 both) {
    const LstmStepBwd& a = both.d[blockIdx.y];
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int m = t & 63, jq = t >> 6;                         // batch row fastest: the quad-layout stores are contiguous
    const int j = jq * 4;
    if (j >= a.H) return;
    const int H = a.H;
    if (m >= a.M) {                                             // rows beyond M of the quad operand must be zero
#pragma unroll
        for (int g = 0; g < 4; ++g) st4(a.dg_q + ((size_t)((g * H + j) >> 2) * 64 + m) * 4, f32x4{0, 0, 0, 0});
        return;
    }
    f32x4 dh = ld4(a.dy + (size_t)m * a.dy_ld + j);
    if (a.dh_planes != nullptr) {
        const float* pl = a.dh_planes + (size_t)m * a.plane_ld + j;
        f32x4 acc = ld4(pl);
        for (int k = 1; k < a.nplanes; ++k) acc += ld4(pl + (size_t)k * a.plane_stride);
        dh += acc;
    }
    const float* gp = a.gates + (size_t)m * a.g_ld + j;
    const f32x4 ig = ld4(gp), fg = ld4(gp + H), gg = ld4(gp + 2 * H), og = ld4(gp + 3 * H);
    const f32x4 cv = ld4(a.c + (size_t)m * a.c_ld + j);
    const f32x4 cp = a.c_prev != nullptr ? ld4(a.c_prev + (size_t)m * a.c_ld + j) : f32x4{0, 0, 0, 0};
    f32x4 tc;
#pragma unroll
    for (int e = 0; e < 4; ++e) tc[e] = fast_tanh(cv[e]);
    f32x4 dc = dh * og * (1.f - tc * tc);
    if (!a.first) dc += ld4(a.dc + (size_t)m * H + j);        // carried through f of the step processed before
    const f32x4 d_o = dh * tc * og * (1.f - og);
    const f32x4 d_i = dc * gg * ig * (1.f - ig);
    const f32x4 d_f = dc * cp * fg * (1.f - fg);
    const f32x4 d_g = dc * ig * (1.f - gg * gg);
    st4(a.dc + (size_t)m * H + j, dc * fg);
    float* o = a.dg + (size_t)m * a.dg_ld + j;
    st4(o, d_i); st4(o + H, d_f); st4(o + 2 * H, d_g); st4(o + 3 * H, d_o);
    st4(a.dg_q + ((size_t)((0 * H + j) >> 2) * 64 + m) * 4, d_i);
    st4(a.dg_q + ((size_t)((1 * H + j) >> 2) * 64 + m) * 4, d_f);
    st4(a.dg_q + ((size_t)((2 * H + j) >> 2) * 64 + m) * 4, d_g);
    st4(a.dg_q + ((size_t)((3 * H + j) >> 2) * 64 + m) * 4, d_o);
}

int bwd_ksplit(int H) {
    const int slabs = (H + 127) / 128;
    int ks = 256 / slabs;
    const int kmax = 4 * H / 8 / 16;       // >= 16 rows per wave and slice (the launch is latency-bound and wants the whole chip)
    if (ks > kmax) ks = kmax;
    return ks < 1 ? 1 : ks;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int fill_common(LstmArgs& a, const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih, const float* b_hh,
                int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m, long long y_ld_t, float* gates, long long g_ld_m,
                long long g_ld_t, float* c, long long c_ld_m, long long c_ld_t, bool train) {
    if (!wp || !gi || !b_ih || !b_hh || !hq || !y || M < 1 || M > 64 || F < 1 || H < 8 || (H & 7) || ndir < 1 || ndir > 2 ||
        (gi_ld_m & 3) || (gi_ld_t & 3) || (y_ld_m & 3) || (y_ld_t & 3) || !aligned16(wp) || !aligned16(gi) || !aligned16(b_ih) ||
        !aligned16(b_hh) || !aligned16(hq) || !aligned16(y))
        return CVC_E_BADARG;
    if (train && (!gates || !c || (g_ld_m & 3) || (g_ld_t & 3) || (c_ld_m & 3) || (c_ld_t & 3) || !aligned16(gates) || !aligned16(c)))
        return CVC_E_BADARG;
    const int Kp = (H + 31) / 32 * 32;
    a.wp = wp; a.w_stride = (long long)(H / 8) * (Kp / 4) * 128;
    a.gi = gi; a.gi_ld_m = gi_ld_m; a.gi_ld_t = gi_ld_t; a.b_ih = b_ih; a.b_hh = b_hh;
    a.M = M; a.F = F; a.H = H; a.Kp = Kp; a.hq = hq; a.h_stride = (long long)Kp * 64;
    a.y = y; a.y_ld_m = y_ld_m; a.y_ld_t = y_ld_t;
    a.gates = train ? gates : nullptr; a.g_ld_m = g_ld_m; a.g_ld_t = g_ld_t;
    a.c = train ? c : nullptr; a.c_ld_m = c_ld_m; a.c_ld_t = c_ld_t;
    return 0;
}

int persistent_impl(LstmArgs& a, int ndir, unsigned* sync, cvc_stream_t stream) {
    const int H = a.H;
    if (!sync || H < 128 || (H & 127) || H > 1024) return CVC_E_BADARG;
    a.sync = sync; a.spin_limit = 1u << 20;
    hipStream_t st = (hipStream_t)stream;
    // 8 waves (K / 8 per wave) when K is a multiple of 256, else 4 waves (K / 4 per wave)
    const bool w8 = (H % 256) == 0;
    const int NC = w8 ? H / 256 : H / 128;
    // (slot 0 = h0 = 0 and the sync words are cleared by the launcher, once the launch is certain)
#define CVC_LSTM_P(MT_, NC_, NW_)                                                                                           \
    return launch_resident(lstm_persistent_kernel<MT_, NC_, NW_>, dim3(H / 8, ndir), NW_ * 64, a, a.hq, a.h_stride * ndir, sync, \
                           SYNC_GROUPS, st)
#define CVC_LSTM_NC(MT_)                                                                                       \
    if (w8) {                                                                                                  \
        switch (NC) { case 1: CVC_LSTM_P(MT_, 1, 8); case 2: CVC_LSTM_P(MT_, 2, 8); case 3: CVC_LSTM_P(MT_, 3, 8); \
                      default: CVC_LSTM_P(MT_, 4, 8); }                                                        \
    }                                                                                                          \
    switch (NC) { case 1: CVC_LSTM_P(MT_, 1, 4); case 3: CVC_LSTM_P(MT_, 3, 4); case 5: CVC_LSTM_P(MT_, 5, 4);     \
                  default: CVC_LSTM_P(MT_, 7, 4); }
    if (a.M <= 32) { CVC_LSTM_NC(1) }
    CVC_LSTM_NC(2)
#undef CVC_LSTM_NC
#undef CVC_LSTM_P
}

int steps_impl(LstmArgs& a, int ndir, cvc_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    // workspace hq: [2 h states + c][ndir][Kp/4][64][4], all zero at the start (h0 = c0 = 0; rows beyond M and the k padding stay 0)
    const long long one = a.h_stride * ndir, n = 3 * one;
    launch_clear(a.hq, n, nullptr, 0, st);
    a.c_q = a.hq + 2 * one;
    const dim3 grid(a.H / 8, ndir);
    for (int s = 0; s < a.F; ++s) {
        a.h_in = a.hq + (size_t)(s & 1) * one;
        a.h_out = a.hq + (size_t)((s + 1) & 1) * one;
        a.t_of[0] = s; a.t_of[1] = a.F - 1 - s;
        if (a.M <= 32) hipLaunchKernelGGL(lstm_step_kernel<1>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(lstm_step_kernel<2>, grid, dim3(256), 0, st, a);
    }
    return cvc_launch_status();
}

}  // namespace

extern "C" int cvc_lstm_persistent_sync_words(void) { return (int)sync_words(SYNC_GROUPS); }

extern "C" int cvc_lstm_seq_persistent_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih,
                                           const float* b_hh, int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m,
                                           long long y_ld_t, unsigned* sync, cvc_stream_t stream) {
    LstmArgs a{};
    if (int rc = fill_common(a, wp, gi, gi_ld_m, gi_ld_t, b_ih, b_hh, M, F, H, ndir, hq, y, y_ld_m, y_ld_t, nullptr, 0, 0, nullptr, 0, 0, false))
        return rc;
    return persistent_impl(a, ndir, sync, stream);
}

extern "C" int cvc_lstm_seq_persistent_train_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t,
                                                 const float* b_ih, const float* b_hh, int M, int F, int H, int ndir, float* hq,
                                                 float* y, long long y_ld_m, long long y_ld_t, float* gates, long long g_ld_m,
                                                 long long g_ld_t, float* c, long long c_ld_m, long long c_ld_t, unsigned* sync,
                                                 cvc_stream_t stream) {
    LstmArgs a{};
    if (int rc = fill_common(a, wp, gi, gi_ld_m, gi_ld_t, b_ih, b_hh, M, F, H, ndir, hq, y, y_ld_m, y_ld_t, gates, g_ld_m, g_ld_t, c, c_ld_m,
                             c_ld_t, true))
        return rc;
    return persistent_impl(a, ndir, sync, stream);
}

extern "C" int cvc_lstm_seq_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih,
                                const float* b_hh, int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m,
                                long long y_ld_t, cvc_stream_t stream) {
    LstmArgs a{};
    if (int rc = fill_common(a, wp, gi, gi_ld_m, gi_ld_t, b_ih, b_hh, M, F, H, ndir, hq, y, y_ld_m, y_ld_t, nullptr, 0, 0, nullptr, 0, 0, false))
        return rc;
    return steps_impl(a, ndir, stream);
}

extern "C" int cvc_lstm_seq_train_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih,
                                      const float* b_hh, int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m,
                                      long long y_ld_t, float* gates, long long g_ld_m, long long g_ld_t, float* c, long long c_ld_m,
                                      long long c_ld_t, cvc_stream_t stream) {
    LstmArgs a{};
    if (int rc = fill_common(a, wp, gi, gi_ld_m, gi_ld_t, b_ih, b_hh, M, F, H, ndir, hq, y, y_ld_m, y_ld_t, gates, g_ld_m, g_ld_t, c, c_ld_m,
                             c_ld_t, true))
        return rc;
    return steps_impl(a, ndir, stream);
}

extern "C" int cvc_lstm_seq_bwd_work(int M, int H, int ndir) {
    if (M < 1 || M > 64 || H < 8 || (H & 7) || ndir < 1 || ndir > 2) return CVC_E_BADARG;
    const long long ntot = (long long)((H + 127) / 128) * 128;
    return (int)(ndir * ((long long)M * H + 4LL * H * 64 + (long long)bwd_ksplit(H) * M * ntot));
}

extern "C" int cvc_lstm_seq_bwd(const float* dy, long long dy_ld_m, long long dy_ld_t, const float* gates, long long g_ld_m,
                                long long g_ld_t, const float* c, long long c_ld_m, long long c_ld_t, const float* w_hh, int M, int F,
                                int H, int ndir, float* dg, float* work, cvc_stream_t stream) {
    if (!dy || !gates || !c || !w_hh || !dg || !work || M < 1 || M > 64 || F < 1 || H < 8 || (H & 7) || ndir < 1 || ndir > 2 ||
        (dy_ld_m & 3) || (dy_ld_t & 3) || (g_ld_m & 3) || (g_ld_t & 3) || (c_ld_m & 3) || (c_ld_t & 3) || !aligned16(dy) ||
        !aligned16(gates) || !aligned16(c) || !aligned16(w_hh) || !aligned16(dg) || !aligned16(work))
        return CVC_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int ks = bwd_ksplit(H);
    const long long ntot = (long long)((H + 127) / 128) * 128;     // plane row length of the backward-data product
    const size_t mh = (size_t)M * H, per_dir = mh + (size_t)4 * H * 64 + (size_t)ks * M * ntot;
    const long long row_ld = (long long)ndir * 4 * H;
    for (int s = 0; s < F; ++s) {
        LstmStepBwd2 both{};
        for (int d = 0; d < ndir; ++d) {
            const long long t = d == 0 ? F - 1 - s : s;           // the forward direction is walked back from the end
            const long long tp = d == 0 ? t - 1 : t + 1;          // where this direction's c_{t-1} lives
            float* base = work + per_dir * d;
            float* dg_q = base + mh;
            float* planes = dg_q + (size_t)4 * H * 64;
            LstmStepBwd& a = both.d[d];
            a.dy = dy + t * dy_ld_t + (long long)d * H; a.dy_ld = dy_ld_m;
            a.dh_planes = s > 0 ? planes : nullptr; a.nplanes = ks; a.plane_stride = (long long)M * ntot; a.plane_ld = ntot;
            a.gates = gates + t * g_ld_t + (long long)d * 4 * H; a.g_ld = g_ld_m;
            a.c = c + t * c_ld_t + (long long)d * H; a.c_ld = c_ld_m;
            a.c_prev = (tp >= 0 && tp < F) ? c + tp * c_ld_t + (long long)d * H : nullptr;
            a.dc = base; a.first = s == 0;
            a.dg = dg + (t * M) * row_ld + (long long)d * 4 * H; a.dg_ld = row_ld;
            a.dg_q = dg_q; a.M = M; a.H = H;
        }
        hipLaunchKernelGGL(lstm_pointwise_bwd_kernel, dim3((H / 4 * 64 + 255) / 256, ndir), dim3(256), 0, st, both);
        if (s + 1 < F) {                                          // the carry of the last processed step is not needed
            for (int d = 0; d < ndir; ++d) {
                float* base = work + per_dir * d;
                float* dg_q = base + mh;
                float* planes = dg_q + (size_t)4 * H * 64;
                // one K slice: the product goes straight into "plane 0" (row stride ntot); several: planes, summed by the next step
                cvc_nn_seg seg{w_hh + (size_t)d * 4 * H * H, planes, H, H, (int)ntot};
                int rc = cvc_linear_nn_planes_fwd(dg_q, 4 * H, M, &seg, 1, ks, planes, stream);
                if (rc) return rc;
            }
        }
    }
    return cvc_launch_status();
}
