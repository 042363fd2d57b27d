// Grounding F1 of generated captions on the device: for every object word of a caption the most attended proposal of every sampled
// frame, tested against the clip's annotated boxes, counted per detection class (cvc.metrics.grounding; Trainer.eval with
// --val_metrics device --eval_obj_grounding).
//
// cvc_grounding_f1: ONE WORKGROUP of sixteen waves per caption row.
//   Words: wave 0 loads the row (lane t = position t), L = the position of the first 0, the class of position t < L is
//     word_cls[seq[t]] (0 for an id outside [0, V) and for a class outside [1, C]); the object words are compacted and the first
//     object word of every class is that class's representative -- at most 63 predicted classes.
//   Picks: the waves take (object word, frame) pairs round robin, two per turn (the second pair's weights are in flight while the
//     first is reduced); a wave reduces the frame's Np weights to (max, first index): every
//     lane scans its j = lane, lane + 64, .. with a strict >, the lanes' maxima meet in a DPP max, the lowest index among the lanes
//     that hold it in a DPP min.  A frame without a weight > -inf picks j = 0, and so does a frame whose first weight is NaN (the
//     sequential scan from j = 0 with a strict > never leaves it).  Slots >= P carry -inf.  pick = f * Np + j goes to the output
//     and, for the phase below, to LDS.
//   Boxes: thread k takes box k < min(nbox, K) of the row's clip (loaded at the kernel's start, beside the words): its class (outside
//     [1, C]: not counted), whether that class is predicted, and whether the representative's pick in the box's frame hits it
//     (2 * inter > union, fp32, no contraction).  The first box of every class then adds the class's three ground-truth counters to
//     the table, lane i of the last wave the three prediction counters of predicted class i: one integer atomic per (class, counter)
//     that is not zero.  Integer sums do not depend on the
//     order of arrival: the table, counts and f1 are bit-reproducible.
//   No host read, no allocation, sizes from the arguments alone: capturable in a HIP graph.
#include "cvc_common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int MAXT = 63;
constexpr int WAVES = 16;                      // a (word, frame) pair is a dependent load and reduction: many pairs in flight per row
constexpr int LDS_LIMIT = 48 * 1024;           // dynamic LDS: the picks [T, F] and three words per box

__device__ __forceinline__ int wave_min_int(int v) {
    auto m = [](int a, int b) { return a < b ? a : b; };
    v = m(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));
    v = m(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));
    v = m(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));
    v = m(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));
    v = m(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false));   // lanes outside the row mask keep their own value
    v = m(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false));
    return __builtin_amdgcn_readlane(v, 63);
}

// One lane's share of a frame's Np weights (j = lane, lane + 64, ..): its largest weight > -inf and that weight's first j.
struct FrameScan {
    float bv;
    int bj;
    bool nan0;                                     // (lane 0) the frame's first weight is NaN
};

__device__ __forceinline__ FrameScan scan_frame(const float* a, int f, int Np, int P, int lane) {
    const long long slot0 = (long long)f * Np;
    FrameScan s = {-INFINITY, INT_MAX, false};
    for (int j = lane; j < Np; j += 64) {
        const float w = slot0 + j < (long long)P ? a[slot0 + j] : -INFINITY;      // a slot >= P: the trimmed axis
        if (j == 0) s.nan0 = w != w;
        if (w > s.bv) {
            s.bv = w;
            s.bj = j;
        }
    }
    return s;
}

// the wave's (max, first index): the sequential search from j = 0 with a strict > (it never leaves a NaN at j = 0)
__device__ __forceinline__ int first_max(FrameScan s) {
    const float m = wave_max(s.bv);
    const int j = wave_min_int(s.bv == m ? s.bj : INT_MAX);
    return (j == INT_MAX || __ballot(s.nan0) != 0ull) ? 0 : j;
}

// a: the picked proposal (x1, y1, x2, y2), g: the annotated box.  No +1 pixel; every product and sum rounded on its own.
__device__ __noinline__ bool box_hit(float a0, float a1, float a2, float a3, float g0, float g1, float g2, float g3) {
#pragma clang fp contract(off)
    const float w = fminf(a2, g2) - fmaxf(a0, g0);
    const float h = fminf(a3, g3) - fmaxf(a1, g1);
    if (w <= 0.f || h <= 0.f) return false;
    const float inter = w * h;
    const float area_a = (a2 - a0) * (a3 - a1);
    const float area_g = (g2 - g0) * (g3 - g1);
    const float uni = (area_a + area_g) - inter;
    return 2.f * inter > uni;
}

__global__ __launch_bounds__(64 * WAVES) void grounding_f1_kernel(const int64_t* seq, const float* att, const float* ppls, const float* gt,
                                                                  const int32_t* nbox, const int32_t* word_cls, int T, int P, int F, int Np,
                                                                  int K, int C, int V, int per_clip, int32_t* pick, int32_t* counts,
                                                                  float* f1, int32_t* table) {
    extern __shared__ int dyn[];
    int* s_pick = dyn;                             // [T, F]: the picks of the object words
    int* s_bc = dyn + T * F;                       // [K]: a box's class, 0 = not counted
    int* s_bh = s_bc + K;                          // [K]: the box is hit
    int* s_bp = s_bh + K;                          // [K]: the box's class is predicted
    __shared__ int s_cls[64];                      // class of position t, 0 = no object word
    __shared__ int s_obj[64];                      // the object words' positions, ascending
    __shared__ int s_rep_t[64], s_rep_c[64];       // the predicted classes: representative position, class
    __shared__ int s_n[2];                         // object words, predicted classes
    __shared__ int s_cnt[6];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int clip = row / per_clip;
    const long long id = (wave == 0 && lane < T) ? (long long)seq[(size_t)row * T + lane] : 0ll;
    // the thread's box is asked for now, beside the words: it is not needed before the picks are done
    int nb = nbox[clip];
    nb = nb < 0 ? 0 : (nb > K ? K : nb);
    float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (tid < nb) {
        const float* gk = gt + ((size_t)clip * K + tid) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = gk[i];
    }

    if (wave == 0) {
        const unsigned long long zeros = __ballot(lane < T && id == 0);
        const int L = zeros ? __builtin_ctzll(zeros) : T;
        int c = 0;
        if (lane < L && id > 0 && id < (long long)V) c = word_cls[id];
        c = (c >= 1 && c <= C) ? c : 0;
        s_cls[lane] = c;
        if (lane < 6) s_cnt[lane] = 0;
        bool rep = c > 0;                          // no earlier position holds the class (position t's class: a lane broadcast)
        for (int t = 0; t < L; ++t) {
            const int ct = __builtin_amdgcn_readlane(c, t);
            rep = rep && !(t < lane && ct == c);
        }
        const unsigned long long objs = __ballot(c > 0), reps = __ballot(rep);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (c > 0) s_obj[__popcll(objs & below)] = lane;
        if (rep) {
            const int i = __popcll(reps & below);
            s_rep_t[i] = lane;
            s_rep_c[i] = c;
        }
        if (lane == 0) {
            s_n[0] = __popcll(objs);
            s_n[1] = __popcll(reps);
        }
    }
    __syncthreads();
    const int n_obj = s_n[0], n_rep = s_n[1];

    // ---- picks: -1 wherever no object word stands, then one wave per (object word, frame)
    int32_t* pick_row = pick + (size_t)row * T * F;
    for (int i = tid; i < T * F; i += 64 * WAVES)
        if (s_cls[i / F] == 0) pick_row[i] = -1;
    // (two pairs per turn: the second pair's weights are on their way while the first pair is reduced)
    const int n_pairs = n_obj * F;
    for (int q = wave; q < n_pairs; q += 2 * WAVES) {
        const int q2 = q + WAVES;
        const bool two = q2 < n_pairs;
        const int t1 = s_obj[q / F], f1_ = q - (q / F) * F;
        const int t2 = two ? s_obj[q2 / F] : t1, f2_ = two ? q2 - (q2 / F) * F : f1_;
        const FrameScan a1 = scan_frame(att + ((size_t)row * T + t1) * P, f1_, Np, P, lane);
        const FrameScan a2 = scan_frame(att + ((size_t)row * T + t2) * P, f2_, Np, P, lane);
        const int slot1 = f1_ * Np + first_max(a1), slot2 = f2_ * Np + first_max(a2);
        if (lane == 0) {
            pick_row[t1 * F + f1_] = slot1;
            s_pick[t1 * F + f1_] = slot1;
            if (two) {
                pick_row[t2 * F + f2_] = slot2;
                s_pick[t2 * F + f2_] = slot2;
            }
        }
    }
    __syncthreads();

    // ---- the clip's boxes
    const float* pp = ppls + (size_t)clip * P * 7;
    for (int k = tid; k < nb; k += 64 * WAVES) {
        if (k != tid) {                            // (beyond the first 64 * WAVES boxes: not loaded at the kernel's start)
            const float* gk = gt + ((size_t)clip * K + k) * 6;
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = gk[i];
        }
        const float fc = g[5], ff = g[4];
        int c = 0, hit = 0, pred = 0;
        if (fc >= 1.f && fc <= (float)C) {
            c = (int)fc;
            int rt = -1;
            for (int i = 0; i < n_rep; ++i)
                if (s_rep_c[i] == c) rt = s_rep_t[i];
            pred = rt >= 0;
            if (pred && ff >= 0.f && ff < (float)F) {
                const int slot = s_pick[rt * F + (int)ff];
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                if (slot < P) {
                    a0 = pp[(size_t)slot * 7 + 0];
                    a1 = pp[(size_t)slot * 7 + 1];
                    a2 = pp[(size_t)slot * 7 + 2];
                    a3 = pp[(size_t)slot * 7 + 3];
                }
                hit = box_hit(a0, a1, a2, a3, g[0], g[1], g[2], g[3]) ? 1 : 0;
            }
        }
        s_bc[k] = c;
        s_bh[k] = hit;
        s_bp[k] = pred;
    }
    __syncthreads();
    // ground-truth side: the first box of a class adds the class's sums
    for (int k = tid; k < nb; k += 64 * WAVES) {
        const int c = s_bc[k];
        if (c == 0) continue;
        bool first = true;
        int n = 0, h = 0;
#pragma unroll 4
        for (int i = 0; i < nb; ++i) {             // (every lane walks all boxes: the reads are broadcasts and run ahead)
            const bool same = s_bc[i] == c;
            first = first && !(same && i < k);
            n += same ? 1 : 0;
            h += same ? s_bh[i] : 0;
        }
        if (!first) continue;
        int32_t* tc = table + (size_t)c * 6;
        atomicAdd(tc + 0, n);
        atomicAdd(&s_cnt[0], n);
        if (s_bp[k]) {
            atomicAdd(tc + 1, n);
            atomicAdd(&s_cnt[1], n);
            if (h) {
                atomicAdd(tc + 2, h);
                atomicAdd(&s_cnt[2], h);
            }
        }
    }
    // prediction side: lane i of the last wave takes predicted class i (the first waves are busy with the boxes)
    if (wave == WAVES - 1 && lane < n_rep) {
        const int c = s_rep_c[lane];
        int in_gt = 0, h = 0;
#pragma unroll 4
        for (int i = 0; i < nb; ++i) {
            const bool same = s_bc[i] == c;
            in_gt |= same ? 1 : 0;
            h |= same ? s_bh[i] : 0;
        }
        int32_t* tc = table + (size_t)c * 6;
        atomicAdd(tc + 3, 1);
        atomicAdd(&s_cnt[3], 1);
        if (in_gt) {
            atomicAdd(tc + 4, 1);
            atomicAdd(&s_cnt[4], 1);
        }
        if (h) {
            atomicAdd(tc + 5, 1);
            atomicAdd(&s_cnt[5], 1);
        }
    }
    __syncthreads();
    if (tid < 6) counts[(size_t)row * 6 + tid] = s_cnt[tid];
    if (tid == 0) {
        const int gt_n = s_cnt[0], gt_hit = s_cnt[2], pred_n = s_cnt[3], pred_hit = s_cnt[5];
        float v = 0.f;
        if (gt_n > 0 && pred_n > 0) {
            const float p = (float)pred_hit / (float)pred_n, r = (float)gt_hit / (float)gt_n;
            if (p + r > 0.f) v = 2.f * p * r / (p + r);
        }
        f1[row] = v;
    }
}

}  // namespace

extern "C" int cvc_grounding_f1(const int64_t* seq, const float* att, const float* ppls, const float* gt_bboxs, const int32_t* nbox,
                                const int32_t* word_cls, int rows, int T, int P, int F, int Np, int K, int C, int V, int per_clip,
                                int32_t* pick, int32_t* counts, float* f1, int32_t* table, cvc_stream_t stream) {
    if (seq == nullptr || att == nullptr || ppls == nullptr || gt_bboxs == nullptr || nbox == nullptr || word_cls == nullptr ||
        pick == nullptr || counts == nullptr || f1 == nullptr || table == nullptr)
        return CVC_E_BADARG;
    if (rows < 1 || T < 1 || T > MAXT || P < 1 || F < 1 || Np < 1 || K < 1 || C < 1 || V < 1 || per_clip < 1 || rows % per_clip != 0)
        return CVC_E_BADARG;
    if ((long long)F * Np > (long long)INT_MAX || (long long)P > (long long)F * Np) return CVC_E_BADARG;
    const long long lds = ((long long)T * F + 3ll * K) * (long long)sizeof(int);
    if (lds > LDS_LIMIT) return CVC_E_TOOBIG;
    hipLaunchKernelGGL(grounding_f1_kernel, dim3(rows), dim3(64 * WAVES), (size_t)lds, (hipStream_t)stream, seq, att, ppls, gt_bboxs, nbox,
                       word_cls, T, P, F, Np, K, C, V, per_clip, pick, counts, f1, table);
    return cvc_launch_status();
}
