// Self-critical training's reward: CIDEr-D (Vedantam et al. 2015; corpus-df mode) of sampled captions against the clip's reference
// captions, and the per-token loss weights that follow from it.  Device tensors in, device tensors out, no host read-back.
//
// cvc_cider_d: ONE WAVE per candidate row, lane p owns the n-grams (n = 1..4) that start at position p -- hence T <= 63.
//   A caption's words are its ids up to and including the first 0 (L words, 1 <= L <= T; all T without a 0).  An n-gram is one exact
//   64-bit key: 16 bits per word holding id + 1, first word in the highest bits, unused positions 0 (the order is part of the key).
//   (Loader and keys: csrc/caption_ngrams.h, with the end mark counted.)
//   Words (as id + 1, 0 past the caption's end) and keys go to LDS; a key's count is the number of the caption's positions that
//   hold it, and every distinct n-gram is counted once, by the lane of its first occurrence.  idf comes from a binary search of
//   the sorted table (precomputed on the host in fp64: no logf here), an n-gram that is not in it has idf_unseen = ln N_doc.
//     v_n[g] = count * idf[g];  s_n(c, r) = sum_g min(v_n^c[g], v_n^r[g]) v_n^r[g] / (|v_n^c| |v_n^r|)   (0 if a norm is 0)
//     reward = 10 * mean_r mean_n s_n(c, r) exp(-(L_c - L_r)^2 / (2 sigma^2));  no reference: 0.
//   Norms and clipped dot products are DPP wave sums (fixed order), references and orders are added in ascending order by every
//   lane alike: a row's result is bit-reproducible and independent of the launch's other rows.  No atomics.
// cvc_scst_weights: the advantage of every row (leave-one-out mean of the clip's other samples, or a given baseline) spread over the
//   caption's steps up to and including the first 0 (cvc.misc.utils._text_mask), one thread per row.
#include "cvc_common.h"
#include "caption_ngrams.h"
#include <math.h>

namespace {

using cvc_caption::MAXT;
using cvc_caption::ngram_key;
using cvc_caption::count_key;

__device__ __forceinline__ float idf_of(const unsigned long long* keys, const float* idf, int G, float idf_unseen, unsigned long long key) {
    int lo = 0, hi = G;
    while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return (lo < G && keys[lo] == key) ? idf[lo] : idf_unseen;
}

__global__ __launch_bounds__(64) void cider_d_kernel(const int64_t* cand, const int64_t* refs, const int32_t* nref, int T, int per_clip,
                                                     int Rmax, const unsigned long long* keys, const float* idf, int G, float idf_unseen,
                                                     float inv_2s2, float* reward, float* per_order) {
#pragma clang fp contract(off)
    __shared__ uint32_t sw[68];
    __shared__ unsigned long long ck[4][64];       // the candidate's keys per order (0 = no n-gram starts here)
    __shared__ unsigned long long rk[64];          // the current reference's keys of the current order
    const int row = blockIdx.x, lane = threadIdx.x;
    const int clip = row / per_clip;
    const int Lc = cvc_caption::load_caption<true>(cand + (size_t)row * T, T, lane, sw);
    float norm_c[4];
#pragma unroll
    for (int n = 1; n <= 4; ++n) {
        const int npos = Lc - n + 1;               // (<= 0: the caption has no n-gram of this order)
        const bool valid = lane < npos;
        const unsigned long long key = valid ? ngram_key(sw, lane, n) : 0ull;
        ck[n - 1][lane] = key;
        __syncthreads();
        float v = 0.f;
        if (valid) {
            bool first;
            const int c = count_key(ck[n - 1], npos, key, lane, &first);
            if (first) v = (float)c * idf_of(keys, idf, G, idf_unseen, key);
        }
        norm_c[n - 1] = sqrtf(wave_sum(v * v));
    }
    int nr = nref[clip];
    nr = nr < 0 ? 0 : (nr > Rmax ? Rmax : nr);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < nr; ++r) {
        const int Lr = cvc_caption::load_caption<true>(refs + ((size_t)clip * Rmax + r) * T, T, lane, sw);
        const float dl = (float)(Lc - Lr);
        const float gauss = expf(-(dl * dl) * inv_2s2);
#pragma unroll
        for (int n = 1; n <= 4; ++n) {
            const int npos = Lr - n + 1;
            const bool valid = lane < npos;
            const unsigned long long key = valid ? ngram_key(sw, lane, n) : 0ull;
            __syncthreads();                       // rk's readers of the previous order are done
            rk[lane] = key;
            __syncthreads();
            float vr = 0.f, term = 0.f;
            if (valid) {
                bool first;
                const int c = count_key(rk, npos, key, lane, &first);
                if (first) {
                    const float w = idf_of(keys, idf, G, idf_unseen, key);
                    bool unused;
                    const int cc = count_key(ck[n - 1], Lc - n + 1, key, 64, &unused);
                    vr = (float)c * w;
                    term = fminf((float)cc * w, vr) * vr;
                }
            }
            const float norm_r = sqrtf(wave_sum(vr * vr));
            const float dot = wave_sum(term);
            if (norm_c[n - 1] > 0.f && norm_r > 0.f) acc[n - 1] += dot / (norm_c[n - 1] * norm_r) * gauss;
        }
    }
    if (lane == 0) {
        float po[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) po[n] = nr > 0 ? 10.f * acc[n] / (float)nr : 0.f;
        reward[row] = 0.25f * ((po[0] + po[1]) + (po[2] + po[3]));
        if (per_order != nullptr) {
#pragma unroll
            for (int n = 0; n < 4; ++n) per_order[(size_t)row * 4 + n] = po[n];
        }
    }
}

__global__ __launch_bounds__(64) void scst_weights_kernel(const float* reward, const float* base, int rows, int S, const int64_t* cand,
                                                          int T, int t_major, float* adv, float* w) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const int clip = row / S;
    float a;
    if (S > 1) {
        float others = 0.f;
        for (int k = 0; k < S; ++k)
            if (clip * S + k != row) others += reward[clip * S + k];
        a = reward[row] - others / (float)(S - 1);
    } else {
        a = reward[row] - base[clip];
    }
    adv[row] = a;
    bool live = true;                              // the steps up to and including the first 0
    for (int t = 0; t < T; ++t) {
        const size_t at = t_major ? (size_t)t * rows + row : (size_t)row * T + t;
        w[at] = live ? a : 0.f;
        live = live && cand[(size_t)row * T + t] != 0;
    }
}

}  // namespace

extern "C" int cvc_cider_d(const int64_t* cand, const int64_t* refs, const int32_t* nref, int rows, int T, int per_clip, int Rmax,
                           const unsigned long long* keys, const float* idf, int G, float idf_unseen, float sigma, float* reward,
                           float* per_order, cvc_stream_t stream) {
    if (cand == nullptr || refs == nullptr || nref == nullptr || reward == nullptr) return CVC_E_BADARG;
    if (rows < 1 || T < 1 || T > MAXT || per_clip < 1 || rows % per_clip != 0 || Rmax < 1 || G < 0) return CVC_E_BADARG;
    if (G > 0 && (keys == nullptr || idf == nullptr)) return CVC_E_BADARG;
    if (!(sigma > 0.f)) return CVC_E_BADARG;
    hipLaunchKernelGGL(cider_d_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, cand, refs, nref, T, per_clip, Rmax, keys, idf, G,
                       idf_unseen, 1.0f / (2.0f * sigma * sigma), reward, per_order);
    return cvc_launch_status();
}

extern "C" int cvc_scst_weights(const float* reward, const float* base, int rows, int per_clip, const int64_t* cand, int T, int t_major,
                                float* adv, float* w, cvc_stream_t stream) {
    if (reward == nullptr || cand == nullptr || adv == nullptr || w == nullptr) return CVC_E_BADARG;
    if (rows < 1 || T < 1 || per_clip < 1 || rows % per_clip != 0) return CVC_E_BADARG;
    if ((per_clip == 1) != (base != nullptr)) return CVC_E_BADARG;       // a given baseline with one sample per clip, and only then
    hipLaunchKernelGGL(scst_weights_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, reward, base, rows, per_clip, cand,
                       T, t_major != 0, adv, w);
    return cvc_launch_status();
}
