// Token-overlap caption metrics on the device: the BLEU statistics, sentence BLEU-1..4 and ROUGE-L of candidate captions against
// their clip's reference captions, one launch (cvc.metrics; validation scores and reward mixes of self-critical training).
//
// cvc_caption_overlap: ONE WAVE per candidate row, as cider_d_kernel (csrc/cider.hip), on the same caption loader and n-gram keys
//   (csrc/caption_ngrams.h) -- but a caption's words here are the ids BEFORE its first 0 (the end mark is no word; L = 0 is possible).
//   BLEU: lane p owns the candidate's n-grams that start at p; a distinct n-gram is counted by the lane of its first occurrence,
//     which keeps the running maximum of the references' counts of its key: correct_n = sum over those lanes of min(count_c, max_r
//     count_r) (an integer DPP wave sum), guess_n = max(0, Lc - n + 1), ref_len = the counted reference length closest to Lc (the
//     shorter on a tie).  p_n = (correct_n + 1e-15) / (guess_n + 1e-9), BLEU_k = bp exp((sum_{n<=k} log p_n) / k), logs added in
//     ascending n, bp = 1 if Lc >= ref_len else exp(1 - ref_len / Lc); 0 when Lc = 0 or the clip has no reference.
//   ROUGE-L: the longest common subsequence of candidate and reference by the bit-vector recurrence of Allison & Dix (1986) in
//     Hyyro's form -- Lr <= 63 columns fit one 64-bit word: per candidate word c, M = ballot(lane < Lr && ref[lane] == c), U = V & M,
//     V = (V + U) | (V - U) from V = ~0; lcs = popcount(~V & (2^Lr - 1)).  p = max_r lcs_r / Lc, q = max_r (lcs_r / Lr) (Lr = 0: 0),
//     ROUGE_L = (1 + b^2) p q / (q + b^2 p), b = 1.2; 0 when Lc = 0, no reference, or p q = 0.
//   Integers are exact; the fp32 scores are formed by every lane alike from wave-uniform integers.  No atomics, no host
//   synchronisation: a row's result is bit-reproducible and independent of the launch's other rows.
#include "cvc_common.h"
#include "caption_ngrams.h"
#include <math.h>

namespace {

using cvc_caption::MAXT;
using cvc_caption::ngram_key;
using cvc_caption::count_key;

__global__ __launch_bounds__(64) void caption_overlap_kernel(const int64_t* cand, const int64_t* refs, const int32_t* nref, int T,
                                                             int per_clip, int Rmax, int32_t* stats, int32_t* lcs_out, float* bleu,
                                                             float* rouge) {
#pragma clang fp contract(off)
    __shared__ uint32_t sw[68];                    // the current caption's words (id + 1)
    __shared__ uint32_t cw[64];                    // the candidate's words
    __shared__ unsigned long long ck[64];          // the candidate's keys of the current order
    __shared__ unsigned long long rk[64];          // the current reference's keys of the current order
    const int row = blockIdx.x, lane = threadIdx.x;
    const int clip = row / per_clip;
    const int Lc = cvc_caption::load_caption<false>(cand + (size_t)row * T, T, lane, sw);
    cw[lane] = sw[lane];
    unsigned long long key_c[4];                   // this lane's n-gram per order; own: it is the first occurrence of its key
    int cnt_c[4], max_r[4];
    bool own[4];
#pragma unroll
    for (int n = 1; n <= 4; ++n) {
        const int npos = Lc - n + 1;               // (<= 0: the caption has no n-gram of this order)
        const bool valid = lane < npos;
        key_c[n - 1] = valid ? ngram_key(sw, lane, n) : 0ull;
        __syncthreads();                           // ck's readers of the previous order are done
        ck[lane] = key_c[n - 1];
        __syncthreads();
        bool first = false;
        cnt_c[n - 1] = valid ? count_key(ck, npos, key_c[n - 1], lane, &first) : 0;
        own[n - 1] = valid && first;
        max_r[n - 1] = 0;
    }
    int nr = nref[clip];
    nr = nr < 0 ? 0 : (nr > Rmax ? Rmax : nr);
    int ref_len = 0, lcs_max = 0;
    float q = 0.f;
    for (int r = 0; r < nr; ++r) {
        const int Lr = cvc_caption::load_caption<false>(refs + ((size_t)clip * Rmax + r) * T, T, lane, sw);
        const int d_new = Lr > Lc ? Lr - Lc : Lc - Lr, d_old = ref_len > Lc ? ref_len - Lc : Lc - ref_len;
        if (r == 0 || d_new < d_old || (d_new == d_old && Lr < ref_len)) ref_len = Lr;
#pragma unroll
        for (int n = 1; n <= 4; ++n) {
            const int npos = Lr - n + 1;
            const unsigned long long key = lane < npos ? ngram_key(sw, lane, n) : 0ull;
            __syncthreads();                       // rk's readers of the previous order are done
            rk[lane] = key;
            __syncthreads();
            if (own[n - 1]) {
                bool unused;
                const int c = count_key(rk, npos, key_c[n - 1], 64, &unused);
                max_r[n - 1] = c > max_r[n - 1] ? c : max_r[n - 1];
            }
        }
        // longest common subsequence: bit j of ~V is set where the DP row rises at reference column j
        const uint32_t mine = sw[lane];
        unsigned long long V = ~0ull;
        for (int i = 0; i < Lc; ++i) {
            const unsigned long long M = __ballot(lane < Lr && mine == cw[i]);
            const unsigned long long U = V & M;
            V = (V + U) | (V - U);
        }
        const int l = __popcll(~V & ((1ull << Lr) - 1ull));          // (Lr <= 63)
        if (lcs_out != nullptr && lane == 0) lcs_out[(size_t)row * Rmax + r] = l;
        lcs_max = l > lcs_max ? l : lcs_max;
        if (Lr > 0) q = fmaxf(q, (float)l / (float)Lr);
    }
    if (lcs_out != nullptr)
        for (int r = nr + lane; r < Rmax; r += 64) lcs_out[(size_t)row * Rmax + r] = -1;
    int correct[4], guess[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        correct[n] = wave_sum_int(own[n] ? (cnt_c[n] < max_r[n] ? cnt_c[n] : max_r[n]) : 0);
        guess[n] = Lc - n > 0 ? Lc - n : 0;
    }
    if (lane != 0) return;
    int32_t* st = stats + (size_t)row * 10;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        st[n] = correct[n];
        st[4 + n] = guess[n];
    }
    st[8] = Lc;
    st[9] = ref_len;
    float b[4] = {0.f, 0.f, 0.f, 0.f}, rl = 0.f;
    if (Lc > 0 && nr > 0) {
        const float bp = Lc >= ref_len ? 1.f : expf(1.f - (float)ref_len / (float)Lc);
        float logs = 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            logs += logf(((float)correct[n] + 1e-15f) / ((float)guess[n] + 1e-9f));
            b[n] = bp * expf(logs / (float)(n + 1));
        }
        if (lcs_max > 0) {
            const float beta2 = 1.2f * 1.2f;
            const float p = (float)lcs_max / (float)Lc;
            rl = (1.f + beta2) * p * q / (q + beta2 * p);
        }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) bleu[(size_t)row * 4 + n] = b[n];
    rouge[row] = rl;
}

}  // namespace

extern "C" int cvc_caption_overlap(const int64_t* cand, const int64_t* refs, const int32_t* nref, int rows, int T, int per_clip, int Rmax,
                                   int32_t* stats, int32_t* lcs, float* bleu, float* rouge, cvc_stream_t stream) {
    if (cand == nullptr || refs == nullptr || nref == nullptr || stats == nullptr || bleu == nullptr || rouge == nullptr) return CVC_E_BADARG;
    if (rows < 1 || T < 1 || T > MAXT || per_clip < 1 || rows % per_clip != 0 || Rmax < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(caption_overlap_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, cand, refs, nref, T, per_clip, Rmax, stats,
                       lcs, bleu, rouge);
    return cvc_launch_status();
}
