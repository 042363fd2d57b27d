// Caption-set diversity: how different the captions of one clip's candidate set are from each other -- the distinct n-grams of the
// set (Div-n), every caption's BLEU statistics against the set's other captions (mBLEU) and the number of different captions
// (cvc.metrics.set_diversity, cvc.metrics.DiversityScorer, cvc.decode.DecodeEngine.set_diversity).
//
// cvc_caption_set_stats: ONE WORKGROUP per clip, one wave per candidate row at a time (up to 16 waves, rows taken round robin), lane p
//   owns the n-grams (n = 1..4) that start at position p, as consensus_cider_kernel (csrc/consensus.hip) -- hence T <= 63.  A caption's
//   words are the ids BEFORE its first 0 (load_caption<false>, the convention of csrc/overlap.hip): L = 0 is possible.
//   Build pass, once per live row: the 4-word window per position (csrc/caption_ngrams.h; the key of order n is the window's highest
//   16 n bits) and the length, to LDS.
//   Pair pass: row i against every live row r of the clip, r ascending, itself included.  The window of one position of r after the
//   other is broadcast (readlane) and compared with the lane's own: the number of leading words on which the two agree says for all
//   four orders at once whether the n-grams are the same one.  From that one walk, per order:
//     r == i: the n-gram's count in the caption and whether this lane is its first occurrence there (own);
//     r != i: its count in r -- the running maximum over r is BLEU's clip, and a count > 0 in a row r < i says that the n-gram was
//       seen earlier in the clip.
//     distinct_n of the clip = the number of (row, lane) with own and not seen earlier;  correct_n of row i = sum over its own lanes
//     of min(count, max_r count_r) (integer DPP wave sums), ref_len = the other rows' length closest to L_i (the shorter on a tie).
//     Row i repeats an earlier row when their lengths and all their windows are equal.
//   The fp32 BLEU expressions are caption_overlap_kernel's, formed from the same integers in the same order, contraction off: mbleu and
//   mbleu_stats have the bits cvc_caption_overlap returns for that candidate and those references.
//   Last pass: twelve threads add the rows' integers into the clip's set_stats, rows in ascending order.
//   No atomics, no global workspace: a clip's outputs are bit-reproducible and independent of the launch's other clips.
//   Per instantiation (gfx950, hipcc -O3): <8> (per_clip <= 8, at most 512 threads): 38 VGPRs, 65 SGPRs, no scratch, no spill,
//   6496 bytes of LDS; <32> (at most 1024 threads): 38 VGPRs, 65 SGPRs, no scratch, no spill, 21 632 bytes of LDS.
#include "cvc_common.h"
#include "caption_ngrams.h"
#include <math.h>

namespace {

using cvc_caption::MAXT;
using cvc_caption::ngram_key;

constexpr int MAX_PER_CLIP = 32;
constexpr int MAX_WAVES = 16;

// lane p's value in every lane (p is wave-uniform)
__device__ __forceinline__ unsigned long long lane_key(unsigned long long v, int p) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, p);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), p);
    return ((unsigned long long)hi << 32) | lo;
}

// on how many leading 16-bit words two windows agree, given their exclusive or (4: on all) -- the n-grams of order n that start
// at the two positions are the same one iff this is >= n, provided one of them is an n-gram at all (its n words are non-zero)
__device__ __forceinline__ int lead_words(unsigned long long x) { return x != 0ull ? (int)__builtin_clzll(x) >> 4 : 4; }

template <int NMAX>
__global__ __launch_bounds__(64 * (NMAX < MAX_WAVES ? NMAX : MAX_WAVES)) void caption_set_stats_kernel(
    const int64_t* cand, const int32_t* live, int T, int per_clip, int32_t* set_stats, int32_t* mbleu_stats, float* mbleu) {
#pragma clang fp contract(off)
    constexpr int WAVES = NMAX < MAX_WAVES ? NMAX : MAX_WAVES;
    __shared__ unsigned long long win[NMAX][64];   // the 4-word window that starts at each position (words as id + 1, 0 past the end)
    __shared__ int len[NMAX];
    __shared__ int alive[NMAX];
    __shared__ int fresh[NMAX][4];                 // the row's n-grams of each order that no earlier position of the clip holds
    __shared__ int uniq[NMAX];                     // 1: a live row that repeats no earlier live row
    __shared__ uint32_t sw[WAVES][68];
    const int clip = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t* rows = cand + (size_t)clip * per_clip * T;
    if ((int)threadIdx.x < per_clip) alive[threadIdx.x] = live == nullptr || live[(size_t)clip * per_clip + threadIdx.x] != 0 ? 1 : 0;
    __syncthreads();

    // ---- build: every live row's windows, once (the trip count is the same for every wave: the loader holds workgroup barriers)
    for (int j0 = 0; j0 < per_clip; j0 += nwaves) {
        const int j = j0 + wave;
        const bool active = j < per_clip && alive[j] != 0;
        const int L = cvc_caption::load_caption<false>(active ? rows + (size_t)j * T : rows, active ? T : 0, lane, sw[wave]);
        if (active) {
            win[j][lane] = ngram_key(sw[wave], lane, 4);
            if (lane == 0) len[j] = L;
        }
    }
    __syncthreads();

    // ---- pairs: row i against every live row of the clip (LDS windows and lengths are read-only from here on)
    for (int i = wave; i < per_clip; i += nwaves) {
        const size_t row = (size_t)clip * per_clip + i;
        int correct[4] = {0, 0, 0, 0}, guess[4] = {0, 0, 0, 0}, fr[4] = {0, 0, 0, 0};
        int Lc = 0, ref_len = 0, nr = 0;
        bool dup = false;
        const bool on = alive[i] != 0;
        if (on) {
            Lc = len[i];
            const unsigned long long wi = win[i][lane];
            int cnt_c[4] = {0, 0, 0, 0}, max_r[4] = {0, 0, 0, 0};
            bool own[4] = {true, true, true, true}, seen[4] = {false, false, false, false};
            for (int r = 0; r < per_clip; ++r) {
                if (alive[r] == 0) continue;
                const int Lr = len[r];
                const unsigned long long wr = win[r][lane];
                int cc[4] = {0, 0, 0, 0};          // row r's counts of the n-grams that start at this lane of row i
                if (r == i) {
                    for (int q = 0; q < Lr; ++q) {
                        const int lead = lead_words(wi ^ lane_key(wr, q));
#pragma unroll
                        for (int n = 1; n <= 4; ++n) {
                            cc[n - 1] += lead >= n ? 1 : 0;
                            own[n - 1] = own[n - 1] && !(lead >= n && q < lane);
                        }
                    }
#pragma unroll
                    for (int n = 0; n < 4; ++n) cnt_c[n] = cc[n];
                    continue;
                }
                for (int q = 0; q < Lr; ++q) {
                    const int lead = lead_words(wi ^ lane_key(wr, q));
#pragma unroll
                    for (int n = 1; n <= 4; ++n) cc[n - 1] += lead >= n ? 1 : 0;
                }
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    max_r[n] = cc[n] > max_r[n] ? cc[n] : max_r[n];
                    seen[n] = seen[n] || (r < i && cc[n] > 0);
                }
                const int d_new = Lr > Lc ? Lr - Lc : Lc - Lr, d_old = ref_len > Lc ? ref_len - Lc : Lc - ref_len;
                if (nr == 0 || d_new < d_old || (d_new == d_old && Lr < ref_len)) ref_len = Lr;
                ++nr;
                if (r < i && Lr == Lc && __ballot(wi != wr) == 0ull) dup = true;
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) {          // a lane past the last n-gram of the order holds none: whatever its zero words met
                const bool mine = lane < Lc - n && own[n];
                correct[n] = wave_sum_int(mine ? (cnt_c[n] < max_r[n] ? cnt_c[n] : max_r[n]) : 0);
                fr[n] = wave_sum_int(mine && !seen[n] ? 1 : 0);
                guess[n] = Lc - n > 0 ? Lc - n : 0;
            }
        }
        if (lane != 0) continue;
#pragma unroll
        for (int n = 0; n < 4; ++n) fresh[i][n] = fr[n];
        uniq[i] = on && !dup ? 1 : 0;
        int32_t* st = mbleu_stats + row * 10;
        const bool scored = on && nr > 0;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            st[n] = scored ? correct[n] : 0;
            st[4 + n] = scored ? guess[n] : 0;
        }
        st[8] = scored ? Lc : 0;
        st[9] = scored ? ref_len : 0;
        float b[4] = {0.f, 0.f, 0.f, 0.f};
        if (scored && Lc > 0) {
            const float bp = Lc >= ref_len ? 1.f : expf(1.f - (float)ref_len / (float)Lc);
            float logs = 0.f;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                logs += logf(((float)correct[n] + 1e-15f) / ((float)guess[n] + 1e-9f));
                b[n] = bp * expf(logs / (float)(n + 1));
            }
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) mbleu[row * 4 + n] = b[n];
    }
    __syncthreads();

    // ---- the clip's integers: slot t by thread t, rows in ascending order
    const int t = threadIdx.x;
    if (t < 12) {
        int v = 0, nlive = 0;
        for (int j = 0; j < per_clip; ++j) {
            if (alive[j] == 0) continue;
            ++nlive;
            if (t < 4) v += fresh[j][t];
            else if (t < 8) v += len[j] - (t - 4) > 0 ? len[j] - (t - 4) : 0;
            else if (t == 9) v += uniq[j];
        }
        if (t == 8) v = nlive;
        if (t == 10) v = nlive >= 2 ? nlive : 0;
        set_stats[(size_t)clip * 12 + t] = v;
    }
}

}  // namespace

extern "C" int cvc_caption_set_stats(const int64_t* cand, const int32_t* live, int rows, int T, int per_clip, int32_t* set_stats,
                                     int32_t* mbleu_stats, float* mbleu, cvc_stream_t stream) {
    if (cand == nullptr || set_stats == nullptr || mbleu_stats == nullptr || mbleu == nullptr) return CVC_E_BADARG;
    if (rows < 1 || T < 1 || T > MAXT || per_clip < 1 || per_clip > MAX_PER_CLIP || rows % per_clip != 0) return CVC_E_BADARG;
    const int nwaves = per_clip < MAX_WAVES ? per_clip : MAX_WAVES;
    if (per_clip <= 8)
        hipLaunchKernelGGL(caption_set_stats_kernel<8>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream, cand, live, T,
                           per_clip, set_stats, mbleu_stats, mbleu);
    else
        hipLaunchKernelGGL(caption_set_stats_kernel<MAX_PER_CLIP>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream,
                           cand, live, T, per_clip, set_stats, mbleu_stats, mbleu);
    return cvc_launch_status();
}
