// Consensus (minimum-Bayes-risk) caption selection: among a clip's candidates keep the one with the highest mean CIDEr-D against the
// clip's other candidates as stand-in references (cvc.cider.CiderD.consensus, cvc.decode.DecodeEngine.consensus).
//
// cvc_consensus_cider: ONE WORKGROUP per clip, one wave per candidate row at a time (up to 16 waves, rows taken round robin), lane p
//   owns the n-grams (n = 1..4) that start at position p, exactly as cider_d_kernel (csrc/cider.hip) -- hence T <= 63.
//   Build pass, once per row: the caption's words (csrc/caption_ngrams.h, the end mark counted), its 4-word window per position (the
//   key of order n is the window's highest 16 n bits where an n-gram starts), per order and position the count of the n-gram at the
//   lane of its first occurrence (0 elsewhere), its idf from ONE binary search of the table -- the four orders' searches walk the
//   table side by side, their loads in flight together -- and the four norms; all to LDS.
//   Pair pass: row i as the candidate against every other live row r of the clip as the reference, r ascending: nothing is looked
//   up again, a pair costs the clipped dot products only.  Counts are taken across lanes, not by scanning LDS: the window of
//   one position after the other is broadcast (readlane) and compared with the lane's own -- the number of leading words on which
//   the two agree says for all four orders at once whether the n-grams match.
//     v_n[g] = count * idf[g];  s_n(c, r) = sum_g min(v_n^c[g], v_n^r[g]) v_n^r[g] / (|v_n^c| |v_n^r|)   (0 if a norm is 0)
//     utility[i] = 10 * mean_r mean_n s_n(i, r) exp(-(L_i - L_r)^2 / (2 sigma^2));  no other live row, or a dead row: 0.
//   The floating-point arithmetic is cider_d_kernel's, expression by expression (same lane ownership, same DPP wave sums,
//   references and orders added in ascending order, contraction off; counts and table look-ups are exact either way): utility[i]
//   has the bits cvc_cider_d returns for that candidate and those references.
//   Pick pass: the first live row with the largest utility (0 without a live row), and that row's T ids copied to best.
//   No atomics, no global workspace: a clip's outputs are bit-reproducible and independent of the launch's other clips.
//   LDS per workgroup: 1820 bytes per row + 4352; the kernel is instantiated for <= 8 and <= 32 rows per clip (18 912 / 62 592 bytes).
#include "cvc_common.h"
#include "caption_ngrams.h"
#include "caption_windows.h"
#include <math.h>

namespace {

using cvc_caption::MAXT;
using cvc_caption::ngram_key;
using cvc_windows::lane_key;
using cvc_windows::lead_words;
using cvc_windows::idf_of4;

constexpr int MAX_PER_CLIP = 32;
constexpr int MAX_WAVES = 16;

template <int NMAX>
__global__ __launch_bounds__(64 * MAX_WAVES) void consensus_cider_kernel(const int64_t* cand, const int32_t* live, int T, int per_clip,
                                                                         const unsigned long long* keys, const float* idf, int G,
                                                                         float idf_unseen, float inv_2s2, float* utility, int32_t* pick,
                                                                         int64_t* best) {
#pragma clang fp contract(off)
    __shared__ unsigned long long win[NMAX][64];   // the 4-word window that starts at each position (words as id + 1, 0 past the end)
    __shared__ float wt[NMAX][4][64];              // idf of the n-gram that starts here, at the lane of its first occurrence
    __shared__ uint8_t cnt[NMAX][4][64];           // its count in the caption there, 0 at every other lane
    __shared__ float norm[NMAX][4];
    __shared__ int len[NMAX];
    __shared__ int alive[NMAX];
    __shared__ float util[NMAX];
    __shared__ uint32_t sw[MAX_WAVES][68];
    const int clip = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t* rows = cand + (size_t)clip * per_clip * T;
    if ((int)threadIdx.x < per_clip) alive[threadIdx.x] = live == nullptr || live[(size_t)clip * per_clip + threadIdx.x] != 0 ? 1 : 0;
    __syncthreads();

    // ---- build: every live row's vectors, once (the trip count is the same for every wave: the loader holds workgroup barriers)
    for (int j0 = 0; j0 < per_clip; j0 += nwaves) {
        const int j = j0 + wave;
        const bool active = j < per_clip && alive[j] != 0;
        const int L = cvc_caption::load_caption<true>(active ? rows + (size_t)j * T : rows, active ? T : 0, lane, sw[wave]);
        if (active) {
            const unsigned long long w4 = ngram_key(sw[wave], lane, 4);
            win[j][lane] = w4;
            if (lane == 0) len[j] = L;
            unsigned long long key[4];
            bool own[4] = {true, true, true, true};
            int c[4] = {0, 0, 0, 0};
            for (int q = 0; q < L; ++q) {          // position q's window against this lane's: all four orders in one walk
                const int lead = lead_words(w4 ^ lane_key(w4, q));
#pragma unroll
                for (int n = 1; n <= 4; ++n) {
                    c[n - 1] += lead >= n ? 1 : 0;
                    own[n - 1] = own[n - 1] && !(lead >= n && q < lane);
                }
            }
#pragma unroll
            for (int n = 1; n <= 4; ++n) {         // an n-gram is owned by the lane of its first occurrence, which keeps its count
                const bool valid = lane < L - n + 1;
                key[n - 1] = valid ? w4 & (~0ull << (64 - 16 * n)) : 0ull;
                own[n - 1] = own[n - 1] && valid;
                if (!own[n - 1]) c[n - 1] = 0;
            }
            float w[4];
            idf_of4(keys, idf, G, idf_unseen, key, own, w);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const float v = own[n] ? (float)c[n] * w[n] : 0.f;
                cnt[j][n][lane] = (uint8_t)c[n];
                wt[j][n][lane] = w[n];
                const float nrm = sqrtf(wave_sum(v * v));
                if (lane == 0) norm[j][n] = nrm;
            }
        }
    }
    __syncthreads();

    // ---- pairs: row i as the candidate, the clip's other live rows as its references (LDS is read-only from here to the barrier)
    for (int i = wave; i < per_clip; i += nwaves) {
        float u = 0.f;
        if (alive[i] != 0) {
            const int Lc = len[i];
            const unsigned long long wi = win[i][lane];
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            int nr = 0;
            for (int r = 0; r < per_clip; ++r) {
                if (r == i || alive[r] == 0) continue;
                ++nr;
                const int Lr = len[r];
                const float dl = (float)(Lc - Lr);
                const float gauss = expf(-(dl * dl) * inv_2s2);
                const unsigned long long wr = win[r][lane];
                int cc[4] = {0, 0, 0, 0};          // the candidate's counts of the reference's n-grams that start at this lane
                for (int q = 0; q < Lc; ++q) {
                    const int lead = lead_words(wr ^ lane_key(wi, q));
#pragma unroll
                    for (int n = 1; n <= 4; ++n) cc[n - 1] += lead >= n ? 1 : 0;
                }
#pragma unroll
                for (int n = 1; n <= 4; ++n) {
                    const int c = (int)cnt[r][n - 1][lane];
                    float vr = 0.f, term = 0.f;
                    if (c > 0) {
                        const float w = wt[r][n - 1][lane];
                        vr = (float)c * w;
                        term = fminf((float)cc[n - 1] * w, vr) * vr;
                    }
                    const float dot = wave_sum(term);
                    const float norm_c = norm[i][n - 1], norm_r = norm[r][n - 1];
                    if (norm_c > 0.f && norm_r > 0.f) acc[n - 1] += dot / (norm_c * norm_r) * gauss;
                }
            }
            float po[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) po[n] = nr > 0 ? 10.f * acc[n] / (float)nr : 0.f;
            u = 0.25f * ((po[0] + po[1]) + (po[2] + po[3]));
        }
        if (lane == 0) {
            util[i] = u;
            utility[(size_t)clip * per_clip + i] = u;
        }
    }
    __syncthreads();

    // ---- pick: the first live row with the largest utility, and its ids (every thread walks the <= 32 values alike)
    int p = -1;
    float top = 0.f;
    for (int j = 0; j < per_clip; ++j)
        if (alive[j] != 0 && (p < 0 || util[j] > top)) {
            p = j;
            top = util[j];
        }
    if (p < 0) p = 0;
    if (threadIdx.x == 0) pick[clip] = p;
    if ((int)threadIdx.x < T) best[(size_t)clip * T + threadIdx.x] = rows[(size_t)p * T + threadIdx.x];
}

}  // namespace

extern "C" int cvc_consensus_cider(const int64_t* cand, const int32_t* live, int rows, int T, int per_clip,
                                   const unsigned long long* keys, const float* idf, int G, float idf_unseen, float sigma,
                                   float* utility, int32_t* pick, int64_t* best, cvc_stream_t stream) {
    if (cand == nullptr || utility == nullptr || pick == nullptr || best == nullptr) return CVC_E_BADARG;
    if (rows < 1 || T < 1 || T > MAXT || per_clip < 1 || per_clip > MAX_PER_CLIP || rows % per_clip != 0 || G < 0) return CVC_E_BADARG;
    if (G > 0 && (keys == nullptr || idf == nullptr)) return CVC_E_BADARG;
    if (!(sigma > 0.f)) return CVC_E_BADARG;
    const int nwaves = per_clip < MAX_WAVES ? per_clip : MAX_WAVES;
    const float inv_2s2 = 1.0f / (2.0f * sigma * sigma);
    if (per_clip <= 8)
        hipLaunchKernelGGL(consensus_cider_kernel<8>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream, cand, live, T,
                           per_clip, keys, idf, G, idf_unseen, inv_2s2, utility, pick, best);
    else
        hipLaunchKernelGGL(consensus_cider_kernel<MAX_PER_CLIP>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream, cand,
                           live, T, per_clip, keys, idf, G, idf_unseen, inv_2s2, utility, pick, best);
    return cvc_launch_status();
}
