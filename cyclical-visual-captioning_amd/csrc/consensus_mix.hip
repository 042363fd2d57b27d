// Consensus (minimum-Bayes-risk) caption selection under a weighted mix of utilities: among a clip's candidates keep the one with the
// highest expected utility against the clip's other candidates, each of them one reference weighted by its (model) probability
// (cvc.metrics.consensus, cvc.decode.DecodeEngine.consensus with a utility mix or weights="model").
//
// cvc_consensus_mix: ONE WORKGROUP per clip, laid out as consensus_cider_kernel (csrc/consensus.hip): one wave per candidate row at a
//   time (up to 16 waves, rows taken round robin), lane p owns the n-grams (n = 1..4) that start at position p -- hence T <= 63.
//   Build pass, once per row: consensus_cider_kernel's, statement by statement -- the caption's words with the end mark counted, its
//   4-word window per position, per order and position the count of the n-gram at the lane of its first occurrence, its idf from
//   one binary search, the four norms -- plus the caption's length WITHOUT the end mark (BLEU's and ROUGE-L's words) and the row's
//   weight.  Without a CIDEr coefficient the table is not read at all.
//   Pair pass: row i as the candidate, every other live row j as its ONLY reference, j ascending.  One walk over the candidate's
//   positions answers everything: the window of one position after the other is broadcast (readlane) and compared with the lane's
//   own reference window -- the number of leading words on which they agree (clz / 16) gives the candidate's count of the
//   reference's n-gram of every order at once, for CIDEr-D's clipped dot products and for BLEU's clipped counts alike (an n-gram
//   that lies before the reference's end mark matches only n-grams before the candidate's, so one count serves both); the broadcast
//   window's first word is the candidate's word for the bit-vector LCS (Allison & Dix / Hyyro, as csrc/overlap.hip) on the way.
//     cider(i; j)   cider_d_kernel's expressions with one reference (csrc/cider.hip; words up to and including the first 0)
//     bleu_k(i; j)  caption_overlap_kernel's expressions with one reference (csrc/overlap.hip; words before the first 0): the sum over
//                   the distinct n-grams of min(count_i, count_j) is taken at the reference's lanes here and at the candidate's there --
//                   the same integer -- and everything floating-point is formed from integers by the same expressions
//     rouge(i; j)   caption_overlap_kernel's, likewise
//     u(i, j) = sum_k coef_k metric_k(i; j) over the coefficients > 0, in the order cider, bleu1..4, rougel
//     w_j = exp(logw_j - max over the clip's live rows of logw) (1 at the maximum, 0 at -inf or NaN; without logw: 1)
//     utility[i] = (sum_j w_j u(i, j)) / (sum_j w_j), both sums over the live j != i in ascending order, rounded term by term; 0 for
//     a dead row, a row without another live row, and a zero denominator.  fp32, contraction off.
//   Pick pass: the first live row with the largest utility (0 without a live row), and that row's T ids copied to best.
//   No atomics, no global workspace: a clip's outputs are bit-reproducible and independent of the launch's other clips.
//   LDS per workgroup: 1828 bytes per row + 4352; the kernel is instantiated for <= 8 and <= 32 rows per clip (18 976 / 62 848 bytes).
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
constexpr int NMETRIC = 6;                         // cider, bleu1..4, rougel (cvc.metrics.REWARD_NAMES)

struct Coef { float c[NMETRIC]; };

template <int NMAX>
__global__ __launch_bounds__(64 * MAX_WAVES) void consensus_mix_kernel(const int64_t* cand, const int32_t* live, const float* logw, int T,
                                                                       int per_clip, const unsigned long long* keys, const float* idf,
                                                                       int G, float idf_unseen, float inv_2s2, Coef coef, float* utility,
                                                                       int32_t* pick, int64_t* best, float* pairs) {
#pragma clang fp contract(off)
    __shared__ unsigned long long win[NMAX][64];   // the 4-word window that starts at each position (words as id + 1, 0 past the end)
    __shared__ float wt[NMAX][4][64];              // idf of the n-gram that starts here, at the lane of its first occurrence
    __shared__ uint8_t cnt[NMAX][4][64];           // its count in the caption there, 0 at every other lane
    __shared__ float norm[NMAX][4];
    __shared__ int len[NMAX];                      // words, the end mark counted (CIDEr-D)
    __shared__ int lenb[NMAX];                     // words before the end mark (BLEU, ROUGE-L)
    __shared__ int alive[NMAX];
    __shared__ float wgt[NMAX];
    __shared__ float util[NMAX];
    __shared__ uint32_t sw[MAX_WAVES][68];
    const int clip = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const size_t row0 = (size_t)clip * per_clip;
    const int64_t* rows = cand + row0 * T;
    const bool use_cider = coef.c[0] > 0.f;
    const bool use_bleu = coef.c[1] > 0.f || coef.c[2] > 0.f || coef.c[3] > 0.f || coef.c[4] > 0.f;
    const bool use_rouge = coef.c[5] > 0.f;
    if ((int)threadIdx.x < per_clip) {
        const int me = threadIdx.x;
        const bool on = live == nullptr || live[row0 + me] != 0;
        float w = on ? 1.f : 0.f;
        if (on && logw != nullptr) {               // the largest log-weight among the clip's live rows (NaN counts as -inf)
            float top = -INFINITY;
            for (int j = 0; j < per_clip; ++j)
                if (live == nullptr || live[row0 + j] != 0) {
                    const float l = logw[row0 + j];
                    top = fmaxf(top, l != l ? -INFINITY : l);
                }
            const float l = logw[row0 + me];
            w = (l != l || l == -INFINITY) ? 0.f : (l == top ? 1.f : expf(l - top));
        }
        alive[me] = on ? 1 : 0;
        wgt[me] = w;
    }
    __syncthreads();

    // ---- build: every live row's vectors, once (the trip count is the same for every wave: the loader holds workgroup barriers)
    for (int j0 = 0; j0 < per_clip; j0 += nwaves) {
        const int j = j0 + wave;
        const bool active = j < per_clip && alive[j] != 0;
        const int L = cvc_caption::load_caption<true>(active ? rows + (size_t)j * T : rows, active ? T : 0, lane, sw[wave]);
        if (active) {
            const unsigned long long w4 = ngram_key(sw[wave], lane, 4);
            win[j][lane] = w4;
            if (lane == 0) {
                len[j] = L;
                lenb[j] = L - (sw[wave][L - 1] == 1u ? 1 : 0);       // (the end mark is word 0 + 1; every other word is >= 2)
            }
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
            float w[4] = {0.f, 0.f, 0.f, 0.f};
            if (use_cider) idf_of4(keys, idf, G, idf_unseen, key, own, w);
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

    // ---- pairs: row i as the candidate, each other live row as its only reference (LDS is read-only from here to the barrier)
    for (int i = wave; i < per_clip; i += nwaves) {
        float u_row = 0.f;
        const bool on_i = alive[i] != 0;
        const int Lc = on_i ? len[i] : 0, Lbc = on_i ? lenb[i] : 0;
        const unsigned long long wi = on_i ? win[i][lane] : 0ull;
        float num = 0.f, den = 0.f;
        for (int r = 0; r < per_clip; ++r) {
            float m[NMETRIC] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (on_i && r != i && alive[r] != 0) {
                const int Lr = len[r], Lbr = lenb[r];
                const unsigned long long wr = win[r][lane];
                const uint32_t mine = (uint32_t)(wr >> 48);
                int cc[4] = {0, 0, 0, 0};          // the candidate's counts of the reference's n-grams that start at this lane
                unsigned long long V = ~0ull;      // bit j of ~V: the LCS row rises at reference column j
                for (int q = 0; q < Lc; ++q) {
                    const unsigned long long x = lane_key(wi, q);
                    const int lead = lead_words(wr ^ x);
#pragma unroll
                    for (int n = 1; n <= 4; ++n) cc[n - 1] += lead >= n ? 1 : 0;
                    if (use_rouge && q < Lbc) {
                        const unsigned long long M = __ballot(lane < Lbr && mine == (uint32_t)(x >> 48));
                        const unsigned long long U = V & M;
                        V = (V + U) | (V - U);
                    }
                }
                if (use_cider) {                   // cider_d_kernel with nr = 1
                    const float dl = (float)(Lc - Lr);
                    const float gauss = expf(-(dl * dl) * inv_2s2);
                    float acc[4] = {0.f, 0.f, 0.f, 0.f};
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
                    float po[4];
#pragma unroll
                    for (int n = 0; n < 4; ++n) po[n] = 10.f * acc[n] / 1.f;
                    m[0] = 0.25f * ((po[0] + po[1]) + (po[2] + po[3]));
                }
                if (use_bleu) {                    // caption_overlap_kernel with nr = 1: ref_len = Lbr
                    int correct[4], guess[4];
#pragma unroll
                    for (int n = 0; n < 4; ++n) {
                        const int c = (int)cnt[r][n][lane];
                        correct[n] = wave_sum_int(lane < Lbr - n ? (c < cc[n] ? c : cc[n]) : 0);
                        guess[n] = Lbc - n > 0 ? Lbc - n : 0;
                    }
                    if (Lbc > 0) {
                        const float bp = Lbc >= Lbr ? 1.f : expf(1.f - (float)Lbr / (float)Lbc);
                        float logs = 0.f;
#pragma unroll
                        for (int n = 0; n < 4; ++n) {
                            logs += logf(((float)correct[n] + 1e-15f) / ((float)guess[n] + 1e-9f));
                            if (coef.c[1 + n] > 0.f) m[1 + n] = bp * expf(logs / (float)(n + 1));
                        }
                    }
                }
                if (use_rouge) {
                    const int l = __popcll(~V & ((1ull << Lbr) - 1ull));         // (Lbr <= 63)
                    float q = 0.f;
                    if (Lbr > 0) q = fmaxf(q, (float)l / (float)Lbr);
                    if (Lbc > 0 && l > 0) {
                        const float beta2 = 1.2f * 1.2f;
                        const float p = (float)l / (float)Lbc;
                        m[5] = (1.f + beta2) * p * q / (q + beta2 * p);
                    }
                }
                float u = 0.f;
#pragma unroll
                for (int k = 0; k < NMETRIC; ++k)
                    if (coef.c[k] > 0.f) u += coef.c[k] * m[k];
                const float w = wgt[r];
                num += w * u;
                den += w;
            }
            if (pairs != nullptr && lane == 0) {
                float* out = pairs + ((row0 + i) * per_clip + r) * NMETRIC;
#pragma unroll
                for (int k = 0; k < NMETRIC; ++k) out[k] = m[k];
            }
        }
        if (den > 0.f) u_row = num / den;
        if (lane == 0) {
            util[i] = u_row;
            utility[row0 + i] = u_row;
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

extern "C" int cvc_consensus_mix(const int64_t* cand, const int32_t* live, const float* logw, int rows, int T, int per_clip,
                                 const unsigned long long* keys, const float* idf, int G, float idf_unseen, float sigma,
                                 const float* coef, float* utility, int32_t* pick, int64_t* best, float* pairs, cvc_stream_t stream) {
    if (cand == nullptr || coef == nullptr || utility == nullptr || pick == nullptr || best == nullptr) return CVC_E_BADARG;
    if (rows < 1 || T < 1 || T > MAXT || per_clip < 1 || per_clip > MAX_PER_CLIP || rows % per_clip != 0) return CVC_E_BADARG;
    Coef c;
    bool any = false;
    for (int k = 0; k < NMETRIC; ++k) {
        if (!(coef[k] >= 0.f) || isinf(coef[k])) return CVC_E_BADARG;
        c.c[k] = coef[k];
        any = any || coef[k] > 0.f;
    }
    if (!any) return CVC_E_BADARG;
    float inv_2s2 = 0.f;
    if (c.c[0] > 0.f) {                            // the table counts only with a CIDEr coefficient
        if (!(sigma > 0.f) || G < 0 || (G > 0 && (keys == nullptr || idf == nullptr))) return CVC_E_BADARG;
        inv_2s2 = 1.0f / (2.0f * sigma * sigma);
    }
    const int nwaves = per_clip < MAX_WAVES ? per_clip : MAX_WAVES;
    if (per_clip <= 8)
        hipLaunchKernelGGL(consensus_mix_kernel<8>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream, cand, live, logw, T,
                           per_clip, keys, idf, G, idf_unseen, inv_2s2, c, utility, pick, best, pairs);
    else
        hipLaunchKernelGGL(consensus_mix_kernel<MAX_PER_CLIP>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream, cand, live,
                           logw, T, per_clip, keys, idf, G, idf_unseen, inv_2s2, c, utility, pick, best, pairs);
    return cvc_launch_status();
}
