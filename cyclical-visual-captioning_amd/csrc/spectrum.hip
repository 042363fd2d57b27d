// Spectral caption-set diversity: how much of the spectrum of a clip's m x m caption-similarity matrix its largest eigenvalue holds --
// Self-CIDEr and its count-vector sibling, LSA-based diversity (Wang & Chan, CVPR 2019), by word id
// (cvc.metrics.set_spectrum, cvc.metrics.SpectrumScorer, cvc.cider.CiderD.self_cider, cvc.decode.DecodeEngine.set_spectrum).
//
// cvc_caption_set_spectrum: ONE WORKGROUP per clip, one wave per candidate row at a time (up to 16 waves, rows taken round robin), lane p
//   owns the n-grams (n = 1..4) that start at position p, as consensus_cider_kernel (csrc/consensus.hip) -- hence T <= 63.  A caption's
//   words are the ids BEFORE its first 0 (load_caption<false>, the convention of csrc/diversity.hip): L = 0 is possible.
//   Build pass, once per live row: the 4-word window per position, first-occurrence ownership and counts from one walk over the
//   row's own windows, ONE four-wide search of the idf table (mode cider), and to LDS per order and lane v_n = count * idf at the
//   lane of the n-gram's first occurrence (0 elsewhere) and the four squared norms.  Mode lsa: v_1 = count, no table, no norm.
//   Pair pass: row a against every live row b >= a.  b's positions are walked once: the window of position q is read from LDS by
//   every lane (one address: a broadcast) and compared with the lane's own -- the number of leading words on which the two agree says
//   for all four orders at once whether the n-grams are the same one, and v_n^b[q] is non-zero only where q owns the n-gram in b, so
//   a lane adds at most one product per order.  DPP wave sums, contraction off, orders added in ascending order:
//     cider: s_n = <v_n^a, v_n^b> / sqrt(|v_n^a|^2 |v_n^b|^2) (0 if a norm is 0), K[a, b] = 0.25 (((s_1 + s_2) + s_3) + s_4)
//     lsa:   K[a, b] = <v_1^a, v_1^b>, an integer below 2^24: exact
//   (the square root of the product of the SQUARED norms: for equal rows the dot product is the squared norm bit for bit and
//   sqrt(x * x) = x, so s_n is exactly 1 -- the diagonal is exactly min(L, 4) / 4 and equal captions give an exactly rank-1 K.)
//   K lives in LDS as fp64 at the rows' indices among the live rows (r(a) = the live rows before a), both triangles written from
//   the one value, zero at indices >= m.
//   Solve, one wave: two-sided Jacobi in fp64 in the parallel round-robin ordering -- M = m rounded up to even (the odd one out
//   meets a zero row), M - 1 rounds per sweep, in round r index M - 1 meets r and (r + k) mod (M - 1) meets (r - k) mod (M - 1),
//   k = 1 .. M / 2 - 1: M / 2 disjoint rotations, found by M / 2 lanes, then applied to the (M / 2)^2 2 x 2 blocks at once: a lane
//   takes a block of the upper triangle through J_1^T (B J_2) and writes it and its transpose, so that K stays exactly symmetric.
//   A rotation is skipped when |K_pq| <= 4 * 2^-53 * trace; a sweep without a rotation ends the solve; at most 16 sweeps.  The
//   ordering depends on m alone: the result is bit-reproducible and independent of the launch's other clips.
//   The eigenvalues are rank-sorted in the wave; one lane forms the two scores in fp64 and rounds them once.
//   No atomics, no global workspace, no host read, no allocation; sizes come from the arguments.
#include "cvc_common.h"
#include "caption_ngrams.h"
#include <math.h>

namespace {

using cvc_caption::MAXT;
using cvc_caption::ngram_key;

constexpr int MAX_PER_CLIP = 32;
constexpr int MAX_WAVES = 16;
constexpr int MAX_SWEEPS = 16;

// lane p's value in every lane (p is wave-uniform)
__device__ __forceinline__ unsigned long long lane_key(unsigned long long v, int p) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, p);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), p);
    return ((unsigned long long)hi << 32) | lo;
}

// on how many leading 16-bit words two windows agree, given their exclusive or (4: on all) -- the n-grams of order n that start
// at the two positions are the same one iff this is >= n, provided one of them is an n-gram at all (its n words are non-zero)
__device__ __forceinline__ int lead_words(unsigned long long x) { return x != 0ull ? (int)__builtin_clzll(x) >> 4 : 4; }

// idf of key[n] where own[n], from the sorted table (cider_d_kernel's binary search, hence the same entry) -- the four searches
// advance together, so that their dependent loads overlap; a lane that owns nothing re-reads keys[0]
__device__ __forceinline__ void idf_of4(const unsigned long long* keys, const float* idf, int G, float idf_unseen,
                                        const unsigned long long (&key)[4], const bool (&own)[4], float (&w)[4]) {
    int lo[4], hi[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        lo[n] = 0;
        hi[n] = own[n] ? G : 0;
    }
    int steps = 0;                                 // [0, G) is empty after floor(log2 G) + 1 halvings
    while (steps < 31 && (1u << steps) <= (unsigned)G) ++steps;
    for (int s = 0; s < steps; ++s) {
        unsigned long long k[4];
        int mid[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            mid[n] = (int)(((unsigned)lo[n] + (unsigned)hi[n]) >> 1);
            k[n] = keys[lo[n] < hi[n] ? mid[n] : 0];
        }
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (lo[n] < hi[n]) {
                if (k[n] < key[n]) lo[n] = mid[n] + 1; else hi[n] = mid[n];
            }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) w[n] = idf_unseen;
    if (G > 0) {
        unsigned long long k[4];
        float v[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int at = lo[n] < G ? lo[n] : 0;
            k[n] = keys[at];
            v[n] = idf[at];
        }
#pragma unroll
        for (int n = 0; n < 4; ++n)
            if (lo[n] < G && k[n] == key[n]) w[n] = v[n];
    }
}

// the solving wave's LDS writes before its later reads by other lanes: a wave runs in lock step and its LDS operations complete in
// order, so this only has to keep the compiler from moving memory operations across it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int NMAX>
__global__ __launch_bounds__(64 * (NMAX < MAX_WAVES ? NMAX : MAX_WAVES)) void caption_set_spectrum_kernel(
    const int64_t* cand, const int32_t* live, int T, int per_clip, int mode, const unsigned long long* keys, const float* idf, int G,
    float idf_unseen, float* gram, double* lam, float* score, int32_t* info) {
#pragma clang fp contract(off)
    constexpr int WAVES = NMAX < MAX_WAVES ? NMAX : MAX_WAVES;
    constexpr int HALF = NMAX / 2;
    __shared__ unsigned long long win[NMAX][64];   // the 4-word window that starts at each position (words as id + 1, 0 past the end)
    __shared__ float v[NMAX][4][64];               // count * idf of the n-gram that starts here, at the lane of its first occurrence
    __shared__ float nsq[NMAX][4];                 // |v_n|^2
    __shared__ double A[NMAX][NMAX];               // K at the live rows' indices, then the solve's working matrix
    __shared__ double rot[HALF][3];                // a round's rotations: c, s, t
    __shared__ int pq[HALF][2];                    // and their index pairs, p < q
    __shared__ double eig[NMAX];
    __shared__ int len[NMAX];
    __shared__ int alive[NMAX];
    __shared__ int ridx[NMAX];                     // the live rows before this one
    __shared__ uint32_t sw[WAVES][68];
    const int clip = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t* rows = cand + (size_t)clip * per_clip * T;
    if ((int)threadIdx.x < per_clip) alive[threadIdx.x] = live == nullptr || live[(size_t)clip * per_clip + threadIdx.x] != 0 ? 1 : 0;
    for (int i = threadIdx.x; i < NMAX * NMAX; i += blockDim.x) (&A[0][0])[i] = 0.0;
    __syncthreads();
    if ((int)threadIdx.x < per_clip) {
        int before = 0;
        for (int j = 0; j < (int)threadIdx.x; ++j) before += alive[j];
        ridx[threadIdx.x] = before;
    }
    int m = 0;
    for (int j = 0; j < per_clip; ++j) m += alive[j];

    // ---- build: every live row's vectors, once (the trip count is the same for every wave: the loader holds workgroup barriers)
    for (int j0 = 0; j0 < per_clip; j0 += nwaves) {
        const int j = j0 + wave;
        const bool active = j < per_clip && alive[j] != 0;
        const int L = cvc_caption::load_caption<false>(active ? rows + (size_t)j * T : rows, active ? T : 0, lane, sw[wave]);
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
            float w[4] = {1.f, 0.f, 0.f, 0.f};     // mode lsa: unigram counts
            if (mode == 0) idf_of4(keys, idf, G, idf_unseen, key, own, w);
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const float val = own[n] ? (float)c[n] * w[n] : 0.f;
                v[j][n][lane] = val;
                const float sq = wave_sum(val * val);
                if (lane == 0) nsq[j][n] = sq;
            }
        }
    }
    __syncthreads();

    // ---- pairs: row a against every live row b >= a (windows, vectors and norms are read-only from here on)
    for (int a = wave; a < per_clip; a += nwaves) {
        if (alive[a] == 0) continue;
        const unsigned long long wa = win[a][lane];
        float va[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) va[n] = v[a][n][lane];
        const int ra = ridx[a];
        for (int b = a; b < per_clip; ++b) {
            if (alive[b] == 0) continue;
            const int Lb = len[b];
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            for (int q = 0; q < Lb; ++q) {
                const int lead = lead_words(wa ^ win[b][q]);
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[n] += lead > n ? va[n] * v[b][n][q] : 0.f;
            }
            float k;
            if (mode == 0) {
                float s[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float dot = wave_sum(acc[n]);
                    const float qa = nsq[a][n], qb = nsq[b][n];
                    s[n] = qa > 0.f && qb > 0.f ? dot / sqrtf(qa * qb) : 0.f;
                }
                k = 0.25f * (((s[0] + s[1]) + s[2]) + s[3]);
            } else {
                k = wave_sum(acc[0]);
            }
            if (lane == 0) {
                const int rb = ridx[b];
                A[ra][rb] = (double)k;
                A[rb][ra] = (double)k;
            }
        }
    }
    __syncthreads();

    if (gram != nullptr) {
        float* g = gram + (size_t)clip * MAX_PER_CLIP * MAX_PER_CLIP;
        for (int i = threadIdx.x; i < MAX_PER_CLIP * MAX_PER_CLIP; i += blockDim.x) {
            const int r = i / MAX_PER_CLIP, c = i % MAX_PER_CLIP;
            g[i] = r < m && c < m ? (float)A[r][c] : 0.f;
        }
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- solve: one wave, two-sided Jacobi, parallel round-robin ordering
    double tr = 0.0;
    for (int i = 0; i < m; ++i) tr += A[i][i];
    const double thr = 4.0 * 0x1p-53 * tr;
    const int M = (m + 1) & ~1, half = M >> 1;
    int sweeps = 0;
    bool settled = false;
    while (sweeps < MAX_SWEEPS && !settled) {
        unsigned long long rotated = 0ull;
        for (int r = 0; r < M - 1; ++r) {
            bool turn = false;
            if (lane < half) {
                const int x = lane == 0 ? M - 1 : (r + lane) % (M - 1);
                const int y = lane == 0 ? r : (r - lane + (M - 1)) % (M - 1);
                const int p = x < y ? x : y, q = x < y ? y : x;
                const double apq = A[p][q];
                double c = 1.0, s = 0.0, t = 0.0;
                if (fabs(apq) > thr) {
                    const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    turn = true;
                }
                rot[lane][0] = c;
                rot[lane][1] = s;
                rot[lane][2] = t;
                pq[lane][0] = p;
                pq[lane][1] = q;
            }
            const unsigned long long now = __ballot(turn);
            rotated |= now;
            wave_sync();
            if (now != 0ull) {
                for (int i = lane; i < half * half; i += 64) {
                    const int k1 = i / half, k2 = i % half;
                    if (k1 > k2) continue;
                    const int p1 = pq[k1][0], q1 = pq[k1][1];
                    if (k1 == k2) {
                        const double t = rot[k1][2];
                        if (rot[k1][1] != 0.0) {
                            const double apq = A[p1][q1];
                            A[p1][p1] = A[p1][p1] - t * apq;
                            A[q1][q1] = A[q1][q1] + t * apq;
                            A[p1][q1] = 0.0;
                            A[q1][p1] = 0.0;
                        }
                        continue;
                    }
                    const int p2 = pq[k2][0], q2 = pq[k2][1];
                    const double c1 = rot[k1][0], s1 = rot[k1][1], c2 = rot[k2][0], s2 = rot[k2][1];
                    const double b00 = A[p1][p2], b01 = A[p1][q2], b10 = A[q1][p2], b11 = A[q1][q2];
                    const double t00 = c2 * b00 - s2 * b01, t01 = s2 * b00 + c2 * b01;
                    const double t10 = c2 * b10 - s2 * b11, t11 = s2 * b10 + c2 * b11;
                    const double r00 = c1 * t00 - s1 * t10, r10 = s1 * t00 + c1 * t10;
                    const double r01 = c1 * t01 - s1 * t11, r11 = s1 * t01 + c1 * t11;
                    A[p1][p2] = r00;
                    A[p2][p1] = r00;
                    A[p1][q2] = r01;
                    A[q2][p1] = r01;
                    A[q1][p2] = r10;
                    A[p2][q1] = r10;
                    A[q1][q2] = r11;
                    A[q2][q1] = r11;
                }
            }
            wave_sync();
        }
        ++sweeps;
        settled = rotated == 0ull;
    }

    // ---- the eigenvalues in descending order (equal values keep their index order), zeros behind them
    if (lane < m) {
        const double d = A[lane][lane];
        int rank = 0;
        for (int j = 0; j < m; ++j) {
            const double e = A[j][j];
            rank += e > d || (e == d && j < lane) ? 1 : 0;
        }
        eig[rank] = d;
    }
    wave_sync();
    if (lane < MAX_PER_CLIP) lam[(size_t)clip * MAX_PER_CLIP + lane] = lane < m ? eig[lane] : 0.0;
    if (lane == 0) {
        double s0 = 0.0, s1 = 0.0;
        if (m >= 2 && tr > 0.0) {
            const double top = eig[0], logm = log((double)m);
            double roots = 0.0;
            for (int i = 0; i < m; ++i) roots += sqrt(eig[i] > 0.0 ? eig[i] : 0.0);
            const double share = top / tr;
            s0 = -log(share < 1.0 ? share : 1.0) / logm + 0.0;
            s1 = top > 0.0 ? -log(sqrt(top) / roots) / logm + 0.0 : 0.0;
        }
        score[(size_t)clip * 2] = (float)s0;
        score[(size_t)clip * 2 + 1] = (float)s1;
        info[(size_t)clip * 2] = m;
        info[(size_t)clip * 2 + 1] = settled ? sweeps : -1;
    }
}

}  // namespace

extern "C" int cvc_caption_set_spectrum(const int64_t* cand, const int32_t* live, int rows, int T, int per_clip, int mode,
                                        const unsigned long long* keys, const float* idf, int G, float idf_unseen, float* gram,
                                        double* lam, float* score, int32_t* info, cvc_stream_t stream) {
    if (cand == nullptr || lam == nullptr || score == nullptr || info == nullptr) return CVC_E_BADARG;
    if (rows < 1 || T < 1 || T > MAXT || per_clip < 1 || per_clip > MAX_PER_CLIP || rows % per_clip != 0) return CVC_E_BADARG;
    if (mode != 0 && mode != 1) return CVC_E_BADARG;
    if (mode == 0 && (G < 0 || (G > 0 && (keys == nullptr || idf == nullptr)))) return CVC_E_BADARG;
    const int nwaves = per_clip < MAX_WAVES ? per_clip : MAX_WAVES;
    if (per_clip <= 8)
        hipLaunchKernelGGL(caption_set_spectrum_kernel<8>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream, cand, live,
                           T, per_clip, mode, keys, idf, G, idf_unseen, gram, lam, score, info);
    else
        hipLaunchKernelGGL(caption_set_spectrum_kernel<MAX_PER_CLIP>, dim3(rows / per_clip), dim3(64 * nwaves), 0, (hipStream_t)stream,
                           cand, live, T, per_clip, mode, keys, idf, G, idf_unseen, gram, lam, score, info);
    return cvc_launch_status();
}
