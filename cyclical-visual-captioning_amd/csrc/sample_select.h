// The selection kernel of sampled decoding and the one function behind its entry points, shared by csrc/sample.hip
// (cvc_sample_select_parts / cvc_sample_select_trunc_parts: contract in that file's header comment) and csrc/constrain.hip
// (cvc_constrained_select_parts: the CONS flag of the same kernel, contract in that file) and csrc/mix.hip (cvc_mixed_select_parts:
// the MIX flag, scheduled sampling's drawn-or-given word, contract in that file).  One definition of the hash counters, the
// noise, the candidate mask, the truncation search and the log-prob: every form rounds alike.  The row loader, the shared argument
// checks and the NC / NP / VEC dispatch are those of every selection block (csrc/select_row.h).
#pragma once
#include "select_row.h"
#include "ban_set.h"
#include "dropout_rng.h"
#include <math.h>

namespace {

constexpr uint32_t KEY_NEG_INF = 0x007fffffu;  // key of -inf: no float compares below it

// what the truncating form of the kernel takes on top of the plain one's arguments (the plain one: nothing)
struct NoTrunc {};
struct TruncArgs { int top_k; float top_p; float* cutoff; int32_t* kept; };
template <bool TRUNC> struct trunc_args { using type = NoTrunc; };
template <> struct trunc_args<true> { using type = TruncArgs; };

// what the constrained form takes on top (csrc/constrain.hip): ConsArgs of csrc/ban_set.h, the row's history and the rules

// what the mixed form takes on top (csrc/mix.hip): the given word per row, the probability of taking the drawn one (device memory),
// the coin's hash site and the nullable outputs
struct NoMix {};
struct MixArgs { const int64_t* given; int given_stride; const float* mix_prob; uint32_t site; int64_t* drawn; uint8_t* took; float* given_logprob; };
template <bool MIX> struct mix_args { using type = NoMix; };
template <> struct mix_args<true> { using type = MixArgs; };

// the float of an order-preserving key: key(a) < key(b) <=> a < b over the non-NaN floats (-0 below +0; keys above key(+inf) and
// below KEY_NEG_INF are NaNs)
__device__ __forceinline__ float unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// the Gumbel perturbation of hash value h (its 23 high bits)
__device__ __forceinline__ float gumbel(uint32_t h) {
    const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;
    return -logf(-logf(u));
}

// NC / NP / VEC: the loader form (csrc/select_row.h).  The candidates are the words whose register slot is not in the thread's
// `banned` mask: UNK, and with CONS the row's whole ban set (a V-bit map in LDS, built from the history and the lists: csrc/ban_set.h).
// TRUNC: the cutoff search of the header comment in front of the Gumbel-max; the noise is then drawn for the kept words only.
// CONS: inv_tau == 0 is the arg-max mode (s = z, no noise, state unread).
// MIX: the plain form's draw, then a per-row coin decides whether the drawn or the given word is written (contract: csrc/mix.hip);
// the given word's logit is published by its owner during the scan and scored against the row's own max / sum-exp.
template <int NC, int NP, bool VEC, bool TRUNC, bool CONS, bool MIX = false>
__global__ __launch_bounds__(WG) void sample_select_kernel(const float* parts, int nparts, long long part_stride, const float* bias,
                                                           int V, int unk, float inv_tau, const uint32_t* state, uint32_t site,
                                                           int64_t* word, int wstride, float* logprob,
                                                           typename trunc_args<TRUNC>::type ta,
                                                           typename cons_args<CONS>::type ca,
                                                           typename mix_args<MIX>::type ma) {
#pragma clang fp contract(off)
    static_assert(!MIX || (!TRUNC && !CONS), "the mixed form draws from the plain distribution");
    __shared__ float red_m[4], red_s[4], red_v[4], red_z[4];
    __shared__ int red_i[4];
    [[maybe_unused]] __shared__ int red_b[4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool noisy = !CONS || inv_tau != 0.f;
    uint32_t seed_lo = 0, seed_hi = 0, call = 0;
    if (noisy) { seed_lo = state[0]; seed_hi = state[1]; call = state[2]; }
    float z[NC];
    load_logit_row<NC, NP, VEC>(parts + (size_t)row * V, nparts, part_stride, bias, V, tid, z);
    auto col = [&](int u) { return ::col<VEC>(tid, u); };
    [[maybe_unused]] __shared__ float zg_pub;              // MIX: the given word's logit, read by thread 0 after the barriers below
    [[maybe_unused]] int g = -1;                           // MIX: the given word, -1 outside [0, V) (uniform over the workgroup)
    if constexpr (MIX) {
        const int64_t g64 = ma.given[(size_t)row * ma.given_stride];
        g = (g64 >= 0 && g64 < (int64_t)V) ? (int)g64 : -1;
    }
    // bit u of `banned` = the word of register slot u is not a candidate: UNK, with CONS any word of the row's ban set
    static_assert(NC <= 32, "one ban bit per register slot");
    uint32_t banned = 0;
    if constexpr (CONS) {
        __shared__ uint32_t bits[WG];                       // V <= 32 * WG
        __shared__ long long hist[CONS_T_MAX];
        build_ban_map<WG>(ca, load_hist_step(ca, row, tid), V, unk, tid, bits, hist);   // (both barriers inside)
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int v = col(u);
            if (v < V && ((bits[v >> 5] >> (v & 31)) & 1u)) banned |= 1u << u;
        }
        const int nb = wave_sum_int(__popc(bits[tid]));
        if (lane == 0) red_b[wave] = nb;                    // read by thread 0 after the barriers below
    } else {
        banned = slot_bit<VEC>(tid, unk, V);                // the one slot with col(u) == unk, without NC compares
    }
    // perturbed scores: the best (s, v) and its logit; the row's maximum logit
    float bs = -INFINITY, bz = -INFINITY, m = -INFINITY;
    int bi = 0x7fffffff;
    const uint32_t base = (uint32_t)row * (uint32_t)V;
    [[maybe_unused]] float theta = -INFINITY, se_full = 0.f, nkept = 0.f, zmin = INFINITY;
    if constexpr (TRUNC) {
        __shared__ float red_c[4], red_p[2][4];
        // the row's maximum (banned words included: the log-prob's) and the candidates' maximum
        float mc = -INFINITY;
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            m = fmaxf(m, z[u]);
            mc = fmaxf(mc, ((banned >> u) & 1u) ? -INFINITY : z[u]);
        }
        m = wave_max(m);
        mc = wave_max(mc);
        if (lane == 0) { red_m[wave] = m; red_c[wave] = mc; }
        __syncthreads();
        m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        mc = fmaxf(fmaxf(red_c[0], red_c[1]), fmaxf(red_c[2], red_c[3]));
        // the thread's share of the log-sum-exp over the full row (the plain form's terms in its order) is taken now; then every banned
        // slot holds -inf like the padding (neither is ever counted: no probe runs at a cutoff of -inf, the last pass tests the mask)
        if (m != -INFINITY) {
#pragma unroll
            for (int u = 0; u < NC; ++u) se_full += expf(z[u] - m);          // padding: exp(-inf) = 0
        }
#pragma unroll
        for (int u = 0; u < NC; ++u)
            if ((banned >> u) & 1u) z[u] = -INFINITY;
        // workgroup sum in a fixed order; alternating slots: one barrier per probe
        int slot = 0;
        auto wg_sum = [&](float x) {
            x = wave_sum(x);
            float* r = red_p[slot];
            slot ^= 1;
            if (lane == 0) r[wave] = x;
            __syncthreads();
            return (r[0] + r[1]) + (r[2] + r[3]);
        };
        if (mc > -INFINITY) {                              // a candidate with a finite logit exists (NaN logits compare false: never kept)
            if (ta.top_k > 0) {
                const float fk = (float)ta.top_k;          // counts are <= 8192: exact in fp32
                uint32_t T = 0;
                for (int b = 31; b >= 0; --b) {
                    const uint32_t c = T | (1u << b);
                    if (c <= KEY_NEG_INF) { T = c; continue; }      // every candidate is >= -inf
                    const float th = unkey(c);
                    float n = 0.f;
#pragma unroll
                    for (int u = 0; u < NC; ++u) n += (z[u] >= th) ? 1.f : 0.f;
                    n = wg_sum(n);
                    if (n >= fk) {
                        T = c;
                        if (n == fk) break;                // exactly k at or above th: that set is C1 (ties compare equal)
                    }
                }
                theta = unkey(T);
            }
            if (ta.top_p < 1.f) {
                float e[NC], tot = 0.f;
#pragma unroll
                for (int u = 0; u < NC; ++u) {
                    e[u] = (z[u] >= theta) ? expf((z[u] - mc) * inv_tau) : 0.f;
                    tot += e[u];
                }
                tot = wg_sum(tot);
                const float need = ta.top_p * tot;         // <= tot: the predicate holds at the lowest cutoff (same sum, same order)
                uint32_t T = 0;
                for (int b = 31; b >= 0; --b) {
                    const uint32_t c = T | (1u << b);
                    if (c <= KEY_NEG_INF) { T = c; continue; }
                    const float th = unkey(c);
                    float s = 0.f;
#pragma unroll
                    for (int u = 0; u < NC; ++u) s += (z[u] >= th) ? e[u] : 0.f;
                    s = wg_sum(s);
                    if (s >= need) T = c;
                }
                theta = fmaxf(theta, unkey(T));
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        const int v = col(u);
        if (v < V) {
            if constexpr (!TRUNC) m = fmaxf(m, z[u]);
            if constexpr (MIX) { if (v == g) zg_pub = z[u]; }
            bool cand = !((banned >> u) & 1u);
            if constexpr (TRUNC) cand = z[u] >= theta && cand;          // this order: one branch per slot (profiles/select_blocks_merge.md)
            if (cand) {
                float s;
                if (noisy) s = z[u] * inv_tau + gumbel(cvc_drop_hash(seed_lo, seed_hi, call, site, base + (uint32_t)v));
                else s = z[u];
                if (better(s, v, bs, bi)) { bs = s; bi = v; bz = z[u]; }
                if constexpr (TRUNC) { nkept += 1.f; zmin = fminf(zmin, z[u]); }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(bs, o, 64), oz = __shfl_xor(bz, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(os, oi, bs, bi)) { bs = os; bi = oi; bz = oz; }
    }
    if constexpr (TRUNC) {
        __shared__ float red_k[4], red_n[4];
        nkept = wave_sum(nkept);
        zmin = -wave_max(-zmin);
        if (lane == 0) { red_k[wave] = nkept; red_n[wave] = zmin; red_v[wave] = bs; red_i[wave] = bi; red_z[wave] = bz; }
        __syncthreads();
        nkept = (red_k[0] + red_k[1]) + (red_k[2] + red_k[3]);
        zmin = fminf(fminf(red_n[0], red_n[1]), fminf(red_n[2], red_n[3]));
    } else {
        m = wave_max(m);
        if (lane == 0) { red_m[wave] = m; red_v[wave] = bs; red_i[wave] = bi; red_z[wave] = bz; }
        __syncthreads();
        m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    }
    float se = se_full;
    if (!TRUNC && m != -INFINITY) {
#pragma unroll
        for (int u = 0; u < NC; ++u) se += expf(z[u] - m);          // padding: exp(-inf) = 0
    }
    se = wave_sum(se);
    if (lane == 0) red_s[wave] = se;
    __syncthreads();
    if (tid == 0) {
        bs = red_v[0]; bi = red_i[0]; bz = red_z[0];
        for (int w = 1; w < 4; ++w)
            if (better(red_v[w], red_i[w], bs, bi)) { bs = red_v[w]; bi = red_i[w]; bz = red_z[w]; }
        const float S = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
        int w = bi;
        if (w < 0 || w >= V) w = 0;        // every score NaN: nothing compared better; the word is a gather index next step
        if constexpr (MIX) {
            // the coin: its own site, the row as counter; u is exact in fp32 and strictly inside (0, 1): p = 0 never takes, p = 1 always
            const uint32_t hc = cvc_drop_hash(seed_lo, seed_hi, call, ma.site, (uint32_t)row);
            const bool took = ((float)(hc >> 9) + 0.5f) * 0x1p-23f < *ma.mix_prob;
            if (ma.drawn != nullptr) ma.drawn[row] = w;
            if (ma.took != nullptr) ma.took[row] = took ? 1 : 0;
            // the forced block's definition and bits (csrc/forced.hip): same m, same S; a given word outside [0, V) scores NaN
            if (ma.given_logprob != nullptr) ma.given_logprob[row] = g >= 0 ? zg_pub - (m + logf(S)) : __builtin_nanf("");
            word[(size_t)row * wstride] = took ? w : (g >= 0 ? g : 0);
        } else {
            word[(size_t)row * wstride] = w;
        }
        if (logprob != nullptr) logprob[row] = bz - (m + logf(S));
        if constexpr (CONS) {
            if (ca.nbanned != nullptr) ca.nbanned[row] = (red_b[0] + red_b[1]) + (red_b[2] + red_b[3]);
        }
        if constexpr (TRUNC) {
            if (ta.cutoff != nullptr) ta.cutoff[row] = zmin;
            if (ta.kept != nullptr) ta.kept[row] = (int32_t)nkept;
        }
    }
}

}  // namespace

// argument checks of the entry points on top of select_row_check (argmax: the constrained block's mode without noise, inv_tau == 0
// and no state)
static int select_check(const float* parts, int nparts, long long part_stride, int M, int V, float inv_tau, const uint32_t* rng_state,
                        int t, const int64_t* word, int word_stride, bool argmax = false) {
    if ((!rng_state && !argmax) || t < 0) return CVC_E_BADARG;
    if (!argmax && (!(inv_tau > 0.f) || !isfinite(inv_tau))) return CVC_E_BADARG;
    return select_row_check(parts, nparts, part_stride, M, V, word, word_stride);
}

// behind every entry point, after select_check: the top_k / top_p rules and the choice of form.  cutoff / kept asked for without
// truncation: the truncating form with both searches off fills them from C0 (same word, same bits as the plain form)
template <bool CONS>
static int select_run(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V, int unk_idx, float inv_tau,
                      int top_k, float top_p, const uint32_t* rng_state, int t, int64_t* word, int word_stride, float* logprob,
                      float* cutoff, int32_t* kept, cvc_stream_t stream, typename cons_args<CONS>::type ca = {}) {
    if (top_k < 0 || !isfinite(top_p) || !(top_p > 0.f) || top_p > 1.f) return CVC_E_BADARG;
    if (top_k >= V - 1) top_k = 0;                         // |C0| <= V - 1: C1 = C0
    const bool trunc = top_k > 0 || top_p < 1.f;
    if (inv_tau == 0.f && trunc) return CVC_E_BADARG;      // the arg-max mode: no distribution to truncate
    const uint32_t site = CVC_SAMPLE_SITE + (uint32_t)t;
    auto launch = [&](auto trunc_, auto ta) {
        select_dispatch(parts, nparts, part_stride, bias, V, [&](auto nc, auto np, auto vec) {
            hipLaunchKernelGGL((sample_select_kernel<decltype(nc)::value, decltype(np)::value, decltype(vec)::value,
                                                     decltype(trunc_)::value, CONS>),
                               dim3(M), dim3(WG), 0, (hipStream_t)stream, parts, nparts, part_stride, bias, V, unk_idx, inv_tau, rng_state,
                               site, word, word_stride, logprob, ta, ca, NoMix{});
        });
    };
    if (trunc || cutoff != nullptr || kept != nullptr) launch(std::true_type{}, TruncArgs{top_k, top_p, cutoff, kept});
    else launch(std::false_type{}, NoTrunc{});
    return cvc_launch_status();
}
