// Self-critical training on captions sampled WITHOUT replacement (stochastic beam search, csrc/beam.hip): importance weights, a
// per-row baseline and the per-token loss weights of a clip's S rollouts, one launch.  The estimator of Kool, van Hoof and Welling
// 2019 ("Stochastic Beams and Where to Find Them" section 4; "Buy 4 REINFORCE Samples, Get a Baseline for Free!").  The rule is
// defined once, in include/cvc_hip_blocks.h (cvc_scst_weights_wor); restated here and in fp64 in tests/wor_ref.py.
//
// Clip b ran the stochastic beam with beam = S + 1: slots 0 .. S-1 are the rollouts, slot S gives only its key, the threshold.
//   live_j = isfinite(G_j);  phi_i = logq_i;  kt = G_S
//   h = cvc_drop_hash(seed_lo, seed_hi, call, CVC_WOR_SITE, b);  u = ((h >> 9) + 0.5) 2^-23;  a = -log u        (a ~ Exp(1) per clip)
//   lambda = -kappa = -kt + log1p((a - 1) exp(kt))       (slot S not live: +inf)  -- the threshold re-conditioned on a root key
//            G_root ~ Gumbel(0) instead of the engine's G_root = 0: exp(-kappa) = a - 1 + exp(-kt)
//   d_i = phi_i + lambda;  x_i = exp(d_i);  log q_i = log(-expm1(-x_i)), taken as d_i + log(-expm1(-x_i) / x_i) for x_i < 1 (ratio 1 at
//            x_i = 0), 0 at x_i = inf;  l_i = phi_i - log q_i (live), -inf (dead)
//   W_i = exp(phi_i) + sum_{j != i} exp(l_j);  B_i = exp(phi_i) f_i + sum_{j != i} exp(l_j) f_j;  W = sum_j exp(l_j)
//            (live j < S, ascending j, every sum shifted by its largest exponent)
//   normalize:  wgt_i = exp(l_i) / W;  adv_i = n_live wgt_i (f_i - B_i / W_i);  est = sum_j wgt_j f_j
//   else:       wgt_i = exp(l_i);      adv_i = wgt_i (f_i - B_i);               est = sum_j wgt_j f_j
//   a dead row: wgt = adv = 0;  w[r, t] = adv_r over the steps up to and including the first 0 of cand[r, :], else 0.
//
// ONE THREAD per row, which recomputes its clip's S <= 7 log-weights (three transcendentals each) instead of sharing them: the whole
// launch is B * S rows of a few hundred flops, and a row that owns all its sums needs no LDS, no barrier and no atomics -- its
// outputs depend on its clip's inputs only and are bit-reproducible.  Thread i == 0 of a clip writes est.  Accurate logf / expf /
// log1pf / expm1f, no contraction.  Launch only: capturable in a HIP graph; the state words are read from device memory, so a
// replay after cvc_sample_advance sees the new `call`.
#include "cvc_common.h"
#include "dropout_rng.h"
#include <math.h>

namespace {

constexpr int WOR_MAX_S = 7;

// log(1 - exp(-exp(d))): the log of the probability that a caption whose sampling log-prob exceeds -lambda by d is in the sample
__device__ __forceinline__ float log_inclusion(float d) {
#pragma clang fp contract(off)
    const float x = expf(d);
    if (isinf(x)) return 0.f;
    if (x < 1.f) {
        const float ratio = x > 0.f ? -expm1f(-x) / x : 1.f;
        return d + logf(ratio);
    }
    return logf(-expm1f(-x));
}

__global__ __launch_bounds__(64) void scst_weights_wor_kernel(const float* reward, const float* logq, const float* G, const uint32_t* state,
                                                              int rows, int S, const int64_t* cand, int T, int t_major, int normalize,
                                                              float* adv, float* wgt, float* est, float* w) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * 64 + threadIdx.x;
    if (row >= rows) return;
    const int clip = row / S, i = row - clip * S;
    const float* f = reward + (size_t)clip * S;
    const float* q = logq + (size_t)clip * (S + 1);
    const float* g = G + (size_t)clip * (S + 1);
    const float kt = g[S];
    float lambda = INFINITY;
    if (isfinite(kt)) {
        const uint32_t h = cvc_drop_hash(state[0], state[1], state[2], CVC_WOR_SITE, (uint32_t)clip);
        const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;
        const float a = -logf(u);
        lambda = -kt + log1pf((a - 1.f) * expf(kt));
    }
    float l[WOR_MAX_S], fj[WOR_MAX_S];
    int n_live = 0;
    float m = -INFINITY;                           // the largest exponent of W
#pragma unroll
    for (int j = 0; j < WOR_MAX_S; ++j) {
        l[j] = -INFINITY;
        fj[j] = 0.f;
        if (j < S && isfinite(g[j])) {
            l[j] = q[j] - log_inclusion(q[j] + lambda);
            fj[j] = f[j];
            m = fmaxf(m, l[j]);
            ++n_live;
        }
    }
    float W = 0.f, E = 0.f;                        // sum_j exp(l_j - m), sum_j exp(l_j - m) f_j
#pragma unroll
    for (int j = 0; j < WOR_MAX_S; ++j)
        if (l[j] > -INFINITY) {
            const float e = expf(l[j] - m);
            W += e;
            E += e * fj[j];
        }
    if (i == 0) est[clip] = n_live == 0 ? 0.f : (normalize ? E / W : expf(m) * E);
    float li = -INFINITY, fi = 0.f, phi = 0.f;
#pragma unroll
    for (int j = 0; j < WOR_MAX_S; ++j)
        if (j == i) { li = l[j]; fi = fj[j]; phi = q[j]; }
    float a_row = 0.f, w_row = 0.f;
    if (li > -INFINITY) {
        float mi = phi;                            // row i's own sums: row i enters with p_i = exp(phi_i) instead of w_i
#pragma unroll
        for (int j = 0; j < WOR_MAX_S; ++j)
            if (j != i) mi = fmaxf(mi, l[j]);
        float Wi = 0.f, Bi = 0.f;
#pragma unroll
        for (int j = 0; j < WOR_MAX_S; ++j) {
            if (j == i) {
                const float e = expf(phi - mi);
                Wi += e;
                Bi += e * fi;
            } else if (l[j] > -INFINITY) {
                const float e = expf(l[j] - mi);
                Wi += e;
                Bi += e * fj[j];
            }
        }
        if (normalize) {
            w_row = expf(li - m) / W;
            a_row = ((float)n_live * w_row) * (fi - Bi / Wi);
        } else {
            w_row = expf(li);
            a_row = w_row * (fi - expf(mi) * Bi);
        }
    }
    wgt[row] = w_row;
    adv[row] = a_row;
    bool on = true;                                // the steps up to and including the first 0
    for (int t = 0; t < T; ++t) {
        const size_t at = t_major ? (size_t)t * rows + row : (size_t)row * T + t;
        w[at] = on ? a_row : 0.f;
        on = on && cand[(size_t)row * T + t] != 0;
    }
}

}  // namespace

extern "C" int cvc_scst_weights_wor(const float* reward, const float* logq, const float* G, const uint32_t* state, int rows, int per_clip,
                                    const int64_t* cand, int T, int t_major, int normalize, float* adv, float* wgt, float* est, float* w,
                                    cvc_stream_t stream) {
    if (reward == nullptr || logq == nullptr || G == nullptr || state == nullptr || cand == nullptr) return CVC_E_BADARG;
    if (adv == nullptr || wgt == nullptr || est == nullptr || w == nullptr) return CVC_E_BADARG;
    if (per_clip < 2 || per_clip > WOR_MAX_S || rows < 1 || rows % per_clip != 0 || T < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(scst_weights_wor_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, reward, logq, G, state, rows,
                       per_clip, cand, T, t_major != 0, normalize != 0, adv, wgt, est, w);
    return cvc_launch_status();
}
