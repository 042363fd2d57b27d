// Sampled decoding: Gumbel-max selection of the next word from softmax(logits / tau) without UNK, n captions per clip.
// The selection block of the decode engine's sampling mode (cvc/decode/engine.py, sample_n / temperature): one workgroup per row
// sums the K-slice slabs of the vocabulary GEMM (+ bias) in the finishing pass's order (cvc_tile_linear_finish: slab 0 + slab 1 +
// ... + bias, so the logits are bit for bit what the greedy / beam selection sees), draws the noise in-kernel from the
// counter-based hash of csrc/dropout_rng.h and writes the word and its log-prob.
//
//   h        = cvc_drop_hash(seed_lo, seed_hi, call, CVC_SAMPLE_SITE + t, r * V + v)
//   u        = ((h >> 9) + 0.5) * 2^-23                  exactly representable, strictly inside (0, 1)
//   g        = -logf(-logf(u))                           accurate logf (not __logf)
//   s        = z[r, v] * inv_tau + g                     product rounded, then the sum (no contraction)
//   word[r]  = argmax over v != unk of s                 ties -> lower index
//   logprob  = z[r, word] - logsumexp_v z[r, v]          full V, UNK included, independent of tau
//
// The state is 4 words of device memory {seed_lo, seed_hi, call, 0}; cvc_sample_advance adds 1 to `call` (the first launch of a
// sampled decode, so a graph replay draws fresh noise).  Every reduction runs in a fixed order: the result is bitwise
// deterministic.  The row's logits stay in registers (NC per thread, V <= 256 * NC_MAX), loaded as float4 where V % 4 == 0.
//
// Truncation (cvc_sample_select_trunc_parts; the TRUNC flag of the same kernel): the arg-max runs over a candidate set C2 only.
//   C0 = { v < V, v != unk }
//   C1 = { v in C0 : z[v] >= theta_k },  theta_k = the top_k-th largest z over C0 (ties with it all kept; top_k = 0: C1 = C0)
//   C2 = { v in C1 : z[v] >= theta_p },  theta_p = the largest z occurring in C1 with mass(theta_p) >= top_p * mass(-inf), where
//        mass(theta) = sum over v in C1, z[v] >= theta of expf((z[v] - max_C1 z) * inv_tau)        (top_p = 1: C2 = C1)
// Both cutoffs are found by a search over the order-preserving 32-bit key of a float, most significant bit first: per probe every
// thread counts its logits (sums its cached e) that are >= the candidate cutoff, then a DPP wave sum and the four wave partials
// through LDS in a fixed order -- non-negative terms in a fixed order, so the predicate is monotone in the cutoff and the result
// bitwise deterministic.  s, the hash counters and the log-prob (full V, the model's, independent of tau / top_k / top_p) are those
// of the plain kernel; cutoff[r] = min over C2 of z, kept[r] = |C2| (a row without a candidate: kept 0, cutoff +inf, word 0).
// With truncation off (top_k = 0 or >= V - 1, top_p = 1) the word and the log-prob are the plain form's bit for bit; cutoff / kept,
// where asked for, come from the truncating form with both searches off (C2 = C0).
//
// The kernel and the function behind the entry points (top_k / top_p rules, choice of form) live in csrc/sample_select.h, shared
// with the constrained block (csrc/constrain.hip); the row loader, the shared argument checks and the dispatch in
// csrc/select_row.h, shared with the forced block too.  This file holds the two entry points and the advance kernel.
#include "sample_select.h"

namespace {

__global__ void sample_advance_kernel(uint32_t* state) {
    if (threadIdx.x == 0) state[2] = state[2] + 1u;
}

}  // namespace

extern "C" int cvc_sample_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                                       int unk_idx, float inv_tau, const uint32_t* rng_state, int t, int64_t* word, int word_stride,
                                       float* logprob, cvc_stream_t stream) {
    const int rc = select_check(parts, nparts, part_stride, M, V, inv_tau, rng_state, t, word, word_stride);
    if (rc != 0) return rc;
    return select_run<false>(parts, nparts, part_stride, bias, M, V, unk_idx, inv_tau, 0, 1.f, rng_state, t, word, word_stride, logprob,
                             nullptr, nullptr, stream);
}

extern "C" int cvc_sample_select_trunc_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                                             int unk_idx, float inv_tau, int top_k, float top_p, const uint32_t* rng_state, int t,
                                             int64_t* word, int word_stride, float* logprob, float* cutoff, int32_t* kept,
                                             cvc_stream_t stream) {
    const int rc = select_check(parts, nparts, part_stride, M, V, inv_tau, rng_state, t, word, word_stride);
    if (rc != 0) return rc;
    return select_run<false>(parts, nparts, part_stride, bias, M, V, unk_idx, inv_tau, top_k, top_p, rng_state, t, word, word_stride,
                             logprob, cutoff, kept, stream);
}

extern "C" int cvc_sample_advance(uint32_t* rng_state, cvc_stream_t stream) {
    if (!rng_state) return CVC_E_BADARG;
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, rng_state);
    return cvc_launch_status();
}
