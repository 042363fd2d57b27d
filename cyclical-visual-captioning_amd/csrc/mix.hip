// Scheduled sampling: the selection block that draws a word and, by a per-row coin, writes either the drawn or the GIVEN word as the
// next step's input.  The selection block of the decode engine's mixed mode (cvc/decode/engine.py, mix=True); the MIX form of the
// sampling kernel (csrc/sample_select.h), so the draw is the plain sampler's code and the log-sum-exp the one the forced block takes.
//
//   drawn[r], logprob[r]  = word and logprob of cvc_sample_select_parts from the same slabs, bias, inv_tau, state and t, bit for bit
//                           (hash site CVC_SAMPLE_SITE + t, counter r * V + v, the same reduction order, UNK excluded)
//   h        = cvc_drop_hash(seed_lo, seed_hi, call, CVC_MIX_SITE + t, r)
//   u        = ((h >> 9) + 0.5) * 2^-23                  exactly representable, strictly inside (0, 1)
//   took[r]  = u < *mix_prob                             exact in fp32; p = 0 never takes, p = 1 always takes (NaN: never)
//   g        = given[r * given_stride] if that lies in [0, V), else 0
//   word[r * word_stride] = took ? drawn : g             a gather index of the next step
//   given_logprob[r] = z[r, g] - logsumexp_v z[r, v]     the bits of cvc_forced_select_parts (same max, same sum-exp in the same
//                                                        order); a given word outside [0, V): NaN, as there
//
// mix_prob is one float of DEVICE memory, read by the kernel: a captured graph serves a changing probability.  drawn, took and
// given_logprob are nullable.  No atomics, every reduction in a fixed order: bitwise deterministic.  The row's logits stay in
// registers (the build fails if this kernel uses scratch: build_hip.py).
#include "sample_select.h"

extern "C" int cvc_mixed_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                                      int unk_idx, float inv_tau, const uint32_t* rng_state, int t, int64_t* word, int word_stride,
                                      float* logprob, const int64_t* given, int given_stride, const float* mix_prob, int64_t* drawn,
                                      uint8_t* took, float* given_logprob, cvc_stream_t stream) {
    const int rc = select_check(parts, nparts, part_stride, M, V, inv_tau, rng_state, t, word, word_stride);
    if (rc != 0) return rc;
    if (!given || given_stride < 1 || !mix_prob) return CVC_E_BADARG;
    const uint32_t site = CVC_SAMPLE_SITE + (uint32_t)t;
    const MixArgs ma{given, given_stride, mix_prob, CVC_MIX_SITE + (uint32_t)t, drawn, took, given_logprob};
    select_dispatch(parts, nparts, part_stride, bias, V, [&](auto nc, auto np, auto vec) {
        hipLaunchKernelGGL((sample_select_kernel<decltype(nc)::value, decltype(np)::value, decltype(vec)::value, false, false, true>),
                           dim3(M), dim3(WG), 0, (hipStream_t)stream, parts, nparts, part_stride, bias, V, unk_idx, inv_tau, rng_state,
                           site, word, word_stride, logprob, NoTrunc{}, NoCons{}, ma);
    });
    return cvc_launch_status();
}
