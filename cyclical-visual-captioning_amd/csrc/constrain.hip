// Constrained decoding: the selection block that knows the row's history (DecodeEngine(no_repeat_ngram / no_immediate_repeat /
// min_len / ban_words / bad_endings)).  The CONS flag of the sampling kernel (csrc/sample_select.h): the row loader
// (csrc/select_row.h), the hash counters, the noise, the candidate mask, the truncation search and the log-prob are that kernel's;
// the mask holds the row's ban set instead of UNK alone.  The top_k / top_p rules and the choice of form are select_run's, there too.
//
// Step t (0 .. T-1) chooses y_t for a row with history y_0 .. y_{t-1} = hist[0 .. t-1] (the engine's words[1 .. t]; BOS is not
// history).  Ban(t, row) is the union of
//   {unk_idx}
//   ban[0 .. nban)                          a fixed list of word ids
//   no_repeat_ngram = n >= 1:               every v for which some j, n-1 <= j <= t-1, has y_j = v and
//                                           y_{j-n+1 .. j-1} = y_{t-n+1 .. t-1}  (n = 1: every earlier word; nothing while t < n-1)
//   no_immediate_repeat:                    y_{t-1}, t >= 1
//   min_len = L:                            word 0 while t < L
//   bad_end[0 .. nbad):                     word 0 when t >= 1 and y_{t-1} is in the list
// and C0 = { v < V } \ Ban.  List ids outside [0, V) are ignored: nothing is read or written at them.
//   inv_tau == 0 (arg-max mode; rng_state may be NULL, top_k / top_p off): word = argmax over C0 of z, ties -> lower index
//   inv_tau > 0: s, the hash counters and the noise of cvc_sample_select_parts, the arg-max over C0 -- the unconstrained sampler's
//                word whenever that is allowed, else an exact draw from the renormalised distribution; with top_k / top_p the C1 /
//                C2 of cvc_sample_select_trunc_parts over this C0 (top_k counts allowed words only)
//   logprob[r] = z[r, word] - logsumexp_v z[r, v]: the model's, full V, banned words included
//   nbanned[r] = |Ban|: distinct ids, UNK included (nullable); cutoff / kept as in cvc_sample_select_trunc_parts (nullable)
//   a row without a candidate: word 0, logprob -inf
// The kernel: one workgroup of 256 per row; the history in LDS (t <= 64: one lane per j), the ban set as a V-bit map in LDS (at
// most 256 words, LDS atomicOr), one barrier, then every thread turns its bits into the mask of its register slots (NC <= 32) that
// the unconstrained forms fill with UNK's slot alone.  Every reduction runs in a fixed order: bitwise deterministic.
#include "sample_select.h"

extern "C" int cvc_constrained_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                                            int unk_idx, float inv_tau, int top_k, float top_p, const uint32_t* rng_state, int t,
                                            int64_t* word, int word_stride, float* logprob, float* cutoff, int32_t* kept,
                                            const int64_t* hist, long long hist_stride, const cvc_constraint* c, int32_t* nbanned,
                                            cvc_stream_t stream) {
    const int rc = select_check(parts, nparts, part_stride, M, V, inv_tau, rng_state, t, word, word_stride, inv_tau == 0.f);
    if (rc != 0) return rc;
    if (t > CONS_T_MAX) return CVC_E_TOOBIG;
    if (!c || cons_rules_check(c) != 0) return CVC_E_BADARG;
    if (t > 0 && (!hist || hist_stride < 1)) return CVC_E_BADARG;
    const ConsArgs ca{hist, hist_stride, t, c->no_repeat_ngram, c->no_immediate_repeat != 0, c->min_len, c->ban, c->nban,
                      c->bad_end, c->nbad, nbanned};
    return select_run<true>(parts, nparts, part_stride, bias, M, V, unk_idx, inv_tau, top_k, top_p, rng_state, t, word, word_stride,
                            logprob, cutoff, kept, stream, ca);
}
