/*
 * cvc_hip_blocks.h -- the per-kernel building blocks of libcvc_hip.so: what the whole-decode drivers (cvc_decode_greedy / _beam),
 * the training-loop drivers (cvc_train_loop_fwd / _bwd) and the host mirror's eager launch lists are composed of.  NOT part of the
 * exported drop-in ABI (hidden visibility): unit tests and cvc/decode.py reach them through cvc_block("name") (cvc_hip.h).
 * Contracts: the section of cvc_hip.h that describes the corresponding driver or core entry point (same argument conventions:
 * raw device pointers, sizes, the launch stream; 0 / hipError_t / CVC_E_*).
 */
#ifndef CVC_HIP_BLOCKS_H
#define CVC_HIP_BLOCKS_H
#include "cvc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

int cvc_attn_scores(int kind, const float* q, const float* w_a, const float* b_a, float inv_temp,
                    const cvc_attn_set* sets, int nsets, int nclip, int nq, int A, cvc_stream_t stream);
int cvc_attn_wsum(const cvc_attn_set* sets, int nsets, int nclip, int nq, int R, float* ctx_sum,
                  cvc_stream_t stream);
int cvc_attn_scores_qparts(int kind, const float* q_parts, int q_nparts, const float* q_bias, const float* w_a,
                           const float* b_a, float inv_temp, const cvc_attn_set* sets, int nsets, int nclip,
                           int nq, int A, cvc_stream_t stream);
int cvc_attn_wsum_quad(const cvc_attn_set* sets, int nsets, int nclip, int nq, int R, float* ctx_sum_q,
                       cvc_stream_t stream);
int cvc_attn_wsum_frag(const cvc_attn_set* sets, int nsets, int nclip, int nq, int R, void* ctx_frag,
                       long long frag_mblk_stride, cvc_stream_t stream);
int cvc_attn_wsum_quad_rm(const cvc_attn_set* sets, int nsets, int nclip, int R, float* ctx_sum_q, float* ctx_sum_rm,
                          cvc_stream_t stream);            /* one query per clip (nq = 1), nclip <= 64 */
int cvc_attn_bwd_pair(int kind, const cvc_grad_src* q, const float* q_bias, const float* w_a, float inv_temp,
                      const cvc_attn_set* sets, int nsets, const cvc_grad_src* d_ctx, int nclip, int nq, int A, int R,
                      float* d_q, float* d_q_q, float* d_w_part, float* const* d_proj, float* const* d_ctxfeat,
                      cvc_stream_t stream);
/* d_feat[b, i, :] += sum_t attn[t][b][i] * d_ctx_all[t][b (of 128 rows)][:]  (t < T <= 32): the context-feature gradient of all T
 * steps of the training loop in one pass over d_feat [B, n, R] (cvc_train_loop.d_ctx_all; reference: the `bmm(att, context)` of
 * modules.py:66-69 / 150-153 under autograd, accumulated over the T decoder steps of captioner.py:242-270) */
int cvc_ctxfeat_bwd_steps(const float* attn, const float* d_ctx_all, int T, int B, int n, int R, float* d_feat, cvc_stream_t stream);
/* d_proj[b, i, :] += sum_t d_s[t][b][i] * w_a * (1 - tanh^2(proj[b, i, :] + q_t[b, :]))  (additive attention; t < T <= 32): the
 * projected-feature gradient of all T steps in one pass.  q: [T] blocks of q_step floats, each q_nplanes planes ([B, A], q_plane
 * floats apart) summed on load (+ q_bias): the h2attn outputs the forward kept (cvc_train_loop.q). */
int cvc_dproj_bwd_steps(const float* q, long long q_step, long long q_plane, int q_nplanes, const float* q_bias, const float* w_a,
                        const float* proj, const float* ds, int T, int B, int n, int A, float* d_proj, cvc_stream_t stream);
/* test / A-B hook of cvc_tile_gemm's 256 x 256 form (round 6, OFF by default: measured no gain inside the training step; applies to
 * M % 256 == 0, N % 256 == 0, M >= 512 and min_wgs .. 256 workgroups, any grid with min_wgs = 1): on = 1 / 0 / -1 (query only),
 * min_wgs > 0 sets the threshold.  Returns the previous on / off setting. */
int cvc_tile_gemm_big(int on, int min_wgs);
/* The K split to pass as `ksplit` for a dense product (callers without a split of their own: the backward pass's dense products) and
 * the grid cvc_tile_gemm launches for it: the largest split with >= 8 k steps per slice whose grid is at most one round of
 * workgroups (one per compute unit), else 1.  chunk_rows = rows one workgroup walks, workgroups = the grid size.  Host only; any of
 * the three outputs may be NULL.  CVC_E_BADARG for M, N < 1 or K not a positive multiple of 16. */
int cvc_tile_gemm_plan(int M, int N, int K, int* ksplit, int* chunk_rows, int* workgroups);
/* Split-K form of cvc_linear_fwd (cvc_hip.h; segments as there): y_parts [ksplit][M][Nout] contiguous, slice s at
 * y_parts + s * M * Nout.  Slice s holds the product over whole 32-column chunks [nch s / ksplit, nch (s + 1) / ksplit) (integer
 * division) of EVERY segment, nch = ceil(k / 32) of that segment, a ragged last chunk ending at k; slice 0 also holds the bias
 * (nullable).  A slice that owns no chunk of any segment is written all the same: exact zeros (slice 0: the bias itself).  The
 * consumer sums the slices in a fixed order.  CVC_E_BADARG: M < 1 or M > 64, Nout < 1, ksplit < 1 or ksplit > 64, y_parts NULL,
 * a gather segment (idx != NULL) with ksplit > 1, and every segment cvc_linear_fwd refuses (nsegs outside 1 .. 4, k < 4 or
 * k % 4, ldx % 4, ldw % 4, x or w NULL or off 16-byte alignment); nothing is launched and y_parts is untouched then.  Pinned by
 * tests/test_gpu_skinny_gemm.py. */
int cvc_linear_splitk_fwd(const cvc_gemm_seg* segs, int nsegs, const float* bias, int M, int Nout,
                          int ksplit, float* y_parts, cvc_stream_t stream);
/* cvc_linear_fwd with the word-selection records fused into the epilogue: top2_part [ceil(Nout / 32)][64][6] floats; block b,
 * row m < M holds {v1, i1, v2, i2, mx, se} of columns [32 b, min(32 b + 32, Nout)) of y (bias included): the largest value and its
 * column, the second largest and its column (columns are GLOBAL int32 indices stored as float bits), mx == v1 bit for bit and
 * se = sum exp(y - mx) over the block's valid columns.  v1 / v2 are the bits of the same launch's y.  Equal values: the lower
 * column comes first (top-1 before top-2, and the kept one of two equal candidates for top-2).  A block with one valid column
 * has (v2, i2) = (-inf, 0x7fffffff).  Rows >= M of every block are untouched.  y_or_null [M][Nout] (ld Nout) receives the logits
 * if given; the records are the same bits either way.  CVC_E_BADARG: top2_part NULL, M < 1, Nout < 1, a refused segment (see
 * above); CVC_E_TOOBIG: M > 64; nothing is launched and neither output is touched then.  cvc_top2_final merges the records. */
int cvc_linear_top2_fwd(const cvc_gemm_seg* segs, int nsegs, const float* bias, int M, int Nout,
                        float* y_or_null, float* top2_part, cvc_stream_t stream);
int cvc_top2_final(const float* part, int nblocks, int M, int unk_idx, int64_t* word, int word_stride,
                   float* logprob, const float* table, int E, float* emb_out, int emb_ld,
                   cvc_stream_t stream);
int cvc_packed_lstm_fwd(const float* wp, const float* xq, int K, const float* b_ih, const float* b_hh,
                        const float* gate_bias, const float* c_prev_q, int M, int R, float* h_dst1_q,
                        float* h_dst2_q, float* c_out_q, cvc_stream_t stream);
int cvc_packed_linear_fwd(const float* wp, const float* xq, int K, const float* bias, int M, int Nout,
                          int ksplit, float* y, int ldy, float* top2_part, cvc_stream_t stream);
int cvc_packed_lstm_embgate_fwd(const float* wp, const float* xq, int K, const float* b_ih, const float* b_hh,
                                const float* gate_bias, const float* emb_gate, const int64_t* word, const float* c_prev_q,
                                int M, int R, float* h_dst1_q, float* h_dst2_q, float* c_out_q, cvc_stream_t stream);
int cvc_packed_lstm_embgate_ex_fwd(const float* wp, long long w_blk_stride, const float* xq, int K, const float* b_ih,
                                   const float* b_hh, const float* gate_bias, const float* emb_gate, const int64_t* word,
                                   const float* c_prev_q, int M, int R, float* h_dst1_q, float* h_dst2_q,
                                   float* c_out_q, int w_cached, cvc_stream_t stream);
int cvc_packed_lstm_late_fwd(const float* wp, long long w_blk_stride, const float* xq, int K, const float* b_ih,
                             const float* b_hh, const float* gate_bias, const float* c_prev_q, int M, int R,
                             float* h_dst1_q, float* h_dst2_q, float* c_out_q, const cvc_gsk_segs* early,
                             cvc_stream_t stream);
int cvc_packed_lstm_train_fwd(const float* wp, const float* xq, int K, const float* b_ih, const float* b_hh,
                              const float* c_prev, int M, int R, float* h_out, float* c_out, float* gates_out,
                              float* h_out2, float* h_out3, cvc_stream_t stream);   /* h_out2/3: further copies of h', nullable */
int cvc_packed_lstm_train_pre_fwd(const float* wp, const float* xq, int K, const float* b_ih, const float* b_hh,
                                  const float* gate_pre, const float* c_prev, int M, int R, float* h_out, float* c_out,
                                  float* gates_out, float* h_out2, float* h_out3, cvc_stream_t stream);
int cvc_packed_lstm_train_drop_fwd(const float* wp, const float* xq, int K, const float* b_ih, const float* b_hh,
                                   const float* gate_pre, const float* c_prev, int M, int R, float* h_out, float* c_out,
                                   float* gates_out, float* h_out2, float* h_drop_out, const uint32_t* rng_state,
                                   unsigned site, float p, cvc_stream_t stream);
int cvc_lstm_pointwise_bwd(const float* d_h, const float* d_c, const float* gates,
                           const float* c_prev, const float* c_new, int M, int R,
                           float* d_gates, float* d_c_prev, float* d_gates_q, cvc_stream_t stream);
int cvc_lstm_pointwise_bwd3(const float* d_h, const float* d_h2, const float* d_h3, const float* d_c,
                            const float* gates, const float* c_prev, const float* c_new, int M, int R,
                            float* d_gates, float* d_c_prev, float* d_gates_q, cvc_stream_t stream);
int cvc_lstm_pointwise_bwd3_drop(const float* d_h, const float* d_h2, const float* d_h3, const uint32_t* rng_state,
                                 unsigned site, float p, const float* d_c, const float* gates, const float* c_prev,
                                 const float* c_new, int M, int R, float* d_gates, float* d_c_prev, float* d_gates_q,
                                 cvc_stream_t stream);
int cvc_pack_lstm_weights(const float* w_ih, int K_ih, const float* w_hh, int K_hh, int R, float* wp,
                          cvc_stream_t stream);
int cvc_linear_nn_planes_fwd(const float* dy_q, int K, int M, const cvc_nn_seg* segs, int nsegs, int ksplit,
                             float* workspace, cvc_stream_t stream);
/* Training form of the per-step recurrence: additionally writes, for every step and direction, what autograd needs --
 * (r, z, n, W_hn h + b_hn) at gates + m * g_ld_m + t * g_ld_t + d * 4H + {0, H, 2H, 3H} (as cvc_gru_seq_persistent_train_fwd).
 * Any H % 8 == 0: the form config 5's encoder width (rnn_size 4096 -> H = 2048, backbone.py:103-104) trains on. */
int cvc_gru_seq_train_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih,
                          const float* b_hh, int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m,
                          long long y_ld_t, float* gates, long long g_ld_m, long long g_ld_t, cvc_stream_t stream);
/* cvc_lstm_pointwise_bwd4 (include/cvc_hip.h) for TWO independent argument sets in ONE launch: the gate-gradient kernels of the two
 * loops of the cyclical pass at a step of their joint back-propagation (same cell, same shape, ~10 us each and latency-bound).
 * Vector form only (every pointer 16-byte aligned, R % 4 == 0): CVC_E_BADARG otherwise, and the caller launches them one by one. */
typedef struct cvc_pw_bwd_args {
    cvc_grad_src d_h[3];
    const float* d_hd;
    const uint32_t* rng_state;
    unsigned site;
    float p;
    const float *d_c, *gates, *c_prev, *c_new;
    int M;
    float *d_gates, *d_c_prev, *d_gates_q, *dg_sum;
    int q_row0;
} cvc_pw_bwd_args;
int cvc_lstm_pointwise_bwd4_pair(const cvc_pw_bwd_args* a, const cvc_pw_bwd_args* b, int R, cvc_stream_t stream);
/* cvc_linear_nn_planes_fwd for TWO 64-row operand groups against one stream of the weights (the two loops of the cyclical pass at
 * B = 64 each share the LSTM cells, captioner.py:86-87): rows 0 .. M - 1 from dy_q, rows 64 .. 64 + M2 - 1 from dy_q2; planes are
 * [ksplit][128][ntot]; with reduce != 0 (or ksplit == 1) the result goes to the segments' dst [128 rows, ld_dst].  Under the same K
 * split a row gets the bits cvc_linear_nn_planes_fwd gives it. */
int cvc_linear_nn_planes2_fwd(const float* dy_q, const float* dy_q2, int K, int M, int M2, const cvc_nn_seg* segs, int nsegs,
                              int ksplit, float* workspace, int reduce, cvc_stream_t stream);
int cvc_beam_select_parts(const float* parts, int nparts, long long part_stride, const float* bias,
                          const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx,
                          int first_step, int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out,
                          float* workspace, cvc_stream_t stream);
/* Sampled decoding (csrc/sample.hip; the kernel in csrc/sample_select.h, the row loader, the argument checks and the dispatch that
 * every selection block below shares in csrc/select_row.h): Gumbel-max sampling from softmax(z / tau) without UNK, one workgroup
 * per row.
 *   z[r, :]  = parts[0][r, :] + ... + parts[nparts-1][r, :] (+ bias), the order of cvc_tile_linear_finish (nparts = 1, bias = NULL:
 *              a finished [M, V] logit matrix); slab p starts part_stride floats after slab p-1
 *   h        = cvc_drop_hash(seed_lo, seed_hi, call, CVC_SAMPLE_SITE + t, r * V + v)      (csrc/dropout_rng.h)
 *   u        = ((h >> 9) + 0.5) * 2^-23,  g = -logf(-logf(u)),  s = z[r, v] * inv_tau + g
 *   word[r * word_stride] = argmax over v != unk_idx of s (ties -> lower index)
 *   logprob[r] = z[r, word] - logsumexp_v z[r, v] (nullable; full V, independent of tau)
 * rng_state: 4 words of device memory {seed_lo, seed_hi, call, 0}; cvc_sample_advance adds 1 to `call` on the stream.
 * V <= 8192, M * V < 2^32; bitwise deterministic. */
#define CVC_SAMPLE_SITE 0x53000000u
int cvc_sample_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V, int unk_idx,
                            float inv_tau, const uint32_t* rng_state, int t, int64_t* word, int word_stride, float* logprob,
                            cvc_stream_t stream);
int cvc_sample_advance(uint32_t* rng_state, cvc_stream_t stream);
/* Scheduled sampling (csrc/mix.hip; the MIX form of the kernel in csrc/sample_select.h): cvc_sample_select_parts, then a per-row
 * coin decides whether the drawn or a GIVEN word is written as the next step's input.
 *   drawn[r], logprob[r] = word and logprob of cvc_sample_select_parts from the same arguments, bit for bit
 *   h       = cvc_drop_hash(seed_lo, seed_hi, call, CVC_MIX_SITE + t, r),  u = ((h >> 9) + 0.5) * 2^-23
 *   took[r] = u < *mix_prob (exact in fp32; 0 never takes, 1 always takes); mix_prob: one float of device memory, read by the kernel
 *   g       = given[r * given_stride] if that lies in [0, V), else 0;   word[r * word_stride] = took ? drawn : g
 *   given_logprob[r] = z[r, g] - logsumexp_v z[r, v], the bits of cvc_forced_select_parts (a given word outside [0, V): NaN)
 * drawn, took, given_logprob are nullable.  The checks of cvc_sample_select_parts; NULL given / mix_prob, given_stride < 1:
 * CVC_E_BADARG.  CVC_MIX_SITE + t is disjoint from CVC_SAMPLE_SITE + t' and from the dropout sites (cvc/dropout.py) for t, t' < 64.
 * Bitwise deterministic. */
#define CVC_MIX_SITE 0x4D000000u
int cvc_mixed_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V, int unk_idx,
                           float inv_tau, const uint32_t* rng_state, int t, int64_t* word, int word_stride, float* logprob,
                           const int64_t* given, int given_stride, const float* mix_prob, int64_t* drawn, uint8_t* took,
                           float* given_logprob, cvc_stream_t stream);
/* The same with top-k / nucleus (top-p) truncation: z, s, the noise, the hash counters and logprob are those of
 * cvc_sample_select_parts; the arg-max runs over a candidate set C2 only.
 *   C0 = { v < V, v != unk_idx }
 *   C1 = { v in C0 : z[v] >= theta_k }, theta_k = the top_k-th largest z over C0, with multiplicity (top_k = 0 or >= |C0|: C1 = C0);
 *        words tied with the top_k-th value are all kept: |C1| may exceed top_k, the set depends on the values only
 *   C2 = { v in C1 : z[v] >= theta_p }, theta_p = the largest z occurring in C1 with mass(theta_p) >= top_p * mass(-inf), where
 *        mass(theta) = sum over v in C1 with z[v] >= theta of expf((z[v] - max_C1 z) * inv_tau), fp32, fixed order (top_p = 1: C2 = C1)
 *   word[r * word_stride] = argmax over v in C2 of s: the word cvc_sample_select_parts draws from the same state, if that lies in C2
 *   logprob[r] = the model's log-prob of the word (full V, independent of tau, top_k, top_p; NOT the truncated distribution's)
 *   cutoff[r] = min over C2 of z, kept[r] = |C2| (both nullable)
 * top_k < 0, top_p outside (0, 1] or not finite: CVC_E_BADARG.  Truncation off (top_k == 0 or >= V - 1, and top_p == 1): word and
 * logprob have the bits of cvc_sample_select_parts -- the plain kernel is launched, or, if cutoff / kept are given, the truncating
 * one with both searches off, which fills them from C0.  Bitwise deterministic. */
int cvc_sample_select_trunc_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                                  int unk_idx, float inv_tau, int top_k, float top_p, const uint32_t* rng_state, int t,
                                  int64_t* word, int word_stride, float* logprob, float* cutoff, int32_t* kept,
                                  cvc_stream_t stream);
/* Constrained decoding (csrc/constrain.hip; the CONS flag of the kernel in csrc/sample_select.h): cvc_sample_select_trunc_parts
 * over a candidate set that depends on the row's history.
 * Step t chooses y_t for a row with history y_0 .. y_{t-1}: element (s, r) at hist[s * hist_stride + r], s < t (the engine's
 * words[1 .. t]; BOS is not history).  Ban(t, r) is the union of
 *   {unk_idx};   ban[0 .. nban): a fixed list of word ids;
 *   no_repeat_ngram = n >= 1: every v for which some j, n-1 <= j <= t-1, has y_j = v and y_{j-n+1 .. j-1} = y_{t-n+1 .. t-1}
 *       (n = 1: every earlier word; nothing is banned while t < n-1);
 *   no_immediate_repeat: y_{t-1}, t >= 1;
 *   min_len = L: word 0 while t < L;
 *   bad_end[0 .. nbad): word 0 when t >= 1 and y_{t-1} is in the list
 * and C0 = { v < V } \ Ban.  Both lists are device memory; ids outside [0, V) are ignored (nothing is read or written at them).
 *   inv_tau == 0: arg-max mode -- word = argmax over C0 of z, ties -> lower index; rng_state may be NULL, top_k / top_p must be off
 *   inv_tau > 0 : s, the hash counters and the noise of cvc_sample_select_parts with the arg-max over C0: the unconstrained
 *                 sampler's word whenever that is allowed, else an exact draw from the renormalised distribution; top_k / top_p:
 *                 the C1 / C2 of cvc_sample_select_trunc_parts with this C0 (top_k counts allowed words only)
 *   logprob[r]  = the model's log-prob of the word (full V, banned words included in the log-sum-exp)
 *   nbanned[r]  = |Ban|, distinct ids, UNK included (nullable); cutoff / kept (nullable) as in cvc_sample_select_trunc_parts
 *   a row without a candidate: word 0, logprob -inf.  Steps after a row's first 0 are computed like any other step.
 * t > 64, V > 8192 or M * V >= 2^32: CVC_E_TOOBIG.  n < 0, n > 64, min_len < 0, nban / nbad outside [0, 256], a NULL list with a
 * non-zero count, truncation together with inv_tau == 0: CVC_E_BADARG.  Bitwise deterministic. */
typedef struct cvc_constraint {
    int no_repeat_ngram;            /* n; 0 = off */
    int no_immediate_repeat;        /* 0 / 1 */
    int min_len;                    /* L; 0 = off */
    int nban;
    const int32_t* ban;             /* device, nban ids */
    const int32_t* bad_end;         /* device, nbad ids */
    int nbad;
} cvc_constraint;
int cvc_constrained_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                                 int unk_idx, float inv_tau, int top_k, float top_p, const uint32_t* rng_state, int t,
                                 int64_t* word, int word_stride, float* logprob, float* cutoff, int32_t* kept,
                                 const int64_t* hist, long long hist_stride, const cvc_constraint* c, int32_t* nbanned,
                                 cvc_stream_t stream);
/* Constrained beam search (csrc/beam.hip: the HIST forms of the row scan and the merge of cvc_beam_select_parts; the ban set is
 * the one definition of csrc/ban_set.h that cvc_constrained_select_parts uses): one beam-search step for hypotheses that carry
 * their own histories, with the rules of constrained decoding applied per hypothesis.
 *   Hypothesis row r = b * beam + k enters step t with history y_0 .. y_{t-1}, the words on its own path from the root: element
 *   (s, r) at hist_in[s * hist_stride + r], s < t (BOS is not history).
 *   Ban(t, r)   = the set of cvc_constrained_select_parts applied to that history: {unk_idx}, ban[], n-gram completion, the
 *                 previous word, word 0 while t < min_len, word 0 after a word of bad_end[].  c == NULL: no rule but UNK.
 *   candidates  = a live row's (k, v) at score_in[k] + z[k, v] - lse[k], the log-sum-exp over the FULL row, banned words included
 *                 (scores stay sums of the model's log-probs); -inf for v in Ban(t, r).  A frozen row (done_in) offers (k, 0) at
 *                 its carried score: the ban is not applied to it, it has already ended.  first_step is t == 0: only row 0 of a
 *                 clip is live.
 *   selection   = the `beam` best of a clip's candidates, ties -> lowest flat (k, v); fewer finite candidates than `beam`: fillers
 *                 at -inf with parent and word in range -- parent, word, score_out, done_out as cvc_beam_select_parts writes them,
 *                 and with nothing banned but UNK the bits of that block on the same inputs.
 *   histories   = for every selected slot (b, sel) with parent kk and word vv:
 *                 hist_out[s * hist_stride + b * beam + sel] = hist_in[s * hist_stride + b * beam + kk] for s < t,
 *                 hist_out[t * hist_stride + b * beam + sel] = vv.  The copy gathers across a clip's rows: hist_in (t steps) and
 *                 hist_out (t + 1 steps) are distinct buffers that ping-pong like score and done; hist_in may be NULL at t == 0.
 *   nbanned[r]  = |Ban(t, r)|, distinct ids, UNK included, for every row, frozen or not (nullable).
 * workspace: 17 * B * beam floats.  The checks of cvc_beam_select_parts; t < 0 or t > 64: CVC_E_TOOBIG; the cvc_constraint checks
 * of cvc_constrained_select_parts (n outside [0, 64], min_len < 0, list counts outside [0, 256], a NULL list with a count), NULL
 * hist_in with t > 0, NULL hist_out, hist_in == hist_out, hist_stride < B * beam: CVC_E_BADARG.  Nothing is launched on a refusal.
 * Bitwise deterministic.  The C driver cvc_decode_beam has no history form: the engine walks or captures its launch list. */
int cvc_beam_select_hist_parts(const float* parts, int nparts, long long part_stride, const float* bias,
                               const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                               const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                               int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out, int32_t* nbanned,
                               float* workspace, cvc_stream_t stream);
/* Diverse (group) beam search (Vijayakumar et al. 2016; csrc/beam.hip: the GROUPS form of the merge of cvc_beam_select_hist_parts,
 * the row scan is that block's): cvc_beam_select_hist_parts with the clip's `beam` = groups * bd slots in `groups` groups that are
 * served in turn within the step, later groups penalised for the words earlier ones took.  Slot k belongs to group g = k / bd.
 *   base        c(k, v) = the candidate of cvc_beam_select_hist_parts: score_in[k] + z[k, v] - lse[k], the log-sum-exp over the full
 *               row, -inf for v in Ban(t, r), a frozen row offers only (k, 0) at its carried score.  t == 0: only the first slot of
 *               each group (k % bd == 0) is live, the others are at -inf.
 *   penalty     for group g, pen(v) = the number of slots selected at this step by groups < g whose parent row was live (not frozen)
 *               and whose word is v (Hamming diversity); aug(k, v) = c(k, v) - lambda * (float)pen(v) in fp32, one rounded
 *               multiply followed by one rounded subtract (no fma).  A frozen row's candidate is not penalised and its selection
 *               does not count toward pen, nor does a filler (a slot selected at -inf: its word is left open below, so it cannot
 *               be part of the rule); -inf stays -inf.
 *   selection   group g takes the bd best of its bd * V candidates by aug, ties -> lowest flat (k, v) with k the clip-wide slot;
 *               the j-th best goes to slot g * bd + j.  The parent of every selected slot lies in its own group.  Fewer finite
 *               candidates than bd: fillers at -inf with the parent in the group and the word in range; every candidate NaN: the
 *               group's first slot and word 0.
 *   outputs     score_out = the UNAUGMENTED c (scores stay sums of the model's log-probs); parent, word, done_out, the histories
 *               and nbanned as cvc_beam_select_hist_parts writes them.
 * groups == 1 is cvc_beam_select_hist_parts bit for bit in every output (lambda then has nothing to act on).  The checks of
 * cvc_beam_select_hist_parts with their codes; groups < 1, beam % groups != 0, lambda negative or not finite: CVC_E_BADARG.  Nothing
 * is launched on a refusal.  Bitwise deterministic; workspace: 17 * B * beam floats. */
int cvc_beam_select_groups_parts(const float* parts, int nparts, long long part_stride, const float* bias,
                                 const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                                 const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                                 int groups, float lambda, int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out,
                                 int32_t* nbanned, float* workspace, cvc_stream_t stream);
/* Final ranking of the hypotheses a history block carried (one launch per decode).  Row r = b * beam + k, its history element (s, r)
 * at hist[s * hist_stride + r], s < T.
 *   len[r]      = position of the first 0 in r's history + 1, or T if there is none.
 *   norm[r]     = score[r] / len[r]^alpha in fp32; alpha == 0: score[r] itself (no power is evaluated).  -inf stays -inf.
 *   order[b, :] = the clip's slots by norm descending, ties -> lowest slot, NaN last.
 * B < 1, beam outside [1, 8], T < 1, hist_stride < B * beam, alpha negative or not finite, a NULL pointer: CVC_E_BADARG; T > 64:
 * CVC_E_TOOBIG. */
int cvc_beam_rank(const int64_t* hist, long long hist_stride, const float* score, int B, int beam, int T, float alpha,
                  int64_t* order, float* norm, int32_t* len, cvc_stream_t stream);
/* Lexically constrained beam search (Anderson et al. 2017; the bank formulation of Post & Vilar 2018; csrc/beam.hip: the FORCE form
 * of the row scan and the BANKS form of the merge of cvc_beam_select_hist_parts): cvc_beam_select_hist_parts with up to C = nforce
 * words per clip that a caption should contain, and the clip's slots in C + 1 banks by the number of forced words met.
 *   forced      force[b * C + j], int32 on the device, C in {1, 2, 3}.  Entry j of clip b is ACTIVE iff 0 < w < V, w != unk_idx and no
 *               entry j' < j of the clip holds the same w; anything else (-1, 0, UNK, out of range, a duplicate) is unused, so a clip
 *               may have fewer than C forced words, or none.  Words only, no phrases.
 *   banks       beam = (C + 1) * bd; slots [j * bd, (j + 1) * bd) of a clip are bank j.  For row r = (b, k) entering step t with
 *               history y_0 .. y_{t-1}: met(r) = the active entries of clip b whose word occurs in the history, n(r) = |met(r)|.
 *               Routing uses n(r) from the history, not the slot.
 *   candidates  the base value c(k, v) is the candidate of cvc_beam_select_hist_parts: score_in[k] + z[k, v] - lse[k], the
 *               log-sum-exp over the full row, -inf for v in Ban(t, r) -- a forced word the ban set holds at this step is -inf for
 *               this step like any banned word -- and a frozen row offers only (k, 0) at its carried score.  t == 0: only slot 0 of
 *               a clip is live.  The TARGET bank of (k, v) is n(r) + 1 if r is live and v is an active forced word of clip b that
 *               is not in met(r), else n(r).
 *   selection   bank j takes the bd best candidates whose target bank is j, over all rows of the clip, ties -> lowest flat (k, v)
 *               with k the clip-wide slot; the i-th best goes to slot j * bd + i.  Fewer than bd finite candidates: the rest of the
 *               bank are fillers -- score_out = -inf, parent in [0, beam), word in [0, V), done_out, the history gather and the
 *               append as for any slot; what a filler holds besides its -inf score is not part of the rule.  A row at -inf offers
 *               only -inf thereafter.
 *   outputs     score_out = c (scores stay sums of the model's log-probs); parent, word, done_out, the histories and nbanned as
 *               cvc_beam_select_hist_parts writes them; nmet[r] = n(r) for every input row (nullable).  There is no implicit
 *               end-of-sentence rule: a hypothesis may end in any bank; min_len and bad_end compose as before.
 *   invariant   every slot with a finite score in bank j has exactly j active forced words in its history.
 * workspace: 21 * B * beam floats (the 17 of cvc_beam_select_hist_parts, then per row its values at the forced words and its met
 * mask).  The checks of cvc_beam_select_hist_parts with their codes; nforce outside [1, 3], beam % (nforce + 1) != 0, NULL force:
 * CVC_E_BADARG.  Nothing is launched on a refusal.  Bitwise deterministic. */
int cvc_beam_select_force_parts(const float* parts, int nparts, long long part_stride, const float* bias,
                                const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                                const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                                const int32_t* force, int nforce, int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out,
                                int32_t* nbanned, int32_t* nmet, float* workspace, cvc_stream_t stream);
/* cvc_beam_rank for the hypotheses of cvc_beam_select_force_parts (force, nforce, V, unk_idx as there).  len and norm as
 * cvc_beam_rank defines them; nmet[r] = the number of the clip's active forced words in r's T-step history.
 *   order[b, :] = the clip's slots by the key: norm is NaN, last; then norm == -inf; nmet descending; norm descending; lowest slot.
 * The best hypothesis is the best-normed one among those that met the most forced words.  The checks of cvc_beam_rank; NULL force or
 * nmet, nforce outside [1, 3], V < 1: CVC_E_BADARG. */
int cvc_beam_rank_force(const int64_t* hist, long long hist_stride, const float* score, const int32_t* force, int nforce, int B,
                        int beam, int T, int V, int unk_idx, float alpha, int64_t* order, float* norm, int32_t* len, int32_t* nmet,
                        cvc_stream_t stream);
/* Stochastic beam search (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them"; csrc/beam.hip: the STOCH forms
 * of the row scan and the merge of cvc_beam_select_hist_parts): a beam-search step whose ranking key is a Gumbel-perturbed sampling
 * log-prob, conditioned top-down so that a child's key never exceeds its parent's.  After T steps a clip's finite slots are a sample
 * WITHOUT replacement, in draw order, from q over length-T prefixes; slot 0 is an exact sample of q; all are pairwise distinct.
 *   state       row r = b * beam + k enters step t with its history (as cvc_beam_select_hist_parts), score_in[r] (the sum of the
 *               model's log-probs), logq_in[r] (its sampling log-prob) and G_in[r] (its perturbed key).  t == 0: only slot 0 of a clip
 *               is live and the caller hands it score = logq = G = 0; slots k > 0 are taken at G = -inf whatever the buffers hold.
 *   candidates  of a live row: the words outside Ban(t, r) of cvc_beam_select_hist_parts (UNK always, the rules of c when given).
 *               lse[r]  = the log-sum-exp of the full row, as in that block.
 *               lseq[r] = the log-sum-exp of z * inv_tau over the candidates ONLY: q(v | r) = exp(z * inv_tau - lseq) is renormalised
 *                         over what may be chosen, the distribution cvc_sample_select_parts / cvc_constrained_select_parts draw from
 *                         (their arg-max leaves the ban set out); with the full-row normaliser slot 0 would not be such a draw.
 *               phi(k, v) = logq_in[k] + (z[k, v] * inv_tau - lseq[k])
 *               g(k, v)   = phi(k, v) + gumbel(cvc_drop_hash(seed_lo, seed_hi, call, CVC_SBS_SITE + t, (r * V + v) mod 2^32)), gumbel
 *                           the definition of cvc_sample_select_parts (u = ((h >> 9) + 0.5) * 2^-23, -logf(-logf(u)))
 *               Z[k]      = max_v g(k, v) over the candidates
 *               key       gt = -log(exp(-G_in[k]) - exp(-Z[k]) + exp(-g)), computed as  d = g - Z;  l = log(-expm1(d)) for d > -ln 2,
 *                         else log1p(-exp(d));  u = (G_in - g) + l;  gt = (G_in - max(u, 0)) - log1p(exp(-|u|)).  The arg-max child
 *                         gets gt = G_in exactly.  Accurate logf / expf / log1pf / expm1f, fp32, no contraction.
 *   other rows  a frozen row (done_in) offers only (k, 0) at gt = G_in[k], logq and score carried; a row at G = -inf, or one whose
 *               every word is banned, offers only -inf.  No NaN leaves the block from such rows.
 *   selection   the `beam` largest gt of the clip, ties -> lowest flat (k, v); the i-th goes to slot i, so slots are in draw order and
 *               G_out is non-increasing over a clip's slots.  Fewer finite candidates than `beam`: fillers as in the history block,
 *               with score_out = logq_out = G_out = -inf.
 *   outputs     score_out = score_in[k] + (z[k, v] - lse[k]) on the RAW logit: the expression and the bits of the history block's
 *               candidate, so scores stay sums of the model's log-probs whatever inv_tau; logq_out = phi; G_out = gt; parent, word,
 *               done_out, the history gather and append, nbanned as cvc_beam_select_hist_parts writes them.
 *   mechanics   gt increases with g, so a row's top `beam` by gt are its top `beam` by s = z * inv_tau + noise: the row scan keeps a
 *               per-row top-`beam` (of s, in registers) and only the beam * beam finalists are transformed, in the merge, from the
 *               raw logit of each finalist, which the scan reloads (`beam` scalars per row, summed in the slab order) instead of
 *               holding a second register copy.  inv_tau == 1 and != 1 are one code path.
 * state: the sampler's device words {seed_lo, seed_hi, call, 0}, read by both kernels (cvc_sample_advance gives a replayed graph
 * fresh noise).  CVC_SBS_SITE + t is disjoint from CVC_SAMPLE_SITE + t', CVC_MIX_SITE + t' and the dropout sites for t, t' <= 64.
 * workspace: 26 * B * beam floats (the 17 of cvc_beam_select_hist_parts, then per row lseq and the raw logits of its 8 finalists).
 * The checks of cvc_beam_select_hist_parts with their codes; inv_tau not finite or <= 0, NULL state / logq_in / G_in / logq_out /
 * G_out, logq_in == logq_out, G_in == G_out, score_in == score_out: CVC_E_BADARG.  Nothing is launched on a refusal.  Graph-capturable;
 * bitwise deterministic for a given state. */
#define CVC_SBS_SITE 0x42000000u
int cvc_beam_select_stoch_parts(const float* parts, int nparts, long long part_stride, const float* bias,
                                const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                                const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                                float inv_tau, const uint32_t* state, const float* logq_in, const float* G_in,
                                int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out, float* logq_out, float* G_out,
                                int32_t* nbanned, float* workspace, cvc_stream_t stream);
/* cvc_beam_backtrack (include/cvc_hip.h) from slot start[b * start_stride] of clip b instead of slot 0 (the same kernel; the slot
 * is clamped to [0, beam) like a parent; start_stride = beam reads column 0 of cvc_beam_rank's order in place).  start == 0
 * everywhere: the bits of cvc_beam_backtrack.  Its checks; NULL start, start_stride < 1: CVC_E_BADARG. */
int cvc_beam_backtrack_from(const int64_t* words, const int64_t* parent, const float* att, int B, int beam, int T, int N,
                            const int64_t* start, long long start_stride, int64_t* seq, float* att_out, cvc_stream_t stream);
/* Teacher-forced decoding (csrc/forced.hip; row loader, argument checks and dispatch of csrc/select_row.h): the log-prob and the
 * rank of a GIVEN word per row, one workgroup per row.
 *   z[r, :]    = parts[0][r, :] + ... + parts[nparts-1][r, :] (+ bias), the order of cvc_tile_linear_finish -- the bits the other
 *                selection blocks see (nparts = 1, bias = NULL: a finished [M, V] logit matrix)
 *   w          = word[r * word_stride], read only (the block writes no word); w outside [0, V): logprob[r] = NaN, rank[r] = -1,
 *                and nothing is read at w
 *   logprob[r] = z[r, w] - logsumexp_v z[r, v]   (nullable; full V, UNK included: the definition of cvc_sample_select_parts)
 *   rank[r]    = #{v : z[r, v] > z[r, w]} + #{v < w : z[r, v] == z[r, w]}   (nullable; 0 <=> w is the arg-max under the lower-index
 *                tie rule; NaN logits compare false)
 * V <= 8192, M * V < 2^32 (CVC_E_TOOBIG otherwise); the argument checks every selection block shares.  Bitwise deterministic. */
int cvc_forced_select_parts(const float* parts, int nparts, long long part_stride, const float* bias, int M, int V,
                            const int64_t* word, int word_stride, float* logprob, int32_t* rank, cvc_stream_t stream);
int cvc_tile_lstm_finish(const float* parts, int nparts, long long part_stride, const float* b_ih, const float* b_hh,
                         const float* gate_bias, int gb_div, const float* c_prev, int M, int R, float* c_out,
                         float* h_out, void* frag1, long long frag1_stride, void* frag2, long long frag2_stride,
                         cvc_stream_t stream);
int cvc_tile_lstm_finish_embgate(const float* parts, int nparts, long long part_stride, const float* b_ih, const float* b_hh,
                                 const float* gate_bias, int gb_div, const float* emb_gate, const int64_t* word, int V,
                                 const float* c_prev, int M, int R, float* c_out, float* h_out, void* frag1,
                                 long long frag1_stride, void* frag2, long long frag2_stride, cvc_stream_t stream);
int cvc_tile_reorder_pack(const int64_t* parent, const int64_t* word, int beam, const float* h_att, const float* c_att,
                          const float* h_lang, const float* c_lang, const float* table, int E, int V,
                          float* c_att_prev, float* c_lang_prev, void* xa, long long xa_stride, void* xl_hlang,
                          long long xl_stride, int rows, int R, cvc_stream_t stream);
int cvc_decode_num_launches(const cvc_decode_plan* plan);                            /* kernels + copies per decode           */
/* test hook: every concat-GEMM on the generic direct-load kernel (see cvc_hip.h, cvc_linear_fwd) */
int cvc_gemm_force_generic(int on);
/* coverage hooks: select among kernel forms that the default path picks per shape (identical results) */
int cvc_tile_gemm_loaders(int on);
int cvc_gru_persistent_waves8(int on);   /* A/B + test hook: 1 (default) = 8 waves per workgroup where H % 256 == 0, 0 = always 4 */
/* ---- training forms of the once-per-clip encoder's small pieces (csrc/encoder_train.hip; model/backbone.py:55-81, 215-235,
 * 274-277, 325-333) -- used by the host mirror's encoder in train() mode (cvc/encoder_ops.py):
 *   cvc_relu_dropout_fwd / _bwd : y = max(x + bias, 0) * keep-mask multiplier of (site, flat index) -- the ReLU -> Dropout tail of the
 *       reference's Linear -> ReLU -> Dropout blocks, mask generated in the kernel (rng_state NULL or p == 0: plain ReLU);
 *       dx = dy * multiplier * [y > 0].  N % 4 == 0.
 *   cvc_bn_relu_train_fwd / _bwd : nn.BatchNorm1d on BATCH statistics over the rows of x [rows, C] (biased variance; running
 *       statistics updated with `momentum` and the unbiased variance, as the module does) followed by ReLU; save_mean / save_invstd [C]
 *       are kept for the backward, which also returns dgamma / dbeta.  workspace: cvc_bn_workspace(rows, C) floats.  C % 4 == 0.
 *   cvc_class_softmax_bwd : backward of cvc_class_softmax_fwd: p_rows [B*N, C] its softmax output, d_rows [B*N, C] / d_sim [B, C, N]
 *       (either nullable) the gradients of its two output layouts -> d_logits [B*N, C] (zero for padded regions).
 *   cvc_layernorm_cat_bwd : backward of cvc_layernorm_cat_fwd: d_out [rows, ld_out] -> dxs[s] [rows, lddx[s]] (nullable per input). */
int cvc_relu_dropout_fwd(const float* x, const float* bias, long long rows, int N, const uint32_t* rng_state, unsigned site,
                         float p, float* y, cvc_stream_t stream);
int cvc_relu_dropout_bwd(const float* dy, const float* y, long long n, const uint32_t* rng_state, unsigned site, float p, float* dx,
                         cvc_stream_t stream);
long long cvc_bn_workspace(long long rows, int C);
int cvc_bn_relu_train_fwd(const float* x, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                          float* running_var, long long rows, int C, float* y, float* save_mean, float* save_invstd,
                          float* workspace, cvc_stream_t stream);
int cvc_bn_relu_train_bwd(const float* x, const float* dy, const float* y, const float* gamma, const float* save_mean,
                          const float* save_invstd, long long rows, int C, float* dx, float* dgamma, float* dbeta,
                          float* workspace, cvc_stream_t stream);
int cvc_class_softmax_bwd(const float* p_rows, const float* d_rows, const float* d_sim, const uint8_t* pad, int B, int N, int C,
                          float* d_logits, cvc_stream_t stream);
int cvc_layernorm_cat_bwd(const float* const* xs, const long long* ldx, const int* widths, int nseg, long long rows, float eps,
                          const float* d_out, long long ld_out, float* const* dxs, const long long* lddx, cvc_stream_t stream);

/* out[row, :] = scale * sum_n w[row, n] X[row / nq, n, :] (w [nclip * nq, n], X [nclip, n, R], nq >= 2): the several-queries
 * weighted sum of cvc_attn_wsum without its softmax -- d_q of dot-product attention (model/modules.py:24-76 under autograd) with
 * w = d_scores, X = proj_context, scale = 1 / temp.  CVC_E_TOOBIG when no group of queries fits the LDS. */
int cvc_attn_weighted_rows(const float* w, const float* X, int nclip, int nq, int n, int R, float scale, float* out, cvc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Small helpers of the training step (deterministic; were library launches):
 * cvc_stable_order -- order[r] = index of the r-th key in a STABLE ascending sort of key[n] (n <= 7168): the row grouping of the
 *   embedding backward (torch.argsort(stable=True) in the host mirror);
 * cvc_col_sum -- out[c] (and out2[c] when given) = sum_s x[s * ld + c], s < S, c < n: bias gradients (nn.Linear / nn.LSTMCell
 *   bias_ih and bias_hh receive the same sum).  ws: cvc_col_sum_ws(S, n) floats (0 -> may be null): row chunks are summed by
 *   separate workgroups and combined by a second launch, fixed order. */
int cvc_stable_order(const int64_t* key, int n, int64_t* order, cvc_stream_t stream);
long long cvc_col_sum_ws(int S, int n);
int cvc_col_sum(const float* x, long long ld, int S, int n, float* out, float* out2, float* ws, cvc_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * LSTM recurrence of the frame-context encoder in its `bilstm` mode (csrc/lstm_seq.hip; reference backbone.py:94-106, 335-338):
 * the recurrent half of nn.LSTM(batch_first, bias) with h0 = c0 = 0, gate order (i, f, g, o), one or two directions (direction 1
 * walks the sequence from the end).  Operands as the GRU entry points of cvc_hip.h have them:
 *   wp     packed W_hh [ndir][H/8][Kp/4][32][4], Kp = H rounded up to 32 (cvc.lstm_seq.pack_lstm_weights: block b, row 8 g + u =
 *          gate g of hidden unit 8 b + u -- no zero rows);
 *   gi     the input projections W_ih x WITHOUT bias: row of (clip m, step t) at gi + m * gi_ld_m + t * gi_ld_t, columns [ndir][4][H];
 *   b_ih, b_hh  [ndir][4H];   y  h_t at y + m * y_ld_m + t * y_ld_t, columns [ndir][H].
 * Training forms additionally write, for every step and direction, what autograd needs:
 *   gates  ACTIVATED (i, f, g, o) at gates + m * g_ld_m + t * g_ld_t + d * 4H + {0, H, 2H, 3H};
 *   c      c_t at c + m * c_ld_m + t * c_ld_t + d * H.
 * Every pointer 16-byte aligned, every stride a multiple of 4 floats, M <= 64; CVC_E_BADARG without launching otherwise.
 *
 * cvc_lstm_seq_persistent_fwd / _train_fwd: one launch for the whole sequence, W_hh in registers, c in the registers of the
 *   workgroup that owns the unit (it never reaches memory in the inference form).  H % 128 == 0, H <= 1024, and a grid of
 *   (H/8, ndir) workgroups that is co-resident; CVC_E_BADARG without launching otherwise.  hq = (F + 1) * ndir * H * 64 floats (one
 *   state slot per step), sync = cvc_lstm_persistent_sync_words() words: arrival counters and, at word 4, an error word that is
 *   non-zero afterwards when a bounded barrier wait timed out -- the outputs are then invalid: repeat with the per-step form.
 * cvc_lstm_seq_fwd / _train_fwd: one launch per time step, any H % 8 == 0.  hq = 3 * ndir * Kp * 64 floats of workspace.
 *   Interchangeable with the persistent form within rounding (the two sum k in different orders), not bit for bit.
 * cvc_lstm_seq_bwd: walks the sequence backwards; per step and direction the gate gradients (dh = dY_t + dgates_{next} W_hh, dc
 *   carried through f) and dgates_t W_hh (cvc_linear_nn_planes_fwd on w_hh [ndir][4H, H], the checkpoint layout).  Output
 *   dg [F * M rows (t * M + m), ndir * 4H]: the pre-activation gradients -- b_ih and b_hh enter the same sum, so this one matrix
 *   gives dW_ih, dX, dW_hh and both biases in dense products over all steps.  work = cvc_lstm_seq_bwd_work(M, H, ndir) floats. */
int cvc_lstm_persistent_sync_words(void);
int cvc_lstm_seq_persistent_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih,
                                const float* b_hh, int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m,
                                long long y_ld_t, unsigned* sync, cvc_stream_t stream);
int cvc_lstm_seq_persistent_train_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih,
                                      const float* b_hh, int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m,
                                      long long y_ld_t, float* gates, long long g_ld_m, long long g_ld_t, float* c, long long c_ld_m,
                                      long long c_ld_t, unsigned* sync, cvc_stream_t stream);
int cvc_lstm_seq_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih, const float* b_hh,
                     int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m, long long y_ld_t, cvc_stream_t stream);
int cvc_lstm_seq_train_fwd(const float* wp, const float* gi, long long gi_ld_m, long long gi_ld_t, const float* b_ih,
                           const float* b_hh, int M, int F, int H, int ndir, float* hq, float* y, long long y_ld_m, long long y_ld_t,
                           float* gates, long long g_ld_m, long long g_ld_t, float* c, long long c_ld_m, long long c_ld_t,
                           cvc_stream_t stream);
int cvc_lstm_seq_bwd_work(int M, int H, int ndir);
int cvc_lstm_seq_bwd(const float* dy, long long dy_ld_m, long long dy_ld_t, const float* gates, long long g_ld_m, long long g_ld_t,
                     const float* c, long long c_ld_m, long long c_ld_t, const float* w_hh, int M, int F, int H, int ndir, float* dg,
                     float* work, cvc_stream_t stream);

/* ---- packed GEMMs with bf16-STORED weights (the WB16 mode of skinny_gemm_packed_kernel, csrc/gemm_packed.hip;
 * DecodeEngine(weights_dtype="bf16")).
 * wp: [ceil(Nout/32)][K/8][32 rows][8 k] bf16 (cvc.decode.pack_weights_bf16; row order of the fp32 pack), 16-byte aligned.
 * Activations, biases, state, accumulation and outputs are fp32 as in cvc_packed_lstm_embgate_ex_fwd / cvc_packed_linear_fwd;
 * every product is w * (x.hi + x.mid + x.lo), all three terms.  Bitwise equal (up to the sign of zero) to the fp32 entry points
 * in split mode 2 on a pack of the same, bf16-exact weights.
 *   lstm: emb_gate / word both set or both null; w_blk_stride = bf16 elements between 32-row blocks (0: dense, K * 32), K may
 *         stop short of the pack; w_cached: the weights keep the default cache policy instead of streaming non-temporally.
 *   linear: ksplit K slices into y + s * M * ldy (bias in slice 0), or row-major y, and / or top2_part records (ksplit == 1).
 * K % 32 == 0, 1 <= M <= 64, R % 8 == 0: else CVC_E_BADARG, before any launch. */
int cvc_packed_lstm_bf16w_fwd(const uint16_t* wp, long long w_blk_stride, const float* xq, int K, const float* b_ih,
                              const float* b_hh, const float* gate_bias, const float* emb_gate, const int64_t* word,
                              const float* c_prev_q, int M, int R, float* h_dst1_q, float* h_dst2_q, float* c_out_q,
                              int w_cached, cvc_stream_t stream);
int cvc_packed_linear_bf16w_fwd(const uint16_t* wp, const float* xq, int K, const float* bias, int M, int Nout, int ksplit,
                                float* y, int ldy, float* top2_part, cvc_stream_t stream);

/* ---- greedy word choice without a selection launch (csrc/sel_keys.h; DecodeEngine(tail="fused"), cvc_decode_desc.tail_keys).
 * A candidate (logit v, word n) is one 64-bit key, (ordered(v) << 32) | (0x7fffffff - n): its unsigned order is "value
 * descending, index ascending", -0 is encoded as +0, a NaN or -inf is never a candidate (as in the records of cvc_packed_linear_fwd), 0 = none.  Buffers of one step: keys
 * [4][64] (slot-major, 16-byte aligned) and key_unk [64] 64-bit words, both ZERO before the step's head runs; ms_part [ceil(V/32)][64][2] floats.
 *   cvc_packed_linear_keys_fwd: the vocabulary head y = x W^T + bias of cvc_packed_linear_fwd (same sums, bit for bit) whose
 *     epilogue posts, per 32-row block b and batch row m < M, the best candidate among the block's columns other than unk_idx to
 *     keys[b % 4][m] with one 64-bit integer max at device scope (no return value), unk_idx's own key to key_unk[m], and writes
 *     {max, sum exp(y - max)} over the block's columns to ms_part[b][m] -- the (mx, se) of cvc_packed_linear_fwd's records.
 *     No y, no records.
 *   cvc_packed_lstm_embgate_keys_fwd: cvc_packed_lstm_embgate_ex_fwd whose word of row m is decoded from keys / key_unk of the
 *     PREVIOUS step: k = max over keys[0..3][m]; k != 0: word 0x7fffffff - low32(k) (the best word other than UNK:
 *     captioner.py:415-422, best or second best if the best is UNK); else key_unk[m] != 0: unk_idx; else 0.
 *   cvc_keys_finalize: words [T][rows] int64 by that rule and logprob [T][rows] (nullable) = the chosen word's logit - (mx +
 *     log se) over the step's ms_part records, for all T steps in one launch; keys [T][4][64], key_unk [T][64], ms_part
 *     [T][nblocks][64][2].
 * Split mode 2 (cvc_gemm_packed_split) only, K % 32 == 0, 1 <= M (rows) <= 64, unk_idx >= 0: else CVC_E_BADARG, before any launch. */
int cvc_packed_linear_keys_fwd(const float* wp, const float* xq, int K, const float* bias, int M, int Nout, int unk_idx,
                               unsigned long long* keys, unsigned long long* key_unk, float* ms_part, cvc_stream_t stream);
int cvc_packed_lstm_embgate_keys_fwd(const float* wp, long long w_blk_stride, const float* xq, int K, const float* b_ih,
                                     const float* b_hh, const float* gate_bias, const float* emb_gate,
                                     const unsigned long long* keys, const unsigned long long* key_unk, int unk_idx,
                                     const float* c_prev_q, int M, int R, float* h_dst1_q, float* h_dst2_q, float* c_out_q,
                                     int w_cached, cvc_stream_t stream);
int cvc_keys_finalize(const unsigned long long* keys, const unsigned long long* key_unk, const float* ms_part, int nblocks, int T,
                      int rows, int unk_idx, int64_t* words, float* logprob, cvc_stream_t stream);

/* ---- self-critical training: the CIDEr-D reward of sampled captions (csrc/cider.hip; cvc.cider.CiderD, Trainer.scst_step).
 * A caption's words are its ids up to and including the first 0 (L words; all T without a 0).  An n-gram (n = 1..4) is an exact
 * 64-bit key: 16 bits per word holding id + 1, the first word in the highest bits, unused positions 0.
 *   cand [rows, T] int64: row c * per_clip + j = sample j of clip c;  refs [rows / per_clip, Rmax, T] int64, of which the first
 *   nref[clip] (int32, clamped to [0, Rmax]) count;  keys [G] ascending as unsigned values with idf [G] = ln N_doc - ln max(1, df)
 *   (computed in fp64 on the host), idf_unseen = ln N_doc for an n-gram that is not in the table (G = 0: keys / idf may be null).
 *   v_n[g] = count * idf[g];  s_n = sum_g min(v_n^c[g], v_n^r[g]) v_n^r[g] / (|v_n^c| |v_n^r|), 0 if a norm is 0, times
 *   exp(-(L_c - L_r)^2 / (2 sigma^2));  per_order [rows, 4] (nullable) = 10 * mean_r s_n;  reward [rows] = mean_n per_order,
 *   0 for a clip without references.
 * One wave per row, no atomics, fixed summation order: a row's result is bit-reproducible and independent of the other rows.
 * Null pointers, rows < 1, T < 1 or T > 63, rows % per_clip != 0, Rmax < 1, G < 0, sigma <= 0: CVC_E_BADARG, before any launch. */
int cvc_cider_d(const int64_t* cand, const int64_t* refs, const int32_t* nref, int rows, int T, int per_clip, int Rmax,
                const unsigned long long* keys, const float* idf, int G, float idf_unseen, float sigma, float* reward,
                float* per_order, cvc_stream_t stream);

/* ---- self-critical training: rewards -> per-token loss weights, one launch (csrc/cider.hip).
 *   per_clip = S > 1: adv[j] = reward[j] - (sum of the clip's other S - 1 rewards, ascending k) / (S - 1); base must be null.
 *   per_clip = 1:     adv[row] = reward[row] - base[row]; base (the greedy caption's reward) must be given.
 *   w[row, t] = adv[row] for the steps up to and including the first 0 of cand [rows, T], 0 after it (the mask of LMCriterion);
 *   w is row-major (row * T + t), or t-major (t * rows + row) with t_major != 0 -- the row order of the C-driven training loops.
 * Null pointers (but base), rows < 1, T < 1, rows % per_clip != 0, base given with S > 1 or missing with S = 1: CVC_E_BADARG. */
int cvc_scst_weights(const float* reward, const float* base, int rows, int per_clip, const int64_t* cand, int T, int t_major,
                     float* adv, float* w, cvc_stream_t stream);

/* ---- self-critical training on captions sampled WITHOUT replacement: importance weights, a per-row baseline and the per-token loss
 * weights, one launch (csrc/scst_wor.hip; cvc.hip.scst_weights_wor, model.scst_loss(wor=), Trainer.scst_step with opts.scst_wor).
 * The estimator of Kool, van Hoof and Welling 2019 ("Stochastic Beams and Where to Find Them" section 4; "Buy 4 REINFORCE Samples,
 * Get a Baseline for Free!") on the output of cvc_beam_select_stoch_parts run with beam = S + 1: slots 0 .. S-1 of a clip are its S
 * rollouts, slot S gives only its key, the threshold.  THIS COMMENT IS THE DEFINITION; the kernel and tests/wor_ref.py restate it.
 *   inputs      per clip b: reward f[b * S + i], i < S;  logq[b * (S + 1) + j] and G[b * (S + 1) + j], j <= S (a per-clip stride of
 *               S + 1);  state = the engine's generator words {seed_lo, seed_hi, call, 0} in device memory.
 *   derived     live_j = isfinite(G_j);  phi_i = logq_i;  kt = G_S;
 *               h = cvc_drop_hash(seed_lo, seed_hi, call, CVC_WOR_SITE, b);  u = ((h >> 9) + 0.5) * 2^-23;  a = -log u.
 *   root key    The engine starts a clip at G_root = 0, which conditions the largest perturbed log-prob on being 0.  The ORDER of the
 *               draws is unaffected, the GAPS between the keys are: the inclusion probability below assumes an unconditioned
 *               threshold.  With E = exp(-G), conditioning the minimum on another value shifts every E alike, so a ~ Exp(1) per clip
 *               stands for exp(-G_root), G_root ~ Gumbel(0), and only the threshold is re-conditioned: exp(-kappa) = a - 1 + exp(-kt).
 *   threshold   lambda = -kappa = -kt + log1p((a - 1) * exp(kt));  slot S not live: lambda = +inf (the beam holds every caption that
 *               exists);  kt = 0 gives lambda = log a.
 *   weight      d_i = phi_i + lambda;  x_i = exp(d_i);  log q_i = log(-expm1(-x_i)) -- for x_i < 1 taken as
 *               d_i + log(-expm1(-x_i) / x_i) with the ratio read as 1 when x_i underflows to 0, and 0 when x_i = inf;
 *               l_i = phi_i - log q_i for a live row, -inf for a dead one.  Everything stays in the log domain until a ratio is
 *               formed: exp(logq) is 0 in fp32 below -88 (ordinary early in training), the normalised weights are not.
 *   own sums    row i's sums carry row i with weight p_i = exp(phi_i) instead of w_i = exp(l_i):
 *               W_i = exp(phi_i) + sum_{j != i} exp(l_j);  B_i = exp(phi_i) f_i + sum_{j != i} exp(l_j) f_j;  W = sum_j exp(l_j);
 *               over live j < S in ascending j, every sum shifted by its largest exponent.
 *   normalize != 0 (what training uses; consistent, biased):
 *               wgt_i = exp(l_i) / W;  adv_i = n_live * wgt_i * (f_i - B_i / W_i);  est_b = sum_j wgt_j f_j;  n_live = the number of
 *               live rollouts (the loss stays on the scale of cvc_scst_weights': when every p is tiny against exp(kappa) all w_j are
 *               equal and adv_i is f_i minus the mean of the others, its leave-one-out advantage).
 *   normalize == 0 (exact, unbiased):
 *               wgt_i = exp(l_i);  adv_i = wgt_i * (f_i - B_i);  est_b = sum_j wgt_j f_j.
 *   dead rows   wgt = adv = 0;  a clip without a live rollout: est = 0.
 *   tokens      w[r, t] = adv_r over the steps up to and including the first 0 of cand [rows, T], else 0; row-major, or t-major with
 *               t_major != 0 (as cvc_scst_weights).
 *   arithmetic  accurate logf / expf / log1pf / expm1f, fp32, no contraction, fixed summation order: a row's outputs depend on its
 *               clip's inputs only and are bit-reproducible.  One thread per row, no atomics, no workspace.  Launch only (the state
 *               is read on the device): capturable in a HIP graph; a replay after cvc_sample_advance uses the new `call`.
 * CVC_WOR_SITE is disjoint from CVC_SAMPLE_SITE + t, CVC_MIX_SITE + t, CVC_SBS_SITE + t (t <= 64) and the dropout sites.
 * rows = B * S, per_clip = S;  outputs adv [rows], wgt [rows], est [B], w [rows * T].
 * A NULL pointer, per_clip < 2 (one rollout's own baseline cancels it) or > 7, rows < 1, rows % per_clip != 0, T < 1: CVC_E_BADARG,
 * before any launch; nothing is written. */
#define CVC_WOR_SITE 0x57000000u
int cvc_scst_weights_wor(const float* reward, const float* logq, const float* G, const uint32_t* state, int rows, int per_clip,
                         const int64_t* cand, int T, int t_major, int normalize, float* adv, float* wgt, float* est, float* w,
                         cvc_stream_t stream);

/* ---- token-overlap caption metrics: BLEU statistics, sentence BLEU-1..4 and ROUGE-L, one launch (csrc/overlap.hip; cvc.metrics).
 * cand / refs / nref / per_clip / Rmax as cvc_cider_d, on the same n-gram keys -- but a caption's words here are the ids BEFORE its
 * first 0 (the end mark is no word, what stands behind it is ignored; all T ids without a 0; L = 0 is possible).
 *   stats [rows, 10] int32, exact: correct_1..4 (sum over the candidate's distinct n-grams of min(count_c, max_r count_r)),
 *     guess_1..4 (max(0, Lc - n + 1)), cand_len Lc, ref_len (the counted reference length closest to Lc, the shorter on a tie; 0
 *     without a reference).
 *   lcs [rows, Rmax] int32 (nullable), exact: the longest-common-subsequence length against reference r; -1 in slots >= nref.
 *   bleu [rows, 4] fp32: p_n = (correct_n + 1e-15) / (guess_n + 1e-9), BLEU_k = bp exp((sum_{n<=k} log p_n) / k), bp = 1 if
 *     Lc >= ref_len else exp(1 - ref_len / Lc); 0 if Lc = 0 or the clip has no reference.
 *   rouge [rows] fp32: p = max_r lcs_r / Lc, q = max_r lcs_r / Lr (Lr = 0: 0), (1 + b^2) p q / (q + b^2 p) with b = 1.2; 0 if
 *     Lc = 0, no reference, or p q = 0.
 * One wave per row, no atomics: a row's result is bit-reproducible and independent of the other rows.
 * Null pointers (but lcs), rows < 1, T < 1 or T > 63, rows % per_clip != 0, Rmax < 1: CVC_E_BADARG, before any launch. */
int cvc_caption_overlap(const int64_t* cand, const int64_t* refs, const int32_t* nref, int rows, int T, int per_clip, int Rmax,
                        int32_t* stats, int32_t* lcs, float* bleu, float* rouge, cvc_stream_t stream);

/* ---- consensus (minimum-Bayes-risk) caption selection: pairwise CIDEr-D among a clip's candidates, one launch
 * (csrc/consensus.hip; cvc.cider.CiderD.consensus, cvc.decode.DecodeEngine.consensus).
 *   cand [rows, T] int64: row c * per_clip + j = candidate j of clip c;  live [rows] int32 (nullable: every row is live), a row with
 *   live == 0 is neither a candidate nor a reference;  keys / idf / G / idf_unseen / sigma and a caption's words as cvc_cider_d.
 *   utility [rows] fp32: the CIDEr-D of the row as the candidate against the clip's other live rows as the references, in ascending
 *     row order -- bit for bit what cvc_cider_d returns for that candidate and those references (per_clip = 1, nref = their number);
 *     0 for a dead row and for a row without another live row in its clip.
 *   pick [clips] int32: the index within the clip of the live row with the largest utility, the lowest index on a tie, 0 for a clip
 *     without a live row;  best [clips, T] int64: that row, all T ids.
 * One workgroup per clip; every caption's n-gram keys, counts, idf weights and norms are built once and kept in LDS for the pairs
 * (one table search per distinct n-gram per launch).  No atomics, no workspace: a clip's outputs are bit-reproducible and
 * independent of the other clips.  Launch only (no host read, no allocation): capturable in a HIP graph.
 * Null pointers (but live; keys / idf with G = 0), rows < 1, rows % per_clip != 0, per_clip < 1 or > 32, T < 1 or > 63, G < 0,
 * sigma <= 0: CVC_E_BADARG, before any launch. */
int cvc_consensus_cider(const int64_t* cand, const int32_t* live, int rows, int T, int per_clip, const unsigned long long* keys,
                        const float* idf, int G, float idf_unseen, float sigma, float* utility, int32_t* pick, int64_t* best,
                        cvc_stream_t stream);

/* ---- consensus selection under a weighted mix of utilities: the expected utility of every candidate against the clip's other
 * candidates, each of them ONE reference weighted by its probability, one launch (csrc/consensus_mix.hip; cvc.metrics.consensus,
 * cvc.decode.DecodeEngine.consensus with a utility mix or weights="model").
 *   cand, live, per_clip, keys / idf / G / idf_unseen / sigma as cvc_consensus_cider;  logw [rows] fp32 (nullable: uniform), the rows'
 *   log-weights, any temperature already applied;  coef [6] fp32 on the HOST, >= 0, in the order cider, bleu1, bleu2, bleu3, bleu4,
 *   rougel (cvc.metrics.REWARD_NAMES).  The table (keys, idf, G, idf_unseen, sigma) is read only with coef[0] > 0.
 *   Pair metrics, live i != j, row i the candidate and row j its only reference:
 *     cider(i; j): bit for bit what cvc_cider_d returns for that candidate and that single reference (words up to and including the
 *       first 0);  bleu_k(i; j), rouge(i; j): bit for bit cvc_caption_overlap's bleu and rouge for them (words before the first 0, the
 *       brevity penalty against row j's length).  A metric whose coefficient is 0 is not computed.
 *   u(i, j) = sum_k coef[k] * metric_k(i; j), added in the order of coef;
 *   w_j = expf(logw_j - max over the clip's live rows of logw): 1 at the maximum, 0 for logw_j = -inf or NaN (such a row is still a
 *     candidate but counts for nothing as a reference);
 *   utility [rows] fp32 = (sum_j w_j u(i, j)) / (sum_j w_j) over the live j != i, j ascending, both sums rounded term by term, fp32,
 *     no contraction; 0 for a dead row, a row without another live row, and a zero denominator.
 *   pick [clips] int32, best [clips, T] int64: as cvc_consensus_cider, on these utilities.
 *   pairs [clips, per_clip, per_clip, 6] fp32 (nullable): the six pair metrics, [c, i, j, k] = metric_k(i; j); zeros on the diagonal,
 *     for dead rows and for metrics with coefficient 0.
 * One workgroup per clip, every caption's windows, counts, idf weights, norms and lengths built once in LDS; one walk per pair serves
 * CIDEr-D's and BLEU's counts of all four orders and ROUGE-L's bit-vector LCS.  No atomics, no workspace: a clip's outputs are
 * bit-reproducible and independent of the other clips.  Launch only (no host read, no allocation): capturable in a HIP graph.
 * Null pointers (but live, logw, pairs; keys / idf with G = 0 or coef[0] = 0), rows < 1, rows % per_clip != 0, per_clip < 1 or > 32,
 * T < 1 or > 63, a negative or non-finite coefficient, all coefficients 0, coef[0] > 0 with sigma <= 0 or G < 0 or (G > 0 and a null
 * table): CVC_E_BADARG, before any launch, nothing written. */
int cvc_consensus_mix(const int64_t* cand, const int32_t* live, const float* logw, int rows, int T, int per_clip,
                      const unsigned long long* keys, const float* idf, int G, float idf_unseen, float sigma, const float* coef,
                      float* utility, int32_t* pick, int64_t* best, float* pairs, cvc_stream_t stream);

/* ---- caption-set diversity: distinct n-grams of a clip's candidate set, every candidate's BLEU statistics against the set's other
 * candidates (mBLEU), distinct captions; one launch (csrc/diversity.hip; cvc.metrics.set_diversity, DecodeEngine.set_diversity).
 *   cand [rows, T] int64, per_clip, live [rows] int32 (nullable: every row is live) as cvc_consensus_cider; a caption's words as
 *   cvc_caption_overlap: the ids BEFORE its first 0 (what stands behind it is ignored; all T ids without a 0; L = 0 is possible; UNK
 *   is a word like any other).  "Live rows": the clip's rows with live != 0.  Every output is written for every row and clip.
 *   set_stats [clips, 12] int32, exact:
 *     0..3  distinct_n, n = 1..4: the number of different n-grams of order n in the union of the live rows
 *     4..7  total_n = sum over the live rows of max(0, L - n + 1)  (total_1: the set's word count)
 *     8     live: the live rows;   9  unique: the live rows whose word sequence equals that of no EARLIER live row of the clip
 *     10    scored: live if live >= 2, else 0;   11  reserved, 0
 *   mbleu_stats [rows, 10] int32, mbleu [rows, 4] fp32: the row as the candidate against the clip's other live rows as its
 *     references, in ascending row order -- cvc_caption_overlap's stats layout (correct_1..4, guess_1..4, cand_len, ref_len) and
 *     floating-point expressions: bit for bit what cvc_caption_overlap returns for that candidate and those references.  All zeros
 *     for a dead row and for a row without another live row in its clip.
 * One workgroup per clip; every caption's 4-word windows are built once and kept in LDS for the pairs.  No atomics, no workspace: a
 * clip's outputs are bit-reproducible and independent of the other clips.  Launch only (no host read, no allocation): capturable
 * in a HIP graph.
 * Null pointers (but live), rows < 1, rows % per_clip != 0, per_clip < 1 or > 32, T < 1 or > 63: CVC_E_BADARG, before any launch. */
int cvc_caption_set_stats(const int64_t* cand, const int32_t* live, int rows, int T, int per_clip, int32_t* set_stats,
                          int32_t* mbleu_stats, float* mbleu, cvc_stream_t stream);

/* ---- spectral caption-set diversity: the eigenvalues of a clip's m x m caption-similarity matrix and the two scores formed from
 * them (Self-CIDEr, LSA-based diversity; Wang & Chan 2019), one launch (csrc/spectrum.hip; cvc.metrics.set_spectrum,
 * DecodeEngine.set_spectrum).
 *   cand [rows, T] int64, per_clip, live [rows] int32 (nullable: every row is live) and a caption's words as cvc_caption_set_stats.
 *   m = the clip's live rows; they are indexed 0 .. m - 1 in ascending row order.
 *   mode 0 (cider): v_n^a[g] = count_a(g) * idf(g), n = 1..4, idf from the sorted table keys / idf [G] as cvc_consensus_cider
 *     (idf_unseen for an absent key); s_n(a, b) = <v_n^a, v_n^b> / (|v_n^a| |v_n^b|), 0 when a norm is 0; K[a, b] = 1/4 sum_n s_n.
 *     Plain CIDEr similarity: no clipping, no length term, no factor 10; K[a, a] = min(L, 4) / 4 exactly where the idf are > 0.
 *   mode 1 (lsa): K[a, b] = sum_w count_a(w) count_b(w) over unigrams, exact; keys / idf / G / idf_unseen are not read.
 *   gram [clips, 32, 32] fp32 (nullable): K at the live rows' indices, exactly symmetric, 0 at indices >= m.
 *   lam [clips, 32] fp64: the eigenvalues of the m x m matrix in descending order, zeros behind them (two-sided Jacobi in fp64, a
 *     fixed parallel round-robin ordering; a rotation is skipped when |K_pq| <= 4 * 2^-53 * trace, a sweep without a rotation ends
 *     the solve, at most 16 sweeps).
 *   score [clips, 2] fp32, formed in fp64 and rounded once, tr = the trace taken before the solve:
 *     0: -log(min(lam_1 / tr, 1)) / log(m);   1: -log(sqrt(lam_1) / sum_i sqrt(max(lam_i, 0))) / log(m);   both 0 where m < 2 or tr = 0.
 *   info [clips, 2] int32: m; the sweeps run, -1 if the 16th still rotated.
 * One workgroup per clip, one wave solves.  No atomics, no workspace: a clip's outputs are bit-reproducible and independent of the
 * other clips.  Launch only (no host read, no allocation): capturable in a HIP graph.
 * Null pointers (but live and gram; keys / idf in mode 1 or with G = 0), rows < 1, rows % per_clip != 0, per_clip < 1 or > 32,
 * T < 1 or > 63, a mode other than 0 or 1, G < 0 in mode 0: CVC_E_BADARG, before any launch. */
int cvc_caption_set_spectrum(const int64_t* cand, const int32_t* live, int rows, int T, int per_clip, int mode,
                             const unsigned long long* keys, const float* idf, int G, float idf_unseen, float* gram, double* lam,
                             float* score, int32_t* info, cvc_stream_t stream);

/* ---- grounding F1 of generated captions: per object word the most attended proposal of every sampled frame, tested against the
 * clip's annotated boxes and counted per detection class, one launch (csrc/grounding.hip; cvc.metrics.grounding, Trainer.eval).
 *   seq [rows, T] int64: row r belongs to clip r / per_clip; its words are the ids before the first 0 (all T without one).
 *   att [rows, T, P] fp32: the weights over the clip's proposals; slot p belongs to frame p / Np, P <= F * Np is the trimmed axis (a
 *     slot >= P has weight -inf and a zero box).  ppls [rows / per_clip, P, 7] fp32 (x1, y1, x2, y2 first).
 *   gt_bboxs [rows / per_clip, K, 6] fp32 (x1, y1, x2, y2, frame, class), of which the first nbox[clip] (int32, clamped to [0, K])
 *     count; a box whose class is outside [1, C] is not counted.
 *   word_cls [V] int32: word id -> class in [1, C], anything else (and an id outside [0, V)): no object word.
 *   pick [rows, T, F] int32: for an object word t and a frame f the slot f * Np + j with the largest weight, the lowest j among
 *     equal maxima, j = 0 when no weight of the frame is > -inf or the first one is NaN; -1 everywhere else.
 *   A class is represented by its first object word; its box in frame f is ppls[clip, pick, 0:4]; it hits an annotated box when
 *   w = min(x2) - max(x1) > 0, h likewise, and 2 w h > area_a + area_g - w h (fp32, no +1 pixel, no contraction).
 *   table [C + 1, 6] int32, ADDED TO, per class: gt, gt_pred, gt_hit (boxes of the class; of a predicted class; hit by the
 *     representative's pick in the box's frame, which lies in [0, F)), pred, pred_in_gt, pred_hit (rows that predict the class; whose
 *     clip has a box of it; at least one of them hit).  counts [rows, 6] int32: the row's own sums over the classes, same order.
 *   f1 [rows] fp32: 2 p r / (p + r) with p = pred_hit / pred, r = gt_hit / gt of the row's counts; 0 when a denominator is 0.
 * One workgroup per row; integer atomics into the table: every output is bit-reproducible.  Launch only (no host read, no
 * allocation): capturable in a HIP graph.
 * Null pointers, rows < 1, T < 1 or > 63, P, F, Np, K, C, V or per_clip < 1, rows % per_clip != 0, P > F * Np: CVC_E_BADARG;
 * (T * F + 3 K) * 4 bytes > 48 KiB (the kernel's LDS): CVC_E_TOOBIG; both before any launch. */
int cvc_grounding_f1(const int64_t* seq, const float* att, const float* ppls, const float* gt_bboxs, const int32_t* nbox,
                     const int32_t* word_cls, int rows, int T, int P, int F, int Np, int K, int C, int V, int per_clip,
                     int32_t* pick, int32_t* counts, float* f1, int32_t* table, cvc_stream_t stream);

/* ---- label smoothing in the vocabulary criterion (csrc/vocab.hip; cvc.functional.vocab_head_nll / vocab_nll label_smoothing=).
 * The three forms of include/cvc_hip.h's criterion with the target distribution (1 - eps) onehot + eps / V of
 * torch.nn.functional.cross_entropy(label_smoothing=eps); the smoothing mass is uniform over all V ids.  Per row, with
 * lse = logsumexp(z):
 *   row_loss = w (lse - (1 - eps) z[t] - (eps / V) sum_v z[v])
 *   pre[v] / d_logits[v] = (g[0]) w (softmax(z)[v] - (1 - eps) [v == t] - eps / V)
 *   row_nll  = w (lse - z[t]), the unsmoothed value (logging), nll_sum[0] its sum over the rows in loss_sum's fixed order;
 *     row_nll and nll_sum are nullable, both or neither.
 * Every other argument, the size limits (fused head: V <= 8192) and the outputs are those of cvc_vocab_head_nll_fwd,
 * cvc_vocab_nll_fwd and cvc_vocab_nll_bwd.  The row's sum of logits is one more fixed-order block reduction: a row stays
 * bit-reproducible.  eps == 0 gives the bits of the unsmoothed entries.  w == 0 rows write zeros.
 * Null pointers (but bias, argmax, row_nll / nll_sum), eps outside [0, 1) or not finite, the unsmoothed entries' size limits:
 * CVC_E_BADARG, before any launch. */
int cvc_vocab_head_nll_ls_fwd(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                              const int64_t* target, const float* w, int M, int V, float eps, float* pre, int ld_pre,
                              int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll, float* nll_sum,
                              cvc_stream_t stream);
int cvc_vocab_nll_ls_fwd(const float* logits, const int64_t* target, const float* w, int M, int V, float eps, float* lse,
                         int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll, float* nll_sum, cvc_stream_t stream);
int cvc_vocab_nll_ls_bwd(const float* logits, const float* lse, const int64_t* target, const float* w, const float* g, int M,
                         int V, float eps, float* d_logits, cvc_stream_t stream);

/* ---- entropy regulariser in the vocabulary criterion (csrc/vocab.hip; cvc.functional.vocab_head_nll / vocab_nll entropy_beta=):
 * the entropy bonus of a policy-gradient loss (Williams & Peng 1991) and the confidence penalty of a cross-entropy loss (Pereyra et
 * al. 2017).  The three label-smoothing entries above with a coefficient beta (finite, any sign; beta > 0 rewards entropy) and an
 * entropy weight m [M] (the 0 / 1 loss mask) beside the NLL weight w [M] (the mask, or advantage x mask: any sign).  Per row, with
 * lse = logsumexp(z) and p[v] = exp(z[v] - lse):
 *   H        = sum_v p[v] (lse - z[v])       every term >= 0, a column at -inf adds exactly 0; summed, not formed as lse - sum p z
 *   row_loss = [the label-smoothing entry's, for w and eps]  -  beta m H
 *   pre[v] / d_logits[v] = [the label-smoothing entry's]  +  (g[0]) beta m p[v] (z[v] - lse + H)      exactly 0 at z[v] = -inf
 *   row_ent  = m H, always written; ent_sum[0] its sum over the rows in loss_sum's fixed order
 *   row_nll / nll_sum as above (nullable, both or neither).
 * H is the entropy of the model's full-vocabulary distribution at temperature 1.  It is one more pass over the row once lse is
 * known (each thread its columns in ascending order) and one more fixed-order block reduction: a row stays bit-reproducible, and
 * the fused and the two-step form agree bit for bit on equal logits.  beta == 0 (the monitor mode) gives the bits of the
 * label-smoothing entries in loss, pre and NLL and still writes row_ent.  m == 0 and w == 0: an exactly zero row.  The backward reads
 * the forward's row_ent and the same m.
 * The row values of these entries are formed in fp64 (the fp32 values exp(z - max) added in fp64, lse = max + log of that sum, H and
 * the three row expressions on top) and written as their fp32 value plus an fp32 remainder: row_lo [3, M] is that workspace (the
 * remainders of row_loss, row_ent, row_nll; contents are the forward's own business).  The sums are one launch behind the row
 * kernel: ent_sum, and with beta != 0 loss_sum and nll_sum, add value + remainder in fp64 in a fixed order and round once -- a sum
 * is the fp64 result rounded to fp32; with beta == 0 row_loss, row_nll and their sums are the label-smoothing entries' (their bits).
 * pre / d_logits are fp32 throughout.
 * Null pointers (but bias, argmax, row_nll / nll_sum; row_lo included), beta not finite, eps outside [0, 1), the unsmoothed entries'
 * size limits (fused head: V <= 8192): CVC_E_BADARG, before any launch. */
int cvc_vocab_head_nll_ent_fwd(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                               const int64_t* target, const float* w, const float* m, int M, int V, float eps, float beta,
                               float* pre, int ld_pre, int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll,
                               float* nll_sum, float* row_ent, float* ent_sum, float* row_lo, cvc_stream_t stream);
int cvc_vocab_nll_ent_fwd(const float* logits, const int64_t* target, const float* w, const float* m, int M, int V, float eps,
                          float beta, float* lse, int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll, float* nll_sum,
                          float* row_ent, float* ent_sum, float* row_lo, cvc_stream_t stream);
int cvc_vocab_nll_ent_bwd(const float* logits, const float* lse, const int64_t* target, const float* w, const float* m,
                          const float* row_ent, const float* g, int M, int V, float eps, float beta, float* d_logits,
                          cvc_stream_t stream);

/* Ensemble decoding (csrc/ensemble.hip; row loader, argument checks and NC / VEC choice of csrc/select_row.h): M members' logits ->
 * one [rows, V] matrix of combined log-probs, one workgroup per row; the selection block of the step then runs on `out` with
 * nparts = 1, bias = NULL.  src (HOST memory, M descriptors, copied into the kernel's arguments): member m's logits are
 * parts[0][r, :] + ... + parts[nparts-1][r, :] (+ bias) in the order of cvc_tile_linear_finish -- the bits that member's own selection
 * block sees; nparts and bias may differ between members.  logw (HOST memory, M floats): the log of the members' weights.
 *   lse_m[r]  = logsumexp_v x_m[r, v];   a_m[v] = (x_m[r, v] - lse_m) + logw[m]
 *   geometric == 0: out[r, v] = log sum_m w_m p_m(v), a streaming log-sum-exp over the members in index order (acc_0 = a_0, acc_m =
 *                   fmaxf(acc, a_m) + log1pf(expf(-fabsf(acc - a_m)))): finite for words far below every member's top, normalised
 *   geometric == 1: out[r, v] = sum_m expf(logw[m]) * (x_m[r, v] - lse_m), unnormalised (product of experts)
 * M == 1, logw = {0}: the row log-softmax.  Columns >= V of out are not written.  fp32, fixed order, no workspace, no atomics:
 * capturable, bitwise deterministic.  1 <= M <= CVC_ENSEMBLE_MAX, V <= 8192, rows * V < 2^32 (CVC_E_TOOBIG as the selection blocks);
 * NULL pointers, M out of range, ld_out < V, a non-finite logw, a member that fails the selection blocks' checks: CVC_E_BADARG. */
#define CVC_ENSEMBLE_MAX 8
typedef struct { const float* parts; int nparts; long long part_stride; const float* bias; } cvc_ensemble_src;
int cvc_ensemble_logprobs(const cvc_ensemble_src* src, int M, const float* logw, int geometric, int rows, int V, float* out,
                          int ld_out, cvc_stream_t stream);
/* out[i] = sum_m expf(logw[m]) * src[m][i], i < n, members in index order, fp32 (the ensemble's region attention).  src: HOST array
 * of M device pointers, logw: HOST memory; both travel in the kernel's arguments.  out may not alias a source other than src[0]. */
int cvc_ensemble_mix(const float* const* src, int M, const float* logw, long long n, float* out, cvc_stream_t stream);

/* ---- word-level distillation in the vocabulary criterion (csrc/distill.hip; cvc.functional.vocab_head_nll / vocab_nll distill=):
 * the criterion against a dense target row, a teacher's next-word distribution (Hinton et al. 2015; Kim & Rush 2016), mixed with the
 * one-hot loss.  Per row m with student logits z (the slabs summed in cvc_vocab_head_nll_fwd's order), teacher scores
 * s = teacher + map[m] * ld_t (any log-scale row, normalised or not; row_map NULL: map[m] = m; int32, device memory), alpha in [0, 1]
 * and tau > 0, with p = softmax(z), p_tau = softmax(z / tau), q = softmax(s / tau):
 *   row_nll  = w (lse(z) - z[t])                              unmixed
 *   row_kd   = w tau^2 sum_v q[v] (log q[v] - log p_tau[v])   unmixed; a teacher entry at -inf adds an exact 0
 *   row_loss = (1 - alpha) row_nll + alpha row_kd
 *   pre[v] / d_logits[v] = (g[0]) w ((1 - alpha) (p[v] - [v == t]) + alpha tau (p_tau[v] - q[v]))
 * loss_sum / nll_sum / kd_sum: the rows added in a fixed order, one launch behind the row kernel.  w == 0: an exactly zero row
 * whatever the teacher row holds.  A mapped teacher row outside [0, t_rows) is not read: that row's loss, kd and pre are NaN.
 * The fused form keeps both rows in registers (V <= 8192) and `pre` may alias slab 0; the two-step form takes any V and leaves
 * stats [5, M] for its backward (contents are the forward's own business).  On equal fp32 logits the two forms agree bit for bit.
 * fp32 only: the row values and their sums are carried as an fp32 value plus an fp32 remainder (error-free sums, fma products, a
 * split logarithm) and rounded once -- a row's KL is a small difference of large sums; pre / d_logits are plain fp32.  Fixed-order
 * reductions, no atomics, no workspace: capturable, bitwise deterministic.
 * Null pointers (but bias, argmax, row_map), alpha outside [0, 1], tau not finite or <= 0, ld_t < V (ld, ld_pre likewise), t_rows < 1,
 * the fused form's V > 8192: CVC_E_BADARG, before any launch. */
int cvc_vocab_head_nll_kd_fwd(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                              const int64_t* target, const float* w, const float* teacher, int ld_t, const int* row_map, int t_rows,
                              int M, int V, float alpha, float tau, float* pre, int ld_pre, int64_t* argmax, float* row_loss,
                              float* loss_sum, float* row_nll, float* nll_sum, float* row_kd, float* kd_sum, cvc_stream_t stream);
int cvc_vocab_nll_kd_fwd(const float* logits, const int64_t* target, const float* w, const float* teacher, int ld_t,
                         const int* row_map, int t_rows, int M, int V, float alpha, float tau, float* stats, int64_t* argmax,
                         float* row_loss, float* loss_sum, float* row_nll, float* nll_sum, float* row_kd, float* kd_sum,
                         cvc_stream_t stream);
int cvc_vocab_nll_kd_bwd(const float* logits, const float* stats, const int64_t* target, const float* w, const float* teacher,
                         int ld_t, const int* row_map, int t_rows, const float* g, int M, int V, float alpha, float tau,
                         float* d_logits, cvc_stream_t stream);

/* ---- SGD with momentum and Adamax behind the clip (csrc/optim.hip; cvc.optim.ClipSGD / ClipAdamax): the reference's other two
 * optimizers (main.py:182-191).  cvc_adam_clip_step (include/cvc_hip.h) with another update rule in its third launch: the same
 * segment and chunk tables, the same norm (chunk sums combined in chunk order), the same coefficient
 * coef = min(1, max_norm / (inv_world * norm + 1e-6)) * inv_world (max_norm <= 0: inv_world; a NaN norm: NaN), the same write_grad
 * (0 leave the gradients, 1 store g * coef, 2 store zero), `skip`, `partial` and `norm_coef`.  Per element, as written below:
 * what is spelled fma is one rounding, nothing else is contracted by the compiler, so that the float4 form (every operand of
 * the rule 16-byte aligned) and the scalar form give the same bits.  SGD's buffer is the one product-and-sum that is not fused.
 *   both      g = grad * coef;   ge = weight_decay != 0 ? fma(weight_decay, p, g) : g
 *   SGD       torch.optim.SGD, dampening 0, no Nesterov, no maximize.  m of the segment = momentum_buffer; v and step are NULL
 *             (the second launch increments only the step counts that are there).
 *               buf = round(momentum * buf) + ge;   p = fma(-lr, buf, p)
 *             The buffer's product is rounded before the sum, as torch's buf.mul_(momentum).add_(g) rounds it: under
 *             cancellation of momentum * buf against g an fma differs from torch's buffer by an ulp of the product, and the
 *             buffer is state that carries the difference into every later step.  A zero buffer gives torch's first step
 *             (buf = ge).  A segment whose m is NULL has no buffer: p = fma(-lr, ge, p), torch's momentum == 0.
 *   Adamax    torch.optim.Adamax, no maximize.  m = exp_avg, v = exp_inf, step = the step count (one float32 on the device, never
 *             NULL), t its value after the second launch's += 1.
 *               m = fma(ge - m, 1 - beta1, m);   u = max(beta2 * u, |ge| + eps);   p = fma(-(lr / (1 - powf(beta1, t))), m / u, p)
 *             The max is torch.maximum's: a NaN on either side gives NaN, so a NaN gradient element leaves NaN in u and p.
 * A void step (*skip != 0 when the launches execute) moves no parameter, state or step count and writes norm_coef = [0, 0];
 * write_grad == 2 still leaves the gradients zero.  Three launches, nothing read back by the host: capturable.
 * CVC_E_BADARG before any launch: a NULL segs / chunks / partial / norm_coef, nseg < 1, nchunk < 1, inv_world <= 0; momentum outside
 * [0, 1); beta1 or beta2 outside [0, 1), eps <= 0 (u = |ge| + eps must not be 0 where m / u is formed). */
int cvc_sgd_clip_step(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm, float inv_world,
                      float momentum, int write_grad, float* partial, float* norm_coef, const int* skip, cvc_stream_t stream);
int cvc_adamax_clip_step(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                         float inv_world, float beta1, float beta2, float eps, int write_grad, float* partial, float* norm_coef,
                         const int* skip, cvc_stream_t stream);

/* ---- Weight averaging (EMA) inside the optimizer step (csrc/optim.hip; cvc.optim._ClipStep.attach_ema).  The three clip + step
 * entries with a shadow per segment: ema[seg] (a device array of nseg device pointers, the segment's n floats each) is the
 * exponential moving average of that parameter, updated in the third launch from the p the rule has just produced, still in
 * registers:
 *     e = fma(p_new - e, 1 - d_eff, e)                       (1 - d_eff formed in fp32)
 * The lerp form: p_new == e leaves e's bits alone.  cvc_optim_seg's layout is unchanged; p, g, the state, the step counts, `partial`
 * and `norm_coef` get the bits of the plain entry.  ema[seg] == NULL: the segment has no shadow and is stepped exactly as the plain
 * entry steps it.  e counts as an operand of the float4 form (16-byte aligned with the rule's others, else the segment's scalar loop).
 * ema_state: two floats on the device, [0] = averaged steps so far, [1] = d_eff of the current step.  The second launch sets
 *     d_eff = warmup ? min(decay, (1 + n) / (10 + n)) : decay     (n = ema_state[0] before this step; the TensorFlow / timm warm-up)
 * and then ema_state[0] += 1.  A void step (*skip != 0) writes neither e nor ema_state.  Three launches, capturable.
 * CVC_E_BADARG before any launch: whatever the plain entry refuses, a NULL ema or ema_state, decay outside [0, 1) (NaN included).
 * cvc_ema_swap: p[i] <-> e[i] over the same tables (segments with a NULL shadow stay): the averaged weights in the parameters' own
 * storage and out again, bit for bit; twice is the identity.  One launch.  BADARG: a NULL table or ema, nseg < 1, nchunk < 1. */
int cvc_adam_clip_step_ema(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                           float inv_world, float beta1, float beta2, float eps, int write_grad, float* partial, float* norm_coef,
                           const int* skip, float* const* ema, float* ema_state, float decay, int warmup, cvc_stream_t stream);
int cvc_sgd_clip_step_ema(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                          float inv_world, float momentum, int write_grad, float* partial, float* norm_coef, const int* skip,
                          float* const* ema, float* ema_state, float decay, int warmup, cvc_stream_t stream);
int cvc_adamax_clip_step_ema(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float max_norm,
                             float inv_world, float beta1, float beta2, float eps, int write_grad, float* partial, float* norm_coef,
                             const int* skip, float* const* ema, float* ema_state, float decay, int warmup, cvc_stream_t stream);
int cvc_ema_swap(const cvc_optim_seg* segs, int nseg, const cvc_optim_chunk* chunks, int nchunk, float* const* ema,
                 cvc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CVC_HIP_BLOCKS_H */
