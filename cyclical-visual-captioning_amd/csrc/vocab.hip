// Word-embedding lookup (forward, backward, the counter-based dropout next to it) and the vocabulary head: log-softmax, masked NLL
// forward and backward, the fused criteria (vocab_nll*, vocab_head_nll) and the greedy top-2 with UNK suppression in its three forms.
// Reference: model/captioner.py:53-68 (embed), :266/:361/:437 (log_softmax(logit)),
// :415-422 (top-2 / UNK rule), misc/utils.py:132-146,181-192 (masked NLL).
// All of it is small elementwise / row-reduction work next to the streaming kernels; the
// point is to keep it on the device and inside the captured decode graph.
// (the beam blocks: csrc/beam.hip; the training step's pointwise backward and small reductions: csrc/lstm_pointwise_bwd.hip)
#include "row_block.h"
#include "sel_keys.h"
#include "gsk.h"
#include "dropout_rng.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------ embedding
__global__ __launch_bounds__(WG) void embed_relu_fwd_kernel(const float* table, const int64_t* idx, const float* drop, DropSpec rng,
                                                            int M, int E, float* out) {
    const int m = blockIdx.y;
    const int e = (blockIdx.x * WG + threadIdx.x) * 4;
    if (e >= E) return;
    f32x4 v = ld4(table + (size_t)idx[m] * E + e);
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    if (drop != nullptr) v *= ld4(drop + (size_t)m * E + e);
    if (rng.state != nullptr) {                               // mask of element (m, e) generated here (dropout_rng.h)
        const uint32_t s0 = rng.state[0], s1 = rng.state[1], s2 = rng.state[2], i0 = (uint32_t)m * (uint32_t)E + (uint32_t)e;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= cvc_drop_mult(rng, s0, s1, s2, i0 + k);
    }
    st4(out + (size_t)m * E + e, v);
}

// y = x * mask(site, element index): nn.Dropout with the counter-based masks, for the sites no producing kernel fuses
__global__ __launch_bounds__(WG) void dropout_rng_kernel(const float* x, DropSpec rng, size_t n, float* y) {
    const size_t i = ((size_t)blockIdx.x * WG + threadIdx.x) * 4;
    if (i >= n) return;
    const uint32_t s0 = rng.state[0], s1 = rng.state[1], s2 = rng.state[2];
    if (i + 4 <= n) {
        f32x4 v = ld4(x + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] *= cvc_drop_mult(rng, s0, s1, s2, (uint32_t)(i + k));
        st4(y + i, v);
    } else {
        for (size_t k = i; k < n; ++k) y[k] = x[k] * cvc_drop_mult(rng, s0, s1, s2, (uint32_t)k);
    }
}

// Deterministic scatter-add without atomics and without a host round trip: the host passes a stable argsort
// of the word indices, so the rows of one word are contiguous in `order` (a "run").  Two passes, both in a fixed
// order: (1) the sorted positions are cut into chunks of EMB_CHUNK; a workgroup walks its chunk and writes one
// partial sum per (word, chunk) piece to part[first sorted position of the piece]; (2) the workgroup of a run's
// first position adds the run's pieces (its own, then the ones starting at the following chunk boundaries) and
// writes that word's gradient row.  A long run -- the BOS / padding word owns about a third of the B*T rows --
// is thereby summed by run/EMB_CHUNK workgroups in parallel instead of one workgroup walking it row by row.
constexpr int EMB_CHUNK = 16;

__global__ __launch_bounds__(WG) void embed_bwd_pieces_kernel(const int64_t* idx, const int64_t* order, const float* drop, DropSpec rng,
                                                              const float* d_out, int M, int E, float* part) {
    const int r0 = blockIdx.y * EMB_CHUNK;
    const int e = (blockIdx.x * WG + threadIdx.x) * 4;
    if (e >= E) return;
    const int r1 = min(M, r0 + EMB_CHUNK);
    int start = r0;
    int64_t w = idx[order[r0]];
    f32x4 acc = {0, 0, 0, 0};
    for (int r = r0; r < r1; ++r) {
        const int64_t m = order[r];
        const int64_t wr = idx[m];
        if (wr != w) {                                         // the piece ends: flush it, open the next one
            st4(part + (size_t)start * E + e, acc);
            acc = f32x4{0, 0, 0, 0};
            start = r;
            w = wr;
        }
        f32x4 g = ld4(d_out + (size_t)m * E + e);
        if (drop != nullptr) g *= ld4(drop + (size_t)m * E + e);
        if (rng.state != nullptr) {                           // the forward's mask, regenerated
            const uint32_t s0 = rng.state[0], s1 = rng.state[1], s2 = rng.state[2], i0 = (uint32_t)m * (uint32_t)E + (uint32_t)e;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] *= cvc_drop_mult(rng, s0, s1, s2, i0 + k);
        }
        acc += g;
    }
    st4(part + (size_t)start * E + e, acc);
}

__global__ __launch_bounds__(WG) void embed_bwd_runs_kernel(const float* table, const int64_t* idx, const int64_t* order,
                                                            const float* part, int M, int E, float* d_table) {
    const int r0 = blockIdx.y;
    const int64_t w = idx[order[r0]];
    if (r0 > 0 && idx[order[r0 - 1]] == w) return;            // not the first row of its word
    const int e = (blockIdx.x * WG + threadIdx.x) * 4;
    if (e >= E) return;
    f32x4 acc = ld4(part + (size_t)r0 * E + e);               // the piece that starts the run
    for (int r = (r0 / EMB_CHUNK + 1) * EMB_CHUNK; r < M && idx[order[r]] == w; r += EMB_CHUNK)
        acc += ld4(part + (size_t)r * E + e);                 // pieces that start at the following chunk boundaries
    const f32x4 t = ld4(table + (size_t)w * E + e);
    acc.x = t.x > 0.f ? acc.x : 0.f; acc.y = t.y > 0.f ? acc.y : 0.f;
    acc.z = t.z > 0.f ? acc.z : 0.f; acc.w = t.w > 0.f ? acc.w : 0.f;
    // ACCUMULATED: a fresh gradient starts from the caller's zero fill (0 + x = x exactly); the three embeddings of a cyclical
    // pass (loops A, B, C share the table, captioner.py:53-68) add up in ONE buffer, call after call, instead of in three
    st4(d_table + (size_t)w * E + e, ld4(d_table + (size_t)w * E + e) + acc);
}

// ------------------------------------------------------------------ log-softmax / top-2 / NLL
__global__ __launch_bounds__(WG) void log_softmax_kernel(const float* logits, int V, float* logp) {
    __shared__ float red[4];
    const float* x = logits + (size_t)blockIdx.x * V;
    float* y = logp + (size_t)blockIdx.x * V;
    float m = -INFINITY;
    for (int v = threadIdx.x; v < V; v += WG) m = fmaxf(m, x[v]);
    m = block_max(m, red);
    float s = 0.f;
    for (int v = threadIdx.x; v < V; v += WG) s += expf(x[v] - m);
    s = block_sum(s, red);
    const float lse = m + logf(s);
    for (int v = threadIdx.x; v < V; v += WG) y[v] = x[v] - lse;
}

// d_x = d_y - exp(y) * sum(d_y)   (y = log_softmax(x))
__global__ __launch_bounds__(WG) void log_softmax_bwd_kernel(const float* logp, const float* d_logp, int V, float* d_logits) {
    __shared__ float red[4];
    const size_t o = (size_t)blockIdx.x * V;
    float s = 0.f;
    for (int v = threadIdx.x; v < V; v += WG) s += d_logp[o + v];
    s = block_sum(s, red);
    for (int v = threadIdx.x; v < V; v += WG) d_logits[o + v] = d_logp[o + v] - expf(logp[o + v]) * s;
}

// d_logp[m, :] = 0 except d_logp[m, target[m]] = -w[m] * g[0]
__global__ __launch_bounds__(WG) void nll_bwd_kernel(const int64_t* target, const float* w, const float* g, int V,
                                                     float* d_logp) {
    const int m = blockIdx.y;
    const int v = blockIdx.x * WG + threadIdx.x;
    if (v >= V) return;
    d_logp[(size_t)m * V + v] = v == (int)target[m] ? -w[m] * g[0] : 0.f;
}

struct Top2 { float v1; int i1; float v2; int i2; };
__device__ __forceinline__ Top2 merge(Top2 a, Top2 b) {
    Top2 r;
    if (better(a.v1, a.i1, b.v1, b.i1)) {
        r.v1 = a.v1; r.i1 = a.i1;
        if (better(a.v2, a.i2, b.v1, b.i1)) { r.v2 = a.v2; r.i2 = a.i2; } else { r.v2 = b.v1; r.i2 = b.i1; }
    } else {
        r.v1 = b.v1; r.i1 = b.i1;
        if (better(b.v2, b.i2, a.v1, a.i1)) { r.v2 = b.v2; r.i2 = b.i2; } else { r.v2 = a.v1; r.i2 = a.i1; }
    }
    return r;
}

__global__ __launch_bounds__(WG) void top2_unk_kernel(const float* logits, int V, int unk, int64_t* word, int wstride,
                                                      float* logprob) {
    __shared__ float red[4];
    __shared__ Top2 tred[4];
    const int row = blockIdx.x;
    const float* x = logits + (size_t)row * V;
    Top2 t{-INFINITY, 0x7fffffff, -INFINITY, 0x7fffffff};
    for (int v = threadIdx.x; v < V; v += WG) {
        const float xv = x[v];
        if (better(xv, v, t.v1, t.i1)) { t.v2 = t.v1; t.i2 = t.i1; t.v1 = xv; t.i1 = v; }
        else if (better(xv, v, t.v2, t.i2)) { t.v2 = xv; t.i2 = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 u;
        u.v1 = __shfl_xor(t.v1, o, 64); u.i1 = __shfl_xor(t.i1, o, 64);
        u.v2 = __shfl_xor(t.v2, o, 64); u.i2 = __shfl_xor(t.i2, o, 64);
        t = merge(t, u);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) tred[wave] = t;
    __syncthreads();
    t = merge(merge(tred[0], tred[1]), merge(tred[2], tred[3]));
    const float m = t.v1;
    float s = 0.f;
    for (int v = threadIdx.x; v < V; v += WG) s += expf(x[v] - m);
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        const bool use2 = (t.i1 == unk) && V > 1;        // captioner.py:417-421
        int w = use2 ? t.i2 : t.i1;
        if ((unsigned)w >= (unsigned)V) w = 0;             // all-NaN row (diverged checkpoint): nothing compares greater; stay in range
        word[(size_t)row * wstride] = w;
        if (logprob != nullptr) logprob[row] = (use2 ? t.v2 : t.v1) - (m + logf(s));
    }
}

// Final stage of the fused vocabulary head: merge the per-block partial records written by the logits
// GEMM epilogue ({top1 v,i, top2 v,i, max, sumexp} per 32-column block and row), apply the UNK rule,
// emit the word, its log-prob, and (optionally) next step's embedded word relu(Emb[word]).
__global__ __launch_bounds__(WG) void top2_final_kernel(const float* part, int nblocks, int unk, int64_t* word, int wstride,
                                                        float* logprob, const float* table, int E, float* emb_out, int emb_ld) {
    __shared__ float red[4];
    __shared__ Top2 tred[4];
    __shared__ int chosen;
    const int row = blockIdx.x;
    Top2 t{-INFINITY, 0x7fffffff, -INFINITY, 0x7fffffff};
    float mx = -INFINITY;
    for (int b = threadIdx.x; b < nblocks; b += WG) {
        const float* rec = part + ((size_t)b * 64 + row) * 6;
        Top2 u{rec[0], __float_as_int(rec[1]), rec[2], __float_as_int(rec[3])};
        t = merge(t, u);
        mx = fmaxf(mx, rec[4]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 u;
        u.v1 = __shfl_xor(t.v1, o, 64); u.i1 = __shfl_xor(t.i1, o, 64);
        u.v2 = __shfl_xor(t.v2, o, 64); u.i2 = __shfl_xor(t.i2, o, 64);
        t = merge(t, u);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) tred[wave] = t;
    mx = block_max(mx, red);                       // (contains the barriers that publish tred)
    t = merge(merge(tred[0], tred[1]), merge(tred[2], tred[3]));
    float se = 0.f;
    for (int b = threadIdx.x; b < nblocks; b += WG) {
        const float* rec = part + ((size_t)b * 64 + row) * 6;
        se += rec[5] * expf(rec[4] - mx);
    }
    se = block_sum(se, red);
    if (threadIdx.x == 0) {
        const bool use2 = (t.i1 == unk) && t.i2 != 0x7fffffff;          // captioner.py:417-421
        int w = use2 ? t.i2 : t.i1;
        if (w == 0x7fffffff || w < 0) w = 0;               // all-NaN logits: no record ever compared greater; the word is
                                                           // also a gather address (table + w * E) here and next step
        word[(size_t)row * wstride] = w;
        if (logprob != nullptr) logprob[row] = (use2 ? t.v2 : t.v1) - (mx + logf(se));
        chosen = w;
    }
    if (emb_out != nullptr) {
        __syncthreads();
        const float* src = table + (size_t)chosen * E;
        for (int e = threadIdx.x * 4; e < E; e += WG * 4) {
            f32x4 v = ld4(src + e);
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            if (emb_ld > 0) st4(emb_out + (size_t)row * emb_ld + e, v);
            else st4(emb_out + ((size_t)(e >> 2) * 64 + row) * 4, v);       // emb_ld == 0: quad layout [E/4][64][4]
        }
    }
}

// The fused greedy tail's only selection work outside the critical path (sel_keys.h): one workgroup per (step, row) decodes the
// word from the step's keys and sums the step's per-block (max, sum-exp) records for the log-prob exactly as top2_final_kernel sums
// its records (same strides, same reductions: the same bits); one launch per decode.
__global__ __launch_bounds__(WG) void keys_finalize_kernel(const unsigned long long* keys, const unsigned long long* key_unk, const float* ms_part,
                                                           int nblocks, int T, int rows, int unk, int64_t* words, float* logprob) {
    __shared__ float red[4];
    const int item = blockIdx.x;
    const int t = item / rows, row = item - t * rows;
    const float* ms = ms_part + ((size_t)t * nblocks * 64 + row) * 2;
    float mx = -INFINITY;
    for (int b = threadIdx.x; b < nblocks; b += WG) mx = fmaxf(mx, ms[(size_t)b * 128]);
    mx = block_max(mx, red);
    float se = 0.f;
    for (int b = threadIdx.x; b < nblocks; b += WG) se += ms[(size_t)b * 128 + 1] * expf(ms[(size_t)b * 128] - mx);
    se = block_sum(se, red);
    if (threadIdx.x == 0) {
        const unsigned long long* kp = keys + (size_t)t * KEY_SLOTS * KEY_ROWS + row;
        unsigned long long kb = 0ull;
#pragma unroll
        for (int s = 0; s < KEY_SLOTS; ++s) kb = kp[s * KEY_ROWS] > kb ? kp[s * KEY_ROWS] : kb;
        const unsigned long long ku = key_unk[(size_t)t * KEY_ROWS + row];
        words[item] = sel_key_word(kb, ku, unk);
        if (logprob != nullptr) {
            const float v = kb != 0ull ? sel_key_value(kb) : (ku != 0ull ? sel_key_value(ku) : -INFINITY);
            logprob[item] = v - (mx + logf(se));
        }
    }
}

// Word selection straight from the partial tiles of a stream-K vocabulary GEMM (gemm_gsk.hip): one workgroup per batch row sums
// the segments of its 32-column blocks (+ bias), takes top-2 / max / sum-exp over the row and finishes like top2_final_kernel.
// ITEMS float4 items per thread (item = 4 columns of one block), every segment load of every item requested before the first
// sum: the kernel is one round trip to the slabs, not ITEMS x segments of them.
template <int ITEMS>
__global__ __launch_bounds__(WG) void top2_slab_kernel(GskSegs g, const float* bias, int V, int unk, int64_t* word, int wstride,
                                                       float* logprob, const float* table, int E, float* emb_out, int emb_ld) {
    __shared__ float red[4];
    __shared__ Top2 tred[4];
    __shared__ int chosen;
    constexpr int MAXS = 6;
    const int row = blockIdx.x;
    const int nitem = ((V + 31) >> 5) * 8;
    f32x4 sv[ITEMS][MAXS], bv[ITEMS];
    int nseg[ITEMS], col0[ITEMS];
    const float* p0[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        const int it = min((int)threadIdx.x + k * WG, nitem - 1);          // past the end: re-read the last item (masked below)
        const int blk = it >> 3, rq = it & 7;
        nseg[k] = gsk_nseg(g, blk >> 3);
        col0[k] = (int)threadIdx.x + k * WG < nitem ? blk * 32 + rq * 4 : V;
        p0[k] = gsk_part(g, blk >> 3, 0, blk & 7) + (size_t)row * 32 + rq * 4;
#pragma unroll
        for (int s = 0; s < MAXS; ++s) sv[k][s] = ld4(p0[k] + (size_t)(s < nseg[k] ? s : nseg[k] - 1) * (8 * 2048));
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[k][e] = (bias != nullptr && col0[k] + e < V) ? bias[col0[k] + e] : 0.f;
    }
    Top2 t{-INFINITY, 0x7fffffff, -INFINITY, 0x7fffffff};
    float mx = -INFINITY;
    f32x4 val[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        f32x4 x = sv[k][0];
#pragma unroll
        for (int s = 1; s < MAXS; ++s) x += s < nseg[k] ? sv[k][s] : f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = MAXS; s < nseg[k]; ++s) x += ld4(p0[k] + (size_t)s * (8 * 2048));
        x += bv[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = col0[k] + e;
            const float xv = v < V ? x[e] : -INFINITY;
            val[k][e] = xv;
            if (v < V) {
                if (better(xv, v, t.v1, t.i1)) { t.v2 = t.v1; t.i2 = t.i1; t.v1 = xv; t.i1 = v; }
                else if (better(xv, v, t.v2, t.i2)) { t.v2 = xv; t.i2 = v; }
                mx = fmaxf(mx, xv);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 u;
        u.v1 = __shfl_xor(t.v1, o, 64); u.i1 = __shfl_xor(t.i1, o, 64);
        u.v2 = __shfl_xor(t.v2, o, 64); u.i2 = __shfl_xor(t.i2, o, 64);
        t = merge(t, u);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) tred[wave] = t;
    mx = block_max(mx, red);                       // (contains the barriers that publish tred)
    t = merge(merge(tred[0], tred[1]), merge(tred[2], tred[3]));
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) se += val[k][e] == -INFINITY ? 0.f : expf(val[k][e] - mx);
    se = block_sum(se, red);
    if (threadIdx.x == 0) {
        const bool use2 = (t.i1 == unk) && t.i2 != 0x7fffffff;          // captioner.py:417-421
        int w = use2 ? t.i2 : t.i1;
        if (w == 0x7fffffff || w < 0) w = 0;               // all-NaN logits: see top2_final_kernel
        word[(size_t)row * wstride] = w;
        if (logprob != nullptr) logprob[row] = (use2 ? t.v2 : t.v1) - (mx + logf(se));
        chosen = w;
    }
    if (emb_out != nullptr) {
        __syncthreads();
        const float* src = table + (size_t)chosen * E;
        for (int e = threadIdx.x * 4; e < E; e += WG * 4) {
            f32x4 v = ld4(src + e);
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            if (emb_ld > 0) st4(emb_out + (size_t)row * emb_ld + e, v);
            else st4(emb_out + ((size_t)(e >> 2) * 64 + row) * 4, v);       // emb_ld == 0: quad layout [E/4][64][4]
        }
    }
}

__global__ __launch_bounds__(WG) void nll_fwd_kernel(const float* logp, const int64_t* target, const float* w, int M, int V,
                                                     float* loss_sum) {
    __shared__ float red[4];
    float s = 0.f;
    for (int m = threadIdx.x; m < M; m += WG) {
        const float wm = w[m];
        if (wm != 0.f) s -= wm * logp[(size_t)m * V + target[m]];
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) loss_sum[0] += s;
}

// Fused vocabulary criterion: one pass over a row of raw logits gives its log-sum-exp, its argmax (ties -> lowest
// index, what torch.max over the log-probs returns) and the row's weighted NLL; no [M, V] log-prob matrix is written.
// LS: label smoothing eps in [0, 1), the target distribution (1 - eps) onehot + eps / V (F.cross_entropy's label_smoothing):
//     row_loss = w (lse - (1 - eps) x[t] - (eps / V) sum_v x[v]),   row_nll = w (lse - x[t]) (the unsmoothed value, nullable)
// -- the row's sum is taken in the pass that looks for the maximum, one more fixed-order block reduction.  eps == 0 gives the
// bits of the LS = false form.
// ENT (with LS): the entropy regulariser beta (finite, any sign) with the entropy weight mrow (the 0 / 1 loss mask):
//     H = sum_v p[v] (lse - z[v]),  p[v] = exp(z[v] - lse)      (every term >= 0; a column at -inf adds exactly 0)
//     row_loss -= beta mrow H,   pre[v] += beta mrow p[v] (z[v] - lse + H)  (exactly 0 at -inf),   row_ent = mrow H
// -- H is one more pass over the row once lse is known, each thread adding its columns in ascending order, and one more
// fixed-order block reduction.  beta == 0 takes the LS expressions in a uniform branch (the same bits) and still writes row_ent.
// The expressions below are shared by the fused and the two-step kernels and are kept from contraction, so that the two forms
// round alike: on equal logits they agree bit for bit.
// The ROW VALUES of this form are formed in fp64: the fp32 values exp(z - max) are added in fp64 (sd), lse = max + log(sd),
// H = sum_v e[v] (lse - z[v]) / sd, and the row's loss, NLL and entropy are fp64 expressions of these.  Each is written as its
// fp32 value plus an fp32 remainder (row_lo), so that the sums over the rows lose nothing to the rows' rounding: a sum is then
// the fp64 value rounded once.  (What fp32 costs here: a row's lse carries 5e-7 and a sum of 33 rows of 20 some 1e-5; the price
// is two more expf passes over the registers and fp64 adds.)  pre and d_logits stay fp32, with the fp32 lse and H rounded to fp32.
// (a column at -inf: e = 0 and lse - z = +inf, whose product would be a NaN -- the difference is clamped to a finite value, so
// the term is an exact 0 without a compare per column)
__device__ __forceinline__ double block_sum_wide(double v, double* dred) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) dred[threadIdx.x >> 6] = v;
    __syncthreads();
    return (dred[0] + dred[1]) + (dred[2] + dred[3]);
}
__device__ __forceinline__ double ent_acc_wide(double h, float e, float z, double lse) {
#pragma clang fp contract(off)
    return h + (double)e * fmin(lse - (double)z, 1e300);
}
struct EntRow { double loss, nll, ent; };
__device__ __forceinline__ EntRow ent_rows_wide(float wm, float mm, float beta, double lse, float xt, float eps, float zs, int V, double H) {
#pragma clang fp contract(off)
    EntRow r;
    r.nll = wm != 0.f ? (double)wm * (lse - (double)xt) : 0.0;
    double base = r.nll;
    if (wm != 0.f && eps != 0.f) base = (double)wm * (lse - (double)(1.f - eps) * (double)xt - (double)(eps / (float)V) * (double)zs);
    const double coef = (double)beta * (double)mm;
    r.loss = coef != 0.0 ? base - coef * H : base;
    r.ent = mm != 0.f ? (double)mm * H : 0.0;
    return r;
}
// v as an fp32 value and the fp32 remainder behind it (0 behind a value that is not finite)
__device__ __forceinline__ void put_wide(float* hi, float* lo, double v) {
    const float h = (float)v;
    *hi = h;
    *lo = h - h == 0.f ? (float)(v - (double)h) : 0.f;
}
__device__ __forceinline__ float ent_row_loss(float wm, float coef, float lse, float xt, float eps, float zs, int V, float H) {
#pragma clang fp contract(off)
    float base = 0.f;
    if (wm != 0.f) base = eps == 0.f ? wm * (lse - xt) : wm * (lse - (1.f - eps) * xt - (eps / (float)V) * zs);
    return coef != 0.f ? base - coef * H : base;
}
// gw: the NLL weight (times the upstream scalar in the two-step backward), coef: beta x mrow (times the same scalar), hit: the
// target's share at this column (ent_hit at the target, else 0), all: every column's share (ent_all)
__device__ __forceinline__ float ent_hit(float eps) { return eps == 0.f ? 1.f : 1.f - eps; }
__device__ __forceinline__ float ent_all(float eps, int V) { return eps == 0.f ? 0.f : eps / (float)V; }
__device__ __forceinline__ float ent_pre(float gw, float coef, float z, float lse, float hit, float all, float H) {
#pragma clang fp contract(off)
    const float p = expf(z - lse);
    const float base = gw != 0.f ? gw * (p - hit - all) : 0.f;
    const float both = base + coef * p * (fmaxf(z - lse, -3.402823466e+38f) + H);       // (z = -inf: p = 0, an exact 0)
    return coef == 0.f ? base : both;
}

template <bool LS, bool ENT = false>
__global__ __launch_bounds__(WG) void vocab_nll_fwd_kernel(const float* logits, const int64_t* target, const float* w, int V,
                                                           float* lse_out, int64_t* argmax, float* row_loss, float eps, float* row_nll,
                                                           float beta = 0.f, const float* mrow = nullptr, float* row_ent = nullptr,
                                                           float* row_lo = nullptr) {
    static_assert(LS || !ENT, "the entropy form is built on the label-smoothing form");
    __shared__ float red[4];
    __shared__ int ired[4];
    __shared__ double dred[4];
    const int row = blockIdx.x;
    const float* x = logits + (size_t)row * V;
    float m = -INFINITY;
    int mi = 0x7fffffff;
    float zs = 0.f;
    for (int v = threadIdx.x; v < V; v += WG) {
        const float xv = x[v];
        if (xv > m) { m = xv; mi = v; }                       // ascending v per thread: first occurrence wins
        if (LS) zs += xv;
    }
    const float bm = block_max(m, red);
    int cand = m == bm ? mi : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ired[threadIdx.x >> 6] = cand;
    __syncthreads();
    const int best = min(min(ired[0], ired[1]), min(ired[2], ired[3]));
    float s = 0.f;
    for (int v = threadIdx.x; v < V; v += WG) s += expf(x[v] - bm);
    s = block_sum(s, red);
    if (LS) zs = block_sum(zs, red);
    double lse_w = 0.0, H_w = 0.0;
    if (ENT) {
        double sd = 0.0;
        for (int v = threadIdx.x; v < V; v += WG) sd += (double)expf(x[v] - bm);
        sd = block_sum_wide(sd, dred);
        lse_w = (double)bm + log(sd);
        double hd = 0.0;
        for (int v = threadIdx.x; v < V; v += WG) hd = ent_acc_wide(hd, expf(x[v] - bm), x[v], lse_w);
        H_w = block_sum_wide(hd, dred) / sd;
    }
    const float H = (float)H_w;
    if (threadIdx.x == 0) {
        const float lse = bm + logf(s);
        lse_out[row] = lse;
        if (argmax != nullptr) argmax[row] = best == 0x7fffffff ? 0 : best;      // all-NaN row: keep the index in range
        const float wm = w[row];
        const float xt = wm != 0.f ? x[target[row]] : 0.f;
        const float nll = wm != 0.f ? wm * (lse - xt) : 0.f;
        if (ENT) {
            // (beta == 0: coef is 0 and the helper returns the label-smoothing value -- formed without contraction, as the compiler
            // forms it in the LS instantiation: a packed multiply and two subtractions -- so the monitor mode has that form's bits)
            const float mm = mrow[row];
            const int M = gridDim.x;
            const EntRow r = ent_rows_wide(wm, mm, beta, lse_w, xt, eps, zs, V, H_w);
            if (beta != 0.f) {
                put_wide(row_loss + row, row_lo + row, r.loss);
                if (row_nll != nullptr) put_wide(row_nll + row, row_lo + 2 * M + row, r.nll);
            } else {
                row_loss[row] = ent_row_loss(wm, 0.f, lse, xt, eps, zs, V, H);
                if (row_nll != nullptr) row_nll[row] = nll;
            }
            put_wide(row_ent + row, row_lo + M + row, r.ent);
        } else if (LS) {
            row_loss[row] = eps == 0.f ? nll : wm != 0.f ? wm * (lse - (1.f - eps) * xt - (eps / (float)V) * zs) : 0.f;
            if (row_nll != nullptr) row_nll[row] = nll;
        } else {
            row_loss[row] = nll;
        }
    }
}

__global__ __launch_bounds__(WG) void row_sum_kernel(const float* row_loss, int M, float* loss_sum) {
    __shared__ float red[4];
    float s = 0.f;
    for (int m = threadIdx.x; m < M; m += WG) s += row_loss[m];
    s = block_sum(s, red);
    if (threadIdx.x == 0) loss_sum[0] = s;
}

// The sums of up to three row vectors in one launch (block b sums vector b, a null vector is skipped).  Bit b of `wide` clear: vector b
// is summed as row_sum_kernel does, so with its bits (what beta == 0 owes the label-smoothing entries).  Set: the rows are added in
// fp64 together with their fp32 remainders lo [3, M] (the row kernels' fp64 values: row + remainder), in the same fixed order, and
// the sum is rounded to fp32 once.
__global__ __launch_bounds__(WG) void row_sums_kernel(const float* r0, float* s0, const float* r1, float* s1, const float* r2, float* s2,
                                                      int M, int wide, const float* lo) {
    __shared__ float red[4];
    __shared__ double dred[4];
    const float* r = blockIdx.x == 0 ? r0 : blockIdx.x == 1 ? r1 : r2;
    float* out = blockIdx.x == 0 ? s0 : blockIdx.x == 1 ? s1 : s2;
    if (r == nullptr) return;
    if ((wide >> blockIdx.x) & 1) {
        double d = 0.0;
        const float* l = lo + (size_t)blockIdx.x * M;
        for (int m = threadIdx.x; m < M; m += WG) d += (double)r[m] + (double)l[m];
        d = block_sum_wide(d, dred);
        if (threadIdx.x == 0) out[0] = (float)d;
        return;
    }
    float s = 0.f;
    for (int m = threadIdx.x; m < M; m += WG) s += r[m];
    s = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// d_logits[m, v] = g[0] * w[m] * (softmax(logits[m])[v] - [v == target[m]])
// LS: ... - (1 - eps) [v == target[m]] - eps / V), the gradient of the smoothed row loss (eps == 0: the bits of LS = false)
// ENT: ... + g[0] beta mrow[m] p (z - lse + H) with H = row_ent[m] / mrow[m] (the forward wrote row_ent = mrow H); beta == 0: the LS bits
template <bool LS, bool ENT = false>
__global__ __launch_bounds__(WG) void vocab_nll_bwd_kernel(const float* logits, const float* lse, const int64_t* target,
                                                           const float* w, const float* g, int V, float* d_logits, float eps,
                                                           float beta = 0.f, const float* mrow = nullptr, const float* row_ent = nullptr) {
    static_assert(LS || !ENT, "the entropy form is built on the label-smoothing form");
    const int m = blockIdx.y;
    const int v = blockIdx.x * WG + threadIdx.x;
    if (v >= V) return;
    const float gw = g[0] * w[m];
    const size_t o = (size_t)m * V + v;
    const bool hit = v == (int)target[m];
    if (ENT && beta != 0.f) {
        const float mm = mrow[m];
        const float H = mm != 0.f ? row_ent[m] / mm : 0.f;
        d_logits[o] = ent_pre(gw, (g[0] * beta) * mm, logits[o], lse[m], hit ? ent_hit(eps) : 0.f, ent_all(eps, V), H);
    } else if (LS && eps != 0.f)
        d_logits[o] = gw == 0.f ? 0.f : gw * (expf(logits[o] - lse[m]) - (hit ? 1.f - eps : 0.f) - eps / (float)V);
    else
        d_logits[o] = gw == 0.f ? 0.f : gw * (expf(logits[o] - lse[m]) - (hit ? 1.f : 0.f));
}

// Vocabulary head criterion folded into the GEMM's finishing pass (captioner.py:266, :313, :361 +
// misc/utils.py:132-146, 181-192): the K-slice slabs of the head's tile GEMM are summed (+ bias) into registers, the row's
// log-sum-exp, argmax and weighted NLL are taken there, and what is WRITTEN is not the logits but
//     pre[m, v] = w[m] * (softmax(logits[m])[v] - [v == target[m]])
// -- the gradient of the row's loss term with respect to the logits, which the backward scales by the upstream scalar.  The
// [B*T, V] logits never exist as a tensor in training.  `pre` may alias slab 0 (every thread reads its columns of all slabs
// before it writes).  V <= 256 * NLL_CACHE.
// LS: label smoothing eps in [0, 1) (the target distribution (1 - eps) onehot + eps / V, F.cross_entropy's label_smoothing):
//     row_loss = w (lse - (1 - eps) x[t] - (eps / V) sum_v x[v]),   pre[m, v] = w[m] (softmax[v] - (1 - eps) [v == t] - eps / V),
//     row_nll  = w (lse - x[t])  (the unsmoothed value, for logging; nullable)
// -- every thread adds its columns in ascending order while they are in registers, one more fixed-order block reduction gives the
// row's sum.  eps == 0 takes the LS = false expressions: the same bits.
// ENT (with LS): the entropy regulariser of vocab_nll_fwd_kernel's comment -- once lse is known every thread adds p (lse - z) over its
// register-resident columns in ascending order, one more fixed-order block reduction gives H, and the epilogue applies
// ent_row_loss / ent_pre.  beta == 0 (the monitor mode) takes the LS expressions in a uniform branch and still writes row_ent.
constexpr int NLL_CACHE = 32;
template <bool LS, bool ENT = false>
__global__ __launch_bounds__(WG) void vocab_head_nll_kernel(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                                                            const int64_t* target, const float* w, int V, float* pre, int ld_pre,
                                                            int64_t* argmax, float* row_loss, float eps, float* row_nll,
                                                            float beta = 0.f, const float* mrow = nullptr, float* row_ent = nullptr,
                                                            float* row_lo = nullptr) {
    static_assert(LS || !ENT, "the entropy form is built on the label-smoothing form");
    __shared__ float red[4];
    __shared__ int ired[4];
    __shared__ double dred[4];
    __shared__ float xt_s;
    const int row = blockIdx.x;
    const float* x = parts + (size_t)row * ld;
    const int tgt = (int)target[row];
    float vals[NLL_CACHE];
    float m = -INFINITY;
    int mi = 0x7fffffff;
    float zs = 0.f;
#pragma unroll
    for (int u = 0; u < NLL_CACHE; ++u) {
        const int v = threadIdx.x + u * WG;
        float xv = -INFINITY;
        if (v < V) {
            xv = x[v];
            for (int p = 1; p < nparts; ++p) xv += x[(size_t)p * part_stride + v];
            if (bias != nullptr) xv += bias[v];
            if (xv > m) { m = xv; mi = v; }                   // ascending v per thread: first occurrence wins
            if (v == tgt) xt_s = xv;
            if (LS) zs += xv;
        }
        vals[u] = xv;
    }
    const float bm = block_max(m, red);
    int cand = m == bm ? mi : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) ired[threadIdx.x >> 6] = cand;
    __syncthreads();
    const int best = min(min(ired[0], ired[1]), min(ired[2], ired[3]));
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NLL_CACHE; ++u)
        if (threadIdx.x + u * WG < V) s += expf(vals[u] - bm);
    s = block_sum(s, red);
    const float lse = bm + logf(s);
    const float wm = w[row];
    const bool smooth = LS && eps != 0.f;
    if (LS) zs = block_sum(zs, red);
    const bool ent = ENT && beta != 0.f;
    const float mm = ENT ? mrow[row] : 0.f;
    double lse_w = 0.0, H_w = 0.0;
    if (ENT) {
        // the two fp64 passes read the row's maximum through copies the compiler cannot see through: it then forms the exponentials
        // again in each pass instead of keeping 32 of them live across the reductions (which costs a wave per SIMD)
        float bm_a = bm, bm_b = bm;
        asm volatile("" : "+v"(bm_a), "+v"(bm_b));
        double sd = 0.0;
#pragma unroll
        for (int u = 0; u < NLL_CACHE; ++u) sd += (double)expf(vals[u] - bm_a);       // (a slot past V holds -inf: it adds nothing)
        sd = block_sum_wide(sd, dred);
        lse_w = (double)bm + log(sd);
        double hd = 0.0;
#pragma unroll
        for (int u = 0; u < NLL_CACHE; ++u) hd = ent_acc_wide(hd, expf(vals[u] - bm_b), vals[u], lse_w);
        H_w = block_sum_wide(hd, dred) / sd;
    }
    const float H = (float)H_w;
    if (threadIdx.x == 0) {
        if (argmax != nullptr) argmax[row] = best == 0x7fffffff ? 0 : best;
        const float nll = wm != 0.f ? wm * (lse - xt_s) : 0.f;
        if (ENT) {
            // (beta == 0: the helper returns the label-smoothing value -- formed without contraction, as the compiler forms it in
            // the LS instantiation: a packed multiply and two subtractions -- so the monitor mode has that form's bits)
            const int M = gridDim.x;
            const EntRow r = ent_rows_wide(wm, mm, beta, lse_w, xt_s, eps, zs, V, H_w);
            if (beta != 0.f) {
                put_wide(row_loss + row, row_lo + row, r.loss);
                if (row_nll != nullptr) put_wide(row_nll + row, row_lo + 2 * M + row, r.nll);
            } else {
                row_loss[row] = ent_row_loss(wm, 0.f, lse, xt_s, eps, zs, V, H);
                if (row_nll != nullptr) row_nll[row] = nll;
            }
            put_wide(row_ent + row, row_lo + M + row, r.ent);
        } else if (LS) {
            row_loss[row] = !smooth ? nll : wm != 0.f ? wm * (lse - (1.f - eps) * xt_s - (eps / (float)V) * zs) : 0.f;
            if (row_nll != nullptr) row_nll[row] = nll;
        } else {
            row_loss[row] = nll;
        }
    }
    float* out = pre + (size_t)row * ld_pre;
    const float hit = smooth ? 1.f - eps : 1.f, all = smooth ? eps / (float)V : 0.f;
#pragma unroll
    for (int u = 0; u < NLL_CACHE; ++u) {
        const int v = threadIdx.x + u * WG;
        if (ent) {
            if (v < V) out[v] = ent_pre(wm, beta * mm, vals[u], lse, v == tgt ? ent_hit(eps) : 0.f, ent_all(eps, V), H);
        } else if (!smooth) {
            if (v < V) out[v] = wm == 0.f ? 0.f : wm * (expf(vals[u] - lse) - (v == tgt ? 1.f : 0.f));
        } else {
            if (v < V) out[v] = wm == 0.f ? 0.f : wm * (expf(vals[u] - lse) - (v == tgt ? hit : 0.f) - all);
        }
    }
}

}  // namespace

#ifdef CVC_EXPERIMENTAL
extern "C" const char* cvc_version(void) { return "cvc_hip 0.2 gfx950 +experimental"; }
#else
extern "C" const char* cvc_version(void) { return "cvc_hip 0.2 gfx950"; }
#endif

static int embed_fwd_impl(const float* table, const int64_t* idx, const float* drop, DropSpec rng, int M, int E, float* out,
                          cvc_stream_t stream) {
    if (!table || !idx || !out || M < 1 || E < 4 || (E & 3) || (long long)M * E > 0xffffffffll) return CVC_E_BADARG;
    hipLaunchKernelGGL(embed_relu_fwd_kernel, dim3((E / 4 + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, table, idx,
                       drop, rng, M, E, out);
    return cvc_launch_status();
}

static int embed_bwd_impl(const float* table, const int64_t* idx, const int64_t* order, const float* drop, DropSpec rng,
                          const float* d_out, int M, int E, float* d_table, float* workspace, cvc_stream_t stream) {
    if (!table || !idx || !order || !d_out || !d_table || !workspace || M < 1 || E < 4 || (E & 3)) return CVC_E_BADARG;
    const int gx = (E / 4 + WG - 1) / WG;
    hipLaunchKernelGGL(embed_bwd_pieces_kernel, dim3(gx, (M + EMB_CHUNK - 1) / EMB_CHUNK), dim3(WG), 0, (hipStream_t)stream, idx,
                       order, drop, rng, d_out, M, E, workspace);
    hipLaunchKernelGGL(embed_bwd_runs_kernel, dim3(gx, M), dim3(WG), 0, (hipStream_t)stream, table, idx, order, workspace, M, E,
                       d_table);
    return cvc_launch_status();
}

extern "C" int cvc_embed_relu_fwd(const float* table, const int64_t* idx, const float* drop, int M, int E, float* out,
                                  cvc_stream_t stream) {
    return embed_fwd_impl(table, idx, drop, cvc_drop_spec(nullptr, 0, 0.f), M, E, out, stream);
}

extern "C" int cvc_embed_relu_bwd(const float* table, const int64_t* idx, const int64_t* order, const float* drop,
                                  const float* d_out, int M, int E, float* d_table, float* workspace, cvc_stream_t stream) {
    return embed_bwd_impl(table, idx, order, drop, cvc_drop_spec(nullptr, 0, 0.f), d_out, M, E, d_table, workspace, stream);
}

extern "C" int cvc_embed_relu_rng_fwd(const float* table, const int64_t* idx, const uint32_t* rng_state, unsigned site, float p, int M,
                                      int E, float* out, cvc_stream_t stream) {
    if (!rng_state || p < 0.f || p >= 1.f) return CVC_E_BADARG;
    return embed_fwd_impl(table, idx, nullptr, cvc_drop_spec(rng_state, site, p), M, E, out, stream);
}

extern "C" int cvc_embed_relu_rng_bwd(const float* table, const int64_t* idx, const int64_t* order, const uint32_t* rng_state,
                                      unsigned site, float p, const float* d_out, int M, int E, float* d_table, float* workspace,
                                      cvc_stream_t stream) {
    if (!rng_state || p < 0.f || p >= 1.f) return CVC_E_BADARG;
    return embed_bwd_impl(table, idx, order, nullptr, cvc_drop_spec(rng_state, site, p), d_out, M, E, d_table, workspace, stream);
}

extern "C" int cvc_dropout_rng(const float* x, long long n, const uint32_t* rng_state, unsigned site, float p, float* y,
                               cvc_stream_t stream) {
    if (!x || !y || !rng_state || n < 1 || n > 0xffffffffll || p < 0.f || p >= 1.f || ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
        return CVC_E_BADARG;
    hipLaunchKernelGGL(dropout_rng_kernel, dim3((unsigned)((n / 4 + WG) / WG)), dim3(WG), 0, (hipStream_t)stream, x,
                       cvc_drop_spec(rng_state, site, p), (size_t)n, y);
    return cvc_launch_status();
}

extern "C" int cvc_log_softmax_fwd(const float* logits, int M, int V, float* logp, cvc_stream_t stream) {
    if (!logits || !logp || M < 1 || V < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(log_softmax_kernel, dim3(M), dim3(WG), 0, (hipStream_t)stream, logits, V, logp);
    return cvc_launch_status();
}

extern "C" int cvc_log_softmax_bwd(const float* logp, const float* d_logp, int M, int V, float* d_logits,
                                   cvc_stream_t stream) {
    if (!logp || !d_logp || !d_logits || M < 1 || V < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3(M), dim3(WG), 0, (hipStream_t)stream, logp, d_logp, V, d_logits);
    return cvc_launch_status();
}

extern "C" int cvc_nll_bwd(const int64_t* target, const float* w, const float* g, int M, int V, float* d_logp,
                           cvc_stream_t stream) {
    if (!target || !w || !g || !d_logp || M < 1 || V < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(nll_bwd_kernel, dim3((V + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, target, w, g, V, d_logp);
    return cvc_launch_status();
}

extern "C" int cvc_top2_unk(const float* logits, int M, int V, int unk_idx, int64_t* word, int word_stride,
                            float* logprob, cvc_stream_t stream) {
    if (!logits || !word || M < 1 || V < 1 || word_stride < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(top2_unk_kernel, dim3(M), dim3(WG), 0, (hipStream_t)stream, logits, V, unk_idx, word, word_stride,
                       logprob);
    return cvc_launch_status();
}

extern "C" int cvc_top2_final(const float* part, int nblocks, int M, int unk_idx, int64_t* word, int word_stride,
                              float* logprob, const float* table, int E, float* emb_out, int emb_ld,
                              cvc_stream_t stream) {
    if (!part || !word || nblocks < 1 || M < 1 || M > 64 || word_stride < 1) return CVC_E_BADARG;
    if (emb_out != nullptr && (!table || E < 4 || (E & 3) || (emb_ld & 3) || (emb_ld != 0 && emb_ld < E))) return CVC_E_BADARG;
    hipLaunchKernelGGL(top2_final_kernel, dim3(M), dim3(WG), 0, (hipStream_t)stream, part, nblocks, unk_idx, word, word_stride,
                       logprob, table, E, emb_out, emb_ld);
    return cvc_launch_status();
}

extern "C" int cvc_keys_finalize(const unsigned long long* keys, const unsigned long long* key_unk, const float* ms_part, int nblocks, int T,
                                 int rows, int unk_idx, int64_t* words, float* logprob, cvc_stream_t stream) {
    if (!keys || !key_unk || !ms_part || !words || nblocks < 1 || T < 1 || rows < 1 || rows > KEY_ROWS || unk_idx < 0) return CVC_E_BADARG;
    hipLaunchKernelGGL(keys_finalize_kernel, dim3(T * rows), dim3(WG), 0, (hipStream_t)stream, keys, key_unk, ms_part, nblocks, T, rows,
                       unk_idx, words, logprob);
    return cvc_launch_status();
}

extern "C" int cvc_top2_slab(const cvc_gsk_segs* logits, const float* bias, int V, int M, int unk_idx, int64_t* word,
                             int word_stride, float* logprob, const float* table, int E, float* emb_out, int emb_ld,
                             cvc_stream_t stream) {
    if (!logits || !logits->slab || logits->nchunk < 1 || logits->U < 1 || logits->maxseg < 1 || logits->unit0 < 0 || !word || V < 2 ||
        M < 1 || M > 64 || word_stride < 1)
        return CVC_E_BADARG;
    if (emb_out != nullptr && (!table || E < 4 || (E & 3) || (emb_ld & 3) || (emb_ld != 0 && emb_ld < E))) return CVC_E_BADARG;
    const int nitem = ((V + 31) / 32) * 8;
    hipStream_t st = (hipStream_t)stream;
    if (nitem <= 5 * WG)
        hipLaunchKernelGGL(top2_slab_kernel<5>, dim3(M), dim3(WG), 0, st, *logits, bias, V, unk_idx, word, word_stride, logprob, table, E,
                           emb_out, emb_ld);
    else if (nitem <= 8 * WG)
        hipLaunchKernelGGL(top2_slab_kernel<8>, dim3(M), dim3(WG), 0, st, *logits, bias, V, unk_idx, word, word_stride, logprob, table, E,
                           emb_out, emb_ld);
    else
        return CVC_E_TOOBIG;
    return cvc_launch_status();
}

extern "C" int cvc_nll_fwd(const float* logp, const int64_t* target, const float* w, int M, int V, float* loss_sum,
                           cvc_stream_t stream) {
    if (!logp || !target || !w || !loss_sum || M < 1 || V < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(nll_fwd_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, logp, target, w, M, V, loss_sum);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_nll_fwd(const float* logits, const int64_t* target, const float* w, int M, int V, float* lse,
                                 int64_t* argmax, float* row_loss, float* loss_sum, cvc_stream_t stream) {
    if (!logits || !target || !w || !lse || !row_loss || !loss_sum || M < 1 || V < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(vocab_nll_fwd_kernel<false>, dim3(M), dim3(WG), 0, (hipStream_t)stream, logits, target, w, V, lse, argmax,
                       row_loss, 0.f, (float*)nullptr);
    hipLaunchKernelGGL(row_sum_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, row_loss, M, loss_sum);
    return cvc_launch_status();
}

// eps in [0, 1) and finite (a NaN fails both comparisons' complement)
static bool smoothing_ok(float eps) { return eps >= 0.f && eps < 1.f; }

// cvc_vocab_nll_fwd with label smoothing; row_nll / nll_sum: the unsmoothed rows and their sum (both or neither)
extern "C" int cvc_vocab_nll_ls_fwd(const float* logits, const int64_t* target, const float* w, int M, int V, float eps, float* lse,
                                    int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll, float* nll_sum,
                                    cvc_stream_t stream) {
    if (!logits || !target || !w || !lse || !row_loss || !loss_sum || M < 1 || V < 1 || !smoothing_ok(eps) || !row_nll != !nll_sum)
        return CVC_E_BADARG;
    hipLaunchKernelGGL(vocab_nll_fwd_kernel<true>, dim3(M), dim3(WG), 0, (hipStream_t)stream, logits, target, w, V, lse, argmax,
                       row_loss, eps, row_nll);
    hipLaunchKernelGGL(row_sum_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, row_loss, M, loss_sum);
    if (row_nll) hipLaunchKernelGGL(row_sum_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, row_nll, M, nll_sum);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_head_nll_fwd(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                                      const int64_t* target, const float* w, int M, int V, float* pre, int ld_pre, int64_t* argmax,
                                      float* row_loss, float* loss_sum, cvc_stream_t stream) {
    if (!parts || nparts < 1 || !target || !w || !pre || !row_loss || !loss_sum || M < 1 || V < 1 || V > WG * NLL_CACHE || ld < V ||
        ld_pre < V)
        return CVC_E_BADARG;
    hipLaunchKernelGGL(vocab_head_nll_kernel<false>, dim3(M), dim3(WG), 0, (hipStream_t)stream, parts, nparts, part_stride, ld, bias, target,
                       w, V, pre, ld_pre, argmax, row_loss, 0.f, (float*)nullptr);
    hipLaunchKernelGGL(row_sum_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, row_loss, M, loss_sum);
    return cvc_launch_status();
}

// cvc_vocab_head_nll_fwd with label smoothing; row_nll / nll_sum: the unsmoothed rows and their sum (both or neither)
extern "C" int cvc_vocab_head_nll_ls_fwd(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                                         const int64_t* target, const float* w, int M, int V, float eps, float* pre, int ld_pre,
                                         int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll, float* nll_sum,
                                         cvc_stream_t stream) {
    if (!parts || nparts < 1 || !target || !w || !pre || !row_loss || !loss_sum || M < 1 || V < 1 || V > WG * NLL_CACHE || ld < V ||
        ld_pre < V || !smoothing_ok(eps) || !row_nll != !nll_sum)
        return CVC_E_BADARG;
    hipLaunchKernelGGL(vocab_head_nll_kernel<true>, dim3(M), dim3(WG), 0, (hipStream_t)stream, parts, nparts, part_stride, ld, bias, target,
                       w, V, pre, ld_pre, argmax, row_loss, eps, row_nll);
    hipLaunchKernelGGL(row_sum_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, row_loss, M, loss_sum);
    if (row_nll) hipLaunchKernelGGL(row_sum_kernel, dim3(1), dim3(WG), 0, (hipStream_t)stream, row_nll, M, nll_sum);
    return cvc_launch_status();
}

// The entropy regulariser's entries (include/cvc_hip_blocks.h): the label-smoothing entries with beta, the entropy weight m and
// row_ent / ent_sum; the sums of the row vectors are one launch (row_sums_kernel: ent_sum always, loss_sum and nll_sum with beta != 0
// are accumulated in fp64; with beta == 0 those two have the label-smoothing entries' bits).  beta finite (a NaN or an inf fails the
// comparison)
static bool beta_ok(float beta) { return beta - beta == 0.f; }

extern "C" int cvc_vocab_nll_ent_fwd(const float* logits, const int64_t* target, const float* w, const float* m, int M, int V, float eps,
                                     float beta, float* lse, int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll,
                                     float* nll_sum, float* row_ent, float* ent_sum, float* row_lo, cvc_stream_t stream) {
    if (!logits || !target || !w || !m || !lse || !row_loss || !loss_sum || !row_ent || !ent_sum || !row_lo || M < 1 || V < 1 || !smoothing_ok(eps) ||
        !beta_ok(beta) || !row_nll != !nll_sum)
        return CVC_E_BADARG;
    hipLaunchKernelGGL((vocab_nll_fwd_kernel<true, true>), dim3(M), dim3(WG), 0, (hipStream_t)stream, logits, target, w, V, lse, argmax,
                       row_loss, eps, row_nll, beta, m, row_ent, row_lo);
    hipLaunchKernelGGL(row_sums_kernel, dim3(3), dim3(WG), 0, (hipStream_t)stream, (const float*)row_loss, loss_sum, (const float*)row_ent,
                       ent_sum, (const float*)row_nll, nll_sum, M, beta != 0.f ? 7 : 2, (const float*)row_lo);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_head_nll_ent_fwd(const float* parts, int nparts, long long part_stride, int ld, const float* bias,
                                          const int64_t* target, const float* w, const float* m, int M, int V, float eps, float beta,
                                          float* pre, int ld_pre, int64_t* argmax, float* row_loss, float* loss_sum, float* row_nll,
                                          float* nll_sum, float* row_ent, float* ent_sum, float* row_lo, cvc_stream_t stream) {
    if (!parts || nparts < 1 || !target || !w || !m || !pre || !row_loss || !loss_sum || !row_ent || !ent_sum || !row_lo || M < 1 || V < 1 ||
        V > WG * NLL_CACHE || ld < V || ld_pre < V || !smoothing_ok(eps) || !beta_ok(beta) || !row_nll != !nll_sum)
        return CVC_E_BADARG;
    hipLaunchKernelGGL((vocab_head_nll_kernel<true, true>), dim3(M), dim3(WG), 0, (hipStream_t)stream, parts, nparts, part_stride, ld, bias,
                       target, w, V, pre, ld_pre, argmax, row_loss, eps, row_nll, beta, m, row_ent, row_lo);
    hipLaunchKernelGGL(row_sums_kernel, dim3(3), dim3(WG), 0, (hipStream_t)stream, (const float*)row_loss, loss_sum, (const float*)row_ent,
                       ent_sum, (const float*)row_nll, nll_sum, M, beta != 0.f ? 7 : 2, (const float*)row_lo);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_nll_ent_bwd(const float* logits, const float* lse, const int64_t* target, const float* w, const float* m,
                                     const float* row_ent, const float* g, int M, int V, float eps, float beta, float* d_logits,
                                     cvc_stream_t stream) {
    if (!logits || !lse || !target || !w || !m || !row_ent || !g || !d_logits || M < 1 || V < 1 || !smoothing_ok(eps) || !beta_ok(beta))
        return CVC_E_BADARG;
    hipLaunchKernelGGL((vocab_nll_bwd_kernel<true, true>), dim3((V + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, logits, lse,
                       target, w, g, V, d_logits, eps, beta, m, row_ent);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_nll_bwd(const float* logits, const float* lse, const int64_t* target, const float* w,
                                 const float* g, int M, int V, float* d_logits, cvc_stream_t stream) {
    if (!logits || !lse || !target || !w || !g || !d_logits || M < 1 || V < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(vocab_nll_bwd_kernel<false>, dim3((V + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, logits, lse,
                       target, w, g, V, d_logits, 0.f);
    return cvc_launch_status();
}

extern "C" int cvc_vocab_nll_ls_bwd(const float* logits, const float* lse, const int64_t* target, const float* w,
                                    const float* g, int M, int V, float eps, float* d_logits, cvc_stream_t stream) {
    if (!logits || !lse || !target || !w || !g || !d_logits || M < 1 || V < 1 || !smoothing_ok(eps)) return CVC_E_BADARG;
    hipLaunchKernelGGL(vocab_nll_bwd_kernel<true>, dim3((V + WG - 1) / WG, M), dim3(WG), 0, (hipStream_t)stream, logits, lse,
                       target, w, g, V, d_logits, eps);
    return cvc_launch_status();
}
