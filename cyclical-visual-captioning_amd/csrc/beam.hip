// Beam search on the device: the selection blocks of a step (cvc_beam_select(_parts) and the history, group and forced-word forms
// cvc_beam_select_hist_parts / _groups_parts / _force_parts: a row scan per hypothesis, then a merge per clip), the final ranking
// (cvc_beam_rank, cvc_beam_rank_force), the walk back along the parent pointers (cvc_beam_backtrack(_from)) and the state gather
// (cvc_gather_rows).  The candidates are log_softmax(logit) of model/captioner.py:437 with its UNK rule; the contracts of the blocks:
// include/cvc_hip.h and include/cvc_hip_blocks.h.  Like the other word-selection blocks (csrc/sample.hip, csrc/constrain.hip, csrc/forced.hip) a file of
// its own, so that a change to a beam form rebuilds the beam kernels and nothing else.
//
// Deliberately NOT done here: moving the row scan onto load_logit_row / select_dispatch of csrc/select_row.h.  The scan's general
// form keeps the float4 element layout with scalar loads, so that its log-sum-exp is the fast form's bit for bit
// (tests/test_gpu_tile_path.py pins that); load_logit_row's scalar form holds its elements in another order, and the shared
// dispatch's NG ladder (1, 2, 4, 5, 8) is not the scan's (1 .. 8).  That changes code and needs measurements on the device.
#include "row_block.h"
#include "ban_set.h"
#include "sample_select.h"      // the STOCH forms: gumbel(), the one definition of the noise, and the hash (dropout_rng.h)
#include <math.h>
#include <type_traits>

namespace {

// ------------------------------------------------------------------ beam bookkeeping
// Candidate (k, v) scores: score[k] + logit[k,v] - lse[k]; -inf for v == unk; a finished hypothesis
// only offers (k, 0) at its carried score.  The `beam` best of a clip's beam*V candidates are among the
// per-row top-`beam`, so stage 1 (one workgroup per hypothesis row, values cached in registers) finds
// those and stage 2 (one workgroup per clip) merges beam*beam candidates.  Ties -> lowest flat (k, v).
constexpr int BEAM_MAX = 8;
constexpr int ROW_CACHE = 32;        // values per thread kept in registers: V <= 256 * 32

// Row scan, one workgroup per hypothesis row: thread tid holds elements (tid + 256 g) * 4 .. + 3 of group g in registers, the
// log-sum-exp comes from per-wave (max, sum) pairs, and the `beam` best are found per WAVE without a barrier (shuffles only), then
// merged by wave 0 -- the row's top `beam` are among the 4 x beam wave winners; ties go to the lower index.
// VEC (the fast form, V % 4 == 0 and aligned operands): float4 loads, all requested up front.  NP > 0: the logits are still the NP
// K-slice slabs of the vocabulary GEMM (+ bias), summed on load in the finishing pass's order (slab 0 + slab 1 + ... + bias,
// cvc_tile_linear_finish), so the finished matrix is never written or read back.
// VEC == false (the general form: any V, any alignment, any number of slabs): scalar, bounds-checked loads and a run-time slab loop
// in the same order, then the SAME code -- its log-sum-exp, candidates and scores are the fast form's bit for bit on the same
// values (tests/test_gpu_tile_path.py; history and figures: profiles/tile_path_pins.md).
// HIST (cvc_beam_select_hist_parts): the row is a hypothesis with a history of its own (ca.hist, ca.t) and the rules of constrained
// decoding.  After the row's loads are issued and its (max, sum) share is taken -- the log-sum-exp runs over the full row -- the
// row's ban set is built as the V-bit LDS map of csrc/ban_set.h and every register slot whose column is in the map is set to -inf,
// where the plain form does that for the one UNK slot; ca.nbanned[row] = the map's pop-count.
// FORCE (cvc_beam_select_force_parts, always with HIST; the rule: the comment of beam_merge_kernel's BANKS form): a row may advance
// to the next bank by any of its clip's unmet forced words, and its sorted top-`beam` need not hold them.  After the ban map is
// applied and before the selection rounds overwrite taken values, the thread whose register slot holds column w_j writes that
// value -- raw, post-ban, the bits cand_v would carry -- to ca.fws[4 * row + j] for every active entry j of the clip (-inf for an
// unused entry), and thread 0 writes the word ca.fws[4 * row + 3]: bits 0-2 the row's met mask (the history is already in LDS),
// bits 8-10 the clip's active entries; ca.nmet[row] = the met mask's pop-count.  Nothing else in the scan changes: cand_v, cand_i,
// lse and nbanned are the HIST form's bit for bit.
// STOCH (cvc_beam_select_stoch_parts, always with HIST, never with FORCE; the rule: the comment of beam_merge_kernel's STOCH form): a
// row's top `beam` are taken by the Gumbel-perturbed value s = z * inv_tau + noise instead of z.  After the ban map is applied the
// registers are scaled by inv_tau in place, the candidate-only log-sum-exp lseq (banned slots and padding hold -inf and add nothing)
// is taken from per-wave (max, sum) pairs like the full row's, and the noise of counter row * V + v is added; the selection rounds
// then run on s unchanged.  cand_v carries s; the RAW logit of each of the row's `beam` finalists is reloaded by lane sel of wave 0
// -- `beam` scalars per row, summed in the slab order of the loader (slab 0 + slab 1 + ... + bias), so they are the bits the
// registers held before the scaling, and no second register copy is kept -- and written to ca.raw[8 * row + sel]; ca.lseq[row].
// lse and nbanned are the HIST form's bit for bit.
struct ForceArgs : ConsArgs { const int32_t* force; int nforce; float* fws; int32_t* nmet; };
struct StochScanArgs : ConsArgs { float inv_tau; const uint32_t* state; uint32_t site; float* lseq; float* raw; };
template <bool HIST, bool FORCE, bool STOCH = false> struct scan_args { using type = typename cons_args<HIST>::type; };
template <> struct scan_args<true, true, false> { using type = ForceArgs; };
template <> struct scan_args<true, false, true> { using type = StochScanArgs; };

// The arithmetic of stochastic beam search, compiled with contraction off like the sampler's kernel (csrc/sample_select.h): the
// scaled logit is one rounded multiply, and no product is ever fused into the add or subtract that follows it.
__device__ __forceinline__ float stoch_scale(float z, float inv_tau) {
#pragma clang fp contract(off)
    return z * inv_tau;
}
// phi = logq + (z * inv_tau - lseq): the sampling log-prob of the child
__device__ __forceinline__ float stoch_phi(float logq, float z, float inv_tau, float lseq) {
#pragma clang fp contract(off)
    const float zt = z * inv_tau;
    return logq + (zt - lseq);
}
// the child's key conditioned on its parent's key G and the row's maximum Z >= g: -log(exp(-G) - exp(-Z) + exp(-g)) in the stable
// form of include/cvc_hip_blocks.h; g == Z gives G exactly (l = -inf, u = -inf)
__device__ __forceinline__ float stoch_condition(float G, float Z, float g) {
#pragma clang fp contract(off)
    const float d = g - Z;
    const float l = d > -0.693147180559945f ? logf(-expm1f(d)) : log1pf(-expf(d));
    const float u = (G - g) + l;
    return (G - fmaxf(u, 0.f)) - log1pf(expf(-fabsf(u)));
}

// Forced words of a clip, f[0 .. C): bit j is set iff entry j is active -- 0 < f[j] < V, f[j] != unk and no earlier entry of the
// clip holds the same word.  The one definition the row scan, the merge and the final ranking share.
__device__ __forceinline__ int force_active(const int32_t* f, int C, int V, int unk) {
    int m = 0;
    for (int j = 0; j < C; ++j) {
        const int w = f[j];
        bool ok = w > 0 && w < V && w != unk;
        for (int i = 0; i < j; ++i) ok = ok && f[i] != w;
        m |= ok ? 1 << j : 0;
    }
    return m;
}

template <int NG, int NP = 0, bool VEC = true, bool HIST = false, bool FORCE = false, bool STOCH = false>      // float4 groups per thread: V <= NG * 1024
__global__ __launch_bounds__(WG) void beam_rowtop4_kernel(const float* logits, int nparts, long long part_stride, const float* bias, int beam,
                                                          int V, int unk, float* cand_v, int* cand_i, float* lse_out,
                                                          typename scan_args<HIST, FORCE, STOCH>::type ca) {
    static_assert(HIST || !FORCE, "the FORCE form is a history form");
    static_assert(!STOCH || (HIST && !FORCE), "the STOCH form is a history form without forced words");
    __shared__ float wm[4], ws[4];
    [[maybe_unused]] __shared__ float wqm[4], wqs[4];       // STOCH: the waves' (max, sum) pairs of the candidate-only log-sum-exp
    [[maybe_unused]] __shared__ int wb[4];
    __shared__ float wv[4 * BEAM_MAX];
    __shared__ int wi[4 * BEAM_MAX];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (size_t)row * V;
    f32x4 v4[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int e = (tid + g * WG) * 4;
        if constexpr (!VEC) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = e + j;
                float xv = -INFINITY;
                if (v < V) {
                    xv = x[v];
                    for (int p = 1; p < nparts; ++p) xv += x[(size_t)p * part_stride + v];
                    if (bias != nullptr) xv += bias[v];
                }
                v4[g][j] = xv;
            }
        } else if (e < V) {
            v4[g] = ld4(x + e);
            if constexpr (NP > 0) {
                f32x4 pv[NP];
#pragma unroll
                for (int p = 1; p < NP; ++p) pv[p] = ld4(x + (size_t)p * part_stride + e);
#pragma unroll
                for (int p = 1; p < NP; ++p) v4[g] += pv[p];
                if (bias != nullptr) v4[g] += ld4(bias + e);
            }
        } else v4[g] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    }
    [[maybe_unused]] long long hv = 0;                       // HIST: this thread's step of the history, requested behind the row's loads
    if constexpr (HIST) hv = load_hist_step(ca, row, tid);
    float m = -INFINITY;
#pragma unroll
    for (int g = 0; g < NG; ++g) m = fmaxf(fmaxf(m, fmaxf(v4[g].x, v4[g].y)), fmaxf(v4[g].z, v4[g].w));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += expf(v4[g][e] - m);          // exp(-inf) = 0 for padding
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (m == -INFINITY) s = 0.f;                                      // a wave that holds only padding (-inf - -inf = nan)
    if (lane == 0) { wm[wave] = m; ws[wave] = s; }
    // the beam best of this wave (unk never selected; HIST: no word of the row's ban set)
    if constexpr (HIST) {
        __shared__ uint32_t bits[WG];                       // V <= 32 * WG
        __shared__ long long hist[CONS_T_MAX];
        build_ban_map<WG>(ca, hv, V, unk, tid, bits, hist);     // (both barriers inside)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int v0 = (tid + g * WG) * 4;                  // a group's four columns share one word of the map
            const uint32_t w = v0 < V ? bits[v0 >> 5] >> (v0 & 31) : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v0 + e < V && ((w >> e) & 1u)) v4[g][e] = -INFINITY;
        }
        const int nb = wave_sum_int(__popc(bits[tid]));
        if (lane == 0) wb[wave] = nb;                       // read by thread 0 after the barrier below
        if constexpr (FORCE) {
            const int32_t* f = ca.force + (size_t)(row / beam) * ca.nforce;
            const int act = force_active(f, ca.nforce, V, unk);
            int met = 0;
            for (int j = 0; j < ca.nforce; ++j) {
                if (!((act >> j) & 1)) {
                    if (tid == 0) ca.fws[(size_t)row * 4 + j] = -INFINITY;
                    continue;
                }
                const int w = f[j];                         // 0 < w < V: one register slot of one thread holds it
                float fv = -INFINITY;
                bool own = false;
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool hit = (tid + g * WG) * 4 + e == w;
                        own = own | hit;
                        fv = hit ? v4[g][e] : fv;
                    }
                if (own) ca.fws[(size_t)row * 4 + j] = fv;
                if (wave == 0) met |= __ballot(lane < ca.t && hist[lane] == (long long)w) != 0ull ? 1 << j : 0;
            }
            if (tid == 0) {
                reinterpret_cast<int*>(ca.fws)[(size_t)row * 4 + 3] = (act << 8) | met;
                if (ca.nmet != nullptr) ca.nmet[row] = __popc(met);
            }
        }
        if constexpr (STOCH) {
            const uint32_t seed_lo = ca.state[0], seed_hi = ca.state[1], call = ca.state[2];
            const uint32_t base = (uint32_t)row * (uint32_t)V;
            float mq = -INFINITY;
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v4[g][e] = stoch_scale(v4[g][e], ca.inv_tau);           // -inf (banned, padding) stays -inf
                    mq = fmaxf(mq, v4[g][e]);
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mq = fmaxf(mq, __shfl_xor(mq, o, 64));
            float sq = 0.f;
            if (mq != -INFINITY) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) sq += expf(v4[g][e] - mq);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
            if (lane == 0) { wqm[wave] = mq; wqs[wave] = sq; }
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t v = (uint32_t)((tid + g * WG) * 4 + e);
                    v4[g][e] += gumbel(cvc_drop_hash(seed_lo, seed_hi, call, ca.site, base + v));
                }
        }
    } else {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) v4[g][e] = ((tid + g * WG) * 4 + e == unk) ? -INFINITY : v4[g][e];
    }
    for (int sel = 0; sel < beam; ++sel) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int v = (tid + g * WG) * 4 + e;
                const bool take = (v < V) & better(v4[g][e], v, bv, bi);
                bv = take ? v4[g][e] : bv;
                bi = take ? v : bi;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            const bool take = better(ov, oi, bv, bi);
            bv = take ? ov : bv;
            bi = take ? oi : bi;
        }
        if (lane == 0) { wv[wave * BEAM_MAX + sel] = bv; wi[wave * BEAM_MAX + sel] = bi; }
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) v4[g][e] = ((tid + g * WG) * 4 + e == bi) ? -INFINITY : v4[g][e];   // taken
    }
    __syncthreads();
    if (wave == 0) {
        if (lane == 0) {
            const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
            float S = 0.f;
            for (int w = 0; w < 4; ++w)
                if (wm[w] != -INFINITY) S += ws[w] * expf(wm[w] - M);
            lse_out[row] = M + logf(S);
            if constexpr (HIST) {
                if (ca.nbanned != nullptr) ca.nbanned[row] = (wb[0] + wb[1]) + (wb[2] + wb[3]);
            }
        }
        if constexpr (STOCH) {
            if (lane == 0) {
                const float M = fmaxf(fmaxf(wqm[0], wqm[1]), fmaxf(wqm[2], wqm[3]));
                float S = 0.f;
                for (int w = 0; w < 4; ++w)
                    if (wqm[w] != -INFINITY) S += wqs[w] * expf(wqm[w] - M);
                ca.lseq[row] = M + logf(S);                    // no candidate: -inf + log 0 = -inf
            }
        }
        [[maybe_unused]] int my_i = 0x7fffffff;                // STOCH: lane sel keeps the row's sel-th finalist
        const int cw = lane / BEAM_MAX, cs = lane % BEAM_MAX;      // lane -> (wave, rank) candidate
        float cv = -INFINITY;
        int ci = 0x7fffffff;
        if (cw < 4 && cs < beam) { cv = wv[cw * BEAM_MAX + cs]; ci = wi[cw * BEAM_MAX + cs]; }
        for (int sel = 0; sel < beam; ++sel) {
            float bv = cv;
            int bi = ci;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                const bool take = better(ov, oi, bv, bi);
                bv = take ? ov : bv;
                bi = take ? oi : bi;
            }
            if (lane == 0) { cand_v[row * BEAM_MAX + sel] = bv; cand_i[row * BEAM_MAX + sel] = bi; }
            if constexpr (STOCH) my_i = lane == sel ? bi : my_i;
            if (ci == bi) { cv = -INFINITY; ci = 0x7fffffff; }
        }
        if constexpr (STOCH) {
            if (lane < beam) {
                float xv = -INFINITY;
                if (my_i >= 0 && my_i < V) {                   // the loader's sum, in its order
                    xv = x[my_i];
                    for (int p = 1; p < nparts; ++p) xv += x[(size_t)p * part_stride + my_i];
                    if (bias != nullptr) xv += bias[my_i];
                }
                ca.raw[row * BEAM_MAX + lane] = xv;
            }
        }
    }
}

// HIST: the hypotheses carry their histories (element (s, r) at hist[s * stride + r]).  After the selection every lane knows the
// parent and the word of each selected slot (the butterfly leaves the winner in all lanes); lane s copies step s < t of the parent's
// history for each of the `beam` selections -- all loads first, then the stores -- and lane 0 appends the word at step t.  The copy
// gathers across the clip's rows: hist_in and hist_out are distinct buffers.
struct NoHist {};
struct HistArgs { const int64_t* in; int64_t* out; long long stride; int t; };
template <bool HIST> struct hist_args { using type = NoHist; };
template <> struct hist_args<true> { using type = HistArgs; };

// GROUPS (cvc_beam_select_groups_parts, always with HIST): diverse beam search, beam = G * bd, slot k of a clip in group g = k / bd.
// The rule, once (restated by include/cvc_hip_blocks.h and in fp64 by tests/beam_groups_ref.py):
//   base      c(k, v) = score[k] + z[k, v] - lse[k], exactly the HIST form's candidate (full-row log-sum-exp, -inf in the row's ban
//             set, a frozen row offers only (k, 0) at its carried score); step 0: only the first slot of each group (k % bd == 0) is
//             live, the others are at -inf.
//   penalty   groups are served in order g = 0 .. G-1 within the step; pen(v) = the number of slots selected at this step by groups
//             < g whose parent row was live (not frozen) and whose word is v (Hamming diversity);
//             aug(k, v) = c(k, v) - lambda * (float)pen(v) in fp32: one rounded multiply, then one rounded subtract (group_aug()
//             below, compiled with contraction off: never an fma).  A frozen row's candidate is not penalised and its selection does
//             not count toward pen, nor does a filler (a slot selected at -inf: it is no hypothesis and its word is arbitrary); -inf stays -inf.
//   selection group g takes the bd best of its bd * V candidates by aug, ties -> lowest flat (k, v) with k the clip-wide slot; the
//             j-th best goes to slot g * bd + j.  score_out is the UNAUGMENTED c; done_out, nbanned and the history gather as in
//             the HIST form.  The parent of every selected slot lies in its own group; fewer finite candidates than bd: fillers at
//             -inf with the parent in the group and the word in range; every candidate NaN: the group's first slot, word 0.
// The row scan (stage 1) does not change: group g penalises at most g * bd <= beam - bd distinct words, and a penalty only lowers
// a value, so at least bd of a row's unpenalised top-`beam` stay unpenalised; each of those is >= everything outside that set under
// the same tie rule, hence the penalised top-bd of a row lies inside the `beam` candidates the row scan already writes.
// Still one wave per clip, one candidate per lane: the G * bd selection rounds are the `beam` butterfly rounds, with the lanes of
// the other groups offering nothing.  Lane 0 keeps (parent live and value finite ? word : -1) of every selected slot in LDS next to
// sel_k / sel_v; at the start of a group each of its lanes counts the entries equal to its candidate's word.  The winner's own lane
// (flat indices are unique) writes score_out from its unaugmented value.  No atomics, no scratch.
// c - lambda * pen with the product rounded on its own.  hipcc's default for device code is -ffp-contract=fast and HIP's __fmul_rn /
// __fsub_rn are plain operators that contract like any other (csrc/label_glue.hip), so contraction is switched off for this function;
// the instructions carry no contract flag and stay a v_mul_f32 and a v_sub_f32 after inlining (checked in the disassembly).
__device__ __forceinline__ float group_aug(float c, float lambda, int pen) {
#pragma clang fp contract(off)
    const float p = lambda * (float)pen;
    return c - p;
}

struct NoGroups {};
struct GroupArgs { int groups; float lambda; };

// BANKS (cvc_beam_select_force_parts, always with HIST, never with GROUPS): lexically constrained beam search (Anderson et al. 2017;
// the bank formulation of Post & Vilar 2018).  The rule, once (restated by include/cvc_hip_blocks.h and in fp64 by tests/force_ref.py):
//   forced    force[b * C + j], j < C = nforce in {1, 2, 3}, int32.  Entry j of clip b is ACTIVE iff 0 < w < V, w != unk and no
//             entry j' < j of the clip holds the same w (force_active()); anything else is unused.
//   banks     beam = (C + 1) * bd; slots [j * bd, (j + 1) * bd) of a clip are bank j.  For row r = (b, k) entering step t with history
//             y_0 .. y_{t-1}: met(r) = the active entries of clip b whose word occurs in the history, n(r) = |met(r)|.  Routing uses
//             n(r) from the history, never the slot.
//   base      c(k, v) = score[k] + z[k, v] - lse[k], exactly the HIST form's candidate (full-row log-sum-exp, -inf in the row's ban
//             set -- a forced word in it is -inf for this step like any banned word -- and a frozen row offers only (k, 0) at its
//             carried score); step 0: only slot 0 of a clip is live.
//   target    the bank of (k, v) is n(r) + 1 if r is live and v is an active forced word of the clip that is not in met(r), else n(r).
//   selection bank j takes the bd best candidates whose target is j over ALL rows of the clip, ties -> lowest flat (k, v) with k the
//             clip-wide slot; the i-th best goes to slot j * bd + i.  Fewer than bd finite candidates: the rest of the bank are
//             fillers -- score_out = -inf, parent in [0, beam), word in [0, V), done_out / the history gather / the append as for
//             any slot; what a filler holds besides its -inf score is not part of the rule.  A row at -inf offers only -inf.
//   outputs   score_out = c (scores stay sums of the model's log-probs); parent, word, done_out, the histories and nbanned as in the
//             HIST form.  No implicit end-of-sentence rule: a hypothesis may end in any bank.
//   invariant every slot with a finite score in bank j has exactly j active forced words in its history.
// Why the row scan's sorted top-`beam` is still enough: a live row has at most C unmet forced words, so the bd best candidates that
// STAY in the row's bank lie among the first bd + C entries of the list the row scan already writes (bd + C <= beam); the candidates
// that ADVANCE are at most C per row, the row's values at its unmet forced words, which the top list need not hold -- the FORCE form
// of the row scan reports them.  Per clip the merge sees at most beam * (bd + 2 C) candidates: 64 at beam 8, C = 3, fewer for every
// other allowed (beam, C).  Still one wave per clip and one candidate per lane: lane -> (k = lane / (bd + 2 C), r = lane % (bd + 2 C)),
// r < bd + C the r-th list entry, the others the advance lane of entry r - (bd + C).  A list entry that is an unmet forced word offers
// nothing from its list lane -- the advance lane carries it -- so flat indices stay unique.  The C + 1 banks are served in turn over
// the `beam` butterfly rounds, the lanes whose target is not the served bank offering (-inf, no index), as GROUPS masks; the winner's
// own lane writes score_out.  No scratch, nothing but shuffles and the sel_k / sel_v words of LDS.
struct BankArgs { const int32_t* force; int nforce; const float* fws; int unk; };
template <bool GROUPS, bool BANKS = false> struct group_args { using type = NoGroups; };
template <> struct group_args<true, false> { using type = GroupArgs; };
template <> struct group_args<false, true> { using type = BankArgs; };

// STOCH (cvc_beam_select_stoch_parts, always with HIST, never with GROUPS or BANKS): stochastic beam search (Kool, van Hoof and
// Welling 2019).  The rule, once (restated by include/cvc_hip_blocks.h and in fp64 by tests/sbs_ref.py):
//   state     row r = (b, k) enters step t with its history, score_in[r] (the sum of the model's log-probs), logq_in[r] (its sampling
//             log-prob) and G_in[r] (its perturbed key); t == 0: only slot 0 of a clip is live, the others are at G = -inf.
//   live row  candidates = the words outside Ban(t, r); lseq[r] = log-sum-exp of z * inv_tau over the candidates ONLY, so that
//             q(v | r) = exp(z * inv_tau - lseq) is the distribution the sampling engine draws from, renormalised over what may be
//             chosen; phi(k, v) = logq_in[k] + (z * inv_tau - lseq[k]); g(k, v) = phi(k, v) + gumbel(hash(seed_lo, seed_hi, call,
//             CVC_SBS_SITE + t, (r * V + v) mod 2^32)); Z[k] = max_v g(k, v); the key is g conditioned on the parent's,
//             gt = -log(exp(-G_in[k]) - exp(-Z[k]) + exp(-g)), in the stable form of stoch_condition(): the arg-max child gets G_in[k].
//   others    a frozen row offers only (k, 0) at gt = G_in[k], logq and score carried; a row at G = -inf or with every word banned
//             offers only -inf.
//   selection the `beam` largest gt of the clip, ties -> lowest flat (k, v); the i-th goes to slot i (draw order); fillers as HIST.
//   outputs   score_out = score_in[k] + (z - lse[k]) on the RAW logit (the HIST form's expression and bits), logq_out = phi,
//             G_out = gt, -inf all three for a filler; parent, word, done_out, the histories as in the HIST form.
// gt increases with g, and g = s + const per row up to rounding, so the row scan's top `beam` by s = z * inv_tau + noise hold the row's
// top `beam` by gt; only these beam * beam finalists are transformed, here: phi and g are recomputed from the raw logit the scan
// reloaded (the noise from the same counter) and Z[k] is the maximum over the row's finalists, so g - Z <= 0 holds in fp32 as well.
// The winner's own lane writes score_out, logq_out and G_out, as GROUPS and BANKS write score_out.
struct NoStoch {};
struct StochArgs { float inv_tau; const uint32_t* state; uint32_t site; const float* lseq; const float* raw; const float* logq_in;
                   const float* G_in; float* logq_out; float* G_out; };
template <bool STOCH> struct stoch_args { using type = NoStoch; };
template <> struct stoch_args<true> { using type = StochArgs; };

template <bool HIST = false, bool GROUPS = false, bool BANKS = false, bool STOCH = false>
__global__ __launch_bounds__(64) void beam_merge_kernel(const float* cand_v, const int* cand_i, const float* lse,
                                                        const float* score_in, const uint8_t* done_in, int beam, int V,
                                                        int first_step, int64_t* parent, int64_t* word, float* score_out,
                                                        uint8_t* done_out, typename hist_args<HIST>::type ha,
                                                        typename group_args<GROUPS, BANKS>::type ga,
                                                        typename stoch_args<STOCH>::type sa) {
    static_assert(HIST || !(GROUPS || BANKS), "the GROUPS and BANKS forms are history forms");
    static_assert(!(GROUPS && BANKS), "groups and banks exclude each other");
    static_assert(!STOCH || (HIST && !GROUPS && !BANKS), "the STOCH form is a history form without groups or banks");
    const int b = blockIdx.x, lane = threadIdx.x;
    [[maybe_unused]] __shared__ int sel_k[BEAM_MAX], sel_v[BEAM_MAX];      // HIST: parent and word of every selected slot
    [[maybe_unused]] __shared__ int sel_p[BEAM_MAX];                       // GROUPS: its word if the parent was live, else -1
    // lane -> candidate (k = lane / beam, r = lane % beam), beam*beam <= 64; BANKS: (bd + 2 C) lanes per row, see above
    int k = lane / beam, r = lane - k * beam;
    float cv = -INFINITY;
    int flat = 0x7fffffff;
    [[maybe_unused]] int bd = beam, pw = -2;             // GROUPS: slots per group; this lane's word if it can be penalised
    [[maybe_unused]] int tb = 0, adv = -1;               // BANKS: the candidate's target bank; the entry of an advance lane
    // STOCH: the row's key, the candidate's unconditioned g (-inf: it offers nothing), and what its lane writes if it wins
    [[maybe_unused]] float c_G = -INFINITY, c_g = -INFINITY, c_sc = -INFINITY, c_lq = -INFINITY;
    if constexpr (GROUPS) bd = beam / ga.groups;
    if constexpr (BANKS) {
        bd = beam / (ga.nforce + 1);
        const int per = bd + 2 * ga.nforce;
        k = lane / per;
        r = lane - k * per;
        adv = r - (bd + ga.nforce);
    }
    if (k < beam) {
        const int row = b * beam + k;
        float sc = score_in[row];
        if (first_step && (GROUPS ? k % bd != 0 : k > 0)) sc = -INFINITY;
        [[maybe_unused]] int unmet = 0;                  // BANKS: the clip's active entries the row's history does not hold
        if constexpr (BANKS) {
            const int fm = reinterpret_cast<const int*>(ga.fws)[(size_t)row * 4 + 3];
            tb = __popc(fm & 7);
            unmet = (fm >> 8) & ~fm & 7;
        }
        if constexpr (STOCH) {
            float G = sa.G_in[row];
            if (first_step && k > 0) G = -INFINITY;
            c_G = G;
            c_sc = sc;
            c_lq = sa.logq_in[row];
            if (done_in[row]) {                          // frozen: (k, 0) at the carried key, logq and score carried
                cv = r == 0 ? G : -INFINITY;
                flat = k * V + r;
            } else {
                const float s = cand_v[row * BEAM_MAX + r];
                const int vi = cand_i[row * BEAM_MAX + r];
                flat = vi == 0x7fffffff ? 0x7fffffff : k * V + vi;
                if (s != -INFINITY && G != -INFINITY && vi != 0x7fffffff) {
                    const float zr = sa.raw[row * BEAM_MAX + r];
                    const float phi = stoch_phi(c_lq, zr, sa.inv_tau, sa.lseq[row]);
                    c_g = phi + gumbel(cvc_drop_hash(sa.state[0], sa.state[1], sa.state[2], sa.site, (uint32_t)row * (uint32_t)V + (uint32_t)vi));
                    c_sc = sc + (zr - lse[row]);
                    c_lq = phi;
                }
            }
        } else if (done_in[row]) {
            // frozen hypothesis: candidates (k, 0) at the carried score, every other (k, v) at -inf; keep the
            // -inf fillers at distinct low flat indices so that tie-breaking matches a full scan
            cv = r == 0 ? sc : -INFINITY;
            flat = adv >= 0 ? 0x7fffffff : k * V + r;
        } else if (adv < 0) {
            const float v = cand_v[row * BEAM_MAX + r];
            const int vi = cand_i[row * BEAM_MAX + r];
            cv = (v == -INFINITY || sc == -INFINITY) ? -INFINITY : sc + (v - lse[row]);
            flat = vi == 0x7fffffff ? 0x7fffffff : k * V + vi;
            if constexpr (GROUPS) pw = vi == 0x7fffffff ? -2 : vi;
            if constexpr (BANKS) {
                for (int j = 0; j < ga.nforce; ++j)
                    if (((unmet >> j) & 1) && ga.force[(size_t)b * ga.nforce + j] == vi) { cv = -INFINITY; flat = 0x7fffffff; }
            }
        } else if constexpr (BANKS) {
            if ((unmet >> adv) & 1) {
                const float v = ga.fws[(size_t)row * 4 + adv];
                cv = (v == -INFINITY || sc == -INFINITY) ? -INFINITY : sc + (v - lse[row]);
                flat = k * V + ga.force[(size_t)b * ga.nforce + adv];
                tb += 1;
            }
        }
    }
    if constexpr (STOCH) {                               // Z[k] over the row's finalists (every lane shuffles), then the conditioned key
        float Z = -INFINITY;
        const int l0 = (k < beam ? k : beam - 1) * beam;
        for (int j = 0; j < beam; ++j) Z = fmaxf(Z, __shfl(c_g, l0 + j, 64));
        if (c_g != -INFINITY) cv = stoch_condition(c_G, Z, c_g);
        if (cv == -INFINITY) { c_sc = -INFINITY; c_lq = -INFINITY; }      // a filler
    }
    [[maybe_unused]] float aug = -INFINITY;              // GROUPS: the candidate's augmented value while its group is served
    [[maybe_unused]] int g0 = 0;                         // GROUPS: first slot of the group being served
    for (int sel = 0; sel < beam; ++sel) {
        float bv = cv;
        int bi = flat;
        if constexpr (GROUPS) {
            if (sel == g0 + bd) g0 = sel;
            const bool mine = k >= g0 && k < g0 + bd;
            if (sel == g0) {                             // a new group: the penalties of the words the groups before it took
                __syncthreads();
                int pen = 0;
                for (int s = 0; s < g0; ++s) pen += sel_p[s] == pw ? 1 : 0;
                aug = mine ? group_aug(cv, ga.lambda, pen) : -INFINITY;
            }
            bv = aug;
            bi = mine ? flat : 0x7fffffff;
        }
        if constexpr (BANKS) {
            const bool mine = tb == sel / bd;
            bv = mine ? cv : -INFINITY;
            bi = mine ? flat : 0x7fffffff;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) {
            int kk = bi / V, vv = bi - kk * V;
            if (bi == 0x7fffffff) { kk = GROUPS ? g0 : 0; vv = 0; }      // every candidate NaN: parent / word feed gathers, keep them in range
            parent[b * beam + sel] = kk;
            word[b * beam + sel] = vv;
            if (!(GROUPS || BANKS || STOCH) || bi == 0x7fffffff) score_out[b * beam + sel] = STOCH ? -INFINITY : bv;
            if constexpr (STOCH) {
                if (bi == 0x7fffffff) { sa.logq_out[b * beam + sel] = -INFINITY; sa.G_out[b * beam + sel] = -INFINITY; }
            }
            const bool frozen = done_in[b * beam + kk] != 0;
            done_out[b * beam + sel] = (frozen || vv == 0) ? 1 : 0;
            if constexpr (GROUPS) sel_p[sel] = (frozen || bi == 0x7fffffff || bv == -INFINITY) ? -1 : vv;
        }
        if constexpr (GROUPS) {
            if (flat == bi && bi != 0x7fffffff) { score_out[b * beam + sel] = cv; aug = -INFINITY; }      // the winner's lane
        }
        if constexpr (BANKS) {
            if (flat == bi && bi != 0x7fffffff) score_out[b * beam + sel] = cv;                           // the winner's lane
        }
        if constexpr (STOCH) {
            if (flat == bi && bi != 0x7fffffff) {                                                         // the winner's lane
                score_out[b * beam + sel] = c_sc;
                sa.logq_out[b * beam + sel] = c_lq;
                sa.G_out[b * beam + sel] = cv;
            }
        }
        if constexpr (HIST) {
            if (lane == 0) {
                const bool none = bi == 0x7fffffff;
                sel_k[sel] = none ? (GROUPS ? g0 : 0) : bi / V;
                sel_v[sel] = none ? 0 : bi - (bi / V) * V;
            }
        }
        if (flat == bi) { cv = -INFINITY; flat = 0x7fffffff; }      // taken (flat indices are unique)
    }
    if constexpr (HIST) {
        __syncthreads();
        int64_t h[BEAM_MAX];
        const bool mine = lane < ha.t;
#pragma unroll
        for (int sel = 0; sel < BEAM_MAX; ++sel)
            if (sel < beam && mine) h[sel] = ha.in[(size_t)lane * ha.stride + b * beam + sel_k[sel]];
#pragma unroll
        for (int sel = 0; sel < BEAM_MAX; ++sel) {
            if (sel < beam && mine) ha.out[(size_t)lane * ha.stride + b * beam + sel] = h[sel];
            if (sel < beam && lane == 0) ha.out[(size_t)ha.t * ha.stride + b * beam + sel] = sel_v[sel];
        }
    }
}

__global__ __launch_bounds__(WG) void gather_rows_kernel(const float* src, const int64_t* parent, int beam, int width,
                                                         float* dst) {
    const int r = blockIdx.y;
    const int c = (blockIdx.x * WG + threadIdx.x) * 4;
    if (c >= width) return;
    const size_t s = (size_t)((r / beam) * beam + (int)parent[r]) * width + c;
    st4(dst + (size_t)r * width + c, ld4(src + s));
}

}  // namespace

// the argument checks of the beam selection blocks
static int beam_select_check(const float* logits, int nparts, const float* score_in, const uint8_t* done_in, int B, int beam, int V,
                             const int64_t* parent, const int64_t* word, const float* score_out, const uint8_t* done_out,
                             const float* workspace) {
    if (nparts < 1) return CVC_E_BADARG;
    if (!logits || !score_in || !done_in || !parent || !word || !score_out || !done_out || !workspace) return CVC_E_BADARG;
    if (B < 1 || beam < 1 || beam > BEAM_MAX || V < beam + 1 || V > WG * ROW_CACHE) return CVC_E_BADARG;
    return 0;
}

// behind the entry points, after the checks: the loader form of the row scan, then the merge.  HIST: the forms of both kernels that
// know the hypotheses' histories (ra: the row scan's history and rules, ma: the merge's gather).  GROUPS: the HIST row scan and the
// merge that serves the groups in turn (ga: their number and the diversity strength).
// BANKS: the FORCE row scan and the merge that serves the banks in turn (ra, ga: the forced words and the rows' workspace slots).
// STOCH: the STOCH row scan and merge (ra, sa: the temperature, the generator state and the rows' workspace slots).
template <bool HIST, bool GROUPS = false, bool BANKS = false, bool STOCH = false>
static int beam_select_run(const float* logits, int nparts, long long part_stride, const float* bias, const float* score_in,
                           const uint8_t* done_in, int B, int beam, int V, int unk_idx, int first_step, int64_t* parent, int64_t* word,
                           float* score_out, uint8_t* done_out, float* workspace, cvc_stream_t stream,
                           typename scan_args<HIST, BANKS, STOCH>::type ra, typename hist_args<HIST>::type ma,
                           typename group_args<GROUPS, BANKS>::type ga = {}, typename stoch_args<STOCH>::type sa = {}) {
    // workspace: [rows*8] candidate values, [rows*8] candidate indices, [rows] lse   (rows = B*beam)
    const int rows = B * beam;
    float* cand_v = workspace;
    int* cand_i = reinterpret_cast<int*>(workspace + (size_t)rows * BEAM_MAX);
    float* lse = workspace + (size_t)rows * BEAM_MAX * 2;
    const bool aligned = (V & 3) == 0 && ((uintptr_t)logits & 15) == 0 && 4 * BEAM_MAX <= 64;
    const bool slabs = aligned && (nparts == 2 || nparts == 4 || nparts == 6 || nparts == 8) && (part_stride & 3) == 0 &&
                       ((uintptr_t)bias & 15) == 0;
    // (a ONE-workgroup-per-clip form -- 2 * beam waves scanning the clip's rows, both merges in LDS, no second launch -- was built
    // and measured in round 6: bit-identical, but 36 us against 25 us for the two launches below at 64 clips x beam 5, V = 5000,
    // 6 slabs: 64 workgroups pulling 600 KB each ingest at ~20 GB/s per compute unit; 320 row workgroups spread the same bytes
    // over the chip)
    const bool fast = (aligned && nparts == 1 && bias == nullptr) || slabs;
    // the loader form of the row scan: NG float4 groups per thread by V; the fast form with its slabs unrolled (NP = their number) or
    // one finished matrix (NP = 0); the general form with a run-time slab loop (NP = 0)
    using std::integral_constant;
    auto scan = [&](auto ng_, auto np_, auto vec_) {
        constexpr int NG = decltype(ng_)::value, NP = decltype(np_)::value;
        constexpr bool VEC = decltype(vec_)::value;
        hipLaunchKernelGGL((beam_rowtop4_kernel<NG, NP, VEC, HIST, BANKS, STOCH>), dim3(rows), dim3(WG), 0, (hipStream_t)stream, logits, nparts,
                           part_stride, bias, beam, V, unk_idx, cand_v, cand_i, lse, ra);
    };
    auto groups = [&](auto ng_) {
        if (!fast) return scan(ng_, integral_constant<int, 0>{}, std::false_type{});
        switch (slabs ? nparts : 0) {
            case 2: scan(ng_, integral_constant<int, 2>{}, std::true_type{}); break;
            case 4: scan(ng_, integral_constant<int, 4>{}, std::true_type{}); break;
            case 6: scan(ng_, integral_constant<int, 6>{}, std::true_type{}); break;
            case 8: scan(ng_, integral_constant<int, 8>{}, std::true_type{}); break;
            default: scan(ng_, integral_constant<int, 0>{}, std::true_type{}); break;
        }
    };
    switch ((V + 4 * WG - 1) / (4 * WG)) {
        case 1: groups(integral_constant<int, 1>{}); break;
        case 2: groups(integral_constant<int, 2>{}); break;
        case 3: groups(integral_constant<int, 3>{}); break;
        case 4: groups(integral_constant<int, 4>{}); break;
        case 5: groups(integral_constant<int, 5>{}); break;
        case 6: groups(integral_constant<int, 6>{}); break;
        case 7: groups(integral_constant<int, 7>{}); break;
        default: groups(integral_constant<int, 8>{}); break;
    }
    hipLaunchKernelGGL((beam_merge_kernel<HIST, GROUPS, BANKS, STOCH>), dim3(B), dim3(64), 0, (hipStream_t)stream, cand_v, cand_i, lse, score_in,
                       done_in, beam, V, first_step, parent, word, score_out, done_out, ma, ga, sa);
    return cvc_launch_status();
}

extern "C" int cvc_beam_select_parts(const float* logits, int nparts, long long part_stride, const float* bias,
                                     const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx,
                                     int first_step, int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out,
                                     float* workspace, cvc_stream_t stream) {
    const int rc = beam_select_check(logits, nparts, score_in, done_in, B, beam, V, parent, word, score_out, done_out, workspace);
    if (rc != 0) return rc;
    return beam_select_run<false>(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, first_step, parent, word,
                                  score_out, done_out, workspace, stream, NoCons{}, NoHist{});
}

extern "C" int cvc_beam_select(const float* logits, const float* score_in, const uint8_t* done_in, int B, int beam, int V,
                               int unk_idx, int first_step, int64_t* parent, int64_t* word, float* score_out,
                               uint8_t* done_out, float* workspace, cvc_stream_t stream) {
    return cvc_beam_select_parts(logits, 1, 0, nullptr, score_in, done_in, B, beam, V, unk_idx, first_step, parent, word, score_out,
                                 done_out, workspace, stream);
}

// Constrained beam search: cvc_beam_select_parts for hypotheses that carry their own histories (contract: include/cvc_hip_blocks.h).
// The HIST forms of the two kernels above; first_step is t == 0; c == NULL: no rule but UNK.
// groups == 0: the history block; groups >= 1 (cvc_beam_select_groups_parts): the GROUPS merge, groups == 1 included -- it is
// the history block bit for bit (nothing is ever penalised) and the tests pin that on the form that serves the groups.
// nforce >= 1 (cvc_beam_select_force_parts): the FORCE row scan and the BANKS merge.
static int beam_select_hist(const float* logits, int nparts, long long part_stride, const float* bias,
                            const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                            const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                            int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out, int32_t* nbanned,
                            float* workspace, cvc_stream_t stream, int groups, float lambda, const int32_t* force = nullptr,
                            int nforce = 0, int32_t* nmet = nullptr) {
    const int rc = beam_select_check(logits, nparts, score_in, done_in, B, beam, V, parent, word, score_out, done_out, workspace);
    if (rc != 0) return rc;
    if (t < 0 || t > CONS_T_MAX) return CVC_E_TOOBIG;
    if (c != nullptr && cons_rules_check(c) != 0) return CVC_E_BADARG;
    if (!hist_out || (t > 0 && !hist_in) || (const int64_t*)hist_out == hist_in || hist_stride < (long long)B * beam) return CVC_E_BADARG;
    const cvc_constraint none = {0, 0, 0, 0, nullptr, nullptr, 0};
    if (c == nullptr) c = &none;
    const ConsArgs ra{hist_in, hist_stride, t, c->no_repeat_ngram, c->no_immediate_repeat != 0, c->min_len, c->ban, c->nban,
                      c->bad_end, c->nbad, nbanned};
    const HistArgs ma{hist_in, hist_out, hist_stride, t};
    if (nforce > 0) {              // the rows' forced-word slots lie behind the history block's 17 floats per row
        float* fws = workspace + (size_t)17 * B * beam;
        return beam_select_run<true, false, true>(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, t == 0 ? 1 : 0,
                                                  parent, word, score_out, done_out, workspace, stream,
                                                  ForceArgs{ra, force, nforce, fws, nmet}, ma, BankArgs{force, nforce, fws, unk_idx});
    }
    if (groups == 0)
        return beam_select_run<true>(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, t == 0 ? 1 : 0, parent,
                                     word, score_out, done_out, workspace, stream, ra, ma);
    return beam_select_run<true, true>(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, t == 0 ? 1 : 0, parent,
                                       word, score_out, done_out, workspace, stream, ra, ma, GroupArgs{groups, lambda});
}

extern "C" int cvc_beam_select_hist_parts(const float* logits, int nparts, long long part_stride, const float* bias,
                                          const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                                          const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                                          int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out, int32_t* nbanned,
                                          float* workspace, cvc_stream_t stream) {
    return beam_select_hist(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, t, hist_in, hist_out, hist_stride, c,
                            parent, word, score_out, done_out, nbanned, workspace, stream, 0, 0.f);
}

// Diverse (group) beam search: cvc_beam_select_hist_parts with the clip's slots in `groups` groups served in turn and a Hamming
// diversity penalty of strength lambda between them (the rule: the comment of beam_merge_kernel's GROUPS form; contract:
// include/cvc_hip_blocks.h).
extern "C" int cvc_beam_select_groups_parts(const float* logits, int nparts, long long part_stride, const float* bias,
                                            const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                                            const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                                            int groups, float lambda, int64_t* parent, int64_t* word, float* score_out,
                                            uint8_t* done_out, int32_t* nbanned, float* workspace, cvc_stream_t stream) {
    if (groups < 1 || (beam >= 1 && beam % groups != 0) || !(lambda >= 0.f) || isinf(lambda)) return CVC_E_BADARG;
    return beam_select_hist(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, t, hist_in, hist_out, hist_stride, c,
                            parent, word, score_out, done_out, nbanned, workspace, stream, groups, lambda);
}

// Lexically constrained beam search: cvc_beam_select_hist_parts with `nforce` forced words per clip and the clip's slots in
// nforce + 1 banks by the number of forced words met (the rule: the comment of beam_merge_kernel's BANKS form; contract:
// include/cvc_hip_blocks.h).  workspace: 21 * B * beam floats.
extern "C" int cvc_beam_select_force_parts(const float* logits, int nparts, long long part_stride, const float* bias,
                                           const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                                           const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                                           const int32_t* force, int nforce, int64_t* parent, int64_t* word, float* score_out,
                                           uint8_t* done_out, int32_t* nbanned, int32_t* nmet, float* workspace, cvc_stream_t stream) {
    if (!force || nforce < 1 || nforce > 3 || (beam >= 1 && beam % (nforce + 1) != 0)) return CVC_E_BADARG;
    return beam_select_hist(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, t, hist_in, hist_out, hist_stride, c,
                            parent, word, score_out, done_out, nbanned, workspace, stream, 0, 0.f, force, nforce, nmet);
}

// Stochastic beam search: cvc_beam_select_hist_parts whose ranking key is a Gumbel-perturbed sampling log-prob conditioned on the
// parent's key (the rule: the comment of beam_merge_kernel's STOCH form; contract: include/cvc_hip_blocks.h).
// workspace: 26 * B * beam floats -- the 17 of cvc_beam_select_hist_parts, then per row lseq and the raw logits of its 8 finalists.
extern "C" int cvc_beam_select_stoch_parts(const float* logits, int nparts, long long part_stride, const float* bias,
                                           const float* score_in, const uint8_t* done_in, int B, int beam, int V, int unk_idx, int t,
                                           const int64_t* hist_in, int64_t* hist_out, long long hist_stride, const cvc_constraint* c,
                                           float inv_tau, const uint32_t* state, const float* logq_in, const float* G_in,
                                           int64_t* parent, int64_t* word, float* score_out, uint8_t* done_out, float* logq_out,
                                           float* G_out, int32_t* nbanned, float* workspace, cvc_stream_t stream) {
    const int rc = beam_select_check(logits, nparts, score_in, done_in, B, beam, V, parent, word, score_out, done_out, workspace);
    if (rc != 0) return rc;
    if (t < 0 || t > CONS_T_MAX) return CVC_E_TOOBIG;
    if (c != nullptr && cons_rules_check(c) != 0) return CVC_E_BADARG;
    if (!hist_out || (t > 0 && !hist_in) || (const int64_t*)hist_out == hist_in || hist_stride < (long long)B * beam) return CVC_E_BADARG;
    if (!(inv_tau > 0.f) || !isfinite(inv_tau) || !state || !logq_in || !G_in || !logq_out || !G_out) return CVC_E_BADARG;
    if ((const float*)logq_out == logq_in || (const float*)G_out == G_in || (const float*)score_out == score_in) return CVC_E_BADARG;
    const cvc_constraint none = {0, 0, 0, 0, nullptr, nullptr, 0};
    if (c == nullptr) c = &none;
    const ConsArgs ra{hist_in, hist_stride, t, c->no_repeat_ngram, c->no_immediate_repeat != 0, c->min_len, c->ban, c->nban,
                      c->bad_end, c->nbad, nbanned};
    const uint32_t site = CVC_SBS_SITE + (uint32_t)t;
    float* lseq = workspace + (size_t)17 * B * beam;
    float* raw = workspace + (size_t)18 * B * beam;
    return beam_select_run<true, false, false, true>(logits, nparts, part_stride, bias, score_in, done_in, B, beam, V, unk_idx, t == 0 ? 1 : 0,
                                                     parent, word, score_out, done_out, workspace, stream,
                                                     StochScanArgs{ra, inv_tau, state, site, lseq, raw}, HistArgs{hist_in, hist_out, hist_stride, t},
                                                     NoGroups{}, StochArgs{inv_tau, state, site, lseq, raw, logq_in, G_in, logq_out, G_out});
}

namespace {
// rank-0 hypothesis of every clip: walk the parent pointers back from the last step (one thread), then copy the words and
// the attention rows of the path (the attention of step t was computed for the PARENT row of the word chosen at step t)
// (start: the slot to walk back from, clip b's at start[b * start_stride], clamped like a parent; NULL: slot 0)
__global__ __launch_bounds__(256) void beam_backtrack_kernel(const int64_t* words, const int64_t* parent, const float* att, int beam,
                                                            int T, int N, int rows, int64_t* seq, float* att_out,
                                                            const int64_t* start = nullptr, long long start_stride = 1) {
    __shared__ int path[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        int k = 0;
        if (start != nullptr) {
            const long long s = start[(size_t)b * start_stride];
            k = s < 0 ? 0 : (s >= beam ? beam - 1 : (int)s);
        }
        for (int t = T - 1; t >= 0; --t) {
            const size_t at = (size_t)t * rows + (size_t)b * beam + k;
            seq[(size_t)b * T + t] = words[at];
            int kp = (int)parent[at];
            kp = kp < 0 ? 0 : (kp >= beam ? beam - 1 : kp);
            path[t] = kp;
            k = kp;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < T * N; idx += 256) {
        const int t = idx / N, n = idx - t * N;
        att_out[((size_t)b * T + t) * N + n] = att[((size_t)t * rows + (size_t)b * beam + path[t]) * N + n];
    }
}

// Final ranking of a clip's hypotheses, one wave per clip.  len(r) = position of the first 0 in r's history + 1, or T without one:
// lane s holds step s of the row and the ballot of (word == 0) gives the position.  norm(r) = score(r) / len(r)^alpha in fp32
// (alpha == 0: score(r) itself, no power is evaluated; -inf stays -inf).  Lane k then counts the slots that come before slot k --
// larger norm, ties -> lowest slot, NaN last -- and writes order[b, that count] = k.
// FORCE (cvc_beam_rank_force): nmet(r) = the number of the clip's active forced words (force_active()) in the row's T-step history,
// one more ballot per entry; the slots then sort by the key (norm is NaN, norm == -inf, nmet descending, norm descending, slot):
// the best hypothesis is the best-normed one among those that met the most forced words, and the fillers at -inf come after
// every hypothesis.
struct NoRankForce {};
struct RankForceArgs { const int32_t* force; int nforce, V, unk; int32_t* nmet; };
template <bool FORCE>
__device__ __forceinline__ void beam_rank_body(const int64_t* hist, long long stride, const float* score, int beam, int T, float alpha,
                                               int64_t* order, float* norm, int32_t* len,
                                               std::conditional_t<FORCE, RankForceArgs, NoRankForce> fa) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int mylen = T;
    [[maybe_unused]] int mymet = 0, act = 0;
    if constexpr (FORCE) act = force_active(fa.force + (size_t)b * fa.nforce, fa.nforce, fa.V, fa.unk);
    for (int k = 0; k < beam; ++k) {
        const long long h = lane < T ? (long long)hist[(size_t)lane * stride + (size_t)b * beam + k] : -1ll;
        const unsigned long long m = __ballot(h == 0);
        const int l = m != 0ull ? __ffsll((long long)m) : T;
        if (lane == k) mylen = l;
        if constexpr (FORCE) {
            int met = 0;
            for (int j = 0; j < fa.nforce; ++j)
                if ((act >> j) & 1) met += __ballot(h == (long long)fa.force[(size_t)b * fa.nforce + j]) != 0ull ? 1 : 0;
            if (lane == k) mymet = met;
        }
    }
    float nv = -INFINITY;
    if (lane < beam) {
        const float sc = score[b * beam + lane];
        nv = alpha == 0.f ? sc : sc / powf((float)mylen, alpha);
        norm[b * beam + lane] = nv;
        len[b * beam + lane] = mylen;
        if constexpr (FORCE) fa.nmet[b * beam + lane] = mymet;
    }
    const bool nan_me = nv != nv;
    [[maybe_unused]] const int cls = nan_me ? 2 : (nv == -INFINITY ? 1 : 0);
    int before = 0;
    for (int j = 0; j < beam; ++j) {
        const float nj = __shfl(nv, j, 64);
        const bool nan_j = nj != nj;
        bool first = nan_me ? (!nan_j || j < lane) : (!nan_j && (nj > nv || (nj == nv && j < lane)));
        if constexpr (FORCE) {
            const int mj = __shfl(mymet, j, 64), cj = nan_j ? 2 : (nj == -INFINITY ? 1 : 0);
            first = cj != cls ? cj < cls : (mj != mymet ? mj > mymet : ((cls == 0 && nj != nv) ? nj > nv : j < lane));
        }
        before += first ? 1 : 0;
    }
    if (lane < beam) order[b * beam + before] = lane;
}
__global__ __launch_bounds__(64) void beam_rank_kernel(const int64_t* hist, long long stride, const float* score, int beam, int T,
                                                       float alpha, int64_t* order, float* norm, int32_t* len) {
    beam_rank_body<false>(hist, stride, score, beam, T, alpha, order, norm, len, NoRankForce{});
}
__global__ __launch_bounds__(64) void beam_rank_force_kernel(const int64_t* hist, long long stride, const float* score, int beam, int T,
                                                             float alpha, int64_t* order, float* norm, int32_t* len, RankForceArgs fa) {
    beam_rank_body<true>(hist, stride, score, beam, T, alpha, order, norm, len, fa);
}
}  // namespace

// the argument checks of the two ranking blocks
static int beam_rank_check(const int64_t* hist, long long hist_stride, const float* score, int B, int beam, int T, float alpha,
                           const int64_t* order, const float* norm, const int32_t* len) {
    if (!hist || !score || !order || !norm || !len || B < 1 || beam < 1 || beam > BEAM_MAX || T < 1) return CVC_E_BADARG;
    if (hist_stride < (long long)B * beam || !(alpha >= 0.f) || isinf(alpha)) return CVC_E_BADARG;
    if (T > CONS_T_MAX) return CVC_E_TOOBIG;
    return 0;
}

extern "C" int cvc_beam_rank(const int64_t* hist, long long hist_stride, const float* score, int B, int beam, int T, float alpha,
                             int64_t* order, float* norm, int32_t* len, cvc_stream_t stream) {
    const int rc = beam_rank_check(hist, hist_stride, score, B, beam, T, alpha, order, norm, len);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(beam_rank_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, hist, hist_stride, score, beam, T, alpha, order, norm,
                       len);
    return cvc_launch_status();
}

// cvc_beam_rank for the hypotheses of cvc_beam_select_force_parts: slots that met more forced words come first (contract:
// include/cvc_hip_blocks.h)
extern "C" int cvc_beam_rank_force(const int64_t* hist, long long hist_stride, const float* score, const int32_t* force, int nforce,
                                   int B, int beam, int T, int V, int unk_idx, float alpha, int64_t* order, float* norm, int32_t* len,
                                   int32_t* nmet, cvc_stream_t stream) {
    if (!force || !nmet || nforce < 1 || nforce > 3 || V < 1) return CVC_E_BADARG;
    const int rc = beam_rank_check(hist, hist_stride, score, B, beam, T, alpha, order, norm, len);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(beam_rank_force_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, hist, hist_stride, score, beam, T, alpha, order,
                       norm, len, RankForceArgs{force, nforce, V, unk_idx, nmet});
    return cvc_launch_status();
}

// behind both back-track entry points: the checks they share and the launch (start == NULL: every clip walks back from slot 0)
static int beam_backtrack_run(const int64_t* words, const int64_t* parent, const float* att, int B, int beam, int T, int N,
                              const int64_t* start, long long start_stride, int64_t* seq, float* att_out, cvc_stream_t stream) {
    if (!words || !parent || !att || !seq || !att_out || B < 1 || beam < 1 || T < 1 || T > 256 || N < 1) return CVC_E_BADARG;
    hipLaunchKernelGGL(beam_backtrack_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, words, parent, att, beam, T, N, B * beam,
                       seq, att_out, start, start_stride);
    return cvc_launch_status();
}

extern "C" int cvc_beam_backtrack_from(const int64_t* words, const int64_t* parent, const float* att, int B, int beam, int T, int N,
                                       const int64_t* start, long long start_stride, int64_t* seq, float* att_out,
                                       cvc_stream_t stream) {
    if (!start || start_stride < 1) return CVC_E_BADARG;
    return beam_backtrack_run(words, parent, att, B, beam, T, N, start, start_stride, seq, att_out, stream);
}

extern "C" int cvc_beam_backtrack(const int64_t* words, const int64_t* parent, const float* att, int B, int beam, int T, int N,
                                  int64_t* seq, float* att_out, cvc_stream_t stream) {
    return beam_backtrack_run(words, parent, att, B, beam, T, N, nullptr, 1, seq, att_out, stream);
}

extern "C" int cvc_gather_rows(const float* src, const int64_t* parent, int rows, int beam, int width, float* dst,
                               cvc_stream_t stream) {
    if (!src || !parent || !dst || rows < 1 || beam < 1 || width < 4 || (width & 3)) return CVC_E_BADARG;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((width / 4 + WG - 1) / WG, rows), dim3(WG), 0, (hipStream_t)stream, src,
                       parent, beam, width, dst);
    return cvc_launch_status();
}
