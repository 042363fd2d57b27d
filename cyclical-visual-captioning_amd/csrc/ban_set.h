// The ban set of constrained decoding, once: what a selection kernel that knows its row's history takes on top of its own arguments,
// the checks of the rules, and the V-bit LDS map built from the history and the lists.  Shared by the sampling kernel's CONS form
// (csrc/sample_select.h, cvc_constrained_select_parts) and the beam row scan's HIST form (csrc/beam.hip,
// cvc_beam_select_hist_parts), so the two cannot drift.  The rule: the comment of cvc_constrained_select_parts in
// include/cvc_hip_blocks.h.
#pragma once
#include "cvc_common.h"

namespace {

constexpr int CONS_T_MAX = 64;                 // history steps: one lane per step
constexpr int CONS_LIST_MAX = 256;             // entries of a list: one thread per entry
struct NoCons {};
// the row's history hist[s * hist_stride + row], s < t, and the rules
struct ConsArgs {
    const int64_t* hist; long long hist_stride; int t;
    int ngram, immediate, min_len;
    const int32_t* ban; int nban;
    const int32_t* bad_end; int nbad;
    int32_t* nbanned;
};
template <bool CONS> struct cons_args { using type = NoCons; };
template <> struct cons_args<true> { using type = ConsArgs; };

// thread tid's step of the row's history (0 past t): a kernel issues this load next to its logit loads, before it waits for them
__device__ __forceinline__ long long load_hist_step(const ConsArgs& ca, int row, int tid) {
    return tid < ca.t ? (long long)ca.hist[(size_t)tid * ca.hist_stride + row] : 0ll;
}

// Ban(t, row) as a bit map over the vocabulary, bit v of bits[v >> 5]: one word of the map per thread of the workgroup (V <= 32 * NT,
// NT >= CONS_LIST_MAX, NT >= CONS_T_MAX), hist = CONS_T_MAX words of LDS, hv = load_hist_step() of this thread.  History to LDS, a
// barrier, then UNK / min_len / the previous word on thread 0, one thread per list entry, lane j for the n-gram that ends at y_j (LDS
// atomicOr), and the barrier after which every thread may read the map.  Ids outside [0, V) set nothing.
template <int NT>
__device__ __forceinline__ void build_ban_map(const ConsArgs& ca, long long hv, int V, int unk, int tid, uint32_t* bits, long long* hist) {
    static_assert(NT >= CONS_LIST_MAX && NT >= CONS_T_MAX, "one thread per list entry, one lane per step");
    const int t = ca.t;
    bits[tid] = 0u;
    if (tid < t) hist[tid] = hv;
    __syncthreads();
    auto ban = [&](long long v) { if (v >= 0 && v < V) atomicOr(&bits[v >> 5], 1u << (v & 31)); };
    if (tid == 0) {
        ban(unk);
        if (t < ca.min_len) ban(0);
        if (ca.immediate && t >= 1) ban(hist[t - 1]);
    }
    if (tid < ca.nban) ban(ca.ban[tid]);
    if (t >= 1 && tid < ca.nbad && (long long)ca.bad_end[tid] == hist[t - 1]) ban(0);
    if (ca.ngram >= 1 && tid < t && tid >= ca.ngram - 1) {          // lane j: y_j is banned if the n - 1 words before it are the last n - 1
        bool same = true;
        for (int i = 1; i < ca.ngram; ++i) same = same && hist[tid - i] == hist[t - i];
        if (same) ban(hist[tid]);
    }
    __syncthreads();
}

}  // namespace

// the checks of the rules every constrained block shares (c != NULL)
static int cons_rules_check(const cvc_constraint* c) {
    if (c->no_repeat_ngram < 0 || c->no_repeat_ngram > CONS_T_MAX || c->min_len < 0) return CVC_E_BADARG;
    if (c->nban < 0 || c->nban > CONS_LIST_MAX || c->nbad < 0 || c->nbad > CONS_LIST_MAX) return CVC_E_BADARG;
    if ((c->nban > 0 && !c->ban) || (c->nbad > 0 && !c->bad_end)) return CVC_E_BADARG;
    return 0;
}
