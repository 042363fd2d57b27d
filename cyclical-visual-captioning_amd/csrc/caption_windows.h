// A caption's 4-word windows in one wave, as the consensus kernels keep them (csrc/consensus.hip, csrc/consensus_mix.hip): lane p holds
//   the window that starts at position p -- four words of 16 bits, the first in the highest bits, 0 past the caption's end
//   (csrc/caption_ngrams.h: ngram_key of order 4).  The n-gram of order n that starts there is the window's highest 16 n bits.
#pragma once
#include "cvc_common.h"

namespace cvc_windows {

// lane p's value in every lane (p is wave-uniform)
__device__ __forceinline__ unsigned long long lane_key(unsigned long long v, int p) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, p);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), p);
    return ((unsigned long long)hi << 32) | lo;
}

// on how many leading 16-bit words two windows agree, given their exclusive or (4: on all) -- the n-grams of order n that start
// at the two positions are the same one iff this is >= n, provided one of them is an n-gram at all (its n words are non-zero)
__device__ __forceinline__ int lead_words(unsigned long long x) { return x != 0ull ? (int)__builtin_clzll(x) >> 4 : 4; }

// idf of key[n] where own[n], from the sorted table (cider_d_kernel's idf_of: the same binary search, hence the same entry) -- the
// four searches advance together, so that their dependent loads overlap; a lane that owns nothing re-reads keys[0]
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

}  // namespace cvc_windows
