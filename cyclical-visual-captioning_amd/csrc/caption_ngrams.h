// A caption in one wave: its words in LDS and the exact 64-bit keys of its n-grams (csrc/cider.hip, csrc/overlap.hip).
//   A caption is a row of T <= 63 int64 ids; lane p owns the n-grams (n = 1..4) that start at position p.  Words are held as id + 1
//   in 16 bits (0 past the caption's end), an n-gram is one key: 16 bits per word, first word in the highest bits, unused
//   positions 0 -- the order n is part of the key, nothing is hashed.
//   COUNT_EOS: the end mark (the first 0) is the caption's last word (CIDEr-D here); else the words are the ids before it (BLEU,
//   ROUGE-L) and L = 0 is possible.
#pragma once
#include "cvc_common.h"

namespace cvc_caption {

constexpr int MAXT = 63;

// the caption's words into sw[0 .. 67] as id + 1 (0 from position L on) -> L
template <bool COUNT_EOS>
__device__ __forceinline__ int load_caption(const int64_t* cap, int T, int lane, uint32_t* sw) {
    const int64_t w = lane < T ? cap[lane] : 1;
    const unsigned long long eos = __ballot(lane < T && w == 0);
    const int L = eos != 0ull ? (int)__builtin_ctzll(eos) + (COUNT_EOS ? 1 : 0) : T;
    __syncthreads();                      // the previous caption's readers are done
    sw[lane] = lane < L ? (uint32_t)((w + 1) & 0xffff) : 0u;
    if (lane < 4) sw[64 + lane] = 0u;
    __syncthreads();
    return L;
}

__device__ __forceinline__ unsigned long long ngram_key(const uint32_t* sw, int lane, int n) {
    unsigned long long k = 0ull;
    for (int i = 0; i < n; ++i) k |= (unsigned long long)sw[lane + i] << (48 - 16 * i);
    return k;
}

// how many of buf[0 .. npos) hold `key`; *first: none of them before `lane`
__device__ __forceinline__ int count_key(const unsigned long long* buf, int npos, unsigned long long key, int lane, bool* first) {
    int c = 0;
    bool f = true;
    for (int q = 0; q < npos; ++q) {
        const bool same = buf[q] == key;
        c += same ? 1 : 0;
        f = f && !(same && q < lane);
    }
    *first = f;
    return c;
}

}  // namespace cvc_caption
