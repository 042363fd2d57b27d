// Word-selection keys of the fused greedy tail (cvc_packed_linear_keys_fwd posts them, cvc_packed_lstm_embgate_keys_fwd and
// cvc_keys_finalize read them): a candidate (logit v, word index n) is ONE 64-bit integer whose unsigned order is "value
// descending, index ascending" -- better() of row_block.h -- so the best candidate of a row is an integer max over the posting
// workgroups, in any order, with no merge pass:
//   key = (ordered(v) << 32) | (0x7fffffff - n),   ordered(v) = the float's bits with the sign flipped (v >= 0) or all bits
//   inverted (v < 0): monotonic.  -0 is encoded as +0 (they compare equal: the lower index decides); a NaN and -inf are never
//   candidates, exactly as in the record form of the head's epilogue ("v > v1" from v1 = -inf); every candidate's key is
//   non-zero, so key 0 means "no candidate".
// A step's candidates live in keys[KEY_SLOTS][KEY_ROWS] (slot = block index % KEY_SLOTS; slot-major, so the 64 rows a wave posts
// with one instruction are 512 contiguous bytes and a row's slots lie on different lines: the memory-side integer max is
// requested per 64-byte line, and a line then takes the posts of a quarter of the workgroups, 8 rows each), UNK's own logit in a
// separate word per row: captioner.py:415-422 picks the best word, or the second best if the best is UNK -- the
// best NON-UNK word, unless there is none (V = 1, or every other logit NaN or -inf), then UNK; a row without any candidate yields word 0.
#pragma once
#include <stdint.h>

constexpr int KEY_SLOTS = 4;
constexpr int KEY_ROWS = 64;                                   // rows per step in both buffers, whatever M is

__device__ __forceinline__ unsigned long long sel_key(float v, int n) {
    if (!(v > -__builtin_inff())) return 0ull;                  // NaN, -inf
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;                              // -0 -> +0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (uint32_t)(0x7fffffff - n);
}
__device__ __forceinline__ float sel_key_value(unsigned long long k) {
    const uint32_t u = (uint32_t)(k >> 32);
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ int sel_key_index(unsigned long long k) { return 0x7fffffff - (int)(uint32_t)(k & 0xffffffffull); }
// the chosen word from the best non-UNK key and UNK's key (see above)
__device__ __forceinline__ int sel_key_word(unsigned long long best, unsigned long long kunk, int unk) {
    return best != 0ull ? sel_key_index(best) : (kunk != 0ull ? unk : 0);
}
