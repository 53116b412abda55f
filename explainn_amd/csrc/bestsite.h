// The best site of a record: the only definition of its key, its site word and its offset check.
//
// record_best_kernel (enrich.hip, float16 activation patterns) and pwm_best_kernel (pwmbest.hip, integer
// PWM scores) both pick, per (unit, record), the largest 15-bit score over the record's live starts and
// strands.  Every (start, strand) becomes the integer key
//     bits << 31 | (~start & 0x3FFFFFFF) << 1 | is_plus
// so the largest key is the largest score, then the lowest start, then '+': one wave maximum per (unit,
// record) decides and nothing depends on the order in which starts are visited.  A live start's key is
// never 0 (start < 2^30, so ~start & 0x3FFFFFFF is not 0): key 0 says "no site".  What the host reads is
// the score's pattern (uint16) and the site word, int32 (start << 1) | is_minus, -1 without a site.
// Device-only, all __forceinline__.
#pragma once
#include "common.h"

constexpr long long BEST_MAX_LEN = 1ll << 30;  // a record this long has no int32 (start << 1 | strand)

__device__ __forceinline__ unsigned long long best_key(unsigned bits, int p, int plus) {
    return ((unsigned long long)bits << 31) | ((unsigned long long)(~(unsigned)p & 0x3FFFFFFFu) << 1) |
           (unsigned long long)plus;
}

// the wave-max key's score pattern and site word
__device__ __forceinline__ uint16_t best_key_bits(unsigned long long key) { return (uint16_t)(key >> 31); }
__device__ __forceinline__ int32_t best_key_site(unsigned long long key) {
    const unsigned low = (unsigned)key & 0x7FFFFFFFu;          // ~start << 1 | is_plus
    return key == 0 ? -1 : (int32_t)((((~(low >> 1)) & 0x3FFFFFFFu) << 1) | ((low & 1u) ^ 1u));
}

// Record [a, b) of a sequence of seq_len bases: offsets that descend or leave [0, seq_len], or a record
// too long for the site word, are not ok: the record has no live start and its length counts as 0.
// Compares only: evaluate it before any read of the sequence.  (A macro: as an inline function the
// compiler simplifies the four compares on their own before it inlines them, and the callers' instruction
// streams come out reordered.)
#define BEST_RECORD_OK(a, b, seq_len) ((a) >= 0 && (b) >= (a) && (b) <= (seq_len) && (b) - (a) < BEST_MAX_LEN)
