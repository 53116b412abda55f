// The quantised motif table as a kernel stages it (pwm_sites_kernel, pwmsites.hip; pwm_best_kernel,
// pwmbest.hip; pwm_variant_kernel, pwmvariants.hip, which walks pwm_best_kernel's layout): which motifs are empty, the word that scores both strands at once, and the limits of the
// geometry.  A motif is an integer table S[w][4], 0 <= S <= bins; the set is int16 [M][wmax][4].
//
// What the two kernels do NOT share is the table's layout in LDS and its N entry.  pwm_sites_kernel sums
// the halves of a word apart, so N holds a sentinel so negative that no window with an N reaches a
// threshold >= 0.  pwm_best_kernel adds whole words (two sums <= 8192 never carry), where a negative half
// would borrow from the other: its N holds 0 and the window's codes are ORed instead.
#pragma once
#include "common.h"

// the only way a width is read: a motif past M, or of a width outside [1, wmax], is empty
__device__ __forceinline__ int pwm_width(const int* __restrict__ widths, int m, int M, int wmax) {
    if (m >= M) return 0;
    const int w = widths[m];
    return (w >= 1 && w <= wmax) ? w : 0;
}

// column j < w, base c < 4 of a motif's table `row` [wmax][4]: the forward score S[j][c] in the low half,
// and in the high half the score the reverse strand takes at the same base, S[w-1-j][3-c] -- one walk over
// a window's codes in forward order scores both strands
__device__ __forceinline__ unsigned pwm_pair_word(const int16_t* row, int w, int j, int c) {
    return (unsigned)(uint16_t)row[j * 4 + c] | ((unsigned)(uint16_t)row[(w - 1 - j) * 4 + 3 - c] << 16);
}

// The tables of the G motifs from m0 on as pwm_best_kernel (pwmbest.hip) and pwm_variant_kernel
// (pwmvariants.hip) walk them, staged by a workgroup of T threads: words [G / 2][wmax][8][2], the words of the
// two motifs of a pair side by side, so that one 64-bit read serves both chains.  A column past a motif's
// width, the codes 4..7 (N) and a motif past M hold 0.  The caller's barrier follows.
template <int G, int T>
__device__ __forceinline__ void pwm_stage_pair_tables(int* words, const int16_t* __restrict__ S,
                                                      const int* __restrict__ widths, int m0, int M, int wmax, int tid) {
    for (int i = tid; i < G * wmax * 8; i += T) {
        // word i: pair q, column j, code c, motif 2 q + h
        const int h = i & 1, c = (i >> 1) & 7, j = (i >> 4) % wmax, q = (i >> 4) / wmax, m = m0 + 2 * q + h;
        unsigned word = 0;
        const int w = pwm_width(widths, m, M, wmax);
        if (j < w && c < 4) word = pwm_pair_word(S + (size_t)m * wmax * 4, w, j, c);
        words[i] = (int)word;
    }
}

// grid.y = the motif groups; a score <= wmax bins <= 8192 (a call without bins passes 1)
inline bool pwm_geometry_ok(const char* who, int M, int wmax, int bins) {
    constexpr int max_m = 65535 * EXPLAINN_PWM_GROUP;
    if (M >= 0 && M <= max_m && wmax >= 1 && wmax <= EXPLAINN_MOTIF_MAX_WIDTH && bins >= 1 &&
        bins <= EXPLAINN_MOTIF_MAX_BINS)
        return true;
    explainn_set_error("%s: need 0 <= M <= %d, 1 <= wmax <= %d and 1 <= bins <= %d (M=%d wmax=%d bins=%d)", who, max_m,
                       EXPLAINN_MOTIF_MAX_WIDTH, EXPLAINN_MOTIF_MAX_BINS, M, wmax, bins);
    return false;
}
