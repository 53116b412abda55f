// Greedy in-silico evolution: one round's selection.  Per sequence b, of
// all substitutions (base a at position p, forward coordinates) the one with the largest objective
//   O_f[a,p] = sum_t (double)w[b,t] (double)delta_f[b,t,a,p]           (t ascending, fp64)
//   O_r[a,p] = sum_t (double)w[b,t] (double)delta_r[b,t,3-a,L-1-p]     (both strands only)
//   gain     = O_f, or 0.5 (O_f + O_r) with both strands
// among the admissible ones -- a is not the base at p (at an N all four are), mask[b,p] != 0,
// gain > min_gain >= 0 -- ties going to the lowest p, then the lowest a.  The winner is logged,
// written into the (B,L) code matrix and, with `lock`, cleared in the mask.  delta_f / delta_r are
// explainn_ism's (B,T,4,L) maps of the batch staged forward / reverse-complemented (the reverse map is
// in its own strand's coordinates, hence 3-a and L-1-p).
// Geometry (an untuned first choice): one workgroup of EV_WAVES waves per 64 sequences, lane =
// sequence, the waves take the positions round-robin.  A lane keeps its best candidate with a strict
// `>` while a and its positions ascend, so the tie rule holds inside a wave; the waves' bests meet in
// LDS under the full order (gain, then position), and wave 0 applies the winner behind the barrier,
// after every read of the workgroup's rows.  No atomics, no workspace; nothing depends on which wave
// finishes first.
#include <cmath>

#include "common.h"

#define EV_WAVES 16                // waves per workgroup (1024 threads)

struct ev_args {
    const float* fwd; const float* rev;     // the two maps (rev null: one strand)
    uint8_t* codes; uint8_t* mask;          // (B,L); mask null = every position open
    const float* weights; int wpr;          // (T,) or, wpr != 0, (B,T)
    int B, T, L, lock;
    double min_gain;
    int32_t* pos; uint8_t* ref; uint8_t* alt; double* gain;    // (B)
};

// (g, p) beats the best so far (bg, bp)?  bp < 0: none yet, and bg is min_gain, which every candidate
// exceeds.  Two candidates never share a position here: a was settled where the position was scanned.
__device__ __forceinline__ bool ev_beats(double g, int p, double bg, int bp) {
    return p >= 0 && (g > bg || (g == bg && p < bp));
}

// O[a] = sum_t w_t delta[b,t,a,pp] from a (B,T,4,L) map (row = its element [b][0][0][0])
__device__ __forceinline__ void ev_map_objective(const float* __restrict__ row, const float* __restrict__ wrow,
                                                 int T, int L, int pp, double (&O)[4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a) O[a] = 0.0;
    for (int t = 0; t < T; ++t) {
        const double w = (double)wrow[t];
        float v[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) v[a] = row[((size_t)t * 4 + a) * L + pp];
#pragma unroll
        for (int a = 0; a < 4; ++a) O[a] += w * (double)v[a];
    }
}

__global__ __launch_bounds__(64 * EV_WAVES) void evolve_select_kernel(const ev_args A) {
    __shared__ double sg[EV_WAVES][64];
    __shared__ int sp[EV_WAVES][64], sa[EV_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bi = blockIdx.x * 64 + lane;
    const bool live = bi < A.B;
    const int b = min(bi, A.B - 1), L = A.L;
    const uint8_t* crow = A.codes + (size_t)b * L;
    const uint8_t* mrow = A.mask ? A.mask + (size_t)b * L : nullptr;
    const float* __restrict__ wrow = A.weights + (A.wpr ? (size_t)b * A.T : 0);
    const float* __restrict__ frow = A.fwd + (size_t)b * A.T * 4 * L;
    const float* __restrict__ rrow = A.rev ? A.rev + (size_t)b * A.T * 4 * L : nullptr;
    double bg = A.min_gain;
    int bp = -1, ba = 0;
    for (int p = wave; p < L; p += EV_WAVES) {
        const int s = crow[p];
        const bool open = live && (!mrow || mrow[p] != 0);
        if (!__any(open)) continue;                    // wave-uniform
        double Of[4], Or[4] = {0.0, 0.0, 0.0, 0.0};
        ev_map_objective(frow, wrow, A.T, L, p, Of);
        if (rrow) ev_map_objective(rrow, wrow, A.T, L, L - 1 - p, Or);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            double g = Of[a];
            if (rrow) g = 0.5 * (g + Or[3 - a]);
            if (open && a != s && g > bg) { bg = g; bp = p; ba = a; }      // (s >= 4, an N, equals no a)
        }
    }
    sg[wave][lane] = bg; sp[wave][lane] = bp; sa[wave][lane] = ba;
    __syncthreads();
    if (wave != 0 || !live) return;
    for (int w = 1; w < EV_WAVES; ++w) {
        const double og = sg[w][lane];
        const int op = sp[w][lane];
        if (ev_beats(og, op, bg, bp)) { bg = og; bp = op; ba = sa[w][lane]; }
    }
    if (bp >= 0) {
        const size_t at = (size_t)b * L + bp;
        A.pos[b] = bp; A.ref[b] = A.codes[at]; A.alt[b] = (uint8_t)ba; A.gain[b] = bg;
        A.codes[at] = (uint8_t)ba;
        if (A.lock && A.mask) A.mask[at] = 0;
    } else {
        A.pos[b] = -1; A.ref[b] = 255; A.alt[b] = 255; A.gain[b] = 0.0;
    }
}

extern "C" int explainn_evolve_pick(const float* delta_fwd, const float* delta_rev, uint8_t* codes,
                                    uint8_t* mutable_mask, const float* weights, int weights_per_row, int B, int T,
                                    int L, int lock, float min_gain, int32_t* pos, uint8_t* ref, uint8_t* alt,
                                    double* gain, void* stream) {
    if (!delta_fwd || !codes || !weights || !pos || !ref || !alt || !gain) {
        explainn_set_error("delta_fwd, codes, weights, pos, ref, alt and gain are required");
        return EXPLAINN_E_ARG;
    }
    if (B < 1 || T < 1 || L < 1) { explainn_set_error("B, T and L must be positive (got %d, %d, %d)", B, T, L); return EXPLAINN_E_ARG; }
    if (!std::isfinite(min_gain) || min_gain < 0.f) {
        explainn_set_error("min_gain must be finite and not negative (got %g)", (double)min_gain);
        return EXPLAINN_E_ARG;
    }
    ev_args A;
    A.fwd = delta_fwd; A.rev = delta_rev;
    A.codes = codes; A.mask = mutable_mask;
    A.weights = weights; A.wpr = weights_per_row;
    A.B = B; A.T = T; A.L = L; A.lock = lock;
    A.min_gain = (double)min_gain;
    A.pos = pos; A.ref = ref; A.alt = alt; A.gain = gain;
    hipLaunchKernelGGL(evolve_select_kernel, dim3((B + 63) / 64), dim3(64 * EV_WAVES), 0,
                       static_cast<hipStream_t>(stream), A);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
