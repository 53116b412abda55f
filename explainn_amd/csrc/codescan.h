// The eval-mode filter activation on base codes: the only definition.
//
// In eval mode BatchNorm1 is folded, so a unit's activation at a start position depends only on the k
// bases under it.  Every kernel that evaluates it from base codes -- site_kernel (interpret.hip),
// sites_kernel (sites.hip), act_hist_kernel (actnull.hip), record_best_kernel (enrich.hip) -- runs the
// expressions of this header, which is what keeps them equal bit for bit: a null histogram calibrates
// call_sites thresholds, record_best scores compare against them, and every test is a dense recount.
// (conv_act_kernel and the MFMA filter bank use another algebra and are tied to this chain by tests.)
//
// The chain: accumulate from 0.f, one add per tap in j order, fp32 (no fast-math: the order is the
// bits), qval (common.h), round to float16.  Device-only, all __forceinline__.  It holds the bit pattern
// of an activation, the tap chain and the staging of a span of codes; what happens to a hit afterwards (its
// position-order rank, block_hit_ranks) is sitescan.h's.
#pragma once
#include <hip/hip_fp16.h>

#include "common.h"

// ---- the bit pattern of an activation --------------------------------------------------------------
// float16(exp(.)) is never negative, so its pattern is one of 32768 (0x0000 .. 0x7FFF) that sort in the
// order of the values they encode (+inf = 0x7C00, the NaN patterns above it): integer compares, maxima
// and histogram bins over patterns are compares, maxima and bins over values.  The mask drops the sign
// a NaN may carry and nothing else.
__device__ __forceinline__ __half act_half(float alpha, float acc, float shift) {
    return __float2half_rn(qval(alpha, acc, shift));       // round-to-nearest-even, overflow -> inf
}
__device__ __forceinline__ unsigned act_bits(float alpha, float acc, float shift) {
    return __half_as_ushort(act_half(alpha, acc, shift)) & 0x7FFFu;
}
// the same as the float16 value numpy stores, widened to fp32
__device__ __forceinline__ float act_value(float alpha, float acc, float shift) {
    return __half2float(act_half(alpha, acc, shift));
}

// ---- the tap chain ---------------------------------------------------------------------------------
// Accumulators: float (one unit's taps, float [k][5]) or float4 (a unit quad's, float4 [k][5]).
__device__ __forceinline__ void cs_zero(float& a) { a = 0.f; }
__device__ __forceinline__ void cs_zero(float4& a) { a = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void cs_add(float& a, float v) { a += v; }
__device__ __forceinline__ void cs_add(float4& a, const float4& v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }

// N independent starts per lane, interleaved inside the tap loop.  Start i reads cp[i][j * step] at tap
// j: a forward start p of staged codes cs is (cs + p, +1); the reverse strand, the filter on
// rc(seq[p : p + k]), meets the complemented code at p + k - 1 - j: (complemented codes + p + k - 1, -1).
// BOTH: the reverse chain of the same starts, rp[i] = complemented codes + p + k - 1, rides in the loop.
template <bool BOTH, int N, typename A>
__device__ __forceinline__ void tap_chains(const A* taps, int k, const uint8_t* const (&cp)[N], int step,
                                           A (&acc)[N], const uint8_t* const (&rp)[N], A (&rev)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) { cs_zero(acc[i]); if (BOTH) cs_zero(rev[i]); }
    for (int j = 0; j < k; ++j) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            cs_add(acc[i], taps[j * 5 + cp[i][j * step]]);
            if (BOTH) cs_add(rev[i], taps[j * 5 + rp[i][-j]]);
        }
    }
}
// one strand
template <int N, typename A>
__device__ __forceinline__ void tap_chain(const A* taps, int k, const uint8_t* const (&cp)[N], int step,
                                          A (&acc)[N]) {
    tap_chains<false>(taps, k, cp, step, acc, cp, acc);
}

// ---- staging a span of codes -----------------------------------------------------------------------
// src[0 .. n) into LDS by nthreads threads: a byte above 4 is read as N and makes the return value 1
// (the caller raises the input flag).  dst gets the codes, or with rc their complements; BOTH: dst the
// codes and comp the complements.
template <bool BOTH>
__device__ __forceinline__ int stage_codes(const uint8_t* __restrict__ src, int n, int tid, int nthreads,
                                           uint8_t* dst, int rc, uint8_t* comp) {
    int bad = 0;
    for (int i = tid; i < n; i += nthreads) {
        int v = src[i];
        if (v > 4) { v = 4; bad = 1; }
        const int w = v < 4 ? 3 - v : v;
        if (BOTH) { dst[i] = (uint8_t)v; comp[i] = (uint8_t)w; }
        else dst[i] = (uint8_t)(rc ? w : v);
    }
    return bad;
}
