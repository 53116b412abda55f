// The eval-mode unit behind the conv sums: the only definition.
//
// One unit in eval mode, from base codes: the raw conv sums g of a pooled window (taps ascending, one
// add per tap, from 0.f), the sign-aware MaxPool extreme, q = qval(alpha, ext, shift), FC1
// (y2 = sh2 + sum_w A2[:,w] q_w, w ascending), ReLU, FC2 (z = fc2 . relu(y2), channels ascending) and
// the eval BatchNorm3 (y3 = inv3 (z + fc2_b - rm3) + b3; the unit's output is relu(y3)).
// ism_units_kernel (ism.hip) and pg_path_kernel (pathgrad.hip) run the expressions of this header, which
// is what their exact statements rest on: ISM's "a substitution that moves no pooled extreme gives
// exactly 0" needs one code for reference and mutant, IG's exact-zero identity baseline and its
// sub-batch invariance need fixed chains.  (ig_eval_dy_kernel, inputgrad.hip, is another layout of this
// algebra -- LDS columns, register chunks of pooled positions -- tied to it by tests; it takes
// unit_inv3 and unit_dout from here.)
//
// The pooled extreme is NOT here, on purpose: ism_ext (ism.hip) folds with fmaxf, pg_pool
// (pathgrad.hip) compares `t > m` because it needs the index of the first maximum.  The two may differ
// on +-0 and on NaN, so each file keeps its own.
//
// Both kernels keep y2[100] per lane and sit at 255-256 VGPRs; what keeps them there (unit_opaque_zero,
// the two FC chains as macros) is explained once, below.  Device-only; functions are __forceinline__.
#pragma once
#include "common.h"

// Codes 0..3 are the bases.  In a baseline row of Integrated Gradients code 4 is an all-zero column (N,
// and the whole `zero` baseline) and code 5 is 0.25 in all four rows (the `uniform` baseline).
#define PG_CODE_ZERO 4
#define PG_CODE_UNIFORM 5

// ---- per-unit constants ----------------------------------------------------------------------------
// al, sh: the folded BatchNorm1 (q = exp(al ext + sh)); sg: the pooling direction (a unit with al < 0
// pools the minimum); inv3, c2, m3, be3: the eval BatchNorm3 behind fc2's bias.
struct unit_consts { float al, sh, sg, inv3, c2, m3, be3; };

__device__ __forceinline__ float unit_inv3(const float* __restrict__ g3, const float* __restrict__ rv3, int u) {
    return g3[u] / sqrtf(rv3[u] + (float)BN_EPS_D);
}
__device__ __forceinline__ unit_consts unit_load(const float* __restrict__ alpha,
                                                 const float* __restrict__ shift,
                                                 const float* __restrict__ fc2_b, const float* __restrict__ g3,
                                                 const float* __restrict__ b3, const float* __restrict__ rm3,
                                                 const float* __restrict__ rv3, int u) {
    unit_consts e;
    e.al = alpha[u]; e.sh = shift[u]; e.sg = e.al < 0.f ? -1.f : 1.f;
    e.inv3 = unit_inv3(g3, rv3, u);
    e.c2 = fc2_b[u]; e.m3 = rm3[u]; e.be3 = b3[u];
    return e;
}
// BatchNorm3 of z = fc2_w . relu(y2), before the unit's ReLU
__device__ __forceinline__ float unit_bn3(const unit_consts& e, float z) {
    return fmaf(e.inv3, z + e.c2 - e.m3, e.be3);
}

// ---- the unit's tables in LDS ----------------------------------------------------------------------
// All nthreads threads of the block call it; the caller's barrier follows.  A2T [n][FC_H]: the unit's A2
// transposed, so that a window's 100 channels are 25 float4 at a wave-uniform address.  Wl [k][8]: the
// tap table by code; codes 4..7 read 0, except that with UNIFORM code 5 is the mean of the four bases
// in exactly this association.  fcs [FC_H]: the unit's fc2 row.
template <bool UNIFORM>
__device__ __forceinline__ void unit_stage(const float* __restrict__ A2, const float* __restrict__ conv_w,
                                           const float* __restrict__ fc2_w, int u, int k, int n, int NS,
                                           int tid, int nthreads, float* A2T, float* Wl, float* fcs) {
    for (int i = tid; i < n * FC_H; i += nthreads) {
        const int w = i / FC_H, r = i - w * FC_H;
        A2T[i] = A2[((size_t)u * FC_H + r) * NS + w];
    }
    for (int i = tid; i < k * 8; i += nthreads) {
        const int t = i >> 3, a = i & 7;
        const float* wr = conv_w + (size_t)u * 4 * k + t;
        float v = 0.f;
        if (a < 4) v = wr[a * k];
        else if (UNIFORM && a == PG_CODE_UNIFORM) v = 0.25f * (((wr[0] + wr[k]) + wr[2 * k]) + wr[3 * k]);
        Wl[i] = v;
    }
    for (int i = tid; i < FC_H; i += nthreads) fcs[i] = fc2_w[(size_t)u * FC_H + i];
}

// ---- the conv sums of a pooled window --------------------------------------------------------------
// g[e] = sum_(t ascending) W[u, code(7w + e + t), t], e = 0..6.  code(position) is the caller's fetch of
// this lane's code: ISM reads its ring in LDS, IG a strided global column.  Positions 7w .. 7w + k + 5.
template <typename F>
__device__ __forceinline__ void unit_window(F code, const float* __restrict__ Wl, int w, int k, float* g) {
    const int q0 = POOLW * w;
#pragma unroll
    for (int e = 0; e < POOLW; ++e) g[e] = 0.f;
    for (int q = 0; q < k + POOLW - 1; ++q) {
        const int c = code(q0 + q);
#pragma unroll
        for (int e = 0; e < POOLW; ++e) {
            const int t = q - e;
            if ((unsigned)t < (unsigned)k) g[e] += Wl[t * 8 + c];
        }
    }
}

// ---- FC1, FC2 --------------------------------------------------------------------------------------
// A zero the compiler cannot see through.  A kernel that walks many positions (ISM) or nodes (IG) per
// lane adds it to the address of every LDS read of A2T and fcs inside that loop: the reads are
// loop-invariant, and without it the compiler hoists the 25 fc2 float4 out of the loop (and, in ISM,
// shares the A2 reads of the d = 1..3 pass with the N pass), keeping 100 or more registers live next to
// y2[100] -- spills.  Take a fresh one per loop trip.
__device__ __forceinline__ int unit_opaque_zero() {
    int fo = 0;
    asm volatile("" : "+v"(fo));
    return fo;
}

// The two chains over y2[100] are macros, not functions, on purpose.  An array handed to a function by
// reference stays in memory until that function is inlined, which is after the early scalar passes, and
// every later decision then falls differently: through a __forceinline__ helper pg_path_kernel came out
// in another schedule (1.2% slower on the MI355X) and ism_units_kernel<2>, <3> with 6 registers more
// (one wave per SIMD in place of two).  As text in the kernel they compile to what hand-written copies
// give.  Names ending in _ are the macros' own.
//
// UNIT_FC1_ADD: y2 += A2T[w] q.  A4: the window's 25 float4 (A2T + w * FC_H, plus the opaque zero
// inside a position / node loop).
#define UNIT_FC1_ADD(Y, A4, Q)                                          \
    do {                                                                \
        const float4* __restrict__ a4_ = (A4);                          \
        const float q_ = (Q);                                           \
        _Pragma("unroll") for (int r4_ = 0; r4_ < FC_H / 4; ++r4_) {    \
            const float4 a_ = a4_[r4_];                                 \
            (Y)[4 * r4_] = fmaf(a_.x, q_, (Y)[4 * r4_]);                \
            (Y)[4 * r4_ + 1] = fmaf(a_.y, q_, (Y)[4 * r4_ + 1]);        \
            (Y)[4 * r4_ + 2] = fmaf(a_.z, q_, (Y)[4 * r4_ + 2]);        \
            (Y)[4 * r4_ + 3] = fmaf(a_.w, q_, (Y)[4 * r4_ + 3]);        \
        }                                                               \
    } while (0)
// UNIT_FC2: z = fc2 . relu(y2), channels ascending from 0.f.  F: the fc2 row (fcs, plus the opaque zero
// inside a position / node loop), read as 25 float4; an address expression, used once per float4 (through
// a local pointer pg_path_kernel falls into the other schedule again).
#define UNIT_FC2(Z, Y, F)                                                       \
    do {                                                                        \
        float z_ = 0.f;                                                         \
        _Pragma("unroll") for (int r4_ = 0; r4_ < FC_H / 4; ++r4_) {            \
            const float4 f4_ = *reinterpret_cast<const float4*>((F) + 4 * r4_); \
            z_ = fmaf(f4_.x, fmaxf((Y)[4 * r4_], 0.f), z_);                     \
            z_ = fmaf(f4_.y, fmaxf((Y)[4 * r4_ + 1], 0.f), z_);                 \
            z_ = fmaf(f4_.z, fmaxf((Y)[4 * r4_ + 2], 0.f), z_);                 \
            z_ = fmaf(f4_.w, fmaxf((Y)[4 * r4_ + 3], 0.f), z_);                 \
        }                                                                       \
        (Z) = z_;                                                               \
    } while (0)

// ---- the head's weight on the unit -----------------------------------------------------------------
// dF/d(unit output) for F = sum_t dl[b,t] logit_t: dl[b,:] . final_w[:,u], tasks ascending
__device__ __forceinline__ float unit_dout(const float* __restrict__ dl, const float* __restrict__ final_w,
                                           int b, int T, int U, int u) {
    float d = 0.f;
    for (int t = 0; t < T; ++t) d = fmaf(dl[(size_t)b * T + t], final_w[(size_t)t * U + u], d);
    return d;
}
