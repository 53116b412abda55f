// Motif comparison on the device ("Motif comparison"): for every (query, target) of
// two sets of position matrices the best ungapped alignment by width-normalised Pearson correlation
// (RSAT's Ncor), over offsets and both strands.  Stand-alone like pwm.hip and shuffle.hip: device pointers
// and a caller's workspace, no explainn_ctx, no allocation, no host sync.
//
// Two launches.
//   motif_prep_kernel, one lane per motif: per column f = (c + pc/4) / (sum c + pc) (0.25 where the
//     denominator is 0), d = f - 0.25 and n = |d|^2; the centred columns as float4 (zero from column w on),
//     the reverse-complement view rc[i] = (d[w-1-i] with A<->T, C<->G), and fp64 prefix sums of n in both
//     orders (entries past w repeat the total).  A width outside [0, wmax] becomes width 0.
//   motif_compare_kernel, one lane per (query, target): a workgroup stages 64 targets and MC_TQ queries
//     in LDS; lane = target, a wave walks its queries one after the other, so every query read is a
//     broadcast and every target read hits 64 different rows of one column -- rows are padded to an odd
//     number of 16-byte (8-byte for the prefix sums) slots, which makes those reads conflict-free.
//     Strand 1 is the query's reverse-complement view against the same target rows: q against rc(t) at
//     offset o is rc(q) against t at offset e = wt - wq - o, with the same overlap.
//     Four consecutive offsets share one pass over the query: a window of four target columns slides
//     through registers, so a step is 2 LDS reads and 16 FMAs, and the four running dot products are
//     named registers (no indexed private array).  Loop bounds are the wave's (the widest target of the
//     tile); a narrower target meets the zero columns that pad its row.  SX and SY of an alignment are
//     two subtractions of prefix sums, in fp64 because those do cancel; the dot product does not (centred
//     form), so it stays fp32.
// The order of evaluation is fixed -- strand 0 before strand 1, offsets ascending, a strictly larger Ncor
// replaces the best -- which is the tie rule and makes the result a pure function of the input.
#include "common.h"

namespace {

constexpr int MC_TT = 64;        // targets per workgroup = lanes of a wave
constexpr int MC_TQ = 8;         // queries per workgroup
constexpr int MC_WAVES = 4;
constexpr int MC_PAD = 3;        // zero columns in front of a target row (three more offsets ride along)

__host__ __device__ inline int mc_stride(int wmax) { return (wmax + 2 * MC_PAD + 1) | 1; }   // odd, >= wmax + 7
__host__ __device__ inline int mc_qp(int wmax) { return wmax + 2 * MC_PAD - 2; }             // prefix entries per query row
__host__ inline size_t mc_lds_bytes(int wmax) {
    const size_t S = mc_stride(wmax);
    return MC_TT * S * 16 + (size_t)MC_TQ * 2 * wmax * 16 + MC_TT * S * 8 + (size_t)MC_TQ * 2 * mc_qp(wmax) * 8;
}

// workspace: D [M][2][wmax] float4 | P [M][2][wmax+1] double | W [M] int32, each 256-byte aligned
struct mc_layout { int64_t d, p, w, bytes; };
__host__ inline mc_layout mc_workspace(int64_t M, int wmax) {
    auto up = [](int64_t v) { return (v + 255) & ~(int64_t)255; };
    mc_layout l;
    l.d = 0;
    l.p = up(M * 2 * wmax * 16);
    l.w = l.p + up(M * 2 * (wmax + 1) * 8);
    l.bytes = l.w + up(M * 4);
    return l;
}

__global__ __launch_bounds__(64) void motif_prep_kernel(const float* __restrict__ m, const int32_t* __restrict__ widths,
                                                        int M, int wmax, float pc, float4* __restrict__ D,
                                                        double* __restrict__ P, int32_t* __restrict__ W) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= M) return;
    int w = widths[i];
    if (w < 0 || w > wmax) w = 0;
    W[i] = w;
    const float* src = m + (size_t)i * wmax * 4;
    float4* d0 = D + (size_t)i * 2 * wmax;
    float4* d1 = d0 + wmax;
    double* p0 = P + (size_t)i * 2 * (wmax + 1);
    double* p1 = p0 + wmax + 1;
    const float quarter = pc * 0.25f;
    double run = 0.0;
    p0[0] = 0.0;
    for (int j = 0; j < wmax; ++j) {
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < w) {
            const float c0 = src[4 * j], c1 = src[4 * j + 1], c2 = src[4 * j + 2], c3 = src[4 * j + 3];
            const float den = ((c0 + c1) + c2) + c3 + pc;
            if (den != 0.f)
                d = make_float4((c0 + quarter) / den - 0.25f, (c1 + quarter) / den - 0.25f,
                                (c2 + quarter) / den - 0.25f, (c3 + quarter) / den - 0.25f);
            d1[w - 1 - j] = make_float4(d.w, d.z, d.y, d.x);
        } else {
            d1[j] = d;
        }
        d0[j] = d;
        run += (double)(((d.x * d.x + d.y * d.y) + d.z * d.z) + d.w * d.w);
        p0[j + 1] = run;
    }
    // the same n, summed from the other end (the thread reads back its own stores)
    run = 0.0;
    p1[0] = 0.0;
    for (int j = 0; j < wmax; ++j) {
        if (j < w) {
            const float4 d = d0[w - 1 - j];
            run += (double)(((d.x * d.x + d.y * d.y) + d.z * d.z) + d.w * d.w);
        }
        p1[j + 1] = run;
    }
}

__device__ __forceinline__ void mc_fma4(float4& acc, const float4 q, const float4 t) {
    acc.x = fmaf(q.x, t.x, acc.x);
    acc.y = fmaf(q.y, t.y, acc.y);
    acc.z = fmaf(q.z, t.z, acc.z);
    acc.w = fmaf(q.w, t.w, acc.w);
}

struct mc_best { float ncor, cor; int o, s, w, found; };

// one finished alignment of the lane's pair: strand s, query-view offset e, running dot product acc
__device__ __forceinline__ void mc_finish(mc_best& b, const float4 acc, int e, int s, int wq, int wt, int need,
                                          const double* __restrict__ qp, const double* __restrict__ tp) {
    const int lo = max(0, -e);
    const int hi = max(min(wq, wt - e), lo);
    const int w = hi - lo;
    const float sx = (float)(qp[hi] - qp[lo]);
    const float sy = (float)(tp[hi + e] - tp[lo + e]);
    const float xy = (acc.x + acc.z) + (acc.y + acc.w);
    const float cor = (sx < EXPLAINN_MOTIF_VAR_FLOOR || sy < EXPLAINN_MOTIF_VAR_FLOOR) ? 0.f : xy / sqrtf(sx * sy);
    const float ncor = cor * (float)w / (float)(wq + wt - w);
    if (w >= need && (!b.found || ncor > b.ncor)) {
        b.ncor = ncor; b.cor = cor; b.w = w; b.s = s; b.found = 1;
        b.o = s ? wt - wq - e : e;
    }
}

// offsets e0 .. e0+3 of one query view against the lane's target row (tr: column 0 of the row)
__device__ __forceinline__ void mc_group(float4& a0, float4& a1, float4& a2, float4& a3, const float4* __restrict__ qd,
                                         const float4* __restrict__ tr, int e0, int wq, int wtm) {
    a0 = a1 = a2 = a3 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int lo = max(0, -(e0 + 3)), hi = min(wq, wtm - e0);
    if (lo >= hi) return;
    const float4* tc = tr + lo + e0;
    // the window lives in a ring of four registers; four steps bring every column back to its register
    float4 r0 = tc[0], r1 = tc[1], r2 = tc[2], r3;
    int i = lo;
    for (; i + 4 <= hi; i += 4, tc += 4) {
        const float4 q0 = qd[i], q1 = qd[i + 1], q2 = qd[i + 2], q3 = qd[i + 3];
        r3 = tc[3];
        mc_fma4(a0, q0, r0); mc_fma4(a1, q0, r1); mc_fma4(a2, q0, r2); mc_fma4(a3, q0, r3);
        r0 = tc[4];
        mc_fma4(a0, q1, r1); mc_fma4(a1, q1, r2); mc_fma4(a2, q1, r3); mc_fma4(a3, q1, r0);
        r1 = tc[5];
        mc_fma4(a0, q2, r2); mc_fma4(a1, q2, r3); mc_fma4(a2, q2, r0); mc_fma4(a3, q2, r1);
        r2 = tc[6];
        mc_fma4(a0, q3, r3); mc_fma4(a1, q3, r0); mc_fma4(a2, q3, r1); mc_fma4(a3, q3, r2);
    }
    for (; i < hi; ++i, ++tc) {
        const float4 q = qd[i];
        r3 = tc[3];
        mc_fma4(a0, q, r0); mc_fma4(a1, q, r1); mc_fma4(a2, q, r2); mc_fma4(a3, q, r3);
        r0 = r1; r1 = r2; r2 = r3;
    }
}

__global__ __launch_bounds__(MC_WAVES * 64) void motif_compare_kernel(
    const float4* __restrict__ Dq, const double* __restrict__ Pq, const int32_t* __restrict__ Wq, int Q,
    const float4* __restrict__ Dt, const double* __restrict__ Pt, const int32_t* __restrict__ Wt, int T, int wmax,
    int ntt, int min_overlap, int both, float* __restrict__ ncor, float* __restrict__ cor,
    int16_t* __restrict__ align) {
    extern __shared__ float4 mc_sm[];
    const int S = mc_stride(wmax), QP = mc_qp(wmax);
    float4* tD = mc_sm;                                   // [64][S]      column j of target r at r*S + j + MC_PAD
    float4* qD = tD + MC_TT * S;                          // [TQ][2][wmax]
    double* tP = reinterpret_cast<double*>(qD + MC_TQ * 2 * wmax);   // [64][S]   prefix x at r*S + x
    double* qP = tP + MC_TT * S;                          // [TQ][2][QP]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = (blockIdx.x % ntt) * MC_TT, q0 = (blockIdx.x / ntt) * MC_TQ;

    for (int idx = tid; idx < MC_TT * S; idx += MC_WAVES * 64) {
        const int r = idx / S, c = idx - r * S, j = c - MC_PAD, t = t0 + r;
        const bool in = t < T;
        tD[idx] = (in && j >= 0 && j < wmax) ? Dt[(size_t)t * 2 * wmax + j] : make_float4(0.f, 0.f, 0.f, 0.f);
        tP[idx] = in ? Pt[(size_t)t * 2 * (wmax + 1) + min(c, wmax)] : 0.0;
    }
    for (int idx = tid; idx < MC_TQ * 2 * wmax; idx += MC_WAVES * 64) {
        const int q = q0 + idx / (2 * wmax);
        qD[idx] = q < Q ? Dq[(size_t)q0 * 2 * wmax + idx] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int idx = tid; idx < MC_TQ * 2 * QP; idx += MC_WAVES * 64) {
        const int row = idx / QP, x = idx - row * QP, q = q0 + (row >> 1);
        qP[idx] = q < Q ? Pq[((size_t)q0 * 2 + row) * (wmax + 1) + min(x, wmax)] : 0.0;
    }
    __syncthreads();

    const int t = t0 + lane;
    const int wt = t < T ? Wt[t] : 0;
    int wtm = wt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) wtm = max(wtm, __shfl_xor(wtm, off, 64));
    wtm = __builtin_amdgcn_readfirstlane(wtm);
    const float4* tr = tD + lane * S + MC_PAD;
    const double* tp = tP + lane * S;

    for (int qi = wave; qi < MC_TQ; qi += MC_WAVES) {
        const int q = q0 + qi;
        if (q >= Q) break;
        const int wq = __builtin_amdgcn_readfirstlane(Wq[q]);
        const int need = max(1, min(min_overlap, min(wq, wt)));
        mc_best b = {0.f, 0.f, 0, 0, 0, 0};
        if (wq > 0 && wtm > 0) {
            const int emin = -(wq - 1), emax = wtm - 1;
            float4 a0, a1, a2, a3;
            {   // strand 0: o = e ascending
                const float4* qd = qD + (qi * 2) * wmax;
                const double* qp = qP + (qi * 2) * QP;
                for (int e0 = emin; e0 <= emax; e0 += 4) {
                    mc_group(a0, a1, a2, a3, qd, tr, e0, wq, wtm);
                    mc_finish(b, a0, e0, 0, wq, wt, need, qp, tp);
                    mc_finish(b, a1, e0 + 1, 0, wq, wt, need, qp, tp);
                    mc_finish(b, a2, e0 + 2, 0, wq, wt, need, qp, tp);
                    mc_finish(b, a3, e0 + 3, 0, wq, wt, need, qp, tp);
                }
            }
            if (both) {   // strand 1: o = wt - wq - e ascending, so e descending
                const float4* qd = qD + (qi * 2 + 1) * wmax;
                const double* qp = qP + (qi * 2 + 1) * QP;
                for (int e0 = emax - 3; e0 + 3 >= emin; e0 -= 4) {
                    mc_group(a0, a1, a2, a3, qd, tr, e0, wq, wtm);
                    mc_finish(b, a3, e0 + 3, 1, wq, wt, need, qp, tp);
                    mc_finish(b, a2, e0 + 2, 1, wq, wt, need, qp, tp);
                    mc_finish(b, a1, e0 + 1, 1, wq, wt, need, qp, tp);
                    mc_finish(b, a0, e0, 1, wq, wt, need, qp, tp);
                }
            }
        }
        if (t < T) {
            const size_t at = (size_t)q * T + t;
            ncor[at] = b.ncor;
            if (cor) cor[at] = b.cor;
            if (align) {
                align[at * 3] = (int16_t)b.o;
                align[at * 3 + 1] = (int16_t)b.s;
                align[at * 3 + 2] = (int16_t)b.w;
            }
        }
    }
}

}  // namespace

extern "C" int64_t explainn_motif_compare_workspace_bytes(int Q, int T, int wmax) {
    if (Q < 0 || T < 0 || wmax < 1) return 0;
    return mc_workspace((int64_t)Q + T, wmax).bytes;
}

extern "C" int explainn_motif_compare(const float* q, const int32_t* q_widths, int Q, const float* t,
                                      const int32_t* t_widths, int T, int wmax, float pseudocount, int min_overlap,
                                      int both_strands, float* ncor, float* cor, int16_t* align, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
    if (Q < 0 || T < 0 || wmax < 1 || min_overlap < 1 || !(pseudocount >= 0.f)) {
        explainn_set_error("motif_compare: need Q, T >= 0, wmax >= 1, min_overlap >= 1, pseudocount >= 0 "
                           "(Q=%d T=%d wmax=%d min_overlap=%d pseudocount=%g)", Q, T, wmax, min_overlap,
                           (double)pseudocount);
        return EXPLAINN_E_ARG;
    }
    if (wmax > EXPLAINN_MOTIF_MAX_WIDTH) {
        explainn_set_error("motif_compare: wmax %d exceeds %d columns", wmax, EXPLAINN_MOTIF_MAX_WIDTH);
        return EXPLAINN_E_UNSUPPORTED;
    }
    if (!t && T != Q) {
        explainn_set_error("motif_compare: t == NULL compares the queries with themselves, T must equal Q (%d, %d)",
                           T, Q);
        return EXPLAINN_E_ARG;
    }
    if (Q == 0 || T == 0) return EXPLAINN_OK;
    if (!q || !q_widths || !ncor || (t && !t_widths)) {
        explainn_set_error("motif_compare: q, q_widths, ncor (and t_widths with t) must be device pointers");
        return EXPLAINN_E_ARG;
    }
    const int64_t M = (int64_t)Q + (t ? T : 0);
    const mc_layout l = mc_workspace(M, wmax);
    if (!workspace || ((uintptr_t)workspace & 15u) || workspace_bytes < l.bytes) {
        explainn_set_error("motif_compare: workspace of %lld bytes, 16-byte aligned, needed (%lld given)",
                           (long long)l.bytes, (long long)workspace_bytes);
        return EXPLAINN_E_ARG;
    }
    const int64_t ntt = ((int64_t)T + MC_TT - 1) / MC_TT, ntq = ((int64_t)Q + MC_TQ - 1) / MC_TQ;
    if (ntt * ntq > 0x7fffffffLL) {
        explainn_set_error("motif_compare: %d x %d pairs exceed one launch; split the queries", Q, T);
        return EXPLAINN_E_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    float4* D = reinterpret_cast<float4*>(ws + l.d);
    double* P = reinterpret_cast<double*>(ws + l.p);
    int32_t* W = reinterpret_cast<int32_t*>(ws + l.w);
    hipLaunchKernelGGL(motif_prep_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, s, q, q_widths, Q, wmax,
                       pseudocount, D, P, W);
    LAUNCH_CHECK();
    const float4* Dt = D;
    const double* Pt = P;
    const int32_t* Wt = W;
    if (t) {
        Dt = D + (size_t)Q * 2 * wmax;
        Pt = P + (size_t)Q * 2 * (wmax + 1);
        Wt = W + Q;
        hipLaunchKernelGGL(motif_prep_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, s, t, t_widths, T, wmax,
                           pseudocount, const_cast<float4*>(Dt), const_cast<double*>(Pt), const_cast<int32_t*>(Wt));
        LAUNCH_CHECK();
    }
    const size_t lds = mc_lds_bytes(wmax);
    if (lds > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&motif_compare_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mc_lds_bytes(EXPLAINN_MOTIF_MAX_WIDTH)));
    hipLaunchKernelGGL(motif_compare_kernel, dim3((unsigned)(ntt * ntq)), dim3(MC_WAVES * 64), lds, s, D, P, W, Q, Dt,
                       Pt, Wt, T, wmax, (int)ntt, min_overlap, both_strands != 0, ncor, cor, align);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
