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
//
// The second half of the file is motif significance (explainn_motif_significance): p-values of alignment
// scores under a per-query null, on the same preparation and conventions.
#include "common.h"
#include "workspace.h"

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
struct mc_pieces { float4* D; double* P; int32_t* W; };
__host__ inline void mc_workspace(Carver& cv, int64_t M, int wmax, mc_pieces* w) {
    cv.take(&w->D, M * 2 * wmax);
    cv.take(&w->P, M * 2 * (wmax + 1));
    cv.take(&w->W, M);
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
    Carver dry;
    mc_pieces w;
    mc_workspace(dry, (int64_t)Q + T, wmax, &w);
    return dry.bytes();
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
    Carver cv(workspace);
    mc_pieces w;
    mc_workspace(cv, M, wmax, &w);
    if (!workspace_ok("motif_compare", workspace, workspace_bytes, cv.bytes(), 16)) return EXPLAINN_E_ARG;
    const int64_t ntt = ((int64_t)T + MC_TT - 1) / MC_TT, ntq = ((int64_t)Q + MC_TQ - 1) / MC_TQ;
    if (ntt * ntq > 0x7fffffffLL) {
        explainn_set_error("motif_compare: %d x %d pairs exceed one launch; split the queries", Q, T);
        return EXPLAINN_E_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float4* D = w.D;
    double* P = w.P;
    int32_t* W = w.W;
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

// ---------------------------------------------------------------------------------------------------------
// Motif significance: p-values of the best alignment under the null of
// Gupta et al. 2007 -- the columns of the query against every column of the database, the score of an
// alignment the sum of quantised column correlations, its null the convolution of the per-column nulls.
//
// Five launches after the preparation of motif_prep_kernel (whose centred columns are turned into unit
// columns while they are staged):
//   motif_colscore_kernel, lane = target, 64 targets (forward columns, [column][lane] so a read is
//     conflict-free) and MS_TQ queries in LDS: the quantised score of every query column against every column
//     of both strand views of the lane's target, a byte each, into the workspace matrix
//     cs[(q*wmax + i)][(s*wmax + j)*Tp + t] (Tp = T rounded up to 16; MS_NONE where the target column does
//     not exist; rows i >= wq are not written).  The reverse-complement view needs no second copy: column j
//     of rc(t) is column wt-1-j with its four entries reversed.
//   motif_hist_kernel, one workgroup per query column: the histogram of its row, integer LDS atomics into one
//     histogram per wave, summed in a fixed order.
//   motif_null_kernel, one workgroup per (query, lo): the pmf of the sum over columns lo .. lo+w-1 for
//     w = 1 .. wq-lo, each from the one before by one convolution (thread = support point, bins ascending,
//     fused multiply-adds, fp64), two pmf buffers in LDS; after every w the suffix sums -- each thread sums a
//     contiguous piece from the top, adds the pieces above it in descending order -- go to the workspace table.
//   motif_pvalue_kernel, one lane per (query, target): strand 0 before strand 1, offsets ascending, the sum of
//     the bytes of the overlap, the table look-up, a strictly smaller p replaces the best; then the Sidak
//     step over the pair's admissible alignments.
//   motif_colscore_copy_kernel: the caller's copy of the matrix without the row padding (only when asked for).
// No float atomics anywhere and every sum in a fixed order: the result is a pure function of the input.
namespace {

constexpr int MS_TT = 64;        // targets per workgroup = lanes of a wave
constexpr int MS_TQ = 8;         // queries per workgroup of the column scores
constexpr int MS_WAVES = 4;
constexpr int MS_THREADS = MS_WAVES * 64;
constexpr int MS_HPAD = 136;     // histogram row in LDS (bins + 1 <= 129)

__host__ __device__ inline int64_t ms_a(int64_t n, int bins) { return bins * (n * (n + 1) / 2) + n; }
__host__ __device__ inline int64_t ms_c(int64_t n, int bins) {
    return bins * (n * (n + 1) * (n + 2) / 6) + n * (n + 1) / 2;
}
// the suffix sums of range (lo, w) of one query: ranges ordered by lo, then by w; range (lo, w) holds w*bins+1
__host__ __device__ inline int64_t ms_sf_off(int lo, int w, int wmax, int bins) {
    return ms_c(wmax, bins) - ms_c(wmax - lo, bins) + ms_a(w - 1, bins);
}
__host__ __device__ inline int ms_tp(int T) { return (T + 15) & ~15; }

// workspace: the preparation's (mc_workspace) | cs [Q*wmax][ld] uint8 | hist [Q*wmax][bins+1] int32 |
// sf [Q][sfq] double, each 256-byte aligned
__host__ inline int64_t ms_ld(int T, int wmax, int S) { return (int64_t)S * wmax * ms_tp(T); }   // a row of cs
struct ms_pieces { mc_pieces prep; uint8_t* cs; int32_t* hist; double* sf; };
__host__ inline void ms_workspace(Carver& cv, int64_t Q, int64_t M, int T, int wmax, int bins, int S, ms_pieces* w) {
    mc_workspace(cv, M, wmax, &w->prep);
    cv.take(&w->cs, Q * wmax * ms_ld(T, wmax, S));
    cv.take(&w->hist, Q * wmax * (bins + 1));
    cv.take(&w->sf, Q * ms_c(wmax, bins));
}
__host__ inline size_t ms_colscore_lds(int wmax) { return (size_t)(MS_TT + MS_TQ) * wmax * 16; }
__host__ inline size_t ms_null_lds(int wmax, int bins) {
    return (size_t)(2 * (wmax * bins + 1) + MS_HPAD + MS_THREADS) * 8;
}

// a centred column as a unit vector; the norm in fp64, zero below the variance floor
__device__ __forceinline__ float4 ms_unit(const float4 d) {
    const double x = d.x, y = d.y, z = d.z, w = d.w;
    const double n = ((x * x + y * y) + z * z) + w * w;
    if (n < (double)EXPLAINN_MOTIF_VAR_FLOOR) return make_float4(0.f, 0.f, 0.f, 0.f);
    const double r = 1.0 / sqrt(n);
    return make_float4((float)(x * r), (float)(y * r), (float)(z * r), (float)(w * r));
}

// the quantised correlation of two unit columns: every operation named, so no contraction can differ
__device__ __forceinline__ int ms_bin(const float4 q, const float4 t, float half_bins, int bins) {
    const float c = fmaf(q.w, t.w, fmaf(q.z, t.z, fmaf(q.y, t.y, __fmul_rn(q.x, t.x))));
    const float x = floorf(fmaf(__fadd_rn(c, 1.0f), half_bins, 0.5f));
    return min(max((int)x, 0), bins);
}

__global__ __launch_bounds__(MS_THREADS) void motif_colscore_kernel(
    const float4* __restrict__ Dq, const int32_t* __restrict__ Wq, int Q, const float4* __restrict__ Dt,
    const int32_t* __restrict__ Wt, int T, int wmax, int ntt, int both, int bins, uint8_t* __restrict__ cs,
    int64_t ld) {
    extern __shared__ float4 ms_sm[];
    float4* tU = ms_sm;                     // [wmax][64]   column j of target r at j*64 + r
    float4* qU = tU + wmax * MS_TT;         // [TQ][wmax]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = (blockIdx.x % ntt) * MS_TT, q0 = (blockIdx.x / ntt) * MS_TQ;
    const int Tp = ms_tp(T);
    for (int idx = tid; idx < wmax * MS_TT; idx += MS_THREADS) {
        const int r = idx & 63, j = idx >> 6, t = t0 + r;
        tU[idx] = t < T ? ms_unit(Dt[(size_t)t * 2 * wmax + j]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int idx = tid; idx < MS_TQ * wmax; idx += MS_THREADS) {
        const int q = q0 + idx / wmax;
        qU[idx] = q < Q ? ms_unit(Dq[(size_t)q * 2 * wmax + idx % wmax]) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int t = t0 + lane;
    const int wt = t < T ? Wt[t] : 0;
    const bool stored = t < Tp;             // the padding lanes of a row carry MS_NONE, lanes past it nothing
    const float half_bins = 0.5f * (float)bins;
    for (int qi = wave; qi < MS_TQ; qi += MS_WAVES) {
        const int q = q0 + qi;
        if (q >= Q) break;
        const int wq = __builtin_amdgcn_readfirstlane(Wq[q]);
        for (int i = 0; i < wq; ++i) {
            const float4 qv = qU[qi * wmax + i];
            uint8_t* row = cs + ((size_t)q * wmax + i) * ld + t;
            for (int j = 0; j < wmax; ++j) {
                int b0 = EXPLAINN_MOTIF_NO_SCORE, b1 = EXPLAINN_MOTIF_NO_SCORE;
                if (j < wt) {
                    b0 = ms_bin(qv, tU[j * MS_TT + lane], half_bins, bins);
                    if (both) {
                        const float4 r = tU[(wt - 1 - j) * MS_TT + lane];
                        b1 = ms_bin(qv, make_float4(r.w, r.z, r.y, r.x), half_bins, bins);
                    }
                }
                if (stored) {
                    row[(size_t)j * Tp] = (uint8_t)b0;
                    if (both) row[(size_t)(wmax + j) * Tp] = (uint8_t)b1;
                }
            }
        }
    }
}

__global__ __launch_bounds__(MS_THREADS) void motif_hist_kernel(const uint8_t* __restrict__ cs, int64_t ld,
                                                                const int32_t* __restrict__ Wq, int wmax, int bins,
                                                                int32_t* __restrict__ hist,
                                                                int32_t* __restrict__ hist_out) {
    __shared__ int h[MS_WAVES][MS_HPAD];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int row = blockIdx.x, q = row / wmax, i = row - q * wmax;
    const int nb = bins + 1;
    for (int b = tid; b < MS_WAVES * MS_HPAD; b += MS_THREADS) (&h[0][0])[b] = 0;
    __syncthreads();
    if (i < Wq[q]) {                        // uniform over the workgroup
        const uint4* p = reinterpret_cast<const uint4*>(cs + (size_t)row * ld);   // ld is a multiple of 16
        const int64_t n16 = ld / 16;
        for (int64_t k = tid; k < n16; k += MS_THREADS) {
            const uint4 v = p[k];
            const unsigned int w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int b = (w4[a] >> (8 * m)) & 255;
                    if (b <= bins) atomicAdd(&h[wave][b], 1);
                }
        }
    }
    __syncthreads();
    for (int b = tid; b < nb; b += MS_THREADS) {
        const int total = (h[0][b] + h[1][b]) + (h[2][b] + h[3][b]);
        hist[(size_t)row * nb + b] = total;
        if (hist_out) hist_out[(size_t)row * nb + b] = total;
    }
}

__global__ __launch_bounds__(MS_THREADS) void motif_null_kernel(const int32_t* __restrict__ hist,
                                                                const int32_t* __restrict__ Wq, int wmax, int bins,
                                                                double* __restrict__ sf, int64_t sfq) {
    extern __shared__ double ms_dm[];
    const int L = wmax * bins + 1;
    double* cur = ms_dm;                    // the pmf of the current width
    double* nxt = cur + L;                  // the next one; between convolutions the suffix sums on their way out
    double* hd = nxt + L;                   // [MS_HPAD] the null of the column being added
    double* part = hd + MS_HPAD;            // [MS_THREADS]
    const int tid = threadIdx.x;
    const int q = blockIdx.x / wmax, lo = blockIdx.x - q * wmax;
    const int wq = Wq[q];
    if (lo >= wq) return;                   // uniform over the workgroup
    const int nb = bins + 1;
    const int32_t* hrow = hist + ((size_t)q * wmax + lo) * nb;
    int64_t cnt = 0;                        // N: every row of the query's histogram sums to it
    for (int b = 0; b < nb; ++b) cnt += hrow[b];
    if (cnt == 0) return;                   // an empty database: nothing is looked up
    const double N = (double)cnt;
    for (int b = tid; b < nb; b += MS_THREADS) cur[b] = (double)hrow[b] / N;
    __syncthreads();
    double* out = sf + (size_t)q * sfq;
    for (int w = 1;; ++w) {
        const int n = w * bins + 1;
        {   // suffix sums of cur[0..n) into nxt, then out
            const int seg = (n + MS_THREADS - 1) / MS_THREADS;
            const int a = min(n, tid * seg), e = min(n, a + seg);
            double local = 0.0;
            for (int s = e - 1; s >= a; --s) local += cur[s];
            part[tid] = local;
            __syncthreads();
            double run = 0.0;
            for (int k = MS_THREADS - 1; k > tid; --k) run += part[k];
            for (int s = e - 1; s >= a; --s) {
                run += cur[s];
                nxt[s] = fmin(run, 1.0);
            }
            __syncthreads();
            double* dst = out + ms_sf_off(lo, w, wmax, bins);
            for (int s = tid; s < n; s += MS_THREADS) dst[s] = nxt[s];
        }
        if (lo + w >= wq) break;
        const int32_t* hnext = hist + ((size_t)q * wmax + lo + w) * nb;
        for (int b = tid; b < nb; b += MS_THREADS) hd[b] = (double)hnext[b] / N;
        __syncthreads();                    // hd is complete, nxt has been copied out
        const int n2 = n + bins;
        for (int s = tid; s < n2; s += MS_THREADS) {
            double acc = 0.0;
            for (int b = 0; b < nb; ++b) {
                const double hb = hd[b];
                if (hb == 0.0) continue;    // uniform: an empty bin adds an exact zero
                const int k = s - b;
                if (k >= 0 && k < n) acc = fma(cur[k], hb, acc);
            }
            nxt[s] = acc;
        }
        __syncthreads();
        double* swap = cur; cur = nxt; nxt = swap;
    }
}

__global__ __launch_bounds__(MS_THREADS) void motif_pvalue_kernel(
    const uint8_t* __restrict__ cs, int64_t ld, const double* __restrict__ sf, int64_t sfq,
    const int32_t* __restrict__ Wq, int Q, const int32_t* __restrict__ Wt, int T, int wmax, int ntt, int min_overlap,
    int S, int bins, double* __restrict__ pvalue, int16_t* __restrict__ align, int32_t* __restrict__ score) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = (blockIdx.x % ntt) * MS_TT + lane;
    const int q = (blockIdx.x / ntt) * MS_WAVES + wave;
    if (q >= Q || t >= T) return;
    const int Tp = ms_tp(T);
    const int wq = __builtin_amdgcn_readfirstlane(Wq[q]);
    const int wt = Wt[t];
    double best = 2.0;
    int bo = 0, bs = 0, bw = 0, bsum = 0, n_align = 0;
    if (wq > 0 && wt > 0) {
        const int need = max(1, min(min_overlap, min(wq, wt)));
        const uint8_t* base = cs + (size_t)q * wmax * ld + t;
        const double* tab = sf + (size_t)q * sfq;
        for (int s = 0; s < S; ++s)
            for (int o = -(wq - 1); o < wt; ++o) {
                const int lo = max(0, -o), hi = min(wq, wt - o), w = hi - lo;
                if (w < need) continue;
                const uint8_t* p = base + (size_t)lo * ld + (size_t)(s * wmax + lo + o) * Tp;
                int sum = 0;
                for (int i = lo; i < hi; ++i, p += ld + Tp) sum += *p;
                const double pa = tab[ms_sf_off(lo, w, wmax, bins) + sum];
                ++n_align;
                if (pa < best) { best = pa; bo = o; bs = s; bw = w; bsum = sum; }
            }
    }
    const size_t at = (size_t)q * T + t;
    pvalue[at] = (n_align == 0 || best >= 1.0) ? 1.0 : -expm1((double)n_align * log1p(-best));
    if (align) {
        align[at * 3] = (int16_t)bo;
        align[at * 3 + 1] = (int16_t)bs;
        align[at * 3 + 2] = (int16_t)bw;
    }
    if (score) score[at] = bsum;
}

__global__ __launch_bounds__(MS_THREADS) void motif_colscore_copy_kernel(const uint8_t* __restrict__ cs, int64_t ld,
                                                                         const int32_t* __restrict__ Wq, int T,
                                                                         int wmax, int S, int64_t total,
                                                                         uint8_t* __restrict__ out) {
    const int Tp = ms_tp(T);
    const int64_t cols = (int64_t)S * wmax * T;
    for (int64_t idx = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * MS_THREADS) {
        const int64_t row = idx / cols, c = idx - row * cols;
        const int64_t sj = c / T, t = c - sj * T;
        const int q = (int)(row / wmax), i = (int)(row - (int64_t)q * wmax);
        out[idx] = i < Wq[q] ? cs[row * ld + sj * Tp + t] : (uint8_t)EXPLAINN_MOTIF_NO_SCORE;
    }
}

}  // namespace

extern "C" int64_t explainn_motif_significance_workspace_bytes(int Q, int T, int wmax, int bins, int both_strands) {
    if (Q < 0 || T < 0 || wmax < 1 || wmax > EXPLAINN_MOTIF_MAX_WIDTH || bins < 2 || bins > EXPLAINN_MOTIF_MAX_BINS)
        return 0;
    Carver dry;
    ms_pieces w;
    ms_workspace(dry, Q, (int64_t)Q + T, T, wmax, bins, both_strands ? 2 : 1, &w);
    return dry.bytes();
}

extern "C" int explainn_motif_significance(const float* q, const int32_t* q_widths, int Q, const float* t,
                                           const int32_t* t_widths, int T, int wmax, float pseudocount,
                                           int min_overlap, int both_strands, int bins, double* pvalue,
                                           int16_t* align, int32_t* score, uint8_t* colscore, int32_t* hist,
                                           void* workspace, int64_t workspace_bytes, void* stream) {
    if (Q < 0 || T < 0 || wmax < 1 || min_overlap < 1 || !(pseudocount >= 0.f) || bins < 2 ||
        bins > EXPLAINN_MOTIF_MAX_BINS) {
        explainn_set_error("motif_significance: need Q, T >= 0, wmax >= 1, min_overlap >= 1, pseudocount >= 0, "
                           "2 <= bins <= %d (Q=%d T=%d wmax=%d min_overlap=%d pseudocount=%g bins=%d)",
                           EXPLAINN_MOTIF_MAX_BINS, Q, T, wmax, min_overlap, (double)pseudocount, bins);
        return EXPLAINN_E_ARG;
    }
    if (wmax > EXPLAINN_MOTIF_MAX_WIDTH) {
        explainn_set_error("motif_significance: wmax %d exceeds %d columns", wmax, EXPLAINN_MOTIF_MAX_WIDTH);
        return EXPLAINN_E_UNSUPPORTED;
    }
    if (!t && T != Q) {
        explainn_set_error("motif_significance: t == NULL takes the queries as the database, T must equal Q (%d, %d)",
                           T, Q);
        return EXPLAINN_E_ARG;
    }
    if (Q == 0 || T == 0) return EXPLAINN_OK;
    if (!q || !q_widths || !pvalue || (t && !t_widths)) {
        explainn_set_error("motif_significance: q, q_widths, pvalue (and t_widths with t) must be device pointers");
        return EXPLAINN_E_ARG;
    }
    const int S = both_strands ? 2 : 1;
    const int64_t M = (int64_t)Q + (t ? T : 0);
    const int64_t ld = ms_ld(T, wmax, S), sfq = ms_c(wmax, bins);
    Carver cv(workspace);
    ms_pieces w;
    ms_workspace(cv, Q, M, T, wmax, bins, S, &w);
    if (!workspace_ok("motif_significance", workspace, workspace_bytes, cv.bytes(), 16)) return EXPLAINN_E_ARG;
    const int64_t ntt = ((int64_t)T + MS_TT - 1) / MS_TT, ntq = ((int64_t)Q + MS_TQ - 1) / MS_TQ;
    const int64_t ntw = ((int64_t)Q + MS_WAVES - 1) / MS_WAVES;
    if (ntt * ntq > 0x7fffffffLL || ntt * ntw > 0x7fffffffLL || (int64_t)Q * wmax > 0x7fffffffLL) {
        explainn_set_error("motif_significance: %d x %d pairs exceed one launch; split the queries", Q, T);
        return EXPLAINN_E_UNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float4* D = w.prep.D;
    double* P = w.prep.P;
    int32_t* W = w.prep.W;
    uint8_t* cs = w.cs;
    int32_t* hs = w.hist;
    double* sf = w.sf;
    hipLaunchKernelGGL(motif_prep_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, s, q, q_widths, Q, wmax,
                       pseudocount, D, P, W);
    LAUNCH_CHECK();
    const float4* Dt = D;
    const int32_t* Wt = W;
    if (t) {
        Dt = D + (size_t)Q * 2 * wmax;
        Wt = W + Q;
        hipLaunchKernelGGL(motif_prep_kernel, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, s, t, t_widths, T, wmax,
                           pseudocount, const_cast<float4*>(Dt), P + (size_t)Q * 2 * (wmax + 1),
                           const_cast<int32_t*>(Wt));
        LAUNCH_CHECK();
    }
    const size_t lds1 = ms_colscore_lds(wmax), lds3 = ms_null_lds(wmax, bins);
    if (lds1 > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&motif_colscore_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)ms_colscore_lds(EXPLAINN_MOTIF_MAX_WIDTH)));
    if (lds3 > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&motif_null_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)ms_null_lds(EXPLAINN_MOTIF_MAX_WIDTH, EXPLAINN_MOTIF_MAX_BINS)));
    hipLaunchKernelGGL(motif_colscore_kernel, dim3((unsigned)(ntt * ntq)), dim3(MS_THREADS), lds1, s, D, W, Q, Dt, Wt,
                       T, wmax, (int)ntt, both_strands != 0, bins, cs, ld);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(motif_hist_kernel, dim3((unsigned)(Q * wmax)), dim3(MS_THREADS), 0, s, cs, ld, W, wmax, bins,
                       hs, hist);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(motif_null_kernel, dim3((unsigned)(Q * wmax)), dim3(MS_THREADS), lds3, s, hs, W, wmax, bins, sf,
                       sfq);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(motif_pvalue_kernel, dim3((unsigned)(ntt * ntw)), dim3(MS_THREADS), 0, s, cs, ld, sf, sfq, W,
                       Q, Wt, T, wmax, (int)ntt, min_overlap, S, bins, pvalue, align, score);
    LAUNCH_CHECK();
    if (colscore) {
        const int64_t total = (int64_t)Q * wmax * S * wmax * T;
        const int64_t blocks = (total + MS_THREADS - 1) / MS_THREADS;
        hipLaunchKernelGGL(motif_colscore_copy_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)),
                           dim3(MS_THREADS), 0, s, cs, ld, W, T, wmax, S, total, colscore);
        LAUNCH_CHECK();
    }
    return EXPLAINN_OK;
}
