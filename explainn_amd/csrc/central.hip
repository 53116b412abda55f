// Motif centrality (DESIGN.md section 3 item 19, section 8 "Centrality"): where in the records the best
// sites of every unit sit, and CentriMo's test of a region that holds more of them than its width explains.
//
// site_positions_kernel: block = (unit, slice of records).  The records are dealt to the slices in chunks of
// CP_T; a thread takes one record, reads its label, its best site and the float16 activation there, and for
// every threshold the activation exceeds (the comparison of sites_kernel: the float16 value, as a float,
// > the float threshold) counts the start into a [T][2][M] LDS histogram with integer atomics.  A site below
// 0 or a start outside [0, M) is checked before it is counted.  One flush per block adds the non-zero bins
// into hist with 32-bit integer global atomics; the blocks of unit 0 also count the labels.  Integers
// throughout: the result does not depend on the geometry.
//
// centrality_test_kernel: a workgroup loops over units.  It turns the unit's primary rows into inclusive
// prefix sums in LDS (a wave per row, a wave scan per 64 bins), so that the sites of any region are one
// difference; then every lane takes (threshold, region) pairs, strided, and evaluates the binomial tail of
// the enriched ones in fp64 -- ln p is computed by one lane from (n, c, w, M) alone -- and the best pair is a
// min over (ln p, width, lo, threshold) keys: nothing depends on the order in which anything arrives.  The
// control rows are summed at the chosen threshold and region by the whole workgroup.
#include <hip/hip_fp16.h>

#include "common.h"
#include "tails.h"

namespace {

constexpr int CP_T = 256;
constexpr int CP_SLICE_BLOCKS = 2048;          // few units: the records are split until a call has about this many blocks
constexpr int CP_MAX_SLICES = 64;
constexpr int CP_MAX_T = EXPLAINN_CENTRALITY_MAX_THRESHOLDS;

__global__ __launch_bounds__(CP_T) void site_positions_kernel(
    const uint16_t* __restrict__ bits, const int32_t* __restrict__ site, const uint8_t* __restrict__ labels,
    const float* __restrict__ thr, int n_records, int T, int M, int* __restrict__ hist,
    unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned cp_sm[];        // bins [T][2][M] | thresholds [CP_MAX_T] | label counts [2]
    const int nb = T * 2 * M, tid = threadIdx.x, u = blockIdx.x;
    float* th = reinterpret_cast<float*>(cp_sm + nb);
    unsigned* cnt = cp_sm + nb + CP_MAX_T;
    for (int b = tid; b < nb; b += CP_T) cp_sm[b] = 0u;
    if (tid < T) th[tid] = thr[(size_t)u * T + tid];
    if (tid < 2) cnt[tid] = 0u;
    __syncthreads();
    const uint16_t* bcol = bits + (size_t)u * n_records;
    const int32_t* scol = site + (size_t)u * n_records;
    unsigned mine[2] = {0u, 0u};
    for (long long r = (long long)blockIdx.y * CP_T + tid; r < n_records; r += (long long)gridDim.y * CP_T) {
        const unsigned lab = labels[r];
        if (lab > 1u) continue;                // left out of both sets
        const int set = lab ? 0 : 1;
        ++mine[set];
        const int sv = scol[r];
        const int start = sv >> 1;
        if (sv < 0 || start >= M) continue;    // no site, or a start no record of this length has
        const float a = __half2float(__ushort_as_half((unsigned short)(bcol[r] & 0x7FFFu)));
        unsigned* h = cp_sm + set * M + start;
        for (int t = 0; t < T; ++t)
            if (a > th[t]) atomicAdd(h + (size_t)t * 2 * M, 1u);
    }
    if (u == 0) {
        if (mine[0]) atomicAdd(&cnt[0], mine[0]);
        if (mine[1]) atomicAdd(&cnt[1], mine[1]);
    }
    __syncthreads();
    int* row = hist + (size_t)u * nb;
    for (int b = tid; b < nb; b += CP_T) {
        const unsigned v = cp_sm[b];
        if (v) atomicAdd(&row[b], (int)v);
    }
    if (u == 0 && tid < 2 && cnt[tid]) atomicAdd(&counts[tid], (unsigned long long)cnt[tid]);
}

size_t site_positions_lds(int T, int M) { return ((size_t)T * 2 * M + CP_MAX_T + 2) * sizeof(unsigned); }

// ------------------------------------------------------------------------------------------- the test
constexpr int CT_T = 512;                      // 8 waves: the fp64 lgamma chain gets 256 registers a lane (as EN_T)
constexpr int CT_WAVES = CT_T / 64;
constexpr int CT_MAX_GRID = 256;               // workgroups of a call at the most

// ln P[X >= c], X ~ Binomial(n, w / M), for an enriched region (c M > n w, so c >= 1 and the terms fall from
// the first one on): the first term from binom_logpmf's three lgammas, the following ones from the ratio
// (n - x) / (x + 1) * q / (1 - q) of neighbouring terms, summed (relative to the first) until x reaches n or
// a term no longer changes the sum
__device__ __noinline__ double binom_logsf(long long n, long long c, int w, int M) {
    const double q = (double)w / (double)M;
    const double first = binom_logpmf((double)n, (double)c, log(q), log1p(-q));
    const double odds = q / (1.0 - q);
    double sum = 1.0, term = 1.0;
    for (long long x = c; x < n; ++x) {
        term *= ((double)(n - x) / (double)(x + 1)) * odds;
        const double s = sum + term;
        if (s == sum) break;
        sum = s;
    }
    return fmin(0.0, first + log(sum));
}

// the smaller ln p; among equal values the narrower region, then the lower lo, then the lower threshold
__device__ __forceinline__ bool ct_better(double lp, int w, int lo, int t, double lq, int wq, int loq, int tq) {
    if (lp != lq) return lp < lq;
    if (w != wq) return w < wq;
    if (lo != loq) return lo < loq;
    return t < tq;
}

// mode 0: `items` regions [j, M-1-j], j = j0 .. j0 + items - 1.  mode 1: `items` = (w1 - w0 + 1) M pairs
// (width, lo), of which those with lo + width <= M are regions.
__global__ __launch_bounds__(CT_T) void centrality_test_kernel(
    const int* __restrict__ hist, const long long* __restrict__ counts, int units, int T, int M, int mode,
    int j0, int w0, long long items, long long regions, long long min_sites, int32_t* __restrict__ best_t,
    int32_t* __restrict__ best_lo, int32_t* __restrict__ best_width, long long* __restrict__ sites,
    long long* __restrict__ count, long long* __restrict__ n_tests, double* __restrict__ log_pvalue,
    double* __restrict__ log_padj, long long* __restrict__ ctrl_sites, long long* __restrict__ ctrl_count,
    double* __restrict__ log_fisher) {
    extern __shared__ unsigned ct_sm[];        // prefix sums of the primary rows [T][M]
    __shared__ double red_lp[CT_WAVES];
    __shared__ long long red_a[CT_WAVES], red_b[CT_WAVES];
    __shared__ int red_w[CT_WAVES], red_lo[CT_WAVES], red_t[CT_WAVES], sel[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        const int* rows = hist + (size_t)u * T * 2 * M;
        __syncthreads();                       // the last unit's evaluation has read the prefix sums
        for (int t = wave; t < T; t += CT_WAVES) {
            const int* row = rows + (size_t)t * 2 * M;
            unsigned* pre = ct_sm + (size_t)t * M;
            unsigned running = 0;
            for (int b0 = 0; b0 < M; b0 += 64) {
                const int b = b0 + lane;
                const unsigned inc = wave_scan_up(b < M ? (unsigned)row[b] : 0u, lane);
                if (b < M) pre[b] = running + inc;
                running += __shfl(inc, 63, 64);
            }
        }
        __syncthreads();
        const long long need = min_sites > 1 ? min_sites : 1;
        double lp = 0.0;
        int bw = 0, blo = 0, bt = 0;           // bw == 0: this lane has met no (threshold, region) yet
        for (int t = 0; t < T; ++t) {
            const unsigned* pre = ct_sm + (size_t)t * M;
            const long long n = pre[M - 1];
            if (n < need) continue;            // not tried (the same for every lane)
            for (long long e = tid; e < items; e += CT_T) {
                int lo, w;
                if (mode == 0) {
                    lo = j0 + (int)e;
                    w = M - 2 * lo;
                } else {
                    w = w0 + (int)(e / M);
                    lo = (int)(e % M);
                    if (lo + w > M) continue;
                }
                const long long c = (long long)pre[lo + w - 1] - (lo ? (long long)pre[lo - 1] : 0ll);
                const double v = c * M > n * w ? binom_logsf(n, c, w, M) : 0.0;
                if (bw == 0 || ct_better(v, w, lo, t, lp, bw, blo, bt)) { lp = v; bw = w; blo = lo; bt = t; }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double lq = __shfl_xor(lp, o, 64);
            const int wq = __shfl_xor(bw, o, 64), loq = __shfl_xor(blo, o, 64), tq = __shfl_xor(bt, o, 64);
            if (wq > 0 && (bw == 0 || ct_better(lq, wq, loq, tq, lp, bw, blo, bt))) { lp = lq; bw = wq; blo = loq; bt = tq; }
        }
        if (lane == 0) { red_lp[wave] = lp; red_w[wave] = bw; red_lo[wave] = blo; red_t[wave] = bt; }
        __syncthreads();
        if (tid == 0) {
            lp = 0.0; bw = 0; blo = 0; bt = 0;
            for (int w = 0; w < CT_WAVES; ++w)
                if (red_w[w] > 0 && (bw == 0 || ct_better(red_lp[w], red_w[w], red_lo[w], red_t[w], lp, bw, blo, bt))) {
                    lp = red_lp[w]; bw = red_w[w]; blo = red_lo[w]; bt = red_t[w];
                }
            red_lp[0] = lp; sel[0] = bw; sel[1] = blo; sel[2] = bt;
        }
        __syncthreads();
        bw = sel[0]; blo = sel[1]; bt = sel[2];
        // the control row at the chosen threshold: all of it, and the region's part
        long long ca = 0, cb = 0;
        if (bw > 0) {
            const int* crow = rows + ((size_t)bt * 2 + 1) * M;
            for (int b = tid; b < M; b += CT_T) {
                const long long v = crow[b];
                ca += v;
                cb += b >= blo && b < blo + bw ? v : 0;
            }
        }
        ca = wave_sum(ca);
        cb = wave_sum(cb);
        if (lane == 0) { red_a[wave] = ca; red_b[wave] = cb; }
        __syncthreads();
        if (tid == 0) {
            lp = red_lp[0];
            ca = 0; cb = 0;
            for (int w = 0; w < CT_WAVES; ++w) { ca += red_a[w]; cb += red_b[w]; }
            long long tried = 0, n = 0, c = 0;
            for (int t = 0; t < T; ++t) tried += (long long)ct_sm[(size_t)t * M + M - 1] >= need ? 1 : 0;
            if (bw > 0) {
                const unsigned* pre = ct_sm + (size_t)bt * M;
                n = pre[M - 1];
                c = (long long)pre[blo + bw - 1] - (blo ? (long long)pre[blo - 1] : 0ll);
            }
            const long long m = bw > 0 ? tried * regions : 0;
            double padj = 0.0;
            if (m > 0) {
                if (lp < -30.0) padj = fmin(0.0, log((double)m) + lp);
                else padj = fmin(0.0, log(-expm1((double)m * log1p(-exp(lp)))));
            }
            const long long Np = counts[0], Nc = counts[1];
            double lf = 0.0;
            // counts that do not belong to hist (c > Np, cb > Nc) have no 2 x 2 table: no test
            if (bw > 0 && Nc > 0 && c <= Np && cb <= Nc && c * Nc > cb * Np) lf = hypergeom_logsf(c, c + cb, Np, Nc);
            best_t[u] = bt;
            best_lo[u] = blo;
            best_width[u] = bw;
            sites[u] = n;
            count[u] = c;
            n_tests[u] = m;
            log_pvalue[u] = lp;
            log_padj[u] = padj;
            ctrl_sites[u] = ca;
            ctrl_count[u] = cb;
            log_fisher[u] = lf;
        }
    }
}

}  // namespace

int launch_site_positions(const uint16_t* best_bits, const int32_t* best_site, const uint8_t* labels,
                          const float* thresholds, int units, int64_t n_records, int T, int M, int32_t* hist,
                          int64_t* counts, hipStream_t s) {
    const size_t sm = site_positions_lds(T, M);
    if (sm > 64 * 1024)                        // the bins alone may fill 64 KiB
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&site_positions_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    const long long chunks = (n_records + CP_T - 1) / CP_T;
    const int slices = (int)std::min<long long>(std::min<long long>(CP_MAX_SLICES, chunks),
                                                std::max<long long>(1, CP_SLICE_BLOCKS / units));
    hipLaunchKernelGGL(site_positions_kernel, dim3(units, slices), dim3(CP_T), sm, s, best_bits, best_site, labels,
                       thresholds, (int)n_records, T, M, hist, reinterpret_cast<unsigned long long*>(counts));
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

int64_t centrality_regions(int M, int mode, int min_width, int max_width, int* j0, int* w0, int64_t* items) {
    const int wlo = std::max(min_width, 1), whi = std::min(max_width, M - 1);
    *j0 = 0; *w0 = wlo; *items = 0;
    if (wlo > whi) return 0;
    if (mode == 0) {
        // w = M - 2j: wlo <= w <= whi
        const int jlo = (M - whi + 1) / 2, jhi = (M - wlo) / 2;
        *j0 = jlo;
        *items = jhi >= jlo ? jhi - jlo + 1 : 0;
        return *items;
    }
    const int64_t nw = whi - wlo + 1;
    *items = nw * M;
    // sum over w of (M - w + 1)
    return nw * (M + 1) - (int64_t)(wlo + whi) * nw / 2;
}

int launch_centrality_test(const int32_t* hist, const int64_t* counts, int units, int T, int M, int mode, int j0,
                           int w0, int64_t items, int64_t regions, int64_t min_sites, int32_t* best_t,
                           int32_t* best_lo, int32_t* best_width, int64_t* sites, int64_t* count, int64_t* n_tests,
                           double* log_pvalue, double* log_padj, int64_t* ctrl_sites, int64_t* ctrl_count,
                           double* log_fisher, hipStream_t s) {
    const size_t sm = (size_t)T * M * sizeof(unsigned);
    hipLaunchKernelGGL(centrality_test_kernel, dim3(units < CT_MAX_GRID ? units : CT_MAX_GRID), dim3(CT_T), sm, s,
                       hist, reinterpret_cast<const long long*>(counts), units, T, M, mode, j0, w0, (long long)items,
                       (long long)regions, (long long)min_sites, best_t, best_lo, best_width,
                       reinterpret_cast<long long*>(sites), reinterpret_cast<long long*>(count),
                       reinterpret_cast<long long*>(n_tests), log_pvalue, log_padj,
                       reinterpret_cast<long long*>(ctrl_sites), reinterpret_cast<long long*>(ctrl_count),
                       log_fisher);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
