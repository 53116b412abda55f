// Motif spacing: for every (anchor unit a, partner unit b), the histogram of
// the distances between their sites, by relative orientation -- and the SpaMo test of a preferred spacing.
//
// Sites come as explainn_call_sites lists them, per (unit, strand) in ascending start.  An ordered pair of
// distinct records (i, j) with d = (start_j - start_i) * strand_i, |d| <= D, adds 1 to
// hist[a][b][strand_i != strand_j][d + D].  Integers throughout: the result does not depend on the geometry.
//
// spacing_hist_kernel: block = (partner, anchor, slice).  The anchor's records (its '+' run and its '-' run
// are one contiguous range) are dealt to the slices in chunks of SP_T; a thread takes one record, finds by
// a lower-bound search the first partner site at start_i - D in the partner's '+' and '-' lists, and walks
// forward while start_j <= start_i + D, counting into a 2 x (2D+1) LDS histogram with integer atomics.  One
// flush per block adds the non-zero bins into hist with 64-bit integer global atomics.  Nothing relies on
// the lists being sorted for memory safety: a search never leaves [lo, hi) and a bin is checked before it
// is counted; an unsorted list only gives a wrong count.
//
// spacing_test_kernel: one lane per (a, b, orientation): the admissible bins (folded when a == b), their
// sum, their largest count and the Bonferroni-corrected binomial tail of it, in fp64.
#include "common.h"
#include "tails.h"                              // binom_logpmf

namespace {

constexpr int SP_T = 256;
constexpr int SP_MAX_D = EXPLAINN_SPACING_MAX_DISTANCE;
constexpr int SP_SLICE_BLOCKS = 2048;          // few pairs: the anchor's records are split until a call has about this many blocks
constexpr int SP_MAX_SLICES = 64;

__device__ __forceinline__ int unit_of(const int32_t* set, int i) { return set ? set[i] : i; }

// first index in [lo, hi) whose start is >= key (hi if none); stays inside [lo, hi) whatever pos holds
__device__ __forceinline__ long long lower_bound(const long long* __restrict__ pos, long long lo, long long hi,
                                                 long long key) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (pos[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(SP_T) void spacing_hist_kernel(
    const long long* __restrict__ pos, const long long* __restrict__ off2, int U,
    const int32_t* __restrict__ anchors, const int32_t* __restrict__ partners, int P, int D,
    unsigned long long* __restrict__ hist) {
    // [2][2D+1]; 32-bit bins: a workgroup adds at most (its anchor records) x (partner records on one start)
    // to a bin, below 2^32 for lists of distinct starts (the header says so); the flush widens to 64 bits
    extern __shared__ unsigned sp_sm[];
    const int nb = 2 * D + 1, tid = threadIdx.x;
    const int ua = unit_of(anchors, blockIdx.y), ub = unit_of(partners, blockIdx.x);
    if (ua < 0 || ua >= U || ub < 0 || ub >= U) return;           // a unit outside the lists counts nothing
    const long long a0 = off2[2 * ua], am = off2[2 * ua + 1], a1 = off2[2 * ua + 2];
    const long long b0 = off2[2 * ub], bm = off2[2 * ub + 1], b1 = off2[2 * ub + 2];
    const long long first = a0 + (long long)blockIdx.z * SP_T, step = (long long)gridDim.z * SP_T;
    if (first >= a1 || b0 >= b1) return;           // no anchor record for this slice, or no partner site
    for (int b = tid; b < 2 * nb; b += SP_T) sp_sm[b] = 0u;
    __syncthreads();
    for (long long i = first + tid; i < a1; i += step) {
        const long long pi = pos[i];
        const int si = i < am ? 1 : -1;
#pragma unroll
        for (int sj = 0; sj < 2; ++sj) {           // the partner's '+' list, then its '-' list
            const long long lo = sj ? bm : b0, hi = sj ? b1 : bm;
            unsigned* h = sp_sm + ((si > 0) != (sj == 0) ? nb : 0) + D;
            for (long long j = lower_bound(pos, lo, hi, pi - D); j < hi; ++j) {
                const long long d = pos[j] - pi;
                if (d > D) break;
                if (j != i && d >= -D) atomicAdd(&h[(int)d * si], 1u);
            }
        }
    }
    __syncthreads();
    unsigned long long* row = hist + ((size_t)blockIdx.y * P + blockIdx.x) * 2 * nb;
    for (int b = tid; b < 2 * nb; b += SP_T) {
        const unsigned v = sp_sm[b];
        if (v) atomicAdd(&row[b], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(SP_T) void spacing_test_kernel(
    const long long* __restrict__ hist, int A, int P, const int32_t* __restrict__ anchors,
    const int32_t* __restrict__ partners, int D, int min_distance, long long min_count,
    long long* __restrict__ total, int32_t* __restrict__ best_distance, long long* __restrict__ best_count,
    double* __restrict__ pvalue) {
    const long long e = (long long)blockIdx.x * SP_T + threadIdx.x;
    if (e >= (long long)A * P * 2) return;
    const int o = (int)(e & 1), b = (int)((e >> 1) % P), a = (int)((e >> 1) / P);
    const bool same = unit_of(anchors, a) == unit_of(partners, b);
    const long long* row = hist + (size_t)e * (2 * D + 1);
    // a == b, same orientation: every unordered pair sits once at +d and once at -d -- the bins d > 0 only;
    // a == b, opposite orientation: every unordered pair sits twice in one bin -- all bins, counts halved
    const bool positive = same && o == 0, halve = same && o == 1;
    const int dmin = positive ? max(min_distance, 1) : min_distance;
    long long n = 0, c = -1;
    int m = 0, best = 0;
    for (int d = positive ? dmin : -D; d <= D; ++d) {
        if (abs(d) < dmin) continue;
        long long v = row[d + D];
        if (halve) v >>= 1;
        n += v;
        ++m;
        if (v > c) { c = v; best = d; }            // the lowest bin index wins a tie
    }
    total[e] = n;
    double p = 1.0;
    if (m == 0 || n < max(min_count, 1ll)) {
        c = 0;
        best = 0;
    } else if (m > 1) {
        const double q = 1.0 / (double)m, logq = log(q), log1mq = log1p(-q), nd = (double)n;
        double sum = 0.0;
        for (long long x = c; x <= n; ++x) {       // c >= n / m: the terms fall from the first one on
            const double s = sum + exp(binom_logpmf(nd, (double)x, logq, log1mq));
            if (s == sum) break;
            sum = s;
        }
        p = fmin(1.0, (double)m * sum);
    }
    best_distance[e] = best;
    best_count[e] = c;
    pvalue[e] = p;
}

}  // namespace

int launch_site_spacing(const int64_t* pos, const int64_t* offsets2, int U, const int32_t* anchors, int A,
                        const int32_t* partners, int P, int D, int64_t* hist, hipStream_t s) {
    static_assert(2 * (2 * SP_MAX_D + 1) * sizeof(unsigned) <= 64 * 1024, "the histogram of a pair fits the LDS");
    const long long pairs = (long long)A * P;
    const int slices = (int)std::min<long long>(SP_MAX_SLICES, std::max<long long>(1, SP_SLICE_BLOCKS / pairs));
    const size_t sm = (size_t)2 * (2 * D + 1) * sizeof(unsigned);
    hipLaunchKernelGGL(spacing_hist_kernel, dim3(P, A, slices), dim3(SP_T), sm, s,
                       reinterpret_cast<const long long*>(pos), reinterpret_cast<const long long*>(offsets2), U,
                       anchors, partners, P, D, reinterpret_cast<unsigned long long*>(hist));
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

int launch_spacing_test(const int64_t* hist, int A, int P, const int32_t* anchors, const int32_t* partners, int D,
                        int min_distance, int64_t min_count, int64_t* total, int32_t* best_distance,
                        int64_t* best_count, double* pvalue, hipStream_t s) {
    const long long lanes = (long long)A * P * 2;
    hipLaunchKernelGGL(spacing_test_kernel, dim3((unsigned)((lanes + SP_T - 1) / SP_T)), dim3(SP_T), 0, s,
                       reinterpret_cast<const long long*>(hist), A, P, anchors, partners, D, min_distance,
                       (long long)min_count, reinterpret_cast<long long*>(total), best_distance,
                       reinterpret_cast<long long*>(best_count), pvalue);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
