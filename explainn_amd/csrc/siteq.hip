// Site q-values ("Site q-values"): the exact Benjamini-Hochberg q-value of every score
// bin of every unit, over ALL the tests of the unit and not over a list of called sites.
//
// A site's score is discrete (a float16 bit pattern, sites.hip; an integer PWM score, pwmsites.hip), so its
// q-value is a function of (unit, bin).  With obs[u][b] the tests of unit u that scored in bin b (every live
// start and strand: explainn_activation_histogram, explainn_pwm_score_histogram), p[u][b] the p-value of the
// bin, N = sum_b obs[u][b] and R[b] = sum_{b' >= b} obs[u][b'] (the tests at least as extreme):
//
//     q[u][b] = min(1, min over b' <= b with R[b'] > 0 of (p[u][b'] * N) / R[b'])
//
// which is BH's  min over ranks j' >= j of p_(j') N / j'  for p non-increasing in b: the tests of a bin share
// a p-value and the last of them has rank R[b].
//
// site_q_kernel: one workgroup per unit, thread t owns the run of bins [t per, (t+1) per).  Integer run sums
// and a chain over the threads give every R; each term is one fp64 multiply and one fp64 divide, and a
// minimum is exact, so the table is a function of the input alone, equal bit for bit to a numpy
// restatement (tests/siteq_model.py).  No atomics on floats.
#include <algorithm>

#include "common.h"

namespace {

constexpr int SQ_T = 256;

__global__ __launch_bounds__(SQ_T) void site_q_kernel(const long long* __restrict__ obs, const double* __restrict__ p,
                                                      int B, double alpha, double* __restrict__ q,
                                                      long long* __restrict__ total, int* __restrict__ first) {
    __shared__ long long above[SQ_T];          // a thread's run sum, then the sum of the runs above its own
    __shared__ double below[SQ_T];             // a thread's run minimum, then the minimum of the runs below its own
    __shared__ long long all;
    __shared__ int over;                       // bins with q > alpha
    const int u = blockIdx.x, tid = threadIdx.x;
    const long long* orow = obs + (size_t)u * B;
    const double* prow = p + (size_t)u * B;
    double* qrow = q + (size_t)u * B;
    const int per = (B + SQ_T - 1) / SQ_T;
    const int lo = min(tid * per, B), hi = min(lo + per, B);
    long long mine = 0;
    for (int b = lo; b < hi; ++b) mine += orow[b];
    above[tid] = mine;
    if (tid == 0) over = 0;
    __syncthreads();
    if (tid == 0) {
        long long after = 0;
        for (int t = SQ_T - 1; t >= 0; --t) {
            const long long v = above[t];
            above[t] = after;
            after += v;
        }
        all = after;
    }
    __syncthreads();
    const double n = (double)all;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    // bins ascending: R falls by what each bin holds
    long long r = above[tid] + mine;
    double low = inf;
    for (int b = lo; b < hi; ++b) {
        if (r > 0) {
            const double term = (prow[b] * n) / (double)r;
            low = term < low ? term : low;
        }
        r -= orow[b];
    }
    below[tid] = low;
    __syncthreads();
    if (tid == 0) {
        double before = inf;
        for (int t = 0; t < SQ_T; ++t) {
            const double v = below[t];
            below[t] = before;
            before = v < before ? v : before;
        }
    }
    __syncthreads();
    r = above[tid] + mine;
    low = below[tid];
    int more = 0;
    for (int b = lo; b < hi; ++b) {
        if (r > 0) {
            const double term = (prow[b] * n) / (double)r;
            low = term < low ? term : low;
        }
        r -= orow[b];
        const double v = low < 1.0 ? low : 1.0;
        qrow[b] = v;
        more += v <= alpha ? 0 : 1;
    }
    if (first && more) atomicAdd(&over, more); // an integer sum: the order does not matter
    __syncthreads();
    if (tid == 0) {
        total[u] = all;
        if (first) first[u] = over;            // q never rises with b: the bins with q <= alpha are those from `over` on
    }
}

}  // namespace

extern "C" int explainn_site_qvalues(const int64_t* obs, const double* p, int units, int bins, double alpha, double* q,
                                     int64_t* total, int32_t* first, void* stream) {
    if (units < 0 || bins < 1 || bins > EXPLAINN_SITEQ_MAX_BINS || !(alpha >= 0.0 && alpha <= 1.0)) {
        explainn_set_error("site_qvalues: need units >= 0, 1 <= bins <= %d and 0 <= alpha <= 1 (units=%d bins=%d "
                           "alpha=%g)", EXPLAINN_SITEQ_MAX_BINS, units, bins, alpha);
        return EXPLAINN_E_ARG;
    }
    if (units == 0) return EXPLAINN_OK;
    if (!obs || !p || !q || !total) {
        explainn_set_error("site_qvalues: obs, p, q and total must be device pointers");
        return EXPLAINN_E_ARG;
    }
    hipLaunchKernelGGL(site_q_kernel, dim3(units), dim3(SQ_T), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(obs), p, bins, alpha, q,
                       reinterpret_cast<long long*>(total), first);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
