// The empirical null of the filter activations ("Calibrated sites"): per unit, the
// exact histogram of the float16 activation explainn_call_sites compares with its threshold, over every
// live start of a device-resident sequence of base codes -- and from it tail counts, totals and the
// threshold of a stated false-positive rate.
//
// The activation is float16(exp(.)): never negative, so its bit pattern is one of 32768 values
// (0x0000 .. 0x7FFF) that sort in the order of the values they encode (+inf = 0x7C00, the NaN patterns
// above it).  A unit's null is therefore a 32768-bin integer histogram without binning error, and
// everything derived from it is an exact function of integers.
//
// act_hist_kernel: block = (unit, slice).  The unit's spans of EXPLAINN_ACT_SPAN starts are dealt round
// robin to its slices; a block keeps ONE 32768 x uint32 histogram in LDS (128 KiB: one block per CU, 16
// waves to hide the LDS-atomic latency) over all its spans -- a call has fewer than 2^31 starts, so no
// bin overflows -- and flushes the non-zero bins once, with 64-bit integer global atomics.  The pattern
// is codescan.h's, with one unit's taps as the accumulator.
//
// act_null_kernel: one wavefront per unit; a sum for the total, then a reverse scan over the bins (as
// sites_scan_tiles_kernel scans forward) for tail[b] = sum_{b' >= b} hist[b'] and the threshold.
#include "codescan.h"

namespace {

constexpr int AN_T = 1024;
constexpr int AN_BINS = EXPLAINN_ACT_BINS;
constexpr int AN_INF = 0x7C00;                 // the bit pattern of +inf: the largest value a threshold takes
constexpr int AN_ILP = 4;                      // positions a thread works on at a time
constexpr int AN_BLOCKS = 1024;                // slices are cut so that a call has about this many blocks
static_assert(EXPLAINN_ACT_SPAN % (AN_ILP * AN_T) == 0, "a span is a whole number of position chunks");
static_assert(AN_BINS == 32768 && AN_BINS % AN_T == 0, "one bin per non-negative float16 pattern");

__global__ __launch_bounds__(AN_T) void act_hist_kernel(
    const uint8_t* __restrict__ seq, long long start, int npos, long long period, int rc,
    const float* __restrict__ Wt, const float* __restrict__ alpha, const float* __restrict__ shift,
    unsigned long long* __restrict__ hist, int k, int nspans, int* __restrict__ flags) {
    extern __shared__ unsigned an_sm[];        // bins [32768] | taps float [k][5] | codes [SPAN + k - 1] bytes
    unsigned* h = an_sm;
    float* Wsm = reinterpret_cast<float*>(an_sm + AN_BINS);
    uint8_t* cs = reinterpret_cast<uint8_t*>(Wsm + k * 5);
    const int u = blockIdx.y, tid = threadIdx.x;
    for (int b = tid; b < AN_BINS; b += AN_T) h[b] = 0u;
    // the unit's taps out of the quad-interleaved table [Uq][k][5][4]
    const float* src = Wt + (size_t)(u >> 2) * k * 20 + (u & 3);
    for (int i = tid; i < k * 5; i += AN_T) Wsm[i] = src[(size_t)i * 4];
    const float al = alpha[u], sh = shift[u];
    const int first = rc ? k - 1 : 0, step = rc ? -1 : 1;
    const bool narrow = period > 0 && period < (1ll << 30);
    int bad = 0;
    for (int span = blockIdx.x; span < nspans; span += gridDim.x) {
        const int t0 = span * EXPLAINN_ACT_SPAN;                   // < npos < 2^31
        const int live_n = min(EXPLAINN_ACT_SPAN, npos - t0);      // start positions of this span
        __syncthreads();                       // the bins are zeroed / the last span's codes are read
        // the span's bases and the k-1 behind its last start: all inside [start, start + npos + k - 1),
        // which the entry point has checked against seq_len
        bad |= stage_codes<false>(seq + start + t0, live_n + k - 1, tid, AN_T, cs, rc, nullptr);
        __syncthreads();
        const long long r0 = period > 0 ? (start + t0) % period : 0;      // the span's first start in its record
        // AN_ILP positions per thread at a time: independent chains of (code byte -> tap -> add) in flight
        for (int p0 = tid; p0 < live_n; p0 += AN_ILP * AN_T) {
            bool live[AN_ILP];
            const uint8_t* cp[AN_ILP];
            float acc[AN_ILP];
#pragma unroll
            for (int i = 0; i < AN_ILP; ++i) {
                const int p = p0 + i * AN_T;
                live[i] = p < live_n;
                // a start whose k-mer would cross the end of its record is not counted
                if (period > 0) {
                    long long r;
                    if (narrow) r = (unsigned)(r0 + p) % (unsigned)period;
                    else { r = r0 + p; if (r >= period) r -= period; }     // p < SPAN < period: one wrap at most
                    live[i] = live[i] && r <= period - k;
                }
                cp[i] = cs + min(p, live_n - 1) + first;       // a dead lane reads staged codes and counts nothing
            }
            tap_chain(Wsm, k, cp, step, acc);
#pragma unroll
            for (int i = 0; i < AN_ILP; ++i)
                if (live[i]) atomicAdd(&h[act_bits(al, acc[i], sh)], 1u);
        }
    }
    if (u == 0 && bad) atomicOr(flags, 1);
    __syncthreads();
    unsigned long long* row = hist + (size_t)u * AN_BINS;
    for (int b = tid; b < AN_BINS; b += AN_T) {
        const unsigned v = h[b];
        if (v) atomicAdd(&row[b], (unsigned long long)v);
    }
}

// One wavefront per unit.  Lane l of chunk c holds bin 64 c + 63 - l, so an inclusive scan up the lanes,
// chunks from the top down, is the sum over the bins from its own upwards.
__global__ __launch_bounds__(64) void act_null_kernel(const unsigned long long* __restrict__ hist, double alpha,
                                                      unsigned long long* __restrict__ tail,
                                                      unsigned long long* __restrict__ total,
                                                      float* __restrict__ thresholds) {
    const int u = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* row = hist + (size_t)u * AN_BINS;
    unsigned long long sum = 0;
    for (int b = lane; b < AN_BINS; b += 64) sum += row[b];
    sum = wave_sum(sum);
    if (lane == 0) total[u] = sum;
    if (!tail && !thresholds) return;
    // at most m null values may exceed the threshold
    const unsigned long long m = (unsigned long long)floor(alpha * (double)sum);
    unsigned long long running = 0;
    int above = 0;                             // patterns b' in [1, 0x7C01] with tail[b'] > m
    for (int c = AN_BINS / 64 - 1; c >= 0; --c) {
        const int b = c * 64 + 63 - lane;
        const unsigned long long inc = wave_scan_up(row[b], lane) + running;
        if (tail) tail[(size_t)u * AN_BINS + b] = inc;
        above += __popcll(__ballot(b >= 1 && b <= AN_INF + 1 && inc > m));
        running = __shfl(inc, 63, 64);
    }
    // tail falls as b rises, so the patterns b <= 0x7C00 with tail[b + 1] <= m are those from `above` on
    if (lane == 0 && thresholds) {
        const int b = sum == 0 ? AN_INF : min(above, AN_INF);
        thresholds[u] = __half2float(__ushort_as_half((unsigned short)b));
    }
}

size_t act_hist_lds(int k) {
    return (size_t)AN_BINS * sizeof(unsigned) + (size_t)k * 5 * sizeof(float) +
           (((size_t)EXPLAINN_ACT_SPAN + k - 1 + 15) & ~(size_t)15);
}

}  // namespace

int launch_activation_histogram(explainn_ctx* c, const uint8_t* seq, int64_t start, int64_t npos, int64_t period,
                                int rc, uint64_t* hist, hipStream_t s) {
    const size_t sm = act_hist_lds(c->k);
    if (sm > 160 * 1024) {
        explainn_set_error("activation_histogram: kernel size %d needs %zu bytes of LDS, more than the device "
                           "allows", c->k, sm);
        return EXPLAINN_E_UNSUPPORTED;
    }
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&act_hist_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    const int nspans = (int)((npos + EXPLAINN_ACT_SPAN - 1) / EXPLAINN_ACT_SPAN);
    const int nslices = std::min(nspans, std::max(1, (AN_BLOCKS + c->U - 1) / c->U));
    hipLaunchKernelGGL(act_hist_kernel, dim3(nslices, c->U), dim3(AN_T), sm, s, seq, (long long)start, (int)npos,
                       (long long)period, rc, c->Wt, c->alpha, c->shift,
                       reinterpret_cast<unsigned long long*>(hist), c->k, nspans, c->flags);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

extern "C" int explainn_activation_null(const uint64_t* hist, int units, double alpha, uint64_t* tail,
                                        uint64_t* total, float* thresholds, void* stream) {
    if (units < 0 || !(alpha >= 0.0 && alpha <= 1.0)) {
        explainn_set_error("activation_null: need units >= 0 and 0 <= alpha <= 1 (units=%d alpha=%g)", units, alpha);
        return EXPLAINN_E_ARG;
    }
    if (units == 0) return EXPLAINN_OK;
    if (!hist || !total) {
        explainn_set_error("activation_null: hist and total must be device pointers");
        return EXPLAINN_E_ARG;
    }
    hipLaunchKernelGGL(act_null_kernel, dim3(units), dim3(64), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned long long*>(hist), alpha,
                       reinterpret_cast<unsigned long long*>(tail), reinterpret_cast<unsigned long long*>(total),
                       thresholds);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
