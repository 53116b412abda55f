// Motif enrichment (DESIGN.md section 3 item 18, section 8 "Enrichment"): per record the best site of every
// unit, and from that matrix a threshold-optimised Fisher test of primary against control records.
//
// record_best_kernel: block = one wavefront = (slice of records, unit quad).  The quad's taps sit in LDS as
// float4 [k][5], as in sites_kernel; the records are dealt round robin to the slices.  A record is walked in
// passes of EXPLAINN_BEST_SPAN starts: the pass's bases (and their complements) are staged in LDS, every
// lane takes SPAN / 64 starts and runs both strands' chains in one tap loop -- codescan.h's chain and bit
// pattern.  Every (start, strand) becomes bestsite.h's integer key: a lane keeps its largest key over the
// record's passes and one wave max per (record, unit) decides.  No atomics but the input flag.
//
// enrich_test_kernel: a workgroup loops over units.  It counts the unit's primary records into a 32768-bin
// LDS histogram, turns it in place into the tail a_t (a block-wide scan from the top pattern down) and parks
// that in its 128 KiB workspace slot; does the same for the control records, whose tail b_t stays in LDS;
// then every lane takes patterns t, t + 512, ... and evaluates the thresholds among them.  All counts are
// 32-bit integer LDS operations (fewer than 2^31 records); the hypergeometric tail is spacing_test's rule in
// fp64, one lane per threshold, and the best threshold is a min over (logp, -pattern) pairs: nothing depends
// on the order in which anything arrives.
#include "bestsite.h"
#include "codescan.h"
#include "tails.h"                             // hypergeom_logsf
#include "workspace.h"

namespace {

constexpr int RB_SPAN = EXPLAINN_BEST_SPAN;
constexpr int RB_ILP = RB_SPAN / 64;           // starts a lane takes per pass
constexpr int RB_BLOCKS = 16384;               // the records are cut into slices until a call has about this many blocks
static_assert(RB_SPAN % 64 == 0 && RB_ILP >= 1, "a pass is a whole number of starts per lane");

// (the second launch bound: the waves per SIMD the two forms run at)
template <bool BOTH>
__global__ __launch_bounds__(64, BOTH ? 4 : 8) void record_best_kernel(
    const uint8_t* __restrict__ seq, long long seq_len, const long long* __restrict__ off, int n_records,
    const float* __restrict__ Wt, const float* __restrict__ alpha, const float* __restrict__ shift,
    uint16_t* __restrict__ best_bits, int32_t* __restrict__ best_site, int U, int k, int* __restrict__ flags) {
    extern __shared__ float4 rb_sm[];          // taps [k][5] | codes [SPAN + k - 1] | their complements, likewise
    const int span_bytes = (RB_SPAN + k - 1 + 15) & ~15;
    uint8_t* cs = reinterpret_cast<uint8_t*>(rb_sm + k * 5);
    uint8_t* cc = cs + span_bytes;
    const int quad = blockIdx.y, lane = threadIdx.x;
    const float4* src = reinterpret_cast<const float4*>(Wt) + (size_t)quad * k * 5;
    for (int i = lane; i < k * 5; i += 64) rb_sm[i] = src[i];
    float al[4], sh[4];
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
        al[uu] = alpha[quad * 4 + uu];         // alpha and shift hold U rounded up to 4 entries
        sh[uu] = shift[quad * 4 + uu];
    }
    int bad = 0;
    for (long long r = blockIdx.x; r < n_records; r += gridDim.x) {
        const long long a = off[r], b = off[r + 1];
        const bool ok = BEST_RECORD_OK(a, b, seq_len);
        if (!ok) bad = 1;
        const int len = ok ? (int)(b - a) : 0;
        const int n_starts = len - k + 1;      // <= 0: the record is shorter than the kernel
        if (n_starts <= 0 && quad == 0)        // no pass stages its bases: they are still checked
            for (int i = lane; i < len; i += 64) bad |= seq[a + i] > 4;
        unsigned long long key[4] = {0ull, 0ull, 0ull, 0ull};     // a live start's key is never 0
        for (int t0 = 0; t0 < n_starts; t0 += RB_SPAN) {
            const int live_n = min(RB_SPAN, n_starts - t0);
            __syncthreads();                   // the taps are staged / the last pass's codes are read
            // the pass's bases and the k - 1 behind its last start: inside [a, b), inside seq
            bad |= stage_codes<true>(seq + a + t0, live_n + k - 1, lane, 64, cs, 0, cc);
            __syncthreads();
            float4 fw[RB_ILP], rv[RB_ILP];
            const uint8_t* fp[RB_ILP];
            const uint8_t* rp[RB_ILP];
#pragma unroll
            for (int i = 0; i < RB_ILP; ++i) {
                const int p = min(lane + i * 64, live_n - 1);      // a dead lane reads staged codes and keeps nothing
                fp[i] = cs + p;
                rp[i] = cc + p + k - 1;
            }
            tap_chains<BOTH>(rb_sm, k, fp, 1, fw, rp, rv);
#pragma unroll
            for (int i = 0; i < RB_ILP; ++i) {
                if (lane + i * 64 >= live_n) continue;
                const int p = t0 + lane + i * 64;
                const float f[4] = {fw[i].x, fw[i].y, fw[i].z, fw[i].w};
                const float g[4] = {rv[i].x, rv[i].y, rv[i].z, rv[i].w};
#pragma unroll
                for (int uu = 0; uu < 4; ++uu) {
                    unsigned long long kk = best_key(act_bits(al[uu], f[uu], sh[uu]), p, 1);
                    if (BOTH) {
                        const unsigned long long km = best_key(act_bits(al[uu], g[uu], sh[uu]), p, 0);
                        kk = km > kk ? km : kk;
                    }
                    key[uu] = kk > key[uu] ? kk : key[uu];
                }
            }
        }
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) {
            const unsigned long long kk = wave_max(key[uu]);
            const int u = quad * 4 + uu;
            if (lane == 0 && u < U) {
                const size_t o = (size_t)u * n_records + r;
                best_bits[o] = best_key_bits(kk);
                if (best_site) best_site[o] = best_key_site(kk);
            }
        }
    }
    if (quad == 0 && bad) atomicOr(flags, 1);
}

size_t record_best_lds(int k) {
    return (size_t)k * 5 * sizeof(float4) + 2 * (((size_t)RB_SPAN + k - 1 + 15) & ~(size_t)15);
}

// ------------------------------------------------------------------------------------------- the test
constexpr int EN_T = 512;                    // 8 waves: the fp64 lgamma chain gets 256 registers a lane
constexpr int EN_BINS = EXPLAINN_ACT_BINS;
constexpr int EN_WAVES = EN_T / 64;
constexpr int EN_MAX_GRID = 256;               // workgroups (and 128 KiB workspace slots) of a call at the most
static_assert(EN_BINS % EN_T == 0, "a lane takes a whole number of patterns");

// In place, h[b] <- sum_{b' >= b} h[b'], by all EN_T threads: chunks of EN_T bins from the top down, thread t
// of a chunk holding its bin EN_T - 1 - t, so that an inclusive scan up the threads is a sum from the bin
// upwards.  The tail also goes to `park` (global) and, when asked for, to `out`.  ws: EN_WAVES words of LDS.
__device__ __forceinline__ void tail_scan(unsigned* h, unsigned* ws, unsigned* __restrict__ park,
                                          unsigned* __restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned running = 0;
    for (int c = EN_BINS / EN_T - 1; c >= 0; --c) {
        const int b = c * EN_T + EN_T - 1 - tid;
        unsigned inc = wave_scan_up(h[b], lane);
        if (lane == 63) ws[wave] = inc;
        __syncthreads();
        unsigned before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < EN_WAVES; ++w) {
            const unsigned t = ws[w];
            before += w < wave ? t : 0;
            total += t;
        }
        inc += running + before;
        h[b] = inc;
        if (park) park[b] = inc;
        if (out) out[b] = inc;
        running += total;
        __syncthreads();                       // ws is rewritten by the next chunk
    }
}

struct EnBest { double logp; int pattern; };

// the smaller logp; among equal values the higher pattern
__device__ __forceinline__ bool en_better(double lp, int pat, double lq, int qat) {
    return lp < lq || (lp == lq && pat > qat);
}

__global__ __launch_bounds__(EN_T) void enrich_test_kernel(
    const uint16_t* __restrict__ bits, const uint8_t* __restrict__ labels, int units, int n_records,
    int32_t* __restrict__ n_thresholds, int32_t* __restrict__ best_pattern, long long* __restrict__ tp,
    long long* __restrict__ fp, double* __restrict__ log_pvalue, double* __restrict__ log_padj,
    long long* __restrict__ u2, double* __restrict__ auroc, long long* __restrict__ counts,
    unsigned* __restrict__ tails, unsigned* __restrict__ workspace) {
    extern __shared__ unsigned en_sm[];        // bins [32768] | scan words [16] | reduction slots
    unsigned* h = en_sm;
    unsigned* ws = en_sm + EN_BINS;
    double* red_lp = reinterpret_cast<double*>(ws + EN_WAVES);             // [16], 8-byte aligned: 64 bytes in
    unsigned long long* red_u2 = reinterpret_cast<unsigned long long*>(red_lp + EN_WAVES);
    int* red_pat = reinterpret_cast<int*>(red_u2 + EN_WAVES);
    int* red_m = red_pat + EN_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* A = workspace + (size_t)blockIdx.x * EN_BINS;                // this workgroup's slot
    for (int u = blockIdx.x; u < units; u += gridDim.x) {
        const uint16_t* col = bits + (size_t)u * n_records;
        unsigned* tl = tails ? tails + (size_t)u * 2 * EN_BINS : nullptr;
        for (int which = 1; which >= 0; --which) {                          // primary (label 1), then control (0)
            __syncthreads();                   // the last unit's evaluation has read h
            for (int b = tid; b < EN_BINS; b += EN_T) h[b] = 0u;
            __syncthreads();
            for (int r = tid; r < n_records; r += EN_T)
                if (labels[r] == which) atomicAdd(&h[col[r] & (EN_BINS - 1)], 1u);
            __syncthreads();
            tail_scan(h, ws, which ? A : nullptr, tl ? tl + (which ? 0 : EN_BINS) : nullptr);
        }
        __syncthreads();                       // A (global, written by this workgroup) and h (LDS) hold the tails
        const long long Np = A[0], Nc = h[0], N = Np + Nc;
        double lp = 0.0;
        int pat = -1, m = 0;
        unsigned long long usum = 0;
        for (int t = tid; t < EN_BINS; t += EN_T) {
            const long long a = A[t], b = h[t];
            const long long a1 = t + 1 < EN_BINS ? A[t + 1] : 0, b1 = t + 1 < EN_BINS ? h[t + 1] : 0;
            if (a == a1 && b == b1) continue;  // no included record holds this pattern
            ++m;
            usum += (unsigned long long)(a - a1) * (unsigned long long)(2 * (Nc - b) + (b - b1));
            const long long n = a + b;
            const double v = a * N > n * Np ? hypergeom_logsf(a, n, Np, Nc) : 0.0;
            if (pat < 0 || en_better(v, t, lp, pat)) { lp = v; pat = t; }
        }
        // wave, then workgroup: sums of m and u2, the best (logp, pattern)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m += __shfl_xor(m, o, 64);
            usum += __shfl_xor(usum, o, 64);
            const double lq = __shfl_xor(lp, o, 64);
            const int qat = __shfl_xor(pat, o, 64);
            if (qat >= 0 && (pat < 0 || en_better(lq, qat, lp, pat))) { lp = lq; pat = qat; }
        }
        if (lane == 0) { red_lp[wave] = lp; red_pat[wave] = pat; red_m[wave] = m; red_u2[wave] = usum; }
        __syncthreads();
        if (tid == 0) {
            lp = 0.0; pat = -1; m = 0; usum = 0;
            for (int w = 0; w < EN_WAVES; ++w) {
                m += red_m[w];
                usum += red_u2[w];
                if (red_pat[w] >= 0 && (pat < 0 || en_better(red_lp[w], red_pat[w], lp, pat))) {
                    lp = red_lp[w]; pat = red_pat[w];
                }
            }
            if (pat < 0) { pat = 0; lp = 0.0; }                            // m == 0: no included record
            double padj = 0.0;
            if (m > 0) {
                if (lp < -30.0) padj = fmin(0.0, log((double)m) + lp);
                else padj = fmin(0.0, log(-expm1((double)m * log1p(-exp(lp)))));
            }
            n_thresholds[u] = m;
            best_pattern[u] = pat;
            tp[u] = A[pat];
            fp[u] = h[pat];
            log_pvalue[u] = lp;
            log_padj[u] = padj;
            u2[u] = (long long)usum;
            auroc[u] = Np > 0 && Nc > 0 ? (double)usum / (2.0 * (double)Np * (double)Nc) : __longlong_as_double(0x7FF8000000000000ll);
            if (u == 0) { counts[0] = Np; counts[1] = Nc; }
        }
    }
}

constexpr size_t EN_LDS = (size_t)EN_BINS * sizeof(unsigned) + EN_WAVES * (sizeof(unsigned) + sizeof(double) +
                                                                            sizeof(unsigned long long) + 2 * sizeof(int));
int enrich_grid(int units) { return units < EN_MAX_GRID ? units : EN_MAX_GRID; }

}  // namespace

int launch_record_best(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets,
                       int64_t n_records, int strands, uint16_t* best_bits, int32_t* best_site, hipStream_t s) {
    const size_t sm = record_best_lds(c->k);
    const long long slices = std::min<long long>(n_records, std::max<long long>(1, (RB_BLOCKS + c->Uq - 1) / c->Uq));
    const dim3 grid((unsigned)slices, c->Uq);
    const long long* off = reinterpret_cast<const long long*>(rec_offsets);
    if (strands == 2)
        hipLaunchKernelGGL(record_best_kernel<true>, grid, dim3(64), sm, s, seq, (long long)seq_len, off,
                           (int)n_records, c->Wt, c->alpha, c->shift, best_bits, best_site, c->U, c->k, c->flags);
    else
        hipLaunchKernelGGL(record_best_kernel<false>, grid, dim3(64), sm, s, seq, (long long)seq_len, off,
                           (int)n_records, c->Wt, c->alpha, c->shift, best_bits, best_site, c->U, c->k, c->flags);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

extern "C" int64_t explainn_enrichment_workspace_bytes(int units, int64_t n_records) {
    if (units < 0 || n_records < 0 || n_records >= (int64_t)1 << 31) return 0;
    return (int64_t)std::max(enrich_grid(units), 1) * EN_BINS * (int64_t)sizeof(unsigned);
}

extern "C" int explainn_enrichment_test(const uint16_t* best_bits, const uint8_t* labels, int units,
                                        int64_t n_records, int32_t* n_thresholds, int32_t* best_pattern,
                                        int64_t* tp, int64_t* fp, double* log_pvalue, double* log_padj,
                                        int64_t* u2, double* auroc, int64_t* counts, uint32_t* tails,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
    if (units < 0 || n_records < 0 || n_records >= (int64_t)1 << 31) {
        explainn_set_error("enrichment_test: need units >= 0 and 0 <= n_records < 2^31 (units=%d n_records=%lld)",
                           units, (long long)n_records);
        return EXPLAINN_E_ARG;
    }
    if (units == 0) return EXPLAINN_OK;
    if ((n_records > 0 && (!best_bits || !labels)) || !n_thresholds || !best_pattern || !tp || !fp || !log_pvalue ||
        !log_padj || !u2 || !auroc || !counts) {
        explainn_set_error("enrichment_test: best_bits, labels and the nine outputs must be device pointers");
        return EXPLAINN_E_ARG;
    }
    if (!workspace_ok("enrichment_test", workspace, workspace_bytes,
                      explainn_enrichment_workspace_bytes(units, n_records), 256))
        return EXPLAINN_E_ARG;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&enrich_test_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)EN_LDS));
    hipLaunchKernelGGL(enrich_test_kernel, dim3(enrich_grid(units)), dim3(EN_T), EN_LDS,
                       static_cast<hipStream_t>(stream), best_bits, labels, units, (int)n_records, n_thresholds,
                       best_pattern, reinterpret_cast<long long*>(tp), reinterpret_cast<long long*>(fp), log_pvalue,
                       log_padj, reinterpret_cast<long long*>(u2), auroc, reinterpret_cast<long long*>(counts),
                       tails, static_cast<unsigned*>(workspace));
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
