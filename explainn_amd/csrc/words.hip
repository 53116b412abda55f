// De novo word discovery (DESIGN.md section 3 item 26, section 8 "Word discovery"): which k-mers occur in more
// records of a primary set than of a control set, and the sites of the best one widened by its enriched
// one-mismatch neighbours.  Three context-free entry points; the greedy loop around them is
// explainn_amd/discover.py.  Everything is integer or fp64 (tails.h), so tests/words_model.py restates it exactly.
//
// Word code: bases A,C,G,T = 0..3, first base most significant, code = sum b_i 4^(k-1-i); rc(code) is the code of
// the reverse complement; with both strands a word is indexed by min(code, rc(code)).  3 <= k <= 10.
//
// Geometry (a first choice, untuned).  All three kernels run 256-thread workgroups that take the records
// blockIdx.x, blockIdx.x + gridDim.x, ... (at most WD_BLOCKS workgroups), a record at a time, the threads
// taking its starts EXPLAINN_WORD_SPAN at a pass.
//   word_count_kernel   a presence bitmap of 4^k bits in LDS (128 KiB at k = 10: one workgroup per CU; 8 KiB at
//                       k = 8).  A lane builds the code of its start from the k bytes; the LDS atomicOr tells
//                       whether the record had the word already, and a new bit is one integer add: into a
//                       workgroup-private LDS table for k <= WD_LDS_COUNT_K = 7 (64 KiB there: two workgroups
//                       per CU), flushed once at the end with adds that run along the table, straight into the
//                       caller's table above: one scattered global atomic per (record, word), which is what
//                       bounds k >= 8.  After a barrier the record's starts are walked again
//                       and the words they set are zeroed -- every set bit of such a word is this record's --,
//                       so the bitmap is cleared in full only once per workgroup, and a record of several passes
//                       keeps its bits until its last one.
//   word_test_kernel    one lane per word; the smallest logp is the largest bit pattern among the negative values,
//                       an integer atomicMax; word_pick_kernel then takes the lowest code that holds it, an
//                       integer atomicMin.  Any grid and any order give the same answer.
//   word_sites_kernel   a lane per start decides '+', '-' or no site and leaves that in a tile of LDS; after the
//                       tile's barrier a lane per BYTE reads the k starts that cover it (the last k - 1 of them
//                       from the tile before: three tiles rotate, so one barrier per tile is enough) and stores
//                       N where one is a site.  Gather form: an output byte has one writer per record and
//                       overlapping sites cannot race.  The count matrix is summed in LDS with integer atomics.
#include <algorithm>

#include "common.h"
#include "tails.h"

namespace {

constexpr int WD_T = 256;
constexpr int WD_BLOCKS = 1024;                // workgroups of a call at the most
#ifndef EXPLAINN_WORD_LDS_COUNT_K
#define EXPLAINN_WORD_LDS_COUNT_K 7            // measured against 6 (profiles/r39_discover_lds_count_ab.txt)
#endif
constexpr int WD_LDS_COUNT_K = EXPLAINN_WORD_LDS_COUNT_K;      // up to here the counts are summed in LDS first
static_assert(WD_T == EXPLAINN_WORD_SPAN, "a pass is one start per thread");

// rc(code): the complement, its 2k bits reversed, the two bits of every base swapped back
__device__ __forceinline__ unsigned wd_rc(unsigned c, int k) {
    const unsigned r = __brev(~c) >> (32 - 2 * k);
    return ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
}

// the code of the window p[0 .. k), whether all its bases are < 4, and whether a byte above 4 was read
__device__ __forceinline__ unsigned wd_window(const uint8_t* __restrict__ p, int k, bool& live, bool& odd) {
    unsigned c = 0, bad = 0;
    for (int j = 0; j < k; ++j) {
        const unsigned b = p[j];
        odd |= b > 4;
        bad |= b > 3;
        c = (c << 2) | (b & 3);
    }
    live = !bad;
    return c;
}

// 0 <= o0 <= o1 <= seq_len: compares only, before any byte of the record is read
__device__ __forceinline__ bool wd_record_ok(long long o0, long long o1, long long seq_len) {
    return o0 >= 0 && o0 <= o1 && o1 <= seq_len;
}

__device__ __forceinline__ void wd_raise(int* __restrict__ flags, int raise) {
    const int all = (__ballot(raise & 1) ? 1 : 0) | (__ballot(raise & 2) ? 2 : 0);
    if ((threadIdx.x & 63) == 0 && all && flags) atomicOr(flags, all);
}

__global__ __launch_bounds__(WD_T) void word_count_kernel(const uint8_t* __restrict__ seq, long long seq_len,
                                                          const long long* __restrict__ off, long long n_records,
                                                          int k, int both, int lds_counts, int* __restrict__ counts,
                                                          int* __restrict__ flags) {
    extern __shared__ unsigned wd_bits[];      // 4^k bits | int [4^k] when lds_counts
    const int tid = threadIdx.x, nwords = 1 << (2 * k), nbw = nwords >> 5;
    unsigned* cnt = wd_bits + nbw;
    for (int i = tid; i < nbw + (lds_counts ? nwords : 0); i += WD_T) wd_bits[i] = 0;
    __syncthreads();
    int raise = 0;
    for (long long r = blockIdx.x; r < n_records; r += gridDim.x) {
        const long long o0 = off[r], o1 = off[r + 1];          // the same in every thread: the barriers below are met by all
        if (!wd_record_ok(o0, o1, seq_len)) {
            raise |= 2;
            continue;
        }
        const long long starts = o1 - o0 - k + 1;
        if (starts <= 0) continue;
        const uint8_t* rec = seq + o0;
        for (long long s = tid; s < starts; s += WD_T) {       // s + k <= o1 - o0
            bool live, odd = false;
            const unsigned c = wd_window(rec + s, k, live, odd);
            if (odd) raise |= 1;
            if (!live) continue;
            const unsigned w = both ? min(c, wd_rc(c, k)) : c, bit = 1u << (w & 31);
            if (!(atomicOr(&wd_bits[w >> 5], bit) & bit)) {    // the record's first occurrence of w
                if (lds_counts) atomicAdd(&cnt[w], 1u);
                else atomicAdd(&counts[w], 1);
            }
        }
        __syncthreads();
        for (long long s = tid; s < starts; s += WD_T) {
            bool live, odd = false;
            const unsigned c = wd_window(rec + s, k, live, odd);
            if (!live) continue;
            const unsigned w = both ? min(c, wd_rc(c, k)) : c;
            wd_bits[w >> 5] = 0;                               // every bit of the word is this record's
        }
        __syncthreads();
    }
    if (lds_counts) {
        for (int i = tid; i < nwords; i += WD_T) {
            const unsigned c = cnt[i];
            if (c) atomicAdd(&counts[i], (int)c);
        }
    }
    wd_raise(flags, raise);
}

__global__ void word_test_init_kernel(long long* __restrict__ best, double* __restrict__ best_logp) {
    best[0] = -1;
    best[1] = 0;
    *best_logp = 0.0;
}

__global__ __launch_bounds__(WD_T) void word_test_kernel(const int* __restrict__ pos, const int* __restrict__ neg,
                                                         long long n_words, long long Np, long long Nc,
                                                         long long min_count, double* __restrict__ logp,
                                                         long long* __restrict__ best, double* __restrict__ best_logp) {
    __shared__ unsigned long long low;
    __shared__ unsigned long long tested;
    const int tid = threadIdx.x;
    if (tid == 0) low = 0, tested = 0;
    __syncthreads();
    unsigned long long key = 0, mine = 0;
    for (long long w = (long long)blockIdx.x * WD_T + tid; w < n_words; w += (long long)gridDim.x * WD_T) {
        const long long a = pos[w], b = neg[w];
        mine += a + b > 0 ? 1 : 0;
        double lp = 0.0;
        if (a >= min_count && a >= 0 && b >= 0 && a <= Np && b <= Nc && a * (Np + Nc) > (a + b) * Np)
            lp = hypergeom_logsf(a, a + b, Np, Nc);
        if (!(lp < 0.0)) lp = 0.0;                             // exactly +0.0 where nothing was found
        logp[w] = lp;
        // among negative doubles the smaller value has the larger bit pattern; +0.0 is pattern 0
        const unsigned long long bits = (unsigned long long)__double_as_longlong(lp);
        key = bits > key ? bits : key;
    }
    key = wave_max(key);
    mine = wave_sum(mine);
    if ((tid & 63) == 0) {
        if (key) atomicMax(&low, key);
        if (mine) atomicAdd(&tested, mine);
    }
    __syncthreads();
    if (tid == 0) {
        if (low) atomicMax(reinterpret_cast<unsigned long long*>(best_logp), low);
        if (tested) atomicAdd(reinterpret_cast<unsigned long long*>(best + 1), tested);
    }
}

// the lowest code that holds the smallest logp; best[0] starts as -1, the largest unsigned value
__global__ __launch_bounds__(WD_T) void word_pick_kernel(const double* __restrict__ logp, long long n_words,
                                                         const double* __restrict__ best_logp,
                                                         long long* __restrict__ best) {
    const unsigned long long want = (unsigned long long)__double_as_longlong(*best_logp);
    if (!want) return;
    for (long long w = (long long)blockIdx.x * WD_T + threadIdx.x; w < n_words; w += (long long)gridDim.x * WD_T)
        if ((unsigned long long)__double_as_longlong(logp[w]) == want)
            atomicMin(reinterpret_cast<unsigned long long*>(best), (unsigned long long)w);
}

// Hamming distance 0 to the seed, or 1 with the differing base accepted at its position
__device__ __forceinline__ bool wd_match(unsigned c, unsigned seed, unsigned long long accept, int k) {
    const unsigned x = c ^ seed, t = (x | (x >> 1)) & 0x55555555u;
    const int d = __popc(t);
    if (d != 1) return d == 0;
    const int j = (__ffs((int)t) - 1) >> 1;                    // the differing base, counted from the last one
    return (accept >> (4 * (k - 1 - j) + ((c >> (2 * j)) & 3))) & 1;
}

__global__ __launch_bounds__(WD_T) void word_sites_kernel(const uint8_t* __restrict__ seq, long long seq_len,
                                                          const long long* __restrict__ off, long long n_records,
                                                          int k, int both, unsigned seed, unsigned long long accept,
                                                          uint8_t* __restrict__ seq_out, long long* __restrict__ pfm,
                                                          long long* __restrict__ totals, int* __restrict__ flags) {
    __shared__ uint8_t hit[3][WD_T];           // 0 / 1 ('+') / 2 ('-') per start of this tile and the two before it
    __shared__ unsigned long long pf[4 * 10], ns;
    const int tid = threadIdx.x;
    if (tid < 40) pf[tid] = 0;
    if (tid == 0) ns = 0;
    __syncthreads();
    unsigned long long mysites = 0, nrec = 0;
    int raise = 0, g = 0;
    for (long long r = blockIdx.x; r < n_records; r += gridDim.x) {
        const long long o0 = off[r], o1 = off[r + 1];          // the same in every thread
        if (!wd_record_ok(o0, o1, seq_len)) {
            raise |= 2;
            continue;
        }
        const long long len = o1 - o0, starts = len - k + 1;
        if (starts <= 0) continue;
        const uint8_t* rec = seq + o0;
        int rec_hit = 0;
        for (long long t0 = 0; t0 < len; t0 += WD_T, g = g == 2 ? 0 : g + 1) {
            const long long s = t0 + tid;
            int h = 0;
            if (s < starts) {                                  // s + k <= len
                bool live, odd = false;
                const unsigned c = wd_window(rec + s, k, live, odd);
                if (odd) raise |= 1;
                if (live) {
                    const unsigned rcw = wd_rc(c, k);
                    h = wd_match(c, seed, accept, k) ? 1 : (both && wd_match(rcw, seed, accept, k) ? 2 : 0);
                    if (h) {
                        ++mysites;
                        if (pfm) {
                            const unsigned m = h == 1 ? c : rcw;   // a '-' site counts the bases of its reverse complement
                            for (int i = 0; i < k; ++i) atomicAdd(&pf[4 * i + ((m >> (2 * (k - 1 - i))) & 3)], 1ull);
                        }
                    }
                }
            }
            hit[g][tid] = (uint8_t)h;
            // tile g is complete behind this barrier; tile g + 1 is not written before everybody has read g - 1 below,
            // because the write of g + 2 = g - 1 lies behind the next barrier
            rec_hit |= __syncthreads_or(h);
            if (seq_out && s < len) {
                const uint8_t* prev = hit[g == 0 ? 2 : g - 1];
                int cov = 0;
                for (int j = 0; j < k; ++j) {                  // the starts s - j that cover byte s
                    const int q = tid - j;
                    cov |= q >= 0 ? hit[g][q] : (s - j >= 0 ? prev[q + WD_T] : 0);
                }
                if (cov) seq_out[o0 + s] = 4;                  // o0 + s < o1 <= seq_len
            }
        }
        nrec += rec_hit ? 1 : 0;
    }
    if (mysites) atomicAdd(&ns, mysites);
    __syncthreads();
    if (pfm && tid < 4 * k && pf[tid]) atomicAdd(reinterpret_cast<unsigned long long*>(pfm) + tid, pf[tid]);
    if (tid == 0) {
        if (ns) atomicAdd(reinterpret_cast<unsigned long long*>(totals), ns);
        if (nrec) atomicAdd(reinterpret_cast<unsigned long long*>(totals) + 1, nrec);
    }
    wd_raise(flags, raise);
}

bool wd_args_ok(const char* who, int64_t seq_len, int64_t n_records, int k) {
    if (k >= EXPLAINN_WORD_MIN_WIDTH && k <= EXPLAINN_WORD_MAX_WIDTH && seq_len >= 0 && n_records >= 0) return true;
    explainn_set_error("%s: need %d <= k <= %d, seq_len >= 0 and n_records >= 0 (k=%d seq_len=%lld n_records=%lld)", who,
                       EXPLAINN_WORD_MIN_WIDTH, EXPLAINN_WORD_MAX_WIDTH, k, (long long)seq_len, (long long)n_records);
    return false;
}

}  // namespace

extern "C" int explainn_word_counts(const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets, int64_t n_records,
                                    int k, int both_strands, int32_t* counts, int32_t* flags, void* stream) {
    if (!wd_args_ok("word_counts", seq_len, n_records, k)) return EXPLAINN_E_ARG;
    if (!rec_offsets || !counts || (seq_len > 0 && !seq)) {
        explainn_set_error("word_counts: seq, rec_offsets and counts must be device pointers");
        return EXPLAINN_E_ARG;
    }
    if (n_records == 0) return EXPLAINN_OK;
    const int lds_counts = k <= WD_LDS_COUNT_K ? 1 : 0;
    const size_t words = (size_t)1 << (2 * k), sm = words / 8 + (lds_counts ? words * sizeof(int) : 0);
    if (sm > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&word_count_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    const unsigned blocks = (unsigned)std::min<int64_t>(n_records, WD_BLOCKS);
    hipLaunchKernelGGL(word_count_kernel, dim3(blocks), dim3(WD_T), sm, static_cast<hipStream_t>(stream), seq,
                       (long long)seq_len, reinterpret_cast<const long long*>(rec_offsets), (long long)n_records, k,
                       both_strands ? 1 : 0, lds_counts, counts, flags);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

extern "C" int explainn_word_test(const int32_t* pos, const int32_t* neg, int64_t n_words, int64_t Np, int64_t Nc,
                                  int64_t min_count, double* logp, int64_t* best, double* best_logp, void* stream) {
    if (n_words < 0 || n_words > ((int64_t)1 << (2 * EXPLAINN_WORD_MAX_WIDTH)) || Np < 0 || Nc < 0 ||
        Np + Nc >= (int64_t)1 << 31 || min_count < 0) {
        explainn_set_error("word_test: need 0 <= n_words <= 4^%d, Np >= 0, Nc >= 0, Np + Nc < 2^31 and min_count >= 0 "
                           "(n_words=%lld Np=%lld Nc=%lld min_count=%lld)", EXPLAINN_WORD_MAX_WIDTH, (long long)n_words,
                           (long long)Np, (long long)Nc, (long long)min_count);
        return EXPLAINN_E_ARG;
    }
    if (!best || !best_logp || (n_words > 0 && (!pos || !neg || !logp))) {
        explainn_set_error("word_test: pos, neg, logp, best and best_logp must be device pointers");
        return EXPLAINN_E_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    long long* b = reinterpret_cast<long long*>(best);
    hipLaunchKernelGGL(word_test_init_kernel, dim3(1), dim3(1), 0, s, b, best_logp);
    LAUNCH_CHECK();
    if (n_words == 0) return EXPLAINN_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>((n_words + WD_T - 1) / WD_T, WD_BLOCKS);
    hipLaunchKernelGGL(word_test_kernel, dim3(blocks), dim3(WD_T), 0, s, pos, neg, (long long)n_words, (long long)Np,
                       (long long)Nc, (long long)min_count, logp, b, best_logp);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(word_pick_kernel, dim3(blocks), dim3(WD_T), 0, s, logp, (long long)n_words, best_logp, b);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

extern "C" int explainn_word_sites(const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets, int64_t n_records,
                                   int k, int both_strands, int64_t seed, uint64_t accept, uint8_t* seq_out,
                                   int64_t* pfm, int64_t* totals, int32_t* flags, void* stream) {
    if (!wd_args_ok("word_sites", seq_len, n_records, k)) return EXPLAINN_E_ARG;
    if (seed < 0 || seed >= (int64_t)1 << (2 * k) || (accept >> (4 * k)) != 0) {
        explainn_set_error("word_sites: need 0 <= seed < 4^k and no accept bit from 4k on (k=%d seed=%lld "
                           "accept=0x%llx)", k, (long long)seed, (unsigned long long)accept);
        return EXPLAINN_E_ARG;
    }
    if (!rec_offsets || !totals || (seq_len > 0 && !seq) || (seq_out && seq_out == seq)) {
        explainn_set_error("word_sites: seq, rec_offsets and totals must be device pointers, and seq_out another "
                           "array than seq");
        return EXPLAINN_E_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    // every byte is copied first; the kernel then stores N over the covered ones only
    if (seq_out && seq_len > 0) HIP_TRY(hipMemcpyAsync(seq_out, seq, (size_t)seq_len, hipMemcpyDeviceToDevice, s));
    if (n_records == 0) return EXPLAINN_OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(n_records, WD_BLOCKS);
    hipLaunchKernelGGL(word_sites_kernel, dim3(blocks), dim3(WD_T), 0, s, seq, (long long)seq_len,
                       reinterpret_cast<const long long*>(rec_offsets), (long long)n_records, k, both_strands ? 1 : 0,
                       (unsigned)seed, (unsigned long long)accept, seq_out, reinterpret_cast<long long*>(pfm),
                       reinterpret_cast<long long*>(totals), flags);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
