// Evaluation metrics on the device (the reference's test.py::_get_performances and the callables of
// architectures.get_metrics): AUROC + average precision for binary targets, Pearson + Spearman
// otherwise, from device-resident row-major (N,T) fp32 targets y and scores s.  Two modes: per task
// (T columns of length N) and global (one column of length N*T, the Trainer's flatten()).  A column
// is a "segment"; segments have equal length n, so they are the second grid dimension everywhere.
//
// Sort: LSD radix sort of 64-bit keys, 8 bits per pass over the upper 32 bits only (4 passes).  The
// upper word is the order-preserving transform of the fp32 value (-0.0 canonicalised to +0.0,
// denormals kept); the lower word is payload -- the binary label, or the element's index for
// Spearman's scatter-back.  Every metric below depends on the payload only through sums over whole
// runs of equal values, so the order inside a run is irrelevant; the scatter is stable anyway
// (in-block rank from wave64 ballots), which makes the sorted array a function of the input alone.
// One pass = histogram, exclusive scan of the (digit, block) counts, scatter: each its own launch.
// Every prefix scan is block sums -> scan of the sums -> apply, ordered by kernel boundaries; there
// is no in-kernel cross-block hand-off anywhere in this file.
//
// After the sort (ascending), one scan of (label sum, last run start) pairs gives every run end e
// its start a and the positives up to e; with C(a) = positives before a and P = all positives:
//   pos = C(e+1) - C(a), neg = (e+1-a) - pos, negatives strictly below = a - C(a)
//   U2  = sum_runs pos * (2*(a - C(a)) + neg)                       AUROC = U2 / (2 P Nneg)
//   AP  = sum_runs (pos * (P - C(a))) / ((n - a) * P)               (descending cumulative counts)
// U2 is summed in 64-bit integers; an AP term is one correctly rounded division of two exactly
// represented integers (both < 2^53 for n <= 2^26).  Spearman: a run a..e gives every member the
// rank (a+e)/2 + 1; d = 2*rank - (n+1) = a + e + 1 - n is an integer with mean exactly 0, scattered
// back to the element's index; rho = sum dx*dy / sqrt(sum dx^2 * sum dy^2) with each product exact in
// fp64.  Pearson: two fp64 passes (means, then centred sums).
//
// Float sums are fixed-order trees: 16 terms per thread, xor-butterfly over the wave, 4 waves, then a
// block per segment over the block partials (at most 64 per thread, then the same tree).  The longest
// sequential chain is 64 additions.  No float atomics; the only atomic is the OR into the status word.
#include "common.h"
#include "workspace.h"

#include <math.h>

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int MT = 256;            // threads per block
constexpr int MI = 16;             // items per thread
constexpr int TILE = MT * MI;      // items per block
constexpr int64_t MAX_COL = (int64_t)1 << 26;   // 2*P*Nneg <= 2^53 up to here
constexpr int MAX_SEG = 65535;     // grid.y

// ---------------------------------------------------------------- small helpers
__device__ __forceinline__ u32 order_key(float v) {
    u32 b = __float_as_uint(v);
    if ((b << 1) == 0) b = 0;                               // -0.0 and +0.0 are one value
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ bool is_finite(float v) {
    return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u;
}
__device__ __forceinline__ size_t elem(int col, u32 pos, int T, int per_task) {
    return per_task ? (size_t)pos * T + col : (size_t)pos;
}
__device__ __forceinline__ u32 shfl_up_t(u32 v, int off) { return (u32)__shfl_up((int)v, off, 64); }
__device__ __forceinline__ u64 shfl_up_t(u64 v, int off) {
    const u32 lo = (u32)__shfl_up((int)(u32)v, off, 64), hi = (u32)__shfl_up((int)(v >> 32), off, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u32 shfl_t(u32 v, int src) { return (u32)__shfl((int)v, src, 64); }
__device__ __forceinline__ u64 shfl_t(u64 v, int src) {
    const u32 lo = (u32)__shfl((int)(u32)v, src, 64), hi = (u32)__shfl((int)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u32 lo = (u32)__shfl_xor((int)(u32)v, off, 64), hi = (u32)__shfl_xor((int)(v >> 32), off, 64);
        v += ((u64)hi << 32) | lo;
    }
    return v;
}
// sum over the block, fixed order (butterfly in the wave, waves 0..3 in order); result in every thread
__device__ __forceinline__ double block_sum_d(double v, double* sm) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}
__device__ __forceinline__ u64 block_sum_u64(u64 v, u64* sm) {
    v = wave_sum_u64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return sm[0] + sm[1] + sm[2] + sm[3];
}

// ---------------------------------------------------------------- keys
// status bits
constexpr u32 FLAG_NONFINITE = 1, FLAG_NOT_BINARY = 2;

__global__ __launch_bounds__(MT) void metrics_keys_binary_kernel(const float* __restrict__ y,
                                                                 const float* __restrict__ s,
                                                                 u64* __restrict__ keys, u32 n, int T,
                                                                 int per_task, u32* __restrict__ status) {
    const int seg = blockIdx.y;
    u32 flags = 0;
#pragma unroll 4
    for (int j = 0; j < MI; ++j) {
        const u32 pos = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (pos < n) {
            const size_t a = elem(seg, pos, T, per_task);
            const float yv = y[a], sv = s[a];
            if (!is_finite(yv) || !is_finite(sv)) flags |= FLAG_NONFINITE;
            else if (yv != 0.f && yv != 1.f) flags |= FLAG_NOT_BINARY;
            keys[(size_t)seg * n + pos] = ((u64)order_key(sv) << 32) | (yv == 1.f ? 1u : 0u);
        }
    }
    if (flags) atomicOr(status, flags);
}

// segments 0..S-1 hold the targets' columns, S..2S-1 the scores'; the low word is the position
__global__ __launch_bounds__(MT) void metrics_keys_linear_kernel(const float* __restrict__ y,
                                                                 const float* __restrict__ s,
                                                                 u64* __restrict__ keys, u32 n, int T,
                                                                 int per_task, int S, u32* __restrict__ status) {
    const int seg = blockIdx.y;
    const float* __restrict__ src = seg < S ? y : s;
    const int col = seg < S ? seg : seg - S;
    u32 flags = 0;
#pragma unroll 4
    for (int j = 0; j < MI; ++j) {
        const u32 pos = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (pos < n) {
            const float v = src[elem(col, pos, T, per_task)];
            if (!is_finite(v)) flags |= FLAG_NONFINITE;
            keys[(size_t)seg * n + pos] = ((u64)order_key(v) << 32) | pos;
        }
    }
    if (flags) atomicOr(status, flags);
}

// ---------------------------------------------------------------- radix pass
// hist[(seg*256 + digit)*nblk + block]: digit-major, so that its exclusive scan is the global start
// of every (digit, block) bucket
__global__ __launch_bounds__(MT) void metrics_hist_kernel(const u64* __restrict__ keys, u32* __restrict__ hist,
                                                          u32 n, int shift, u32 nblk) {
    __shared__ u32 h[256];
    const int seg = blockIdx.y;
    h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < MI; ++j) {
        const u32 pos = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (pos < n) atomicAdd(&h[(u32)(keys[(size_t)seg * n + pos] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[((size_t)seg * 256 + threadIdx.x) * nblk + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter.  Tile order = (wave, j, lane): wave w owns items w*1024 .. w*1024+1023 of the tile.
// Per item the lanes of equal digit are found with 8 ballots; the rank inside the wave is the wave's
// running count of that digit plus the number of lower lanes in the group.
__global__ __launch_bounds__(MT) void metrics_scatter_kernel(const u64* __restrict__ in, u64* __restrict__ out,
                                                             const u32* __restrict__ offs, u32 n, int shift,
                                                             u32 nblk) {
    __shared__ u32 cnt_[4 * 256];
    const int seg = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    volatile u32* cnt = cnt_ + wave * 256;
#pragma unroll
    for (int w = 0; w < 4; ++w) cnt_[w * 256 + tid] = 0;
    __syncthreads();
    const u32 base = blockIdx.x * TILE + wave * (64 * MI);
    const u64 lower = ((u64)1 << lane) - 1;
    u64 k[MI];
    u32 r[MI];
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const u32 pos = base + j * 64 + lane;
        k[j] = pos < n ? in[(size_t)seg * n + pos] : ~(u64)0;
    }
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const bool valid = base + j * 64 + lane < n;
        const u32 d = (u32)(k[j] >> shift) & 255u;
        u64 m = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 bal = __ballot(bit);
            m &= bit ? bal : ~bal;
        }
        const u32 before = __popcll(m & lower);
        const u32 c = cnt[d];
        r[j] = c + before;
        if (valid && before == 0) cnt[d] = c + __popcll(m);   // the group's lowest lane
    }
    __syncthreads();
    {
        // thread = digit: exclusive sum over the waves plus the bucket's global start
        u32 run = offs[((size_t)seg * 256 + tid) * nblk + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const u32 c = cnt_[w * 256 + tid];
            cnt_[w * 256 + tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        if (base + j * 64 + lane < n) {
            const u32 d = (u32)(k[j] >> shift) & 255u;
            const u32 dst = cnt[d] + r[j];
            if (dst < n) out[(size_t)seg * n + dst] = k[j];
        }
    }
}

// ---------------------------------------------------------------- three-launch scan
// Traits: T, id(), op(a,b) (associative and commutative), load(seg,i), store(seg,i,inclusive,own).
struct HistScan {                  // exclusive sum of the bucket counts, in place
    typedef u32 T;
    u32* a; u32 len;
    __device__ static T id() { return 0; }
    __device__ static T op(T x, T y) { return x + y; }
    __device__ T load(int seg, u32 i) const { return a[(size_t)seg * len + i]; }
    __device__ void store(int seg, u32 i, T incl, T own) const { a[(size_t)seg * len + i] = incl - own; }
};
// pair (labels so far, last run start so far) over the sorted keys; inclusive
template <bool LABEL>
struct RunScan {
    typedef u64 T;
    const u64* keys; u64* out; u32 len;
    __device__ static T id() { return 0; }
    __device__ static T op(T x, T y) {
        const u32 mx = (u32)x > (u32)y ? (u32)x : (u32)y;
        return (((x >> 32) + (y >> 32)) << 32) | mx;
    }
    __device__ T load(int seg, u32 i) const {
        const u64 k = keys[(size_t)seg * len + i];
        const bool start = i == 0 || (u32)(keys[(size_t)seg * len + i - 1] >> 32) != (u32)(k >> 32);
        return ((u64)(LABEL ? (u32)k & 1u : 0u) << 32) | (start ? i : 0u);
    }
    __device__ void store(int seg, u32 i, T incl, T) const { out[(size_t)seg * len + i] = incl; }
};

// inclusive scan of a tile held in (wave, j, lane) order; total = the whole tile's
template <class Tr>
__device__ __forceinline__ void block_scan(typename Tr::T (&v)[MI], typename Tr::T& total, typename Tr::T* sm) {
    typedef typename Tr::T T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T carry = Tr::id();
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        T x = v[j];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const T up = shfl_up_t(x, off);
            if (lane >= off) x = Tr::op(up, x);
        }
        x = Tr::op(carry, x);
        v[j] = x;
        carry = shfl_t(x, 63);
    }
    __syncthreads();
    if (lane == 0) sm[wave] = carry;
    __syncthreads();
    T off = Tr::id();
    for (int w = 0; w < wave; ++w) off = Tr::op(off, sm[w]);
    total = Tr::op(Tr::op(sm[0], sm[1]), Tr::op(sm[2], sm[3]));
#pragma unroll
    for (int j = 0; j < MI; ++j) v[j] = Tr::op(off, v[j]);
}

template <class Tr>
__global__ __launch_bounds__(MT) void metrics_scan_reduce_kernel(Tr tr, typename Tr::T* __restrict__ sums, u32 nb) {
    typedef typename Tr::T T;
    __shared__ T sm[4];
    const int seg = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T acc = Tr::id();
#pragma unroll 4
    for (int j = 0; j < MI; ++j) {
        const u32 i = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (i < tr.len) acc = Tr::op(acc, tr.load(seg, i));
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = shfl_up_t(acc, off);
        if (lane >= off) acc = Tr::op(up, acc);
    }
    if (lane == 63) sm[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0)
        sums[(size_t)seg * nb + blockIdx.x] = Tr::op(Tr::op(sm[0], sm[1]), Tr::op(sm[2], sm[3]));
}

// inclusive scan of the nb block sums of every segment, in place: one block per segment, tile after
// tile with the running total carried (integers: the order does not matter)
template <class Tr>
__global__ __launch_bounds__(MT) void metrics_scan_sums_kernel(typename Tr::T* __restrict__ sums, u32 nb) {
    typedef typename Tr::T T;
    __shared__ T sm[4];
    const int seg = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* __restrict__ a = sums + (size_t)seg * nb;
    T carry = Tr::id();
    for (u32 base = 0; base < nb; base += TILE) {
        T v[MI];
#pragma unroll
        for (int j = 0; j < MI; ++j) {
            const u32 i = base + wave * (64 * MI) + j * 64 + lane;
            v[j] = i < nb ? a[i] : Tr::id();
        }
        T total;
        block_scan<Tr>(v, total, sm);
#pragma unroll
        for (int j = 0; j < MI; ++j) {
            const u32 i = base + wave * (64 * MI) + j * 64 + lane;
            if (i < nb) a[i] = Tr::op(carry, v[j]);
        }
        carry = Tr::op(carry, total);
        __syncthreads();
    }
}

// sums: the inclusive scanned block sums (NULL when there is one block per segment)
template <class Tr>
__global__ __launch_bounds__(MT) void metrics_scan_apply_kernel(Tr tr, const typename Tr::T* __restrict__ sums,
                                                                u32 nb) {
    typedef typename Tr::T T;
    __shared__ T sm[4];
    const int seg = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 base = blockIdx.x * TILE + wave * (64 * MI);
    T v[MI], own[MI];
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const u32 i = base + j * 64 + lane;
        own[j] = v[j] = i < tr.len ? tr.load(seg, i) : Tr::id();
    }
    T total;
    block_scan<Tr>(v, total, sm);
    const T off = (sums && blockIdx.x > 0) ? sums[(size_t)seg * nb + blockIdx.x - 1] : Tr::id();
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const u32 i = base + j * 64 + lane;
        if (i < tr.len) tr.store(seg, i, Tr::op(off, v[j]), own[j]);
    }
}

template <class Tr>
int launch_scan(Tr tr, typename Tr::T* sums, int segs, hipStream_t st) {
    const u32 nb = (tr.len + TILE - 1) / TILE;
    if (nb > 1) {
        hipLaunchKernelGGL(metrics_scan_reduce_kernel<Tr>, dim3(nb, segs), dim3(MT), 0, st, tr, sums, nb);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(metrics_scan_sums_kernel<Tr>, dim3(segs), dim3(MT), 0, st, sums, nb);
        LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(metrics_scan_apply_kernel<Tr>, dim3(nb, segs), dim3(MT), 0, st, tr,
                       nb > 1 ? (const typename Tr::T*)sums : (const typename Tr::T*)nullptr, nb);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

// ---------------------------------------------------------------- binary pair
// per block: the runs that END in the block's tile
__global__ __launch_bounds__(MT) void metrics_binary_terms_kernel(const u64* __restrict__ keys,
                                                                  const u64* __restrict__ scan,
                                                                  u64* __restrict__ part_u, double* __restrict__ part_ap,
                                                                  u32 n, u32 nblk) {
    __shared__ double smd[4];
    __shared__ u64 smu[4];
    const int seg = blockIdx.y;
    const u64* __restrict__ kk = keys + (size_t)seg * n;
    const u64* __restrict__ sc = scan + (size_t)seg * n;
    const u64 P = sc[n - 1] >> 32;
    u64 u2 = 0;
    double ap = 0.0;
#pragma unroll 2
    for (int j = 0; j < MI; ++j) {
        const u32 i = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (i < n) {
            const u32 hi = (u32)(kk[i] >> 32);
            if (i == n - 1 || (u32)(kk[i + 1] >> 32) != hi) {
                const u64 e = sc[i];
                const u32 a = (u32)e;
                const u64 Ca = a ? sc[a - 1] >> 32 : 0;
                const u64 pos = (e >> 32) - Ca;
                const u64 neg = (u64)(i + 1 - a) - pos;
                u2 += pos * (2 * ((u64)a - Ca) + neg);
                if (pos) ap += (double)(pos * (P - Ca)) / (double)((u64)(n - a) * P);
            }
        }
    }
    const double aps = block_sum_d(ap, smd);
    const u64 us = block_sum_u64(u2, smu);
    if (threadIdx.x == 0) {
        part_u[(size_t)seg * nblk + blockIdx.x] = us;
        part_ap[(size_t)seg * nblk + blockIdx.x] = aps;
    }
}

__global__ __launch_bounds__(MT) void metrics_binary_final_kernel(const u64* __restrict__ scan,
                                                                  const u64* __restrict__ part_u,
                                                                  const double* __restrict__ part_ap,
                                                                  double* __restrict__ auroc, double* __restrict__ ap,
                                                                  int64_t* __restrict__ counts, u32 n, u32 nblk) {
    __shared__ double smd[4];
    __shared__ u64 smu[4];
    const int seg = blockIdx.x;
    u64 u2 = 0;
    double a = 0.0;
    for (u32 b = threadIdx.x; b < nblk; b += MT) {
        u2 += part_u[(size_t)seg * nblk + b];
        a += part_ap[(size_t)seg * nblk + b];
    }
    const double as = block_sum_d(a, smd);
    const u64 us = block_sum_u64(u2, smu);
    if (threadIdx.x == 0) {
        const u64 P = scan[(size_t)seg * n + n - 1] >> 32, Nn = (u64)n - P;
        auroc[seg] = (P == 0 || Nn == 0) ? (double)NAN : (double)us / (double)(2 * P * Nn);
        ap[seg] = P == 0 ? 0.0 : as;
        counts[2 * seg] = (int64_t)P;
        counts[2 * seg + 1] = (int64_t)Nn;
    }
}

// ---------------------------------------------------------------- linear pair
// every run end writes its position at the run's start
__global__ __launch_bounds__(MT) void metrics_run_ends_kernel(const u64* __restrict__ keys,
                                                              const u64* __restrict__ scan,
                                                              u32* __restrict__ end_at, u32 n) {
    const int seg = blockIdx.y;
    const u64* __restrict__ kk = keys + (size_t)seg * n;
#pragma unroll 4
    for (int j = 0; j < MI; ++j) {
        const u32 i = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (i < n && (i == n - 1 || (u32)(kk[i + 1] >> 32) != (u32)(kk[i] >> 32))) {
            const u32 a = (u32)scan[(size_t)seg * n + i];
            if (a < n) end_at[(size_t)seg * n + a] = i;
        }
    }
}

// d = 2*rank - (n+1) = start + end + 1 - n, written at the element's original position
__global__ __launch_bounds__(MT) void metrics_ranks_kernel(const u64* __restrict__ keys,
                                                           const u64* __restrict__ scan,
                                                           const u32* __restrict__ end_at, int* __restrict__ d,
                                                           u32 n) {
    const int seg = blockIdx.y;
#pragma unroll 4
    for (int j = 0; j < MI; ++j) {
        const u32 i = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (i < n) {
            const u32 a = (u32)scan[(size_t)seg * n + i];
            const u32 idx = (u32)keys[(size_t)seg * n + i];
            if (a < n && idx < n) {
                const u32 e = end_at[(size_t)seg * n + a];
                d[(size_t)seg * n + idx] = (int)(a + e + 1) - (int)n;
            }
        }
    }
}

// part[(seg*K + k)*nblk + block]
__global__ __launch_bounds__(MT) void metrics_sums_kernel(const float* __restrict__ y, const float* __restrict__ s,
                                                          double* __restrict__ part, u32 n, int T, int per_task,
                                                          u32 nblk) {
    __shared__ double sm[4];
    const int seg = blockIdx.y;
    double sy = 0.0, ss = 0.0;
#pragma unroll 4
    for (int j = 0; j < MI; ++j) {
        const u32 pos = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (pos < n) {
            const size_t a = elem(seg, pos, T, per_task);
            sy += (double)y[a];
            ss += (double)s[a];
        }
    }
    sy = block_sum_d(sy, sm);
    ss = block_sum_d(ss, sm);
    if (threadIdx.x == 0) {
        part[((size_t)seg * 2 + 0) * nblk + blockIdx.x] = sy;
        part[((size_t)seg * 2 + 1) * nblk + blockIdx.x] = ss;
    }
}

__global__ __launch_bounds__(MT) void metrics_means_kernel(const double* __restrict__ part, double* __restrict__ mean,
                                                           u32 n, u32 nblk) {
    __shared__ double sm[4];
    const int seg = blockIdx.x;
    double sy = 0.0, ss = 0.0;
    for (u32 b = threadIdx.x; b < nblk; b += MT) {
        sy += part[((size_t)seg * 2 + 0) * nblk + b];
        ss += part[((size_t)seg * 2 + 1) * nblk + b];
    }
    sy = block_sum_d(sy, sm);
    ss = block_sum_d(ss, sm);
    if (threadIdx.x == 0) {
        mean[2 * seg] = sy / (double)n;
        mean[2 * seg + 1] = ss / (double)n;
    }
}

// centred sums (Pearson, k = 0..2) and the rank sums (Spearman, k = 3..5): yy, ss, ys each
__global__ __launch_bounds__(MT) void metrics_centred_kernel(const float* __restrict__ y, const float* __restrict__ s,
                                                             const double* __restrict__ mean,
                                                             const int* __restrict__ d, double* __restrict__ part,
                                                             u32 n, int T, int per_task, int S, u32 nblk) {
    __shared__ double sm[4];
    const int seg = blockIdx.y;
    const double my = mean[2 * seg], ms = mean[2 * seg + 1];
    const int* __restrict__ dy = d + (size_t)seg * n;
    const int* __restrict__ ds = d + (size_t)(S + seg) * n;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int j = 0; j < MI; ++j) {
        const u32 pos = blockIdx.x * TILE + j * MT + threadIdx.x;
        if (pos < n) {
            const size_t a = elem(seg, pos, T, per_task);
            const double cy = (double)y[a] - my, cs = (double)s[a] - ms;
            acc[0] += cy * cy;
            acc[1] += cs * cs;
            acc[2] += cy * cs;
            const long long ry = dy[pos], rs = ds[pos];
            acc[3] += (double)(ry * ry);
            acc[4] += (double)(rs * rs);
            acc[5] += (double)(ry * rs);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double v = block_sum_d(acc[k], sm);
        if (threadIdx.x == 0) part[((size_t)seg * 6 + k) * nblk + blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(MT) void metrics_linear_final_kernel(const double* __restrict__ part,
                                                                  double* __restrict__ pearson,
                                                                  double* __restrict__ spearman, u32 nblk) {
    __shared__ double sm[4];
    const int seg = blockIdx.x;
    double tot[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double v = 0.0;
        for (u32 b = threadIdx.x; b < nblk; b += MT) v += part[((size_t)seg * 6 + k) * nblk + b];
        tot[k] = block_sum_d(v, sm);
    }
    if (threadIdx.x == 0) {
        // a constant column has a centred sum of exactly 0 only when its mean is exact; its rank sum
        // is always exactly 0.  Both correlations are undefined then (scipy: ConstantInputWarning).
        const bool constant = tot[3] == 0.0 || tot[4] == 0.0;
        pearson[seg] = (constant || tot[0] == 0.0 || tot[1] == 0.0)
                           ? (double)NAN : tot[2] / (sqrt(tot[0]) * sqrt(tot[1]));
        spearman[seg] = constant ? (double)NAN : tot[5] / (sqrt(tot[3]) * sqrt(tot[4]));
    }
}

// ---------------------------------------------------------------- host side
struct Layout {
    u32 n, nblk, hist_nb;
    int S, segs;                      // columns; sorted segments (S binary, 2S linear)
    // the workspace's pieces (null after a dry run) and its size
    u64 *keys_a = nullptr, *keys_b = nullptr, *run_sums = nullptr;
    u32 *hist = nullptr, *hist_sums = nullptr, *end_at = nullptr;
    double *part = nullptr, *aux = nullptr;
    int* d = nullptr;
    int64_t total;
};

// the geometry of a call and its workspace carved from ws (ws == nullptr: a dry run for the size)
int make_layout(int64_t N, int T, int mode, int kind, Layout* L, void* ws = nullptr) {
    if (N < 1 || T < 1) {
        explainn_set_error("metrics: need N >= 1 and T >= 1 (N=%lld T=%d)", (long long)N, T);
        return EXPLAINN_E_ARG;
    }
    if ((mode != EXPLAINN_METRICS_GLOBAL && mode != EXPLAINN_METRICS_PER_TASK) ||
        (kind != EXPLAINN_METRICS_BINARY && kind != EXPLAINN_METRICS_LINEAR)) {
        explainn_set_error("metrics: unknown mode %d / kind %d", mode, kind);
        return EXPLAINN_E_ARG;
    }
    const bool per_task = mode == EXPLAINN_METRICS_PER_TASK;
    if (N > MAX_COL || (!per_task && N * (int64_t)T > MAX_COL)) {
        explainn_set_error("metrics: a column of %lld values exceeds the limit of 2^26 (the AUROC "
                           "division is exact up to there)", (long long)(per_task ? N : N * (int64_t)T));
        return EXPLAINN_E_ARG;
    }
    const int S = per_task ? T : 1;
    const int segs = kind == EXPLAINN_METRICS_LINEAR ? 2 * S : S;
    if (segs > MAX_SEG) {
        explainn_set_error("metrics: %d tasks exceed the per-task limit of %d", T,
                           kind == EXPLAINN_METRICS_LINEAR ? MAX_SEG / 2 : MAX_SEG);
        return EXPLAINN_E_ARG;
    }
    L->n = (u32)(per_task ? N : N * (int64_t)T);
    L->S = S;
    L->segs = segs;
    L->nblk = (L->n + TILE - 1) / TILE;
    L->hist_nb = (256u * L->nblk + TILE - 1) / TILE;
    Carver cv(ws);
    const int64_t cells = (int64_t)segs * L->n;
    cv.take(&L->keys_a, cells);
    cv.take(&L->keys_b, cells);
    cv.take(&L->hist, (int64_t)segs * 256 * L->nblk);
    cv.take(&L->hist_sums, (int64_t)segs * L->hist_nb);
    cv.take(&L->run_sums, (int64_t)segs * L->nblk);
    if (kind == EXPLAINN_METRICS_BINARY) {
        cv.take(&L->part, (int64_t)S * L->nblk * 2);            // u64 U2 partials | fp64 AP partials
    } else {
        cv.take(&L->part, (int64_t)S * L->nblk * 6);            // also holds pass one's 2 sums
        cv.take(&L->aux, (int64_t)S * 2);                       // means
        cv.take(&L->end_at, cells);
        cv.take(&L->d, cells);
    }
    L->total = cv.bytes();
    return EXPLAINN_OK;
}

// ascending LSD sort of the keys' upper words: four 8-bit passes, result back in keys_a
int sort_segments(const Layout& L, hipStream_t st) {
    u64* a = L.keys_a;
    u64* b = L.keys_b;
    u32* hist = L.hist;
    const dim3 grid(L.nblk, L.segs);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 32 + 8 * pass;
        hipLaunchKernelGGL(metrics_hist_kernel, grid, dim3(MT), 0, st, a, hist, L.n, shift, L.nblk);
        LAUNCH_CHECK();
        HistScan hs{hist, 256u * L.nblk};
        const int rc = launch_scan(hs, L.hist_sums, L.segs, st);
        if (rc != EXPLAINN_OK) return rc;
        hipLaunchKernelGGL(metrics_scatter_kernel, grid, dim3(MT), 0, st, a, b, hist, L.n, shift, L.nblk);
        LAUNCH_CHECK();
        u64* t = a; a = b; b = t;
    }
    return EXPLAINN_OK;
}

int check_call(const void* y, const void* s, const void* o1, const void* o2, const void* status,
               const void* ws, int64_t ws_bytes, const Layout& L, const char* who) {
    if (!y || !s || !o1 || !o2 || !status || !ws) {
        explainn_set_error("%s: null pointer argument", who);
        return EXPLAINN_E_ARG;
    }
    return workspace_ok(who, ws, ws_bytes, L.total, 1) ? EXPLAINN_OK : EXPLAINN_E_ARG;
}

}  // namespace

extern "C" int64_t explainn_metrics_workspace_bytes(int64_t N, int T, int mode, int kind) {
    Layout L;
    const int rc = make_layout(N, T, mode, kind, &L);
    return rc == EXPLAINN_OK ? L.total : (int64_t)rc;
}

extern "C" int explainn_metrics_binary(const float* y, const float* s, int64_t N, int T, int mode,
                                       double* auroc, double* ap, int64_t* counts, unsigned int* status,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    Layout L;
    int rc = make_layout(N, T, mode, EXPLAINN_METRICS_BINARY, &L, workspace);
    if (rc != EXPLAINN_OK) return rc;
    rc = check_call(y, s, auroc, ap, status, workspace, workspace_bytes, L, "metrics_binary");
    if (rc != EXPLAINN_OK) return rc;
    if (!counts) {
        explainn_set_error("metrics_binary: null pointer argument");
        return EXPLAINN_E_ARG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int per_task = mode == EXPLAINN_METRICS_PER_TASK;
    const dim3 grid(L.nblk, L.segs);
    u64 *keys = L.keys_a, *scan = L.keys_b;
    hipLaunchKernelGGL(metrics_keys_binary_kernel, grid, dim3(MT), 0, st, y, s, keys, L.n, T, per_task, status);
    LAUNCH_CHECK();
    rc = sort_segments(L, st);
    if (rc != EXPLAINN_OK) return rc;
    RunScan<true> rs{keys, scan, L.n};
    rc = launch_scan(rs, L.run_sums, L.segs, st);
    if (rc != EXPLAINN_OK) return rc;
    u64* part_u = reinterpret_cast<u64*>(L.part);
    double* part_ap = L.part + (size_t)L.S * L.nblk;
    hipLaunchKernelGGL(metrics_binary_terms_kernel, grid, dim3(MT), 0, st, keys, scan, part_u, part_ap, L.n,
                       L.nblk);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_binary_final_kernel, dim3(L.S), dim3(MT), 0, st, scan, part_u, part_ap, auroc,
                       ap, counts, L.n, L.nblk);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

extern "C" int explainn_metrics_linear(const float* y, const float* s, int64_t N, int T, int mode,
                                       double* pearson, double* spearman, unsigned int* status,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
    Layout L;
    int rc = make_layout(N, T, mode, EXPLAINN_METRICS_LINEAR, &L, workspace);
    if (rc != EXPLAINN_OK) return rc;
    rc = check_call(y, s, pearson, spearman, status, workspace, workspace_bytes, L, "metrics_linear");
    if (rc != EXPLAINN_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int per_task = mode == EXPLAINN_METRICS_PER_TASK;
    const dim3 grid(L.nblk, L.segs), cols(L.nblk, L.S);
    u64 *keys = L.keys_a, *scan = L.keys_b;
    u32* end_at = L.end_at;
    int* d = L.d;
    double *part = L.part, *mean = L.aux;
    hipLaunchKernelGGL(metrics_keys_linear_kernel, grid, dim3(MT), 0, st, y, s, keys, L.n, T, per_task, L.S,
                       status);
    LAUNCH_CHECK();
    rc = sort_segments(L, st);
    if (rc != EXPLAINN_OK) return rc;
    RunScan<false> rs{keys, scan, L.n};
    rc = launch_scan(rs, L.run_sums, L.segs, st);
    if (rc != EXPLAINN_OK) return rc;
    hipLaunchKernelGGL(metrics_run_ends_kernel, grid, dim3(MT), 0, st, keys, scan, end_at, L.n);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_ranks_kernel, grid, dim3(MT), 0, st, keys, scan, end_at, d, L.n);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_sums_kernel, cols, dim3(MT), 0, st, y, s, part, L.n, T, per_task, L.nblk);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_means_kernel, dim3(L.S), dim3(MT), 0, st, part, mean, L.n, L.nblk);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_centred_kernel, cols, dim3(MT), 0, st, y, s, mean, d, part, L.n, T, per_task,
                       L.S, L.nblk);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(metrics_linear_final_kernel, dim3(L.S), dim3(MT), 0, st, part, pearson, spearman,
                       L.nblk);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
