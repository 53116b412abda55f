// Motif tree and merged cluster motifs ("Motif tree"): agglomerate the motifs of a
// self-comparison (explainn_motif_compare) into a dendrogram, cut it, place every member in the frame of its
// cluster from the alignments the comparison found, and pool the placed count matrices.  Stand-alone like
// motifs.hip: device pointers and a caller's workspace, no explainn_ctx, no allocation, no host sync.
//
//   motif_tree_prepare_kernel, one lane per (row, column): q = (int32) rintf(ncor * 2^20) of the upper-triangle
//     entry of the pair, into two symmetric M x M matrices: L, the linkage as an int64 (the sum of q over the
//     leaf pairs of two clusters for average linkage, their max / min for single / complete), and K, the best
//     leaf pair as a packed key (q biased to unsigned << 32 | 65535 - i << 16 | 65535 - j: the larger key is
//     the larger q, then the smaller i, then the smaller j), which merges by max.
//   motif_tree_kernel, ONE workgroup of 1024 lanes, the M - 1 steps inside, workgroup barriers between their
//     phases (it uses one CU; the loop is sequential across steps).  Per live slot c the best partner b > c --
//     largest linkage as a double, (double) sum / (double) pairs, ties to the smaller b -- is cached in LDS
//     (value 8 bytes, partner 2, and 2 for the list below).  A step: every lane derives (F, H) of the step
//     from the best leaf pair of (lo, hi); barrier; lanes over leaves move the leaves of hi into lo's frame,
//     lanes over slots combine rows lo and hi of L and K into row and column lo and either compare the new
//     (c, lo) entry with c's cache or, when c's cached partner was lo or hi, put c on a list, and reduce the
//     new entries with c > lo to row lo's own cache entry; barrier; the waves rescan the listed rows, one row
//     a wave, a short list's rows split over 2 to 16 waves each (one more barrier); barrier; the argmax over the cache, ties to the smaller slot; barrier.  Every value is an integer or one correctly rounded division of integers, so the result
//     does not depend on the order of the list or of the lanes.
//   motif_tree_cut_*: one lane per leaf walks its chain of merges above the cut (gone[slot] is the step that
//     merged a slot away), integer atomicMin / atomicMax per slot for the frame bounds, then the shifts are
//     moved so that the smallest of a cluster is 0.
//   motif_tree_pool_kernel: one workgroup per cluster, lanes over (column, base), the members in ascending leaf
//     order, fp64 adds of the placed fp32 entries.  No float atomics.
#include <cmath>

#include "common.h"
#include "workspace.h"

namespace {

constexpr int MT_THREADS = 1024;
constexpr int MT_WAVES = MT_THREADS / 64;
constexpr int MT_NONE = 0xFFFF;
constexpr int MT_BATCH = 4;      // slots a lane reads at a time in the placement and update passes
constexpr int MT_POOL_THREADS = 256;

// workspace: L [M][M] int64 | K [M][M] uint64 | size [M] int32 | slot [M] int32, each 256-byte aligned
struct mt_pieces { int64_t* L; uint64_t* K; int* size; int* slot; };
__host__ inline void mt_workspace(Carver& cv, int64_t M, mt_pieces* w) {
    cv.take(&w->L, M * M);
    cv.take(&w->K, M * M);
    cv.take(&w->size, M);
    cv.take(&w->slot, M);
}
// LDS: val [M] double | part [M] uint16 | list [M] uint16 | rv [16] double | rc [16] int | pv [16] double |
// pc [16] int | n_list int
__host__ __device__ inline size_t mt_tail(int M) { return ((size_t)12 * M + 7) & ~(size_t)7; }
__host__ inline size_t mt_lds_bytes(int M) { return mt_tail(M) + 2 * MT_WAVES * 12 + 16; }

__global__ __launch_bounds__(256) void motif_tree_prepare_kernel(const float* __restrict__ ncor, int M, int64_t total,
                                                                 int64_t* __restrict__ L, uint64_t* __restrict__ K) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int r = (int)(idx / M), c = (int)(idx - (int64_t)r * M);
        const int i = min(r, c), j = max(r, c);
        int64_t l = 0;
        uint64_t k = 0;
        if (i != j) {
            const int q = (int)rintf(ncor[(size_t)i * M + j] * 1048576.0f);
            l = q;
            k = ((uint64_t)((uint32_t)q ^ 0x80000000u) << 32) | ((uint64_t)(65535 - i) << 16) | (uint64_t)(65535 - j);
        }
        L[idx] = l;
        K[idx] = k;
    }
}

__device__ __forceinline__ double mt_value(int64_t s, int na, int nb, int avg) {
    return avg ? (double)s / (double)((int64_t)na * nb) : (double)s;
}

// the best partner b > c of slot c among the 64-entry blocks seg, seg + nseg, .. of its row, by one wave;
// every lane returns it
__device__ __forceinline__ void mt_scan_part(int c, int M, const int64_t* L, const int* size, int avg, int lane,
                                             int seg, int nseg, double& bv, int& bp) {
    const int nc = size[c];
    const int64_t* row = L + (size_t)c * M;
    bv = -INFINITY;
    bp = MT_NONE;
    auto take = [&](int64_t s, int nb, int b) {
        if (nb > 0) {
            const double v = mt_value(s, nc, nb, avg);
            if (v > bv) { bv = v; bp = b; }
        }
    };
    const int step = 64 * nseg;
    int b = c + 1 + lane + 64 * seg;
    for (; b + 3 * step < M; b += 4 * step) {            // four independent loads in flight, taken in ascending b
        const int n0 = size[b], n1 = size[b + step], n2 = size[b + 2 * step], n3 = size[b + 3 * step];
        const int64_t s0 = row[b], s1 = row[b + step], s2 = row[b + 2 * step], s3 = row[b + 3 * step];
        take(s0, n0, b);
        take(s1, n1, b + step);
        take(s2, n2, b + 2 * step);
        take(s3, n3, b + 3 * step);
    }
    for (; b < M; b += step) take(row[b], size[b], b);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int op = __shfl_xor(bp, off, 64);
        if (ov > bv || (ov == bv && op < bp)) { bv = ov; bp = op; }
    }
}

// the whole row by one wave, into the cache
__device__ __forceinline__ void mt_scan_row(int c, int M, const int64_t* L, const int* size, int avg, int lane,
                                            double* val, uint16_t* part) {
    double bv;
    int bp;
    mt_scan_part(c, M, L, size, avg, lane, 0, 1, bv, bp);
    if (lane == 0) {
        val[c] = bv;
        part[c] = (uint16_t)bp;
    }
}

// the live slot with the largest cached value, ties to the smaller slot; one barrier inside
__device__ __forceinline__ int mt_argmax(int M, const int* size, const double* val, const uint16_t* part, double* rv,
                                         int* rc, int tid, int lane, int wave) {
    double bv = -INFINITY;
    int bc = 0x7fffffff;
    for (int c = tid; c < M; c += MT_THREADS)
        if (part[c] != MT_NONE) {                        // a merged slot has no partner: the cache alone tells
            const double v = val[c];
            if (bc == 0x7fffffff || v > bv) { bv = v; bc = c; }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(bv, off, 64);
        const int oc = __shfl_xor(bc, off, 64);
        if (oc != 0x7fffffff && (bc == 0x7fffffff || ov > bv || (ov == bv && oc < bc))) { bv = ov; bc = oc; }
    }
    if (lane == 0) {
        rv[wave] = bv;
        rc[wave] = bc;
    }
    __syncthreads();
    bv = rv[0];
    bc = rc[0];
    for (int k = 1; k < MT_WAVES; ++k) {
        const double ov = rv[k];
        const int oc = rc[k];
        if (oc != 0x7fffffff && (bc == 0x7fffffff || ov > bv || (ov == bv && oc < bc))) { bv = ov; bc = oc; }
    }
    return bc;
}

__global__ __launch_bounds__(MT_THREADS) void motif_tree_kernel(
    const int16_t* __restrict__ align, const int32_t* __restrict__ widths, int M, int linkage, int64_t* L, uint64_t* K,
    int* size, int* slot, int32_t* log, int64_t* link, int32_t* gone, int32_t* flips, int32_t* shifts) {
    extern __shared__ double mt_sm[];
    double* val = mt_sm;
    uint16_t* part = reinterpret_cast<uint16_t*>(val + M);
    uint16_t* list = part + M;
    double* rv = reinterpret_cast<double*>(reinterpret_cast<char*>(mt_sm) + mt_tail(M));
    int* rc = reinterpret_cast<int*>(rv + MT_WAVES);
    double* pv = reinterpret_cast<double*>(rc + MT_WAVES);
    int* pc = reinterpret_cast<int*>(pv + MT_WAVES);
    int* n_list = pc + MT_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int avg = linkage == EXPLAINN_LINKAGE_AVERAGE;

    for (int c = tid; c < M; c += MT_THREADS) {
        size[c] = 1;
        slot[c] = c;
        gone[c] = -1;
        flips[c] = 0;
        shifts[c] = 0;
    }
    if (M < 2) return;
    __syncthreads();
    for (int c = wave; c < M; c += MT_WAVES) mt_scan_row(c, M, L, size, avg, lane, val, part);
    __syncthreads();
    int lo = mt_argmax(M, size, val, part, rv, rc, tid, lane, wave);

    for (int t = 0; t < M - 1; ++t) {
        if (lo >= M) return;                             // no live pair: cannot happen with M - t live slots
        const int hi = part[lo];
        const int nlo = size[lo], nhi = size[hi];
        const int64_t s = L[(size_t)lo * M + hi];
        const uint64_t key = K[(size_t)lo * M + hi];
        const int i = 65535 - (int)((key >> 16) & 65535), j = 65535 - (int)(key & 65535);
        const int rs = align[((size_t)i * M + j) * 3 + 1] & 1, o = align[((size_t)i * M + j) * 3];
        // the step's transform: the anchor stays, the moved leaf is put where the pair's alignment says
        const bool j_moves = slot[j] == hi;
        const int a = j_moves ? i : j, m = j_moves ? j : i;
        const int wa = widths[a], wm = widths[m];
        const int ro = j_moves ? o : (rs ? widths[i] + o - widths[j] : -o);
        const int fa = flips[a], ha = shifts[a], fm = flips[m], hm = shifts[m];
        const int ft = rs ^ fa;
        const int ht = fa ? ha + wa + ro - wm : ha - ro;
        const int F = ft ^ fm;
        const int H = ht - (F ? -(hm + wm) : hm);
        if (tid == 0) {
            *n_list = 0;
            int32_t* rec = log + (size_t)t * 8;
            rec[0] = lo; rec[1] = hi; rec[2] = nlo + nhi; rec[3] = i; rec[4] = j; rec[5] = F; rec[6] = H; rec[7] = 0;
            link[(size_t)t * 2] = s;
            link[(size_t)t * 2 + 1] = avg ? (int64_t)nlo * nhi : 1;
            gone[hi] = t;
        }
        __syncthreads();

        // a lane owns M / 1024 leaves and slots; it reads four of them at a time so that the trips through
        // global memory overlap (a step is bound by them)
        for (int y0 = tid; y0 < M; y0 += MT_BATCH * MT_THREADS) {
            int sl[MT_BATCH];
#pragma unroll
            for (int u = 0; u < MT_BATCH; ++u) {
                const int y = y0 + u * MT_THREADS;
                sl[u] = y < M ? slot[y] : -1;
            }
#pragma unroll
            for (int u = 0; u < MT_BATCH; ++u) {
                const int y = y0 + u * MT_THREADS;
                if (sl[u] != hi) continue;
                const int f = flips[y], h = shifts[y];
                flips[y] = f ^ F;
                shifts[y] = (F ? -(h + widths[y]) : h) + H;
                slot[y] = lo;
            }
        }
        int64_t* Llo = L + (size_t)lo * M;
        uint64_t* Klo = K + (size_t)lo * M;
        const int64_t* Lhi = L + (size_t)hi * M;
        const uint64_t* Khi = K + (size_t)hi * M;
        double rbv = -INFINITY;                          // row lo's best partner c > lo among this lane's slots
        int rbp = MT_NONE;
        for (int c0 = tid; c0 < M; c0 += MT_BATCH * MT_THREADS) {
            int ncs[MT_BATCH];
            int64_t xs[MT_BATCH], ys[MT_BATCH];
            uint64_t kxs[MT_BATCH], kys[MT_BATCH];
#pragma unroll
            for (int u = 0; u < MT_BATCH; ++u) {         // the rows of a merged slot are read too: harmless
                const int c = c0 + u * MT_THREADS;
                const int cc = c < M ? c : c0;
                ncs[u] = c < M ? size[cc] : 0;
                xs[u] = Llo[cc];
                ys[u] = Lhi[cc];
                kxs[u] = Klo[cc];
                kys[u] = Khi[cc];
            }
#pragma unroll
            for (int u = 0; u < MT_BATCH; ++u) {
                const int c = c0 + u * MT_THREADS;
                const int nc = ncs[u];
                if (c == lo || c == hi || nc == 0) continue;
                const int64_t x = xs[u], y = ys[u];
                const int64_t n = linkage == EXPLAINN_LINKAGE_AVERAGE ? x + y
                                  : linkage == EXPLAINN_LINKAGE_SINGLE ? (x > y ? x : y) : (x < y ? x : y);
                const uint64_t kn = kxs[u] > kys[u] ? kxs[u] : kys[u];
                Llo[c] = n;
                L[(size_t)c * M + lo] = n;
                Klo[c] = kn;
                K[(size_t)c * M + lo] = kn;
                const double v = mt_value(n, nc, nlo + nhi, avg);      // the new linkage of (lo, c)
                if (c > lo && v > rbv) { rbv = v; rbp = c; }           // c ascends: the first maximum stays
                if (c < hi) {
                    const int p = part[c];
                    if (p == lo || p == hi) {
                        list[atomicAdd(n_list, 1)] = (uint16_t)c;
                    } else if (c < lo) {
                        const double cur = val[c];
                        if (v > cur || (v == cur && lo < p)) { val[c] = v; part[c] = (uint16_t)lo; }
                    }
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(rbv, off, 64);
            const int op = __shfl_xor(rbp, off, 64);
            if (ov > rbv || (ov == rbv && op < rbp)) { rbv = ov; rbp = op; }
        }
        if (lane == 0) {                                 // the argmax read rv, rc before this step's first barrier
            rv[wave] = rbv;
            rc[wave] = rbp;
        }
        if (tid == 0) {
            size[lo] = nlo + nhi;
            size[hi] = 0;
            val[hi] = -INFINITY;
            part[hi] = (uint16_t)MT_NONE;
        }
        __syncthreads();

        if (tid == 0) {                                  // row lo's cache entry from the waves' partials
            double bv = rv[0];
            int bp = rc[0];
            for (int k = 1; k < MT_WAVES; ++k)
                if (rv[k] > bv || (rv[k] == bv && rc[k] < bp)) { bv = rv[k]; bp = rc[k]; }
            val[lo] = bv;
            part[lo] = (uint16_t)bp;
        }
        const int n = *n_list;
        int nseg = 1;                                    // a short list: several waves share a row
        while (n > 0 && nseg * 2 * n <= MT_WAVES) nseg *= 2;
        if (nseg == 1) {
            for (int k = wave; k < n; k += MT_WAVES) mt_scan_row(list[k], M, L, size, avg, lane, val, part);
        } else {                                         // uniform over the workgroup: n is
            const int k = wave / nseg, seg = wave % nseg;
            if (k < n) {
                double bv;
                int bp;
                mt_scan_part(list[k], M, L, size, avg, lane, seg, nseg, bv, bp);
                if (lane == 0) {
                    pv[wave] = bv;
                    pc[wave] = bp;
                }
            }
            __syncthreads();
            if (k < n && seg == 0 && lane == 0) {
                double bv = pv[wave];
                int bp = pc[wave];
                for (int g = 1; g < nseg; ++g)
                    if (pv[wave + g] > bv || (pv[wave + g] == bv && pc[wave + g] < bp)) { bv = pv[wave + g]; bp = pc[wave + g]; }
                val[list[k]] = bv;
                part[list[k]] = (uint16_t)bp;
            }
        }
        __syncthreads();
        if (t == M - 2) break;
        lo = mt_argmax(M, size, val, part, rv, rc, tid, lane, wave);
    }
}

__global__ __launch_bounds__(256) void motif_tree_cut_init_kernel(int M, int32_t* __restrict__ slot_lo,
                                                                  int32_t* __restrict__ slot_hi) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= M) return;
    slot_lo[c] = 0x7fffffff;
    slot_hi[c] = (int32_t)0x80000000;
}

__global__ __launch_bounds__(256) void motif_tree_cut_walk_kernel(
    const int32_t* __restrict__ log, const int64_t* __restrict__ link, const int32_t* __restrict__ gone,
    const int32_t* __restrict__ widths, int M, int64_t thr, int32_t* __restrict__ labels, int32_t* __restrict__ flips,
    int32_t* __restrict__ shifts, int32_t* slot_lo, int32_t* slot_hi) {
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= M) return;
    const int w = widths[y];
    int c = y, f = 0, h = 0;
    for (int guard = 0; guard < M; ++guard) {            // a chain holds at most M - 1 steps
        const int t = gone[c];
        if (t < 0 || t >= M - 1) break;
        if (link[(size_t)t * 2] < thr * link[(size_t)t * 2 + 1]) break;
        const int32_t* rec = log + (size_t)t * 8;
        const int next = rec[0];
        if (next < 0 || next >= M) break;                // not a log of this tree
        const int F = rec[5] & 1;
        f ^= F;
        h = (F ? -(h + w) : h) + rec[6];
        c = next;
    }
    labels[y] = c;
    flips[y] = f;
    shifts[y] = h;
    atomicMin(&slot_lo[c], h);
    atomicMax(&slot_hi[c], h + w);
}

__global__ __launch_bounds__(256) void motif_tree_cut_norm_kernel(const int32_t* __restrict__ labels, int M,
                                                                  const int32_t* __restrict__ slot_lo,
                                                                  int32_t* __restrict__ shifts) {
    const int y = blockIdx.x * 256 + threadIdx.x;
    if (y >= M) return;
    shifts[y] -= slot_lo[labels[y]];
}

__global__ __launch_bounds__(MT_POOL_THREADS) void motif_tree_pool_kernel(
    const float* __restrict__ x, const int32_t* __restrict__ widths, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ flips, const int32_t* __restrict__ shifts, const int32_t* __restrict__ cluster_slots,
    int M, int wmax, int span, double* __restrict__ merged, int32_t* __restrict__ support) {
    const int c = blockIdx.x;
    const int s = cluster_slots[c];
    for (int e = threadIdx.x; e < span * 4; e += MT_POOL_THREADS) {
        const int col = e >> 2, a = e & 3;
        double acc = 0.0;
        int n = 0;
        for (int y = 0; y < M; ++y) {
            if (labels[y] != s) continue;
            int w = widths[y];
            if (w < 0 || w > wmax) w = 0;
            const int cc = col - shifts[y];
            if (cc < 0 || cc >= w) continue;
            const float* m = x + (size_t)y * wmax * 4;
            acc += (double)((flips[y] & 1) ? m[(w - 1 - cc) * 4 + 3 - a] : m[cc * 4 + a]);
            ++n;
        }
        merged[((size_t)c * span + col) * 4 + a] = acc;
        if (a == 0) support[(size_t)c * span + col] = n;
    }
}

inline bool mt_linkage_ok(int linkage) {
    return linkage == EXPLAINN_LINKAGE_SINGLE || linkage == EXPLAINN_LINKAGE_COMPLETE ||
           linkage == EXPLAINN_LINKAGE_AVERAGE;
}

}  // namespace

extern "C" int64_t explainn_motif_tree_workspace_bytes(int M, int linkage) {
    if (M < 0 || M > EXPLAINN_MOTIF_TREE_MAX_LEAVES || !mt_linkage_ok(linkage)) return 0;
    Carver dry;
    mt_pieces w;
    mt_workspace(dry, M, &w);
    return dry.bytes();
}

extern "C" int explainn_motif_tree(const float* ncor, const int16_t* align, const int32_t* widths, int M, int linkage,
                                   int32_t* log, int64_t* link, int32_t* gone, int32_t* flips, int32_t* shifts,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    if (M < 0 || !mt_linkage_ok(linkage)) {
        explainn_set_error("motif_tree: need M >= 0 and a linkage of EXPLAINN_LINKAGE_* (M=%d linkage=%d)", M, linkage);
        return EXPLAINN_E_ARG;
    }
    if (M > EXPLAINN_MOTIF_TREE_MAX_LEAVES) {
        explainn_set_error("motif_tree: %d motifs exceed %d (the per-slot cache of the one-workgroup loop is in LDS)",
                           M, EXPLAINN_MOTIF_TREE_MAX_LEAVES);
        return EXPLAINN_E_UNSUPPORTED;
    }
    if (M == 0) return EXPLAINN_OK;
    if (!ncor || !align || !widths || !gone || !flips || !shifts || (M > 1 && (!log || !link))) {
        explainn_set_error("motif_tree: ncor, align, widths, log, link, gone, flips, shifts must be device pointers");
        return EXPLAINN_E_ARG;
    }
    Carver cv(workspace);
    mt_pieces w;
    mt_workspace(cv, M, &w);
    if (!workspace_ok("motif_tree", workspace, workspace_bytes, cv.bytes(), 16)) return EXPLAINN_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = (int64_t)M * M;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(motif_tree_prepare_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s,
                       ncor, M, total, w.L, w.K);
    LAUNCH_CHECK();
    const size_t lds = mt_lds_bytes(M);
    if (lds > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&motif_tree_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mt_lds_bytes(EXPLAINN_MOTIF_TREE_MAX_LEAVES)));
    hipLaunchKernelGGL(motif_tree_kernel, dim3(1), dim3(MT_THREADS), lds, s, align, widths, M, linkage, w.L, w.K,
                       w.size, w.slot, log, link, gone, flips, shifts);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

extern "C" int explainn_motif_tree_cut(const int32_t* log, const int64_t* link, const int32_t* gone,
                                       const int32_t* widths, int M, int threshold, int32_t* labels, int32_t* flips,
                                       int32_t* shifts, int32_t* slot_lo, int32_t* slot_hi, void* stream) {
    if (M < 0 || threshold < 1) {
        explainn_set_error("motif_tree_cut: need M >= 0 and a threshold of at least 1 (M=%d threshold=%d)", M,
                           threshold);
        return EXPLAINN_E_ARG;
    }
    if (M == 0) return EXPLAINN_OK;
    if (!gone || !widths || !labels || !flips || !shifts || !slot_lo || !slot_hi || (M > 1 && (!log || !link))) {
        explainn_set_error("motif_tree_cut: log, link, gone, widths and the outputs must be device pointers");
        return EXPLAINN_E_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((M + 255) / 256));
    hipLaunchKernelGGL(motif_tree_cut_init_kernel, grid, dim3(256), 0, s, M, slot_lo, slot_hi);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(motif_tree_cut_walk_kernel, grid, dim3(256), 0, s, log, link, gone, widths, M,
                       (int64_t)threshold, labels, flips, shifts, slot_lo, slot_hi);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(motif_tree_cut_norm_kernel, grid, dim3(256), 0, s, labels, M, slot_lo, shifts);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

extern "C" int explainn_motif_tree_pool(const float* x, const int32_t* widths, const int32_t* labels,
                                        const int32_t* flips, const int32_t* shifts, const int32_t* cluster_slots,
                                        int M, int wmax, int C, int span, double* merged, int32_t* support,
                                        void* stream) {
    if (M < 0 || C < 0 || C > M || span < 0 || wmax < 1 || wmax > EXPLAINN_MOTIF_MAX_WIDTH ||
        (int64_t)span * 4 > 0x7fffffffLL) {
        explainn_set_error("motif_tree_pool: need 0 <= C <= M, span >= 0, 1 <= wmax <= %d (M=%d C=%d span=%d wmax=%d)",
                           EXPLAINN_MOTIF_MAX_WIDTH, M, C, span, wmax);
        return EXPLAINN_E_ARG;
    }
    if (C == 0 || span == 0) return EXPLAINN_OK;
    if (!x || !widths || !labels || !flips || !shifts || !cluster_slots || !merged || !support) {
        explainn_set_error("motif_tree_pool: every array must be a device pointer");
        return EXPLAINN_E_ARG;
    }
    hipLaunchKernelGGL(motif_tree_pool_kernel, dim3((unsigned)C), dim3(MT_POOL_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, widths, labels, flips, shifts, cluster_slots, M, wmax, span,
                       merged, support);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
