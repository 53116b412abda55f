// The COUNT / scan / EMIT scheme of a site caller (sites.hip: filter sites, pwmsites.hip: known-motif
// sites; DESIGN.md section 8, "Motif sites").  A row is whatever the caller lists separately (a unit; a
// (motif, strand)); a block of the caller's kernel handles one tile of EXPLAINN_SITES_TILE start positions
// for four consecutive rows at a time.  Two passes of that kernel recompute the hits instead of storing them:
//   COUNT  sites per (row, tile)                                             -> cnt[row][tile]
//   scan   per row: exclusive scan of cnt over the tiles (in place), total   -> tot[row]
//          then offsets[row] = exclusive scan of tot over the rows (int64, [rows + 1])
//   EMIT   rank = offsets[row] + cnt[row][tile] + rank inside the tile (ballots and popcounts in thread =
//          position order); records with rank >= capacity are dropped
// so per row the sites ascend in position.  Integer adds in tile, row and thread order: no rank depends on
// the order anything arrives in.  The caller's kernel decides what a hit is; everything that turns hits
// into ranks -- the workspace, the four launches, the tile geometry, the rank rule -- is here.
#pragma once
#include "common.h"
#include "workspace.h"

namespace {

enum { SITES_COUNT = 0, SITES_EMIT = 1 };

// ---- the workspace: cnt int [rows][tiles] | tot int64 [rows] ---------------------------------------
struct SiteWorkspace {
    int* cnt = nullptr;
    long long* tot = nullptr;
    int ntiles = 0;
};

int64_t sites_tiles(int64_t npos) { return (npos + EXPLAINN_SITES_TILE - 1) / EXPLAINN_SITES_TILE; }

SiteWorkspace site_workspace(Carver& cv, int64_t rows, int64_t npos) {
    const int64_t tiles = sites_tiles(npos);
    SiteWorkspace w;
    w.ntiles = (int)tiles;
    cv.take(&w.cnt, rows * tiles);
    cv.take(&w.tot, rows);
    return w;
}

int64_t site_workspace_bytes(int64_t rows, int64_t npos) {
    Carver dry;
    site_workspace(dry, rows, npos);
    return dry.bytes();
}

// ---- the two scans ---------------------------------------------------------------------------------
// One wavefront per row: cnt[r][.] <- its exclusive scan over the tiles, tot[r] <- the row's sites.
// A row has fewer than 2^31 sites (one per position at most), so the in-row prefix stays int.
__global__ __launch_bounds__(64) void sites_scan_tiles_kernel(int* __restrict__ cnt,
                                                              long long* __restrict__ tot, int ntiles) {
    const int u = blockIdx.x, lane = threadIdx.x;
    int* row = cnt + (size_t)u * ntiles;
    int running = 0;
    for (int b0 = 0; b0 < ntiles; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < ntiles ? row[b] : 0;
        const int inc = wave_scan_up(v, lane);
        if (b < ntiles) row[b] = running + (inc - v);
        running += __shfl(inc, 63, 64);
    }
    if (lane == 0) tot[u] = running;
}

// One wavefront: offsets[0 .. U] <- exclusive scan of the rows' totals.
__global__ __launch_bounds__(64) void sites_scan_units_kernel(const long long* __restrict__ tot,
                                                              long long* __restrict__ offsets, int U) {
    const int lane = threadIdx.x;
    long long running = 0;
    for (int u0 = 0; u0 < U; u0 += 64) {
        const int u = u0 + lane;
        const long long v = u < U ? tot[u] : 0;
        const long long inc = wave_scan_up(v, lane);
        if (u < U) offsets[u] = running + (inc - v);
        running += __shfl(inc, 63, 64);
    }
    if (lane == 0) offsets[U] = running;
}

// ---- the driver ------------------------------------------------------------------------------------
// offsets[0 .. rows] of n_positions starts and, with emit, the records.  launch(mode) launches the caller's
// kernel for std::integral_constant<int, SITES_COUNT | SITES_EMIT>; an empty call only zeroes the offsets.
template <typename Launch>
int site_passes(int rows, int64_t n_positions, const SiteWorkspace& w, long long* offsets, bool emit, hipStream_t s,
                Launch launch) {
    if (rows == 0 || n_positions == 0) {
        HIP_TRY(hipMemsetAsync(offsets, 0, (size_t)(rows + 1) * sizeof(long long), s));
        return EXPLAINN_OK;
    }
    launch(std::integral_constant<int, SITES_COUNT>());
    LAUNCH_CHECK();
    hipLaunchKernelGGL(sites_scan_tiles_kernel, dim3(rows), dim3(64), 0, s, w.cnt, w.tot, w.ntiles);
    LAUNCH_CHECK();
    hipLaunchKernelGGL(sites_scan_units_kernel, dim3(1), dim3(64), 0, s, w.tot, offsets, rows);
    LAUNCH_CHECK();
    if (!emit) return EXPLAINN_OK;
    launch(std::integral_constant<int, SITES_EMIT>());
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

}  // namespace

// ---- the position-order rank of a hit --------------------------------------------------------------
// All T threads of the block call it, thread order = position order, for four rows:
// rank[uu] = hits of row uu in the threads below this one, total[uu] = hits of the block.  Ballots and
// popcounts, per-wave totals in wtot (LDS): no rank depends on the order anything arrives in.
template <int T>
__device__ __forceinline__ void block_hit_ranks(const bool (&hit)[4], int (*wtot)[T / 64], int (&rank)[4],
                                                int (&total)[4]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
        const unsigned long long bal = __ballot(hit[uu]);
        rank[uu] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[uu][wave] = __popcll(bal);
    }
    __syncthreads();
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < T / 64; ++w) {
            const int t = wtot[uu][w];
            before += w < wave ? t : 0;
            all += t;
        }
        rank[uu] += before;
        total[uu] = all;
    }
    __syncthreads();                           // wtot is rewritten by the next call
}

// ---- what a caller's kernel does with its tile and its four rows -----------------------------------
// the tile's first start and how many starts it has
__device__ __forceinline__ void site_tile(int tile, int npos, int& t0, int& live_n) {
    t0 = tile * EXPLAINN_SITES_TILE;                        // < npos < 2^31
    live_n = min(EXPLAINN_SITES_TILE, npos - t0);
}

// EMIT: the rank of the tile's first site of rows row0 .. row0 + 3 (a row past `rows` has none)
template <int MODE>
__device__ __forceinline__ void site_bases(const long long* offsets, const int* cnt, int ntiles, int tile,
                                           int row0, int rows, long long (&base)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = row0 + r;
        base[r] = (MODE == SITES_EMIT && row < rows) ? offsets[row] + cnt[(size_t)row * ntiles + tile] : 0;
    }
}

// after block_hit_ranks of one position chunk: EMIT calls store(rank, r) for a hit whose rank the buffers
// hold; run[] counts the tile's sites in the chunks so far.  (A store lambda captures by value: with
// references the kernels take other registers.)
template <int MODE, typename Store>
__device__ __forceinline__ void site_step(const bool (&hit)[4], const int (&pre)[4], const int (&total)[4],
                                          const long long (&base)[4], long long capacity, int (&run)[4],
                                          Store store) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (MODE == SITES_EMIT && hit[r]) {
            const long long rank = base[r] + run[r] + pre[r];
            if (rank < capacity) store(rank, r);
        }
        run[r] += total[r];
    }
}

// COUNT: the tile's sites of rows row0 .. row0 + 3, by threads 0 .. 3
template <int MODE>
__device__ __forceinline__ void site_counts(int* cnt, int ntiles, int tile, int row0, int rows, const int (&run)[4]) {
    const int tid = threadIdx.x;
    if (MODE == SITES_COUNT && tid < 4 && row0 + tid < rows)
        cnt[(size_t)(row0 + tid) * ntiles + tile] = tid == 0 ? run[0] : tid == 1 ? run[1] : tid == 2 ? run[2] : run[3];
}
