// The two scans between the COUNT and the EMIT pass of a site caller (sites.hip: filter sites,
// pwmsites.hip: known-motif sites): per row the exclusive scan of its per-tile counts, then the exclusive
// scan of the rows' totals.  A row is whatever the caller lists separately (a unit; a (motif, strand)).
// Integer adds in tile and row order: no rank depends on the order anything arrives in.
#pragma once
#include "common.h"

namespace {

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

}  // namespace
