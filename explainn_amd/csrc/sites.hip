// Calling motif sites ("Motif sites"): every (unit, start position) of a
// device-resident sequence of base codes whose float16 activation exceeds the unit's threshold, as a
// compacted list -- what the reference gets from the dense float16 (N,U,Lo) activation array with
// np.where (interpret.py:375-429) and writes to sites/filter<u>.fa.
//
// In eval mode BatchNorm1 is folded, so a unit's activation at a position depends only on the k bases
// under it: one gather pass over the codes, tile by tile, lists the hits of every unit without a
// window ever being cut.  The activation is the one definition of codescan.h, which is what makes a
// site here a position where float16(linears[:3]) > threshold, bit for bit.
//
// Block = (tile of SITES_TILE positions, unit quad); a row of sitescan.h's COUNT / scan / EMIT scheme is a
// unit, so per unit the sites ascend in position and no rank depends on the order atomics arrive in.
#include "codescan.h"
#include "sitescan.h"

namespace {

constexpr int SITES_T = 256;
static_assert(EXPLAINN_SITES_TILE % SITES_T == 0, "a tile is a whole number of position chunks");

template <int MODE>
__global__ __launch_bounds__(SITES_T) void sites_kernel(
    const uint8_t* __restrict__ seq, long long start, int npos, long long period, int rc,
    const float* __restrict__ Wt, const float* __restrict__ alpha, const float* __restrict__ shift,
    const float* __restrict__ thr, int* __restrict__ cnt, const long long* __restrict__ offsets,
    int* __restrict__ pos, float* __restrict__ score, long long capacity, int U, int k, int ntiles,
    int* __restrict__ flags) {
    extern __shared__ float4 Wsm[];            // [k][5] | codes [SITES_TILE + k - 1] bytes
    uint8_t* cs = reinterpret_cast<uint8_t*>(Wsm + k * 5);
    __shared__ int wtot[4][SITES_T / 64];
    const int tile = blockIdx.x, quad = blockIdx.y, tid = threadIdx.x;
    int t0, live_n;
    site_tile(tile, npos, t0, live_n);
    const float4* src = reinterpret_cast<const float4*>(Wt) + (size_t)quad * k * 5;
    for (int i = tid; i < k * 5; i += SITES_T) Wsm[i] = src[i];
    // the tile's bases and the k-1 behind its last start: all inside [start, start + npos + k - 1),
    // which the entry point has checked against seq_len.  The reverse strand reads the complement.
    const int bad = stage_codes<false>(seq + start + t0, live_n + k - 1, tid, SITES_T, cs, rc, nullptr);
    if (MODE == SITES_COUNT && quad == 0 && bad) atomicOr(flags, 1);
    float al[4], sh[4], th[4];
    long long base[4];
#pragma unroll
    for (int uu = 0; uu < 4; ++uu) {
        const int u = min(quad * 4 + uu, U - 1);
        al[uu] = alpha[u];
        sh[uu] = shift[u];
        th[uu] = thr[u];
    }
    site_bases<MODE>(offsets, cnt, ntiles, tile, quad * 4, U, base);
    __syncthreads();
    const int first = rc ? k - 1 : 0, step = rc ? -1 : 1;      // (the codes are complemented already)
    int run[4] = {0, 0, 0, 0};                 // sites of this tile in earlier position chunks
    for (int p0 = 0; p0 < live_n; p0 += SITES_T) {
        const int p = p0 + tid;
        bool live = p < live_n;
        // a start whose k-mer would cross the end of its record is never a site
        if (period > 0 && (start + t0 + p) % period > period - k) live = false;
        float a16[4] = {0.f, 0.f, 0.f, 0.f};
        if (live) {
            const uint8_t* const cp[1] = {cs + p + first};
            float4 acc[1];
            tap_chain(Wsm, k, cp, step, acc);
            const float av[4] = {acc[0].x, acc[0].y, acc[0].z, acc[0].w};
#pragma unroll
            for (int uu = 0; uu < 4; ++uu) a16[uu] = act_value(al[uu], av[uu], sh[uu]);
        }
        bool hit[4];
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) hit[uu] = live && a16[uu] > th[uu];
        int pre[4], total[4];
        block_hit_ranks<SITES_T>(hit, wtot, pre, total);
        site_step<MODE>(hit, pre, total, base, capacity, run, [=](long long rank, int uu) {
            if (quad * 4 + uu < U) {
                pos[rank] = t0 + p;
                if (score) score[rank] = a16[uu];
            }
        });
    }
    site_counts<MODE>(cnt, ntiles, tile, quad * 4, U, run);
}

}  // namespace

int64_t sites_workspace_bytes(const explainn_ctx* c, int64_t npos) { return site_workspace_bytes(c->U, npos); }

bool sites_workspace_ok(const explainn_ctx* c, int64_t npos, const void* workspace, int64_t workspace_bytes) {
    return workspace_ok("call_sites", workspace, workspace_bytes, sites_workspace_bytes(c, npos), 256);
}

int launch_call_sites(explainn_ctx* c, const uint8_t* seq, int64_t start, int64_t npos, int64_t period,
                      int rc, const float* thr, int64_t* offsets, int32_t* pos, float* score,
                      int64_t capacity, void* workspace, hipStream_t s) {
    Carver cv(workspace);
    const SiteWorkspace w = site_workspace(cv, c->U, npos);
    long long* off = reinterpret_cast<long long*>(offsets);
    const size_t sm = (size_t)c->k * 5 * sizeof(float4) + ((EXPLAINN_SITES_TILE + c->k - 1 + 15) & ~15);
    return site_passes(c->U, npos, w, off, pos != nullptr && capacity > 0, s, [&](auto mode) {
        hipLaunchKernelGGL(sites_kernel<decltype(mode)::value>, dim3(w.ntiles, c->Uq), dim3(SITES_T), sm, s, seq,
                           (long long)start, (int)npos, (long long)period, rc, c->Wt, c->alpha, c->shift, thr, w.cnt,
                           (const long long*)off, pos, score, (long long)capacity, c->U, c->k, w.ntiles, c->flags);
    });
}
