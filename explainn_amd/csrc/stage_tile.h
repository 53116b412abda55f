// The back half of the kernels that stage a batch of base codes out of a device-resident sequence
// (scan.hip: stage_windows, variants.hip: stage_edits): a block's 64 rows x 64 positions tile of codes
// in LDS -> codesT, pk2, nmask, bm.  Must write exactly what pack_tile<true> (pack.hip) writes for the
// materialised (B,L) matrix; this is that function's second half, on the same tile.
#pragma once
#include "common.h"

#define SW_WAVES 8          // wavefronts per staging block (64 rows x 64 positions), as PACK_WAVES

// tile[row][position] is complete (the caller has synchronised): rows b0.., positions p0.. of block bx
__device__ __forceinline__ void stage_tile_store(
    const uint8_t (&tile)[64][68], int lane, int q, int bx, int b0, int p0, uint8_t* __restrict__ codesT,
    uint32_t* __restrict__ pk2, uint32_t* __restrict__ nmask, int B, int L, int Bs, int PW, int NW,
    unsigned long long* __restrict__ bm, int Lp) {
    for (int pp = q; pp < 64; pp += SW_WAVES) {
        const int po = p0 + pp;
        if (po < L) codesT[(size_t)po * Bs + b0 + lane] = tile[lane][pp];
    }
    if (q < 4) {
        uint32_t w2 = 0, nm = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = tile[lane][16 * q + i];
            w2 |= (c > 3u ? 1u : c) << (2 * i);
        }
        const int wi = (p0 >> 4) + q;
        if (wi < PW) pk2[(size_t)wi * Bs + b0 + lane] = w2;
        if (q < 2) {
#pragma unroll
            for (int i = 0; i < 32; ++i) nm |= (tile[lane][32 * q + i] > 3u ? 1u : 0u) << i;
            const int ni = (p0 >> 5) + q;
            if (ni < NW) nmask[(size_t)ni * Bs + b0 + lane] = nm;
        }
    }
    if (bm != nullptr && q >= SW_WAVES - 4) {
        const int qq = q - (SW_WAVES - 4);
        const bool live = b0 + lane < B;
        unsigned long long mine = 0ull;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = tile[lane][16 * qq + i];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const unsigned long long bal = __ballot(live && c == (uint32_t)a);
                mine = (lane == 16 * a + i) ? bal : mine;
            }
        }
        const int a = lane >> 4, pq = p0 + 16 * qq + (lane & 15);
        if (pq < Lp) bm[((size_t)a * ((B + 63) / 64) + bx) * Lp + pq] = mine;
    }
}
