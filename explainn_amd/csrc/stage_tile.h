// Both halves of the kernels that stage a batch of base codes out of a device-resident sequence
// (scan.hip: stage_windows, variants.hip: stage_edits, haplotypes.hip: stage_haplotypes).  A block is
// 64 rows x 64 positions; a wave owns the rows q, q + 8, ... and a lane one position of each.
//   front   stage_front_of: the block's tile, the thread's wave and lane, and hq, the offset inside
//           its row that the lane's output position reads (the reverse complement reads backwards)
//   middle  the kernel's own: where byte hq of row b lives.  Rows with edits share load_edit and
//           edit_source
//   back    stage_rows_codes: the bytes read -> codes in the LDS tile; stage_tile_finish: the tile
//           -> codesT, pk2, nmask, bm and the flag
// The back must write exactly what pack_tile<true> (pack.hip) writes for the materialised (B,L) matrix;
// stage_tile_store is that function's second half, on the same tile.
#pragma once
#include "common.h"

#define SW_WAVES 8                  // wavefronts per staging block (64 rows x 64 positions), as PACK_WAVES
#define SW_ROWS (64 / SW_WAVES)     // rows of the block a wave owns

struct stage_front {
    int bx, b0, p0;                 // the block, its first row and first position
    int lane, q;                    // q is wave-uniform: row tables are read once per wave
    int p;                          // the lane's output position
    long long hq;                   // ... and the offset inside the row that it reads
};

__device__ __forceinline__ stage_front stage_front_of(int rc, int L) {
    stage_front f;
    f.bx = blockIdx.x; f.b0 = f.bx * 64; f.p0 = blockIdx.y * 64;
    f.lane = threadIdx.x & 63;
    f.q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    f.p = f.p0 + f.lane;
    f.hq = rc ? (long long)L - 1 - f.p : (long long)f.p;
    return f;
}

__device__ __forceinline__ long long wadd(long long a, long long b) {      // wrapping, never undefined
    return (long long)((unsigned long long)a + (unsigned long long)b);
}
__device__ __forceinline__ long long wsub(long long a, long long b) {
    return (long long)((unsigned long long)a - (unsigned long long)b);
}

// Edit e of an explainn_edits or explainn_haplotypes (the edit-table fields have one name in both).
// A table the host never saw: an index outside the table, a negative length or an alt run that leaves
// the pool returns false, with all four zero; nothing of such a record becomes an address.
template <class Tables>
__device__ __forceinline__ bool load_edit(const Tables& t, int e, long long& pos, int& rl, int& al, int& ao) {
    bool ok = e >= 0 && e < t.n_edits;
    if (ok) {
        pos = t.pos[e]; rl = t.ref_len[e]; al = t.alt_len[e]; ao = t.alt_off[e];
        ok = rl >= 0 && al >= 0 && ao >= 0 && (long long)ao + al <= t.alt_bytes;
    }
    if (!ok) { pos = 0; rl = 0; al = 0; ao = 0; }
    return ok;
}

// The one source address of haplotype offset g, or null where it reads outside the sequence (N, not
// flagged).  have: an edit begins at or before g; the last such begins at hstart (on the haplotype),
// has alt bases alt[ao : ao + al] and the shift `shift` behind it.  A single edit has hstart = pos and
// shift = al - rl.  Wrapping arithmetic: a wild start or pos must not be undefined, and every index is
// range-checked before it is used.
__device__ __forceinline__ const uint8_t* edit_source(const uint8_t* seq, long long seq_len, const uint8_t* alt,
                                                      long long g, bool have, long long hstart, long long shift,
                                                      int al, int ao) {
    const long long d = wsub(g, hstart);
    if (have && d >= 0 && d < al) return alt + ao + d;
    const long long t = have ? wsub(g, shift) : g;
    return t >= 0 && t < seq_len ? seq + t : nullptr;
}

// a byte read from the sequence or the alt pool -> its code: complemented under rc, 4 = N, any other
// value is N too and raises bad
__device__ __forceinline__ uint8_t stage_code(int v, int rc, int& bad) {
    if (v < 4) return rc ? 3 - v : v;
    if (v != 4) bad = 1;
    return 4;
}

// v[r] is the byte row q + SW_WAVES*r reads at the lane's position (4 where it reads none) -> the tile
__device__ __forceinline__ void stage_rows_codes(uint8_t (&tile)[64][68], const stage_front& f,
                                                 const int (&v)[SW_ROWS], int rc, int B, int L, int& bad) {
#pragma unroll
    for (int r = 0; r < SW_ROWS; ++r) {
        const int i = f.q + SW_WAVES * r;
        // padding lanes / past the end: 'A', as pack_tile
        tile[i][f.lane] = (f.b0 + i < B && f.p < L) ? stage_code(v[r], rc, bad) : 0;
    }
}

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

// every wave has written its rows of the tile: the barrier, the stores, the flag
__device__ __forceinline__ void stage_tile_finish(
    const uint8_t (&tile)[64][68], const stage_front& f, int bad, uint8_t* __restrict__ codesT,
    uint32_t* __restrict__ pk2, uint32_t* __restrict__ nmask, int B, int L, int Bs, int PW, int NW,
    int* __restrict__ flags, unsigned long long* __restrict__ bm, int Lp) {
    __syncthreads();
    stage_tile_store(tile, f.lane, f.q, f.bx, f.b0, f.p0, codesT, pk2, nmask, B, L, Bs, PW, NW, bm, Lp);
    if (bad) atomicOr(flags, 1);
}

// The launch of a staging kernel: `head` are the kernel's own leading arguments (the sequence, its row
// source, rc); the batch's arrays follow in every kernel alike.
template <class Kernel, class... Head>
int launch_stage_rows(explainn_ctx* c, Kernel kernel, int B, hipStream_t s, Head... head) {
    hipLaunchKernelGGL(kernel, dim3((B + 63) / 64, (c->NW * 32 + 63) / 64), dim3(64 * SW_WAVES), 0, s, head...,
                       c->codesT, c->pk2, c->nmask, B, c->L, c->Bs, c->PW, c->NW, c->flags, c->bm, c->Lp);
    LAUNCH_CHECK();
    c->staged_B = B;
    return EXPLAINN_OK;
}
