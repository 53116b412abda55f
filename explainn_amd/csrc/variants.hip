// Scoring sequence variants ("Variant effects").
//
//   stage_edits   a device-resident sequence of base codes, a row table and an edit table -> the packed
//                 batch whose row b is L bases of the haplotype of that row's edit, in the layouts
//                 pack_onehot_kernel<true> writes for the materialised (B,L) matrix -- without the
//                 haplotypes or that matrix ever existing
//
// Edit e replaces seq[pos : pos + ref_len] by alt[alt_off : alt_off + alt_len]:
//     H = seq[:pos] + alt[alt_off : alt_off + alt_len] + seq[pos + ref_len:]
// and a row is H[row_start : row_start + L].  Haplotype offset g therefore reads
//     seq[g]                        g < pos
//     alt[alt_off + g - pos]        pos <= g < pos + alt_len
//     seq[g - alt_len + ref_len]    otherwise
// A row without an edit (row_edit < 0) is the edit of zero bases by zero bases.
#include "common.h"
#include "stage_tile.h"

// Rows have unrelated starts: as in stage_windows' |step| >= 64 branch every wave reads its rows'
// 64-byte runs straight from global memory, one selected address per lane (left flank, alt pool or
// right flank), all of a wave's rows in flight before the first is used.
__global__ __launch_bounds__(64 * SW_WAVES) void stage_edits_kernel(
    const uint8_t* __restrict__ seq, long long seq_len, explainn_edits ed, long long row0, int rc,
    uint8_t* __restrict__ codesT, uint32_t* __restrict__ pk2, uint32_t* __restrict__ nmask, int B, int L,
    int Bs, int PW, int NW, int* __restrict__ flags, unsigned long long* __restrict__ bm, int Lp) {
    __shared__ uint8_t tile[64][68];
    const int bx = blockIdx.x, by = blockIdx.y;
    const int b0 = bx * 64, p0 = by * 64;
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // the row tables are read once per wave
    const int p = p0 + lane;
    // haplotype offset of output position p inside its row: the reverse complement reads the row backwards
    const long long hq = rc ? (long long)L - 1 - p : (long long)p;
    int bad = 0;
    int v[64 / SW_WAVES];
#pragma unroll
    for (int r = 0; r < 64 / SW_WAVES; ++r) {
        const int b = b0 + q + SW_WAVES * r;
        v[r] = 4;
        if (b < B) {                                 // (wave-uniform)
            const long long start = ed.row_start[row0 + b];
            const int e = ed.row_edit[row0 + b];
            long long pos = 0;
            int rl = 0, al = 0, ao = 0;
            // a table the host never saw: an edit index past the table, a negative length or an alt run
            // that leaves the pool makes the whole row N and raises the flag; nothing of it is an address
            bool ok = e < ed.n_edits;
            if (e >= 0 && ok) {
                pos = ed.pos[e]; rl = ed.ref_len[e]; al = ed.alt_len[e]; ao = ed.alt_off[e];
                ok = rl >= 0 && al >= 0 && ao >= 0 && (long long)ao + al <= ed.alt_bytes;
            }
            if (p < L) {
                if (!ok) {
                    bad = 1;
                } else {
                    // wrapping arithmetic: a wild start or pos must not be undefined, and every index
                    // is range-checked before it is used
                    const long long g = (long long)((unsigned long long)start + (unsigned long long)hq);
                    const long long d = (long long)((unsigned long long)g - (unsigned long long)pos);
                    const uint8_t* src = nullptr;
                    if (g < pos) {
                        if (g >= 0 && g < seq_len) src = seq + g;
                    } else if (d >= 0 && d < al) {
                        src = ed.alt + ao + d;
                    } else {
                        const long long t = (long long)((unsigned long long)g - (unsigned long long)al +
                                                        (unsigned long long)rl);
                        if (t >= 0 && t < seq_len) src = seq + t;
                    }
                    if (src) v[r] = *src;            // outside the sequence: N, not flagged
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 64 / SW_WAVES; ++r) {
        const int i = q + SW_WAVES * r, b = b0 + i;
        uint8_t code = 0;                            // padding lanes / past the end: 'A', as pack_tile
        if (b < B && p < L) {
            if (v[r] < 4) code = rc ? 3 - v[r] : v[r];
            else { code = 4; if (v[r] != 4) bad = 1; }
        }
        tile[i][lane] = code;
    }
    __syncthreads();
    stage_tile_store(tile, lane, q, bx, b0, p0, codesT, pk2, nmask, B, L, Bs, PW, NW, bm, Lp);
    if (bad) atomicOr(flags, 1);
}

int launch_stage_edits(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const explainn_edits* ed,
                       int64_t row0, int B, int rc, hipStream_t s) {
    hipLaunchKernelGGL(stage_edits_kernel, dim3((B + 63) / 64, (c->NW * 32 + 63) / 64), dim3(64 * SW_WAVES),
                       0, s, seq, (long long)seq_len, *ed, (long long)row0, rc, c->codesT, c->pk2, c->nmask, B,
                       c->L, c->Bs, c->PW, c->NW, c->flags, c->bm, c->Lp);
    LAUNCH_CHECK();
    c->staged_B = B;
    return EXPLAINN_OK;
}
