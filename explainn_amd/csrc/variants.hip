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
    const stage_front f = stage_front_of(rc, L);
    int bad = 0;
    int v[SW_ROWS];
#pragma unroll
    for (int r = 0; r < SW_ROWS; ++r) {
        const int b = f.b0 + f.q + SW_WAVES * r;
        v[r] = 4;
        if (b < B) {                                 // (wave-uniform)
            const long long start = ed.row_start[row0 + b];
            const int e = ed.row_edit[row0 + b];
            long long pos = 0;
            int rl = 0, al = 0, ao = 0;
            // a bad edit makes the whole row N and raises the flag; no edit is the edit of nothing
            const bool ok = e < 0 || load_edit(ed, e, pos, rl, al, ao);
            if (f.p < L) {
                if (!ok) {
                    bad = 1;
                } else {
                    const long long g = wadd(start, f.hq);
                    const uint8_t* src = edit_source(seq, seq_len, ed.alt, g, g >= pos, pos, (long long)al - rl, al, ao);
                    if (src) v[r] = *src;
                }
            }
        }
    }
    stage_rows_codes(tile, f, v, rc, B, L, bad);
    stage_tile_finish(tile, f, bad, codesT, pk2, nmask, B, L, Bs, PW, NW, flags, bm, Lp);
}

int launch_stage_edits(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const explainn_edits* ed,
                       int64_t row0, int B, int rc, hipStream_t s) {
    return launch_stage_rows(c, stage_edits_kernel, B, s, seq, (long long)seq_len, *ed, (long long)row0, rc);
}
