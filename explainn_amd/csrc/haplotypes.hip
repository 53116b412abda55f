// Scoring haplotypes ("Haplotypes"): several variants per window.
//
//   stage_haplotypes   a device-resident sequence of base codes, a row table, an index list and an edit
//                      table -> the packed batch whose row b is L bases of the haplotype that carries
//                      the row's run of edits, in the layouts pack_onehot_kernel<true> writes for the
//                      materialised (B,L) matrix
//
// Row b carries the edits e_i = edit_index[row_first[b] + i], i < row_count[b], ordered and
// non-overlapping (pos[e_i] + ref_len[e_i] <= pos[e_{i+1}]):
//     H = seq[:pos_0] + alt_0 + seq[pos_0 + ref_0 : pos_1] + alt_1 + ... + seq[pos_{c-1} + ref_{c-1}:]
// and the row is H[row_start : row_start + L].  With after_i = sum_{m<=i} (alt_len_m - ref_len_m), the
// shift behind edit i, and hstart_i = pos_i + after_{i-1}, where edit i begins in H (nondecreasing),
// haplotype offset g reads
//     seq[g]                           g < hstart_0
//     alt[alt_off_i + g - hstart_i]    hstart_i <= g < hstart_i + alt_len_i
//     seq[g - after_i]                 otherwise, i the last edit with hstart_i <= g
// which is edit_source (stage_tile.h); stage_edits_kernel (variants.hip) calls it with its one edit.
#include "common.h"
#include "stage_tile.h"

namespace {
// a wave's own LDS strip is written by its lanes and read across them: LDS operations of one wave
// complete in order, so all that is needed is that the compiler keeps them in order
__device__ __forceinline__ void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ long long lane_i64(long long v, int l) {         // lane l's value, wave-uniform
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v & 0xffffffffu), l);
    const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
}  // namespace

// stage_edits_kernel's shape: a block is 64 rows x 64 positions, a wave owns 8 rows and reads their
// tables wave-uniformly.  A row's run is walked in chunks of 64 edits, lane i holding edit c0 + i: the
// lanes validate their edits, a wave prefix sum of alt_len - ref_len (plus the carry of the chunks
// before) gives every edit's hstart and the shift behind it, and the chunk is parked in the wave's LDS
// strip, where every lane (= output position) binary-searches the last edit with hstart <= g.  hstart
// is nondecreasing along the run, so a later chunk's hit overrides an earlier one.  The whole run is
// walked by every tile of the row: a bad edit anywhere in it makes the whole row N, in every tile.
// Only then is the row's one source address per lane known; the byte loads of a wave's 8 rows are
// issued together at the end.
__global__ __launch_bounds__(64 * SW_WAVES) void stage_haplotypes_kernel(
    const uint8_t* __restrict__ seq, long long seq_len, explainn_haplotypes hp, long long row0, int rc,
    uint8_t* __restrict__ codesT, uint32_t* __restrict__ pk2, uint32_t* __restrict__ nmask, int B, int L,
    int Bs, int PW, int NW, int* __restrict__ flags, unsigned long long* __restrict__ bm, int Lp) {
    constexpr int ROWS = SW_ROWS;
    __shared__ uint8_t tile[64][68];
    __shared__ long long run_h[SW_WAVES][64];        // hstart of the chunk's edits
    __shared__ long long run_s[SW_WAVES][64];        // the shift behind each of them
    __shared__ int run_al[SW_WAVES][64];
    __shared__ int run_ao[SW_WAVES][64];
    const stage_front f = stage_front_of(rc, L);
    const int b0 = f.b0, lane = f.lane, q = f.q;
    int bad = 0;
    // the tables of the wave's 8 rows in one load: lane r holds row r's, read back lane by lane below
    long long start_v = 0, first_v = 0;
    int count_v = 0;
    if (lane < ROWS && b0 + q + SW_WAVES * lane < B) {
        const long long row = row0 + b0 + q + SW_WAVES * lane;
        start_v = hp.row_start[row]; first_v = hp.row_first[row]; count_v = hp.row_count[row];
    }
    const uint8_t* src[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {                 // (unrolled: src[] stays in registers)
        const int b = b0 + q + SW_WAVES * r;
        src[r] = nullptr;
        if (b >= B) continue;                        // (wave-uniform)
        const int cnt = __builtin_amdgcn_readlane(count_v, r);
        const long long fst = lane_i64(first_v, r);
        // a table the host never saw: nothing of it becomes an address before it is range-checked, and
        // whatever fails makes the whole row N and raises the flag.  The run must lie inside edit_index
        bool ok = cnt >= 0 && fst >= 0 && cnt <= hp.n_index && fst <= hp.n_index - cnt;
        const long long g = wadd(lane_i64(start_v, r), f.hq);
        bool have = false;                           // an edit with hstart <= g exists: the last such is
        long long sel_h = 0, sel_s = 0;              // ... at sel_h, with shift sel_s behind it,
        int sel_al = 0, sel_ao = 0;                  // ... and these alt bases
        if (ok) {                                    // (wave-uniform)
            long long carry = 0, last_pos = 0;
            int last_rl = 0;
            for (long long c0 = 0; c0 < cnt; c0 += 64) {
                const int n = cnt - c0 < 64 ? (int)(cnt - c0) : 64;
                long long pos = 0;
                int rl = 0, al = 0, ao = 0;
                if (lane < n && !load_edit(hp, hp.edit_index[fst + c0 + lane], pos, rl, al, ao)) ok = false;
                // ordered and non-overlapping: the edit before (the neighbouring lane's, or the last of
                // the chunk before) ends at or before this one's pos.  prev <= pos makes the difference
                // exact as an unsigned number, whatever the positions are
                long long prev = __shfl_up(pos, 1);
                int prev_rl = __shfl_up(rl, 1);
                if (lane == 0) { prev = last_pos; prev_rl = last_rl; }
                if (lane < n && (lane > 0 || c0 > 0) &&
                    !(prev <= pos && (unsigned long long)wsub(pos, prev) >= (unsigned long long)prev_rl))
                    ok = false;
                // after = the shift behind the edit: inclusive wave prefix sum of alt_len - ref_len
                // (0 in the lanes past the run) on top of the chunks before
                const long long delta = (long long)al - rl;
                const long long after = wadd(wave_scan_up(delta, lane), carry);
                wave_lds_order();                    // the searches of the chunk before are done
                run_h[q][lane] = wadd(pos, wsub(after, delta));
                run_s[q][lane] = after;
                run_al[q][lane] = al;
                run_ao[q][lane] = ao;
                wave_lds_order();
                if (run_h[q][0] <= g) {
                    int j = 0;                       // the last edit of the chunk with hstart <= g
#pragma unroll
                    for (int step = 32; step > 0; step >>= 1)
                        if (j + step < n && run_h[q][j + step] <= g) j += step;
                    have = true;
                    sel_h = run_h[q][j]; sel_s = run_s[q][j]; sel_al = run_al[q][j]; sel_ao = run_ao[q][j];
                }
                carry = __shfl(after, 63);
                last_pos = __shfl(pos, n - 1);
                last_rl = __shfl(rl, n - 1);
            }
        }
        const bool row_ok = !__any(!ok);            // (voted by the whole wave, outside the p < L branch)
        if (f.p < L) {
            if (!row_ok) bad = 1;
            else src[r] = edit_source(seq, seq_len, hp.alt, g, have, sel_h, sel_s, sel_al, sel_ao);
        }
    }
    int v[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) v[r] = src[r] ? *src[r] : 4;
    stage_rows_codes(tile, f, v, rc, B, L, bad);
    stage_tile_finish(tile, f, bad, codesT, pk2, nmask, B, L, Bs, PW, NW, flags, bm, Lp);
}

int launch_stage_haplotypes(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const explainn_haplotypes* hp,
                            int64_t row0, int B, int rc, hipStream_t s) {
    return launch_stage_rows(c, stage_haplotypes_kernel, B, s, seq, (long long)seq_len, *hp, (long long)row0, rc);
}
