// Scoring a long sequence with overlapping windows ("Tiled scan").
//
//   stage_windows   a device-resident sequence of base codes -> the packed batch whose row b is
//                   seq[start0 + b*step : ... + L] (optionally reverse-complemented), in the layouts
//                   pack_onehot_kernel<true> writes for the materialised (B,L) matrix -- without
//                   that matrix ever existing
//   scan_unfold     the pooled track of a run of tiles -> the [u][w][b] layout fc_fwd reads, for a
//                   sub-batch of windows whose stride is a multiple of the pooling width
//
// In eval mode a unit's raw conv sum at a sequence position does not depend on the window around
// it, and MaxPool1d(7,7) puts its grid at the window's start: windows whose starts differ by a
// multiple of 7 share every pooled value of their overlap.  With stride 7m, window i's pooled vector
// is the slice [m*i, m*i + n) of ONE pooled track, which the filter bank computes once, on tiles
// (windows of the same length L placed 7n apart: tile j's pooled value w is track entry n*j + w).
#include "common.h"
#include "stage_tile.h"

// Rows of one block overlap in the sequence when |step| < 64: the bytes the block needs are then one
// run of 63*|step| + 64 <= SW_SEG bytes, read once, coalesced, into LDS.  With |step| >= 64 the rows'
// 64-byte runs are disjoint: each wave reads its rows' runs directly (64 contiguous bytes per load).
#define SW_SEG 4096

// The middle is arithmetic: byte hq of row b is seq[start0 + b*step + hq] (stage_tile.h has both ends).
__global__ __launch_bounds__(64 * SW_WAVES) void stage_windows_kernel(
    const uint8_t* __restrict__ seq, long long seq_len, long long start0, long long step, int rc,
    uint8_t* __restrict__ codesT, uint32_t* __restrict__ pk2, uint32_t* __restrict__ nmask, int B, int L,
    int Bs, int PW, int NW, int* __restrict__ flags, unsigned long long* __restrict__ bm, int Lp) {
    __shared__ uint8_t tile[64][68];
    __shared__ uint8_t seg[SW_SEG];
    const stage_front f = stage_front_of(rc, L);
    int bad = 0;
    const long long astep = step < 0 ? -step : step;
    if (astep < 64) {
        // the block's 64 positions are the run [off0, off0 + 64) of every row's window, ascending
        // (rc = 0) or descending (rc = 1) in the lane: f.hq = off0 + lo_lane
        const long long off0 = rc ? (long long)L - 64 - f.p0 : (long long)f.p0;
        const int lo_lane = rc ? 63 - f.lane : f.lane;
        const int rows = min(64, B - f.b0);
        const long long first = start0 + (long long)f.b0 * step, last = first + (long long)(rows - 1) * step;
        const long long lo = (first < last ? first : last) + off0;
        const int span = (int)((rows - 1) * astep) + 64;
        for (int t = threadIdx.x; t < span; t += 64 * SW_WAVES) {
            const long long g = lo + t;
            seg[t] = (g >= 0 && g < seq_len) ? seq[g] : (uint8_t)4;     // outside the sequence: N, not flagged
        }
        __syncthreads();
        for (int i = f.q; i < 64; i += SW_WAVES) {
            uint8_t code = 0;                           // padding lanes / past the end: 'A', as pack_tile
            if (f.b0 + i < B && f.p < L)
                code = stage_code(seg[(int)(first + (long long)i * step + off0 - lo) + lo_lane], rc, bad);
            tile[i][f.lane] = code;
        }
    } else {
        int v[SW_ROWS];
#pragma unroll
        for (int r = 0; r < SW_ROWS; ++r) {
            const int b = f.b0 + f.q + SW_WAVES * r;
            const long long g = start0 + (long long)b * step + f.hq;
            v[r] = (b < B && f.p < L && g >= 0 && g < seq_len) ? seq[g] : 4;
        }
        stage_rows_codes(tile, f, v, rc, B, L, bad);
    }
    stage_tile_finish(tile, f, bad, codesT, pk2, nmask, B, L, Bs, PW, NW, flags, bm, Lp);
}

int launch_stage_windows(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, int64_t start0, int64_t step,
                         int B, int rc, hipStream_t s) {
    return launch_stage_rows(c, stage_windows_kernel, B, s, seq, (long long)seq_len, (long long)start0,
                             (long long)step, rc);
}

// ---------------------------------------------------------------------------------------------
// Unfold.  The track lives in the caller's workspace as blocks of up to TB tiles, each block in the
// filter bank's own output layout [u][w][Bs] (the filter bank wrote it there): track entry P = n*j + w
// of unit u is blk[j / TB][(u*n + w)*Bs + j % TB].  Window `it` of the track (it counts in the
// direction the tiles were staged) reads P = m*it + w, w = 0..n-1, and lands in column
// it - tlo, or thi - 1 - it when the tiles hold the reverse complement: that strand's window it is
// window NW - 1 - it of the caller's order.
//
// One workgroup per (64 tile columns, unit): the n rows of those columns (plus one column of halo:
// a window starting in the last tile ends in the next) are read along the tile axis -- 256
// contiguous bytes per row -- into LDS in track order, and every window that starts in these tiles
// is written from there, coalesced along the batch axis.
// ---------------------------------------------------------------------------------------------
#define UNF_THREADS 256
#define UNF_COLS 64

__global__ __launch_bounds__(UNF_THREADS) void scan_unfold_kernel(
    const float* __restrict__ track, float* __restrict__ ext, int n, int Bs, int m, int rc, long long tlo,
    long long thi, long long ja0, long long J, int TB, long long blk_elems) {
    extern __shared__ float trk[];                    // [(UNF_COLS + 1) * n], index P - n*ja
    const int u = blockIdx.y, lane = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long long ja = ja0 + (long long)UNF_COLS * blockIdx.x;
    {
        const long long j = ja + lane;
        const float* src = track + (j < J ? (j / TB) * blk_elems + (size_t)u * n * Bs + j % TB : 0);
        for (int r0 = q; r0 < n; r0 += 4 * (UNF_THREADS / 64)) {
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = min(r0 + i * (UNF_THREADS / 64), n - 1);
                v[i] = j < J ? src[(size_t)r * Bs] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + i * (UNF_THREADS / 64);
                if (r < n) trk[lane * n + r] = v[i];
            }
        }
        const long long jh = ja + UNF_COLS;           // the halo column
        for (int r = threadIdx.x; r < n; r += UNF_THREADS)
            trk[UNF_COLS * n + r] = jh < J ? track[(jh / TB) * blk_elems + ((size_t)u * n + r) * Bs + jh % TB] : 0.f;
    }
    __syncthreads();
    // the windows that start in tiles [ja, ja + 64): m*it in [n*ja, n*(ja + 64))
    long long a = (ja * n + m - 1) / m, b = ((ja + UNF_COLS) * n + m - 1) / m;
    a = a > tlo ? a : tlo;
    b = b < thi ? b : thi;
    const int cnt = (int)(b - a);
    if (cnt <= 0) return;
    const int base = (int)(a * m - ja * n);           // track offset of window a's first pooled value
    float* dst = ext + (size_t)u * n * Bs + (rc ? (thi - 1 - a) : (a - tlo));
    for (int w = 0; w < n; ++w) {
        for (int ii = threadIdx.x; ii < cnt; ii += UNF_THREADS) {
            const float v = trk[base + m * ii + w];
            dst[(long long)w * Bs + (rc ? -ii : ii)] = v;
        }
    }
}

// windows [i0, i0 + Bw) of the caller's order out of NWin, stride 7m: track -> c->ext
int launch_scan_unfold(explainn_ctx* c, const float* track, int64_t blk_elems, int64_t J, int TB, int m,
                       int64_t NWin, int64_t i0, int Bw, int rc, hipStream_t s) {
    const long long tlo = rc ? NWin - i0 - Bw : i0, thi = tlo + Bw;
    const long long ja0 = tlo * m / c->n, jlast = (thi - 1) * m / c->n;
    const int groups = (int)((jlast - ja0) / UNF_COLS + 1);
    const size_t sm = (size_t)(UNF_COLS + 1) * c->n * sizeof(float);
    hipLaunchKernelGGL(scan_unfold_kernel, dim3(groups, c->U), dim3(UNF_THREADS), sm, s, track, c->ext, c->n,
                       c->Bs, m, rc, tlo, thi, ja0, (long long)J, TB, (long long)blk_elems);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

// elements of one track block: the filter bank's output array (api.hip, carve: rows up to whole unit
// groups, plus the dump words behind the last row)
int64_t scan_track_block_elems(const explainn_ctx* c) {
    return (int64_t)32 * conv_tiles_padded(c->U, c->k) * c->n * c->Bs + 64;
}

// tiles that cover every pooled value a window of the scan reads
int64_t scan_tiles(const explainn_ctx* c, int64_t n_windows, int m) {
    return ((int64_t)m * (n_windows - 1) + c->n + c->n - 1) / c->n;
}
