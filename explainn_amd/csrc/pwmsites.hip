// Known-motif sites ("Known-motif sites"): where do the motifs of a database occur in
// a device-resident sequence of base codes -- what FIMO lists, and what the reference vendors PWMScan for.
//
// A motif is an integer score table S[w][4], 0 <= S <= bins (the host quantises its log-odds,
// explainn_amd/pwmsites.py), so a site's score is an integer <= w * bins <= 8192 and everything below is exact
// integer work except the null, which is fp64 sums of positive terms in a fixed order:
//
//   explainn_pwm_null   per motif the distribution of the score of a random w-mer drawn iid from the
//                       background, column by column (a gather: one lane per score value, the four bases in
//                       order, no atomics), its tail, and the smallest score whose tail is <= pcut
//   explainn_pwm_sites  every (motif, strand, start) with score >= the motif's threshold, as a compacted
//                       list: the COUNT / scan / EMIT scheme of sitescan.h with one row per (motif, strand)
//   explainn_pwm_score_histogram  per motif the histogram of the scores of ALL live windows, both strands:
//                       what a q-value over every test needs (siteq.hip); the scan's walk, counted in LDS
//
// Scan geometry (a first choice): a workgroup is a tile of EXPLAINN_SITES_TILE starts x a group of
// EXPLAINN_PWM_GROUP motifs.  The tile's codes and the group's tables sit in LDS; a table entry (column j,
// code c) is pwmtab.h's pair word, so one pass over the window's codes, in forward order, scores both
// strands.  Code 4 (N) holds a sentinel so negative in both halves that no sum reaches a threshold >= 0.
#include <limits.h>

#include <algorithm>

#include "codescan.h"
#include "pwmtab.h"
#include "sitescan.h"

namespace {

constexpr int PS_T = 256;                       // one lane per start, four position chunks per tile
constexpr int PS_CHUNKS = EXPLAINN_SITES_TILE / PS_T;
constexpr int PS_G = EXPLAINN_PWM_GROUP;
constexpr int PS_N = -16384;                    // 64 of them stay inside int32; one outweighs 63 x 128
static_assert(EXPLAINN_SITES_TILE % PS_T == 0, "a tile is a whole number of position chunks");
static_assert(PS_G % 2 == 0, "block_hit_ranks ranks four rows = two motifs x two strands at a time");
static_assert(EXPLAINN_MOTIF_MAX_WIDTH * EXPLAINN_MOTIF_MAX_BINS + PS_N < 0, "an N outweighs the rest of a window");

// tab [G][wmax][8] <- the pair words of motifs m0 .. m0 + G - 1 (zero past a motif's width and for an empty
// motif), the sentinel in both halves at code 4, by nthreads threads
__device__ __forceinline__ void stage_pair_tables(const int16_t* __restrict__ S, const int* __restrict__ widths,
                                                  int m0, int G, int M, int wmax, int tid, int nthreads, int* tab) {
    for (int i = tid; i < G * wmax * 8; i += nthreads) {
        const int g = i / (wmax * 8), r = i - g * wmax * 8, j = r >> 3, c = r & 7, m = m0 + g;
        unsigned word = 0;
        const int w = pwm_width(widths, m, M, wmax);
        if (j < w) {
            const int16_t* row = S + (size_t)m * wmax * 4;
            word = c < 4 ? pwm_pair_word(row, w, j, c) : (unsigned)(uint16_t)PS_N | ((unsigned)(uint16_t)PS_N << 16);
        }
        tab[i] = (int)word;
    }
}

// the widest motif that may start at position p of a tile that staged nstage bases: it ends inside the staged
// bases and, with a period, inside its record; 0 past the tile's live_n starts
__device__ __forceinline__ int pwm_start_limit(int p, int live_n, int nstage, long long first, long long period) {
    int l = p < live_n ? nstage - p : 0;
    if (period > 0 && l > 0) l = (int)min((long long)l, period - (first + p) % period);
    return l;
}

template <int MODE>
__global__ __launch_bounds__(PS_T) void pwm_sites_kernel(
    const uint8_t* __restrict__ seq, long long start, int npos, int span, long long period, int both,
    const int16_t* __restrict__ S, const int* __restrict__ widths, const int* __restrict__ thr,
    const double* __restrict__ tail, int tail_stride, int* __restrict__ cnt,
    const long long* __restrict__ offsets, int* __restrict__ pos, int* __restrict__ score,
    double* __restrict__ pvalue, long long capacity, int M, int wmax, int ntiles) {
    extern __shared__ int tab[];               // [PS_G][wmax][8] | codes [SITES_TILE + wmax - 1] bytes
    uint8_t* cs = reinterpret_cast<uint8_t*>(tab + PS_G * wmax * 8);
    __shared__ int wtot[4][PS_T / 64];
    const int tile = blockIdx.x, tid = threadIdx.x, m0 = blockIdx.y * PS_G;
    int t0, live_n;
    site_tile(tile, npos, t0, live_n);
    // the tile's bases and the wmax-1 behind its last start, as far as the sequence goes: span = the bases
    // from `start` to the end of what the call may read, >= npos (the entry point has checked it)
    const int nstage = min(live_n + wmax - 1, span - t0);
    stage_codes<false>(seq + start + t0, nstage, tid, PS_T, cs, 0, nullptr);
    stage_pair_tables(S, widths, m0, PS_G, M, wmax, tid, PS_T, tab);
    // per position chunk: the widest motif that may start at this lane's position
    int lim[PS_CHUNKS];
#pragma unroll
    for (int c = 0; c < PS_CHUNKS; ++c) lim[c] = pwm_start_limit(c * PS_T + tid, live_n, nstage, start + t0, period);
    __syncthreads();
    for (int q = 0; q < PS_G / 2; ++q) {
        const int ma = m0 + 2 * q;             // motifs ma, ma + 1: rows 2 ma .. 2 ma + 3
        if (ma >= M) break;                    // (the same in every thread)
        int w[2], th[2];
        long long base[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            w[i] = pwm_width(widths, ma + i, M, wmax);
            th[i] = ma + i < M ? thr[ma + i] : INT_MAX;
        }
        site_bases<MODE>(offsets, cnt, ntiles, tile, 2 * ma, 2 * M, base);
        int run[4] = {0, 0, 0, 0};             // sites of this tile in earlier position chunks
#pragma unroll
        for (int c = 0; c < PS_CHUNKS; ++c) {
            if (c * PS_T >= live_n) break;
            const int p = c * PS_T + tid;
            // the two motifs walk the window together: one code read serves both, and the two table reads
            // are independent chains; the wider one goes on alone.  wl = 0 where the start is not live.
            const bool live[2] = {w[0] >= 1 && w[0] <= lim[c], w[1] >= 1 && w[1] <= lim[c]};
            const int wl[2] = {live[0] ? w[0] : 0, live[1] ? w[1] : 0};
            const int* tb0 = tab + 2 * q * wmax * 8;
            const int* tb1 = tb0 + wmax * 8;
            const uint8_t* cp = cs + p;            // cp[j] is read for j < max(wl) <= lim[c] only
            int sc[4] = {0, 0, 0, 0};
            int j = 0;
            for (const int wb = min(wl[0], wl[1]); j < wb; ++j) {
                const int code = cp[j], v0 = tb0[j * 8 + code], v1 = tb1[j * 8 + code];
                sc[0] += (int)(short)(v0 & 0xFFFF);
                sc[1] += v0 >> 16;
                sc[2] += (int)(short)(v1 & 0xFFFF);
                sc[3] += v1 >> 16;
            }
            const bool first = wl[0] > wl[1];
            const int* tbw = first ? tb0 : tb1;
            int fw = 0, rw = 0;
            for (const int wa = max(wl[0], wl[1]); j < wa; ++j) {
                const int v = tbw[j * 8 + cp[j]];
                fw += (int)(short)(v & 0xFFFF);
                rw += v >> 16;
            }
            sc[0] += first ? fw : 0;
            sc[1] += first ? rw : 0;
            sc[2] += first ? 0 : fw;
            sc[3] += first ? 0 : rw;
            bool hit[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                hit[2 * i] = live[i] && sc[2 * i] >= th[i];
                hit[2 * i + 1] = live[i] && both && sc[2 * i + 1] >= th[i];
            }
            int pre[4], total[4];
            block_hit_ranks<PS_T>(hit, wtot, pre, total);
            site_step<MODE>(hit, pre, total, base, capacity, run, [=](long long rank, int r) {
                pos[rank] = t0 + p;
                if (score) score[rank] = sc[r];
                if (pvalue)
                    pvalue[rank] = (unsigned)sc[r] < (unsigned)tail_stride
                                       ? tail[(size_t)(ma + (r >> 1)) * tail_stride + sc[r]] : 0.0;
            });
        }
        site_counts<MODE>(cnt, ntiles, tile, 2 * ma, 2 * M, run);
    }
}

// ---- the observed score histogram --------------------------------------------------------------------
// hist[m][s] += the live windows of motif m, on either requested strand, whose integer score is s: every test
// the scan above would make, not only the sites -- what a q-value over all tests needs (siteq.hip).
//
// Geometry (a first choice): block = (motif group, slice).  A group is G motifs, G chosen by the entry point
// so that G rows of wmax bins + 2 uint32 bins, the group's pair-word tables and one tile's codes fit the LDS;
// the tiles of EXPLAINN_SITES_TILE starts are dealt round robin to the slices.  One lane per start, PH_Q motifs
// at a time: the walk is pwm_sites_kernel's (pair words, the N sentinel), the count an integer LDS atomic.
// A block flushes its non-zero bins once, with 64-bit integer global atomics.  Integers throughout: the
// result does not depend on G, on the slices or on how a caller chunks the sequence.
constexpr int PH_T = EXPLAINN_SITES_TILE;      // one lane per start of a tile
constexpr int PH_Q = 4;                        // motifs a lane walks together
constexpr int PH_BLOCKS = 1024;                // slices are cut so that a call has about this many blocks
constexpr int PH_LDS = 160 * 1024;
constexpr int PH_SLICE_TILES = EXPLAINN_PWM_HIST_SLICE / EXPLAINN_SITES_TILE;
static_assert(PH_T == 1024, "a tile is one workgroup of the largest size");
static_assert(2ll * EXPLAINN_PWM_HIST_SLICE <= (1ll << 31), "two counts per start stay inside a 32-bit bin");

__global__ __launch_bounds__(PH_T) void pwm_hist_kernel(
    const uint8_t* __restrict__ seq, long long start, int npos, int span, long long period, int both,
    const int16_t* __restrict__ S, const int* __restrict__ widths, unsigned long long* __restrict__ hist, int M,
    int wmax, int row_len, int G, int ntiles) {
    extern __shared__ int ph_sm[];             // bins [G][row_len] | tables [G][wmax][8] | codes [TILE + wmax - 1] bytes
    unsigned* h = reinterpret_cast<unsigned*>(ph_sm);
    int* tab = ph_sm + G * row_len;
    uint8_t* cs = reinterpret_cast<uint8_t*>(tab + G * wmax * 8);
    const int tid = threadIdx.x, m0 = blockIdx.x * G;
    for (int b = tid; b < G * row_len; b += PH_T) h[b] = 0u;
    stage_pair_tables(S, widths, m0, G, M, wmax, tid, PH_T, tab);
    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
        int t0, live_n;
        site_tile(tile, npos, t0, live_n);
        __syncthreads();                       // the bins and tables are written / the last tile's codes are read
        const int nstage = min(live_n + wmax - 1, span - t0);
        stage_codes<false>(seq + start + t0, nstage, tid, PH_T, cs, 0, nullptr);
        const int lim = pwm_start_limit(tid, live_n, nstage, start + t0, period);
        __syncthreads();
        const uint8_t* cp = cs + tid;          // cp[j] is read for j < w <= lim only
        // PH_Q motifs walk the window together: one code read serves all, and their table reads are independent
        // chains (one chain per lane left the walk waiting on LDS latency: DESIGN.md section 8).  A table is
        // zero past its motif's width, so every chain may run to the widest live motif of the set.
        for (int g = 0; g < G; g += PH_Q) {
            int w[PH_Q], fw[PH_Q], rw[PH_Q], wl = 0;
            const int* tb[PH_Q];
#pragma unroll
            for (int i = 0; i < PH_Q; ++i) {
                const int wi = g + i < G ? pwm_width(widths, m0 + g + i, M, wmax) : 0;
                w[i] = wi <= lim ? wi : 0;     // 0: an empty motif, past the group, or no live window here
                tb[i] = tab + min(g + i, G - 1) * wmax * 8;
                wl = max(wl, w[i]);
                fw[i] = rw[i] = 0;
            }
            for (int j = 0; j < wl; ++j) {
                const int code = cp[j];
#pragma unroll
                for (int i = 0; i < PH_Q; ++i) {
                    const int v = tb[i][j * 8 + code];
                    fw[i] += (int)(short)(v & 0xFFFF);
                    rw[i] += v >> 16;
                }
            }
            // an N makes both sums negative; a table entry outside [0, bins] may leave the row: neither counts
#pragma unroll
            for (int i = 0; i < PH_Q; ++i) {
                if (w[i] == 0) continue;
                unsigned* row = h + (g + i) * row_len;
                if ((unsigned)fw[i] < (unsigned)row_len) atomicAdd(&row[fw[i]], 1u);
                if (both && (unsigned)rw[i] < (unsigned)row_len) atomicAdd(&row[rw[i]], 1u);
            }
        }
    }
    __syncthreads();
    const int nb = min(G, M - m0) * row_len;
    unsigned long long* out = hist + (size_t)m0 * row_len;
    for (int b = tid; b < nb; b += PH_T) {
        const unsigned v = h[b];
        if (v) atomicAdd(&out[b], (unsigned long long)v);
    }
}

// motifs per workgroup: as many rows, with their tables, as the LDS holds beside a tile's codes, one at least
// (the largest row, 64 x 128 + 2 bins, is 32.8 KB: four fit), EXPLAINN_PWM_GROUP at the most
int pwm_hist_group(int wmax, int row_len) {
    const size_t per = ((size_t)row_len + (size_t)wmax * 8) * sizeof(int);
    const size_t room = PH_LDS - ((EXPLAINN_SITES_TILE + wmax - 1 + 15) & ~15);
    return (int)std::min<size_t>(EXPLAINN_PWM_GROUP, room / per);
}

// ---- the null ----------------------------------------------------------------------------------------
constexpr int PN_T = 256;

// One workgroup per motif.  The score of a random w-mer: pdf after column j lives on [0, (j+1) bins];
// pdf_new[s] = sum_a bg[a] pdf_old[s - S[j][a]], a = 0..3 in order, one lane per s.  Then the tail: every
// thread sums its run of scores from the top down, thread 0 chains the runs from the top down, and
// tail[s] = (sum inside the run from its top to s) + (the runs above): sums of non-negative terms, so the
// tail never rises with s and "the smallest s with tail[s] <= pcut" is the number of s with tail[s] > pcut.
__global__ __launch_bounds__(PN_T) void pwm_null_kernel(const int16_t* __restrict__ S, const int* __restrict__ widths,
                                                        int wmax, int bins, double bg0, double bg1, double bg2,
                                                        double bg3, double pcut, double* __restrict__ tail,
                                                        int* __restrict__ thr) {
    extern __shared__ double pn_lds[];         // two buffers [wmax bins + 1] | the threads' run sums [PN_T]
    __shared__ int above;
    const int m = blockIdx.x, tid = threadIdx.x;
    const int cap = wmax * bins + 1, stride = cap + 1;
    double* cur = pn_lds;
    double* nxt = pn_lds + cap;
    double* part = pn_lds + 2 * cap;
    double* trow = tail ? tail + (size_t)m * stride : nullptr;
    const int w = pwm_width(widths, m, m + 1, wmax);     // one workgroup per motif: m < M
    if (w == 0) {                              // an empty motif: no distribution, the out-of-range threshold
        if (trow) for (int s = tid; s < stride; s += PN_T) trow[s] = 0.0;
        if (tid == 0) thr[m] = 1;
        return;
    }
    const int n = w * bins + 1;                // scores 0 .. w bins
    for (int s = tid; s < n; s += PN_T) cur[s] = s == 0 ? 1.0 : 0.0;
    if (tid == 0) above = 0;
    __syncthreads();
    const double bg[4] = {bg0, bg1, bg2, bg3};
    for (int j = 0; j < w; ++j) {
        const int16_t* col = S + ((size_t)m * wmax + j) * 4;
        const int sa[4] = {col[0], col[1], col[2], col[3]};
        const int top_old = j * bins, top_new = top_old + bins;
        for (int s = tid; s <= top_new; s += PN_T) {
            double acc = 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int idx = s - sa[a];
                if (idx >= 0 && idx <= top_old) acc += bg[a] * cur[idx];
            }
            nxt[s] = acc;
        }
        __syncthreads();
        double* t = cur; cur = nxt; nxt = t;
    }
    const int per = (n + PN_T - 1) / PN_T;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    double run = 0.0;
    for (int s = hi - 1; s >= lo; --s) run += cur[s];
    part[tid] = run;
    __syncthreads();
    if (tid == 0) {
        double after = 0.0;                    // the runs above thread t's
        for (int t = PN_T - 1; t >= 0; --t) {
            const double v = part[t];
            part[t] = after;
            after += v;
        }
    }
    __syncthreads();
    const double after = part[tid];
    int mine = 0;
    run = 0.0;
    for (int s = hi - 1; s >= lo; --s) {
        run += cur[s];
        const double v = run + after;
        nxt[s] = v;
        mine += v > pcut ? 1 : 0;
    }
    if (mine) atomicAdd(&above, mine);         // an integer sum: the order does not matter
    __syncthreads();
    if (trow) for (int s = tid; s < stride; s += PN_T) trow[s] = s < n ? nxt[s] : 0.0;
    if (tid == 0) thr[m] = above;              // n = w bins + 1 when no tail is <= pcut
}

}  // namespace

extern "C" int explainn_pwm_null(const int16_t* scores, const int32_t* widths, int M, int wmax, int bins, double bg_a,
                                 double bg_c, double bg_g, double bg_t, double pcut, double* tail,
                                 int32_t* thresholds, void* stream) {
    if (!pwm_geometry_ok("pwm_null", M, wmax, bins)) return EXPLAINN_E_ARG;
    if (!(pcut >= 0.0 && pcut <= 1.0)) {
        explainn_set_error("pwm_null: pcut must be in [0, 1] (got %g)", pcut);
        return EXPLAINN_E_ARG;
    }
    const double bg[4] = {bg_a, bg_c, bg_g, bg_t};
    for (int a = 0; a < 4; ++a)
        if (!(bg[a] > 0.0 && bg[a] <= 1.0)) {
            explainn_set_error("pwm_null: every background frequency must be in (0, 1] (got %g)", bg[a]);
            return EXPLAINN_E_ARG;
        }
    if (M == 0) return EXPLAINN_OK;
    if (!scores || !widths || !thresholds) {
        explainn_set_error("pwm_null: scores, widths and thresholds must be device pointers");
        return EXPLAINN_E_ARG;
    }
    const size_t sm = ((size_t)2 * (wmax * bins + 1) + PN_T) * sizeof(double);      // <= 133136 bytes
    if (sm > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pwm_null_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    hipLaunchKernelGGL(pwm_null_kernel, dim3(M), dim3(PN_T), sm, static_cast<hipStream_t>(stream), scores, widths,
                       wmax, bins, bg_a, bg_c, bg_g, bg_t, pcut, tail, thresholds);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

// a row of sitescan.h's scheme is a (motif, strand): 2 m = '+', 2 m + 1 = '-'
extern "C" int64_t explainn_pwm_sites_workspace_bytes(int M, int64_t n_positions) {
    return (M < 0 || n_positions < 0) ? 0 : site_workspace_bytes(2 * (int64_t)M, n_positions);
}

extern "C" int explainn_pwm_sites(const uint8_t* seq, int64_t seq_len, int64_t start, int64_t n_positions,
                                  int64_t period, int both_strands, const int16_t* scores, const int32_t* widths,
                                  int M, int wmax, const int32_t* thresholds, const double* tail, int bins,
                                  int64_t* offsets, int32_t* pos, int32_t* score, double* pvalue, int64_t capacity,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
    if (!pwm_geometry_ok("pwm_sites", M, wmax, bins)) return EXPLAINN_E_ARG;
    if (start < 0 || n_positions < 0 || start + n_positions > seq_len || n_positions + wmax >= (int64_t)INT_MAX) {
        explainn_set_error("pwm_sites: need 0 <= start, start + n_positions <= seq_len and n_positions + wmax < 2^31 "
                           "(start=%lld n_positions=%lld seq_len=%lld)", (long long)start, (long long)n_positions,
                           (long long)seq_len);
        return EXPLAINN_E_ARG;
    }
    if (period < 0 || capacity < 0) {
        explainn_set_error("pwm_sites: period and capacity must not be negative");
        return EXPLAINN_E_ARG;
    }
    if (!offsets) { explainn_set_error("pwm_sites: offsets is required"); return EXPLAINN_E_ARG; }
    if (pvalue && !tail) { explainn_set_error("pwm_sites: pvalue needs tail"); return EXPLAINN_E_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool none = M == 0 || n_positions == 0;              // takes no pointer but offsets
    if (!none && (!seq || !scores || !widths || !thresholds)) {
        explainn_set_error("pwm_sites: seq, scores, widths and thresholds must be device pointers");
        return EXPLAINN_E_ARG;
    }
    if (!none && !workspace_ok("pwm_sites", workspace, workspace_bytes,
                               explainn_pwm_sites_workspace_bytes(M, n_positions), 256))
        return EXPLAINN_E_ARG;
    Carver cv(workspace);
    const SiteWorkspace w = none ? SiteWorkspace{} : site_workspace(cv, 2 * M, n_positions);
    long long* off = reinterpret_cast<long long*>(offsets);
    // the bases the call may read from `start` on: n_positions + wmax - 1, clipped to the sequence
    const int span = (int)std::min<int64_t>(n_positions + wmax - 1, seq_len - start);
    const size_t sm = (size_t)PS_G * wmax * 8 * sizeof(int) + ((EXPLAINN_SITES_TILE + wmax - 1 + 15) & ~15);
    const int both = both_strands ? 1 : 0, stride = wmax * bins + 2;
    return site_passes(2 * M, n_positions, w, off, pos != nullptr && capacity > 0, s, [&](auto mode) {
        hipLaunchKernelGGL(pwm_sites_kernel<decltype(mode)::value>, dim3(w.ntiles, (M + PS_G - 1) / PS_G), dim3(PS_T),
                           sm, s, seq, (long long)start, (int)n_positions, span, (long long)period, both, scores,
                           widths, thresholds, tail, stride, w.cnt, (const long long*)off, pos, score, pvalue,
                           (long long)capacity, M, wmax, w.ntiles);
    });
}

extern "C" int explainn_pwm_score_histogram(const uint8_t* seq, int64_t seq_len, int64_t start, int64_t n_positions,
                                            int64_t period, int both_strands, const int16_t* scores,
                                            const int32_t* widths, int M, int wmax, int bins, int64_t* hist,
                                            void* stream) {
    if (!pwm_geometry_ok("pwm_score_histogram", M, wmax, bins)) return EXPLAINN_E_ARG;
    if (start < 0 || n_positions < 0 || start + n_positions > seq_len || n_positions + wmax >= (int64_t)INT_MAX) {
        explainn_set_error("pwm_score_histogram: need 0 <= start, start + n_positions <= seq_len and n_positions + "
                           "wmax < 2^31 (start=%lld n_positions=%lld seq_len=%lld)", (long long)start,
                           (long long)n_positions, (long long)seq_len);
        return EXPLAINN_E_ARG;
    }
    if (period < 0) {
        explainn_set_error("pwm_score_histogram: period must not be negative");
        return EXPLAINN_E_ARG;
    }
    if (M == 0 || n_positions == 0) return EXPLAINN_OK;
    if (!seq || !scores || !widths || !hist) {
        explainn_set_error("pwm_score_histogram: seq, scores, widths and hist must be device pointers");
        return EXPLAINN_E_ARG;
    }
    const int row_len = wmax * bins + 2, G = pwm_hist_group(wmax, row_len);
    const int span = (int)std::min<int64_t>(n_positions + wmax - 1, seq_len - start);
    const size_t sm = (size_t)G * (row_len + wmax * 8) * sizeof(int) + ((EXPLAINN_SITES_TILE + wmax - 1 + 15) & ~15);
    if (sm > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pwm_hist_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    // about PH_BLOCKS blocks, and no slice of more than EXPLAINN_PWM_HIST_SLICE starts
    const int ntiles = (int)sites_tiles(n_positions), groups = (M + G - 1) / G;
    const int slices = std::min(ntiles, std::max({1, (PH_BLOCKS + groups - 1) / groups,
                                                  (ntiles + PH_SLICE_TILES - 1) / PH_SLICE_TILES}));
    hipLaunchKernelGGL(pwm_hist_kernel, dim3(groups, slices), dim3(PH_T), sm, static_cast<hipStream_t>(stream), seq,
                       (long long)start, (int)n_positions, span, (long long)period, both_strands ? 1 : 0, scores,
                       widths, reinterpret_cast<unsigned long long*>(hist), M, wmax, row_len, G, ntiles);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
