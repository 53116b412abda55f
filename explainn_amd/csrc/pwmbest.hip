// Known-motif enrichment and centrality (DESIGN.md section 3 item 21, section 8 "Known-motif enrichment"):
// per (motif, record) the largest integer PWM score over the record's live starts and both strands, and
// where it sits -- explainn_record_best for score tables in place of a model's filters.  The matrix it
// writes is what explainn_enrichment_test and explainn_site_positions read: a quantised score is an
// integer <= 8192, a 15-bit pattern that sorts like the score.
//
// Geometry (a first choice): a 256-thread workgroup = (a slice of records, a group of EXPLAINN_PWM_GROUP
// motifs).  The group's tables sit in LDS once per workgroup, sized by the call's wmax, as
// pwmtab.h's pair words, so one walk over a window's codes in forward order scores both strands.  Two things
// differ from pwm_sites_kernel:
//   * the words of the two motifs a lane walks together lie side by side, [pair][column][code][2], so one
//     64-bit LDS read serves both chains (a column past a motif's width holds 0: the wider motif of a
//     pair goes on alone by adding zeros to the other);
//   * the halves are accumulated in place (two sums <= 8192 never carry), so N cannot be a negative
//     sentinel: N holds 0 and the window's codes are ORed -- bit 2 of the OR marks a window with an N.
// The four waves share the tables and nothing else: the records of a slice are dealt round robin to the
// waves, and a wave walks its record in passes of EXPLAINN_PWM_BEST_SPAN starts over its own staged codes
// [SPAN + wmax - 1]; what lies past the record's end is staged as N, so a window that leaves the record
// is dead by the same test and every trip count is wave-uniform.  A lane takes SPAN / 64 starts, lane +
// 64 i, and walks them TOGETHER with the two motifs: up to four independent (code read, table read)
// chains in flight -- the walk is LDS-latency bound otherwise.  A lane's starts ascend, so it keeps
// (score, site) of the first strictly larger score -- per start the larger strand, '+' on a tie -- and
// only its final best becomes bestsite.h's key for the one wave maximum per (record, motif).  With one
// pass (records up to SPAN bases) the codes are staged once per record; a longer record restages its
// passes per motif pair (320 bytes a pass, from L2).  The records are cut into slices until the call has about PB_BLOCKS workgroups: several rounds of
// the device, so that a last, part-filled round costs little.  No atomics but the input flag; no
// block-wide barrier after the tables are staged.
#include <limits.h>

#include <algorithm>

#include "bestsite.h"
#include "common.h"
#include "pwmtab.h"

namespace {

constexpr int PB_T = 256;
constexpr int PB_WAVES = PB_T / 64;
constexpr int PB_SPAN = EXPLAINN_PWM_BEST_SPAN;
constexpr int PB_ILP = PB_SPAN / 64;           // starts a lane takes per pass
constexpr int PB_G = EXPLAINN_PWM_GROUP;
constexpr int PB_BLOCKS = 16384;               // the records are cut into slices until a call has about this many blocks
static_assert(PB_SPAN % 64 == 0 && PB_ILP == 4, "pb_walk is instantiated for one to four starts per lane");
static_assert(PB_G % 2 == 0, "the motifs of a group are walked in pairs");
static_assert(EXPLAINN_MOTIF_MAX_WIDTH * EXPLAINN_MOTIF_MAX_BINS < 65536, "two sums share a word without a carry");

// the wave's LDS writes are seen by its own later reads (and the other way round): one wave, no s_barrier
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// src[0 .. n) -> cs[0 .. total), N past n; a byte above 4 reads as N.  n <= total.
__device__ __forceinline__ void pb_stage(const uint8_t* __restrict__ src, int n, int total, int lane, uint8_t* cs) {
    for (int i = lane; i < total; i += 64) {
        int v = 4;
        if (i < n) v = min((int)src[i], 4);
        cs[i] = (uint8_t)v;
    }
}

// N starts of one lane, cp + 64 i, against a motif pair's table tb [column][8]: .x the first motif's word,
// .y the second's.  wb <= wa: the widths of the narrower and the wider motif; `first`: the first is the
// wider.  p0: the start of cp relative to the record.  (bs, bw)[2]: the lane's best (score, site) per
// motif so far, bs < 0 = none; a later start replaces it only with a strictly larger score.
template <int N>
__device__ __forceinline__ void pb_walk(const int2* tb, const uint8_t* cp, int wb, int wa, bool first, bool has0,
                                        bool has1, int both, int p0, int (&bs)[2], int (&bw)[2]) {
    int a0[N], a1[N], nb[N], nw[N];
#pragma unroll
    for (int i = 0; i < N; ++i) a0[i] = a1[i] = nb[i] = 0;
    int j = 0;
    for (; j < wb; ++j) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int code = cp[i * 64 + j];       // j < wa <= wmax: inside the staged codes
            const int2 v = tb[j * 8 + code];
            nb[i] |= code;
            a0[i] += v.x;
            a1[i] += v.y;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) nw[i] = nb[i];
    for (; j < wa; ++j) {                          // the wider one goes on alone: the other's columns hold 0
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int code = cp[i * 64 + j];
            const int2 v = tb[j * 8 + code];
            nw[i] |= code;
            a0[i] += v.x;
            a1[i] += v.y;
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int site = (p0 + i * 64) << 1;
        // live: the motif is not empty and its window holds no N (past the record's end all is N)
        const bool live[2] = {has0 && !((first ? nw[i] : nb[i]) & 4), has1 && !((first ? nb[i] : nw[i]) & 4)};
        const int acc[2] = {a0[i], a1[i]};
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int f = acc[m] & 0xFFFF, r = both ? (int)((unsigned)acc[m] >> 16) : 0;
            const int s = max(f, r);
            if (live[m] && s > bs[m]) {
                bs[m] = s;
                bw[m] = site | (r > f ? 1 : 0);    // '+' on a tie
            }
        }
    }
}

__global__ __launch_bounds__(PB_T) void pwm_best_kernel(
    const uint8_t* __restrict__ seq, long long seq_len, const long long* __restrict__ off, int n_records, int both,
    const int16_t* __restrict__ S, const int* __restrict__ widths, uint16_t* __restrict__ best_bits,
    int32_t* __restrict__ best_site, int M, int wmax, int* __restrict__ flags) {
    // tables int2 [PB_G / 2][wmax][8] | codes [PB_WAVES][span_bytes]; every offset a multiple of 16
    extern __shared__ __attribute__((aligned(16))) int2 pb_tab[];
    const int span_bytes = (PB_SPAN + wmax - 1 + 15) & ~15;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m0 = blockIdx.y * PB_G;
    uint8_t* cs = reinterpret_cast<uint8_t*>(pb_tab + (PB_G / 2) * wmax * 8) + wave * span_bytes;
    pwm_stage_pair_tables<PB_G, PB_T>(reinterpret_cast<int*>(pb_tab), S, widths, m0, M, wmax, tid);
    __syncthreads();                           // the only block-wide barrier: the waves part here
    const int total = PB_SPAN + wmax - 1;
    int bad = 0;
    for (long long r = (long long)blockIdx.x * PB_WAVES + wave; r < n_records; r += (long long)gridDim.x * PB_WAVES) {
        const long long a = off[r], b = off[r + 1];
        const bool ok = BEST_RECORD_OK(a, b, seq_len);            // before any read of seq
        if (!ok) bad = 1;
        const int len = ok ? (int)(b - a) : 0;
        const uint8_t* rec = seq + (ok ? a : 0);
        const bool one_pass = len <= PB_SPAN;
        if (one_pass && len > 0) {
            wave_sync();                       // the last record's reads are done
            pb_stage(rec, len, total, lane, cs);
            wave_sync();
        }
        for (int q = 0; q < PB_G / 2; ++q) {
            const int ma = m0 + 2 * q;         // motifs ma, ma + 1
            if (ma >= M) break;                // (the same in every thread)
            const int w0 = pwm_width(widths, ma, M, wmax), w1 = pwm_width(widths, ma + 1, M, wmax);
            const int2* tb = pb_tab + q * wmax * 8;
            const int wb = min(w0, w1), wa = max(w0, w1);
            const bool first = w0 > w1;
            // the starts the narrower live motif of the pair has in this record (<= 0: none)
            const int n_starts = wa > 0 ? len - (wb > 0 ? wb : wa) + 1 : 0;
            int bs[2] = {-1, -1}, bw[2] = {0, 0};
            for (int t0 = 0; t0 < n_starts; t0 += PB_SPAN) {
                if (!one_pass) {
                    wave_sync();
                    pb_stage(rec + t0, min(total, len - t0), total, lane, cs);
                    wave_sync();
                }
                const int chunks = (min(PB_SPAN, n_starts - t0) + 63) >> 6;       // (wave-uniform)
                const uint8_t* cp = cs + lane;
                switch (chunks) {
                    case 1: pb_walk<1>(tb, cp, wb, wa, first, w0 > 0, w1 > 0, both, t0 + lane, bs, bw); break;
                    case 2: pb_walk<2>(tb, cp, wb, wa, first, w0 > 0, w1 > 0, both, t0 + lane, bs, bw); break;
                    case 3: pb_walk<3>(tb, cp, wb, wa, first, w0 > 0, w1 > 0, both, t0 + lane, bs, bw); break;
                    default: pb_walk<4>(tb, cp, wb, wa, first, w0 > 0, w1 > 0, both, t0 + lane, bs, bw); break;
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                // a live start's key is never 0
                const unsigned long long mine = bs[i] < 0 ? 0ull : best_key((unsigned)bs[i], bw[i] >> 1, (bw[i] & 1) ^ 1);
                const unsigned long long kk = wave_max(mine);
                const int m = ma + i;
                if (lane == 0 && m < M) {
                    const size_t o = (size_t)m * n_records + r;
                    best_bits[o] = best_key_bits(kk);
                    if (best_site) best_site[o] = best_key_site(kk);
                }
            }
        }
    }
    if (blockIdx.y == 0 && lane == 0 && bad && flags) atomicOr(flags, 1);
}

}  // namespace

extern "C" int explainn_pwm_record_best(const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets,
                                        int64_t n_records, int both_strands, const int16_t* scores,
                                        const int32_t* widths, int M, int wmax, uint16_t* best_bits,
                                        int32_t* best_site, int32_t* flags, void* stream) {
    if (seq_len < 0 || n_records < 0 || n_records >= (int64_t)1 << 31) {
        explainn_set_error("pwm_record_best: need seq_len >= 0 and 0 <= n_records < 2^31 (seq_len=%lld n_records=%lld)",
                           (long long)seq_len, (long long)n_records);
        return EXPLAINN_E_ARG;
    }
    if (!pwm_geometry_ok("pwm_record_best", M, wmax, 1)) return EXPLAINN_E_ARG;
    if (M == 0 || n_records == 0) return EXPLAINN_OK;
    if (!rec_offsets || !scores || !widths || !best_bits || (seq_len > 0 && !seq)) {
        explainn_set_error("pwm_record_best: seq, rec_offsets, scores, widths and best_bits must be device pointers");
        return EXPLAINN_E_ARG;
    }
    const int groups = (M + PB_G - 1) / PB_G;
    const long long per_block = (n_records + PB_WAVES - 1) / PB_WAVES;
    const long long slices = std::min<long long>(per_block, std::max<long long>(1, PB_BLOCKS / groups));
    const size_t sm = (size_t)PB_G * wmax * 8 * sizeof(int) + (size_t)PB_WAVES * ((PB_SPAN + wmax - 1 + 15) & ~15);
    hipLaunchKernelGGL(pwm_best_kernel, dim3((unsigned)slices, groups), dim3(PB_T), sm, static_cast<hipStream_t>(stream),
                       seq, (long long)seq_len, reinterpret_cast<const long long*>(rec_offsets), (int)n_records,
                       both_strands ? 1 : 0, scores, widths, best_bits, best_site, M, wmax, flags);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
