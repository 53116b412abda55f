// Variant effects on known motifs (DESIGN.md section 3 item 25, section 8 "Variant effects on known motifs"):
// per (motif, variant, allele) the largest integer PWM score over the windows the allele touches, on one or
// both strands, and where it sits -- explainn_pwm_record_best for the two haplotypes of a variant, neither of
// which is materialised.  The edit table is explainn_edits' (variants.hip), the tables and the pair words are
// pwmtab.h's, the key is bestsite.h's with the window's index i in place of the start.
//
// Geometry (a first choice): pwm_best_kernel's frame.  A 256-thread workgroup = (a slice of variants, a group of
// EXPLAINN_PWM_GROUP motifs); the group's pair-word tables sit in LDS once per workgroup and the four waves
// share nothing else.  A wave takes its variants round robin and stages both alleles' segments
// [pos - wmax + 1, pos + l + wmax - 1) of the two haplotypes -- at most 254 bytes each, spliced from seq and
// alt, N outside the haplotype and past the segment -- so a window that leaves the haplotype is dead by the
// same test as one that holds an N.  An SNV under a motif of 12 columns has 24 (allele, start) pairs: a lane
// per start would idle most of the wave.  A lane is instead (motif pair q of 8, allele of 2, start phase of
// 4): it walks the starts phase, phase + 4, ... of its pair -- two at a time, two independent (code read,
// table read) chains -- with one 64-bit table read per (column, code) as pb_walk does.  The two motifs of a
// pair share a window's START, not its index: start u counts from the first window of the wider motif, the
// narrower one joins at u = wa - wb with its own index u - (wa - wb).  Starts ascend within a lane, so it
// keeps the first strictly larger score; a 4-lane maximum of the key decides across the phases: the tie rule
// (lowest index, then '+') holds whatever the visiting order.  No atomics but the flags; no block-wide
// barrier after the tables are staged.
#include <algorithm>

#include "bestsite.h"
#include "common.h"
#include "pwmtab.h"

namespace {

constexpr int PV_T = 256;
constexpr int PV_WAVES = PV_T / 64;
constexpr int PV_G = EXPLAINN_PWM_GROUP;
constexpr int PV_CAP = EXPLAINN_PWM_VARIANT_MAX_ALLELE;
constexpr int PV_PHASES = 4;
// a segment's bytes: l + 2 wmax - 2 <= 254 staged from the haplotype, and N up to the last byte the second
// start of a lane's last step can read: (wmax - wa) + (wa + l - 2 + PV_PHASES) + wa - 1 <= 257
constexpr int PV_SEG = 272;
constexpr int PV_BLOCKS = 4096;                // the variants are cut into slices until a call has about this many blocks
static_assert(PV_G == 16, "a wave's lanes are 8 motif pairs x 2 alleles x 4 phases");
static_assert(PV_CAP + 2 * EXPLAINN_MOTIF_MAX_WIDTH + PV_PHASES - 3 < PV_SEG && PV_SEG % 16 == 0, "the segment's room");
static_assert(EXPLAINN_MOTIF_MAX_WIDTH * EXPLAINN_MOTIF_MAX_BINS < 65536, "two sums share a word without a carry");

// the wave's LDS writes are seen by its own later reads (and the other way round): one wave, no s_barrier
__device__ __forceinline__ void pv_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One allele's segment -> cs[0 .. PV_SEG): byte t is base pos - wmax + 1 + t of the haplotype
// seq[:pos] + allele + seq[pos + ref_len:], whose length is n_hap; N outside it and from `seg` on.  `own`: the
// allele's l bytes (alt + alt_off), NULL for the reference allele, which is seq's.  Every source index is
// checked against its array before the read.  Returns whether a byte above 4 was read.
__device__ __forceinline__ bool pv_stage(const uint8_t* __restrict__ seq, long long seq_len, const uint8_t* own,
                                         long long pos, int ref_len, int l, long long n_hap, int wmax, int seg,
                                         int lane, uint8_t* cs) {
    bool odd = false;
    for (int t = lane; t < PV_SEG; t += 64) {
        int v = 4;
        const long long h = pos - wmax + 1 + t;
        if (t < seg && h >= 0 && h < n_hap) {
            int b = 4;
            if (own && h >= pos && h < pos + l) {
                b = own[h - pos];                  // 0 <= h - pos < l = alt_len: inside the pool (checked by the caller)
            } else {
                const long long src = h < pos ? h : h - l + ref_len;
                if (src >= 0 && src < seq_len) b = seq[src];
            }
            odd |= b > 4;
            v = min(b, 4);
        }
        cs[t] = (uint8_t)v;
    }
    return odd;
}

__global__ __launch_bounds__(PV_T) void pwm_variant_kernel(
    const uint8_t* __restrict__ seq, long long seq_len, const long long* __restrict__ pos,
    const int* __restrict__ ref_len, const int* __restrict__ alt_len, const int* __restrict__ alt_off,
    const uint8_t* __restrict__ alt, long long alt_bytes, int n_variants, int both, const int16_t* __restrict__ S,
    const int* __restrict__ widths, uint16_t* __restrict__ best_bits, int32_t* __restrict__ best_site, int M, int wmax,
    int* __restrict__ flags) {
    // tables int2 [PV_G / 2][wmax][8] | codes [PV_WAVES][2 alleles][PV_SEG]; every offset a multiple of 16
    extern __shared__ __attribute__((aligned(16))) int2 pv_tab[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m0 = blockIdx.y * PV_G;
    uint8_t* cs = reinterpret_cast<uint8_t*>(pv_tab + (PV_G / 2) * wmax * 8) + wave * 2 * PV_SEG;
    pwm_stage_pair_tables<PV_G, PV_T>(reinterpret_cast<int*>(pv_tab), S, widths, m0, M, wmax, tid);
    __syncthreads();                           // the only block-wide barrier: the waves part here
    // what a lane is, for every variant: motifs ma, ma + 1 of pair q, allele A, phase
    const int q = lane >> 3, A = (lane >> 2) & 1, phase = lane & (PV_PHASES - 1), ma = m0 + 2 * q;
    const int w0 = pwm_width(widths, ma, M, wmax), w1 = pwm_width(widths, ma + 1, M, wmax);
    const int wb = min(w0, w1), wa = max(w0, w1), lead = wa - wb;
    const bool first = w0 > w1;                // motif ma is the wider one
    const int2* tb = pv_tab + q * wmax * 8;
    const uint8_t* cp = cs + A * PV_SEG + (wmax - wa);         // start u = 0 of the wider motif
    int raise = 0;
    for (long long v = (long long)blockIdx.x * PV_WAVES + wave; v < n_variants; v += (long long)gridDim.x * PV_WAVES) {
        const long long p = pos[v];
        const int rl = ref_len[v], al = alt_len[v], ao = alt_off[v];
        // compares only, before any read of seq or alt (the same in every lane)
        const bool ok = p >= 0 && rl >= 0 && al >= 0 && rl <= PV_CAP && al <= PV_CAP && p <= seq_len - rl && ao >= 0 &&
                        (long long)ao + al <= alt_bytes;
        int bs[2] = {-1, -1}, bw[2] = {0, 0};
        if (ok) {
            pv_wave_sync();                    // the last variant's reads are done
            const bool odd0 = pv_stage(seq, seq_len, nullptr, p, rl, rl, seq_len, wmax, rl + 2 * wmax - 2, lane, cs);
            const bool odd1 = pv_stage(seq, seq_len, alt + ao, p, rl, al, seq_len - rl + al, wmax, al + 2 * wmax - 2,
                                       lane, cs + PV_SEG);
            if (odd0 || odd1) raise |= 1;
            pv_wave_sync();
            const int l = A ? al : rl;
            const int count = wa > 0 ? wa + l - 1 : 0;         // the starts the wider motif has at this allele
            for (int u = phase; u < count; u += 2 * PV_PHASES) {
                // starts u and u + PV_PHASES together; the second may lie past count: it reads staged N and is dropped
                int a0[2] = {0, 0}, a1[2] = {0, 0}, nb[2] = {0, 0}, nw[2] = {0, 0};
                for (int j = 0; j < wa; ++j) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int code = cp[u + i * PV_PHASES + j];        // <= wmax + wa + l + 1 <= 257 < PV_SEG
                        const int2 t = tb[j * 8 + code];
                        nw[i] |= code;
                        if (j < wb) nb[i] |= code;
                        a0[i] += t.x;
                        a1[i] += t.y;
                    }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int uu = u + i * PV_PHASES;
                    // live: the start exists for this motif, the motif is not empty, the window holds no N
                    const bool wide = uu < count && !(nw[i] & 4), narrow = uu < count && uu >= lead && wb > 0 && !(nb[i] & 4);
                    const bool live[2] = {first ? wide : narrow, first ? narrow : wide};
                    const int index[2] = {first ? uu : uu - lead, first ? uu - lead : uu};
                    const int acc[2] = {a0[i], a1[i]};
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        const int f = acc[m] & 0xFFFF, r = both ? (int)((unsigned)acc[m] >> 16) : 0;
                        const int s = max(f, r);
                        if (live[m] && s > bs[m]) {
                            bs[m] = s;
                            bw[m] = (index[m] << 1) | (r > f ? 1 : 0);     // '+' on a tie
                        }
                    }
                }
            }
        } else {
            raise |= 2;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // a live start's key is never 0; the maximum over the four phases of (pair, allele)
            unsigned long long kk = bs[i] < 0 ? 0ull : best_key((unsigned)bs[i], bw[i] >> 1, (bw[i] & 1) ^ 1);
#pragma unroll
            for (int off = 1; off < PV_PHASES; off <<= 1) {
                const unsigned long long t = __shfl_xor(kk, off, 64);
                kk = t > kk ? t : kk;
            }
            const int m = ma + i;
            if (phase == 0 && m < M) {
                const size_t o = ((size_t)m * n_variants + v) * 2 + A;
                best_bits[o] = best_key_bits(kk);
                if (best_site) best_site[o] = best_key_site(kk);
            }
        }
    }
    if (blockIdx.y == 0 && flags) {
        const int all = (__ballot(raise & 1) ? 1 : 0) | (__ballot(raise & 2) ? 2 : 0);
        if (lane == 0 && all) atomicOr(flags, all);
    }
}

}  // namespace

extern "C" int explainn_pwm_variant_best(const uint8_t* seq, int64_t seq_len, const int64_t* pos, const int32_t* ref_len,
                                         const int32_t* alt_len, const int32_t* alt_off, const uint8_t* alt,
                                         int64_t alt_bytes, int64_t n_variants, int both_strands, const int16_t* scores,
                                         const int32_t* widths, int M, int wmax, uint16_t* best_bits, int32_t* best_site,
                                         int32_t* flags, void* stream) {
    if (seq_len < 0 || alt_bytes < 0 || n_variants < 0 || n_variants >= (int64_t)1 << 30) {
        explainn_set_error("pwm_variant_best: need seq_len >= 0, alt_bytes >= 0 and 0 <= n_variants < 2^30 "
                           "(seq_len=%lld alt_bytes=%lld n_variants=%lld)",
                           (long long)seq_len, (long long)alt_bytes, (long long)n_variants);
        return EXPLAINN_E_ARG;
    }
    if (!pwm_geometry_ok("pwm_variant_best", M, wmax, 1)) return EXPLAINN_E_ARG;
    if (M == 0 || n_variants == 0) return EXPLAINN_OK;
    if (!pos || !ref_len || !alt_len || !alt_off || !scores || !widths || !best_bits || (seq_len > 0 && !seq) ||
        (alt_bytes > 0 && !alt)) {
        explainn_set_error("pwm_variant_best: seq, pos, ref_len, alt_len, alt_off, alt, scores, widths and best_bits "
                           "must be device pointers");
        return EXPLAINN_E_ARG;
    }
    const int groups = (M + PV_G - 1) / PV_G;
    const long long per_block = (n_variants + PV_WAVES - 1) / PV_WAVES;
    const long long slices = std::min<long long>(per_block, std::max<long long>(1, PV_BLOCKS / groups));
    const size_t sm = (size_t)PV_G * wmax * 8 * sizeof(int) + (size_t)PV_WAVES * 2 * PV_SEG;
    hipLaunchKernelGGL(pwm_variant_kernel, dim3((unsigned)slices, groups), dim3(PV_T), sm,
                       static_cast<hipStream_t>(stream), seq, (long long)seq_len,
                       reinterpret_cast<const long long*>(pos), ref_len, alt_len, alt_off, alt, (long long)alt_bytes,
                       (int)n_variants, both_strands ? 1 : 0, scores, widths, best_bits, best_site, M, wmax, flags);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
