// Dinucleotide-preserving shuffles on the device ("Shuffles"): the r-th shuffle of
// every row of base codes, the Altschul-Erickson Euler path in a form that needs no edge lists.
// Stand-alone: needs no explainn_ctx, only device pointers; no workspace, no allocation, no host sync.
//
// One lane per (row, r), 64-lane workgroups, no barrier: a lane shares nothing with its neighbours.
// State of a lane: the 5 x 5 pair counts c[a][b] in LDS, lane-minor (counter (a,b) of lane t is word
// (5a+b)*64 + t, so a wave's access is conflict-free whatever (a,b) each lane asks for); the last exits
// e(v) and the row's own last exits as 3 bits per symbol of one register each; the symbols that need a
// last exit as a bit mask; 16 emitted symbols in four registers used as a byte shift register.  The R
// lanes of a row read the same code bytes (broadcast loads, 16 B at a time where the address allows).
// No floating point, no atomics, no dynamically indexed private array (every run-time index is an LDS
// address or a shift count).
//
// The order of draws is part of the result and is restated in tests/shuffle_model.py:
//   draw t (t = 0, 1, ... per (row, r)) = mix(key + GOLD*(t+1)) >> 32, reduced to [0, m) by the high
//   half of the 32 x 32-bit product;  key = mix(mix(mix(seed + GOLD) ^ row) ^ r), row = row0 + i;
//   mix = the splitmix64 finaliser.
//   1. first picks: v = 0..4 ascending, every v that needs a last exit draws one from c[v][b], b != v;
//   2. while the picks hold a cycle: the cycle is the one reached from the lowest v whose picks do not
//      lead to the final symbol; its vertices redraw in ascending order; at most max_rounds cycles are
//      popped, then the row's own last exits are taken and `capped` is set;
//   3. the walk: one draw per position at which the current symbol has unreserved edges left.
#include "common.h"

namespace {

constexpr int SH_T = 64;
constexpr uint64_t SH_GOLD = 0x9e3779b97f4a7c15ULL;

__device__ __forceinline__ uint64_t sh_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ULL;
    z ^= z >> 27; z *= 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
// the next draw of the lane's stream, reduced to [0, m)
__device__ __forceinline__ uint32_t sh_draw(uint64_t key, uint32_t& t, uint32_t m) {
    t += 1;
    return __umulhi((uint32_t)(sh_mix(key + SH_GOLD * (uint64_t)t) >> 32), m);
}
// the number of prefix sums of (c0..c4) that are <= j: the first symbol whose cumulative count exceeds j
__device__ __forceinline__ uint32_t sh_pick(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t j) {
    uint32_t acc = c0, b = j >= acc;
    acc += c1; b += j >= acc;
    acc += c2; b += j >= acc;
    acc += c3; b += j >= acc;
    return b;
}
__device__ __forceinline__ uint32_t sh_sym(uint32_t byte) { return byte < 4u ? byte : 4u; }

// a last exit of symbol V (a compile-time constant in the unrolled callers) drawn from c[V][b], b != V
template <int V>
__device__ __forceinline__ uint32_t sh_draw_exit(const uint32_t* cl, uint64_t key, uint32_t& t) {
    uint32_t c[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) c[b] = b == V ? 0u : cl[(V * 5 + b) * SH_T];
    const uint32_t d = c[0] + c[1] + c[2] + c[3] + c[4];
    return sh_pick(c[0], c[1], c[2], c[3], sh_draw(key, t, d));
}
#define SH_FOR_V(X) X(0) X(1) X(2) X(3) X(4)

__global__ __launch_bounds__(SH_T) void dinuc_shuffle_kernel(const uint8_t* __restrict__ codes, int64_t total,
                                                             int L, int R, uint64_t seed, int64_t row0,
                                                             int max_rounds, uint8_t* __restrict__ out,
                                                             uint8_t* __restrict__ capped) {
    __shared__ uint32_t cnt[25 * SH_T];
    const int tid = threadIdx.x;
    const int64_t gid = (int64_t)blockIdx.x * SH_T + tid;
    if (gid >= total) return;
    const int64_t i = gid / R;
    const uint32_t r = (uint32_t)(gid - i * R);
    const uint8_t* row = codes + i * L;
    uint8_t* dst = out + gid * L;
    if (L < 3) {
        for (int p = 0; p < L; ++p) dst[p] = (uint8_t)sh_sym(row[p]);
        if (capped) capped[gid] = 0;
        return;
    }
    uint32_t* cl = cnt + tid;                    // counter (a,b) of this lane: cl[(5a+b)*SH_T]
#pragma unroll
    for (int q = 0; q < 25; ++q) cl[q * SH_T] = 0u;

    // ---- counts, the row's own last exits, the symbols that have a successor ----
    const uint32_t first = sh_sym(row[0]);
    uint32_t prev = first, own = 0u, occ = 0u;
    auto feed = [&](uint32_t byte) {
        const uint32_t s = sh_sym(byte);
        cl[(prev * 5 + s) * SH_T] += 1u;
        own = (own & ~(7u << (3 * prev))) | (s << (3 * prev));
        occ |= 1u << prev;
        prev = s;
    };
    int p = 1;
    for (; p < L && ((uintptr_t)(row + p) & 15u); ++p) feed(row[p]);
    for (; p + 16 <= L; p += 16) {
        const uint4 w = *reinterpret_cast<const uint4*>(row + p);
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 16; ++q) feed((ww[q >> 2] >> (8 * (q & 3))) & 255u);
    }
    for (; p < L; ++p) feed(row[p]);
    const uint32_t last = prev;
    const uint32_t need = occ & ~(1u << last);   // every such symbol has a successor other than itself

    // ---- last exits by cycle popping ----
    const uint64_t key = sh_mix(sh_mix(sh_mix(seed + SH_GOLD) ^ (uint64_t)(row0 + i)) ^ (uint64_t)r);
    uint32_t t = 0u, e = 0u, cap = 0u;
#define SH_FIRST(V) if ((need >> V) & 1u) e |= sh_draw_exit<V>(cl, key, t) << (3 * V);
    SH_FOR_V(SH_FIRST)
#undef SH_FIRST
    for (int rounds = 0;; ++rounds) {
        uint32_t u = 8u;                         // a vertex on the first cycle found, 8 = none
#pragma unroll
        for (uint32_t v = 0; v < 5; ++v) {
            uint32_t cur = v;
#pragma unroll
            for (int s = 0; s < 5; ++s) cur = cur != last ? (e >> (3 * cur)) & 7u : cur;
            if (u == 8u && ((need >> v) & 1u) && cur != last) u = cur;
        }
        if (u == 8u) break;
        if (rounds >= max_rounds) { e = own; cap = 1u; break; }
        uint32_t cyc = 0u;
#pragma unroll
        for (int s = 0; s < 4; ++s) { cyc |= 1u << u; u = (e >> (3 * u)) & 7u; }
#define SH_REDRAW(V) if ((cyc >> V) & 1u) e = (e & ~(7u << (3 * V))) | (sh_draw_exit<V>(cl, key, t) << (3 * V));
        SH_FOR_V(SH_REDRAW)
#undef SH_REDRAW
    }
    // reserve one unit of c[v][e(v)]
#pragma unroll
    for (uint32_t v = 0; v < 5; ++v)
        if ((need >> v) & 1u) cl[(v * 5 + ((e >> (3 * v)) & 7u)) * SH_T] -= 1u;

    // ---- the walk; 16 symbols per 16-byte store from the first aligned address on ----
    int head = (int)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    head = head < L ? head : L;
    uint32_t w0 = 0u, w1 = 0u, w2 = 0u, w3 = 0u;
    int held = 0;
    uint32_t cur = first;
    for (int q = 0; q < L; ++q) {
        if (q > 0) {
            uint32_t* cv = cl + cur * 5 * SH_T;
            const uint32_t c0 = cv[0], c1 = cv[SH_T], c2 = cv[2 * SH_T], c3 = cv[3 * SH_T], c4 = cv[4 * SH_T];
            const uint32_t m = c0 + c1 + c2 + c3 + c4;
            uint32_t b;
            if (m > 0u) {
                b = sh_pick(c0, c1, c2, c3, sh_draw(key, t, m));
                const uint32_t cb = b == 0u ? c0 : b == 1u ? c1 : b == 2u ? c2 : b == 3u ? c3 : c4;
                cv[b * SH_T] = cb - 1u;
            } else {
                b = (e >> (3 * cur)) & 7u;       // the reserved last exit
            }
            cur = b;
        }
        if (q < head) {
            dst[q] = (uint8_t)cur;
        } else {
            w0 = (w0 >> 8) | (w1 << 24);
            w1 = (w1 >> 8) | (w2 << 24);
            w2 = (w2 >> 8) | (w3 << 24);
            w3 = (w3 >> 8) | (cur << 24);
            if (++held == 16) {
                *reinterpret_cast<uint4*>(dst + q - 15) = make_uint4(w0, w1, w2, w3);
                held = 0;
            }
        }
    }
    // the tail: the `held` youngest bytes of the shift register, oldest first
    for (int s = held; s < 16; ++s) {
        w0 = (w0 >> 8) | (w1 << 24);
        w1 = (w1 >> 8) | (w2 << 24);
        w2 = (w2 >> 8) | (w3 << 24);
        w3 >>= 8;
    }
    for (int s = 0; s < held; ++s) {
        dst[L - held + s] = (uint8_t)(w0 & 255u);
        w0 = (w0 >> 8) | (w1 << 24);
        w1 = (w1 >> 8) | (w2 << 24);
        w2 = (w2 >> 8) | (w3 << 24);
        w3 >>= 8;
    }
    if (capped) capped[gid] = (uint8_t)cap;
}

}  // namespace

extern "C" int explainn_dinucleotide_shuffle(const uint8_t* codes, int64_t N, int L, int R, uint64_t seed,
                                             int64_t row0, int max_rounds, uint8_t* out, uint8_t* capped,
                                             void* stream) {
    if (N < 0 || L < 1 || R < 1) {
        explainn_set_error("dinucleotide_shuffle: need N >= 0, L >= 1, R >= 1 (N=%lld L=%d R=%d)", (long long)N,
                           L, R);
        return EXPLAINN_E_ARG;
    }
    if (N == 0) return EXPLAINN_OK;
    if (!codes || !out) {
        explainn_set_error("dinucleotide_shuffle: codes and out must be device pointers");
        return EXPLAINN_E_ARG;
    }
    const int64_t blocks_max = 0x7fffffffLL;
    if (N > blocks_max * SH_T / R) {
        explainn_set_error("dinucleotide_shuffle: N*R = %lld*%d exceeds one launch; split the rows (row0)",
                           (long long)N, R);
        return EXPLAINN_E_UNSUPPORTED;
    }
    const int64_t total = N * R;
    if (max_rounds <= 0) {
        const int64_t d = 64LL * L;
        max_rounds = d > 0x7fffffffLL ? 0x7fffffff : (int)d;
    }
    hipLaunchKernelGGL(dinuc_shuffle_kernel, dim3((unsigned)((total + SH_T - 1) / SH_T)), dim3(SH_T), 0,
                       static_cast<hipStream_t>(stream), codes, total, L, R, seed, row0, max_rounds, out, capped);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
