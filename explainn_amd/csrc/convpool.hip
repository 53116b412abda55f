// The filter bank: Conv1d(4U->U, k, groups=U) + BatchNorm1 + exp + MaxPool1d(7,7)
// (architectures/__init__.py:73-81) as ONE kernel that never materialises the conv output.
//
// One-hot input makes the convolution a sum of one table entry per tap: conv[b,u,p] = sum_j W[u, s[b,p+j], j].
// Rounds 1-2 did that as a gather (dinucleotide tables in LDS, 40 B of LDS traffic per unit and
// position, 0.61 of the LDS array); round 3 puts it on the matrix core as a GEMM against the one-hot
// bits.  BatchNorm+exp are monotone per unit, so the 7-wide max-pool runs on the raw sums with the
// sign of alpha = gamma1/sigma1 choosing max or min; only the pooled extreme (and its offset, for
// the backward routing) leaves the kernel: ext[u][w][b], idx[u][w][b].
#include <cstdlib>
#include <type_traits>

#include "common.h"

// ---------------------------------------------------------------------------------------------
// The filter bank on the matrix core.  conv[u][(b,p)] = sum_k Wf[u][k] X[k][(b,p)] with
// k = 4 tap + base and X the one-hot bit "sequence b has base a at position p + tap": a GEMM whose A
// operand is the filters as three bf16 pieces (sum = the fp32 weight exactly, every product with a
// 0/1 bit exact, fp32 accumulation) and whose B operand is generated from the 2-bit codes -- a lane
// needs the one-hot images of TWO consecutive bases (8 bf16 = one 16-byte entry of a 16-entry LDS
// table indexed by the 4 code bits; the 64-entry table also zeroes the taps that see an N).
// v_mfma_f32_32x32x16_bf16: tile = 32 units x 32 sequences at ONE position, 4 taps per k-step.
// A wave (= a workgroup; one per SIMD, 512 registers) owns 32 sequences, UT unit tiles whose
// fragments stay in registers, and a range of pooling windows; it walks the positions in order and
// keeps the running maximum and the first position that reached it (strict >), so the conv output
// never exists.  Units with gamma1 < 0 pool the minimum: their filters are negated in Wf and the
// sign comes back at the store.
// The instruction stream is laid out by hand (sched_barrier after every MFMA): an MFMA holds the
// SIMD's vector issue for 8 of its 32 cycles, so behind each one go its share of the vector work of
// the NEIGHBOURING positions -- the max/argmax update of the previous position (three accumulator
// sets rotate X A B A B A B so that the window length 7 needs no parity), the table addresses and
// LDS reads of the next position's operands (three operand buffers, same rotation), and the stores
// of the previous window.
// Roof: 3 pieces x KS k-steps x 32 clk per (32 units, 32 sequences, position) on the matrix pipe.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) __bf16 cbf16x8;
typedef float cf32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t cu32x4 __attribute__((ext_vector_type(4)));

template <int KS, int UT> struct cpm_state {
    cu32x4 Wr[UT][KS][3];        // A fragments (pieces hi, mid, lo)
    cf32x16 acc[3][UT];          // accumulator sets X, A, B
    float best[UT][16];
    uint32_t arg[UT][16];
    cu32x4 bop[3][KS];           // B operands of three positions
    uint32_t xs[3], nx[2];       // the window's codes / N bits, shifted to the lane's k-half
    uint32_t gw[4], mw[3];       // words of the NEXT window (global loads in flight)
    uint32_t smask[UT][16];      // 0x80000000 where that unit pools the minimum
    uint32_t so, so4;            // running offsets (idx bytes, ext bytes) of the stores of the previous window
    uint32_t r1, r5;             // its row strides in elements (0 while there is no previous window)
};
struct cpm_args {
    const uint32_t* pk2; const uint32_t* nmask; float* ext; uint8_t* idx;
    int n, Bs, PW, NW, t0, b, kh; uint32_t tbase;
    uint32_t row1, row5;         // n Bs and 5 n Bs: element strides between the rows a lane stores
    __amdgpu_buffer_rsrc_t rext, ridx;   // raw buffer descriptors of ext (bytes) and idx
};
__device__ __forceinline__ constexpr int cpm_role(int i) { return i == 0 ? 0 : ((i & 1) ? 1 : 2); }

template <int KS, int UT>
__device__ __forceinline__ void cpm_fetch(cpm_state<KS, UT>& S, const cpm_args& A, int w) {
    const int p0 = POOLW * w, wi = p0 >> 4, ni = p0 >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) S.gw[i] = A.pk2[(size_t)min(wi + i, A.PW - 1) * A.Bs + A.b];
#pragma unroll
    for (int i = 0; i < 3; ++i) S.mw[i] = A.nmask[(size_t)min(ni + i, A.NW - 1) * A.Bs + A.b];
}
// window w's words -> xs / nx (the fetched words are consumed; the fetch of window w + 1 follows)
template <int KS, int UT>
__device__ __forceinline__ void cpm_window_words(cpm_state<KS, UT>& S, const cpm_args& A, int w) {
    const int p0 = POOLW * w;
    const int sh = (p0 & 15) * 2, nsh = p0 & 31;
    const uint32_t w0 = __funnelshift_r(S.gw[0], S.gw[1], sh), w1 = __funnelshift_r(S.gw[1], S.gw[2], sh),
                   w2 = __funnelshift_r(S.gw[2], S.gw[3], sh);
    // the lane's k-half starts two taps further on
    S.xs[0] = __funnelshift_r(w0, w1, 4 * A.kh); S.xs[1] = __funnelshift_r(w1, w2, 4 * A.kh);
    S.xs[2] = w2 >> (4 * A.kh);
    const uint32_t nm0 = __funnelshift_r(S.mw[0], S.mw[1], nsh), nm1 = __funnelshift_r(S.mw[1], S.mw[2], nsh);
    S.nx[0] = __funnelshift_r(nm0, nm1, 2 * A.kh); S.nx[1] = nm1 >> (2 * A.kh);
    cpm_fetch(S, A, w + 1);
}
// B operand of (position i of the window in xs, k-step ks) into buffer `buf`
template <int KS, int UT, int I, int KSI, int BUF>
__device__ __forceinline__ void cpm_operand(cpm_state<KS, UT>& S, const cpm_args& A) {
    typedef __attribute__((address_space(3))) cu32x4 lds_u4;
    typedef __attribute__((address_space(3))) char lds_char;
    constexpr int off = 2 * I + 8 * KSI, wd = off >> 5, o = off & 31;
    constexpr int noff = I + 4 * KSI, nwd = noff >> 5, no = noff & 31;
    uint32_t cs, ns;
    if constexpr (o + 4 <= 32) {
        if constexpr (o >= 4) cs = S.xs[wd] >> (o - 4); else cs = S.xs[wd] << (4 - o);
    } else {
        cs = __funnelshift_r(S.xs[wd], S.xs[wd + 1], o) << 4;
    }
    if constexpr (no + 2 <= 32) {
        if constexpr (no >= 8) ns = S.nx[nwd] >> (no - 8); else ns = S.nx[nwd] << (8 - no);
    } else {
        ns = __funnelshift_r(S.nx[nwd], S.nx[nwd + 1], no) << 8;
    }
    const uint32_t a = ((cs & 0xF0u) | A.tbase) | (ns & 0x300u);
    S.bop[BUF][KSI] = *reinterpret_cast<const lds_u4*>((const lds_char*)(size_t)a);
}
// max / argmax update of element (t, r) with the sums of position PI held in set ROLE, in two halves:
// the compare (lane mask into an SGPR pair) and, two elements later, the two selects that read it --
// a select within two instructions of the compare that writes its mask costs wait states, and a
// mask the compiler carries itself across the MFMA blocks gets materialised in a VGPR.  Inline
// assembly, so the distance is this file's business (cpm_position keeps three masks in rotation).
template <int KS, int UT, bool IDX, int PI, int ROLE>
__device__ __forceinline__ void cpm_update_cmp(cpm_state<KS, UT>& S, int t, int r, unsigned long long& gt) {
    const float v = S.acc[ROLE][t][r];
    if (PI == 0) {
        S.best[t][r] = v;                  // (the offset starts with position 1's select: 0 or 1)
    } else if (IDX) {
        asm volatile("v_cmp_gt_f32_e64 %0, %1, %2" : "=s"(gt) : "v"(v), "v"(S.best[t][r]));
    } else {
        // (fmaxf would canonicalise both operands first: three v_max per element)
        float bv = S.best[t][r];
        asm volatile("v_max_f32 %0, %0, %1" : "+v"(bv) : "v"(v));
        S.best[t][r] = bv;
    }
}
template <int KS, int UT, bool IDX, int PI, int ROLE>
__device__ __forceinline__ void cpm_update_sel(cpm_state<KS, UT>& S, int t, int r, unsigned long long gt) {
    if (PI != 0 && IDX) {
        const float v = S.acc[ROLE][t][r];
        float bv = S.best[t][r];
        uint32_t av = PI == 1 ? 0u : S.arg[t][r];
        asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(bv) : "v"(v), "s"(gt));
        if (PI == 1) asm volatile("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(av) : "s"(gt));
        else asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(av) : "n"(PI), "s"(gt));
        S.best[t][r] = bv; S.arg[t][r] = av;
    }
}
template <int KS, int UT, bool IDX, int PI, int ROLE>
__device__ __forceinline__ void cpm_update(cpm_state<KS, UT>& S, int t, int r) {
    unsigned long long gt = 0;
    cpm_update_cmp<KS, UT, IDX, PI, ROLE>(S, t, r, gt);
    asm volatile("s_nop 1");
    cpm_update_sel<KS, UT, IDX, PI, ROLE>(S, t, r, gt);
}
// store element (t, r) of window w: ext[u][w][b] (+ idx), 32 consecutive sequences per half-wave.
// Raw buffer stores: one descriptor per array + a 32-bit lane offset that walks the rows (so = the
// element offset of the lane's row, advanced as the stores go: 64 precomputed row pointers were 128
// SGPRs, spilled to lanes and read back with five wait states in front of every store).  The
// descriptor's range check is what makes the wave's first window cheap: it has no predecessor to
// store, so its offsets are parked beyond num_records with stride 0 and the hardware drops the writes
// (a dump word in memory instead had 960 waves hammering the same 4 cache lines: 9 K cycles each).
template <int KS, int UT, bool IDX>
__device__ __forceinline__ void cpm_store(cpm_state<KS, UT>& S, const cpm_args& A, int t, int r) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(S.best[t][r]) ^ S.smask[t][r], A.rext, (int)S.so4, 0, 0);
    if (IDX) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)S.arg[t][r], A.ridx, (int)S.so, 0, 0);
    // next element: row + 1, or + 5 at the end of a group of four (rows 8(r/4) + 4 kh + r%4)
    if (IDX) S.so += (r & 3) == 3 ? S.r5 : S.r1;
    S.so4 += (r & 3) == 3 ? 4u * S.r5 : 4u * S.r1;
}
#define CPM_OOB 0xFFFFFF00u

// element offset, inside the group's rows, of the lane's first row (tile 0, r = 0) of window w
__device__ __forceinline__ uint32_t cpm_store_origin(const cpm_args& A, int w) {
    return (uint32_t)((4 * A.kh * A.n + w) * A.Bs + A.b);
}

// One position: its MFMAs with the neighbouring positions' vector work dealt out behind them.
// Vector units of position I of window w, in order:
//   I == 6: the next window's words; then the operands of position I + 1 (of the next window for I == 6);
//   I == 0: update with position 6 of window w - 1 (set B), then the stores of the first half of the
//           tiles of window w - 1 (the wave's first window has no predecessor: it runs the same code
//           on don't-care registers and its stores are dropped by the range check);
//   I == 1: the stores of the other tiles of window w - 1, then the update (an assignment) with position 0;
//   I >= 2: the update with position I - 1.
// The MFMAs are inline assembly: accumulators in arch VGPRs (the update reads them directly; the
// compiler's own choice at one wave per SIMD is AccVGPRs, one v_accvgpr_read per element and
// position), filter fragments and B operands in AccVGPRs.  What the compiler then cannot see is the
// matrix-pipe hazard "MFMA result read by a vector instruction": the updates of a position come
// behind at least CPM_GUARD MFMAs of the next one (>= 64 cycles of matrix pipe), and the wave's last
// position is followed by explicit wait states.
#define CPM_GUARD 2
// compile-time loop (the bodies index register arrays: nothing may be left to the loop unroller,
// whose size limit once left a position rolled and the whole state in scratch)
template <int K0, int K1, typename F>
__device__ __forceinline__ void cpm_static_for(F&& f) {
    if constexpr (K0 < K1) {
        f(std::integral_constant<int, K0>{});
        cpm_static_for<K0 + 1, K1>(f);
    }
}
// the vector units of position I and the MFMA each one is issued behind
template <int KS, int UT, int I> struct cpm_sched {
    static constexpr int NM = 3 * KS * UT;
    static constexpr int T0 = (UT + 1) / 2;                     // tiles stored at position 0
    static constexpr int NX = I == 6 ? 1 : 0, NG = KS, NE = 16 * UT;
    static constexpr int NS0 = I == 0 ? 16 * T0 : 0;            // after the updates
    static constexpr int NS1 = I == 1 ? 16 * (UT - T0) : 0;     // before the updates
    // weights in units of ~5 issue cycles (tools/mfma_probe.hip: a vector instruction behind an MFMA
    // ~5, a store ~30): words 12, operand 5, update 3 (assignment 1), a pair of stores + offsets 9
    static constexpr int WX = 12, WG = 5, WE = (I == 1) ? 1 : 3, WS = 9;
    static constexpr int TOT = NX * WX + NG * WG + NE * WE + (NS0 + NS1) * WS;
    static constexpr int NU = NX + NG + NS1 + NE + NS0;
    static constexpr int E0 = NX + NG + NS1;                    // first update unit
    static constexpr int weight(int k) {
        return k < NX ? WX : k < NX + NG ? WG : k < E0 ? WS : k < E0 + NE ? WE : WS;
    }
    static constexpr int slot(int k) {
        int cum = 0;
        for (int j = 0; j < k; ++j) cum += weight(j);
        int sl = (cum * NM) / (TOT > 0 ? TOT : 1);
        // the updates (and the stores behind them) not before CPM_GUARD MFMAs of this position
        if (k >= E0 && sl < CPM_GUARD) sl = CPM_GUARD < NM ? CPM_GUARD : NM - 1;
        return sl < NM ? sl : NM - 1;
    }
    static constexpr int first_unit(int m) {                    // first unit with slot >= m
        int k = 0;
        while (k < NU && slot(k) < m) ++k;
        return k;
    }
};

template <int KS, int UT, bool IDX, int I>
__device__ __forceinline__ void cpm_position(cpm_state<KS, UT>& S, const cpm_args& A, int w) {
    typedef cpm_sched<KS, UT, I> SC;
    constexpr int NM = SC::NM;
    constexpr int RM = cpm_role(I), RN = cpm_role((I + 1) % POOLW), RP = cpm_role((I + POOLW - 1) % POOLW);
    constexpr int PI = (I + POOLW - 1) % POOLW;
    unsigned long long gt[3] = {0, 0, 0};
    cpm_static_for<0, NM>([&](auto mc) {
        constexpr int m = decltype(mc)::value;
        constexpr int pc = 2 - m / (KS * UT), ks = (m / UT) % KS, t = m % UT;
        if constexpr (m < UT)
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0"
                         : "=&v"(S.acc[RM][t]) : "a"(S.Wr[t][ks][pc]), "a"(S.bop[RM][ks]));
        else
            asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0"
                         : "+v"(S.acc[RM][t]) : "a"(S.Wr[t][ks][pc]), "a"(S.bop[RM][ks]));
        cpm_static_for<SC::first_unit(m), SC::first_unit(m + 1)>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if constexpr (k < SC::NX) {
                cpm_window_words(S, A, w + 1);
            } else if constexpr (k < SC::NX + SC::NG) {
                cpm_operand<KS, UT, (I + 1) % POOLW, k - SC::NX, RN>(S, A);
            } else if constexpr (k < SC::E0) {
                constexpr int e = k - SC::NX - SC::NG;
                cpm_store<KS, UT, IDX>(S, A, SC::T0 + e / 16, e % 16);
            } else if constexpr (k < SC::E0 + SC::NE) {
                constexpr int e = k - SC::E0;
                if constexpr (e == 0 && NM <= CPM_GUARD) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
                cpm_update_cmp<KS, UT, IDX, PI, RP>(S, e / 16, e % 16, gt[e % 3]);
                if constexpr (e > 1) cpm_update_sel<KS, UT, IDX, PI, RP>(S, (e - 2) / 16, (e - 2) % 16, gt[(e - 2) % 3]);
                if constexpr (e == SC::NE - 1) {
                    cpm_update_sel<KS, UT, IDX, PI, RP>(S, (e - 1) / 16, (e - 1) % 16, gt[(e - 1) % 3]);
                    cpm_update_sel<KS, UT, IDX, PI, RP>(S, e / 16, e % 16, gt[e % 3]);
                }
            } else {
                constexpr int e = k - SC::E0 - SC::NE;
                cpm_store<KS, UT, IDX>(S, A, e / 16, e % 16);
            }
        });
        __builtin_amdgcn_sched_barrier(0);
    });
}

template <int KS, int UT, bool IDX>
__device__ __forceinline__ void cpm_window(cpm_state<KS, UT>& S, const cpm_args& A, int w) {
    cpm_position<KS, UT, IDX, 0>(S, A, w);
    cpm_position<KS, UT, IDX, 1>(S, A, w);
    cpm_position<KS, UT, IDX, 2>(S, A, w);
    cpm_position<KS, UT, IDX, 3>(S, A, w);
    cpm_position<KS, UT, IDX, 4>(S, A, w);
    cpm_position<KS, UT, IDX, 5>(S, A, w);
    cpm_position<KS, UT, IDX, 6>(S, A, w);
}

// The filter fragments go straight into AccVGPRs (through the compiler they came as 30 loads into
// VGPRs + 120 v_accvgpr_write); nothing else the compiler sees depends on them, so the kernel waits
// for them explicitly (s_waitcnt vmcnt(0) before the first window).
template <int KS, int UT>
__device__ __forceinline__ void cpm_load_fragments(cpm_state<KS, UT>& S, const cu32x4* wsrc) {
    cpm_static_for<0, UT * KS * 3>([&S, wsrc](auto ic) {
        constexpr int i = decltype(ic)::value;           // (t, ks, pc) in table order
        cu32x4& dst = S.Wr[i / (KS * 3)][(i / 3) % KS][i % 3];
        const cu32x4* src = wsrc + 64 * i;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(dst) : "v"(src));
    });
}

// ---------------------------------------------------------------------------------------------
// BatchNorm1's batch statistics inside the filter-bank launch (train forward, one-hot input).
// The filter bank needs none of them (the sign of gamma1 is folded into Wf / Wsg by the tables), and
// at one wave per SIMD its grid leaves SIMDs idle: so the launch carries `naux` more one-wave
// workgroups (the leading z slices of the grid; ids past naux return at once) that do the work of
// moments_kernel and prep1_stats_kernel<true> beside it, off the step's critical path:
//   phase 1  input moments from the bit masks bm: item (d, a, h) = the two base pairs (a, 2h) and
//            (a, 2h + 1) at gap d, 8k items dealt over the workgroups; exact integer pair counts per
//            position, window sums from their prefix sums -> G, m (every entry an exact count /
//            (B Lo): any split of the items gives the same bits);
//   hand-off G and m stored write-through (agent-scope relaxed atomic stores), drained, then one
//            relaxed ticket add per workgroup; every workgroup polls the ticket relaxed with s_sleep
//            until all naux have arrived and then makes ONE agent-scope acquire;
//   phase 2  the BatchNorm1 fold of units id, id + naux, ... (up to BN1_NU of them per pass over G):
//            prep1_stats_kernel<true>'s fp64 arithmetic in its order -- lane l plays that kernel's
//            threads l and l + 64, and the two 64-lane sums are added as its red[0] + red[1];
//            the units' wave sums run side by side and lane uu finishes unit uu.
// Where the chain's time goes at C2 (tools/cpm_stamp.hip, profiles/r33_bn1_chain_stamps.txt): phase 1
// 8.8 us, waiting for the last ticket 4.4, the two trips over G 7.4, sums and finish 1.7 -- 22.6 us
// beside a filter bank of 26.
// Progress does not depend on dispatch order or XCD placement: only these workgroups wait, they wait
// only for each other, and the filter-bank waves never wait for anything.  naux is far below the
// waves the chip holds at once (>= 1024), so the filter-bank waves in front of a waiting workgroup
// finish and every auxiliary workgroup is eventually dispatched, whatever the order.  The wait is
// bounded all the same (BN1_SPIN_TICKS, far above any launch of this kernel): past it the workgroup
// sets EXPLAINN_FLAG_BN1_TIMEOUT in the context's flags word and skips phase 2.
// ---------------------------------------------------------------------------------------------
struct cpm_bn1_args {
    const unsigned long long* bm; double* G; double* m;
    const float* conv_w; const float* conv_b; const float* g1; const float* b1;
    float* rm; float* rv; int64_t* nbt;
    float* alpha; float* shift; double* mug; double* sig1; double* Gw;
    int* ticket; int* flags;
    int naux, nz;                // auxiliary workgroups, the leading z slices that hold them (0: none)
    int U, U4, k, B, L, Lp;
};
typedef __attribute__((address_space(1))) unsigned long long bn1_gu64;
typedef __attribute__((address_space(1))) int bn1_gi32;
typedef __attribute__((address_space(1))) float bn1_gf32;
// Register budget: the chain is dependent round trips (~1 us each beside the matrix load), so it
// holds as many loads in flight as the form's registers allow without raising its arch VGPR count
// past what its occupancy leaves (VGPRs and AccVGPRs share one file).  The forms with one wave per
// SIMD anyway (UT = 2, KS >= 2: 196..203 arch VGPRs + 68..172 AccVGPRs of 512) take four position
// passes at once, six tiles of each (72 64-bit loads), and 38 rows of G per round trip; the others
// stay under the ~110 arch VGPRs of the UT = 1 forms (two passes of three tiles, 12 rows), or a form
// loses a wave per SIMD.
template <int KS, int UT> struct bn1_cfg {
    static constexpr bool big = UT == 2 && KS >= 2;
    static constexpr int PQ = big ? 4 : 2;    // phase 1: 64-position passes per round trip
    static constexpr int TQ = big ? 6 : 3;    // phase 1: 64-sequence tiles of each pass per round trip (3 loads each)
    static constexpr int CH = big ? 38 : 12;  // phase 2: rows of G per round trip (k = 19: 76 rows, two trips)
};
#define BN1_NU 2                 // phase 2: units per pass over G
#define BN1_SPIN_TICKS 10000000ull   // 100 ms of the 100 MHz wall clock

__device__ __forceinline__ void bn1_store(double* p, double v) {
    __hip_atomic_store((bn1_gu64*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// phase 1, item (d, a, h): base a against the partner bases a' = 2h, 2h + 1 at gap d.  Lane =
// position q of a 64-position pass; P = inclusive prefix sums of the pair counts over q (exact
// integers), G[(a,j),(a',j+d)] = (P(j+Lo-1) - P(j-1)) / (B Lo), kept by lane j.  The passes of a
// round trip are counted first and their scans run side by side (one scan depth per PQ passes).
// P(j-1) is the first pass's exclusive scan at lane j; P(j+Lo-1) lies in one of two passes; every
// other pass only adds its total to the carry.
template <int TQ, int PQ>
__device__ __forceinline__ void bn1_moments_item(const cpm_bn1_args& X, int item, int lane) {
    const int d = item >> 3, a = (item >> 1) & 3, ab = (item & 1) * 2;
    const int NT = (X.B + 63) / 64, Lo = X.L - X.k + 1, K4 = 4 * X.k;
    const size_t plane = (size_t)NT * X.Lp;
    const unsigned long long* __restrict__ m0 = X.bm + (size_t)a * plane;
    const unsigned long long* __restrict__ m1 = X.bm + (size_t)ab * plane + d;
    long long carry[2] = {0, 0}, plo[2] = {0, 0}, phi[2] = {0, 0};
    const int jhi = lane + Lo - 1;
    const int pa = (Lo - 1) >> 6;                          // the passes that hold a P(jhi): pa, pa + 1
    for (int p0 = 0; p0 * 64 < X.L; p0 += PQ) {
        int c[PQ][2], qo[PQ];
        bool ok[PQ];
#pragma unroll
        for (int p = 0; p < PQ; ++p) {
            const int q = (p0 + p) * 64 + lane;
            ok[p] = q + d < X.L;
            qo[p] = min(q, X.L - 1 - d);                   // (a lane past the end reads a valid word and counts 0)
            c[p][0] = c[p][1] = 0;
        }
        for (int t0 = 0; t0 < NT; t0 += TQ) {              // 3 PQ TQ loads in flight
            unsigned long long x0[PQ][TQ], x1[PQ][2][TQ];
#pragma unroll
            for (int p = 0; p < PQ; ++p)
#pragma unroll
                for (int i = 0; i < TQ; ++i) {
                    const size_t o = (size_t)min(t0 + i, NT - 1) * X.Lp + qo[p];
                    x0[p][i] = m0[o];
                    x1[p][0][i] = m1[o];
                    x1[p][1][i] = m1[plane + o];
                }
#pragma unroll
            for (int p = 0; p < PQ; ++p)
#pragma unroll
                for (int i = 0; i < TQ; ++i)
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        c[p][s] += (ok[p] && t0 + i < NT) ? __popcll(x0[p][i] & x1[p][s][i]) : 0;
        }
        int v[PQ][2];
#pragma unroll
        for (int p = 0; p < PQ; ++p) { v[p][0] = c[p][0]; v[p][1] = c[p][1]; }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
#pragma unroll
            for (int p = 0; p < PQ; ++p)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int y = __shfl_up(v[p][s], off, 64);
                    if (lane >= off) v[p][s] += y;
                }
#pragma unroll
        for (int p = 0; p < PQ; ++p) {
            const int pg = p0 + p;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (pg == 0) plo[s] = v[p][s] - c[p][s];
                if (pg == pa || pg == pa + 1) {
                    const int vhi = __shfl(v[p][s], jhi & 63, 64);
                    if ((jhi >> 6) == pg) phi[s] = carry[s] + vhi;
                }
                carry[s] += __builtin_amdgcn_readlane(v[p][s], 63);
            }
        }
    }
    const int j = lane;
    if (j < X.k - d) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const long long sj = phi[s] - plo[s];
            const double v = (double)sj / ((double)X.B * (double)Lo);
            const int row = a * X.k + j, col = (ab + s) * X.k + j + d;
            bn1_store(X.G + (size_t)row * K4 + col, v);
            bn1_store(X.G + (size_t)col * K4 + row, v);
            if (row == col) bn1_store(X.m + row, v);
        }
    }
}

// phase 2: the BatchNorm1 fold of up to BN1_NU units (us[0..nu)) in one pass over G.  The units'
// parameters and running statistics are asked for together with the filters and m, in front of the
// passes over G; lane uu plays prep1_stats_kernel's thread 0 of unit us[uu] and finishes the fold of
// its unit beside the other lanes'.
template <int CH>
__device__ __forceinline__ void bn1_fold_units(const cpm_bn1_args& X, const int (&us)[BN1_NU], int nu, int lane) {
    const int K4 = 4 * X.k, Lo = X.L - X.k + 1;
    const int i0 = lane, i1 = lane + 64;                   // the two columns of this lane
    const int c0i = min(i0, K4 - 1), c1i = min(i1, K4 - 1);
    float wl[BN1_NU][2];
#pragma unroll
    for (int uu = 0; uu < BN1_NU; ++uu) {
        const int u = min(us[uu], X.U - 1);
        wl[uu][0] = X.conv_w[(size_t)u * K4 + c0i];
        wl[uu][1] = X.conv_w[(size_t)u * K4 + c1i];
    }
    const double m0 = X.m[c0i], m1 = X.m[c1i];
    int ul = us[0];
#pragma unroll
    for (int uu = 1; uu < BN1_NU; ++uu) ul = lane == uu ? us[uu] : ul;
    const bool fin = lane < nu && ul < X.U;                // this lane finishes unit ul
    // the units' five scalars in ONE register across the passes over G: lane 8 uu + f asks for
    // scalar f of unit us[uu] (g1, b1, conv_b, rm, rv)
    float par = 0.f;
    static_assert(BN1_NU <= 8, "lane 8 uu + f: eight units' scalars fit the wave");
    {
        const int pu = lane >> 3, pf = lane & 7;
        int uq = us[0];
#pragma unroll
        for (int uu = 1; uu < BN1_NU; ++uu) uq = pu == uu ? us[uu] : uq;
        // (the array bases go through an opaque asm: a select among kernel arguments the compiler can
        // see becomes an indexed table of them in scratch, for every wave of the launch)
        unsigned long long ps[5] = {(unsigned long long)X.g1, (unsigned long long)X.b1, (unsigned long long)X.conv_b,
                                    (unsigned long long)X.rm, (unsigned long long)X.rv};
#pragma unroll
        for (int f = 0; f < 5; ++f) asm volatile("" : "+s"(ps[f]));
        unsigned long long pa = ps[4];
#pragma unroll
        for (int f = 3; f >= 0; --f) pa = pf == f ? ps[f] : pa;
        if (pu < nu && pf < 5 && uq < X.U) par = ((const bn1_gf32*)pa)[uq];
    }
    // (G w)[i] = sum_c G[c][i] w[c]: even c into ge, odd c into go, in prep1_stats_kernel's order
    double ge[BN1_NU][2], go[BN1_NU][2];
#pragma unroll
    for (int uu = 0; uu < BN1_NU; ++uu) ge[uu][0] = ge[uu][1] = go[uu][0] = go[uu][1] = 0;
    for (int cb = 0; cb < K4; cb += CH) {
        double gv[CH][2];
#pragma unroll
        for (int cc = 0; cc < CH; ++cc) {
            const int c = min(cb + cc, K4 - 1);
            gv[cc][0] = X.G[(size_t)c * K4 + c0i];
            gv[cc][1] = X.G[(size_t)c * K4 + c1i];
        }
#pragma unroll
        for (int cc = 0; cc < CH; cc += 2) {
            const int c = cb + cc;
            if (c < K4) {                                  // (K4 = 4k is even: rows come in pairs)
#pragma unroll
                for (int uu = 0; uu < BN1_NU; ++uu) {
                    const float we = __int_as_float(__builtin_amdgcn_readlane(
                        __float_as_int(c < 64 ? wl[uu][0] : wl[uu][1]), c & 63));
                    const float wo = __int_as_float(__builtin_amdgcn_readlane(
                        __float_as_int(c + 1 < 64 ? wl[uu][0] : wl[uu][1]), (c + 1) & 63));
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        ge[uu][h] = fma(gv[cc][h], (double)we, ge[uu][h]);
                        go[uu][h] = fma(gv[cc + 1][h], (double)wo, go[uu][h]);
                    }
                }
            }
        }
    }
    STAMP(4);
    // prep1_stats_kernel's thread i (i < K4) holds mu_p = w_i m_i and q_p = w_i (G w)_i; its block
    // sum is wave 0's sum (threads 0..63) + wave 1's (64..127).  The sums of all units side by side.
    double sm[BN1_NU][2][2];                               // [unit][mu_p, q_p][wave]
#pragma unroll
    for (int uu = 0; uu < BN1_NU; ++uu) {
        const bool live = uu < nu && us[uu] < X.U;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = h ? i1 : i0;
            const double gw = ge[uu][h] + go[uu][h];
            double mu_p = 0, q_p = 0;
            if (live && i < K4) {
                X.Gw[(size_t)us[uu] * K4 + i] = gw;
                mu_p = fma((double)wl[uu][h], h ? m1 : m0, mu_p);
                q_p = fma((double)wl[uu][h], gw, q_p);
            }
            sm[uu][0][h] = mu_p;
            sm[uu][1][h] = q_p;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)                 // (wave_sum_d of each, in step)
#pragma unroll
        for (int uu = 0; uu < BN1_NU; ++uu)
#pragma unroll
            for (int w = 0; w < 2; ++w)
#pragma unroll
                for (int h = 0; h < 2; ++h) sm[uu][w][h] += __shfl_xor(sm[uu][w][h], off, 64);
    double mu = sm[0][0][0] + sm[0][0][1], wGw = sm[0][1][0] + sm[0][1][1];
#pragma unroll
    for (int uu = 1; uu < BN1_NU; ++uu) {
        const double mu_u = sm[uu][0][0] + sm[uu][0][1], wGw_u = sm[uu][1][0] + sm[uu][1][1];
        mu = lane == uu ? mu_u : mu;
        wGw = lane == uu ? wGw_u : wGw;
    }
    float sc[5];                                           // g1, b1, conv_b, rm, rv of this lane's unit
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        sc[f] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(par), f));
#pragma unroll
        for (int uu = 1; uu < BN1_NU; ++uu)
            sc[f] = lane == uu ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(par), 8 * uu + f)) : sc[f];
    }
    if (fin)
        bn1_fold_finish(mu, wGw, ul, sc[0], sc[1], sc[2], sc[3], sc[4], X.B, Lo, X.alpha, X.shift, X.mug, X.sig1,
                        X.rm, X.rv, X.nbt);
    else if (lane < nu) { X.alpha[ul] = 0.f; X.shift[ul] = 0.f; }      // (a padding row of the unit grid)
}

// one auxiliary workgroup (id < naux): phase 1, the hand-off, phase 2
template <int KS, int UT>
__device__ __forceinline__ void cpm_bn1(const cpm_bn1_args& X, int id, int lane) {
    typedef bn1_cfg<KS, UT> cfg;
    STAMP(0);
    for (int item = id; item < 8 * X.k; item += X.naux) bn1_moments_item<cfg::TQ, cfg::PQ>(X, item, lane);
    // publish: the write-through stores of G / m drained, then this workgroup's ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    STAMP(1);
    if (lane == 0) __hip_atomic_fetch_add((bn1_gi32*)X.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // wait for every auxiliary workgroup: relaxed polls, bounded, then ONE agent-scope acquire
    const unsigned long long t0 = wall_clock64();
    while (__builtin_amdgcn_readfirstlane(
               __hip_atomic_load((bn1_gi32*)X.ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < X.naux) {
        if (wall_clock64() - t0 > BN1_SPIN_TICKS) {
            if (lane == 0)
                __hip_atomic_fetch_or((bn1_gi32*)X.flags, EXPLAINN_FLAG_BN1_TIMEOUT, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    STAMP(2);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    STAMP(3);
    for (int u0 = id; u0 < X.U4; u0 += BN1_NU * X.naux) {
        int us[BN1_NU], nu = 0;
#pragma unroll
        for (int uu = 0; uu < BN1_NU; ++uu) {
            us[uu] = u0 + uu * X.naux;
            if (us[uu] < X.U4) nu = uu + 1;
        }
        bn1_fold_units<cfg::CH>(X, us, nu, lane);
    }
    STAMP(5);
}

template <int KS, int UT, bool IDX>
__global__ __launch_bounds__(64, (UT == 1 && KS <= 5) ? 2 : 1) void conv_pool_mm_kernel(
    const uint32_t* __restrict__ pk2, const uint32_t* __restrict__ nmask,
    const cu32x4* __restrict__ Wf, const cu32x4* __restrict__ Wsg,
    float* __restrict__ ext, uint8_t* __restrict__ idx, int n, int Bs, int PW, int NW, int wper,
    const cpm_bn1_args bn1) {
    __shared__ __attribute__((aligned(1024))) cu32x4 oh[64];      // [N bits of the two taps][code pair]
    typedef __attribute__((address_space(3))) char lds_char;
    const int lane = threadIdx.x;
    if constexpr (IDX) {      // (train forward) the leading bn1.nz z slices: BatchNorm1's workgroups
        if ((int)blockIdx.z < bn1.nz) {
            const int id = ((int)blockIdx.z * (int)gridDim.y + (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x;
            if (id < bn1.naux) cpm_bn1<KS, UT>(bn1, id, lane);
            return;
        }
    }
    STAMP(0);
    {
        const int c4 = lane & 15, nb = lane >> 4;
        uint32_t r[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cde = (c4 >> (2 * h)) & 3;
            const uint32_t one = ((nb >> h) & 1) ? 0u : 0x3F80u;     // bf16 1.0
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q == 2 * h + (cde >> 1)) r[q] = one << (16 * (cde & 1));
        }
        oh[lane] = cu32x4{r[0], r[1], r[2], r[3]};
    }
    cpm_state<KS, UT> S;
    cpm_args A;
    A.pk2 = pk2; A.nmask = nmask; A.ext = ext; A.idx = idx; A.n = n; A.Bs = Bs; A.PW = PW; A.NW = NW;
    A.t0 = blockIdx.y * UT; A.b = blockIdx.x * 32 + (lane & 31); A.kh = lane >> 5;
    A.tbase = (uint32_t)(size_t)(const lds_char*)oh;
    A.row1 = (uint32_t)(n * Bs); A.row5 = 5u * A.row1;
    {   // descriptors of the group's own 32 UT rows: offsets stay far below 2^31 at any model size
        // (made wave-uniform by hand: a descriptor the compiler cannot prove uniform gets a
        // readfirstlane waterfall loop around every store -- seen in the stamped build of this kernel)
        const size_t row0 = (size_t)32 * A.t0 * n * Bs;
        const int span = __builtin_amdgcn_readfirstlane(32 * UT * n * Bs);
        auto uniform = [](auto* q) {
            const unsigned long long v = reinterpret_cast<unsigned long long>(q);
            const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
            return reinterpret_cast<decltype(q)>(((unsigned long long)hi << 32) | lo);
        };
        A.rext = __builtin_amdgcn_make_buffer_rsrc(uniform(ext + row0), 0, 4 * span, 0x00020000);
        A.ridx = __builtin_amdgcn_make_buffer_rsrc(uniform(idx + row0), 0, span, 0x00020000);
    }
    const int wbeg = (IDX ? (int)blockIdx.z - bn1.nz : (int)blockIdx.z) * wper, wend = min(n, wbeg + wper);
    if (wbeg >= wend) return;
    cpm_load_fragments(S, Wf + (size_t)A.t0 * KS * 3 * 64 + lane);
    cpm_fetch(S, A, wbeg);
    {
        const cu32x4* ssrc = Wsg + ((size_t)A.t0 * 2 + A.kh) * 4;
#pragma unroll
        for (int t = 0; t < UT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const cu32x4 v = ssrc[t * 8 + q];
#pragma unroll
                for (int i = 0; i < 4; ++i) S.smask[t][4 * q + i] = v[i];
            }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    STAMP(1);
    cpm_window_words(S, A, wbeg);
    // operands of the first position
    cpm_static_for<0, KS>([&](auto kc) { cpm_operand<KS, UT, 0, decltype(kc)::value, 0>(S, A); });
    STAMP(2);
    // (one copy of the window code for every window: a separate first-window body doubled the code
    // every wave runs through cold)
#pragma unroll 1
    for (int w = wbeg; w < wend; ++w) {
        const bool first = w == wbeg;
        S.so = first ? CPM_OOB : cpm_store_origin(A, w - 1);
        S.so4 = first ? CPM_OOB : 4u * S.so;
        S.r1 = first ? 0u : A.row1; S.r5 = first ? 0u : A.row5;
        cpm_window<KS, UT, IDX>(S, A, w);
        if (first) STAMP(3);
    }
    STAMP(4);
    // the last window: its position 6 sits in set B (results of the last MFMAs: wait them out)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) cpm_update<KS, UT, IDX, POOLW - 1, 2>(S, t, r);
    S.so = cpm_store_origin(A, wend - 1);
    S.so4 = 4u * S.so;
    S.r1 = A.row1; S.r5 = A.row5;
#pragma unroll
    for (int t = 0; t < UT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) cpm_store<KS, UT, IDX>(S, A, t, r);
    STAMP(5);
}

static int conv_pool_mm_ut(const explainn_ctx* c) {
    if (const char* e = getenv("EXPLAINN_CPM_UT")) { const int v = atoi(e); if (v == 1 || (v == 2 && conv_ksteps(c->k) <= 5)) return v; }
    return conv_ut(c->k);
}

static int conv_pool_mm_parts(const explainn_ctx* c, int B, int ut) {
    // Window ranges per (32 sequences, unit group).  A wave costs about one window's worth of fixed
    // work (fragments, table, the cold first pass through the code, the last stores) plus its windows,
    // and the launch takes as many rounds as its waves need SIMD slots: pick the split that minimises
    // rounds x (windows per wave + 1).
    if (const char* e = getenv("EXPLAINN_CPM_PARTS")) { const int v = atoi(e); if (v >= 1) return min(v, c->n); }
    const int groups = ut == 1 ? (c->U + 31) / 32 : conv_tiles_padded(c->U, c->k) / ut, sb = (B + 31) / 32;
    const int cols = groups * sb, slots = (ut == 1 && conv_ksteps(c->k) <= 5) ? 2048 : 1024;
    int best = 1;
    long best_cost = -1;
    for (int p = 1; p <= c->n; ++p) {
        const int wper = (c->n + p - 1) / p, np = (c->n + wper - 1) / wper;
        if (np != p) continue;                                    // (same split as a smaller p)
        const long rounds = ((long)cols * np + slots - 1) / slots;
        const long cost = rounds * (wper + 1);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = p; }
    }
    return best;
}

// BatchNorm1's workgroups in the filter-bank launch (cpm_bn1): one per phase-1 item (d, a, h) and
// two units each in phase 2 at C2.  EXPLAINN_BN1_AUX (experiments; read per step, so that a test can
// run both paths in one process): 0 = the separate launches, N > 0 = N workgroups whatever the shape
// -- at most 256, a quarter of the waves the chip holds at once even at one wave per SIMD, so that
// the progress argument of cpm_bn1 stands.
// Where it pays, measured on MI355X (profiles/r04_bn1_ab.txt): the chain took ~30 us on these
// workgroups then (22.6 since r33, profiles/r33_bn1_chain_stamps.txt; the bounds below are r04's and
// have not been measured again), so it leaves the critical path only beside a one-round filter bank
// about that long.
// C2 (960 workgroups, 200 bp): 0.2029 -> 0.1972 ms per step.  Forced on, the other shapes lose: the
// small grids (100 units x 64 sequences 0.0982 -> 0.1006, 300 x 128 0.1306 -> 0.1390; 104 and 520
// workgroups), multi-round C3 0.550 -> 0.557 and C5 3.45 -> 3.49 (the workgroups take slots from a
// filter bank that has no idle SIMDs), and C4's 1000 bp 1.197 -> 1.213 (phase 1 grows with L).
int conv_pool_bn1_workgroups(const explainn_ctx* c, int B) {
    if (const char* e = getenv("EXPLAINN_BN1_AUX")) return min(max(atoi(e), 0), 256);
    const int ut = conv_pool_mm_ut(c);
    const int parts = conv_pool_mm_parts(c, B, ut);
    const int wper = (c->n + parts - 1) / parts;
    const long blocks = (long)((B + 31) / 32) * (ut == 1 ? (c->U + 31) / 32 : conv_tiles_padded(c->U, c->k) / ut) *
                        ((c->n + wper - 1) / wper);
    const int slots = (ut == 1 && conv_ksteps(c->k) <= 5) ? 2048 : 1024;
    return blocks >= 768 && blocks <= slots && c->L <= 256 ? 8 * c->k : 0;
}

// bn1 != nullptr: the launch also carries BatchNorm1's workgroups (train forward, want_idx)
static int launch_conv_pool_mm(explainn_ctx* c, const explainn_params* p, int B, bool want_idx,
                               cpm_bn1_args* bn1, hipStream_t s) {
    const int ut = conv_pool_mm_ut(c);
    const int parts = conv_pool_mm_parts(c, B, ut);
    const int wper = (c->n + parts - 1) / parts;
    dim3 grid((B + 31) / 32, ut == 1 ? (c->U + 31) / 32 : conv_tiles_padded(c->U, c->k) / ut, (c->n + wper - 1) / wper);
    cpm_bn1_args none = {};
    if (bn1) {
        const int slice = (int)(grid.x * grid.y);
        bn1->nz = (bn1->naux + slice - 1) / slice;
        grid.z += bn1->nz;
    }
    const cpm_bn1_args& bn1v = bn1 ? *bn1 : none;
#define ARGS grid, dim3(64), 0, s, c->pk2, c->nmask, reinterpret_cast<const cu32x4*>(c->Wf), \
             reinterpret_cast<const cu32x4*>(c->Wsg), c->ext, c->idx, c->n, c->Bs, c->PW, c->NW, wper, bn1v
#define CALLKS(KSv, UTv)                                                                        \
    if (want_idx) hipLaunchKernelGGL((conv_pool_mm_kernel<KSv, UTv, true>), ARGS);              \
    else hipLaunchKernelGGL((conv_pool_mm_kernel<KSv, UTv, false>), ARGS);
#define CALLUT(KSv) if (ut == 2) { CALLKS(KSv, 2); } else { CALLKS(KSv, 1); }
    switch (conv_ksteps(c->k)) {
#ifndef CPM_ONLY5     /* (development builds: -DCPM_ONLY5 compiles the k = 17..20 forms only) */
        case 1: { CALLUT(1); } break;
        case 2: { CALLUT(2); } break;
        case 3: { CALLUT(3); } break;
        case 4: { CALLUT(4); } break;
        case 6: { CALLKS(6, 1); } break;
        case 7: { CALLKS(7, 1); } break;
        case 8: { CALLKS(8, 1); } break;
#endif
        case 5: { CALLUT(5); } break;
        default: explainn_set_error("kernel_size %d not instantiated (2..32)", c->k); return EXPLAINN_E_UNSUPPORTED;
    }
#undef CALLUT
#undef CALLKS
#undef ARGS
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

int launch_conv_pool(explainn_ctx* c, const explainn_params* p, int B, bool want_idx, hipStream_t s) {
    return launch_conv_pool_mm(c, p, B, want_idx, nullptr, s);
}

// train forward on one-hot input with the input moments and the BatchNorm1 fold inside the launch
// (naux = conv_pool_bn1_workgroups(c, B) > 0): bm must hold the batch's bit masks and bn1_ticket must be 0
int launch_conv_pool_train(explainn_ctx* c, const explainn_params* p, int B, int naux, hipStream_t s) {
    cpm_bn1_args a = {c->bm, c->G, c->m, p->conv_w, p->conv_b, p->bn1_w, p->bn1_b, p->bn1_rm, p->bn1_rv,
                      p->bn1_nbt, c->alpha, c->shift, c->mug, c->sig1, c->Gw, c->bn1_ticket, c->flags,
                      naux, 0, c->U, c->U4, c->k, B, c->L, c->Lp};
    return launch_conv_pool_mm(c, p, B, true, &a, s);
}

// ---------------------------------------------------------------------------------------------
// model.linears[:3] (test.py:159-160): per-position activations exp(alpha*conv+shift), (B,U,Lo).
// Auxiliary export path: one block per (sequence, unit quad), threads over positions.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_act_kernel(const uint8_t* __restrict__ codesT,
                                                       const float* __restrict__ Wt,
                                                       const float* __restrict__ alpha,
                                                       const float* __restrict__ shift,
                                                       float* __restrict__ acts, int U, int k,
                                                       int L, int Lo, int Bs) {
    extern __shared__ float4 Wsm[];            // [k][5], then codes [L] as bytes
    uint8_t* cs = reinterpret_cast<uint8_t*>(Wsm + k * 5);
    const int b = blockIdx.x, quad = blockIdx.y;
    const float4* src = reinterpret_cast<const float4*>(Wt) + (size_t)quad * k * 5;
    for (int i = threadIdx.x; i < k * 5; i += 256) Wsm[i] = src[i];
    for (int p = threadIdx.x; p < L; p += 256) cs[p] = codesT[(size_t)p * Bs + b];
    __syncthreads();
    for (int p = threadIdx.x; p < Lo; p += 256) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < k; ++j) {
            const float4 v = Wsm[j * 5 + cs[p + j]];
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        const float av[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) {
            const int u = quad * 4 + uu;
            if (u < U) acts[((size_t)b * U + u) * Lo + p] = qval(alpha[u], av[uu], shift[u]);
        }
    }
}

int launch_conv_act(explainn_ctx* c, int B, float* acts, hipStream_t s) {
    const size_t sm = (size_t)c->k * 5 * sizeof(float4) + ((c->L + 15) & ~15);
    hipLaunchKernelGGL(conv_act_kernel, dim3(B, c->Uq), dim3(256), sm, s, c->codesT, c->Wt, c->alpha,
                       c->shift, acts, c->U, c->k, c->L, c->Lo, c->Bs);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
