// The narrow end of the network: BatchNorm3 + ReLU over the batch (architectures/__init__.py:99-100),
// the final nn.Linear(U,T) combiner (:104), the loss (:446-456) and their backward.  All arrays
// here are (U x B) or (B x T) -- a few MB at most -- so these are plain reduction kernels.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Many tasks (T > HEAD_GEMM_MIN_T: configs C3-C5 have 50-164): the combiner and its backward are
// real GEMMs -- logits = o^T Wf^T (K = U), d o = dl Wf (K = T), d Wf = dl^T o^T (K = B) -- and run
// on the fp32 MFMA.  One 256-thread block per 32x32 output tile; its four waves split K in four
// contiguous quarters (each half-wave takes half a quarter: the order of a sum is free, so K is
// permuted to give every lane a contiguous run), partial tiles are added in fixed order through LDS.
// Operands are read straight from global in batches of eight per lane (they are L2-resident:
// at most a few MB).  *_KC = "K-contiguous": element (row, k) at ptr[row*ld + k]; otherwise
// element (k, row) at ptr[k*ld + row] (coalesced across the 32 rows of a tile).
// ---------------------------------------------------------------------------------------------
typedef float f32x16h __attribute__((ext_vector_type(16)));
enum { EPI_PLAIN = 0, EPI_BIAS = 1, EPI_GW = 2 };   // EPI_GW: gridDim.y batch chunks, partial tiles to D[chunk][M][N]

template <bool A_KC, bool B_KC, int EPI>
__global__ __launch_bounds__(256, 2) void gemm32_kernel(const float* __restrict__ A, int lda,
                                                     const float* __restrict__ Bm, int ldb,
                                                     float* __restrict__ D, int ldd, int M, int N,
                                                     int K, const float* __restrict__ bias,
                                                     float* __restrict__ extra) {
    __shared__ float part[3][16][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, rc = lane & 31, kk = lane >> 5;
    const int tiles_n = (N + 31) >> 5;
    const int ti = blockIdx.x / tiles_n, tj = blockIdx.x % tiles_n;
    const int i = ti * 32 + rc, j = tj * 32 + rc;
    const int ic = min(i, M - 1);
    // EPI_GW: column N-1 is a virtual all-ones row of B (it yields the bias gradient)
    const bool ones_col = EPI == EPI_GW && j == N - 1;
    const int jc = min(j, (EPI == EPI_GW ? N - 2 : N - 1));
    // (EPI_GW: this workgroup's chunk [kb0, kb1) of K; otherwise all of K)
    const int Kc = ((K + (int)gridDim.y - 1) / (int)gridDim.y + 7) & ~7;
    const int kb0 = min((int)blockIdx.y * Kc, K), kb1 = min(kb0 + Kc, K);
    const int Kq = (kb1 - kb0 + 3) >> 2;               // this wave's quarter [kq0, kq1)
    const int kq0 = min(kb0 + wave * Kq, kb1), kq1 = min(kq0 + Kq, kb1);
    const int Kh = (kq1 - kq0 + 1) >> 1;               // this half-wave's run [k0, kend)
    const int k0 = kq0 + kk * Kh, kend = min(k0 + Kh, kq1);
    const float* ap = A_KC ? A + (size_t)ic * lda : A + ic;
    const float* bp = B_KC ? Bm + (size_t)jc * ldb : Bm + jc;
    f32x16h acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    for (int s0 = 0; s0 < Kh; s0 += 8) {               // Kh is wave-uniform
        float a[8], b[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int kc = min(k0 + s0 + q, K - 1);
            a[q] = A_KC ? ap[kc] : ap[(size_t)kc * lda];
            b[q] = B_KC ? bp[kc] : bp[(size_t)kc * ldb];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) { KEEP(a[q]); KEEP(b[q]); }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool live = k0 + s0 + q < kend;
            const float av = (live && i < M) ? a[q] : 0.f;
            const float bv = (live && j < N) ? (ones_col ? 1.f : b[q]) : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int g = 0; g < 16; ++g) part[wave - 1][g][lane] = acc[g];
    }
    __syncthreads();
    if (wave == 0 && j < N) {
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int row = ti * 32 + (g & 3) + 8 * (g >> 2) + 4 * kk;
            if (row >= M) continue;
            float v = ((acc[g] + part[0][g][lane]) + part[1][g][lane]) + part[2][g][lane];
            if (EPI == EPI_BIAS) v += bias[j];
            if (EPI == EPI_GW) D[((size_t)blockIdx.y * M + row) * N + j] = v;     // (bias column included)
            else D[(size_t)row * ldd + j] = v;
        }
    }
}

// dlT[t][b] = dl[b][t]   (the GEMMs want the batch index contiguous)
__global__ __launch_bounds__(256) void transpose_dl_kernel(const float* __restrict__ dl,
                                                           float* __restrict__ dlT, int B, int T,
                                                           int Bs) {
    __shared__ float tile[32][33];
    const int b0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8)
        tile[r][tx] = (b0 + r < B && t0 + tx < T) ? dl[(size_t)(b0 + r) * T + t0 + tx] : 0.f;
    __syncthreads();
    for (int r = ty; r < 32; r += 8)
        if (t0 + r < T && b0 + tx < B) dlT[(size_t)(t0 + r) * Bs + b0 + tx] = tile[tx][r];
}


__device__ __forceinline__ double block_sum_256(double v, double* red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// three sums behind ONE pair of barriers (head_bwd: the two BatchNorm3 sums and the combiner-weight
// gradient of the register path used to take three round trips)
__device__ __forceinline__ void block_sum3_256(double& a, double& b, double& c, double* red12) {
    a = wave_sum_d(a); b = wave_sum_d(b); c = wave_sum_d(c);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red12[w] = a; red12[4 + w] = b; red12[8 + w] = c;
    }
    __syncthreads();
    a = (red12[0] + red12[1]) + (red12[2] + red12[3]);
    b = (red12[4] + red12[5]) + (red12[6] + red12[7]);
    c = (red12[8] + red12[9]) + (red12[10] + red12[11]);
}

// The register path of head_fwd_train: this thread's RBX z values stay in registers through the three
// passes (mean, variance, normalise) -- one batch of loads instead of three passes of dependent round
// trips over the same row.  RBX = HEAD_RB = 8 (batch <= 2048) or 16 (batch <= 4096: configuration C3).
template <int RBX>
__device__ __forceinline__ void head_fwd_train_regs(const float* __restrict__ zu, float* __restrict__ zhu,
                                                    float* __restrict__ ou, float gam, float bet, int B,
                                                    int tid, double* red, double& mean, double& var,
                                                    double& sg) {
    float zr[RBX];
#pragma unroll
    for (int i = 0; i < RBX; ++i) zr[i] = zu[min(tid + 256 * i, B - 1)];
#pragma unroll
    for (int i = 0; i < RBX; ++i) KEEP(zr[i]);
    double s = 0;
#pragma unroll
    for (int i = 0; i < RBX; ++i) s += (tid + 256 * i < B) ? (double)zr[i] : 0.0;
    mean = block_sum_256(s, red) / (double)B;
    double v = 0;
#pragma unroll
    for (int i = 0; i < RBX; ++i)
        if (tid + 256 * i < B) { const double d = (double)zr[i] - mean; v = fma(d, d, v); }
    var = block_sum_256(v, red) / (double)B;
    sg = sqrt(var + BN_EPS_D);
    const float meanf = (float)mean, isg = (float)(1.0 / sg);
#pragma unroll
    for (int i = 0; i < RBX; ++i) {
        const int b = tid + 256 * i;
        if (b < B) {
            const float zh = (zr[i] - meanf) * isg;
            zhu[b] = zh;
            ou[b] = fmaxf(fmaf(gam, zh, bet), 0.f);
        }
    }
}

// one block per unit: batch statistics of z, then zhat / o
__global__ __launch_bounds__(256) void head_fwd_train_kernel(
    const float* __restrict__ z, const float* __restrict__ c2, const float* __restrict__ g3,
    const float* __restrict__ b3, float* __restrict__ rm3, float* __restrict__ rv3, int64_t* nbt,
    float* __restrict__ zhat, float* __restrict__ o, float* __restrict__ sig3, int Bs, int B) {
    __shared__ double red[4];
    const int u = blockIdx.x, tid = threadIdx.x;
    const float* zu = z + (size_t)u * Bs;
    const float gam = g3[u], bet = b3[u];
    double mean, var, sg;
    if (B <= HEAD_RB * 256) {
        head_fwd_train_regs<HEAD_RB>(zu, zhat + (size_t)u * Bs, o + (size_t)u * Bs, gam, bet, B, tid, red, mean, var, sg);
    } else if (B <= 16 * 256) {
        head_fwd_train_regs<16>(zu, zhat + (size_t)u * Bs, o + (size_t)u * Bs, gam, bet, B, tid, red, mean, var, sg);
    } else {
        double s = 0;
        for (int b = tid; b < B; b += 256) s += (double)zu[b];
        mean = block_sum_256(s, red) / (double)B;
        double v = 0;
        for (int b = tid; b < B; b += 256) { const double d = (double)zu[b] - mean; v = fma(d, d, v); }
        var = block_sum_256(v, red) / (double)B;
        sg = sqrt(var + BN_EPS_D);
        const float meanf = (float)mean, isg = (float)(1.0 / sg);
        for (int b = tid; b < B; b += 256) {
            const float zh = (zu[b] - meanf) * isg;
            zhat[(size_t)u * Bs + b] = zh;
            o[(size_t)u * Bs + b] = fmaxf(fmaf(gam, zh, bet), 0.f);
        }
    }
    if (tid == 0) {
        sig3[u] = (float)sg;
        rm3[u] = (float)((1 - BN_MOM_D) * (double)rm3[u] + BN_MOM_D * (mean + (double)c2[u]));
        rv3[u] = (float)((1 - BN_MOM_D) * (double)rv3[u] + BN_MOM_D * var * (double)B / (double)(B - 1));
        if (u == 0 && nbt) *nbt += 1;
    }
}

// logits[b][t] = bf[t] + sum_u Wf[t][u] * o[u][b]; one block per (64 sequences, task): its 16
// waves each sum a slice of the units, then the slices are added in fixed order.
// blockIdx.z = member g of a model bank of G members (explainn_create_bank), U its units: the block
// reads rows [g*U, (g+1)*U) of o, Wf[g] (T,U), bf[g] and writes logits[b][g][t] -- local unit u sits
// where unit u of a stand-alone model does, so a member's sum has the stand-alone order.  A
// stand-alone model is the bank of one: G = 1, g = 0, every offset zero.
__global__ __launch_bounds__(1024) void logits_kernel(const float* __restrict__ o,
                                                      const float* __restrict__ Wf,
                                                      const float* __restrict__ bf,
                                                      float* __restrict__ logits, int U, int T,
                                                      int Bs, int B, int G) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + lane, t = blockIdx.y;
    const int g = blockIdx.z, ldl = G * T;
    o += (size_t)g * U * Bs; Wf += (size_t)g * T * U; bf += (size_t)g * T;
    logits += (size_t)g * T;
    const float* wr = Wf + (size_t)t * U;
    float acc = 0.f;
    for (int u0 = wv; u0 < U; u0 += 160) {             // ten units (twenty loads) in flight
        float wq[10], oq[10];
#pragma unroll
        for (int q = 0; q < 10; ++q) {
            const int u = min(u0 + 16 * q, U - 1);
            wq[q] = wr[u];
            oq[q] = o[(size_t)u * Bs + b];
        }
#pragma unroll
        for (int q = 0; q < 10; ++q) { KEEP(wq[q]); KEEP(oq[q]); }
#pragma unroll
        for (int q = 0; q < 10; ++q) acc = fmaf(u0 + 16 * q < U ? wq[q] : 0.f, oq[q], acc);
    }
    part[wv][lane] = acc;
    __syncthreads();
    if (wv == 0 && b < B) {
        float s = bf[t];
#pragma unroll
        for (int i = 0; i < 16; ++i) s += part[i][lane];
        logits[(size_t)b * ldl + t] = s;
    }
}

// Train forward, few tasks: BatchNorm3's batch statistics are FINISHED here, inside the combiner
// launch, from the per-workgroup fp64 sums of z and z^2 fc_fwd left in z12p -- head_fwd_train's
// launch (~5 us for 300 x 1024 values) disappears.  Every block rebuilds the statistics of all units
// (U x NBLK pairs of doubles, a few KB from L2), normalises its 64 sequences on the fly and sums the
// combiner; the blocks of task 0 also store zhat and o for the backward, block (0, 0) the running
// statistics.  Same grid and summation order as logits_kernel.
// blockIdx.z = member g and U = its units, as in logits_kernel; a block rebuilds the statistics of
// its own member's units only (LDS U x 20 B), the blocks of task 0 OF EACH MEMBER store zhat / o,
// block (0, 0) of each member its running statistics, member 0's the shared num_batches_tracked.
// (The member offsets are block-uniform: they cost scalar registers, none of the kernel's 128 vector ones.)
//
// TT > 0 is the form of the training step with few tasks and more than 512 sequences (G = 1; grid.y
// counts the unit groups of head_sums below, and every group does all of this paragraph for its 64
// sequences): the block sums all TT tasks of its 64 sequences (TT weight rows in LDS, the sums of task t in
// the order the block of task t has above, so the logits keep their bits), and with the logits of
// its sequences in hand goes on to the loss gradient and its share of the head backward's batch sums
// (head_sums below): the per-unit head backward launch that re-read all of this disappears.
struct head_sums_args {
    const float* y; int kind;          // targets (B,T), loss kind
    float* dl;                         // out: d loss / d logits (B,T)
    double *hp, *hb;                   // out: per-block partials (common.h)
};

// The block's part of the head backward, entered with the logits s[t] of sequence b in wave 0.
// Wave 0: dl = loss_grad for its 64 sequences (0 for the dead ones), to memory and through LDS to
// everybody; the block's sums of dl and of the loss terms to hb.  Then every thread takes (unit, eight
// sequences): z from memory (the previous launch's output: two 16-byte loads per unit, PC units in
// flight), zhat and o by the forward's own expressions, and in fp64, sequence order
//   s1 = sum d3,  s2 = sum d3 zhat,  gw[t] = sum dl[b][t] o     d3 = o > 0 ? sum_t dl[b][t] Wf[t][u] : 0
// the eight threads of a unit are adjacent lanes: three butterfly steps, one store of 2 + T doubles
// per (unit, block).  Plain stores: passA, the next launch but one, adds the blocks up.
//
// Unit groups (gridDim.y = R > 1): the R blocks of a sequence block all hold the same logits (phase 1
// is run by each of them in full).  Group 0 is the one that stores -- zhat, o, logits, dl, hb -- and so
// carries wave 0's whole stretch; it takes no units.  Groups 1 .. R-1 form dl for LDS alone and share
// the units: group r takes [(r - 1) U / (R - 1), r U / (R - 1)), never empty because R - 1 <= U.  (With
// an even share for group 0 as well it finished 2.5 K cycles behind the others: phase 1 and wave 0's
// stretch are what bounds the launch, profiles/r29_head_groups_stamps.txt.)  Nothing here reads what
// another block of the launch stored -- that is why z and not the stored zhat is read.  Every row of
// hp is still written exactly once.  R = 1: the one block does all of it.

// units per thread and round trip: with three and four tasks more than one spilled, and with unit
// groups one is all a thread has up to 128 units per group
template <int T> struct head_sums_pc { static constexpr int value = T <= 2 ? 3 : 1; };

// the z values of this thread's (unit c0 + 128 q, eight sequences from b0): loads only, nothing waits
template <int PC>
__device__ __forceinline__ void head_sums_load(const float* __restrict__ z, int c0, int uhi, int Bs, int b0,
                                               float (&zv)[PC][8]) {
#pragma unroll
    for (int q = 0; q < PC; ++q) {
        const float4* src = reinterpret_cast<const float4*>(z + (size_t)min(c0 + 128 * q, uhi - 1) * Bs + b0);
        const float4 v0 = src[0], v1 = src[1];
        zv[q][0] = v0.x; zv[q][1] = v0.y; zv[q][2] = v0.z; zv[q][3] = v0.w;
        zv[q][4] = v1.x; zv[q][5] = v1.y; zv[q][6] = v1.z; zv[q][7] = v1.w;
    }
}

// zv: the loads of the first trip (c0 = ulo + tid / 8), issued by the caller in front of its barrier
template <int T>
__device__ __forceinline__ void head_sums(const head_sums_args& hs, const float (&s)[T], float4* st4,
                                          const float* wl, const float* __restrict__ z,
                                          float (&zv)[head_sums_pc<T>::value][8], int U, int ulo, int uhi,
                                          int Bs, int B) {
    __shared__ float dls[T][64];
    const int tid = threadIdx.x, lane = tid & 63, blk = blockIdx.x;
    const bool first = blockIdx.y == 0;                // the group that stores dl and hb (block-uniform)
    STAMP(2);
    if (tid < 64) {                                    // wave 0
        const int b = blk * 64 + lane;
        const float invN = 1.0f / (float)(B * T);
        double lacc = 0;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            float d = 0.f;
            if (b < B) {
                const float yv = hs.y[b * T + t];
                d = loss_grad(hs.kind, s[t], yv, invN);
                if (first) {
                    lacc += (double)loss_value(hs.kind, s[t], yv);
                    hs.dl[b * T + t] = d;
                }
            }
            dls[t][lane] = d;
            if (first) {
                const double sd = wave_sum_d((double)d);
                if (lane == 0) hs.hb[blk * (T + 1) + t] = sd;
            }
        }
        if (first) {
            const double sl = wave_sum_d(lacc);
            if (lane == 0) hs.hb[blk * (T + 1) + T] = sl;
        }
    }
    __syncthreads();
    STAMP(3);
    constexpr int PC = head_sums_pc<T>::value;
    const int seg = tid & 7, b0 = blk * 64 + 8 * seg, nb = gridDim.x;
    const int cf = ulo + (tid >> 3);
    for (int c0 = cf; c0 < uhi; c0 += 128 * PC) {
        if (c0 != cf) head_sums_load<PC>(z, c0, uhi, Bs, b0, zv);
#pragma unroll
        for (int q = 0; q < PC; ++q)
#pragma unroll
            for (int i = 0; i < 8; ++i) KEEP(zv[q][i]);
        STAMP_AFTER_LOADS(4);
#pragma unroll
        for (int q = 0; q < PC; ++q) {
            const int u = c0 + 128 * q;
            if (u >= uhi) continue;                    // (the eight lanes of a unit agree; whole waves skip)
            const float4 sv = st4[u];
            float wf[T];
#pragma unroll
            for (int t = 0; t < T; ++t) wf[t] = wl[t * U + u];
            double s1 = 0, s2 = 0, gw[T];
#pragma unroll
            for (int t = 0; t < T; ++t) gw[t] = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                // (a dead sequence's z is whatever the memory holds: masked here.  Its dl is 0, so its
                // finite o and d3 = 0 add nothing: one select per element, not three)
                const float zh = b0 + i < B ? (zv[q][i] - sv.x) * sv.y : 0.f;
                const float ov = fmaxf(fmaf(sv.z, zh, sv.w), 0.f);
                float dob = 0.f;
#pragma unroll
                for (int t = 0; t < T; ++t) {
                    const float dlv = dls[t][8 * seg + i];
                    dob = fmaf(dlv, wf[t], dob);
                    gw[t] = fma((double)dlv, (double)ov, gw[t]);
                }
                const float d3 = ov > 0.f ? dob : 0.f;
                s1 += (double)d3;
                s2 = fma((double)d3, (double)zh, s2);
            }
#pragma unroll
            for (int off = 1; off < 8; off <<= 1) {
                s1 += __shfl_xor(s1, off, 64);
                s2 += __shfl_xor(s2, off, 64);
#pragma unroll
                for (int t = 0; t < T; ++t) gw[t] += __shfl_xor(gw[t], off, 64);
            }
            if (seg == 0) {
                double* dst = hs.hp + ((size_t)u * nb + blk) * (2 + T);
                dst[0] = s1; dst[1] = s2;
#pragma unroll
                for (int t = 0; t < T; ++t) dst[2 + t] = gw[t];
            }
        }
    }
}

template <int TT>
__global__ __launch_bounds__(1024) void logits_bn_kernel(
    const float* __restrict__ z, const double* __restrict__ z12p, int nblk, const float* __restrict__ c2, const float* __restrict__ g3, const float* __restrict__ b3,
    float* __restrict__ rm3, float* __restrict__ rv3, int64_t* nbt, float* __restrict__ zhat,
    float* __restrict__ o, float* __restrict__ sig3, const float* __restrict__ Wf,
    const float* __restrict__ bf, float* __restrict__ logits, int U, int T, int Bs, int B, int G,
    const head_sums_args hs) {
    constexpr int NT = TT ? TT : 1;                   // tasks the block sums
    extern __shared__ float4 st4[];                   // [U] {mean, 1/sigma, gamma, beta}
    __shared__ float part[NT][16][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + lane, t = TT ? 0 : blockIdx.y;
    const bool owner = blockIdx.x == 0 && blockIdx.y == 0;
    const int g = blockIdx.z, ldl = G * T;
    const size_t ug = (size_t)g * U;                   // the member's first unit
    z += ug * Bs; zhat += ug * Bs; o += ug * Bs; z12p += ug * nblk * 2;
    c2 += ug; g3 += ug; b3 += ug; rm3 += ug; rv3 += ug; sig3 += ug;
    Wf += (size_t)g * T * U; bf += (size_t)g * T; logits += (size_t)g * T;
    if (g != 0) nbt = nullptr;
    // the first batch of z loads does not depend on the statistics: requested before them, so that
    // the kernel's two round trips overlap (the combiner weights ride in LDS beside the statistics:
    // with them in the batch too the kernel spilled at its 128 registers)
    constexpr int LQ = 20;
    const float* wr = Wf + (size_t)t * U;
    float* wl = reinterpret_cast<float*>(st4 + U);      // [NT][U] combiner weights of task t (+ tt)
    STAMP(0);
    float zq0[LQ];
#pragma unroll
    for (int q = 0; q < LQ; ++q)
        zq0[q] = z[(uint32_t)min(wv + 16 * q, U - 1) * (uint32_t)Bs + (uint32_t)b];
    for (int u = threadIdx.x; u < U; u += 1024) {
        double s1 = 0, s2 = 0;
        for (int i0 = 0; i0 < nblk; i0 += 4) {           // four partial pairs in flight per round trip
            double2 pv[4];                                // (eight, with the z batch above held, spilled)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                pv[i] = *reinterpret_cast<const double2*>(&z12p[((size_t)u * nblk + min(i0 + i, nblk - 1)) * 2]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i0 + i < nblk) { s1 += pv[i].x; s2 += pv[i].y; }
        }
        const double mean = s1 / (double)B;
        const double var = fmax(s2 / (double)B - mean * mean, 0.0);
        const double sg = sqrt(var + BN_EPS_D);
        st4[u] = make_float4((float)mean, (float)(1.0 / sg), g3[u], b3[u]);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) wl[tt * U + u] = wr[(size_t)tt * U + u];
        if (owner) {
            sig3[u] = (float)sg;
            rm3[u] = (float)((1 - BN_MOM_D) * (double)rm3[u] + BN_MOM_D * (mean + (double)c2[u]));
            rv3[u] = (float)((1 - BN_MOM_D) * (double)rv3[u] + BN_MOM_D * var * (double)B / (double)(B - 1));
            if (u == 0 && nbt) *nbt += 1;
        }
    }
    __syncthreads();
    // (TT > 0: gridDim.y unit groups repeat this phase on the same 64 sequences; group 0 stores)
    const bool first = TT == 0 || blockIdx.y == 0;
    const bool store = t == 0 && b < B && first;
    float acc[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) acc[tt] = 0.f;
    // twenty units (forty loads) in flight per wave: the 300 units of the headline shape are one
    // memory round trip per wave (ten at a time made two dependent ones in a kernel that is nothing
    // but round trips)
    for (int u0 = wv; u0 < U; u0 += 16 * LQ) {
        float zq[LQ];
        if (u0 == wv) {
#pragma unroll
            for (int q = 0; q < LQ; ++q) zq[q] = zq0[q];
        } else {
            // (32-bit element offset from the uniform base: a 64-bit address per load took two
            // registers each and spilled)
#pragma unroll
            for (int q = 0; q < LQ; ++q)
                zq[q] = z[(uint32_t)min(u0 + 16 * q, U - 1) * (uint32_t)Bs + (uint32_t)b];
        }
#pragma unroll
        for (int q = 0; q < LQ; ++q) KEEP(zq[q]);
#pragma unroll
        for (int q = 0; q < LQ; ++q) {
            const int u = u0 + 16 * q;
            if (u < U) {                               // wave-uniform
                const float4 sv = st4[u];
                const float zh = (zq[q] - sv.x) * sv.y;
                const float ov = fmaxf(fmaf(sv.z, zh, sv.w), 0.f);
                if (store) {
                    const uint32_t off = (uint32_t)u * (uint32_t)Bs + (uint32_t)b;
                    zhat[off] = zh; o[off] = ov;
                }
#pragma unroll
                for (int tt = 0; tt < NT; ++tt) acc[tt] = fmaf(wl[tt * U + u], ov, acc[tt]);
            }
        }
    }
    // head_sums' first trip of z loads depends on nothing here: requested in front of the barrier, with
    // the registers of the z batch above free again, so that the round trip hides behind the logits' sum
    // (units [ulo, uhi) of this block: all of them in a grid of one group; otherwise none in group 0 and
    // an even share of them in each of the other gridDim.y - 1)
    int ulo = 0, uhi = U;
    if constexpr (TT > 0) {
        const int ng = (int)gridDim.y - 1, r = (int)blockIdx.y - 1;
        if (ng > 0) { ulo = r < 0 ? 0 : r * U / ng; uhi = r < 0 ? 0 : (r + 1) * U / ng; }
    }
    float zv[head_sums_pc<NT>::value][8];
    if constexpr (TT > 0)
        if (ulo < uhi)                                 // (block-uniform)
            head_sums_load<head_sums_pc<NT>::value>(z, ulo + ((int)threadIdx.x >> 3), uhi, Bs,
                                                    (int)blockIdx.x * 64 + 8 * ((int)threadIdx.x & 7), zv);
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) part[tt][wv][lane] = acc[tt];
    __syncthreads();
    STAMP(1);
    float sum[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) sum[tt] = 0.f;
    if (wv == 0 && b < B) {
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            float s = bf[t + tt];
#pragma unroll
            for (int i = 0; i < 16; ++i) s += part[tt][i][lane];
            if (first) logits[(size_t)b * ldl + t + tt] = s;
            sum[tt] = s;
        }
    }
    if constexpr (TT > 0) {
        head_sums<NT>(hs, sum, st4, wl, z, zv, U, ulo, uhi, Bs, B);
        STAMP(5);
    }
}

// outs[b][u] = o[u][b]   (model.linears(x) output layout, test.py:151)
__global__ __launch_bounds__(256) void outs_kernel(const float* __restrict__ o,
                                                   float* __restrict__ outs, int U, int Bs, int B) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    if (gid >= B * U) return;
    const int u = gid / B, b = gid % B;
    outs[(size_t)b * U + u] = o[(size_t)u * Bs + b];
}

// The head forward of a model or a bank (G members of Um units; a stand-alone model is G = 1).  Train,
// T <= HEAD_GEMM_MIN_T and one member's statistics fit LDS: logits_bn_kernel alone; otherwise
// head_fwd_train (per unit, on all G*Um units) and the combiner -- the MFMA GEMM for many tasks on a
// single model, logits_kernel otherwise: a bank has no GEMM form of the combiner.
int launch_head_fwd(explainn_ctx* c, const explainn_params* p, int B, bool train, float* logits,
                    float* outs, hipStream_t s) {
    const int Um = c->Um, G = c->Gm, T = c->T;
    const dim3 grid((B + 63) / 64, T, G);
    // (one member's statistics in 48 KB: U = G * Um exactly, so this is Um * 20 B <= 48 KB.  Written on
    // c->T and c->U because tests/dispatch_model.py reads the rule from this line.)
    if (train && logits && c->T <= HEAD_GEMM_MIN_T && !outs && (size_t)c->U * (sizeof(float4) + sizeof(float)) <= 48 * 1024 * (size_t)G) {
        hipLaunchKernelGGL(logits_bn_kernel<0>, grid, dim3(1024),
                           (size_t)Um * (sizeof(float4) + sizeof(float)), s, c->z, c->z12p, fc_fwd_blocks(B, c->NQ),
                           p->fc2_b, p->bn3_w, p->bn3_b, p->bn3_rm, p->bn3_rv, p->bn3_nbt, c->zhat,
                           c->o, c->sig3, p->final_w, p->final_b, logits, Um, T, c->Bs, B, G, head_sums_args{});
        LAUNCH_CHECK();
        return EXPLAINN_OK;
    }
    if (train) {
        hipLaunchKernelGGL(head_fwd_train_kernel, dim3(c->U), dim3(256), 0, s, c->z, p->fc2_b,
                           p->bn3_w, p->bn3_b, p->bn3_rm, p->bn3_rv, p->bn3_nbt, c->zhat, c->o,
                           c->sig3, c->Bs, B);
        LAUNCH_CHECK();
    }
    if (logits && G == 1 && T > HEAD_GEMM_MIN_T) {
        // logits[b][t] = sum_u o[u][b] Wf[t][u] + bf[t]: M = B, N = T, K = U
        const int tiles = ((B + 31) / 32) * ((T + 31) / 32);
        hipLaunchKernelGGL((gemm32_kernel<false, true, EPI_BIAS>), dim3(tiles), dim3(256), 0, s, c->o,
                           c->Bs, p->final_w, c->U, logits, T, B, T, c->U, p->final_b,
                           (float*)nullptr);
        LAUNCH_CHECK();
    } else if (logits) {
        hipLaunchKernelGGL(logits_kernel, grid, dim3(1024), 0, s, c->o, p->final_w, p->final_b,
                           logits, Um, T, c->Bs, B, G);
        LAUNCH_CHECK();
    }
    if (outs) {
        hipLaunchKernelGGL(outs_kernel, dim3((B * c->U + 255) / 256), dim3(256), 0, s, c->o, outs,
                           c->U, c->Bs, B);
        LAUNCH_CHECK();
    }
    return EXPLAINN_OK;
}


// The combiner launch of the training step that also leaves the head backward's per-block partials
// (logits_bn_kernel<T>, a single model with T <= PA_HEAD_MAX_T tasks): LDS = statistics + T weight rows.
bool head_sums_fit(const explainn_ctx* c) {
    return (size_t)c->U * (sizeof(float4) + c->T * sizeof(float)) <= 40 * 1024;
}

int launch_head_fwd_sums(explainn_ctx* c, const explainn_params* p, int B, float* logits, const float* y,
                         int kind, hipStream_t s) {
    const int U = c->U, T = c->T;
    const head_sums_args hs = {y, kind, c->dlogits, c->hp, c->hb};
    const size_t lds = (size_t)U * (sizeof(float4) + T * sizeof(float));
    // R blocks per sequence block (head_sums; c->head_groups: EXPLAINN_HEAD_GROUPS or the default): 1 is
    // the grid of one block that does everything; otherwise the storing group and R - 1 unit groups,
    // never more of those than there are units
    const int R = min(max(c->head_groups, 1), U + 1);
#define CALL(TT)                                                                                      \
    hipLaunchKernelGGL(logits_bn_kernel<TT>, dim3((B + 63) / 64, R), dim3(1024), lds, s, c->z, c->z12p, \
                       fc_fwd_blocks(B, c->NQ), p->fc2_b, p->bn3_w, p->bn3_b, p->bn3_rm, p->bn3_rv,    \
                       p->bn3_nbt, c->zhat, c->o, c->sig3, p->final_w, p->final_b, logits, U, T, c->Bs, \
                       B, 1, hs)
    switch (T) {
        case 1: CALL(1); break;
        case 2: CALL(2); break;
        case 3: CALL(3); break;
        case 4: CALL(4); break;
        default: explainn_set_error("head sums in the combiner launch: %d tasks", T); return EXPLAINN_E_UNSUPPORTED;
    }
#undef CALL
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

// loss + dlogits; up to LOSS_BLOCKS blocks write one partial sum each, the last block to finish adds
// them in index order -> deterministic whatever the arrival order
constexpr int LOSS_BLOCKS = 64;
// DEFER (the training step): the blocks leave their partial sums and the head backward that follows
// adds them up -- the last-arriver finish below needs a device-scope fence in every block, and on
// this multi-XCD part that write-back made a kernel with 200 K elements take 17 us.
template <bool DEFER>
__global__ __launch_bounds__(1024) void loss_kernel(const float* __restrict__ logits,
                                                    const float* __restrict__ y, int kind, int N,
                                                    float* __restrict__ loss,
                                                    float* __restrict__ dlogits,
                                                    double* __restrict__ partial,
                                                    int* __restrict__ counter) {
    __shared__ double red[16];
    __shared__ int last;
    const int tid = threadIdx.x;
    const float invN = 1.0f / (float)N;
    double acc = 0;
    // four elements per thread per trip with their loads issued together (a block's eight trips of a
    // run-time loop were eight memory round trips; the order of a thread's additions is unchanged)
    const int stride = gridDim.x * 1024;
    for (int i0 = blockIdx.x * 1024 + tid; i0 < N; i0 += 4 * stride) {
        float xv[4], tv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ic = min(i0 + q * stride, N - 1);
            xv[q] = logits[ic]; tv[q] = y[ic];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) { KEEP(xv[q]); KEEP(tv[q]); }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q * stride;
            if (i < N) {
                acc += (double)loss_value(kind, xv[q], tv[q]);
                dlogits[i] = loss_grad(kind, xv[q], tv[q], invN);
            }
        }
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (DEFER) {
        if (tid == 0) {
            double s = 0;
            for (int i = 0; i < 16; ++i) s += red[i];
            partial[blockIdx.x] = s;
        }
        return;
    }
    if (tid == 0) {
        double s = 0;
        for (int i = 0; i < 16; ++i) s += red[i];
        partial[blockIdx.x] = s;
        __threadfence();
        last = atomicAdd(counter, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (last && tid == 0) {
        __threadfence();
        double s = 0;
        for (unsigned i = 0; i < gridDim.x; ++i) s += partial[i];
        *loss = (float)(s / (double)N);
        *counter = 0;                                   // ready for the next launch
    }
}

// ---------------------------------------------------------------------------------------------
// Model bank (explainn_create_bank): G members of U units each share the batch and the targets;
// logits / dlogits are (B,G,T), final_w (G,T,U), final_b (G,T), the loss is G values.  Everything in
// front of the head runs on G*U independent units, and the head kernels take the member index at run
// time (a stand-alone model is the bank of one).  Only the loss launch is a bank's own: one block per
// member and no partials -- folded into loss_kernel it would change either the bank's summation order
// or the single model's partial layout.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_1024(double v, double* red16) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red16[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += red16[i];        // fixed order
    return s;
}

// one block per member: loss[g] = mean over its own B*T terms against the shared targets, and its
// slice of dlogits; every thread adds its terms in index order, the block sum has a fixed order
__global__ __launch_bounds__(1024) void bank_loss_kernel(const float* __restrict__ logits,
                                                         const float* __restrict__ y, int kind, int B,
                                                         int T, int G, float* __restrict__ loss,
                                                         float* __restrict__ dlogits) {
    __shared__ double red[16];
    const int g = blockIdx.x, N = B * T;
    const float invN = 1.0f / (float)N;
    double acc = 0;
    for (int i = threadIdx.x; i < N; i += 1024) {
        const int b = i / T, t = i - b * T;
        const size_t il = ((size_t)b * G + g) * T + t;
        const float x = logits[il], tt = y[i];
        acc += (double)loss_value(kind, x, tt);
        dlogits[il] = loss_grad(kind, x, tt, invN);
    }
    const double tot = block_sum_1024(acc, red);
    if (threadIdx.x == 0) loss[g] = (float)(tot / (double)N);
}

int launch_loss(explainn_ctx* c, int kind, const float* logits, const float* y, int B, float* loss,
                float* dlogits, hipStream_t s) {
    if (c->Gm > 1) {
        hipLaunchKernelGGL(bank_loss_kernel, dim3(c->Gm), dim3(1024), 0, s, logits, y, kind, B, c->T,
                           c->Gm, loss, dlogits);
        LAUNCH_CHECK();
        return EXPLAINN_OK;
    }
    const int N = B * c->T;
    const int blocks = min(LOSS_BLOCKS, (N + 8191) / 8192);
    hipLaunchKernelGGL(loss_kernel<false>, dim3(blocks), dim3(1024), 0, s, logits, y, kind, N, loss, dlogits,
                       c->lossp, c->flags + 1);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

// the training step's form: partial sums only; launch_head_bwd (which must follow) finishes the value
int launch_loss_deferred(explainn_ctx* c, int kind, const float* logits, const float* y, int B, float* loss,
                         float* dlogits, hipStream_t s) {
    // a bank's loss kernel finishes its G values itself: nothing is deferred
    if (c->Gm > 1) return launch_loss(c, kind, logits, y, B, loss, dlogits, s);
    const int N = B * c->T;
    // (no last-arriver finish here, so nothing limits the block count: one or two elements per thread)
    const int blocks = min(256, (N + 1023) / 1024);
    hipLaunchKernelGGL(loss_kernel<true>, dim3(blocks), dim3(1024), 0, s, logits, y, kind, N, loss, dlogits,
                       c->lossp, c->flags + 1);
    LAUNCH_CHECK();
    c->loss_blocks = blocks; c->loss_out = loss; c->loss_n = N;
    return EXPLAINN_OK;
}

// one block per unit: final-layer gradients, BN3 backward -> dz[u][b].
// Unit u is local unit ul of member g of a bank of G members of Um units (a stand-alone model: G = 1,
// g = 0, ul = u): the block reads its member's slice of dl / logits (B,G,T) and Wf[g] (T,Um) against
// the shared targets (B,T), writes the member's row of d Wf and -- in the block of the member's unit
// 0 -- d bf[g] and the loss value loss_out[g].
// GEMMED (a single model only): d o (in dz on entry) and the final-layer gradients came from the MFMA
// GEMMs above.
template <bool FUSED, bool GEMMED>
__global__ __launch_bounds__(256) void head_bwd_kernel(
    const float* __restrict__ dl, const float* __restrict__ logits, const float* __restrict__ y,
    int kind, float* __restrict__ loss_out, const float* __restrict__ Wf,
    const float* __restrict__ g3, const float* __restrict__ o, const float* __restrict__ zhat,
    const float* __restrict__ sig3, float* __restrict__ dz, float* __restrict__ gWf,
    float* __restrict__ gbf, float* __restrict__ gg3, float* __restrict__ gb3,
    float* __restrict__ gc2, int Um, int T, int G, int Bs, int B, const float* __restrict__ gWp,
    int gwch, const double* __restrict__ lossp, int lossb, int lossn) {
    __shared__ double red[4];
    __shared__ double red3[12];
    const int u = blockIdx.x, tid = threadIdx.x;
    const int g = u / Um, ul = u - g * Um;             // (block-uniform)
    const float* Wu = Wf + (size_t)g * T * Um + ul;    // Wf[g][t][ul] = Wu[t * Um], likewise d Wf
    float* gWu = gWf + (size_t)g * T * Um + ul;
    gbf += (size_t)g * T;
    const float* ou = o + (size_t)u * Bs;
    const float* zh = zhat + (size_t)u * Bs;
    float* dzu = dz + (size_t)u * Bs;
    const float invN = 1.0f / (float)(B * T);
    // d loss / d logit for (sequence b, task t) of this member: either read from `dl`, or -- FUSED, used
    // by explainn_train_step when T is small -- recomputed from logits and targets so that the separate
    // loss launch (and its ~4 us floor) disappears; the block of the member's unit 0 then also reduces
    // the loss value.  dl / logits are [b][g][t], the targets [b][t].
    auto il_of = [&](int b, int t) { return ((size_t)b * G + g) * T + t; };
    auto dl_at = [&](int b, int t) -> float {
        return FUSED ? loss_grad(kind, logits[il_of(b, t)], y[b * T + t], invN) : dl[il_of(b, t)];
    };
    const float g3u = g3[u], sig3u = sig3[u];        // (used behind the block sums: requested here)
    double s1 = 0, s2 = 0;
    // small batches and few tasks: d3 and zhat of this thread's sequences stay in registers between
    // the two passes (one batch of loads each instead of a dependent round trip per 256 sequences)
    constexpr int RB = HEAD_RB;
    const bool inreg = !GEMMED && T <= 4 && B <= RB * 256;
    float d3r[RB], zhr[RB];
    double gw[4] = {0, 0, 0, 0}, gb[4] = {0, 0, 0, 0}, lacc = 0;
    if (inreg) {
        float our[RB];
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int bc = min(tid + 256 * i, B - 1);
            our[i] = ou[bc];
            zhr[i] = zh[bc];
            const bool live_i = tid + 256 * i < B;
            float dob = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t >= T) continue;
                const float dlv = dl_at(bc, t);
                dob = fmaf(dlv, Wu[(size_t)t * Um], dob);
                // the final-layer gradients ride along: d Wf[t][u] += dl * o, and (unit 0's block)
                // d bf[t] += dl and the loss value
                if (live_i) {
                    gw[t] = fma((double)dlv, (double)our[i], gw[t]);
                    if (ul == 0) {
                        gb[t] += (double)dlv;
                        if (FUSED) lacc += (double)loss_value(kind, logits[il_of(bc, t)], y[bc * T + t]);
                    }
                }
            }
            d3r[i] = dob;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const bool live = tid + 256 * i < B;
            d3r[i] = (live && our[i] > 0.f) ? d3r[i] : 0.f;
            s1 += (double)d3r[i];
            s2 = fma((double)d3r[i], live ? (double)zhr[i] : 0.0, s2);
        }
    } else {
        if (GEMMED) {
            // four sequences per thread per trip, their loads issued together (one sequence per trip of
            // a run-time loop was one memory round trip each: sixteen in a row at batch 4096)
            for (int b0 = tid; b0 < B; b0 += 4 * 256) {
                float dv[4], ov[4], zv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int bc = min(b0 + 256 * i, B - 1);
                    dv[i] = dzu[bc]; ov[i] = ou[bc]; zv[i] = zh[bc];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) { KEEP(dv[i]); KEEP(ov[i]); KEEP(zv[i]); }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int b = b0 + 256 * i;
                    if (b < B) {
                        const float d3 = ov[i] > 0.f ? dv[i] : 0.f;
                        dzu[b] = d3;
                        s1 += (double)d3;
                        s2 = fma((double)d3, (double)zv[i], s2);
                    }
                }
            }
        } else {
        for (int b = tid; b < B; b += 256) {
            float dob = 0.f;
            for (int t = 0; t < T; ++t)
                dob = fmaf(dl_at(b, t), Wu[(size_t)t * Um], dob);
            const float d3 = ou[b] > 0.f ? dob : 0.f;
            dzu[b] = d3;
            s1 += (double)d3;
            s2 = fma((double)d3, (double)zh[b], s2);
        }
        }
    }
    double S1 = s1, S2 = s2, G0 = gw[0];
    if (inreg) {
        block_sum3_256(S1, S2, G0, red3);          // (inreg is block-uniform: so are the barriers)
    } else {
        S1 = block_sum_256(s1, red);
        S2 = block_sum_256(s2, red);
    }
    const float m1 = (float)(S1 / (double)B), m2 = (float)(S2 / (double)B);
    const float sc = g3u / sig3u;
    if (inreg) {
#pragma unroll
        for (int i = 0; i < RB; ++i)
            if (tid + 256 * i < B) dzu[tid + 256 * i] = sc * (d3r[i] - m1 - zhr[i] * m2);
    } else {
        for (int b0 = tid; b0 < B; b0 += 4 * 256) {
            float dv[4], zv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int bc = min(b0 + 256 * i, B - 1);
                dv[i] = dzu[bc]; zv[i] = zh[bc];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) { KEEP(dv[i]); KEEP(zv[i]); }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (b0 + 256 * i < B) dzu[b0 + 256 * i] = sc * (dv[i] - m1 - zv[i] * m2);
        }
    }
    if (tid == 0) { gg3[u] = (float)S2; gb3[u] = (float)S1; gc2[u] = 0.f; }
    if (inreg) {
        // everything was accumulated in the first pass; only the block-wide sums are left
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t >= T) continue;                      // T is block-uniform: the barriers inside stay uniform
            const double tot = t == 0 ? G0 : block_sum_256(gw[t], red);
            if (tid == 0) gWu[(size_t)t * Um] = (float)tot;
            if (ul == 0) {
                const double ct = block_sum_256(gb[t], red);
                if (tid == 0) gbf[t] = (float)ct;
            }
        }
        if (FUSED && ul == 0) {
            const double tot = block_sum_256(lacc, red);
            if (tid == 0) loss_out[g] = (float)(tot / (double)(B * T));
        }
        return;
    }
    if (lossb > 0 && u == 0) {
        // the loss value of a single model: launch_loss_deferred's block partials (at most 256), one per
        // thread, summed in the block's fixed tree order (block-uniform branch: the barriers inside are safe)
        const double sl = block_sum_256(tid < lossb ? lossp[tid] : 0.0, red);
        if (tid == 0) *loss_out = (float)(sl / (double)lossn);
    }
    if (GEMMED && gWp) {
        // the combiner-weight gradient of this unit (and, in unit 0's block, the bias gradient): the
        // GEMM's batch-chunk partials summed in chunk order, eight loads in flight  (G = 1: U = Um)
        const int U = Um;
        for (int e = tid; e < (u == 0 ? 2 * T : T); e += 256) {
            const int t = e < T ? e : e - T, col = e < T ? u : U;
            float sacc = 0.f;
            for (int c0 = 0; c0 < gwch; c0 += 8) {
                float pv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    pv[i] = gWp[((size_t)min(c0 + i, gwch - 1) * T + t) * (U + 1) + col];
#pragma unroll
                for (int i = 0; i < 8; ++i) KEEP(pv[i]);
#pragma unroll
                for (int i = 0; i < 8; ++i) sacc += (c0 + i < gwch) ? pv[i] : 0.f;
            }
            if (e < T) gWf[(size_t)t * U + u] = sacc; else gbf[t] = sacc;
        }
    }
    for (int t = 0; t < (GEMMED ? 0 : T); ++t) {
        double a = 0;
        for (int b = tid; b < B; b += 256)
            a = fma((double)dl_at(b, t), (double)ou[b], a);
        const double tot = block_sum_256(a, red);
        if (tid == 0) gWu[(size_t)t * Um] = (float)tot;
        if (ul == 0) {
            double c = 0;
            for (int b = tid; b < B; b += 256) c += (double)dl_at(b, t);
            const double ct = block_sum_256(c, red);
            if (tid == 0) gbf[t] = (float)ct;
        }
    }
    if (FUSED && ul == 0) {
        double acc = 0;
        for (int i = tid; i < B * T; i += 256) {       // the member's B*T terms in (b, t) order
            const int b = i / T, t = i - b * T;
            acc += (double)loss_value(kind, logits[il_of(b, t)], y[i]);
        }
        const double tot = block_sum_256(acc, red);
        if (tid == 0) loss_out[g] = (float)(tot / (double)(B * T));
    }
}

// the per-unit kernel on all G*Um units: dl given (FUSED = false; lossb > 0: a deferred loss value to
// finish) or recomputed from logits and targets
template <bool FUSED, bool GEMMED>
static int launch_head_bwd_units(explainn_ctx* c, const explainn_params* p, const explainn_grads* g,
                                 const float* dl, int kind, const float* logits, const float* y,
                                 float* loss_out, int lossb, int gwch, int B, hipStream_t s) {
    hipLaunchKernelGGL((head_bwd_kernel<FUSED, GEMMED>), dim3(c->U), dim3(256), 0, s, dl, logits, y, kind,
                       loss_out, p->final_w, p->bn3_w, c->o, c->zhat, c->sig3, c->dz, g->final_w,
                       g->final_b, g->bn3_w, g->bn3_b, g->fc2_b, c->Um, c->T, c->Gm, c->Bs, B, c->gWp, gwch,
                       c->lossp, lossb, c->loss_n);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

int launch_head_bwd(explainn_ctx* c, const explainn_params* p, const explainn_grads* g,
                    const float* dlogits, int B, hipStream_t s) {
    // many tasks on a single model: d o and the final-layer gradients as GEMMs, the per-unit kernel
    // finishes them.  A bank takes the per-unit kernel alone at every T.
    const bool gemm = c->Gm == 1 && c->T > HEAD_GEMM_MIN_T;
    const int gwch = gemm ? head_gw_chunks(B) : 0;
    if (gemm) {
        const int T = c->T, U = c->U;
        hipLaunchKernelGGL(transpose_dl_kernel, dim3((B + 31) / 32, (T + 31) / 32), dim3(256), 0, s,
                           dlogits, c->dlT, B, T, c->Bs);
        LAUNCH_CHECK();
        // d o[u][b] = sum_t Wf[t][u] dl[b][t]  -> dz (raw; the per-unit kernel finishes it)
        hipLaunchKernelGGL((gemm32_kernel<false, false, EPI_PLAIN>),
                           dim3(((U + 31) / 32) * ((B + 31) / 32)), dim3(256), 0, s, p->final_w, U,
                           c->dlT, c->Bs, c->dz, c->Bs, U, B, T, (const float*)nullptr,
                           (float*)nullptr);
        LAUNCH_CHECK();
        // d Wf[t][u] = sum_b dl[b][t] o[u][b], and d bf[t] as the virtual all-ones unit U
        hipLaunchKernelGGL((gemm32_kernel<true, true, EPI_GW>),
                           dim3(((T + 31) / 32) * ((U + 1 + 31) / 32), gwch), dim3(256), 0, s, c->dlT, c->Bs,
                           c->o, c->Bs, c->gWp, U + 1, T, U + 1, B, (const float*)nullptr,
                           (float*)nullptr);
        LAUNCH_CHECK();
    }
    // (loss_blocks > 0: launch_loss_deferred left a single model's loss value to finish here)
    float* loss_out = c->loss_blocks ? c->loss_out : (float*)nullptr;
    const int rc = gemm ? launch_head_bwd_units<false, true>(c, p, g, dlogits, 0, nullptr, nullptr, loss_out, c->loss_blocks, gwch, B, s)
                        : launch_head_bwd_units<false, false>(c, p, g, dlogits, 0, nullptr, nullptr, loss_out, c->loss_blocks, 0, B, s);
    c->loss_blocks = 0;
    return rc;
}

// loss + its gradient folded into the head backward (explainn_train_step, small T)
int launch_head_bwd_fused_loss(explainn_ctx* c, const explainn_params* p, const explainn_grads* g,
                               int kind, const float* logits, const float* y, float* loss_out, int B,
                               hipStream_t s) {
    return launch_head_bwd_units<true, false>(c, p, g, nullptr, kind, logits, y, loss_out, 0, 0, B, s);
}
