// Integrated Gradients along the straight path x_a = x' + a (x - x') in eval mode (DESIGN.md section 3,
// item 12).  The convolution is linear in x, so the raw conv sums along the path are an exact
// interpolation of the sums at the two ends,
//   g_a[b,u,j] = g'[b,u,j] + a (g[b,u,j] - g'[b,u,j]),
// and both ends are rebuilt from base codes (x: the staged codes; x': a code row per sequence, with
// code 4 = an all-zero column -- N, and the whole `zero` baseline -- and code 5 = 0.25 in all four
// rows, the `uniform` baseline).  Only what sits behind the convolution is evaluated per node
// a_s = (s + 1/2)/S: BatchNorm1 (affine), exp, MaxPool(7,7) of the interpolated sums, the per-unit FC
// and the head's weight.  With D_a = dF/dg_a (non-zero at each pooled window's argmax only, first
// index on a tie, sign-aware for a negative BatchNorm1 scale) and F = sum_t dl[b,t] logit_t,
//   G[b,u,j]  = (1/S) sum_s D_(a_s)[b,u,j]                                       (s ascending)
//   IG[b,a,p] = (x - x')[b,a,p] sum_u sum_(t: 0 <= p-t < 7n) W[u,a,t] G[b,u,p-t]  (u, t ascending)
// The unit itself (window sums, FC1, FC2, BatchNorm3, the LDS tables, the baseline codes) is
// unit_eval.h's.  pg_path: workgroup = (256 sequences, unit), lane = sequence; the unit's A2 (as
// [w][100]) and fc2 row sit in LDS and are read at wave-uniform addresses.  A lane first writes g and
// g' of its sequence (taps ascending, the same code for both ends) into its own columns of the workspace and
// zeroes its column of G, then walks the two ends (forward only: the unit outputs behind the endpoint
// logits) and the S nodes (forward, backward to the pooled values, G += alpha dy / S at the argmax:
// lane-exclusive addresses, plain read-modify-write).  pg_gather: the transposed convolution, one
// owner per output element.  pg_logits: the two ends' logits, units in order.  No float atomics.
#include "common.h"
#include "unit_eval.h"

#define PG_WAVES 4
#define PG_POS 8                   // positions per pg_gather wave
#define PG_UT 64                   // units whose filters one LDS pass of pg_gather stages
#define PG_WS_CAP (1LL << 30)      // workspace bytes the sub-batch size aims at

// ---- workspace of a sub-batch of S sequences (S a multiple of 64), J = 7n covered conv positions:
//   G, GX, GB  [U][J][S] fp32      the path-averaged gradient, g of x, g of x'
//   O          [2][U][S] fp32      the unit outputs at a = 1 and a = 0
//   BT         [L][S]    uint8     the baseline's codes, position-major
static int64_t pg_per_sequence_bytes(const explainn_ctx* c) {
    const int64_t J = (int64_t)POOLW * c->n;
    return ((int64_t)c->U * (3 * J + 2)) * (int64_t)sizeof(float) + c->L;
}

int pathgrad_sub_batch(const explainn_ctx* c, int B) {
    return sub_batch_of(PG_WS_CAP, pg_per_sequence_bytes(c), B);
}

int64_t pathgrad_workspace_bytes(const explainn_ctx* c, int B) {
    return pg_per_sequence_bytes(c) * (int64_t)pathgrad_sub_batch(c, B);
}

// the baseline of the sub-batch [b0, b0 + Bsub) as codes, position-major; rc: the reverse complement
// of the given rows (the strand the staged batch runs on)
__global__ __launch_bounds__(256) void pg_base_kernel(const uint8_t* __restrict__ codes, int kind, int rc,
                                                      uint8_t* __restrict__ BT, int L, int b0, int Bsub,
                                                      int S) {
    const int bi = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (bi >= S) return;
    uint8_t v = kind == EXPLAINN_IG_BASELINE_UNIFORM ? PG_CODE_UNIFORM : PG_CODE_ZERO;
    if (kind == EXPLAINN_IG_BASELINE_CODES && bi < Bsub) {
        const uint8_t s = codes[(size_t)(b0 + bi) * L + (rc ? L - 1 - p : p)];
        v = s < 4 ? (uint8_t)(rc ? 3 - s : s) : (uint8_t)PG_CODE_ZERO;
    }
    BT[(size_t)p * S + bi] = v;
}

// Window w's conv sums of both ends, from the lane's columns.
__device__ __forceinline__ void pg_load(const float* __restrict__ gx, const float* __restrict__ gb, size_t rs,
                                        float* vx, float* vb) {
#pragma unroll
    for (int e = 0; e < POOLW; ++e) { vx[e] = gx[e * rs]; vb[e] = gb[e * rs]; }
}

// The pooled extreme of a window at path position a and its offset: first index on an exact tie,
// the minimum where BatchNorm1's scale is negative (a compare, for the index; ism.hip's ism_ext folds
// with fmaxf).  mode 0: the node a; 1: the end x; 2: the end x'.
__device__ __forceinline__ float pg_pool(const float* vx, const float* vb, float a, int mode, float sg,
                                         int& idx) {
    float m = 0.f;
    idx = 0;
#pragma unroll
    for (int e = 0; e < POOLW; ++e) {
        const float v = mode == 0 ? fmaf(a, vx[e] - vb[e], vb[e]) : (mode == 1 ? vx[e] : vb[e]);
        const float t = sg * v;
        if (e == 0) m = t;
        else if (t > m) { m = t; idx = e; }
    }
    return sg * m;
}

__global__ __launch_bounds__(64 * PG_WAVES) void pg_path_kernel(
    const uint8_t* __restrict__ codesT, const uint8_t* __restrict__ BT, const float* __restrict__ conv_w,
    const float* __restrict__ alpha, const float* __restrict__ shift, const float* __restrict__ A2,
    const float* __restrict__ sh2, const float* __restrict__ fc2_w, const float* __restrict__ fc2_b,
    const float* __restrict__ g3, const float* __restrict__ b3, const float* __restrict__ rm3,
    const float* __restrict__ rv3, const float* __restrict__ dl, const float* __restrict__ final_w,
    float* __restrict__ G, float* __restrict__ GX, float* __restrict__ GB, float* __restrict__ O, int U,
    int T, int k, int n, int NS, int Bs, int b0, int Bsub, int S, int steps) {
    extern __shared__ __attribute__((aligned(16))) float pg_sm[];     // A2T [n][FC_H]
    __shared__ __attribute__((aligned(16))) float Wl[MAX_K * 8];      // [t][code]: 4 = N, 5 = uniform
    __shared__ __attribute__((aligned(16))) float fcs[FC_H];
    int u, chunk;
    if (!unit_chunk_of_block(U, u, chunk)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unit_stage<true>(A2, conv_w, fc2_w, u, k, n, NS, tid, 64 * PG_WAVES, pg_sm, Wl, fcs);
    __syncthreads();
    const int bw = chunk * 64 * PG_WAVES + wave * 64;
    if (bw >= Bsub) return;                        // wave-uniform; no barrier below
    const int bi = bw + lane;
    const bool live = bi < Bsub;
    const int bic = min(bi, Bsub - 1);             // a dead lane repeats the last sequence and stores nothing
    const float* A2T = pg_sm;
    const unit_consts uc = unit_load(alpha, shift, fc2_b, g3, b3, rm3, rv3, u);
    const int J = POOLW * n;
    const size_t rs = (size_t)S;
    const size_t ub = (size_t)u * J * rs + bic;
    float* __restrict__ Gu = G + ub;
    float* __restrict__ gxu = GX + ub;
    float* __restrict__ gbu = GB + ub;

    // ---- both ends' conv sums into the lane's own columns; its column of G starts at zero ----
    {
        const uint8_t* __restrict__ cx = codesT + b0 + bic;
        const uint8_t* __restrict__ cb = BT + bic;
        for (int w = 0; w < n; ++w) {
            float g[POOLW], h[POOLW];
            unit_window([&](int q) -> int { return cx[(size_t)q * Bs]; }, Wl, w, k, g);
            unit_window([&](int q) -> int { return cb[(size_t)q * rs]; }, Wl, w, k, h);
            if (live) {
#pragma unroll
                for (int e = 0; e < POOLW; ++e) {
                    const size_t o = (size_t)(POOLW * w + e) * rs;
                    gxu[o] = g[e]; gbu[o] = h[e]; Gu[o] = 0.f;
                }
            }
        }
    }
    const float dout = unit_dout(dl, final_w, b0 + bic, T, U, u);     // dF / d(unit output)
    const float invS = 1.f / (float)steps;

    // ---- the two ends (s = -2: x, s = -1: x'), then the nodes ----
    for (int s = -2; s < steps; ++s) {
        const int mode = s == -2 ? 1 : (s == -1 ? 2 : 0);
        const float a = ((float)s + 0.5f) * invS;
        const int fo = unit_opaque_zero();         // on the LDS reads of this node (unit_eval.h)
        float y2[FC_H];
#pragma unroll
        for (int r = 0; r < FC_H; ++r) y2[r] = sh2[(size_t)u * FC_H + r];
        // a window's sums are loaded one window ahead of their use
        float vx[POOLW], vb[POOLW], nx[POOLW], nb[POOLW];
        pg_load(gxu, gbu, rs, vx, vb);
        for (int w = 0; w < n; ++w) {
            const size_t on = (size_t)(POOLW * min(w + 1, n - 1)) * rs;
            pg_load(gxu + on, gbu + on, rs, nx, nb);
            int idx;
            const float q = qval(uc.al, pg_pool(vx, vb, a, mode, uc.sg, idx), uc.sh);
            UNIT_FC1_ADD(y2, reinterpret_cast<const float4*>(A2T + fo + w * FC_H), q);
#pragma unroll
            for (int e = 0; e < POOLW; ++e) { vx[e] = nx[e]; vb[e] = nb[e]; }
        }
        float z;
        UNIT_FC2(z, y2, fcs + fo);
        const float y3 = unit_bn3(uc, z);
        if (mode != 0) {
            if (live) O[((size_t)(mode - 1) * U + u) * rs + bi] = fmaxf(y3, 0.f);
            continue;
        }
        const float dz = y3 > 0.f ? dout * uc.inv3 : 0.f;
        if (!__any(live && dz != 0.f)) continue;   // wave-uniform: every lane's unit is closed here
        // e[r] = dF/dy2[r], in y2's registers
#pragma unroll
        for (int r4 = 0; r4 < FC_H / 4; ++r4) {
            const float4 f = *reinterpret_cast<const float4*>(fcs + fo + 4 * r4);
            y2[4 * r4] = y2[4 * r4] > 0.f ? dz * f.x : 0.f; y2[4 * r4 + 1] = y2[4 * r4 + 1] > 0.f ? dz * f.y : 0.f;
            y2[4 * r4 + 2] = y2[4 * r4 + 2] > 0.f ? dz * f.z : 0.f; y2[4 * r4 + 3] = y2[4 * r4 + 3] > 0.f ? dz * f.w : 0.f;
        }
        pg_load(gxu, gbu, rs, vx, vb);
        for (int w = 0; w < n; ++w) {
            const size_t on = (size_t)(POOLW * min(w + 1, n - 1)) * rs;
            pg_load(gxu + on, gbu + on, rs, nx, nb);
            const float4* __restrict__ a4 = reinterpret_cast<const float4*>(A2T + fo + w * FC_H);
            float dq = 0.f;
#pragma unroll
            for (int r4 = 0; r4 < FC_H / 4; ++r4) {
                const float4 av = a4[r4];
                dq = fmaf(av.x, y2[4 * r4], dq); dq = fmaf(av.y, y2[4 * r4 + 1], dq);
                dq = fmaf(av.z, y2[4 * r4 + 2], dq); dq = fmaf(av.w, y2[4 * r4 + 3], dq);
            }
            int idx;
            const float q = qval(uc.al, pg_pool(vx, vb, a, 0, uc.sg, idx), uc.sh);
            // dF/dg at the argmax = alpha q dq (BatchNorm1 scale, exp', FC1), averaged over the nodes
            if (live) {
                float* gp = Gu + (size_t)(POOLW * w + idx) * rs;
                *gp = fmaf(uc.al * (dq * q), invS, *gp);
            }
#pragma unroll
            for (int e = 0; e < POOLW; ++e) { vx[e] = nx[e]; vb[e] = nb[e]; }
        }
    }
}

// logits of the two ends: out[end][b][t] = final_b[t] + sum_u final_w[t,u] O[end][u][b], units in order
__global__ __launch_bounds__(256) void pg_logits_kernel(const float* __restrict__ O,
                                                        const float* __restrict__ final_w,
                                                        const float* __restrict__ final_b,
                                                        float* __restrict__ lx, float* __restrict__ lb, int U,
                                                        int T, int b0, int Bsub, int S) {
    const int bi = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y, end = blockIdx.z;
    if (bi >= Bsub) return;
    const float* __restrict__ o = O + (size_t)end * U * S + bi;
    float acc = 0.f;
    for (int u = 0; u < U; ++u) acc = fmaf(final_w[(size_t)t * U + u], o[(size_t)u * S], acc);
    (end == 0 ? lx : lb)[(size_t)(b0 + bi) * T + t] = acc + final_b[t];
}

// IG of the sub-batch: workgroup = (64 sequences, 4 tiles of PG_POS positions), wave = tile, lane =
// sequence.  Per LDS pass PG_UT units' filters (float4 over the bases) are staged; a wave takes the
// units in order and, per unit, the rows G[u][j] that reach its tile from the highest j down (taps
// ascending for every position), eight rows per load batch.  Row j = P0 + 7 - 8c - r meets position
// P0 + i at tap t = 8c + r + i - 7.
__global__ __launch_bounds__(256) void pg_gather_kernel(
    const float* __restrict__ G, const float* __restrict__ W, const uint8_t* __restrict__ codesT,
    const uint8_t* __restrict__ BT, float* __restrict__ ig, int U, int k, int L, int n, int Bs, int b0,
    int Bsub, int S) {
    __shared__ float4 Ws[PG_UT * MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int bi = blockIdx.x * 64 + lane, P0 = (blockIdx.y * 4 + wave) * PG_POS;
    const bool live = bi < Bsub;
    const int bic = min(bi, Bsub - 1);
    const int J = POOLW * n;
    const int nch = (k + 14) / 8;                               // row batches: t runs to k - 1
    float4 acc[PG_POS];
#pragma unroll
    for (int i = 0; i < PG_POS; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int u0 = 0; u0 < U; u0 += PG_UT) {
        __syncthreads();
        stage_filters4<false, PG_UT>(W, nullptr, u0, U, k, tid, 256, Ws);
        __syncthreads();
        if (P0 >= L) continue;                                   // wave-uniform; the barriers are above
        const int ue = min(u0 + PG_UT, U);
        for (int u = u0; u < ue; ++u) {
            const float4* __restrict__ wu = Ws + (u - u0) * MAX_K;
            const float* __restrict__ gu = G + (size_t)u * J * S + bic;
            for (int c = 0; c < nch; ++c) {
                float v[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int j = P0 + 7 - 8 * c - r;
                    v[r] = gu[(size_t)min(max(j, 0), J - 1) * S];
                }
#pragma unroll
                for (int r = 0; r < 8; ++r) KEEP(v[r]);
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    const int j = P0 + 7 - 8 * c - r;
                    const float g = (j >= 0 && j < J) ? v[r] : 0.f;
#pragma unroll
                    for (int i = 0; i < PG_POS; ++i) {
                        const int t = 8 * c + r + i - 7;
                        if ((unsigned)t < (unsigned)k) fma4(acc[i], wu[t], g);
                    }
                }
            }
        }
    }
    if (!live || P0 >= L) return;
    float* __restrict__ ob = ig + (size_t)(b0 + bi) * 4 * L;
#pragma unroll
    for (int i = 0; i < PG_POS; ++i) {
        const int p = P0 + i;
        if (p >= L) break;
        const int sx = codesT[(size_t)p * Bs + b0 + bi], sb = BT[(size_t)p * S + bi];
        const float av[4] = {acc[i].x, acc[i].y, acc[i].z, acc[i].w};
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float xv = sx == a ? 1.f : 0.f;
            const float bv = sb == a ? 1.f : (sb == PG_CODE_UNIFORM ? 0.25f : 0.f);
            const float d = xv - bv;
            ob[(size_t)a * L + p] = d != 0.f ? d * av[a] : 0.f;       // exactly 0 where x == x'
        }
    }
}

// ---------------------------------------------------------------------------------------------
int launch_pathgrad(explainn_ctx* c, const explainn_params* p, int B, int kind, const uint8_t* base_codes,
                    int rc, const float* dlogits, int steps, float* ig, float* logits_x, float* logits_base,
                    void* ws, int64_t ws_bytes, hipStream_t s) {
    // the sub-batch the caller's workspace holds: the rule of pathgrad_sub_batch on ws_bytes
    const int64_t least = SUB_BATCH_STEP * pg_per_sequence_bytes(c);
    if (ws_bytes < least) {
        explainn_set_error("integrated-gradients workspace of %lld bytes holds no 64-sequence sub-batch "
                           "(%lld needed)", (long long)ws_bytes, (long long)least);
        return EXPLAINN_E_ARG;
    }
    const int S = sub_batch_of(ws_bytes, pg_per_sequence_bytes(c), B), J = POOLW * c->n;
    const size_t plane = (size_t)c->U * J * S;
    float* G = static_cast<float*>(ws);
    float* GX = G + plane;
    float* GB = GX + plane;
    float* O = GB + plane;
    uint8_t* BT = reinterpret_cast<uint8_t*>(O + (size_t)2 * c->U * S);
    const size_t sm = (size_t)c->n * FC_H * sizeof(float);            // <= 64 KB (n <= 160)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pg_path_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    for (int b0 = 0; b0 < B; b0 += S) {
        const int Bsub = min(S, B - b0);
        hipLaunchKernelGGL(pg_base_kernel, dim3((S + 255) / 256, c->L), dim3(256), 0, s, base_codes, kind, rc,
                           BT, c->L, b0, Bsub, S);
        LAUNCH_CHECK();
        const int chunks = (Bsub + 64 * PG_WAVES - 1) / (64 * PG_WAVES);
        hipLaunchKernelGGL(pg_path_kernel, dim3(chunks, units_grid(c->U)), dim3(64 * PG_WAVES), sm, s,
                           c->codesT, BT, p->conv_w, c->alpha, c->shift, c->A2, c->sh2, p->fc2_w, p->fc2_b,
                           p->bn3_w, p->bn3_b, p->bn3_rm, p->bn3_rv, dlogits, p->final_w, G, GX, GB, O, c->U,
                           c->T, c->k, c->n, c->NS, c->Bs, b0, Bsub, S, steps);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(pg_logits_kernel, dim3((Bsub + 255) / 256, c->T, 2), dim3(256), 0, s, O, p->final_w,
                           p->final_b, logits_x, logits_base, c->U, c->T, b0, Bsub, S);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(pg_gather_kernel, dim3((Bsub + 63) / 64, (c->L + 4 * PG_POS - 1) / (4 * PG_POS)),
                           dim3(256), 0, s, G, p->conv_w, c->codesT, BT, ig, c->U, c->k, c->L, c->n, c->Bs, b0,
                           Bsub, S);
        LAUNCH_CHECK();
    }
    return EXPLAINN_OK;
}
