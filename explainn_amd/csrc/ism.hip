// In-silico mutagenesis: the change of every logit when one base of
// a sequence is replaced by each of the other three, in eval mode,
//   delta[b,t,a,p] = logit_t(x_b with column p := one-hot(a)) - logit_t(x_b).
// A substitution at p moves the raw conv sum g[u,j] at j in [p-k+1, p] only, hence at most
// NW = ceil((k-1)/7)+1 pooled windows per unit, hence one correction of FC1's pre-activation:
//   d_j = W[u,a,p-j] - W[u,s,p-j]   (s = the reference base; an N reference contributes 0)
//   dq_w = qval(alpha, ext over the window of g + d, shift) - q_w
//   y2' = y2 + sum_w A2[:,w] dq_w,  z' = fc2_w . relu(y2') ,  o' = relu(BN3_eval(z' + fc2_b))
//   delta[b,t,a,p] = sum_u final_w[t,u] (o'_u - o_u)       (units in order)
// The unit itself (window sums, FC1, FC2, BatchNorm3, the LDS tables) is unit_eval.h's.
// ism_units: workgroup = (256 sequences, unit), lane = sequence.  Each lane rebuilds its own g, y2
// and o from the codes with the same code that evaluates the substitutions, so a substitution that
// changes no pooled extreme gives exactly 0.  Lanes iterate over a = (s + d) & 3, d = 1..3 (an N
// reference counts as s = 0 there, and a wave-uniform extra pass d = 0 covers a = 0 where some lane
// has N at p), so the three substitutions of a position share the A2 reads.  The unit's A2 (as
// [w][100]) and fc2 row sit in LDS and are read at wave-uniform addresses.  Out: dout[u][d][p][b].
// ism_sum: delta = sum_u final_w[t,u] dout[u][d][p][b], one owner per element, units in order;
// reference rows and positions whose windows MaxPool1d drops are written as 0.  No float atomics.
#include "common.h"
#include "unit_eval.h"

#define ISM_WAVES 4
#define ISM_RING 64                // per-lane code ring (positions mod 64), >= k + 13
#define ISM_SUM_P 4                // positions per ism_sum workgroup (one per wave)
#define ISM_UNROLL 8               // units per load batch in ism_sum
#define ISM_WS_CAP (1LL << 30)     // workspace bytes the sub-batch size aims at

__host__ __device__ inline int ism_nw(int k) { return (k + 5) / 7 + 1; }   // ceil((k-1)/7) + 1
__host__ __device__ inline int ism_pend(int k, int n, int L) { return min(L, POOLW * n + k - 1); }

// The pooled extreme as MaxPool1d folds it (fmaxf; pathgrad.hip's pg_pool needs the index and compares)
__device__ __forceinline__ float ism_ext(const float* g, float sg) {
    float m = sg * g[0];
#pragma unroll
    for (int e = 1; e < POOLW; ++e) m = fmaxf(m, sg * g[e]);
    return sg * m;
}

// z[d] = sum_r fc2[r] relu(y2[r] + sum_(slots i) A2[wb+i][r] dq[d][i]), r and i ascending.
template <int ND, int NW>
__device__ __forceinline__ void ism_fc(const float (&y2)[FC_H], const float* __restrict__ A2T,
                                       const float* __restrict__ fcs, const float (&dq)[ND][NW], int wb,
                                       float (&z)[ND]) {
#pragma unroll
    for (int d = 0; d < ND; ++d) z[d] = 0.f;
    const int fo = unit_opaque_zero();             // on every LDS read below (unit_eval.h)
#pragma unroll
    for (int r4 = 0; r4 < FC_H / 4; ++r4) {
        float y[ND][4];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int i = 0; i < 4; ++i) y[d][i] = y2[4 * r4 + i];
        // every slot, also those whose dq is 0 in every lane: a branch per slot, the same for all r4,
        // is merged by the compiler into one per slot around all 25 chunks -- 100 ND registers live
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const float4 a = *reinterpret_cast<const float4*>(A2T + fo + max(wb + i, 0) * FC_H + 4 * r4);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                y[d][0] = fmaf(a.x, dq[d][i], y[d][0]); y[d][1] = fmaf(a.y, dq[d][i], y[d][1]);
                y[d][2] = fmaf(a.z, dq[d][i], y[d][2]); y[d][3] = fmaf(a.w, dq[d][i], y[d][3]);
            }
        }
        const float4 f = *reinterpret_cast<const float4*>(fcs + fo + 4 * r4);
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            z[d] = fmaf(f.x, fmaxf(y[d][0], 0.f), z[d]); z[d] = fmaf(f.y, fmaxf(y[d][1], 0.f), z[d]);
            z[d] = fmaf(f.z, fmaxf(y[d][2], 0.f), z[d]); z[d] = fmaf(f.w, fmaxf(y[d][3], 0.f), z[d]);
        }
    }
}

// dq[i] of every slot for substitution base a (per lane): window = slot's g with d_j added where
// t = p - j is a tap.  Slots not in vmask stay 0.
template <int NW>
__device__ __forceinline__ void ism_dq(const float (&G)[NW][POOLW], const float (&q0)[NW],
                                       const float (&ws)[NW][POOLW], const float* __restrict__ Wl,
                                       int wb, int p, int k, int a, unsigned vmask, const unit_consts& uc,
                                       float (&dq)[NW]) {
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        dq[i] = 0.f;
        if (vmask & (1u << i)) {
            float g[POOLW];
#pragma unroll
            for (int e = 0; e < POOLW; ++e) {
                const int t = p - (POOLW * (wb + i) + e);
                g[e] = G[i][e];
                if ((unsigned)t < (unsigned)k) g[e] = G[i][e] + (Wl[t * 8 + a] - ws[i][e]);
            }
            dq[i] = qval(uc.al, ism_ext(g, uc.sg), uc.sh) - q0[i];
        }
    }
}

template <int NW>
__global__ __launch_bounds__(64 * ISM_WAVES) void ism_units_kernel(
    const uint8_t* __restrict__ codesT, const float* __restrict__ conv_w, const float* __restrict__ alpha,
    const float* __restrict__ shift, const float* __restrict__ A2, const float* __restrict__ sh2,
    const float* __restrict__ fc2_w, const float* __restrict__ fc2_b, const float* __restrict__ g3,
    const float* __restrict__ b3, const float* __restrict__ rm3, const float* __restrict__ rv3,
    float* __restrict__ dout, int U, int k, int L, int n, int NS, int Bs, int b0, int Bsub, int S) {
    extern __shared__ __attribute__((aligned(16))) float ism_sm[];    // A2T [n][FC_H]
    __shared__ __attribute__((aligned(16))) float Wl[MAX_K * 8];      // [t][a], a = 4..7 -> 0 (N)
    __shared__ __attribute__((aligned(16))) float fcs[FC_H];
    __shared__ uint8_t ring[ISM_WAVES][ISM_RING * 64];
    int u, chunk;
    if (!unit_chunk_of_block(U, u, chunk)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unit_stage<false>(A2, conv_w, fc2_w, u, k, n, NS, tid, 64 * ISM_WAVES, ism_sm, Wl, fcs);
    __syncthreads();
    const int bw = chunk * 64 * ISM_WAVES + wave * 64;
    if (bw >= Bsub) return;                        // wave-uniform; no barrier below
    const int bi = bw + lane;
    const bool live = bi < Bsub;
    const uint8_t* __restrict__ col = codesT + b0 + min(bi, Bsub - 1);
    uint8_t* rg = ring[wave];
    const float* A2T = ism_sm;
    const unit_consts uc = unit_load(alpha, shift, fc2_b, g3, b3, rm3, rv3, u);
    const auto code = [&](int q) -> int { return rg[(q & (ISM_RING - 1)) * 64 + lane]; };

    // code ring: positions [0, k+6) first; window w > 0 adds [7w+k-1, 7w+k+6) from pf (loaded one
    // window ahead).  Only this lane's column is touched: no barrier.
    uint8_t pf[POOLW];
    auto ring_start = [&]() {
        uint8_t c0[MAX_K + POOLW - 1];
#pragma unroll
        for (int i = 0; i < MAX_K + POOLW - 1; ++i) c0[i] = col[(size_t)min(i, L - 1) * Bs];
#pragma unroll
        for (int i = 0; i < MAX_K + POOLW - 1; ++i)
            if (i < k + POOLW - 1) rg[i * 64 + lane] = c0[i];
#pragma unroll
        for (int i = 0; i < POOLW; ++i) pf[i] = col[(size_t)min(k + POOLW - 1 + i, L - 1) * Bs];
    };
    auto ring_advance = [&](int w) {              // window w >= 1 enters
        const int q = POOLW * w + k - 1;
#pragma unroll
        for (int i = 0; i < POOLW; ++i) rg[((q + i) & (ISM_RING - 1)) * 64 + lane] = pf[i];
#pragma unroll
        for (int i = 0; i < POOLW; ++i) pf[i] = col[(size_t)min(q + POOLW + i, L - 1) * Bs];
    };

    // ---- the unmutated sequence: y2 = sh2 + sum_w A2[:,w] q_w (w ascending), z, o ----
    float y2[FC_H];
#pragma unroll
    for (int r = 0; r < FC_H; ++r) y2[r] = sh2[(size_t)u * FC_H + r];
    ring_start();
    for (int w = 0; w < n; ++w) {
        if (w > 0) ring_advance(w);
        float g[POOLW];
        unit_window(code, Wl, w, k, g);
        const float q = qval(uc.al, ism_ext(g, uc.sg), uc.sh);
        UNIT_FC1_ADD(y2, reinterpret_cast<const float4*>(A2T + w * FC_H), q);
    }
    // z by the chain of ism_fc, channels ascending (with every dq = 0 that gives these values:
    // fmaf(a, 0, y) = y)
    float z0;
    UNIT_FC2(z0, y2, fcs);
    const float o0 = fmaxf(unit_bn3(uc, z0), 0.f);

    // ---- the substitutions, position by position ----
    // G[i] = g of window wt - (NW-1) + i (wt = the newest window entered); every window a
    // substitution at p reaches is among them (whi - wlo <= NW - 1)
    float G[NW][POOLW];
#pragma unroll
    for (int i = 0; i < NW; ++i)
#pragma unroll
        for (int e = 0; e < POOLW; ++e) G[i][e] = 0.f;
    ring_start();
    int wt = -1;
    const int pend = ism_pend(k, n, L);
    const size_t plane = (size_t)L * S;          // dout stride of one substitution slot d
    float* __restrict__ du = dout + (size_t)u * 4 * plane + bi;
    for (int p = 0; p < pend; ++p) {
        if (p % POOLW == 0 && p / POOLW < n) {
            wt = p / POOLW;
            if (wt > 0) ring_advance(wt);
#pragma unroll
            for (int i = 0; i + 1 < NW; ++i)
#pragma unroll
                for (int e = 0; e < POOLW; ++e) G[i][e] = G[i + 1][e];
            unit_window(code, Wl, wt, k, G[NW - 1]);
        }
        const int wb = wt - (NW - 1);
        const int wlo = p - k + 1 <= 0 ? 0 : (p - k + 1) / POOLW;
        unsigned vmask = 0;                        // slots holding a window the substitution reaches
#pragma unroll
        for (int i = 0; i < NW; ++i) if (wb + i >= wlo) vmask |= 1u << i;
        const int s = rg[(p & (ISM_RING - 1)) * 64 + lane];
        const int sa = s < 4 ? s : 0;
        float q0[NW], ws[NW][POOLW];
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            q0[i] = 0.f;
#pragma unroll
            for (int e = 0; e < POOLW; ++e) ws[i][e] = 0.f;
            if (vmask & (1u << i)) {
                q0[i] = qval(uc.al, ism_ext(G[i], uc.sg), uc.sh);
#pragma unroll
                for (int e = 0; e < POOLW; ++e) {
                    const int t = p - (POOLW * (wb + i) + e);
                    if ((unsigned)t < (unsigned)k) ws[i][e] = Wl[t * 8 + s];
                }
            }
        }
        float dq[3][NW];
#pragma unroll
        for (int d = 0; d < 3; ++d) ism_dq<NW>(G, q0, ws, Wl, wb, p, k, (sa + d + 1) & 3, vmask, uc, dq[d]);
        bool moved = false;                        // some extreme of this lane moved
#pragma unroll
        for (int i = 0; i < NW; ++i) moved = moved || dq[0][i] != 0.f || dq[1][i] != 0.f || dq[2][i] != 0.f;
        float o3[3] = {0.f, 0.f, 0.f};
        if (__any(live && moved)) {
            float z[3];
            ism_fc<3, NW>(y2, A2T, fcs, dq, wb, z);
#pragma unroll
            for (int d = 0; d < 3; ++d) o3[d] = fmaxf(unit_bn3(uc, z[d]), 0.f) - o0;
        }
        if (live) {
#pragma unroll
            for (int d = 0; d < 3; ++d) du[(size_t)(d + 1) * plane + (size_t)p * S] = o3[d];
        }
        // a = 0 where the reference is N (the passes above covered a = 1, 2, 3 there)
        if (__any(live && s >= 4)) {
            float dn[1][NW];
            ism_dq<NW>(G, q0, ws, Wl, wb, p, k, 0, vmask, uc, dn[0]);
            bool nmoved = false;
#pragma unroll
            for (int i = 0; i < NW; ++i) nmoved = nmoved || dn[0][i] != 0.f;
            float on = 0.f;
            if (__any(live && s >= 4 && nmoved)) {
                float z[1];
                ism_fc<1, NW>(y2, A2T, fcs, dn, wb, z);
                on = fmaxf(unit_bn3(uc, z[0]), 0.f) - o0;
            }
            if (live && s >= 4) du[(size_t)p * S] = on;
        }
    }
}

// delta[b][t][a][p] for the sub-batch [b0, b0+Bsub): workgroup = (64 sequences, ISM_SUM_P positions),
// wave = position, lane = sequence; tasks in chunks of TC, units in order.
template <int TC>
__global__ __launch_bounds__(64 * ISM_SUM_P) void ism_sum_kernel(
    const float* __restrict__ dout, const uint8_t* __restrict__ codesT, const float* __restrict__ final_w,
    float* __restrict__ delta, int U, int T, int k, int L, int n, int Bs, int b0, int Bsub, int S) {
    const int lane = threadIdx.x & 63, p = blockIdx.y * ISM_SUM_P + (threadIdx.x >> 6);
    const int bi = blockIdx.x * 64 + lane;
    if (p >= L) return;
    const bool live = bi < Bsub;
    const int bic = min(bi, Bsub - 1), b = b0 + bic;
    const int s = codesT[(size_t)p * Bs + b];
    const int sa = s < 4 ? s : 0;
    const bool tail = p >= ism_pend(k, n, L);
    const size_t plane = (size_t)L * S;
    float* __restrict__ db = delta + (size_t)b * T * 4 * L + p;
    for (int d = 0; d < 4; ++d) {
        const int a = (sa + d) & 3;
        // d = 0 is the reference base (exactly 0) unless the reference is N
        const bool own = d > 0 || s >= 4;
        const bool any = !tail && __any(live && own);
        for (int t0 = 0; t0 < T; t0 += TC) {
            float acc[TC];
#pragma unroll
            for (int j = 0; j < TC; ++j) acc[j] = 0.f;
            if (any) {
                const float* __restrict__ src = dout + (size_t)d * plane + (size_t)p * S + bic;
                for (int u0 = 0; u0 < U; u0 += ISM_UNROLL) {
                    float v[ISM_UNROLL];
#pragma unroll
                    for (int j = 0; j < ISM_UNROLL; ++j)
                        v[j] = src[(size_t)min(u0 + j, U - 1) * 4 * plane];
#pragma unroll
                    for (int j = 0; j < ISM_UNROLL; ++j) KEEP(v[j]);
#pragma unroll
                    for (int j = 0; j < ISM_UNROLL; ++j) {
                        if (u0 + j < U) {
                            const float x = own ? v[j] : 0.f;
#pragma unroll
                            for (int tt = 0; tt < TC; ++tt)
                                acc[tt] = fmaf(final_w[(size_t)min(t0 + tt, T - 1) * U + u0 + j], x, acc[tt]);
                        }
                    }
                }
            }
            if (live) {
#pragma unroll
                for (int tt = 0; tt < TC; ++tt)
                    if (t0 + tt < T) db[((size_t)(t0 + tt) * 4 + a) * L] = own ? acc[tt] : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// sub-batch: a multiple of 64 sequences whose dout stays near ISM_WS_CAP (at least 64): sub_batch_of's
// rule, in the text tests/dispatch_model.py reads the step and the cap from
static_assert(SUB_BATCH_STEP == 64, "ism_sub_batch spells the step of sub_batch_of out");
int ism_sub_batch(const explainn_ctx* c, int B) {
    const int64_t per = (int64_t)c->U * 4 * c->L * (int64_t)sizeof(float);
    int64_t s = ISM_WS_CAP / per / 64 * 64;
    if (s < 64) s = 64;
    const int64_t bb = ((int64_t)B + 63) / 64 * 64;
    return (int)(s < bb ? s : bb);
}

int64_t ism_workspace_bytes(const explainn_ctx* c, int B) {
    return (int64_t)c->U * 4 * c->L * (int64_t)ism_sub_batch(c, B) * (int64_t)sizeof(float);
}

template <int NW>
static int ism_units_launch(explainn_ctx* c, const explainn_params* p, float* ws, int b0, int Bsub, int S,
                            hipStream_t s) {
    const size_t sm = (size_t)c->n * FC_H * sizeof(float);            // <= 64 KB (n <= 160)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ism_units_kernel<NW>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    const int chunks = (Bsub + 64 * ISM_WAVES - 1) / (64 * ISM_WAVES);
    hipLaunchKernelGGL((ism_units_kernel<NW>), dim3(chunks, units_grid(c->U)), dim3(64 * ISM_WAVES), sm, s,
                       c->codesT, p->conv_w, c->alpha, c->shift, c->A2, c->sh2, p->fc2_w, p->fc2_b,
                       p->bn3_w, p->bn3_b, p->bn3_rm, p->bn3_rv, ws, c->U, c->k, c->L, c->n, c->NS, c->Bs,
                       b0, Bsub, S);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

int launch_ism(explainn_ctx* c, const explainn_params* p, int B, float* delta, float* ws, hipStream_t s) {
    const int S = ism_sub_batch(c, B);
    for (int b0 = 0; b0 < B; b0 += S) {
        const int Bsub = min(S, B - b0);
        int rc = EXPLAINN_OK;
        switch (ism_nw(c->k)) {
            case 2: rc = ism_units_launch<2>(c, p, ws, b0, Bsub, S, s); break;
            case 3: rc = ism_units_launch<3>(c, p, ws, b0, Bsub, S, s); break;
            case 4: rc = ism_units_launch<4>(c, p, ws, b0, Bsub, S, s); break;
            case 5: rc = ism_units_launch<5>(c, p, ws, b0, Bsub, S, s); break;
            case 6: rc = ism_units_launch<6>(c, p, ws, b0, Bsub, S, s); break;
            default: explainn_set_error("kernel_size %d has no ISM instantiation", c->k); return EXPLAINN_E_UNSUPPORTED;
        }
        if (rc != EXPLAINN_OK) return rc;
        const dim3 grid((Bsub + 63) / 64, (c->L + ISM_SUM_P - 1) / ISM_SUM_P);
#define ISM_SUM_ARGS grid, dim3(64 * ISM_SUM_P), 0, s, ws, c->codesT, p->final_w, delta, c->U, c->T, c->k, \
                     c->L, c->n, c->Bs, b0, Bsub, S
        if (c->T == 1) hipLaunchKernelGGL((ism_sum_kernel<1>), ISM_SUM_ARGS);
        else if (c->T <= 4) hipLaunchKernelGGL((ism_sum_kernel<4>), ISM_SUM_ARGS);
        else hipLaunchKernelGGL((ism_sum_kernel<8>), ISM_SUM_ARGS);
#undef ISM_SUM_ARGS
        LAUNCH_CHECK();
    }
    return EXPLAINN_OK;
}
