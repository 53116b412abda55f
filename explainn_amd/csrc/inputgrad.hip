// The gradient of the logits with respect to the input x (B,4,L): saliency, gradient x input,
// Integrated Gradients, the per-base contributions TF-MoDISco reads.
//
// With g[b,u,j] the conv output (j < Lo), dy[u][w][b] = dL/d(BatchNorm1 output) at window w's argmax
// p* = 7w + idx (what passB leaves, or ig_eval_dy below in eval mode), alpha = gamma1/sigma1,
// S1 = sum dy, S2 = sum dy*chat (the sums fin_unit forms), N = B*Lo:
//   train  dL/dg[b,u,j] = alpha (dy [j = p*] - S1/N - (S2/sigma1) (g - mu)/N)
//   eval   dL/dg[b,u,j] = alpha dy [j = p*]
//   dx[b,a,p] = sum_u sum_(t: 0 <= p-t < Lo) W[u,a,t] dL/dg[b,u,p-t]
// Three terms: the sparse one (alpha dy W at p* + t, the only one in eval mode), a constant (4, L)
// table and -- because the g term is linear in x -- sum_(d,a') H_p[a,a',d] x[b,a',p+d] with
//   H_p[a,a',d] = sum_u c_u sum_(t valid at p, 0 <= t+d < k) W[u,a,t] W[u,a',t+d],
//   c_u = -alpha_u S2_u / (sigma1_u N).
// "t valid at p" is t in [tlo, thi] = [max(0, p-Lo+1), min(k-1, p)]; tlo + thi is nondecreasing in p
// and identifies the pair, so it indexes the 2k-1 distinct tables (the interior class is k-1).
// Every sum is in a fixed order; no float atomics.
#include "common.h"
#include "unit_eval.h"

#define IG_POS 8             // positions per input_grad workgroup
#define IG_UT 64             // units whose filters one LDS pass stages (16 per wave)

__device__ __forceinline__ int ig_class(int p, int k, int Lo) {
    return max(0, p - Lo + 1) + min(k - 1, p);
}

// ---------------------------------------------------------------------------------------------
// Eval mode: dy from dlogits through the eval-mode head and FC (DESIGN section 3 item 5 with the
// eval tables: T = V2 A2, k0' = 0, M = 0, no dropout).  Workgroup = (128 sequences, unit), lane =
// sequence.  y2 = A2 q + sh2 is recomputed here (the forward keeps no ReLU bits in eval mode): the
// unit's A2 is staged in LDS (rows padded to whole chunks of 16 pooled positions, zeros past n) and
// read at wave-uniform addresses; each thread's 100 channels live in an LDS column, the pooled
// positions go by in register chunks of 16 -- another layout of unit_eval.h's algebra.
#define IG_WC 16
#define IG_DY_THREADS 128
__host__ __device__ inline int ig_nsp(int n) { return (n + IG_WC - 1) / IG_WC * IG_WC; }
__global__ __launch_bounds__(IG_DY_THREADS) void ig_eval_dy_kernel(
    const float* __restrict__ dl, const float* __restrict__ final_w, const float* __restrict__ g3,
    const float* __restrict__ rv3, const float* __restrict__ fc2_w, const float* __restrict__ o,
    const float* __restrict__ ext, const float* __restrict__ alpha, const float* __restrict__ shift,
    const float* __restrict__ A2, const float* __restrict__ sh2, float* __restrict__ dy, int U,
    int T, int n, int NS, int Bs, int B) {
    extern __shared__ __attribute__((aligned(16))) float igsm[];
    float* ys = igsm;                                  // [FC_H][IG_DY_THREADS]
    float* A2s = igsm + FC_H * IG_DY_THREADS;          // [FC_H][nsp]
    const int u = blockIdx.y, tid = threadIdx.x, b = blockIdx.x * IG_DY_THREADS + tid;
    const int nsp = ig_nsp(n);
    const bool live = b < B;
    const float* __restrict__ Au = A2 + (size_t)u * FC_H * NS;
    for (int i = tid; i < FC_H * nsp; i += IG_DY_THREADS) {
        const int r = i / nsp, w = i - r * nsp;
        A2s[i] = w < n ? Au[(size_t)r * NS + w] : 0.f;
    }
    for (int r = 0; r < FC_H; ++r) ys[r * IG_DY_THREADS + tid] = sh2[(size_t)u * FC_H + r];
    const float a1 = alpha[u], s1 = shift[u];
    const float* __restrict__ eu = ext + (size_t)u * n * Bs;
    const int bl = min(b, Bs - 1);
    __syncthreads();
    for (int w0 = 0; w0 < n; w0 += IG_WC) {
        float q[IG_WC];
#pragma unroll
        for (int j = 0; j < IG_WC; ++j)
            q[j] = (live && w0 + j < n) ? qval(a1, eu[(size_t)min(w0 + j, n - 1) * Bs + bl], s1) : 0.f;
        for (int r = 0; r < FC_H; ++r) {
            const float4* __restrict__ ar = reinterpret_cast<const float4*>(A2s + r * nsp + w0);
            float y = ys[r * IG_DY_THREADS + tid];
#pragma unroll
            for (int j4 = 0; j4 < IG_WC / 4; ++j4) {
                const float4 a = ar[j4];
                y = fmaf(a.x, q[4 * j4], y); y = fmaf(a.y, q[4 * j4 + 1], y);
                y = fmaf(a.z, q[4 * j4 + 2], y); y = fmaf(a.w, q[4 * j4 + 3], y);
            }
            ys[r * IG_DY_THREADS + tid] = y;
        }
    }
    // dz = (dl . Wf[:,u]) [y3 > 0] gamma3 / sqrt(rv3 + eps); y3 > 0 exactly where the stored o is
    const float dout = live ? unit_dout(dl, final_w, b, T, U, u) : 0.f;
    const float inv3 = unit_inv3(g3, rv3, u);
    const float dz = (live && o[(size_t)u * Bs + bl] > 0.f) ? dout * inv3 : 0.f;
    for (int r = 0; r < FC_H; ++r) {
        const float y = ys[r * IG_DY_THREADS + tid];
        ys[r * IG_DY_THREADS + tid] = y > 0.f ? dz * fc2_w[(size_t)u * FC_H + r] : 0.f;
    }
    for (int w0 = 0; w0 < n; w0 += IG_WC) {
        float dq[IG_WC];
#pragma unroll
        for (int j = 0; j < IG_WC; ++j) dq[j] = 0.f;
        for (int r = 0; r < FC_H; ++r) {
            const float4* __restrict__ ar = reinterpret_cast<const float4*>(A2s + r * nsp + w0);
            const float e = ys[r * IG_DY_THREADS + tid];
#pragma unroll
            for (int j4 = 0; j4 < IG_WC / 4; ++j4) {
                const float4 a = ar[j4];
                dq[4 * j4] = fmaf(e, a.x, dq[4 * j4]); dq[4 * j4 + 1] = fmaf(e, a.y, dq[4 * j4 + 1]);
                dq[4 * j4 + 2] = fmaf(e, a.z, dq[4 * j4 + 2]); dq[4 * j4 + 3] = fmaf(e, a.w, dq[4 * j4 + 3]);
            }
        }
#pragma unroll
        for (int j = 0; j < IG_WC; ++j) {
            const int w = w0 + j;
            if (live && w < n) {
                const float qv = qval(a1, eu[(size_t)w * Bs + b], s1);
                dy[((size_t)u * n + w) * Bs + b] = dq[j] * qv;       // d/d(BN1 output) = dq * exp'
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Train mode, per unit: S1, S2 from passB's partials (fixed order), then the fp64 coefficients
// coef[u] = {c_u, k_u} with c_u = -alpha S2/(sigma1 N) and k_u = -alpha S1/N - c_u mu (mu = the mean
// of the raw conv sum, mug).  One 64-thread block per unit.
__global__ __launch_bounds__(64) void ig_coef_kernel(const float* __restrict__ S12p,
                                                     const double* __restrict__ sig1,
                                                     const double* __restrict__ mug,
                                                     const float* __restrict__ g1,
                                                     double* __restrict__ coef, int NG, int Bs, int B,
                                                     int Lo) {
    const int u = blockIdx.x, tid = threadIdx.x;
    const int NT16 = Bs / 16, nt16 = (B + 15) / 16;
    double S1 = 0, S2 = 0;
    for (int t = tid; t < NG * nt16; t += 64) {
        const int grp = t / nt16, tl = t - grp * nt16;
        const float2 pv = *reinterpret_cast<const float2*>(&S12p[(((size_t)u * NG + grp) * NT16 + tl) * 2]);
        S1 += (double)pv.x; S2 += (double)pv.y;
    }
    S1 = wave_sum_d(S1); S2 = wave_sum_d(S2);
    if (tid == 0) {
        const double sg = sig1[u], a = (double)g1[u] / sg, N = (double)B * (double)Lo;
        const double cu = -a * S2 / (sg * N);
        coef[2 * u] = cu;
        coef[2 * u + 1] = -a * S1 / N - cu * mug[u];
    }
}

// P[d][a'][a][t] = sum_u c_u W[u,a,t] W[u,a',t+d-(k-1)] (0 where t+d-(k-1) is outside the filter) and
// R[a][t] = sum_u k_u W[u,a,t]: one thread per entry, units in order, fp64.
__global__ __launch_bounds__(256) void ig_pair_kernel(const float* __restrict__ W,
                                                      const double* __restrict__ coef,
                                                      double* __restrict__ P, double* __restrict__ R,
                                                      int U, int k) {
    const int D = 2 * k - 1, K4 = 4 * k;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < D * 16 * k) {
        const int t = e % k, a = (e / k) & 3, a2 = (e / (4 * k)) & 3, d = e / (16 * k);
        const int t2 = t + d - (k - 1);
        double s = 0;
        if (t2 >= 0 && t2 < k)
            for (int u = 0; u < U; ++u)
                s = fma(coef[2 * u] * (double)W[(size_t)u * K4 + a * k + t], (double)W[(size_t)u * K4 + a2 * k + t2], s);
        P[e] = s;
    } else if (e < D * 16 * k + K4) {
        const int i = e - D * 16 * k;                       // = a*k + t
        double s = 0;
        for (int u = 0; u < U; ++u) s = fma(coef[2 * u + 1], (double)W[(size_t)u * K4 + i], s);
        R[i] = s;
    }
}

// Hc[cls][d][a'] (float4 over a) = sum_(t in [tlo,thi]) P[d][a'][a][t]; Cc[cls] (float4 over a) =
// sum_(t in [tlo,thi]) R[a][t], for the class cls = tlo + thi of some position (classes no position
// has stay zero).
__global__ __launch_bounds__(256) void ig_tables_kernel(const double* __restrict__ P,
                                                        const double* __restrict__ R,
                                                        float* __restrict__ Hc, float* __restrict__ Cc,
                                                        int k, int L, int Lo) {
    const int D = 2 * k - 1;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= D * (D * 16 + 4)) return;
    const int cls = e / (D * 16 + 4), i = e % (D * 16 + 4);
    int tlo = 0, thi = -1;
    for (int p = 0; p < L; ++p)
        if (ig_class(p, k, Lo) == cls) { tlo = max(0, p - Lo + 1); thi = min(k - 1, p); break; }
    double s = 0;
    if (i < D * 16) {
        const int a = i & 3, a2 = (i >> 2) & 3, d = i >> 4;
        for (int t = tlo; t <= thi; ++t) s += P[(((size_t)d * 4 + a2) * 4 + a) * k + t];
        Hc[(size_t)cls * D * 16 + i] = (float)s;
    } else {
        const int a = i - D * 16;
        for (int t = tlo; t <= thi; ++t) s += R[a * k + t];
        Cc[cls * 4 + a] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------
// dx as a gather: workgroup = (64 sequences, IG_POS = 8 positions), lane = sequence (dy, idx and the
// codes are [..][b]: coalesced).  The four waves split the units: per LDS pass IG_UT units' filters
// (times alpha, float4 over the bases) are staged and wave w takes units 16w .. 16w+15 of them, in
// order, for all eight positions; a unit's windows are loaded together (one memory round trip) while
// the previous unit is summed.  The four wave sums are added in wave order through LDS, the train
// terms are added per position, and the tile goes out through LDS along p.  Deterministic.
//   TRAIN  adds the constant table and the H term: one-hot input looks up H[cls][d][s] (N adds 0),
//          DENSE input multiplies H by x (4 FMAs per (d, a')).
#define IG_WMAX 8            // windows whose argmax can reach 8 consecutive positions: <= (k+12)/7 + 1
__device__ __forceinline__ void ig_load_unit(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                             size_t row, int wlo, int whi, int Bs, int b, float* dv, int* iv) {
#pragma unroll
    for (int j = 0; j < IG_WMAX; ++j) {
        const size_t o = (row + min(wlo + j, whi)) * Bs + b;
        dv[j] = dy[o];
        iv[j] = idx[o];
    }
}

template <bool TRAIN, bool DENSE>
__global__ __launch_bounds__(256) void input_grad_kernel(
    const float* __restrict__ dy, const uint8_t* __restrict__ idx, const float* __restrict__ alpha,
    const float* __restrict__ W, const uint8_t* __restrict__ codesT, const float* __restrict__ x,
    const float4* __restrict__ Hc, const float4* __restrict__ Cc, float* __restrict__ dx, int U,
    int k, int L, int Lo, int n, int Bs, int B) {
    __shared__ float4 Ws[IG_UT * MAX_K];                  // also the wave sums [4][IG_POS][64] float4
    __shared__ float ot[4][64][IG_POS + 1];
    __shared__ uint8_t cs[(IG_POS + 2 * MAX_K - 2) * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b0 = blockIdx.x * 64, b = b0 + lane, P0 = blockIdx.y * IG_POS;
    const bool live = b < B;
    const int bl = min(b, Bs - 1);
    float4 acc[IG_POS];
#pragma unroll
    for (int i = 0; i < IG_POS; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- sparse term: alpha dy W[u,:,p-p*] for every window whose argmax reaches the tile ----
    int wlo = P0 - k - 5;
    wlo = wlo <= 0 ? 0 : (wlo + 6) / 7;
    const int whi = min(n - 1, (P0 + IG_POS - 1) / POOLW);
    for (int u0 = 0; u0 < U; u0 += IG_UT) {
        __syncthreads();
        stage_filters4<true, IG_UT>(W, alpha, u0, U, k, tid, 256, Ws);
        __syncthreads();
        const int ub = u0 + (IG_UT / 4) * wave, ue = min(ub + IG_UT / 4, U);
        if (ub >= ue) continue;                               // wave-uniform
        float dv[IG_WMAX], dn[IG_WMAX];
        int iv[IG_WMAX], in_[IG_WMAX];
        ig_load_unit(dy, idx, (size_t)ub * n, wlo, whi, Bs, bl, dv, iv);
        for (int u = ub; u < ue; ++u) {
            if (u + 1 < ue) ig_load_unit(dy, idx, (size_t)(u + 1) * n, wlo, whi, Bs, bl, dn, in_);
            const float4* __restrict__ wu = Ws + (u - u0) * MAX_K;
#pragma unroll
            for (int j = 0; j < IG_WMAX; ++j) {
                if (wlo + j > whi) break;                     // wave-uniform
                const float d = live ? dv[j] : 0.f;
                const int ps = POOLW * (wlo + j) + iv[j];
#pragma unroll
                for (int i = 0; i < IG_POS; ++i) {
                    const int t = P0 + i - ps;
                    if ((unsigned)t < (unsigned)k) fma4(acc[i], wu[t], d);
                }
            }
#pragma unroll
            for (int j = 0; j < IG_WMAX; ++j) { dv[j] = dn[j]; iv[j] = in_[j]; }
        }
    }
    __syncthreads();
    float4* red = Ws;                                         // [wave][i][lane]
#pragma unroll
    for (int i = 0; i < IG_POS; ++i) red[(wave * IG_POS + i) * 64 + lane] = acc[i];
    if (TRAIN && !DENSE) {
        const int nq = IG_POS + 2 * k - 2, q0 = P0 - (k - 1);
        for (int i = tid; i < nq * 64; i += 256) {
            const int qq = i >> 6, l = i & 63, q = q0 + qq;
            cs[i] = (q >= 0 && q < L && b0 + l < B) ? codesT[(size_t)q * Bs + b0 + l] : (uint8_t)4;
        }
    }
    __syncthreads();
    // ---- wave w finishes positions 2w, 2w+1: the wave sums in order, then the train terms ----
#pragma unroll
    for (int h = 0; h < IG_POS / 4; ++h) {
        const int i = (IG_POS / 4) * wave + h, p = P0 + i;
        float4 s = red[i * 64 + lane];
#pragma unroll
        for (int v = 1; v < 4; ++v) {
            const float4 r = red[(v * IG_POS + i) * 64 + lane];
            s.x += r.x; s.y += r.y; s.z += r.z; s.w += r.w;
        }
        if (TRAIN && p < L) {
            const int D = 2 * k - 1, q0 = P0 - (k - 1);
            const int cls = ig_class(p, k, Lo);
            float4 t = Cc[cls];
            const float4* __restrict__ hrow = Hc + (size_t)cls * D * 4;
            const int dlo = max(0, (k - 1) - p), dhi = min(D - 1, L - 1 - p + (k - 1));
            const float* __restrict__ xb = DENSE ? x + (size_t)min(b, B - 1) * 4 * L : nullptr;
            for (int d = dlo; d <= dhi; ++d) {
                const int q = p + d - (k - 1);
                if (DENSE) {
#pragma unroll
                    for (int a2 = 0; a2 < 4; ++a2) {
                        const float xv = live ? xb[(size_t)a2 * L + q] : 0.f;
                        fma4(t, hrow[d * 4 + a2], xv);
                    }
                } else {
                    const int sc = cs[(q - q0) * 64 + lane];
                    if (sc < 4) {
                        const float4 hv = hrow[d * 4 + sc];
                        t.x += hv.x; t.y += hv.y; t.z += hv.z; t.w += hv.w;
                    }
                }
            }
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        ot[0][lane][i] = s.x; ot[1][lane][i] = s.y; ot[2][lane][i] = s.z; ot[3][lane][i] = s.w;
    }
    __syncthreads();
    // ---- store: (B,4,L) rows run along p ----
    for (int e = tid; e < 64 * 4 * IG_POS; e += 256) {
        const int pl = e % IG_POS, row = e / IG_POS, bb = row >> 2, a = row & 3;
        const int p = P0 + pl;
        if (b0 + bb < B && p < L) dx[((size_t)(b0 + bb) * 4 + a) * L + p] = ot[a][bb][pl];
    }
}

// ---------------------------------------------------------------------------------------------
int launch_ig_eval_dy(explainn_ctx* c, const explainn_params* p, const float* dlogits, int B,
                      hipStream_t s) {
    const size_t sm = (size_t)FC_H * (IG_DY_THREADS + ig_nsp(c->n)) * sizeof(float);   // <= 115 KB (n <= 160)
    if (sm > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&ig_eval_dy_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm));
    hipLaunchKernelGGL(ig_eval_dy_kernel, dim3((B + IG_DY_THREADS - 1) / IG_DY_THREADS, c->U), dim3(IG_DY_THREADS), sm, s, dlogits, p->final_w,
                       p->bn3_w, p->bn3_rv, p->fc2_w, c->o, c->ext, c->alpha, c->shift, c->A2, c->sh2,
                       c->dy, c->U, c->T, c->n, c->NS, c->Bs, B);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

int launch_ig_tables(explainn_ctx* c, const explainn_params* p, int B, hipStream_t s) {
    const int k = c->k, D = 2 * k - 1;
    hipLaunchKernelGGL(ig_coef_kernel, dim3(c->U), dim3(64), 0, s, c->S12p, c->sig1, c->mug, p->bn1_w,
                       c->igcoef, fc_ng(c->NQ), c->Bs, B, c->Lo);
    LAUNCH_CHECK();
    const int npair = D * 16 * k + 4 * k;
    hipLaunchKernelGGL(ig_pair_kernel, dim3((npair + 255) / 256), dim3(256), 0, s, p->conv_w, c->igcoef,
                       c->igP, c->igR, c->U, k);
    LAUNCH_CHECK();
    const int ntab = D * (D * 16 + 4);
    hipLaunchKernelGGL(ig_tables_kernel, dim3((ntab + 255) / 256), dim3(256), 0, s, c->igP, c->igR,
                       c->igH, c->igC, k, c->L, c->Lo);
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}

int launch_input_grad(explainn_ctx* c, const explainn_params* p, int B, bool train, const float* dense_x,
                      float* dx, hipStream_t s) {
    const dim3 grid((B + 63) / 64, (c->L + IG_POS - 1) / IG_POS);
#define IG_ARGS grid, dim3(256), 0, s, c->dy, c->idx, c->alpha, p->conv_w, c->codesT, dense_x, \
                reinterpret_cast<const float4*>(c->igH), reinterpret_cast<const float4*>(c->igC), dx, \
                c->U, c->k, c->L, c->Lo, c->n, c->Bs, B
    if (!train) hipLaunchKernelGGL((input_grad_kernel<false, false>), IG_ARGS);
    else if (dense_x) hipLaunchKernelGGL((input_grad_kernel<true, true>), IG_ARGS);
    else hipLaunchKernelGGL((input_grad_kernel<true, false>), IG_ARGS);
#undef IG_ARGS
    LAUNCH_CHECK();
    return EXPLAINN_OK;
}
