// Sync-BN: the training step over R shards of one batch as eight phases with
// an exchange between them, so that every BatchNorm sees the statistics of the WHOLE batch.
//
// A phase runs the existing launches of its part of the step on this rank's B_local sequences and
// ends with a combine kernel that folds the producers' chunk partials into per-unit (per-table)
// fp64 totals: the exchange Xi, whose layout does not depend on B_local.  The caller sums Xi over
// the ranks in place; the next phase starts with a distribute kernel that writes the global totals
// back in the form the consumers already read (chunk 0 = the total, every other chunk 0), and calls
// those consumers with B_global where they divide by the batch.  prep1_stats, prep2 and mid use B
// only as that normaliser, and fin not at all, so the kernels of the per-shard step are unchanged.
//
//   phase 1  pack + filter tables, input moments                 -> X1  pair counts behind G, m
//   phase 2  prep1_stats (B_global), filter bank, qmom           -> X2  sum q, sum q q' about 0
//   phase 3  prep2 (B_global), fc_fwd                            -> X3  sum z, sum z^2
//   phase 4  BatchNorm3 forward + combiner: logits               (no exchange: the forward ends)
//   phase 5  loss gradient (or the caller's dlogits), head sums  -> X4  sum d3, sum d3 zhat, the
//                                                                       combiner gradients, the loss
//   phase 6  BatchNorm3 backward apply, passA                    -> X5  EQ, Se
//   phase 7  mid (B_global), passB, conv_bwd                     -> X6  S1, S2, filter-gradient sums
//   phase 8  fin
//
// Every gradient is then global: the combiner's and BatchNorm3's come from X4, FC / BatchNorm2 from
// the global EQ / Se in mid, the filter and BatchNorm1 from the global S1 / S2 / D in fin.  None is
// reduced again by the caller.
#include "common.h"

namespace {

__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0;
    for (int i = 0; i < nw; ++i) s += red[i];      // fixed order: every rank and run the same bits
    return s;
}

// ---- X1: the exact pair counts.  moments_kernel stores G = count / (B Lo) correctly rounded, so
// G B Lo is within half a unit of the integer count (counts < 2^51): rint recovers it exactly, and
// the distribute step divides the global count exactly as moments_kernel would on the whole batch.
__global__ void sync_bn1_combine(const double* __restrict__ G, const double* __restrict__ m,
                                 double* __restrict__ X, int K4, double BLo) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < K4 * K4) X[i] = rint(G[i] * BLo);
    else if (i < K4 * K4 + K4) X[i] = rint(m[i - K4 * K4] * BLo);
}
__global__ void sync_bn1_dist(const double* __restrict__ X, double* __restrict__ G,
                              double* __restrict__ m, int K4, int B, int Lo) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < K4 * K4) G[i] = X[i] / ((double)B * (double)Lo);
    else if (i < K4 * K4 + K4) m[i - K4 * K4] = X[i] / ((double)B * (double)Lo);
}

// ---- X2: qmom's chunk partials are sums about s = the geometric mean of q over this shard's first 16
// sequences (qs0), a shift no other rank shares.  In fp64 they become sums about zero (an identity, no approximation beyond fp64
// rounding of the products):  sum q = S1 + B s,  sum q q' = S2 + s S1' + S1 s' + B s s'.
// X2 = [U][NS] sum q | [U][NS][NS] sum q q'.
__global__ __launch_bounds__(256) void sync_qmom_combine(const float* __restrict__ qs0,
                                                         const float* __restrict__ S1p,
                                                         const float* __restrict__ S2p,
                                                         double* __restrict__ X, int U, int n, int NS,
                                                         int QCH, int B) {
    const int u = blockIdx.x;
    const float* s1u = S1p + (size_t)u * QCH * NS;
    const float* s2u = S2p + (size_t)u * QCH * NS * NS;
    const float* su = qs0 + (size_t)u * NS;
    double* xa = X + (size_t)u * NS;
    double* xb = X + (size_t)U * NS + (size_t)u * NS * NS;
    for (int e = threadIdx.x; e < NS * NS + NS; e += blockDim.x) {
        if (e < NS) {
            double s1 = 0;
            for (int ch = 0; ch < QCH; ++ch) s1 += (double)s1u[(size_t)ch * NS + e];
            xa[e] = e < n ? s1 + (double)B * (double)su[e] : 0.0;
            continue;
        }
        const int f = e - NS, w = f / NS, wp = f - w * NS;
        if (w >= n || wp >= n) { xb[f] = 0.0; continue; }
        double a = 0, b = 0, c = 0;
        for (int ch = 0; ch < QCH; ++ch) {
            a += (double)s1u[(size_t)ch * NS + w];
            b += (double)s1u[(size_t)ch * NS + wp];
            c += (double)s2u[(size_t)ch * NS * NS + f];
        }
        const double sw = su[w], swp = su[wp];
        xb[f] = c + sw * b + a * swp + (double)B * sw * swp;
    }
}
// The global sums back as chunk 0 of qmom's output, about the shift s = the global mean rounded to
// fp32 (shared by all ranks: it is computed from the exchanged totals).  Cancellation: prep2 forms
// cov = S2/B - (S1/B)^2 with S1 ~ 0 about this shift, so S2 carries the variance directly; the
// fp64 totals lose at most ~1e-16 E[q^2] absolute to rounding, i.e. 1e-16 E[q^2]/var relative --
// below fp32's own rounding of S2 unless var / mean^2 < 1e-8.
__global__ __launch_bounds__(256) void sync_qmom_dist(const double* __restrict__ X,
                                                      float* __restrict__ qs0, float* __restrict__ S1p,
                                                      float* __restrict__ S2p, int U, int n, int NS,
                                                      int QCH, int B) {
    const int u = blockIdx.x;
    const double* xa = X + (size_t)u * NS;
    const double* xb = X + (size_t)U * NS + (size_t)u * NS * NS;
    float* su = qs0 + (size_t)u * NS;
    float* s1u = S1p + (size_t)u * QCH * NS;
    float* s2u = S2p + (size_t)u * QCH * NS * NS;
    const double Bd = (double)B;
    for (int e = threadIdx.x; e < NS * NS + NS; e += blockDim.x) {
        if (e < NS) {
            const float s = e < n ? (float)(xa[e] / Bd) : 0.f;
            su[e] = s;
            s1u[e] = e < n ? (float)(xa[e] - Bd * (double)s) : 0.f;
            for (int ch = 1; ch < QCH; ++ch) s1u[(size_t)ch * NS + e] = 0.f;
            continue;
        }
        const int f = e - NS, w = f / NS, wp = f - w * NS;
        float v = 0.f;
        if (w < n && wp < n) {
            const double sw = (double)(float)(xa[w] / Bd), swp = (double)(float)(xa[wp] / Bd);
            v = (float)(xb[f] - sw * xa[wp] - xa[w] * swp + Bd * sw * swp);
        }
        s2u[f] = v;
        for (int ch = 1; ch < QCH; ++ch) s2u[(size_t)ch * NS * NS + f] = 0.f;
    }
}

// ---- X3: fc_fwd's per-workgroup fp64 sums of z and z^2, summed per unit in workgroup order
__global__ void sync_z_combine(const double* __restrict__ z12p, double* __restrict__ X, int U,
                               int nblk) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    double s1 = 0, s2 = 0;
    for (int i = 0; i < nblk; ++i) {
        s1 += z12p[((size_t)u * nblk + i) * 2];
        s2 += z12p[((size_t)u * nblk + i) * 2 + 1];
    }
    X[2 * u] = s1;
    X[2 * u + 1] = s2;
}

// BatchNorm3 forward from the global sums (the statistics of logits_bn_kernel), one block per unit
__global__ __launch_bounds__(256) void sync_bn3_fwd(const double* __restrict__ X,
                                                    const float* __restrict__ z,
                                                    const float* __restrict__ c2,
                                                    const float* __restrict__ g3,
                                                    const float* __restrict__ b3,
                                                    float* __restrict__ rm3, float* __restrict__ rv3,
                                                    int64_t* nbt, float* __restrict__ zhat,
                                                    float* __restrict__ o, float* __restrict__ sig3,
                                                    int Bs, int B, int Bg) {
    const int u = blockIdx.x;
    const double mean = X[2 * u] / (double)Bg;
    const double var = fmax(X[2 * u + 1] / (double)Bg - mean * mean, 0.0);
    const double sg = sqrt(var + BN_EPS_D);
    const float meanf = (float)mean, isg = (float)(1.0 / sg), gam = g3[u], bet = b3[u];
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float zh = (z[(size_t)u * Bs + b] - meanf) * isg;
        zhat[(size_t)u * Bs + b] = zh;
        o[(size_t)u * Bs + b] = fmaxf(fmaf(gam, zh, bet), 0.f);
    }
    if (threadIdx.x == 0) {
        sig3[u] = (float)sg;
        rm3[u] = (float)((1 - BN_MOM_D) * (double)rm3[u] + BN_MOM_D * (mean + (double)c2[u]));
        rv3[u] = (float)((1 - BN_MOM_D) * (double)rv3[u] + BN_MOM_D * var * (double)Bg / (double)(Bg - 1));
        if (u == 0 && nbt) *nbt += 1;
    }
}

// d loss / d logits of the global mean loss (1 / (B_global T)) and this shard's loss sum -> X4.
// One block (a fixed-order sum, identical bits on every run); like sync_head_sums below it is a
// plain form, not tuned for many tasks -- tools/syncbn_probe.py reports the phases' times.
__global__ __launch_bounds__(1024) void sync_loss(const float* __restrict__ logits,
                                                  const float* __restrict__ y, int kind, int N,
                                                  float invN, float* __restrict__ dl,
                                                  double* __restrict__ xloss) {
    __shared__ double red[16];
    double acc = 0;
    for (int i = threadIdx.x; i < N; i += 1024) {
        const float x = logits[i], t = y[i];
        acc += (double)loss_value(kind, x, t);
        dl[i] = loss_grad(kind, x, t, invN);
    }
    acc = block_sum_d(acc, red);
    if (threadIdx.x == 0) *xloss = acc;
}

// X4 = [U][2] sum d3, sum d3 zhat | [T][U] d Wf | [T] d bf | loss sum.  One block per unit:
// d3 = relu'(o) (Wf^T dl), kept in dz for the apply step.
__global__ __launch_bounds__(256) void sync_head_sums(const float* __restrict__ dl, float scale,
                                                      const float* __restrict__ Wf,
                                                      const float* __restrict__ o,
                                                      const float* __restrict__ zhat,
                                                      float* __restrict__ dz, double* __restrict__ X,
                                                      int U, int T, int Bs, int B) {
    __shared__ double red[4];
    const int u = blockIdx.x;
    const float* ou = o + (size_t)u * Bs;
    const float* zh = zhat + (size_t)u * Bs;
    double s1 = 0, s2 = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        float dob = 0.f;
        for (int t = 0; t < T; ++t) dob = fmaf(dl[(size_t)b * T + t] * scale, Wf[(size_t)t * U + u], dob);
        const float d3 = ou[b] > 0.f ? dob : 0.f;
        dz[(size_t)u * Bs + b] = d3;
        s1 += (double)d3;
        s2 = fma((double)d3, (double)zh[b], s2);
    }
    s1 = block_sum_d(s1, red);
    s2 = block_sum_d(s2, red);
    if (threadIdx.x == 0) { X[2 * u] = s1; X[2 * u + 1] = s2; }
    for (int t = 0; t < T; ++t) {
        double a = 0, c = 0;
        for (int b = threadIdx.x; b < B; b += 256) {
            const double d = (double)(dl[(size_t)b * T + t] * scale);
            a = fma(d, (double)ou[b], a);
            c += d;
        }
        a = block_sum_d(a, red);
        if (threadIdx.x == 0) X[2 * U + (size_t)t * U + u] = a;
        if (u == 0) {
            c = block_sum_d(c, red);
            if (threadIdx.x == 0) X[2 * U + (size_t)T * U + t] = c;
        }
    }
}

// BatchNorm3 backward with the global sums, and the head gradients out of X4
__global__ __launch_bounds__(256) void sync_head_apply(const double* __restrict__ X,
                                                       const float* __restrict__ g3,
                                                       const float* __restrict__ zhat,
                                                       const float* __restrict__ sig3,
                                                       float* __restrict__ dz, float* __restrict__ gWf,
                                                       float* __restrict__ gbf, float* __restrict__ gg3,
                                                       float* __restrict__ gb3, float* __restrict__ gc2,
                                                       float* __restrict__ loss_out, int U, int T,
                                                       int Bs, int B, int Bg) {
    const int u = blockIdx.x;
    const double S1 = X[2 * u], S2 = X[2 * u + 1];
    const float m1 = (float)(S1 / (double)Bg), m2 = (float)(S2 / (double)Bg);
    const float sc = g3[u] / sig3[u];
    float* dzu = dz + (size_t)u * Bs;
    const float* zh = zhat + (size_t)u * Bs;
    for (int b = threadIdx.x; b < B; b += 256) dzu[b] = sc * (dzu[b] - m1 - zh[b] * m2);
    for (int t = threadIdx.x; t < T; t += 256) {
        gWf[(size_t)t * U + u] = (float)X[2 * U + (size_t)t * U + u];
        if (u == 0) gbf[t] = (float)X[2 * U + (size_t)T * U + t];
    }
    if (threadIdx.x == 0) {
        gg3[u] = (float)S2; gb3[u] = (float)S1; gc2[u] = 0.f;
        if (u == 0 && loss_out) *loss_out = (float)(X[2 * U + (size_t)T * U + T] / ((double)Bg * (double)T));
    }
}

// ---- X5: passA's chunk partials summed per unit: [U][NS][100] EQ | [U][100] Se
__global__ __launch_bounds__(256) void sync_passA_combine(const float* __restrict__ EQp,
                                                          const float* __restrict__ Sep,
                                                          double* __restrict__ X, int U, int NS,
                                                          int ACH) {
    const int u = blockIdx.x;
    const int ne = NS * FC_H;
    for (int e = threadIdx.x; e < ne + FC_H; e += blockDim.x) {
        double s = 0;
        if (e < ne) {
            for (int ch = 0; ch < ACH; ++ch) s += (double)EQp[((size_t)u * ACH + ch) * ne + e];
            X[(size_t)u * ne + e] = s;
        } else {
            const int r = e - ne;
            for (int ch = 0; ch < ACH; ++ch) s += (double)Sep[((size_t)u * ACH + ch) * FC_H + r];
            X[(size_t)U * ne + (size_t)u * FC_H + r] = s;
        }
    }
}
__global__ __launch_bounds__(256) void sync_passA_dist(const double* __restrict__ X,
                                                       float* __restrict__ EQp, float* __restrict__ Sep,
                                                       int U, int NS, int ACH) {
    const int u = blockIdx.x;
    const int ne = NS * FC_H;
    for (int e = threadIdx.x; e < ne + FC_H; e += blockDim.x) {
        if (e < ne) {
            const float v = (float)X[(size_t)u * ne + e];
            for (int ch = 0; ch < ACH; ++ch) EQp[((size_t)u * ACH + ch) * ne + e] = ch == 0 ? v : 0.f;
        } else {
            const int r = e - ne;
            const float v = (float)X[(size_t)U * ne + (size_t)u * FC_H + r];
            for (int ch = 0; ch < ACH; ++ch) Sep[((size_t)u * ACH + ch) * FC_H + r] = ch == 0 ? v : 0.f;
        }
    }
}

// ---- X6: passB's S1/S2 tile partials and conv_bwd's filter-gradient partials per unit:
// [U][2] S1, S2 | [U][4k] D
__global__ __launch_bounds__(256) void sync_conv_combine(const float* __restrict__ S12p,
                                                         const float* __restrict__ Dspp,
                                                         double* __restrict__ X, int U, int K4, int NG,
                                                         int NT16, int nt16, int dsp_stride,
                                                         int dsp_count) {
    __shared__ double red[4];
    const int u = blockIdx.x;
    double s1 = 0, s2 = 0;
    for (int t = threadIdx.x; t < NG * nt16; t += 256) {
        const int grp = t / nt16, tl = t - grp * nt16;
        const float* pv = S12p + (((size_t)u * NG + grp) * NT16 + tl) * 2;
        s1 += (double)pv[0]; s2 += (double)pv[1];
    }
    s1 = block_sum_d(s1, red);
    s2 = block_sum_d(s2, red);
    if (threadIdx.x == 0) { X[2 * u] = s1; X[2 * u + 1] = s2; }
    for (int i = threadIdx.x; i < K4; i += 256) {
        double d = 0;
        for (int t = 0; t < dsp_count; ++t) d += (double)Dspp[((size_t)u * dsp_stride + t) * K4 + i];
        X[2 * U + (size_t)u * K4 + i] = d;
    }
}
__global__ __launch_bounds__(256) void sync_conv_dist(const double* __restrict__ X,
                                                      float* __restrict__ S12p, float* __restrict__ Dspp,
                                                      int U, int K4, int NG, int NT16, int nt16,
                                                      int dsp_stride) {
    const int u = blockIdx.x;
    for (int t = threadIdx.x; t < NG * nt16; t += 256) {
        const int grp = t / nt16, tl = t - grp * nt16;
        float* pv = S12p + (((size_t)u * NG + grp) * NT16 + tl) * 2;
        pv[0] = t == 0 ? (float)X[2 * u] : 0.f;
        pv[1] = t == 0 ? (float)X[2 * u + 1] : 0.f;
    }
    for (int i = threadIdx.x; i < K4; i += 256)
        Dspp[((size_t)u * dsp_stride) * K4 + i] = (float)X[2 * U + (size_t)u * K4 + i];
}

#define TRY(call)                           \
    do {                                    \
        int rc_ = (call);                   \
        if (rc_ != EXPLAINN_OK) return rc_; \
    } while (0)

}  // namespace

int64_t sync_exchange_elems(const explainn_ctx* c, int phase) {
    const int64_t U = c->U, NS = c->NS, K4 = c->K4, T = c->T;
    switch (phase) {
        case 1: return K4 * K4 + K4;
        case 2: return U * NS + U * NS * NS;
        case 3: return 2 * U;
        case 5: return 2 * U + T * U + T + 1;
        case 6: return U * NS * FC_H + U * FC_H;
        case 7: return 2 * U + U * K4;
        default: return 0;
    }
}

int sync_phase(explainn_ctx* c, int phase, const explainn_sync_args* a, const double* xin,
               double* xout, hipStream_t s) {
    const int B = a->B_local, Bg = a->B_global;
    const explainn_params* p = a->params;
    const explainn_grads* g = a->grads;
    const int U = c->U;
    switch (phase) {
        case 1:
            c->fwd_B = 0; c->tail_B = 0; c->keep_B = 0;   // (not sync_next: explainn_sync_phase advances it)
            c->eval_valid = false;             // the train-mode folds overwrite the eval-mode tables
            c->dense_x = nullptr;
            if (a->x) TRY(launch_pack_tables(c, a->x, p, B, s));
            else {
                TRY(launch_pack(c, nullptr, B, false, s));
                TRY(launch_prep1_tables(c, p, s));
            }
            TRY(launch_moments(c, B, s));
            hipLaunchKernelGGL(sync_bn1_combine, dim3((c->K4 * c->K4 + c->K4 + 255) / 256), dim3(256), 0, s,
                               c->G, c->m, xout, c->K4, (double)B * (double)c->Lo);
            LAUNCH_CHECK();
            break;
        case 2:
            hipLaunchKernelGGL(sync_bn1_dist, dim3((c->K4 * c->K4 + c->K4 + 255) / 256), dim3(256), 0, s,
                               xin, c->G, c->m, c->K4, Bg, c->Lo);
            LAUNCH_CHECK();
            TRY(launch_prep1(c, p, Bg, true, s));
            TRY(launch_conv_pool(c, p, B, true, s));
            TRY(launch_qmoments(c, B, s));
            hipLaunchKernelGGL(sync_qmom_combine, dim3(U), dim3(256), 0, s, c->qs0, c->qS1p, c->qS2p, xout,
                               U, c->n, c->NS, c->QCH, B);
            LAUNCH_CHECK();
            break;
        case 3:
            hipLaunchKernelGGL(sync_qmom_dist, dim3(U), dim3(256), 0, s, xin, c->qs0, c->qS1p, c->qS2p, U,
                               c->n, c->NS, c->QCH, Bg);
            LAUNCH_CHECK();
            TRY(launch_prep2(c, p, Bg, true, s));
            TRY(launch_fc_fwd(c, p, B, true, a->keep_mask, a->dropout_p, a->seed, s));
            hipLaunchKernelGGL(sync_z_combine, dim3((U + 255) / 256), dim3(256), 0, s, c->z12p, xout, U,
                               fc_fwd_blocks(B, c->NQ));
            LAUNCH_CHECK();
            break;
        case 4:
            hipLaunchKernelGGL(sync_bn3_fwd, dim3(U), dim3(256), 0, s, xin, c->z, p->fc2_b, p->bn3_w,
                               p->bn3_b, p->bn3_rm, p->bn3_rv, p->bn3_nbt, c->zhat, c->o, c->sig3, c->Bs, B,
                               Bg);
            LAUNCH_CHECK();
            TRY(launch_head_fwd(c, p, B, false, a->logits, nullptr, s));
            // fwd_B stays 0: the default backward entry points must not run on a sync step's state
            break;
        case 5: {
            const float* dl = a->dlogits;
            float scale = a->dl_scale;
            if (!dl) {
                hipLaunchKernelGGL(sync_loss, dim3(1), dim3(1024), 0, s, a->logits, a->targets, a->loss_kind,
                                   B * c->T, 1.0f / ((float)Bg * (float)c->T), c->dlogits,
                                   xout + 2 * U + (size_t)c->T * U + c->T);
                LAUNCH_CHECK();
                dl = c->dlogits;
                scale = 1.f;
            } else {
                HIP_TRY(hipMemsetAsync(xout + 2 * U + (size_t)c->T * U + c->T, 0, sizeof(double), s));
            }
            hipLaunchKernelGGL(sync_head_sums, dim3(U), dim3(256), 0, s, dl, scale, p->final_w, c->o,
                               c->zhat, c->dz, xout, U, c->T, c->Bs, B);
            LAUNCH_CHECK();
            break;
        }
        case 6:
            hipLaunchKernelGGL(sync_head_apply, dim3(U), dim3(256), 0, s, xin, p->bn3_w, c->zhat, c->sig3,
                               c->dz, g->final_w, g->final_b, g->bn3_w, g->bn3_b, g->fc2_b,
                               a->dlogits ? nullptr : a->loss_out, U, c->T, c->Bs, B, Bg);
            LAUNCH_CHECK();
            TRY(launch_passA(c, B, nullptr, s));
            hipLaunchKernelGGL(sync_passA_combine, dim3(U), dim3(256), 0, s, c->EQp, c->Sep, xout, U, c->NS,
                               c->ACH);
            LAUNCH_CHECK();
            break;
        case 7:
            hipLaunchKernelGGL(sync_passA_dist, dim3(U), dim3(256), 0, s, xin, c->EQp, c->Sep, U, c->NS,
                               c->ACH);
            LAUNCH_CHECK();
            TRY(launch_mid_bwd(c, p, g, Bg, s));
            TRY(launch_passB(c, B, s));
            TRY(launch_conv_bwd(c, B, s));
            hipLaunchKernelGGL(sync_conv_combine, dim3(U), dim3(256), 0, s, c->S12p, c->Dspp, xout, U, c->K4,
                               fc_ng(c->NQ), c->Bs / 16, (B + 15) / 16, c->dsp_stride, c->dsp_count);
            LAUNCH_CHECK();
            break;
        case 8:
            hipLaunchKernelGGL(sync_conv_dist, dim3(U), dim3(256), 0, s, xin, c->S12p, c->Dspp, U, c->K4,
                               fc_ng(c->NQ), c->Bs / 16, (B + 15) / 16, c->dsp_stride);
            LAUNCH_CHECK();
            c->dsp_count = 1;
            TRY(launch_fin_bwd(c, p, g, B, a->freeze_top_n_filters, s));
            break;
        default:
            explainn_set_error("sync phase %d outside 1..%d", phase, EXPLAINN_SYNC_PHASES);
            return EXPLAINN_E_ARG;
    }
    return EXPLAINN_OK;
}
