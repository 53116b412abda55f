// extern "C" entry points of libexplainn_hip.so (declared in include/explainn_hip.h) and the
// context that owns the device scratch.  Each entry point enqueues its pipeline stages on the
// caller's stream and returns; see DESIGN.md section 3 for the stage list.
#include <assert.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cstdlib>
#include <cstring>

#include "common.h"
#include "workspace.h"

static thread_local char g_err[512] = "";

void explainn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* explainn_last_error(void) { return g_err; }

namespace {
void carve(explainn_ctx* c, Carver& cv) {
    const int64_t U = c->U, U4 = c->U4, n = c->n, Bs = c->Bs, NS = c->NS, K4 = c->K4;
    cv.take(&c->codesT, (int64_t)c->L * Bs);
    cv.take(&c->pk2, (int64_t)c->PW * Bs);
    cv.take(&c->nmask, (int64_t)c->NW * Bs);
    cv.take(&c->bm, (int64_t)4 * (Bs / 64) * c->Lp);
    cv.take(&c->G, K4 * K4);
    cv.take(&c->m, K4);
    cv.take(&c->alpha, U4);
    cv.take(&c->shift, U4);
    cv.take(&c->mug, U4);
    cv.take(&c->sig1, U4);
    cv.take(&c->Gw, U4 * K4);
    cv.take(&c->Wt, (int64_t)c->Uq * c->k * 20);
    cv.take(&c->Wf, (int64_t)conv_tiles_padded(c->U, c->k) * conv_ksteps(c->k) * 3 * 512);
    cv.take(&c->Wsg, (int64_t)conv_tiles_padded(c->U, c->k) * 32);
    // (rows up to whole unit groups of the filter-bank GEMM: its waves store their padding rows too)
    const int64_t Upad = (int64_t)32 * conv_tiles_padded(c->U, c->k);
    // (+ 64: the dump words behind the last row, see cpm_position)
    cv.take(&c->ext, Upad * n * Bs + 64);
    cv.take(&c->idx, Upad * n * Bs + 64);
    cv.take(&c->qs0, U * NS);
    cv.take(&c->qS1p, U * c->QCH * NS);
    cv.take(&c->qS2p, U * c->QCH * NS * NS);
    cv.take(&c->qbar, U * NS);
    cv.take(&c->VC, U * FC_H * NS);
    cv.take(&c->A2, U * FC_H * NS);
    cv.take(&c->A2f, c->NQ <= FC_BF_MAXN ? 0 : U * FC_MT * fc_nk4q(c->NQ) * 256);
    cv.take(&c->A2h, c->NQ <= FC_BF_MAXN ? U * FC_MT * fc_ks32(c->NQ) * 3 * 256 : 0);
    cv.take(&c->sh2, U * FC_H);
    cv.take(&c->sig2, U * FC_H);
    cv.take(&c->z, U * Bs);
    cv.take(&c->zhat, U * Bs);
    cv.take(&c->o, U * Bs);
    cv.take(&c->sig3, U);
    c->ZBLK = fc_fwd_blocks((int)Bs, c->NQ);
    cv.take(&c->z12p, U * c->ZBLK * 2);
    cv.take(&c->bits, U * Bs + 4);
    cv.take(&c->dz, U * Bs + 4);
    cv.take(&c->EQp, U * c->ACH * FC_H * NS);
    cv.take(&c->Sep, U * c->ACH * FC_H);
    cv.take(&c->EQs, U * FC_H * NS);
    cv.take(&c->Ttf, U * fc_nw16(c->NQ) * 3 * 4 * 256);          // bf16 x 3 pieces (fc.hip passB)
    cv.take(&c->Mff, U * fc_nw16(c->NQ) * 4 * fc_nw16(c->NQ) * 64);
    cv.take(&c->k0p, U * NS);
    cv.take(&c->dy, U4 * n * Bs);
    cv.take(&c->S12p, U * fc_ng(c->NQ) * (Bs / 16) * 2);
    cv.take(&c->Dspp, U * (Bs / 4) * K4);
    cv.take(&c->dlogits, (int64_t)c->maxB * c->Gm * c->T);
    cv.take(&c->flags, 64);
    cv.take(&c->bn1_ticket, 64);
    cv.take(&c->dlT, (int64_t)c->T * Bs);
    cv.take(&c->gWp, c->T > HEAD_GEMM_MIN_T && c->Gm == 1 ? (int64_t)head_gw_chunks(c->maxB) * c->T * (c->U + 1) : 0);
    cv.take(&c->lossp, 256);
    {
        // (a bank and T > PA_HEAD_MAX_T never take the route that uses them)
        const bool sums = c->Gm == 1 && c->T <= PA_HEAD_MAX_T;
        const int64_t blks = (c->maxB + 63) / 64;
        cv.take(&c->hp, sums ? U * blks * (2 + PA_HEAD_MAX_T) : 0);
        cv.take(&c->hb, sums ? blks * (1 + PA_HEAD_MAX_T) : 0);
    }
    cv.take(&c->site_cnt, U4 * Bs);
    cv.take(&c->site_off, U4 * Bs);
    const int64_t D = 2 * c->k - 1;
    cv.take(&c->igcoef, U4 * 2);
    cv.take(&c->igP, D * 16 * c->k);
    cv.take(&c->igR, K4);
    cv.take(&c->igH, D * D * 16);
    cv.take(&c->igC, D * 4);
}

int check_batch(const explainn_ctx* c, int B) {
    if (!c) { explainn_set_error("null context"); return EXPLAINN_E_ARG; }
    if (B < 1 || B > c->maxB) {
        explainn_set_error("batch %d outside [1, max_batch=%d]", B, c->maxB);
        return EXPLAINN_E_ARG;
    }
    return EXPLAINN_OK;
}

#define TRY(call)                    \
    do {                             \
        int rc_ = (call);            \
        if (rc_ != EXPLAINN_OK) return rc_; \
    } while (0)

// Per-stage device times (explainn_stage_timing / explainn_stage_times): with timing on, every
// stage of the training step is bracketed by two HIP events on the launch stream.
const char* const kStageNames[ST_COUNT] = {
    "pack_tables", "moments", "prep1_stats", "conv_pool", "qmom", "prep2", "fc_fwd", "head_fwd",
    "loss", "head_bwd", "passA", "mid", "passB", "conv_bwd", "fin_bwd"};
#define STAGE(id, call)                                                                 \
    do {                                                                                \
        if (c->timing) HIP_TRY(hipEventRecord(c->ev0[id], s));                          \
        TRY(call);                                                                      \
        if (c->timing) { HIP_TRY(hipEventRecord(c->ev1[id], s)); c->timed |= 1u << (id); } \
    } while (0)

// Drop whatever work is pending on the context -- a train forward awaiting its backward (fwd_B), a
// train_step_fc awaiting its _conv half (tail_B), an eval_keep forward awaiting its input gradient
// (keep_B), a sync-BN step between phases (sync_next): their calls then fail with E_STATE.
void drop_pending(explainn_ctx* c) { c->fwd_B = 0; c->tail_B = 0; c->keep_B = 0; c->sync_next = 0; }

// The folded tables depend on the parameters only: rebuilt when the caller's parameter version
// moved (or is unknown), not per batch -- predict.py's loop and a validation pass run pack +
// filter bank + FC + head per batch and nothing else.
int eval_tables(explainn_ctx* c, const explainn_params* p, int B, hipStream_t s) {
    if (!(c->eval_valid && p->version != 0 && p->version == c->eval_version)) {
        TRY(launch_prep1_tables(c, p, s));
        TRY(launch_prep1(c, p, B, false, s));
        TRY(launch_prep2(c, p, B, false, s));
        c->eval_valid = true;
        c->eval_version = p->version;
    }
    return EXPLAINN_OK;
}

int eval_front(explainn_ctx* c, const float* x, int B, const explainn_params* p, hipStream_t s) {
    // every eval-mode entry point overwrites scratch a pending backward would read (codes, ext,
    // idx, z, bits ...): whatever train forward was in flight is gone, and its backward must fail
    // with E_STATE instead of returning the eval batch's gradients
    drop_pending(c);
    if (c->dense) {
        if (!x) { explainn_set_error("dense input mode needs x"); return EXPLAINN_E_ARG; }
        c->staged_B = 0;
    } else {
        TRY(launch_pack(c, x, B, false, s));
    }
    return eval_tables(c, p, B, s);
}

// The eval-mode forward of every entry point that runs the whole network: the dense or one-hot filter
// bank (want_idx: the pooling's argmax offsets are stored too), the FC, the head (logits and / or outs).
int eval_forward(explainn_ctx* c, const float* x, int B, const explainn_params* p, bool want_idx,
                 float* logits, float* outs, hipStream_t s) {
    TRY(eval_front(c, x, B, p, s));
    if (c->dense) TRY(launch_dense_conv_pool(c, x, p, B, s));
    else TRY(launch_conv_pool(c, p, B, want_idx, s));
    TRY(launch_fc_fwd(c, p, B, false, nullptr, 0.f, 0, s));
    return launch_head_fwd(c, p, B, false, logits, outs, s);
}
}  // namespace

// What the entry points that fold units through `final` in kernels of their own answer on a bank.
#define NOT_ON_BANK(c, what)                                                                        \
    do {                                                                                            \
        if ((c) && (c)->Gm > 1) {                                                                    \
            explainn_set_error(what " is not available on a model bank (%d members): run it on one " \
                               "member, ExplaiNNBank.member(g)", (c)->Gm);                           \
            return EXPLAINN_E_UNSUPPORTED;                                                          \
        }                                                                                           \
    } while (0)

// the largest unit count the kernels in front of the head are tested at (tests/test_gpu_properties.py
// and tests/test_gpu_bank.py: 2000 units); nothing larger has run, so nothing larger is accepted
#define BANK_MAX_UNITS 2000

static int create_ctx(explainn_ctx** out, int groups, int units_per_member, int kernel_size,
                      int sequence_length, int n_features, int max_batch, int device) {
    if (!out) { explainn_set_error("out is null"); return EXPLAINN_E_ARG; }
    *out = nullptr;
    if (groups < 1 || units_per_member < 1 || n_features < 1 || max_batch < 1) {
        explainn_set_error("%scnn_units, n_features and max_batch must be positive", groups < 1 ? "groups, " : "");
        return EXPLAINN_E_ARG;
    }
    if (groups > 1 && (int64_t)groups * units_per_member > BANK_MAX_UNITS) {
        explainn_set_error("a bank of %d x %d units exceeds the %d units a context supports", groups,
                           units_per_member, BANK_MAX_UNITS);
        return EXPLAINN_E_UNSUPPORTED;
    }
    const int cnn_units = groups * units_per_member;
    if (kernel_size < 2 || kernel_size > MAX_K) {
        explainn_set_error("kernel_size %d unsupported (2..%d)", kernel_size, MAX_K);
        return EXPLAINN_E_UNSUPPORTED;
    }
    const int Lo = sequence_length - kernel_size + 1;
    const int n = Lo / POOLW;
    if (n < 1) {
        explainn_set_error("sequence_length %d too short for kernel_size %d and MaxPool1d(7,7)",
                           sequence_length, kernel_size);
        return EXPLAINN_E_ARG;
    }
    const int NQ = nq_bucket(n);
    if (NQ == 0) {
        explainn_set_error("pooled length n=%d exceeds the largest instantiated kernel (%d)", n, MAX_NQ);
        return EXPLAINN_E_UNSUPPORTED;
    }
    HIP_TRY(hipSetDevice(device));                 // (nothing allocated yet)
    explainn_ctx* c = new explainn_ctx();
    memset(c, 0, sizeof(*c));
    c->Gm = groups; c->Um = units_per_member;
    c->U = cnn_units; c->k = kernel_size; c->L = sequence_length; c->T = n_features;
    c->maxB = max_batch; c->device = device;
    c->Lo = Lo; c->n = n; c->U4 = (cnn_units + 3) & ~3; c->Uq = c->U4 / 4;
    c->NQ = NQ; c->NS = ns_stride(NQ); c->K4 = 4 * kernel_size;
    // Batch stride of every [..][b] array: a multiple of 64 lanes, but an ODD multiple, so that the
    // row stride (4*Bs bytes) is never a multiple of 512 B: with Bs = 1024 every row of ext/dy/...
    // was exactly 4096 B apart and all rows of a wavefront (and of every unit) landed on the same
    // memory channel (channel camping: ~8 us per dependent load, profiles/r01_c).
    c->Bs = (max_batch + 63) & ~63;
    if (((c->Bs / 64) & 1) == 0) c->Bs += 64;
    // fc.hip has no device-side test of b < Bs: a 16-sequence tile that starts below B <= max_batch ends
    // below Bs because Bs is a multiple of 64 and not below max_batch (both by the two lines above)
    assert(c->Bs % 64 == 0 && c->Bs >= max_batch);
    // ... and it addresses a unit's [n][Bs] rows, dead rows of the bucket's last tile included, with 32-bit
    // byte offsets behind a range-checked descriptor
    if ((int64_t)(NQ + 32) * c->Bs * 4 > (int64_t)INT32_MAX) {
        explainn_set_error("max_batch %d: the rows of one unit (%d x %d floats) exceed 32-bit byte offsets",
                           max_batch, NQ + 32, c->Bs);
        delete c;
        return EXPLAINN_E_UNSUPPORTED;
    }
    c->NW = (sequence_length + 31) / 32 + 2; c->PW = 2 * c->NW;
    c->Lp = ((c->NW * 32 + 63) / 64) * 64;
    {
        int q = (max_batch + 127) / 128;
        const int64_t per = (int64_t)c->U * c->NS * c->NS * 4;
        const int cap = (int)((int64_t)(64 << 20) / (per > 0 ? per : 1));
        if (q > 8) q = 8;
        if (q > cap) q = cap;
        if (q < 1) q = 1;
        c->QCH = q;
        int a = (max_batch + 255) / 256;                 // passA: two 128-sequence waves per chunk (fc.hip)
        if (a > 16) a = 16;
        if (a < 1) a = 1;
        c->ACH = a;
        // tuning overrides (experiments only; defaults above are what is tested and benchmarked)
        if (const char* e = getenv("EXPLAINN_ACH")) { const int v = atoi(e); if (v >= 1 && v <= 16) c->ACH = v; }
        if (const char* e = getenv("EXPLAINN_QCH")) { const int v = atoi(e); if (v >= 1 && v <= cap && v <= 8) c->QCH = v; }
        // blocks per 64 sequences of the head sums' combiner launch (head.hip, launch_head_fwd_sums): 1 = one
        // block that does everything, R = the storing block and R - 1 unit groups; the launch clamps
        // it to [1, U + 1]
        c->head_groups = HEAD_GROUPS_DEFAULT;
        if (const char* e = getenv("EXPLAINN_HEAD_GROUPS")) c->head_groups = atoi(e);
    }
    Carver dry;
    carve(c, dry);
    c->bytes = dry.bytes();
    hipError_t e = hipMalloc(&c->base, c->bytes);
    if (e != hipSuccess) {
        explainn_set_error("hipMalloc(%lld bytes) failed: %s", (long long)c->bytes, hipGetErrorString(e));
        delete c;
        return EXPLAINN_E_HIP;
    }
    Carver real(c->base);
    carve(c, real);
    e = hipMemset(c->base, 0, c->bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        explainn_set_error("scratch memset failed: %s", hipGetErrorString(e));
        (void)hipFree(c->base);
        delete c;
        return EXPLAINN_E_HIP;
    }
    // from here on every failure releases what was acquired (explainn_destroy copes with the
    // members that are still null)
    int rc = [&]() -> int {
        TRY(prep_configure(c));
        TRY(bwd_configure(c));
        TRY(fc_configure(c));
        return EXPLAINN_OK;
    }();
    if (rc != EXPLAINN_OK) { explainn_destroy(c); return rc; }
    *out = c;
    return EXPLAINN_OK;
}

extern "C" int explainn_create(explainn_ctx** out, int cnn_units, int kernel_size,
                               int sequence_length, int n_features, int max_batch, int device) {
    return create_ctx(out, 1, cnn_units, kernel_size, sequence_length, n_features, max_batch, device);
}

extern "C" int explainn_create_bank(explainn_ctx** out, int groups, int cnn_units, int kernel_size,
                                    int sequence_length, int n_features, int max_batch, int device) {
    return create_ctx(out, groups, cnn_units, kernel_size, sequence_length, n_features, max_batch, device);
}

extern "C" int explainn_groups(const explainn_ctx* c) { return c ? c->Gm : 0; }

extern "C" void explainn_destroy(explainn_ctx* c) {
    if (!c) return;
    for (int i = 0; i < ST_COUNT; ++i) {
        if (c->ev0[i]) (void)hipEventDestroy(c->ev0[i]);
        if (c->ev1[i]) (void)hipEventDestroy(c->ev1[i]);
    }
    if (c->base) (void)hipFree(c->base);
    delete c;
}

extern "C" int64_t explainn_scratch_bytes(const explainn_ctx* c) { return c ? c->bytes : 0; }

extern "C" int explainn_forward_eval(explainn_ctx* c, const float* x, int B,
                                     const explainn_params* p, float* logits, void* stream) {
    TRY(check_batch(c, B));
    return eval_forward(c, x, B, p, false, logits, nullptr, static_cast<hipStream_t>(stream));
}

// Eval forward that keeps what the input gradient needs: the argmax offsets of the pooling (the
// forward above skips storing them) next to ext and o, which every eval forward keeps.  The logits are
// those of explainn_forward_eval, bit for bit: idx is an extra output of the same filter-bank pass.
extern "C" int explainn_forward_eval_keep(explainn_ctx* c, const float* x, int B,
                                          const explainn_params* p, float* logits, void* stream) {
    NOT_ON_BANK(c, "explainn_forward_eval_keep");
    TRY(check_batch(c, B));
    TRY(eval_forward(c, x, B, p, true, logits, nullptr, static_cast<hipStream_t>(stream)));
    c->keep_B = B;
    c->keep_x = c->dense ? x : nullptr;
    return EXPLAINN_OK;
}

extern "C" int explainn_input_grad(explainn_ctx* c, const float* dlogits, int B,
                                   const explainn_params* p, float* dx, void* stream) {
    NOT_ON_BANK(c, "explainn_input_grad");
    TRY(check_batch(c, B));
    if (!dlogits || !dx) { explainn_set_error("dlogits and dx are required"); return EXPLAINN_E_ARG; }
    if (c->keep_B != B) {
        explainn_set_error("input_grad(B=%d) without a matching forward_eval_keep (last B=%d)", B, c->keep_B);
        return EXPLAINN_E_STATE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(launch_ig_eval_dy(c, p, dlogits, B, s));
    return launch_input_grad(c, p, B, false, nullptr, dx, s);
}

extern "C" int64_t explainn_ism_workspace_bytes(const explainn_ctx* c, int B) {
    if (check_batch(c, B) != EXPLAINN_OK) return 0;
    return ism_workspace_bytes(c, B);
}

extern "C" int explainn_ism(explainn_ctx* c, const float* x, int B, const explainn_params* p,
                            float* logits, float* delta, void* workspace, int64_t workspace_bytes,
                            void* stream) {
    NOT_ON_BANK(c, "explainn_ism");
    TRY(check_batch(c, B));
    if (!logits || !delta || !workspace) {
        explainn_set_error("logits, delta and workspace are required");
        return EXPLAINN_E_ARG;
    }
    if (c->dense) { explainn_set_error("in-silico mutagenesis works on base codes: one-hot input only"); return EXPLAINN_E_UNSUPPORTED; }
    if (!workspace_ok("ism", workspace, workspace_bytes, ism_workspace_bytes(c, B), 1)) return EXPLAINN_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(eval_forward(c, x, B, p, false, logits, nullptr, s));
    return launch_ism(c, p, B, delta, static_cast<float*>(workspace), s);
}

extern "C" int64_t explainn_integrated_gradients_workspace_bytes(const explainn_ctx* c, int B) {
    if (check_batch(c, B) != EXPLAINN_OK) return 0;
    return pathgrad_workspace_bytes(c, B);
}

extern "C" int explainn_integrated_gradients(explainn_ctx* c, const float* x, int B, const explainn_params* p,
                                             int baseline_kind, const uint8_t* baseline_codes,
                                             const float* dlogits, int steps, float* ig, float* logits_x,
                                             float* logits_base, void* workspace, int64_t workspace_bytes,
                                             void* stream) {
    NOT_ON_BANK(c, "explainn_integrated_gradients");
    TRY(check_batch(c, B));
    if (!dlogits || !ig || !logits_x || !logits_base || !workspace) {
        explainn_set_error("dlogits, ig, logits_x, logits_base and workspace are required");
        return EXPLAINN_E_ARG;
    }
    if (steps < 1) { explainn_set_error("integrated gradients need steps >= 1 (got %d)", steps); return EXPLAINN_E_ARG; }
    if (baseline_kind != EXPLAINN_IG_BASELINE_ZERO && baseline_kind != EXPLAINN_IG_BASELINE_UNIFORM &&
        baseline_kind != EXPLAINN_IG_BASELINE_CODES) {
        explainn_set_error("unknown baseline kind %d", baseline_kind);
        return EXPLAINN_E_ARG;
    }
    if (baseline_kind == EXPLAINN_IG_BASELINE_CODES && !baseline_codes) {
        explainn_set_error("baseline kind `codes` needs baseline_codes");
        return EXPLAINN_E_ARG;
    }
    if (c->dense) { explainn_set_error("integrated gradients walk a path between base codes: one-hot input only"); return EXPLAINN_E_UNSUPPORTED; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = x ? 0 : c->staged_rc;
    TRY(eval_front(c, x, B, p, s));
    return launch_pathgrad(c, p, B, baseline_kind, baseline_codes, rc, dlogits, steps, ig, logits_x, logits_base,
                           workspace, workspace_bytes, s);
}

extern "C" int explainn_unit_outputs(explainn_ctx* c, const float* x, int B,
                                     const explainn_params* p, float* outs, void* stream) {
    TRY(check_batch(c, B));
    return eval_forward(c, x, B, p, false, nullptr, outs, static_cast<hipStream_t>(stream));
}

extern "C" int explainn_unit_activations(explainn_ctx* c, const float* x, int B,
                                         const explainn_params* p, float* acts, void* stream) {
    TRY(check_batch(c, B));
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(eval_front(c, x, B, p, s));
    if (c->dense) return launch_dense_conv_act(c, x, B, acts, s);
    TRY(launch_conv_act(c, B, acts, s));
    return EXPLAINN_OK;
}

namespace {
// What every explainn_stage_* entry point does once its own arguments have passed: the packed codes of
// a pending backward are overwritten, and the staged batch is of this strand (returned as 0 / 1).
int stage_begin(explainn_ctx* c, int reverse_complement) {
    drop_pending(c);
    c->staged_rc = reverse_complement ? 1 : 0;
    return c->staged_rc;
}
}  // namespace

extern "C" int explainn_stage_codes(explainn_ctx* c, const uint8_t* codes, int B,
                                    int reverse_complement, void* stream) {
    TRY(check_batch(c, B));
    if (!codes) { explainn_set_error("codes is null"); return EXPLAINN_E_ARG; }
    return launch_pack_codes(c, codes, B, stage_begin(c, reverse_complement), static_cast<hipStream_t>(stream));
}

extern "C" int explainn_stage_windows(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, int64_t start0,
                                      int64_t step, int B, int reverse_complement, void* stream) {
    TRY(check_batch(c, B));
    if (!seq || seq_len < 0) { explainn_set_error("seq is null or seq_len negative"); return EXPLAINN_E_ARG; }
    return launch_stage_windows(c, seq, seq_len, start0, step, B, stage_begin(c, reverse_complement),
                                static_cast<hipStream_t>(stream));
}

// AUTO takes the shared track where it is legal and was measured faster than staging every window, by
// more than the two legs' spreads (tools/scan_probe.py -> profiles/r11_scan_probe.json: MI355X, 10^6
// bases, both strands, 300 and 100 units x k 19 x L 200; DESIGN.md section 8 has the table).  SHARED
// won at stride 7, 14 and 49 on both shapes (300 units: 6.87 against 10.51 ms, 3.66 / 5.11, 1.37 / 1.51)
// and LOST at 98 and 203 (0.94 / 0.85, 0.72 / 0.52): past m = 7 the filter bank no longer dominates
// what a window costs and the track's extra launches and tile rounding do.
#define SCAN_AUTO_MAX_M 7             // the largest stride / 7 at which SHARED won
// the fewest windows per call at which SHARED was measured to win (20 405, at stride 49); nothing
// smaller was measured, so nothing smaller is sent there
#define SCAN_AUTO_MIN_WINDOWS 20000

namespace {
// the mode a call runs in (a negative code for a bad argument)
int scan_resolve_mode(const explainn_ctx* c, int64_t n_windows, int64_t stride, int mode) {
    if (!c) { explainn_set_error("null context"); return EXPLAINN_E_ARG; }
    if (n_windows < 1 || stride < 1 || stride > (int64_t)1 << 30) {
        explainn_set_error("scan needs n_windows >= 1 and 1 <= stride <= 2^30 (got %lld, %lld)",
                           (long long)n_windows, (long long)stride);
        return EXPLAINN_E_ARG;
    }
    if (mode == EXPLAINN_SCAN_AUTO) {
        const bool shared = stride % POOLW == 0 && stride / POOLW <= SCAN_AUTO_MAX_M &&
                            n_windows >= SCAN_AUTO_MIN_WINDOWS;
        return shared ? EXPLAINN_SCAN_SHARED : EXPLAINN_SCAN_WINDOWS;
    }
    if (mode == EXPLAINN_SCAN_WINDOWS) return mode;
    if (mode == EXPLAINN_SCAN_SHARED) {
        if (stride % POOLW != 0) {
            explainn_set_error("EXPLAINN_SCAN_SHARED needs a stride that is a multiple of %d (got %lld)", POOLW,
                               (long long)stride);
            return EXPLAINN_E_ARG;
        }
        return mode;
    }
    explainn_set_error("unknown scan mode %d", mode);
    return EXPLAINN_E_ARG;
}

int64_t scan_shared_bytes(const explainn_ctx* c, int64_t n_windows, int64_t stride) {
    const int64_t J = scan_tiles(c, n_windows, (int)(stride / POOLW));
    return (J + c->maxB - 1) / c->maxB * scan_track_block_elems(c) * (int64_t)sizeof(float);
}

// Rows the context stages itself, max_batch at a time: stage(i0, Bw) stages rows [i0, i0 + Bw), and
// their logits (n_rows, [G,] T) and unit outputs (n_rows, units), either may be null, land behind
// those of the rows before.  Nothing stays staged.
template <class Stage>
int score_rows(explainn_ctx* c, int64_t n_rows, const explainn_params* p, float* logits, float* outs,
               hipStream_t s, Stage stage) {
    const int64_t row = (int64_t)c->Gm * c->T;
    for (int64_t i0 = 0; i0 < n_rows; i0 += c->maxB) {
        const int Bw = (int)(n_rows - i0 < c->maxB ? n_rows - i0 : c->maxB);
        TRY(stage(i0, Bw));
        TRY(eval_forward(c, nullptr, Bw, p, false, logits ? logits + i0 * row : nullptr,
                         outs ? outs + i0 * c->U : nullptr, s));
    }
    c->staged_B = 0;
    return EXPLAINN_OK;
}
}  // namespace

extern "C" int64_t explainn_scan_workspace_bytes(const explainn_ctx* c, int64_t n_windows, int64_t stride,
                                                 int mode) {
    const int m = scan_resolve_mode(c, n_windows, stride, mode);
    if (m < 0) return m;
    return m == EXPLAINN_SCAN_SHARED ? scan_shared_bytes(c, n_windows, stride) : 0;
}

extern "C" int explainn_scan(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, int64_t start,
                             int64_t n_windows, int64_t stride, int reverse_complement,
                             const explainn_params* p, float* logits, int mode, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    const int md = scan_resolve_mode(c, n_windows, stride, mode);
    if (md < 0) return md;
    if (!seq || seq_len < 0 || !p || !logits) {
        explainn_set_error("seq, params and logits are required, seq_len >= 0");
        return EXPLAINN_E_ARG;
    }
    if (c->dense) { explainn_set_error("a scan works on base codes: not in dense input mode"); return EXPLAINN_E_UNSUPPORTED; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int rc = reverse_complement ? 1 : 0;
    const int64_t row = (int64_t)c->Gm * c->T;       // logits are (n_windows, [G,] T)
    drop_pending(c);
    if (md == EXPLAINN_SCAN_WINDOWS)
        return score_rows(c, n_windows, p, logits, nullptr, s, [&](int64_t i0, int Bw) {
            return launch_stage_windows(c, seq, seq_len, start + i0 * stride, stride, Bw, rc, s);
        });
    if (!workspace_ok("scan", workspace, workspace_bytes, scan_shared_bytes(c, n_windows, stride), 256))
        return EXPLAINN_E_ARG;
    // the pooled track: tiles of L bases placed 7n apart, through the filter bank in blocks of up to
    // max_batch tiles.  Each block is the filter bank's whole output array, so the filter bank writes
    // it straight into the workspace (its output pointer is swapped for the launch): no copy.
    const int m = (int)(stride / POOLW), TB = c->maxB;
    const int64_t tstep = (int64_t)POOLW * c->n, J = scan_tiles(c, n_windows, m);
    const int64_t blk = scan_track_block_elems(c), Leff = stride * (n_windows - 1) + c->L;
    float* track = static_cast<float*>(workspace);
    float* const own_ext = c->ext;
    for (int64_t j0 = 0; j0 < J; j0 += TB) {
        const int Bt = (int)(J - j0 < TB ? J - j0 : TB);
        // reverse strand: rc(window i) is forward window n_windows-1-i of rc(seq[start : start+Leff]),
        // whose tile j starts L + 7n*j bases before the region's end
        const int64_t s0 = rc ? start + Leff - c->L - tstep * j0 : start + tstep * j0;
        TRY(launch_stage_windows(c, seq, seq_len, s0, rc ? -tstep : tstep, Bt, rc, s));
        if (j0 == 0) TRY(eval_front(c, nullptr, Bt, p, s));
        c->ext = track + (j0 / TB) * blk;
        const int r = launch_conv_pool(c, p, Bt, false, s);
        c->ext = own_ext;
        TRY(r);
    }
    for (int64_t i0 = 0; i0 < n_windows; i0 += c->maxB) {
        const int Bw = (int)(n_windows - i0 < c->maxB ? n_windows - i0 : c->maxB);
        TRY(launch_scan_unfold(c, track, blk, J, TB, m, n_windows, i0, Bw, rc, s));
        TRY(launch_fc_fwd(c, p, Bw, false, nullptr, 0.f, 0, s));
        TRY(launch_head_fwd(c, p, Bw, false, logits + i0 * row, nullptr, s));
    }
    c->staged_B = 0;
    return EXPLAINN_OK;
}

namespace {
// What can be checked of these tables without reading them (their arrays live on the device).  The
// edit-table half, which explainn_edits and explainn_haplotypes share field by field, once the counts
// have passed:
template <class Tables>
int check_edit_table(const Tables* t) {
    if (t->n_edits > 0 && (!t->pos || !t->ref_len || !t->alt_len || !t->alt_off)) {
        explainn_set_error("an edit table of %lld edits needs pos, ref_len, alt_len and alt_off", (long long)t->n_edits);
        return EXPLAINN_E_ARG;
    }
    if (t->alt_bytes > 0 && !t->alt) { explainn_set_error("alt is null but alt_bytes is %lld", (long long)t->alt_bytes); return EXPLAINN_E_ARG; }
    return EXPLAINN_OK;
}

int check_edits(const uint8_t* seq, int64_t seq_len, const explainn_edits* ed, int64_t row0) {
    if (!seq || seq_len < 0) { explainn_set_error("seq is null or seq_len negative"); return EXPLAINN_E_ARG; }
    if (!ed || !ed->row_start || !ed->row_edit || row0 < 0) {
        explainn_set_error("edits, its row_start and row_edit are required, row0 >= 0");
        return EXPLAINN_E_ARG;
    }
    if (ed->n_edits < 0 || ed->alt_bytes < 0 || ed->alt_bytes >= (int64_t)1 << 31) {
        explainn_set_error("edits needs n_edits >= 0 and 0 <= alt_bytes < 2^31 (got %lld, %lld)",
                           (long long)ed->n_edits, (long long)ed->alt_bytes);
        return EXPLAINN_E_ARG;
    }
    return check_edit_table(ed);
}

int check_haplotypes(const uint8_t* seq, int64_t seq_len, const explainn_haplotypes* hp, int64_t row0) {
    if (!seq || seq_len < 0) { explainn_set_error("seq is null or seq_len negative"); return EXPLAINN_E_ARG; }
    if (!hp || !hp->row_start || !hp->row_first || !hp->row_count || row0 < 0) {
        explainn_set_error("haplotypes, its row_start, row_first and row_count are required, row0 >= 0");
        return EXPLAINN_E_ARG;
    }
    if (hp->n_index < 0 || hp->n_edits < 0 || hp->alt_bytes < 0 || hp->alt_bytes >= (int64_t)1 << 31) {
        explainn_set_error("haplotypes needs n_index >= 0, n_edits >= 0 and 0 <= alt_bytes < 2^31 (got %lld, %lld, %lld)",
                           (long long)hp->n_index, (long long)hp->n_edits, (long long)hp->alt_bytes);
        return EXPLAINN_E_ARG;
    }
    if (hp->n_index > 0 && !hp->edit_index) {
        explainn_set_error("edit_index is null but n_index is %lld", (long long)hp->n_index);
        return EXPLAINN_E_ARG;
    }
    return check_edit_table(hp);
}

// The front of explainn_score_edits / explainn_score_haplotypes (`name`), whose rows are `scored`
// on base codes; check() is check_edits / check_haplotypes of the call's tables.
template <class Check>
int score_rows_begin(explainn_ctx* c, const char* name, const char* scored, int64_t n_rows,
                     const explainn_params* p, const float* logits, const float* outs, Check check) {
    if (!c) { explainn_set_error("null context"); return EXPLAINN_E_ARG; }
    if (n_rows < 1 || !p) { explainn_set_error("%s needs n_rows >= 1 and params", name); return EXPLAINN_E_ARG; }
    if (!logits && !outs) { explainn_set_error("%s needs logits or outs (both are null)", name); return EXPLAINN_E_ARG; }
    TRY(check());
    if (c->dense) { explainn_set_error("%s are scored on base codes: not in dense input mode", scored); return EXPLAINN_E_UNSUPPORTED; }
    drop_pending(c);
    return EXPLAINN_OK;
}
}  // namespace

extern "C" int explainn_stage_edited_windows(explainn_ctx* c, const uint8_t* seq, int64_t seq_len,
                                             const explainn_edits* edits, int64_t row0, int B,
                                             int reverse_complement, void* stream) {
    TRY(check_batch(c, B));
    TRY(check_edits(seq, seq_len, edits, row0));
    return launch_stage_edits(c, seq, seq_len, edits, row0, B, stage_begin(c, reverse_complement),
                              static_cast<hipStream_t>(stream));
}

extern "C" int explainn_score_edits(explainn_ctx* c, const uint8_t* seq, int64_t seq_len,
                                    const explainn_edits* edits, int64_t n_rows, int reverse_complement,
                                    const explainn_params* p, float* logits, float* outs, void* stream) {
    TRY(score_rows_begin(c, "score_edits", "edits", n_rows, p, logits, outs,
                         [&] { return check_edits(seq, seq_len, edits, 0); }));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return score_rows(c, n_rows, p, logits, outs, s, [&](int64_t i0, int Bw) {
        return launch_stage_edits(c, seq, seq_len, edits, i0, Bw, reverse_complement ? 1 : 0, s);
    });
}

extern "C" int explainn_stage_haplotype_windows(explainn_ctx* c, const uint8_t* seq, int64_t seq_len,
                                                const explainn_haplotypes* haps, int64_t row0, int B,
                                                int reverse_complement, void* stream) {
    TRY(check_batch(c, B));
    TRY(check_haplotypes(seq, seq_len, haps, row0));
    return launch_stage_haplotypes(c, seq, seq_len, haps, row0, B, stage_begin(c, reverse_complement),
                                   static_cast<hipStream_t>(stream));
}

extern "C" int explainn_score_haplotypes(explainn_ctx* c, const uint8_t* seq, int64_t seq_len,
                                         const explainn_haplotypes* haps, int64_t n_rows, int reverse_complement,
                                         const explainn_params* p, float* logits, float* outs, void* stream) {
    TRY(score_rows_begin(c, "score_haplotypes", "haplotypes", n_rows, p, logits, outs,
                         [&] { return check_haplotypes(seq, seq_len, haps, 0); }));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return score_rows(c, n_rows, p, logits, outs, s, [&](int64_t i0, int Bw) {
        return launch_stage_haplotypes(c, seq, seq_len, haps, i0, Bw, reverse_complement ? 1 : 0, s);
    });
}

extern "C" int64_t explainn_call_sites_workspace_bytes(const explainn_ctx* c, int64_t n_positions) {
    if (!c || n_positions < 0 || n_positions + c->k >= (int64_t)1 << 31) return 0;
    return sites_workspace_bytes(c, n_positions);
}

namespace {
// The range of start positions call_sites and activation_histogram take of a raw code sequence: every
// k-mer of [start, start + n_positions) lies inside the sequence, and a position fits an int.
int check_code_range(const char* what, const explainn_ctx* c, int64_t seq_len, int64_t start, int64_t n_positions) {
    if (!c) { explainn_set_error("null context"); return EXPLAINN_E_ARG; }
    if (start < 0 || n_positions < 0 || n_positions + c->k >= (int64_t)1 << 31 ||
        seq_len - start < n_positions + c->k - 1) {
        explainn_set_error("%s needs 0 <= start, start + n_positions + k - 1 <= seq_len and "
                           "n_positions + k < 2^31 (start %lld, n_positions %lld, k %d, seq_len %lld)", what,
                           (long long)start, (long long)n_positions, c->k, (long long)seq_len);
        return EXPLAINN_E_ARG;
    }
    return EXPLAINN_OK;
}

// What an entry point that reads a raw code sequence with the eval-mode tables does once its own
// arguments have passed: `what` are done "on base codes", so not in dense input mode; nothing is staged
// by such a call and what was staged (or pending) is not kept; the folded tables are current.
int code_scan_begin(explainn_ctx* c, const explainn_params* p, const char* what, hipStream_t s) {
    if (!c) { explainn_set_error("null context"); return EXPLAINN_E_ARG; }
    if (c->dense) { explainn_set_error("%s on base codes: not in dense input mode", what); return EXPLAINN_E_UNSUPPORTED; }
    drop_pending(c);
    c->staged_B = 0;
    return eval_tables(c, p, 1, s);
}
}  // namespace

extern "C" int explainn_call_sites(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, int64_t start,
                                   int64_t n_positions, int64_t period, int reverse_complement,
                                   const explainn_params* p, const float* thresholds, int64_t* offsets,
                                   int32_t* pos, float* score, int64_t capacity, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
    if (!seq || !p || !thresholds || !offsets) {
        explainn_set_error("seq, params, thresholds and offsets are required");
        return EXPLAINN_E_ARG;
    }
    TRY(check_code_range("call_sites", c, seq_len, start, n_positions));
    if (period < 0 || capacity < 0) { explainn_set_error("period and capacity must not be negative"); return EXPLAINN_E_ARG; }
    if (!sites_workspace_ok(c, n_positions, workspace, workspace_bytes)) return EXPLAINN_E_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(code_scan_begin(c, p, "sites are called", s));
    return launch_call_sites(c, seq, start, n_positions, period, reverse_complement ? 1 : 0, thresholds,
                             offsets, pos, score, capacity, workspace, s);
}

extern "C" int explainn_activation_histogram(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, int64_t start,
                                             int64_t n_positions, int64_t period, int reverse_complement,
                                             const explainn_params* p, uint64_t* hist, void* stream) {
    if (!seq || !p || !hist) { explainn_set_error("seq, params and hist are required"); return EXPLAINN_E_ARG; }
    TRY(check_code_range("activation_histogram", c, seq_len, start, n_positions));
    if (period < 0) { explainn_set_error("period must not be negative"); return EXPLAINN_E_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(code_scan_begin(c, p, "activations are counted", s));
    if (n_positions == 0) return EXPLAINN_OK;
    return launch_activation_histogram(c, seq, start, n_positions, period, reverse_complement ? 1 : 0, hist, s);
}

extern "C" int explainn_record_best(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets,
                                    int64_t n_records, int strands, const explainn_params* p, uint16_t* best_bits,
                                    int32_t* best_site, void* stream) {
    if (!seq || !p || !rec_offsets || !best_bits) {
        explainn_set_error("seq, rec_offsets, params and best_bits are required");
        return EXPLAINN_E_ARG;
    }
    if (seq_len < 0 || n_records < 0 || n_records >= (int64_t)1 << 31 || (strands != 1 && strands != 2)) {
        explainn_set_error("record_best needs seq_len >= 0, 0 <= n_records < 2^31 and strands 1 or 2 "
                           "(seq_len %lld, n_records %lld, strands %d)", (long long)seq_len, (long long)n_records,
                           strands);
        return EXPLAINN_E_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(code_scan_begin(c, p, "best sites are found", s));
    if (n_records == 0) return EXPLAINN_OK;
    return launch_record_best(c, seq, seq_len, rec_offsets, n_records, strands, best_bits, best_site, s);
}

// the checks the two spacing entry points share: the unit sets' sizes and the distance
static int check_spacing(const char* what, int A, int P, int max_distance) {
    if (A < 0 || P < 0 || A > 65535) {
        explainn_set_error("%s: need 0 <= A <= 65535 anchors and P >= 0 partners (A=%d P=%d)", what, A, P);
        return EXPLAINN_E_ARG;
    }
    if (max_distance < 0 || max_distance > EXPLAINN_SPACING_MAX_DISTANCE) {
        explainn_set_error("%s: max_distance must be in [0, %d] (got %d)", what, EXPLAINN_SPACING_MAX_DISTANCE,
                           max_distance);
        return EXPLAINN_E_ARG;
    }
    return EXPLAINN_OK;
}

extern "C" int explainn_site_spacing(const int64_t* pos, const int64_t* offsets2, int U, const int32_t* anchors,
                                     int A, const int32_t* partners, int P, int max_distance, int64_t* hist,
                                     void* stream) {
    TRY(check_spacing("site_spacing", A, P, max_distance));
    if (U < 0 || (!anchors && A != U) || (!partners && P != U)) {
        explainn_set_error("site_spacing: a null unit set means all %d units (A=%d P=%d)", U, A, P);
        return EXPLAINN_E_ARG;
    }
    if (A == 0 || P == 0) return EXPLAINN_OK;
    if (!pos || !offsets2 || !hist) {
        explainn_set_error("site_spacing: pos, offsets2 and hist must be device pointers");
        return EXPLAINN_E_ARG;
    }
    return launch_site_spacing(pos, offsets2, U, anchors, A, partners, P, max_distance, hist,
                               static_cast<hipStream_t>(stream));
}

extern "C" int explainn_spacing_test(const int64_t* hist, int A, int P, const int32_t* anchors,
                                     const int32_t* partners, int max_distance, int min_distance, int64_t min_count,
                                     int64_t* total, int32_t* best_distance, int64_t* best_count, double* pvalue,
                                     void* stream) {
    TRY(check_spacing("spacing_test", A, P, max_distance));
    if (min_distance < 0 || min_count < 0) {
        explainn_set_error("spacing_test: min_distance and min_count must not be negative (%d, %lld)", min_distance,
                           (long long)min_count);
        return EXPLAINN_E_ARG;
    }
    if (A == 0 || P == 0) return EXPLAINN_OK;
    if (!hist || !total || !best_distance || !best_count || !pvalue) {
        explainn_set_error("spacing_test: hist and the four outputs must be device pointers");
        return EXPLAINN_E_ARG;
    }
    return launch_spacing_test(hist, A, P, anchors, partners, max_distance, min_distance, min_count, total,
                               best_distance, best_count, pvalue, static_cast<hipStream_t>(stream));
}

// the checks the two centrality entry points share: the histogram's shape
static int check_centrality(const char* what, int units, int T, int M) {
    if (units < 0 || T < 1 || T > EXPLAINN_CENTRALITY_MAX_THRESHOLDS || M < 1 ||
        (int64_t)T * 2 * M * (int64_t)sizeof(int32_t) > 64 * 1024) {
        explainn_set_error("%s: need units >= 0, 1 <= T <= %d thresholds, M >= 1 starts and a [T][2][M] int32 "
                           "histogram of at most 64 KiB (units=%d T=%d M=%d): split the thresholds", what,
                           EXPLAINN_CENTRALITY_MAX_THRESHOLDS, units, T, M);
        return EXPLAINN_E_ARG;
    }
    return EXPLAINN_OK;
}

extern "C" int explainn_site_positions(const uint16_t* best_bits, const int32_t* best_site, const uint8_t* labels,
                                       const float* thresholds, int units, int64_t n_records, int T, int M,
                                       int32_t* hist, int64_t* counts, void* stream) {
    TRY(check_centrality("site_positions", units, T, M));
    if (n_records < 0 || n_records >= (int64_t)1 << 31) {
        explainn_set_error("site_positions: need 0 <= n_records < 2^31 (got %lld)", (long long)n_records);
        return EXPLAINN_E_ARG;
    }
    if (!counts) { explainn_set_error("site_positions: counts must be a device pointer"); return EXPLAINN_E_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s));
    if (units == 0 || n_records == 0) return EXPLAINN_OK;
    if (!best_bits || !best_site || !labels || !thresholds || !hist) {
        explainn_set_error("site_positions: best_bits, best_site, labels, thresholds and hist must be device pointers");
        return EXPLAINN_E_ARG;
    }
    return launch_site_positions(best_bits, best_site, labels, thresholds, units, n_records, T, M, hist, counts, s);
}

extern "C" int explainn_centrality_test(const int32_t* hist, const int64_t* counts, int units, int T, int M, int mode,
                                        int min_width, int max_width, int64_t min_sites, int32_t* best_t,
                                        int32_t* best_lo, int32_t* best_width, int64_t* sites, int64_t* count,
                                        int64_t* n_tests, double* log_pvalue, double* log_padj, int64_t* ctrl_sites,
                                        int64_t* ctrl_count, double* log_fisher, void* stream) {
    TRY(check_centrality("centrality_test", units, T, M));
    if ((mode != 0 && mode != 1) || min_width < 1 || max_width < min_width || min_sites < 0) {
        explainn_set_error("centrality_test: need mode 0 (centred) or 1 (local), 1 <= min_width <= max_width and "
                           "min_sites >= 0 (mode=%d min_width=%d max_width=%d min_sites=%lld)", mode, min_width,
                           max_width, (long long)min_sites);
        return EXPLAINN_E_ARG;
    }
    int j0, w0;
    int64_t items;
    const int64_t regions = centrality_regions(M, mode, min_width, max_width, &j0, &w0, &items);
    if (regions > EXPLAINN_CENTRALITY_MAX_REGIONS) {
        explainn_set_error("centrality_test: %lld regions per unit, %d at the most: narrow max_width (M=%d "
                           "min_width=%d max_width=%d)", (long long)regions, EXPLAINN_CENTRALITY_MAX_REGIONS, M,
                           min_width, max_width);
        return EXPLAINN_E_ARG;
    }
    if (units == 0) return EXPLAINN_OK;
    if (!hist || !counts || !best_t || !best_lo || !best_width || !sites || !count || !n_tests || !log_pvalue ||
        !log_padj || !ctrl_sites || !ctrl_count || !log_fisher) {
        explainn_set_error("centrality_test: hist, counts and the eleven outputs must be device pointers");
        return EXPLAINN_E_ARG;
    }
    return launch_centrality_test(hist, counts, units, T, M, mode, j0, w0, items, regions, min_sites, best_t, best_lo,
                                  best_width, sites, count, n_tests, log_pvalue, log_padj, ctrl_sites, ctrl_count,
                                  log_fisher, static_cast<hipStream_t>(stream));
}

extern "C" int explainn_filter_act_max(explainn_ctx* c, const float* x, int B,
                                       const explainn_params* p, const uint8_t* select,
                                       float* unit_max, void* stream) {
    TRY(check_batch(c, B));
    if (!unit_max) { explainn_set_error("unit_max is null"); return EXPLAINN_E_ARG; }
    if (c->dense) { explainn_set_error("the filter export works on base codes: one-hot input only"); return EXPLAINN_E_UNSUPPORTED; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(eval_front(c, x, B, p, s));
    return launch_filter_act_max(c, B, select, unit_max, s);
}

extern "C" int explainn_filter_sites(explainn_ctx* c, const float* x, int B, const explainn_params* p,
                                     const uint8_t* select, const float* thresholds, int site_cap,
                                     int32_t* site_total, int32_t* pfm, uint8_t* hit, void* stream) {
    TRY(check_batch(c, B));
    if (!thresholds || !site_total || !pfm) {
        explainn_set_error("thresholds, site_total and pfm are required");
        return EXPLAINN_E_ARG;
    }
    if (site_cap <= 0) { explainn_set_error("site_cap must be positive"); return EXPLAINN_E_ARG; }
    if (c->dense) { explainn_set_error("the filter export works on base codes: one-hot input only"); return EXPLAINN_E_UNSUPPORTED; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    TRY(eval_front(c, x, B, p, s));
    return launch_filter_sites(c, B, select, thresholds, site_cap, site_total, pfm, hit, s);
}

namespace {
// the train forward; head_sums: the combiner launch also leaves the head backward's batch sums of a
// training step with targets sums_y (head_sums_in_combiner below decides, nobody else)
int forward_train(explainn_ctx* c, const float* x, int B, const explainn_params* p,
                  const uint8_t* keep_mask, float dropout_p, uint64_t seed, float* logits,
                  bool head_sums, const float* sums_y, int loss_kind, void* stream) {
    TRY(check_batch(c, B));
    if (B == 1) {
        // torch raises here (BatchNorm over one value); the reason for train.py:297-302
        explainn_set_error("Expected more than 1 value per channel when training, got input size "
                           "[1, %d, 1]", FC_H * c->U);
        return EXPLAINN_E_BATCH1;
    }
    if (dropout_p < 0.f || dropout_p >= 1.f) {
        explainn_set_error("dropout_p must be in [0,1)");
        return EXPLAINN_E_ARG;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    c->fwd_B = 0; c->keep_B = 0; c->sync_next = 0;   // (not tail_B: train_step_front clears it, train_step_fc sets it)
    c->eval_valid = false;             // the train-mode folds overwrite the eval-mode tables
    // the one-hot batch is packed and the filter tables are built by one launch; a staged batch of
    // base codes (x == NULL) is already packed and only needs the tables
    c->dense_x = nullptr;
    if (c->dense) {
        // soft input: no codes to pack; the stages that touch x take the dense kernels (dense.hip)
        if (!x) { explainn_set_error("dense input mode needs x"); return EXPLAINN_E_ARG; }
        c->staged_B = 0;
        STAGE(ST_PACK, launch_prep1_tables(c, p, s));
        STAGE(ST_MOMENTS, launch_dense_moments(c, x, B, s));
        STAGE(ST_PREP1, launch_prep1(c, p, B, true, s));
        STAGE(ST_CONV_POOL, launch_dense_conv_pool(c, x, p, B, s));
        c->dense_x = x;
    } else {
    if (x) STAGE(ST_PACK, launch_pack_tables(c, x, p, B, s));
    else {
        TRY(launch_pack(c, x, B, false, s));
        STAGE(ST_PACK, launch_prep1_tables(c, p, s));
    }
    // input moments (bit masks -> Gram -> BatchNorm1 fold) and the filter bank.  The filter bank reads
    // none of the statistics, and at one wave per SIMD it leaves SIMDs idle: the moment chain runs
    // inside its launch, on workgroups of its own (convpool.hip, cpm_bn1).  (Round 1 forked the chain
    // onto a side stream instead; the filter bank of that time filled every wave slot and the two
    // stretched each other.)  Grids too small to hide the chain keep the separate launches.
    if (const int naux = conv_pool_bn1_workgroups(c, B)) {
        STAGE(ST_CONV_POOL, launch_conv_pool_train(c, p, B, naux, s));
    } else {
        STAGE(ST_MOMENTS, launch_moments(c, B, s));
        STAGE(ST_PREP1, launch_prep1(c, p, B, true, s));
        STAGE(ST_CONV_POOL, launch_conv_pool(c, p, B, true, s));
    }
    }
    STAGE(ST_QMOM, launch_qmoments(c, B, s));
    STAGE(ST_PREP2, launch_prep2(c, p, B, true, s));
    STAGE(ST_FC_FWD, launch_fc_fwd(c, p, B, true, keep_mask, dropout_p, seed, s));
    if (head_sums) STAGE(ST_HEAD_FWD, launch_head_fwd_sums(c, p, B, logits, sums_y, loss_kind, s));
    else STAGE(ST_HEAD_FWD, launch_head_fwd(c, p, B, true, logits, nullptr, s));
    c->fwd_B = B;
    return EXPLAINN_OK;
}
}  // namespace

extern "C" int explainn_forward_train(explainn_ctx* c, const float* x, int B,
                                      const explainn_params* p, const uint8_t* keep_mask,
                                      float dropout_p, uint64_t seed, float* logits, void* stream) {
    return forward_train(c, x, B, p, keep_mask, dropout_p, seed, logits, false, nullptr, 0, stream);
}

namespace {
// the backward after the head, in the two halves a data-parallel run overlaps its all-reduce with:
// after backward_fc every gradient from fc1_w to final_b (the tail of explainn_grads) is final;
// backward_conv then produces conv_w, conv_b, bn1_w, bn1_b
int backward_fc(explainn_ctx* c, int B, const explainn_params* p, const explainn_grads* g,
                const pa_head_args* head, hipStream_t s) {
    STAGE(ST_PASSA, launch_passA(c, B, head, s));
    STAGE(ST_MID, launch_mid_bwd(c, p, g, B, s));
    return EXPLAINN_OK;
}

int backward_conv(explainn_ctx* c, int B, const explainn_params* p, const explainn_grads* g,
                  int freeze_top_n_filters, hipStream_t s) {
    STAGE(ST_PASSB, launch_passB(c, B, s));
    if (c->dense_x) STAGE(ST_CONV_BWD, launch_dense_conv_bwd(c, c->dense_x, B, s));
    else STAGE(ST_CONV_BWD, launch_conv_bwd(c, B, s));
    STAGE(ST_FIN, launch_fin_bwd(c, p, g, B, freeze_top_n_filters, s));
    return EXPLAINN_OK;
}

// Few tasks and a small batch: the head backward runs inside passA (fc.hip; mode 1 = dlogits given,
// 2 = from the loss).  Every passA wave then makes the full-batch pass of BatchNorm3's backward
// itself: worth a launch (~5 us) up to a few hundred sequences -- 0.120 -> 0.115 ms per step at 100
// units x 64 sequences -- and a wash at 1024 (passA +9.6 us, head_bwd -9.6 us; MI355X), so larger
// batches keep the per-unit kernel, or in the training step take head_sums_in_combiner below.
// A bank never rides: passA's prologue has no member index ("Model bank").
bool head_rides_in_passA(const explainn_ctx* c, int B) {
    if (c->Gm > 1) return false;
    return c->T <= PA_HEAD_MAX_T && B <= 512;
}

// Few tasks and a LARGER batch: the head backward's two batch sums per unit are formed where the
// data already sits in registers -- the combiner launch of the forward (head.hip, logits_bn_kernel<T>:
// per block of 64 sequences, partials) -- and passA adds the partials up and forms dz in its main loop
// (fc.hip, HEAD == 2): the per-unit head backward launch (9.3 us at 300 units x 1024 sequences) goes.
// Only the training step can take it (the combiner needs the targets); a bank, sync-BN, caller-given
// dlogits, T > PA_HEAD_MAX_T and batches that ride in passA keep their routes.
// EXPLAINN_HEAD_PARTIALS=0|1 (read per step, so that one process can run both) forces the per-unit
// kernel / this route wherever it is legal.  Default: on for one task -- measured at 300 x 1024,
// 100 x 1024 and 300 x 2048.  Two to four tasks were measured faster at
// 300 x 1024 only, and their kernels spill registers in some pooled-length buckets: off unless asked for.
bool head_sums_in_combiner(const explainn_ctx* c, int B, const float* logits, const float* targets) {
    if (c->Gm > 1 || c->T > PA_HEAD_MAX_T || c->T > HEAD_GEMM_MIN_T || !logits || !targets || B < 2) return false;
    if (head_rides_in_passA(c, B) || !head_sums_fit(c)) return false;
    if (const char* e = getenv("EXPLAINN_HEAD_PARTIALS")) return atoi(e) != 0;
    return c->T == 1;
}

pa_head_args head_in_passA(explainn_ctx* c, const explainn_params* p, const explainn_grads* g, int mode,
                           const float* dl, int kind, const float* logits, const float* y,
                           float* loss_out) {
    pa_head_args h = {mode, c->T, kind, dl, logits, y, loss_out, p->final_w, p->bn3_w, c->o, c->zhat,
                      c->sig3, c->dz, g->final_w, g->final_b, g->bn3_w, g->bn3_b, g->fc2_b};
    return h;
}

int backward_tail(explainn_ctx* c, int B, const explainn_params* p, const explainn_grads* g,
                  int freeze_top_n_filters, const pa_head_args* head, hipStream_t s) {
    TRY(backward_fc(c, B, p, g, head, s));
    return backward_conv(c, B, p, g, freeze_top_n_filters, s);
}
}  // namespace

extern "C" int explainn_backward(explainn_ctx* c, const float* dlogits, int B,
                                 const explainn_params* p, const explainn_grads* g,
                                 int freeze_top_n_filters, void* stream) {
    TRY(check_batch(c, B));
    if (c->fwd_B != B) {
        explainn_set_error("backward(B=%d) without a matching train-mode forward (last B=%d)", B,
                           c->fwd_B);
        return EXPLAINN_E_STATE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (head_rides_in_passA(c, B)) {
        const pa_head_args h = head_in_passA(c, p, g, 1, dlogits, 0, nullptr, nullptr, nullptr);
        return backward_tail(c, B, p, g, freeze_top_n_filters, &h, s);
    }
    STAGE(ST_HEAD_BWD, launch_head_bwd(c, p, g, dlogits, B, s));
    return backward_tail(c, B, p, g, freeze_top_n_filters, nullptr, s);
}

extern "C" int explainn_backward_input(explainn_ctx* c, const float* dlogits, int B,
                                       const explainn_params* p, const explainn_grads* g,
                                       int freeze_top_n_filters, float* dx, void* stream) {
    NOT_ON_BANK(c, "explainn_backward_input");
    if (!dx) { explainn_set_error("dx is null"); return EXPLAINN_E_ARG; }
    TRY(explainn_backward(c, dlogits, B, p, g, freeze_top_n_filters, stream));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // passB left dy and the partial sums S1, S2; the BatchNorm1 statistics are those of the forward
    TRY(launch_ig_tables(c, p, B, s));
    return launch_input_grad(c, p, B, true, c->dense_x, dx, s);
}

extern "C" int explainn_loss_grad(explainn_ctx* c, int loss_kind, const float* logits,
                                  const float* targets, int B, float* loss_out, float* dlogits,
                                  void* stream) {
    TRY(check_batch(c, B));
    if (loss_kind != EXPLAINN_LOSS_BCE_WITH_LOGITS && loss_kind != EXPLAINN_LOSS_MSE) {
        explainn_set_error("unknown loss kind %d", loss_kind);
        return EXPLAINN_E_ARG;
    }
    return launch_loss(c, loss_kind, logits, targets, B, loss_out, dlogits,
                       static_cast<hipStream_t>(stream));
}

namespace {
int train_step_front(explainn_ctx* c, const float* x, const float* targets, int B,
                     const explainn_params* p, const explainn_grads* g, int loss_kind,
                     float dropout_p, uint64_t seed, float* logits, float* loss_out, void* stream) {
    if (loss_kind != EXPLAINN_LOSS_BCE_WITH_LOGITS && loss_kind != EXPLAINN_LOSS_MSE) {
        explainn_set_error("unknown loss kind %d", loss_kind);
        return EXPLAINN_E_ARG;
    }
    if (c) c->tail_B = 0;
    TRY(check_batch(c, B));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (head_sums_in_combiner(c, B, logits, targets)) {
        // few tasks, batch > 512: loss gradient and batch-sum partials ride in the combiner launch of
        // the forward, passA finishes them -- no head backward launch
        TRY(forward_train(c, x, B, p, nullptr, dropout_p, seed, logits, true, targets, loss_kind, stream));
        const pa_sums_args ps = {c->zhat, c->dlogits, c->dz, p->final_w, p->bn3_w, p->bn3_b, c->sig3,
                                 c->T, (B + 63) / 64, c->hp, c->hb,
                                 g->final_w, g->final_b, g->bn3_w, g->bn3_b, g->fc2_b, loss_out};
        STAGE(ST_PASSA, launch_passA_sums(c, B, ps, s));
        STAGE(ST_MID, launch_mid_bwd(c, p, g, B, s));
        return EXPLAINN_OK;
    }
    TRY(explainn_forward_train(c, x, B, p, nullptr, dropout_p, seed, logits, stream));
    if (head_rides_in_passA(c, B)) {
        // few tasks, small batch: loss, loss gradient and head backward all ride in passA's prologue
        const pa_head_args h = head_in_passA(c, p, g, 2, nullptr, loss_kind, logits, targets, loss_out);
        return backward_fc(c, B, p, g, &h, s);
    }
    if (c->T <= 4) {
        // few tasks: the loss gradient is recomputed inside the head backward (one launch less)
        STAGE(ST_HEAD_BWD, launch_head_bwd_fused_loss(c, p, g, loss_kind, logits, targets, loss_out, B, s));
    } else {
        STAGE(ST_LOSS, launch_loss_deferred(c, loss_kind, logits, targets, B, loss_out, c->dlogits, s));
        STAGE(ST_HEAD_BWD, launch_head_bwd(c, p, g, c->dlogits, B, s));
    }
    return backward_fc(c, B, p, g, nullptr, s);
}
}  // namespace

extern "C" int explainn_train_step(explainn_ctx* c, const float* x, const float* targets, int B,
                                   const explainn_params* p, const explainn_grads* g, int loss_kind,
                                   float dropout_p, uint64_t seed, int freeze_top_n_filters,
                                   float* logits, float* loss_out, void* stream) {
    TRY(train_step_front(c, x, targets, B, p, g, loss_kind, dropout_p, seed, logits, loss_out, stream));
    return backward_conv(c, B, p, g, freeze_top_n_filters, static_cast<hipStream_t>(stream));
}

extern "C" int explainn_train_step_fc(explainn_ctx* c, const float* x, const float* targets, int B,
                                      const explainn_params* p, const explainn_grads* g,
                                      int loss_kind, float dropout_p, uint64_t seed, float* logits,
                                      float* loss_out, void* stream) {
    TRY(train_step_front(c, x, targets, B, p, g, loss_kind, dropout_p, seed, logits, loss_out, stream));
    c->tail_B = B;
    return EXPLAINN_OK;
}

extern "C" int explainn_train_step_conv(explainn_ctx* c, int B, const explainn_params* p,
                                        const explainn_grads* g, int freeze_top_n_filters,
                                        void* stream) {
    TRY(check_batch(c, B));
    if (c->tail_B != B) {
        explainn_set_error("train_step_conv(B=%d) without a matching train_step_fc (pending B=%d)",
                           B, c->tail_B);
        return EXPLAINN_E_STATE;
    }
    c->tail_B = 0;
    return backward_conv(c, B, p, g, freeze_top_n_filters, static_cast<hipStream_t>(stream));
}

extern "C" int64_t explainn_sync_exchange_elems(const explainn_ctx* c, int phase) {
    if (!c || phase < 1 || phase > EXPLAINN_SYNC_PHASES) return 0;
    return sync_exchange_elems(c, phase);
}

extern "C" int explainn_sync_phase(explainn_ctx* c, int phase, const explainn_sync_args* a,
                                   const double* exchange_in, double* exchange_out, void* stream) {
    NOT_ON_BANK(c, "sync-BN (explainn_sync_phase)");
    if (!a || !a->params || !a->grads) { explainn_set_error("sync phase: args, params and grads are required"); return EXPLAINN_E_ARG; }
    TRY(check_batch(c, a->B_local));
    if (phase < 1 || phase > EXPLAINN_SYNC_PHASES) {
        explainn_set_error("sync phase %d outside 1..%d", phase, EXPLAINN_SYNC_PHASES);
        return EXPLAINN_E_ARG;
    }
    if (a->B_global < 2 || a->B_global < a->B_local) {
        explainn_set_error("sync-BN needs B_global >= max(2, B_local) (B_local %d, B_global %d)", a->B_local,
                           a->B_global);
        return EXPLAINN_E_ARG;
    }
    if (c->dense) { explainn_set_error("sync-BN works on one-hot input / base codes only (dense input mode is on)"); return EXPLAINN_E_UNSUPPORTED; }
    if (phase == 3 && (a->dropout_p < 0.f || a->dropout_p >= 1.f)) {
        explainn_set_error("dropout_p must be in [0,1)");
        return EXPLAINN_E_ARG;
    }
    if (phase == 4 && !a->logits) { explainn_set_error("sync phase 4 needs logits"); return EXPLAINN_E_ARG; }
    if (phase == 5) {
        if (!a->dlogits && (!a->logits || !a->targets)) {
            explainn_set_error("sync phase 5 needs dlogits, or logits and targets");
            return EXPLAINN_E_ARG;
        }
        if (!a->dlogits && a->loss_kind != EXPLAINN_LOSS_BCE_WITH_LOGITS && a->loss_kind != EXPLAINN_LOSS_MSE) {
            explainn_set_error("unknown loss kind %d", a->loss_kind);
            return EXPLAINN_E_ARG;
        }
    }
    // the phases run in order on one batch: each one but the first continues the one before
    if (phase != 1 && c->sync_next != phase) {
        explainn_set_error("sync phase %d out of order (expected %d)", phase, c->sync_next ? c->sync_next : 1);
        return EXPLAINN_E_STATE;
    }
    if (phase != 1 && c->sync_B != a->B_local) {
        explainn_set_error("sync phase %d with B_local %d, the step started with %d", phase, a->B_local, c->sync_B);
        return EXPLAINN_E_STATE;
    }
    const bool needs_in = phase == 2 || phase == 3 || phase == 4 || phase == 6 || phase == 7 || phase == 8;
    if ((needs_in && !exchange_in) || (sync_exchange_elems(c, phase) > 0 && !exchange_out)) {
        explainn_set_error("sync phase %d: exchange buffer missing", phase);
        return EXPLAINN_E_ARG;
    }
    c->sync_next = 0;
    TRY(sync_phase(c, phase, a, exchange_in, exchange_out, static_cast<hipStream_t>(stream)));
    c->sync_B = a->B_local;
    c->sync_next = phase < EXPLAINN_SYNC_PHASES ? phase + 1 : 0;
    return EXPLAINN_OK;
}

extern "C" int explainn_dense_input(explainn_ctx* c, int enable) {
    if (!c) { explainn_set_error("null context"); return EXPLAINN_E_ARG; }
    c->dense = enable != 0;
    drop_pending(c);
    return EXPLAINN_OK;
}

extern "C" int explainn_stage_onehot(explainn_ctx* c, const float* x, int B, void* stream) {
    TRY(check_batch(c, B));
    if (!x) { explainn_set_error("x is null"); return EXPLAINN_E_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    drop_pending(c);                   // the packed codes of a pending backward are overwritten
    TRY(launch_pack(c, x, B, true, s));  // with the bit masks: the batch may feed a train forward
    c->staged_B = B;
    c->staged_rc = 0;
    return EXPLAINN_OK;
}

extern "C" int explainn_stage_timing(explainn_ctx* c, int enable) {
    if (!c) { explainn_set_error("null context"); return EXPLAINN_E_ARG; }
    if (enable && !c->ev0[0]) {
        for (int i = 0; i < ST_COUNT; ++i) {
            HIP_TRY(hipEventCreate(&c->ev0[i]));
            HIP_TRY(hipEventCreate(&c->ev1[i]));
        }
    }
    c->timing = enable != 0;
    c->timed = 0;
    return EXPLAINN_OK;
}

extern "C" int explainn_stage_count(void) { return ST_COUNT; }
extern "C" const char* explainn_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

extern "C" int explainn_stage_times(explainn_ctx* c, float* us, int cap) {
    if (!c || !us || cap < ST_COUNT) { explainn_set_error("stage_times: need room for %d floats", ST_COUNT); return EXPLAINN_E_ARG; }
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < ST_COUNT; ++i) {
        us[i] = -1.f;                                   // stage did not run in the last step
        if (c->timed & (1u << i)) {
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, c->ev0[i], c->ev1[i]));
            us[i] = ms * 1e3f;
        }
    }
    c->timed = 0;
    return EXPLAINN_OK;
}

extern "C" int explainn_debug_keep_bits(explainn_ctx* c, int B, uint32_t* out, void* stream) {
    TRY(check_batch(c, B));
    if (!out) { explainn_set_error("out is null"); return EXPLAINN_E_ARG; }
    if (c->fwd_B != B) {
        explainn_set_error("keep_bits(B=%d) without a train-mode forward of that batch in flight (last B=%d)",
                           B, c->fwd_B);
        return EXPLAINN_E_STATE;
    }
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)B * sizeof(uint4), c->bits, (size_t)c->Bs * sizeof(uint4),
                             (size_t)B * sizeof(uint4), (size_t)c->U, hipMemcpyDeviceToDevice,
                             static_cast<hipStream_t>(stream)));
    return EXPLAINN_OK;
}

extern "C" int explainn_input_flags(explainn_ctx* c, int* flags_host, void* stream) {
    if (!c || !flags_host) { explainn_set_error("null argument"); return EXPLAINN_E_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(flags_host, c->flags, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(c->flags, 0, sizeof(int), s));
    HIP_TRY(hipStreamSynchronize(s));
    return EXPLAINN_OK;
}
