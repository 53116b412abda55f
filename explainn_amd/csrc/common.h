// Internal definitions shared by the gfx950 kernels of libexplainn_hip.so.
// Data layout in HBM: everything per-sequence is stored with the batch
// index fastest ("lane = sequence"), so a 64-wide wavefront reads/writes 256 contiguous bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/explainn_hip.h"

#define FC_H 100          // hidden width of the per-unit FC (architectures/__init__.py:86)
#define HEAD_RB 8            // head kernels keep up to HEAD_RB*256 sequences per unit in registers
#define HEAD_GEMM_MIN_T 8   // more tasks than this: combiner forward/backward as MFMA GEMMs (head.hip)
#define HEAD_GROUPS_DEFAULT 4   // blocks per sequence block of the head sums' combiner launch (EXPLAINN_HEAD_GROUPS)
// d Wf = dl^T o^T has K = batch and only ceil(T/32) x ceil((U+1)/32) output tiles (20 at C3): the batch is
// cut into chunks of >= 128 sequences, one workgroup per (tile, chunk), summed per unit in head_bwd
#define HEAD_GW_MAXCH 32
__host__ inline int head_gw_chunks(int B) { int c = (B + 127) / 128; return c < 1 ? 1 : (c > HEAD_GW_MAXCH ? HEAD_GW_MAXCH : c); }
#define POOLW 7           // MaxPool1d(7,7)        (architectures/__init__.py:81)
#define BN_EPS_D 1e-5     // architectures/__init__.py:79,90,99
#define BN_MOM_D 0.1
#define WAVE 64
#define MAX_K 32          // kernel sizes instantiated for the conv kernels
#define MAX_NQ 160        // largest pooled length with an instantiated FC kernel

struct explainn_ctx {
    int U, k, L, T, maxB, device;
    int Gm, Um;           // model bank: Gm members of Um units each (U = Gm*Um); Gm = 1: a single model
    int Lo, n;            // conv output length, pooled length
    int U4, Uq;           // units rounded up to 4, number of unit quads
    int NQ, NS;           // instantiated pooled-length bucket (>= n), its row stride (mult. of 4)
    int Bs;               // batch stride of every [..][b] array (= maxB rounded up to 64)
    int K4;               // 4*k
    int QCH;              // b-chunks of the q-moment kernel
    int ACH;              // b-chunks of passA
    int head_groups;      // blocks per sequence block of the combiner launch that carries the head sums
    // per-stage timing (explainn_stage_timing): events bracketing every stage of the training step
    bool timing; unsigned timed;
    hipEvent_t ev0[16], ev1[16];
    // ---- state of the step in flight ----
    int fwd_B;            // batch of the last train forward (0 = none)
    int tail_B;           // batch of a train_step_fc whose train_step_conv is still due (0 = none)
    int fwd_drop;         // dropout was active
    float fwd_scale;      // 1/(1-p)
    // ---- device scratch ----
    char* base; int64_t bytes;
    uint8_t* codesT;      // [L][Bs]          base code per position, 0..3, 4 = N
    uint32_t* pk2;        // [PW][Bs]         2-bit codes, 16 positions per word (N -> 0)
    uint32_t* nmask;      // [NW][Bs]         1 bit per position, set where N
    int PW, NW;
    unsigned long long* bm;  // [4][tiles][Lp] the batch as bit masks per (base, position): bit b of tile t
                          //                = sequence 64t+b has that base there (train mode, pack.hip)
    int Lp;               // positions per bm row (the pack grid's coverage: NW*32 rounded up to 64)
    double* G;            // [4k][4k]         mean window-indicator second moment
    double* m;            // [4k]             mean window indicator
    float* alpha;         // [U4]             BN1 scale   gamma1/sigma1
    float* shift;         // [U4]             BN1 shift   (bias and mean folded in)
    double* mug;          // [U4]             mean of the raw conv sum
    double* sig1;         // [U4]
    double* Gw;           // [U4][4k]
    float* Wt;            // [Uq][k][5][4]    filter taps, unit-quad interleaved, code 4 -> 0
    uint32_t* Wsg;        // [tiles32][2 k-halves][16]: 0x80000000 where the unit pools the minimum, in the
                          // order a lane of the filter-bank GEMM holds its 16 rows
    uint16_t* Wf;         // [tiles32 (padded to whole unit groups)][KS][3 pieces][64 lanes][8] bf16: the filters as
                          // A fragments of v_mfma_f32_32x32x16_bf16 (k = 4 tap + base), sign(gamma1) folded in
    float* ext;           // [U4 (padded to 64-unit groups)][n][Bs]  pooled extreme of the raw conv sum
    uint8_t* idx;         // [U4][n][Bs]      argmax offset 0..6 inside the pooling window
    float* qs0;           // [U][NS]          shift for the q moments (geometric mean of q over the first 16 sequences)
    float* qS1p;          // [U][QCH][NS]
    float* qS2p;          // [U][QCH][NS][NS]
    double* qbar;         // [U][NS]
    float* VC;            // [U][100][NS]     V1 . C  (BN2 variance in prep2, BN2 backward in mid)
    float* A2;            // [U][100][NS]     FC1 weights with BN2 folded in
    float* A2f;           // [U][7][NK4Q][64][4] the same in MFMA 16x16x4 A-fragment order (fc_fwd stages it)
    float* A2h;           // [U][7][KS][3][64][8] bf16: the same as three bf16 pieces in the A-fragment order of
                          // v_mfma_f32_16x16x32_bf16 (fc_fwd for n <= FC_BF_MAXN; KS = 32-wide k-steps)
    float* sh2;           // [U][100]
    float* sig2;          // [U][100]
    float* z;             // [U][Bs]          FC2 output (without its bias)
    float* zhat;          // [U][Bs]
    float* o;             // [U][Bs]          unit outputs
    float* sig3;          // [U]
    double* z12p;         // [U][ZBLK][2] per-workgroup fp64 sums of z and z^2 from fc_fwd (train)
    int ZBLK;             // fc_fwd workgroups per unit at the largest batch
    uint4* bits;          // [U][Bs]          100 bits per (unit, sequence): relu'>0 and kept
    float* dz;            // [U][Bs]
    float* EQp;           // [U][ACH][NS][100]  passA's partial sums, w-major (four rows r = one 16-byte store)
    float* Sep;           // [U][ACH][100]
    float* EQs;           // [U][100][NS]
    float* Ttf;           // [U][NW16][3][4][64][8] bf16: T as three bf16 pieces in the A-fragment order of
                          //                        v_mfma_f32_16x16x32_bf16 (passB copies it to LDS)
    float* Mff;           // [U][NW16][4 NW16][64] M in A-fragment order, k order (j',i') -> v = 16j'+4g+i' 
    float* k0p;           // [U][NS]
    float* dy;            // [U4][n][Bs]
    float* S12p;          // [U][NG][Bs/16][2] per (w-tile group, 16-sequence tile): sum dy, sum dy*chat
    float* Dspp;          // [U][Bs/16][4k]     filter-gradient partials (one per 32-sequence block and window half)
    int dsp_stride, dsp_count;   // partial slots per unit / how many of them the last conv_bwd wrote
    float* dlogits;       // [maxB][T]         (train_step only)
    float* dlT;           // [T][Bs]   d loss / d logits, task-major (head GEMMs, T > HEAD_GEMM_MIN_T)
    int loss_blocks, loss_n; float* loss_out;   // a deferred loss value (launch_loss_deferred -> launch_head_bwd)
    float* gWp;           // [HEAD_GW_CHUNKS][T][U+1]  batch-chunk partials of the combiner-weight gradient
    double* lossp;        // [64]      per-block partial sums of the loss
    double* hp;           // [U][ceil(maxB/64)][6] the combiner launch's per-block partials of the head backward's
                          //           batch sums: {sum d3, sum d3 zhat, sum dl[t] o (t < T)} (head.hip -> passA)
    double* hb;           // [ceil(maxB/64)][5]    per block: sum_b dl[b][t] (t < T), then its loss terms
    int staged_B;         // batch size of the codes explainn_stage_codes() staged, 0 = none
    // eval-mode tables (filter tables, BatchNorm1/2 folds, FC1 fragments) held in the scratch are
    // those of parameter version eval_version; a train-mode forward overwrites them
    bool eval_valid;
    uint64_t eval_version;
    // soft (not one-hot) input: explainn_dense_input switches the stages that touch x to dense.hip
    bool dense;
    const float* dense_x;  // x of the train forward in flight (its backward reads it again)
    int* flags;           // [1]
    int* bn1_ticket;      // [1]  arrivals of the filter bank's BatchNorm1 workgroups (convpool.hip),
                          //      zeroed by the launch in front of it (pack_tables / prep1_tables)
    int* site_cnt;        // [U4][Bs]  sites per (unit, sequence) of the current batch (filter->PWM export)
    int* site_off;        // [U4][Bs]  their exclusive scan in sequence order, plus the running total
    // input gradient (inputgrad.hip): D = 2k-1 tap offsets / position classes
    double* igcoef;       // [U4][2]   per-unit coefficients c_u, k_u of the train-mode dense terms
    double* igP;          // [D][4][4][k] unit sums of filter products at tap offset d
    double* igR;          // [4][k]
    float* igH;           // [D classes][D][4 a'][4 a]  the H tables
    float* igC;           // [D classes][4]             the constant table
    int keep_B;           // batch of the last explainn_forward_eval_keep (0 = none)
    int sync_next, sync_B;  // sync-BN: the phase due next (0 = none) and the step's B_local
    const float* keep_x;  // its x when it ran the dense kernels (read again by explainn_input_grad)
    int staged_rc;        // the staged codes are the reverse complement of the rows that were given
};

enum explainn_stage {
    ST_PACK, ST_MOMENTS, ST_PREP1, ST_CONV_POOL, ST_QMOM, ST_PREP2, ST_FC_FWD, ST_HEAD_FWD, ST_LOSS,
    ST_HEAD_BWD, ST_PASSA, ST_MID, ST_PASSB, ST_CONV_BWD, ST_FIN, ST_COUNT
};

// ---- error plumbing (api.hip) ----
void explainn_set_error(const char* fmt, ...);
#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess) {                                                    \
            explainn_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                               __FILE__, __LINE__);                                \
            (void)hipGetLastError();  /* reported here: not left for the next launch check */ \
            return EXPLAINN_E_HIP;                                                 \
        }                                                                          \
    } while (0)
#define LAUNCH_CHECK()  HIP_TRY(hipGetLastError())

// ---- launchers, one per pipeline stage (defined next to their kernels) ----
int launch_pack(explainn_ctx* c, const float* x, int B, bool counts, hipStream_t s);
int launch_prep1(explainn_ctx* c, const explainn_params* p, int B, bool train, hipStream_t s);
int launch_moments(explainn_ctx* c, int B, hipStream_t s);
int launch_prep1_tables(explainn_ctx* c, const explainn_params* p, hipStream_t s);
int launch_conv_pool(explainn_ctx* c, const explainn_params* p, int B, bool want_idx, hipStream_t s);
// train forward, one-hot input: > 0 when the filter-bank launch also computes the input moments and
// the BatchNorm1 fold, on that many workgroups of its own (launch_conv_pool_train) -- no moments /
// prep1_stats launches in front of it; 0: the separate launches
int conv_pool_bn1_workgroups(const explainn_ctx* c, int B);
int launch_conv_pool_train(explainn_ctx* c, const explainn_params* p, int B, int naux, hipStream_t s);
int launch_pack_tables(explainn_ctx* c, const float* x, const explainn_params* p, int B, hipStream_t s);
int launch_pack_codes(explainn_ctx* c, const uint8_t* codes, int B, int rc, hipStream_t s);
int launch_conv_act(explainn_ctx* c, int B, float* acts, hipStream_t s);
int launch_filter_act_max(explainn_ctx* c, int B, const uint8_t* select, float* umax, hipStream_t s);
int launch_filter_sites(explainn_ctx* c, int B, const uint8_t* select, const float* thr, int cap,
                        int* site_total, int* pfm, uint8_t* hit, hipStream_t s);
int launch_qmoments(explainn_ctx* c, int B, hipStream_t s);
int launch_prep2(explainn_ctx* c, const explainn_params* p, int B, bool train, hipStream_t s);
int launch_fc_fwd(explainn_ctx* c, const explainn_params* p, int B, bool train,
                  const uint8_t* keep_mask, float drop_p, uint64_t seed, hipStream_t s);
int launch_head_fwd(explainn_ctx* c, const explainn_params* p, int B, bool train, float* logits,
                    float* outs, hipStream_t s);
// The train forward's combiner launch with the head backward's batch sums riding in it (head.hip): the
// loss gradient to c->dlogits, per-block partials to c->hp / c->hb; passA finishes them (fc.hip).
// head_sums_fit: the launch's LDS (statistics + T weight rows) fits.
bool head_sums_fit(const explainn_ctx* c);
int launch_head_fwd_sums(explainn_ctx* c, const explainn_params* p, int B, float* logits, const float* y,
                         int kind, hipStream_t s);
int launch_loss_deferred(explainn_ctx* c, int kind, const float* logits, const float* y, int B, float* loss,
                         float* dlogits, hipStream_t s);
int launch_loss(explainn_ctx* c, int kind, const float* logits, const float* y, int B,
                float* loss, float* dlogits, hipStream_t s);
int launch_head_bwd(explainn_ctx* c, const explainn_params* p, const explainn_grads* g,
                    const float* dlogits, int B, hipStream_t s);
int launch_head_bwd_fused_loss(explainn_ctx* c, const explainn_params* p, const explainn_grads* g,
                               int kind, const float* logits, const float* y, float* loss_out, int B,
                               hipStream_t s);
// The head backward of a few-task model (T <= PA_HEAD_MAX_T) rides in passA's prologue (fc.hip):
// mode 1 = d loss / d logits given (dl), mode 2 = recomputed from logits and targets (+ the loss value)
#define PA_HEAD_MAX_T 4
struct pa_head_args {
    int mode, T, kind;
    const float *dl, *logits, *y;
    float* loss_out;
    const float *Wf, *g3, *o, *zhat, *sig3;
    float *dz, *gWf, *gbf, *gg3, *gb3, *gc2;
};
// The third head-backward route (few tasks, batch > 512): the combiner launch left per-block partials
// of the batch sums (hp, hb; nblk blocks of 64 sequences) and the loss gradient dl; a passA wave adds
// its unit's partials and forms dz in its main loop.  The first line is what that loop reads.
struct pa_sums_args {
    const float *zhat, *dl; float* dz; const float *Wf, *g3, *b3, *sig3;
    int T, nblk;
    const double *hp, *hb;
    float *gWf, *gbf, *gg3, *gb3, *gc2, *loss_out;
};
int launch_passA(explainn_ctx* c, int B, const pa_head_args* head, hipStream_t s);
int launch_passA_sums(explainn_ctx* c, int B, const pa_sums_args& ps, hipStream_t s);
int launch_mid_bwd(explainn_ctx* c, const explainn_params* p, const explainn_grads* g, int B,
                   hipStream_t s);
int launch_passB(explainn_ctx* c, int B, hipStream_t s);
int launch_conv_bwd(explainn_ctx* c, int B, hipStream_t s);
int launch_fin_bwd(explainn_ctx* c, const explainn_params* p, const explainn_grads* g, int B,
                   int freeze_n, hipStream_t s);

// input gradient (inputgrad.hip): eval-mode dy from dlogits; the train-mode tables; dx
int launch_ig_eval_dy(explainn_ctx* c, const explainn_params* p, const float* dlogits, int B, hipStream_t s);
int launch_ig_tables(explainn_ctx* c, const explainn_params* p, int B, hipStream_t s);
int launch_input_grad(explainn_ctx* c, const explainn_params* p, int B, bool train, const float* dense_x,
                      float* dx, hipStream_t s);

// in-silico mutagenesis (ism.hip): the caller's workspace for one sub-batch of B sequences; the
// per-unit substitution kernels and the per-task sum, sub-batch by sub-batch
int64_t ism_workspace_bytes(const explainn_ctx* c, int B);
int launch_ism(explainn_ctx* c, const explainn_params* p, int B, float* delta, float* ws, hipStream_t s);

// Integrated Gradients (pathgrad.hip): the workspace the call is meant to run with; the path walk in
// conv-sum space, the endpoint logits and the transposed convolution, sub-batch by sub-batch (the
// sub-batch is what the caller's workspace holds).  The batch's codes are in c->codesT.
int64_t pathgrad_workspace_bytes(const explainn_ctx* c, int B);
int launch_pathgrad(explainn_ctx* c, const explainn_params* p, int B, int kind, const uint8_t* base_codes,
                    int rc, const float* dlogits, int steps, float* ig, float* logits_x, float* logits_base,
                    void* ws, int64_t ws_bytes, hipStream_t s);

// tiled scan of a long sequence (scan.hip): windows of a device-resident sequence staged as a batch;
// the pooled track of a run of tiles (blocks of TB tiles in the filter bank's output layout, in the
// caller's workspace) unfolded into c->ext for windows [i0, i0 + Bw) of n_windows at stride 7m
int launch_stage_windows(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, int64_t start0, int64_t step,
                         int B, int rc, hipStream_t s);
int launch_scan_unfold(explainn_ctx* c, const float* track, int64_t blk_elems, int64_t J, int TB, int m,
                       int64_t n_windows, int64_t i0, int Bw, int rc, hipStream_t s);
int64_t scan_track_block_elems(const explainn_ctx* c);
int64_t scan_tiles(const explainn_ctx* c, int64_t n_windows, int m);

// variant effects (variants.hip): rows [row0, row0 + B) of an edit table's row table staged as a batch
int launch_stage_edits(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const explainn_edits* ed,
                       int64_t row0, int B, int rc, hipStream_t s);
// haplotypes (haplotypes.hip): the same for rows that carry a run of edits each
int launch_stage_haplotypes(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const explainn_haplotypes* hp,
                            int64_t row0, int B, int rc, hipStream_t s);

// motif sites (sites.hip): the compacted (unit, position, score) list of a range of start positions
int64_t sites_workspace_bytes(const explainn_ctx* c, int64_t npos);
bool sites_workspace_ok(const explainn_ctx* c, int64_t npos, const void* workspace, int64_t workspace_bytes);
int launch_call_sites(explainn_ctx* c, const uint8_t* seq, int64_t start, int64_t npos, int64_t period,
                      int rc, const float* thr, int64_t* offsets, int32_t* pos, float* score,
                      int64_t capacity, void* workspace, hipStream_t s);
int launch_activation_histogram(explainn_ctx* c, const uint8_t* seq, int64_t start, int64_t npos, int64_t period,
                                int rc, uint64_t* hist, hipStream_t s);
// motif enrichment (enrich.hip): per record the best site of every unit (the test itself takes no context)
int launch_record_best(explainn_ctx* c, const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets,
                       int64_t n_records, int strands, uint16_t* best_bits, int32_t* best_site, hipStream_t s);
// motif spacing (spacing.hip): distance histograms of site lists and their test; no context.  The largest
// distance keeps a pair's 2 x (2D+1) histogram of 32-bit bins at 16 KiB of LDS.
static_assert(EXPLAINN_SPACING_MAX_DISTANCE == 1024, "spacing.hip sizes its LDS histogram for this cap");
int launch_site_spacing(const int64_t* pos, const int64_t* offsets2, int U, const int32_t* anchors, int A,
                        const int32_t* partners, int P, int D, int64_t* hist, hipStream_t s);
int launch_spacing_test(const int64_t* hist, int A, int P, const int32_t* anchors, const int32_t* partners, int D,
                        int min_distance, int64_t min_count, int64_t* total, int32_t* best_distance,
                        int64_t* best_count, double* pvalue, hipStream_t s);
// motif centrality (central.hip): position histograms of best sites and CentriMo's test; no context.
// centrality_regions: the admissible regions of a call (their number is returned) and how the kernel
// enumerates them: j0 / items in centred mode, w0 / items in local mode.
int launch_site_positions(const uint16_t* best_bits, const int32_t* best_site, const uint8_t* labels,
                          const float* thresholds, int units, int64_t n_records, int T, int M, int32_t* hist,
                          int64_t* counts, hipStream_t s);
int64_t centrality_regions(int M, int mode, int min_width, int max_width, int* j0, int* w0, int64_t* items);
int launch_centrality_test(const int32_t* hist, const int64_t* counts, int units, int T, int M, int mode, int j0,
                           int w0, int64_t items, int64_t regions, int64_t min_sites, int32_t* best_t,
                           int32_t* best_lo, int32_t* best_width, int64_t* sites, int64_t* count, int64_t* n_tests,
                           double* log_pvalue, double* log_padj, int64_t* ctrl_sites, int64_t* ctrl_count,
                           double* log_fisher, hipStream_t s);

int launch_dense_moments(explainn_ctx* c, const float* x, int B, hipStream_t s);
int launch_dense_conv_pool(explainn_ctx* c, const float* x, const explainn_params* p, int B, hipStream_t s);
int launch_dense_conv_bwd(explainn_ctx* c, const float* x, int B, hipStream_t s);
int launch_dense_conv_act(explainn_ctx* c, const float* x, int B, float* acts, hipStream_t s);

// sync-BN (syncbn.hip): the step as phases with an exchange between them
int64_t sync_exchange_elems(const explainn_ctx* c, int phase);
int sync_phase(explainn_ctx* c, int phase, const explainn_sync_args* a, const double* xin,
               double* xout, hipStream_t s);

int prep_configure(explainn_ctx* c);
int bwd_configure(explainn_ctx* c);
int fc_configure(explainn_ctx* c);

// In-kernel stamps (tools/stampbench.hip defines EXPLAINN_STAMP; the library build compiles them out)
#ifdef EXPLAINN_STAMP
extern __device__ unsigned long long g_stamps[];
#define STAMP(i)                                                                                  \
    do {                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if ((threadIdx.x & 63) == 0)                                                              \
            g_stamps[((size_t)(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z)) * (blockDim.x / 64) + threadIdx.x / 64) * 8 + (i)] = t_; \
    } while (0)
#define STAMP_AFTER_LOADS(i) do { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(i); } while (0)
#else
#define STAMP(i) do { } while (0)
#define STAMP_AFTER_LOADS(i) do { } while (0)
#endif

// KEEP(x): pins a loaded value in a VGPR at this point.  hipcc otherwise sinks a global load into the
// predicated block of its only use (`cond ? f(load) : 0`), which yields one `s_cbranch_execz;
// global_load; s_waitcnt vmcnt(0)` per element -- a fully serialised fetch (22 K cycles for 26 rows).
// Pattern: issue all loads into an array, KEEP() each element in a second loop, then compute.
#define KEEP(x) asm volatile("" : "+v"(x))

// A raw buffer descriptor over the `bytes` bytes at p (no stride, no swizzle: the 32-bit offset of an
// access is range-checked against `bytes`; a load beyond returns 0 and a store beyond is dropped).
// p and bytes must be the same in every lane of the wave: they are made uniform by hand here, because a
// descriptor the compiler cannot prove uniform gets a readfirstlane loop around every access.
template <class P>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(P* p, uint32_t bytes) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), 0,
                                             (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
__device__ __forceinline__ float rsrc_load_f32(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void rsrc_store_f32(float v, __amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)voff, (int)soff, 0);
}

// The sub-batch of an entry point that works through a batch in pieces of one workspace (ISM, IG): the
// sequences that fit cap_bytes at per_sequence_bytes each, in whole steps (a wave: lane = sequence), at
// least one step, no more than the batch rounded up to a step.
#define SUB_BATCH_STEP 64
__host__ inline int sub_batch_of(int64_t cap_bytes, int64_t per_sequence_bytes, int B) {
    int64_t s = cap_bytes / per_sequence_bytes / SUB_BATCH_STEP * SUB_BATCH_STEP;
    if (s < SUB_BATCH_STEP) s = SUB_BATCH_STEP;
    const int64_t bb = ((int64_t)B + SUB_BATCH_STEP - 1) / SUB_BATCH_STEP * SUB_BATCH_STEP;
    return (int)(s < bb ? s : bb);
}

// acc += w s, one FMA per base (the transposed convolutions of inputgrad.hip and pathgrad.hip)
__device__ __forceinline__ void fma4(float4& acc, const float4& w, float s) {
    acc.x = fmaf(w.x, s, acc.x); acc.y = fmaf(w.y, s, acc.y);
    acc.z = fmaf(w.z, s, acc.z); acc.w = fmaf(w.w, s, acc.w);
}

// The filters of units u0 .. u0 + UT - 1 as float4 over the bases, Ws[uu * MAX_K + t] (zeros past U), by
// all nthreads threads of the block between two barriers of the caller; SCALED: times the unit's alpha.
template <bool SCALED, int UT>
__device__ __forceinline__ void stage_filters4(const float* __restrict__ W, const float* __restrict__ alpha,
                                               int u0, int U, int k, int tid, int nthreads, float4* Ws) {
    for (int i = tid; i < UT * k; i += nthreads) {
        const int uu = i / k, t = i - uu * k, u = u0 + uu;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (u < U) {
            const float a = SCALED ? alpha[u] : 1.f;
            const float* wr = W + (size_t)u * 4 * k + t;
            v = SCALED ? make_float4(a * wr[0], a * wr[k], a * wr[2 * k], a * wr[3 * k])
                       : make_float4(wr[0], wr[k], wr[2 * k], wr[3 * k]);
        }
        Ws[uu * MAX_K + t] = v;
    }
}

// The filter bank as a GEMM (convpool.hip) on v_mfma_f32_32x32x16_bf16: k-steps of 16 (4 taps x 4
// bases), 32-unit tiles, two tiles per wave while their fragments and three operand buffers fit
__host__ __device__ inline int conv_ksteps(int k) { return (k + 3) / 4; }
__host__ __device__ inline int conv_ut(int k) { return conv_ksteps(k) <= 5 ? 2 : 1; }
__host__ __device__ inline int conv_tiles_padded(int U, int k) {
    const int ut = conv_ut(k);
    return (((U + 31) / 32 + ut - 1) / ut) * ut;
}

// The filter bank's tables for unit u (all threads of the block call it): Wt (per-tap table,
// unit-quad interleaved, entry 4 = N = zero: the export and dense kernels), Wf / Wsg (the GEMM's A
// fragments and pooling signs) from the current filters.  wsh: 4*MAX_K floats of LDS.
__device__ __forceinline__ void filter_tables_unit(const float* __restrict__ conv_w,
                                                   const float* __restrict__ gamma1,
                                                   float* __restrict__ Wt,
                                                   uint16_t* __restrict__ Wf, uint32_t* __restrict__ Wsg,
                                                   int U, int k, int u, int tid, int nthreads,
                                                   float* wsh) {
    const int K4 = 4 * k;
    for (int i = tid; i < K4; i += nthreads) {
        const int a = i / k, j = i % k;
        const float wv = (u < U) ? conv_w[(size_t)u * K4 + i] : 0.f;
        Wt[((size_t)(u >> 2) * k + j) * 20 + a * 4 + (u & 3)] = wv;
        wsh[i] = wv;
    }
    for (int j = tid; j < k; j += nthreads) Wt[((size_t)(u >> 2) * k + j) * 20 + 16 + (u & 3)] = 0.f;
    __syncthreads();
    // Wf: the unit's row of the A operand of the filter-bank GEMM (convpool.hip), k = 4 tap + base,
    // as three bf16 pieces whose sum is the fp32 weight exactly.  The pooling direction is folded in:
    // a unit with gamma1 < 0 pools the minimum, so its row is negated (exact) and the kernel takes the
    // maximum for everybody and gives the sign back when it stores.
    const int KS = conv_ksteps(k);
    const float sgn = (u < U && gamma1[u] < 0.f) ? -1.f : 1.f;
    // D row of unit u: 8 (r/4) + 4 kh + r%4 within its tile
    if (tid == 0) Wsg[((u >> 5) * 2 + ((u >> 2) & 1)) * 16 + 4 * ((u & 31) >> 3) + (u & 3)] = sgn < 0.f ? 0x80000000u : 0u;
    for (int kk = tid; kk < 16 * KS; kk += nthreads) {
        const int j = kk >> 2, a = kk & 3;
        const float wv = j < k ? sgn * wsh[a * k + j] : 0.f;
        const uint32_t hb = __float_as_uint(wv) & 0xffff0000u;
        const float r1 = wv - __uint_as_float(hb);
        const uint32_t mb = __float_as_uint(r1) & 0xffff0000u;
        const float r2 = r1 - __uint_as_float(mb);
        // A fragment of v_mfma_f32_32x32x16_bf16: lane 32 (k/8 mod 2) + row, element k mod 8
        const int ks = kk >> 4, lane = 32 * ((kk >> 3) & 1) + (u & 31), e = kk & 7;
        uint16_t* dst = Wf + ((((size_t)(u >> 5) * KS + ks) * 3) * 64 + lane) * 8 + e;
        dst[0] = (uint16_t)(hb >> 16);
        dst[512] = (uint16_t)(mb >> 16);
        dst[1024] = (uint16_t)(__float_as_uint(r2) >> 16);
    }
}

// (unit, chunk) of a workgroup of a per-unit kernel launched on a grid (chunks, units rounded up to 8
// [, groups]).  Workgroups are dealt to the 8 XCDs round-robin in dispatch order (x fastest), so
// blockIdx-order (chunk, unit) puts the G chunks of one unit on G different XCDs and every one of
// them pulls the unit's weight fragments through its own L2.  This mapping gives the workgroups
// with equal (linear id mod 8) -- one XCD -- the chunks of the same unit: the fragments cross the
// fabric once and the other chunks hit that L2.  Placement is a speed matter only (the hardware
// promises nothing): results do not depend on it.  Returns false for the padding units.
#ifndef EXPLAINN_XCD_MAP
#define EXPLAINN_XCD_MAP 1
#endif
__device__ __forceinline__ bool unit_chunk_of_block(int U, int& u, int& chunk) {
#if EXPLAINN_XCD_MAP
    const int G = gridDim.x, L = blockIdx.y * G + blockIdx.x;
    const int slot = L >> 3;
    u = (slot / G) * 8 + (L & 7);
    chunk = slot - (slot / G) * G;
#else
    u = blockIdx.y; chunk = blockIdx.x;
#endif
    return u < U;
}
__host__ inline int units_grid(int U) { return (U + 7) & ~7; }

// The end of the train-mode BatchNorm1 fold of unit u, from mu = w.m and wGw = w'Gw (both fp64):
// alpha, shift, the saved mean / sigma for the backward and the running statistics.  One copy for
// prep1_stats_kernel and the filter bank's BatchNorm1 workgroups (convpool.hip), so that the two
// give the same bits.
__device__ __forceinline__ void bn1_fold_finish(double mu, double wGw, int u, float g1u, float b1u,
                                                float cbu, float rmu, float rvu, int B, int Lo,
                                                float* __restrict__ alpha, float* __restrict__ shift,
                                                double* __restrict__ mug, double* __restrict__ sig1,
                                                float* __restrict__ rm, float* __restrict__ rv, int64_t* nbt) {
    double var = wGw - mu * mu;
    var = var > 0 ? var : 0;
    const double sg = sqrt(var + BN_EPS_D);
    const double a = (double)g1u / sg;
    alpha[u] = (float)a;
    shift[u] = (float)((double)b1u - a * mu);
    mug[u] = mu;
    sig1[u] = sg;
    const double N1 = (double)B * (double)Lo;
    rm[u] = (float)((1 - BN_MOM_D) * (double)rmu + BN_MOM_D * ((double)cbu + mu));
    rv[u] = (float)((1 - BN_MOM_D) * (double)rvu + BN_MOM_D * var * N1 / (N1 - 1));
    if (u == 0 && nbt) *nbt += 1;
}

// q = exp(alpha*ext + shift): every consumer must evaluate it identically
__device__ __forceinline__ float qval(float alpha, float ext, float shift) {
    // v_exp_f32 path: ~2 ulp, far inside the 1e-4 parity budget, and 10x fewer instructions
    return __expf(fmaf(alpha, ext, shift));
}

// The loss of one (logit x, target t): its value, and d/dx of the mean over 1/invN terms.  The only
// definition: every route to a loss or its gradient (head.hip, passA's prologue in fc.hip,
// syncbn.hip) evaluates these expressions, which is what keeps the routes equal bit for bit.  Two
// functions, because most callers need one of them and must not pay for the other's transcendentals.
__device__ __forceinline__ float loss_value(int kind, float x, float t) {
    if (kind == EXPLAINN_LOSS_BCE_WITH_LOGITS) return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
    const float e = x - t;
    return e * e;
}
__device__ __forceinline__ float loss_grad(int kind, float x, float t, float invN) {
    if (kind == EXPLAINN_LOSS_BCE_WITH_LOGITS) return (1.0f / (1.0f + expf(-x)) - t) * invN;
    const float e = x - t;
    return 2.0f * e * invN;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the integer forms (int, unsigned, long long, unsigned long long): sum, maximum, and the inclusive
// scan up the lanes (lane = threadIdx.x & 63; lane 63 ends up with the wave's sum)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_integral<T>::value, "floating point sums: wave_sum(float), wave_sum_d");
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
    static_assert(std::is_integral<T>::value, "an integer maximum");
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T t = __shfl_xor(v, off, 64);
        v = t > v ? t : v;
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_scan_up(T v, int lane) {
    static_assert(std::is_integral<T>::value, "an integer scan");
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// Row stride NS of every per-unit table with one entry per pooled position (q, T, M, EQ, VC rows):
// NQ rounded up in chunks of at most 36 floats, each a multiple of 4 (float4-aligned rows; the
// chunking dates from the scalar-operand FC of profiles/r01_b and is kept as the layout).
__host__ __device__ constexpr int chunk_count(int len) { return (len + 35) / 36; }
__host__ __device__ constexpr int chunk_len(int len) {
    return (((len + chunk_count(len) - 1) / chunk_count(len)) + 3) & ~3;
}
// q / T / M / EQ rows: NQ payload floats
__host__ __device__ constexpr int ns_stride(int NQ) { return chunk_count(NQ) * chunk_len(NQ); }

// pooled-length buckets with instantiated FC kernels (0 if unsupported)
static inline int nq_bucket(int n) {
    static const int b[] = {4, 8, 12, 16, 20, 24, 26, 28, 32, 40, 48, 56, 64, 72, 84, 96,
                            112, 128, 140, 160};
    for (unsigned i = 0; i < sizeof(b) / sizeof(b[0]); ++i)
        if (b[i] >= n) return b[i];
    return 0;
}
// the bucket below NQ (n > nq_lower(NQ) for every n that dispatches to NQ)
__host__ __device__ constexpr int nq_lower(int NQ) {
    constexpr int b[] = {0, 4, 8, 12, 16, 20, 24, 26, 28, 32, 40, 48, 56, 64, 72, 84, 96, 112, 128, 140, 160};
    int lo = 0;
    for (int i = 1; i < 21; ++i) if (b[i] == NQ) lo = b[i - 1];
    return lo;
}
// ---- tiling of the FC kernels (fc.hip) on v_mfma_f32_16x16x4_f32 ----
#define FC_MT 7                                          // 16-channel tiles covering the 100 hidden channels
__host__ __device__ constexpr int fc_nk4(int NQ) { return (NQ + 3) / 4; }      // k-steps over pooled positions
__host__ __device__ constexpr int fc_nk4q(int NQ) { return (fc_nk4(NQ) + 3) / 4; }  // ... in float4 groups of 4
__host__ __device__ constexpr int fc_nw16(int NQ) { return (NQ + 15) / 16; }   // 16-wide tiles of pooled positions
// workgroups per unit of an fc_fwd launch (fc.hip: fc_fwd_waves x FC_BTW tiles of 16 sequences)
#ifndef FC_BTW
#define FC_BTW 4
#endif
// wavefronts per fc_fwd workgroup.  The weight fragments are staged once per workgroup (21 KB in the
// bf16 form: a quarter of the kernel at C2, tools/stampbench), but 8-wave workgroups need 6 waves
// per SIMD to be resident at once (600 workgroups on 256 CUs) and at 80 registers the train kernels
// spill; fewer, longer waves (8 tiles each) lost more in latency hiding than the staging saved
__host__ __device__ constexpr int fc_fwd_waves(int NQ) { return 4; }
__host__ __device__ constexpr int fc_fwd_blocks(int B, int NQ) {
    return ((B + 15) / 16 + fc_fwd_waves(NQ) * FC_BTW - 1) / (fc_fwd_waves(NQ) * FC_BTW);
}
#define FC_BF_MAXN 96                                     // fc_fwd runs on the bf16 matrix core (exact 3x3 split) up to here
__host__ __device__ constexpr int fc_ks32(int NQ) { return (NQ + 31) / 32; }   // 32-wide k-steps of the bf16 form
// passA / passB split the w tiles into groups of WGT (one wave / workgroup per group)
__host__ __device__ constexpr int fc_wgt(int NQ) { return fc_nw16(NQ) <= 2 ? fc_nw16(NQ) : 3; }
__host__ __device__ constexpr int fc_ng(int NQ) { return (fc_nw16(NQ) + fc_wgt(NQ) - 1) / fc_wgt(NQ); }

#define NQ_DISPATCH(NQv, CALL)                                                        \
    switch (NQv) {                                                                    \
        case 4: { CALL(4); } break;     case 8: { CALL(8); } break;                   \
        case 12: { CALL(12); } break;   case 16: { CALL(16); } break;                 \
        case 20: { CALL(20); } break;   case 24: { CALL(24); } break;                 \
        case 26: { CALL(26); } break;   case 28: { CALL(28); } break;                 \
        case 32: { CALL(32); } break;   case 40: { CALL(40); } break;                 \
        case 48: { CALL(48); } break;   case 56: { CALL(56); } break;                 \
        case 64: { CALL(64); } break;   case 72: { CALL(72); } break;                 \
        case 84: { CALL(84); } break;   case 96: { CALL(96); } break;                 \
        case 112: { CALL(112); } break; case 128: { CALL(128); } break;               \
        case 140: { CALL(140); } break; case 160: { CALL(160); } break;               \
        default: explainn_set_error("pooled length bucket %d not instantiated", NQv); \
                 return EXPLAINN_E_UNSUPPORTED;                                       \
    }
