/*
 * explainn_hip.h -- C ABI of libexplainn_hip.so: the MI355X (gfx950) implementation of the
 * ExplaiNN batched forward/backward over one-hot DNA.
 *
 * The reference (oriolfornes/ExplaiNN) has no FFI: its boundary for this path is the Python
 * nn.Module surface.  Each entry point below names the reference interface it replaces
 * (paths relative to /root/reference/explainn/).  All pointers except `explainn_ctx*`,
 * `explainn_params*`, `explainn_grads*` and the out-parameters documented as host are DEVICE
 * pointers (fp32, contiguous, row-major, the reference's state_dict shapes).  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  No call synchronises the device unless
 * it says so; nothing here allocates in the launch path (scratch is owned by the context).
 *
 * Every function returns 0 on success, a negative EXPLAINN_E_* code otherwise;
 * explainn_last_error() gives the message for the calling thread.
 */
#ifndef EXPLAINN_HIP_H
#define EXPLAINN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXPLAINN_OK 0
#define EXPLAINN_E_ARG (-1)        /* bad shape / argument                                   */
#define EXPLAINN_E_HIP (-2)        /* a HIP runtime call failed                               */
#define EXPLAINN_E_BATCH1 (-3)     /* train mode with B == 1 (torch BatchNorm raises there)   */
#define EXPLAINN_E_STATE (-4)      /* backward without a matching train-mode forward          */
#define EXPLAINN_E_UNSUPPORTED (-5)

#define EXPLAINN_LOSS_BCE_WITH_LOGITS 0 /* architectures/__init__.py:453-455 nn.BCEWithLogitsLoss() */
#define EXPLAINN_LOSS_MSE 1             /* architectures/__init__.py:456     nn.MSELoss()           */

typedef struct explainn_ctx explainn_ctx;

/* The 14 parameters + 6 running statistics of the reference module, by state_dict key
 * (architectures/__init__.py:72-104).  U = cnn_units, k = kernel_size, n = floor((L-k+1)/7),
 * T = n_features.  The running_* arrays are updated in place by a train-mode forward, exactly
 * as torch.nn.BatchNorm1d does (momentum 0.1, unbiased variance into running_var); the
 * num_batches_tracked pointers may be NULL. */
typedef struct explainn_params {
    const float* conv_w;   /* linears.0.weight   (U,4,k)                                  */
    const float* conv_b;   /* linears.0.bias     (U)                                      */
    const float* bn1_w;    /* linears.1.weight   (U)                                      */
    const float* bn1_b;    /* linears.1.bias     (U)                                      */
    float* bn1_rm;         /* linears.1.running_mean (U)                                  */
    float* bn1_rv;         /* linears.1.running_var  (U)                                  */
    const float* fc1_w;    /* linears.6.weight   (100U,n,1)                               */
    const float* fc1_b;    /* linears.6.bias     (100U)                                   */
    const float* bn2_w;    /* linears.7.weight   (100U)                                   */
    const float* bn2_b;    /* linears.7.bias     (100U)                                   */
    float* bn2_rm;         /* linears.7.running_mean (100U)                               */
    float* bn2_rv;         /* linears.7.running_var  (100U)                               */
    const float* fc2_w;    /* linears.10.weight  (U,100,1)                                */
    const float* fc2_b;    /* linears.10.bias    (U)                                      */
    const float* bn3_w;    /* linears.11.weight  (U)                                      */
    const float* bn3_b;    /* linears.11.bias    (U)                                      */
    float* bn3_rm;         /* linears.11.running_mean (U)                                 */
    float* bn3_rv;         /* linears.11.running_var  (U)                                 */
    const float* final_w;  /* final.weight       (T,U)                                    */
    const float* final_b;  /* final.bias         (T)                                      */
    int64_t* bn1_nbt;      /* linears.1.num_batches_tracked  () int64, may be NULL        */
    int64_t* bn2_nbt;      /* linears.7.num_batches_tracked                               */
    int64_t* bn3_nbt;      /* linears.11.num_batches_tracked                              */
    /* Version of the VALUES behind the pointers above, maintained by the caller: bump it whenever
     * a parameter or running statistic changes (the Python binding derives it from torch's tensor
     * version counters).  Eval-mode entry points keep the folded BatchNorm / filter tables of the
     * last version they saw and rebuild them only when it differs.  0 = unknown: rebuild on
     * every call (what a zero-initialised struct gets). */
    uint64_t version;
} explainn_params;

/* Gradient outputs, same shapes as the parameters; every array is OVERWRITTEN (not
 * accumulated).  What `loss.backward()` leaves in `.grad` at selene/__init__.py:291. */
typedef struct explainn_grads {
    float* conv_w; float* conv_b; float* bn1_w; float* bn1_b;
    float* fc1_w;  float* fc1_b;  float* bn2_w; float* bn2_b;
    float* fc2_w;  float* fc2_b;  float* bn3_w; float* bn3_b;
    float* final_w; float* final_b;
} explainn_grads;

/* Replaces ExplaiNN.__init__ (architectures/__init__.py:44-107) as far as device state goes:
 * fixes (cnn_units, kernel_size, sequence_length, n_features) and allocates scratch for
 * batches of up to max_batch sequences on HIP device `device`.  Synchronous. */
int explainn_create(explainn_ctx** out, int cnn_units, int kernel_size, int sequence_length,
                    int n_features, int max_batch, int device);
/* A model bank: `groups` (G) independently parameterised ExplaiNN models of cnn_units (U) units each,
 * trained on the SAME batches and targets in one fused step -- the N initialisations of train.py's
 * --initialize (train.py:221-255), an ensemble, a seed study.  Up to the combiner the G models are one
 * filter bank of G*U independent units; the head has a member index.  Member g owns units
 * [g*U, (g+1)*U).  On a bank context the entry points keep their signatures and read the arrays with
 * the bank's shapes, member-major: every per-unit array has G*U where a single model has U (conv_w
 * (G*U,4,k), fc1_w (100*G*U,n,1), ... keep_mask (B,100*G*U)), final_w is (G,T,U), final_b (G,T),
 * logits / dlogits are (B,G,T), targets stay (B,T) and are shared, loss_out is G floats (each the mean
 * over that member's own B*T terms); explainn_grads likewise.  num_batches_tracked stays one scalar
 * per BatchNorm (all members step together).  freeze_top_n_filters = n zeroes rows [0,n) of EVERY
 * member.  Member g's results are those of a stand-alone model with its parameters, to the rounding
 * of the order of sums in the head.
 * Supported on a bank: explainn_forward_eval, explainn_forward_train, explainn_backward,
 * explainn_loss_grad, explainn_train_step, explainn_train_step_fc / _conv (the flat gradient buffer
 * is element-wise, so a data-parallel all-reduce is unchanged), explainn_unit_outputs (B,G*U),
 * explainn_unit_activations, the filter export (per unit), explainn_stage_codes / _stage_onehot /
 * _stage_windows / _stage_edited_windows / _stage_haplotype_windows, explainn_scan in every mode
 * (logits (n_windows,G,T)), explainn_score_edits and explainn_score_haplotypes (logits (n_rows,G,T),
 * outs (n_rows,G*U)), explainn_dense_input, explainn_input_flags, stage timing, explainn_debug_keep_bits (G*U,B,4).
 * EXPLAINN_E_UNSUPPORTED on a bank (they fold units through `final` in kernels of their own; run them
 * on one member's model; the context stays usable): explainn_forward_eval_keep, explainn_input_grad,
 * explainn_backward_input, explainn_ism, explainn_integrated_gradients, explainn_sync_phase.
 * groups == 1 is explainn_create.  More than 2000 units in all (the largest count tested): EXPLAINN_E_UNSUPPORTED. */
int explainn_create_bank(explainn_ctx** out, int groups, int cnn_units /* per member */, int kernel_size,
                         int sequence_length, int n_features, int max_batch, int device);
/* number of members of the context: 1 for explainn_create */
int explainn_groups(const explainn_ctx* ctx);
void explainn_destroy(explainn_ctx* ctx);
const char* explainn_last_error(void);
/* bytes of device scratch the context holds */
int64_t explainn_scratch_bytes(const explainn_ctx* ctx);

/* ExplaiNN.forward in eval mode (architectures/__init__.py:109-114; callers predict.py:81-82,
 * selene/__init__.py:334).  x: (B,4,L) fp32 one-hot rows ACGT, N = all-zero column
 * (sequence/__init__.py:19-26).  logits: (B,T). */
int explainn_forward_eval(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                          float* logits, void* stream);

/* ExplaiNN.forward in train mode (caller selene/__init__.py:288): batch statistics in the three
 * BatchNorms, running statistics updated in place, Dropout(0.3) after the first FC
 * (architectures/__init__.py:92).  keep_mask: optional (B,100U) uint8 keep-mask (1 = keep)
 * that replaces the built-in generator -- for parity tests; NULL uses the counter-based
 * generator keyed by (seed, b, unit, channel).  dropout_p == 0 disables dropout.
 * Keeps what explainn_backward needs inside ctx (one step in flight per context). */
int explainn_forward_train(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                           const uint8_t* keep_mask, float dropout_p, uint64_t seed,
                           float* logits, void* stream);

/* Autograd backward of the train-mode forward above (selene/__init__.py:291 loss.backward()):
 * dlogits (B,T) -> all 14 parameter gradients.  freeze_top_n_filters zeroes rows [0,n) of the
 * filter gradient (the hook selene/__init__.py:509-515 / :254-257). */
int explainn_backward(explainn_ctx* ctx, const float* dlogits, int B, const explainn_params* p,
                      const explainn_grads* g, int freeze_top_n_filters, void* stream);

/* The input gradient: what autograd gives as x.grad after model(x) and backward(dlogits) in the
 * reference, whose module is plain torch (saliency maps, gradient x input, Integrated Gradients,
 * the per-base contributions TF-MoDISco reads).  dx: device, fp32 (B,4,L), OVERWRITTEN.
 *
 * explainn_forward_eval_keep: explainn_forward_eval (same logits, bit for bit) that also keeps the
 * pooling's argmax offsets for explainn_input_grad.  explainn_input_grad: dlogits (B,T) -> dx for the
 * last eval_keep forward of B sequences; EXPLAINN_E_STATE when another call came in between (any
 * forward, explainn_stage_codes / _stage_onehot / _dense_input).  An eval forward gives no
 * parameter gradients.
 * explainn_backward_input: explainn_backward (the same 14 gradients, bit for bit) plus dx of the
 * train-mode forward, through BatchNorm1's batch statistics.
 * With x == NULL (a staged batch of base codes) dx is the gradient with respect to the one-hot tensor
 * the forward ran on: the one-hot of the codes, or of their reverse complement when they were staged
 * with reverse_complement != 0 (un-flip it -- dx[:, ::-1, ::-1] -- for the gradient in the staged
 * strand's coordinates).  N columns get their gradient like any other column (the reference's x.grad
 * there is the gradient with respect to an all-zero column).  Soft input (explainn_dense_input) gives
 * the gradient at that x. */
int explainn_forward_eval_keep(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                               float* logits, void* stream);
int explainn_input_grad(explainn_ctx* ctx, const float* dlogits, int B, const explainn_params* p,
                        float* dx, void* stream);
int explainn_backward_input(explainn_ctx* ctx, const float* dlogits, int B, const explainn_params* p,
                            const explainn_grads* g, int freeze_top_n_filters, float* dx, void* stream);

/* In-silico mutagenesis, eval mode: the change of every logit when one base is substituted,
 *   delta[b,t,a,p] = logit_t(x_b with column p replaced by one-hot(a)) - logit_t(x_b),  a = A,C,G,T,
 * fp32 (B,T,4,L) on the device, OVERWRITTEN, plus logits (B,T), bit-identical to
 * explainn_forward_eval on the same batch (absolute mutant logits = logits[:,:,None,None] + delta).
 * Exactly 0 at the reference base (a = the base at p), at positions whose conv windows all fall in the
 * tail MaxPool1d(7,7) drops (p >= 7n + k - 1), and for any substitution that moves no unit's pooled
 * extreme.  At an N position all four rows are real substitutions; substitutions to N are not
 * computed.  x == NULL means the staged batch; for codes staged with reverse_complement != 0 the
 * output is in the coordinates of the strand the model ran on, as for explainn_input_grad.  One-hot
 * and base codes only: in dense input mode EXPLAINN_E_UNSUPPORTED.  Like every eval entry point it
 * ends a pending train forward (its backward then returns EXPLAINN_E_STATE).  No host sync.
 * workspace: device memory of at least explainn_ism_workspace_bytes(ctx, B) bytes (the caller's: the
 * context's own scratch does not grow); larger batches run in sub-batches of that size. */
int64_t explainn_ism_workspace_bytes(const explainn_ctx* ctx, int B);
int explainn_ism(explainn_ctx* ctx, const float* x, int B, const explainn_params* p, float* logits,
                 float* delta, void* workspace, int64_t workspace_bytes, void* stream);

/* Integrated Gradients in eval mode along the straight path x' + a (x - x'), midpoint rule with
 * `steps` nodes a_s = (s + 1/2)/steps:
 *   ig[b,a,p] = (x - x')[b,a,p] * (1/steps) sum_s d(sum_t dlogits[b,t] logit_t)/dx[b,a,p] at node s,
 * fp32 (B,4,L) on the device, OVERWRITTEN.  The convolution is linear in x, so the path is walked in
 * the space of the conv sums (rebuilt from base codes at both ends) and only BatchNorm1, exp, the
 * pooling, the per-unit FC and the head are evaluated per node; one transposed convolution maps the
 * path-averaged gradient back to x.  Baseline x': EXPLAINN_IG_BASELINE_ZERO (all-zero columns),
 * _UNIFORM (0.25 in all four rows of every position) or _CODES (baseline_codes: device, uint8 (B,L),
 * 0..3, anything else = N = an all-zero column).  Where x' == x the result is exactly 0, as it is at
 * positions whose conv windows all fall in the tail MaxPool1d(7,7) drops.  logits_x / logits_base:
 * (B,T) logits at the two ends of the path, from the code that evaluates the nodes (within the
 * project's 1e-4 of explainn_forward_eval, not bit-identical), so that the caller can form the
 * convergence delta sum(ig) - sum_t dlogits (logits_x - logits_base).
 * x == NULL means the staged batch; for codes staged with reverse_complement != 0 the output is in
 * the coordinates of the strand the model ran on and baseline_codes are reverse-complemented the
 * same way.  One-hot and base codes only: in dense input mode EXPLAINN_E_UNSUPPORTED.  steps < 1 or
 * _CODES without baseline_codes: EXPLAINN_E_ARG.  Like every eval entry point it ends a pending train
 * forward (its backward then returns EXPLAINN_E_STATE).  No host sync.  Not on a bank.
 * workspace: device memory, the caller's; explainn_integrated_gradients_workspace_bytes(ctx, B) is
 * the size the call is meant to run with.  Any size that holds a 64-sequence sub-batch (the value
 * for B = 64) is accepted: the batch runs in sub-batches of the largest multiple of 64 sequences that
 * fits, and the result does not depend on the split. */
enum { EXPLAINN_IG_BASELINE_ZERO = 0, EXPLAINN_IG_BASELINE_UNIFORM = 1, EXPLAINN_IG_BASELINE_CODES = 2 };
int64_t explainn_integrated_gradients_workspace_bytes(const explainn_ctx* ctx, int B);
int explainn_integrated_gradients(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                                  int baseline_kind, const uint8_t* baseline_codes, const float* dlogits,
                                  int steps, float* ig, float* logits_x, float* logits_base,
                                  void* workspace, int64_t workspace_bytes, void* stream);

/* Greedy in-silico evolution: one round's selection.  In-silico evolution changes each sequence toward
 * an objective one substitution per round -- take the ISM maps, apply the best admissible single
 * substitution, repeat.  The reference has no such call.
 *
 * The objective of base a at position p of sequence b (coordinates of the given strand), fp64:
 *   O_f[a,p] = sum_t (double)w[b,t] * (double)delta_f[b,t,a,p]            t ascending
 *   O_r[a,p] = sum_t (double)w[b,t] * (double)delta_r[b,t,3-a,L-1-p]      both strands only
 *   gain     = O_f, or 0.5 * (O_f + O_r) with both strands
 * delta_fwd / delta_rev: device fp32 (B,T,4,L), explainn_ism's maps of the batch staged with
 * reverse_complement = 0 / 1 (the reverse map is in its own strand's coordinates, see explainn_ism);
 * delta_rev NULL = one strand.  weights: device fp32, (T) for every sequence or, weights_per_row != 0,
 * (B,T).  A candidate is admissible when a is not the base at p (at an N, any code above 3, all four
 * bases are), mutable_mask[b,p] != 0 (NULL: every position) and gain > min_gain, min_gain >= 0 and
 * finite (else EXPLAINN_E_ARG).  The winner is the largest gain, then the lowest p, then the lowest a:
 * it is written into codes (B,L, in place), logged in pos / ref / alt (ref = the byte it replaced) /
 * gain, (B) each, and, with lock != 0, its position is closed in mutable_mask (in place; with a NULL
 * mask there is nothing to lock), so a later round cannot revisit it.  A sequence without an admissible
 * candidate logs pos = -1, ref = alt = 255, gain = 0 and keeps its codes.  No context, no workspace, no
 * allocation, no host sync, no atomics: one launch on `stream`. */
int explainn_evolve_pick(const float* delta_fwd, const float* delta_rev, uint8_t* codes,
                         uint8_t* mutable_mask, const float* weights, int weights_per_row, int B, int T, int L,
                         int lock, float min_gain, int32_t* pos, uint8_t* ref, uint8_t* alt, double* gain,
                         void* stream);

/* get_loss (architectures/__init__.py:446-456), mean reduction, fused with its gradient:
 * loss_out (1 float, device) and dlogits (B,T, device). */
int explainn_loss_grad(explainn_ctx* ctx, int loss_kind, const float* logits, const float* targets,
                       int B, float* loss_out, float* dlogits, void* stream);

/* One whole training step of the hot loop selene/__init__.py:288-291 without the optimiser:
 * train forward + loss + backward, enqueued back to back on `stream`. */
int explainn_train_step(explainn_ctx* ctx, const float* x, const float* targets, int B,
                        const explainn_params* p, const explainn_grads* g, int loss_kind,
                        float dropout_p, uint64_t seed, int freeze_top_n_filters,
                        float* logits, float* loss_out, void* stream);

/* The same step in the two halves a data-parallel run overlaps its gradient all-reduce with
 * (selene/__init__.py:288-291 has no such split; the reference is single-device):
 * explainn_train_step_fc runs forward, loss and the backward down to the per-unit FC stage -- on
 * return (in stream order) every gradient from fc1_w to final_b, the contiguous tail of a flat
 * buffer laid out in explainn_grads order and 97-99 % of its bytes, is final and may be handed to
 * RCCL on another stream; explainn_train_step_conv finishes the step (conv_w, conv_b, bn1_w,
 * bn1_b).  fc + conv == explainn_train_step, bit for bit. */
int explainn_train_step_fc(explainn_ctx* ctx, const float* x, const float* targets, int B,
                           const explainn_params* p, const explainn_grads* g, int loss_kind,
                           float dropout_p, uint64_t seed, float* logits, float* loss_out,
                           void* stream);
int explainn_train_step_conv(explainn_ctx* ctx, int B, const explainn_params* p,
                             const explainn_grads* g, int freeze_top_n_filters, void* stream);

/* model.linears(x_rep) in eval mode (test.py:151): per-unit outputs (B,U). */
int explainn_unit_outputs(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                          float* outs, void* stream);
/* model.linears[:3](x_rep) in eval mode (test.py:159-160): exp(BN(conv)) per position,
 * (B,U,L-k+1). */
int explainn_unit_activations(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                              float* acts, void* stream);

/* Filter -> PWM export, replacing the dense float16 (N,U,Lo) host array of
 * test.py:128-166 and the Python loops of interpret.py:363-459.  Both calls stream batches; the
 * accumulators live in caller memory (device pointers) and persist across calls.
 *
 * select: [B] bytes or NULL -- 1 = the sequence is one of the "well predicted" ones
 * (interpret.py:310-361, host logic); unselected sequences contribute nothing.
 *
 * explainn_filter_act_max: unit_max[u] = max(unit_max[u], max over selected sequences and positions
 * of the eval-mode activation rounded to float16 as test.py:137 stores it).  Zero unit_max before
 * the first batch; interpret.py:373's threshold is 0.5 * unit_max (in float16). */
int explainn_filter_act_max(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                            const uint8_t* select, float* unit_max, void* stream);
/* explainn_filter_sites: every start position j of a selected sequence whose float16 activation
 * exceeds thresholds[u] is a site x[j : j+k] (interpret.py:401-421); pfm[u][t][a] (int32, (U,k,4),
 * A/C/G/T; an N inside a site counts for no letter) += its letters (interpret.py:431-459).  Sites
 * are ranked in (call, sequence, position) order -- feed the forward strand's batches first, then the
 * reverse strand's, as interpret.py:385-429 iterates -- and only the first site_cap per unit count
 * (interpret.py:423-425, 1e6 there); site_total[u] (int32 [U], zero before the first batch) carries
 * the rank across calls and ends as min(#sites, site_cap).  hit: optional (B,U) bytes out, 1 = the
 * sequence has at least one position above the unit's threshold (interpret.py:485-490). */
int explainn_filter_sites(explainn_ctx* ctx, const float* x, int B, const explainn_params* p,
                          const uint8_t* select, const float* thresholds, int site_cap,
                          int32_t* site_total, int32_t* pfm, uint8_t* hit, void* stream);

/* Base-code input: instead of the fp32 one-hot (16*L bytes per sequence) hand the
 * sequences over as a (B,L) byte matrix of base codes -- 0,1,2,3 = A,C,G,T, 4 = N, the integers
 * sequence.one_hot_encode (sequence/__init__.py:8-28) turns into one-hot columns -- and let the
 * kernel reverse-complement them on the fly when reverse_complement != 0 (the augmentation of
 * train.py:275-278 / predict.py:78-79 without a second copy of the data).  The codes are packed
 * into the context; every entry point above that takes `x` then accepts x == NULL, meaning "the
 * staged batch" (B must match, else EXPLAINN_E_STATE; passing a real x discards the staged batch).
 * Other byte values are treated as N and raise bit 0 of explainn_input_flags. */
int explainn_stage_codes(explainn_ctx* ctx, const uint8_t* codes, int B, int reverse_complement,
                         void* stream);

/* Scoring a sequence longer than sequence_length (L) with overlapping windows -- what a user of the
 * reference does by materialising every window on the host and calling predict.py.
 *
 * explainn_stage_windows: like explainn_stage_codes, but the batch is cut out of ONE device-resident
 * sequence: seq holds seq_len base codes (0..3 = ACGT, 4 = N) and row b of the staged batch is
 * seq[start0 + b*step : start0 + b*step + L]; start0 and step are signed.  A position outside
 * [0, seq_len) reads as N and raises no flag; a byte above 4 inside it is N and raises bit 0 of
 * explainn_input_flags.  reverse_complement != 0 reverse-complements every row on the fly.  The context
 * then holds exactly what explainn_stage_codes would hold for the materialised (B,L) matrix: every
 * entry point that takes x == NULL runs on it, train mode included.
 *
 * explainn_scan: the eval-mode logits of the windows seq[start + i*stride : ... + L],
 * i = 0 .. n_windows-1, fp32 (n_windows,T) on the device -- (n_windows,G,T) on a bank context.  With
 * reverse_complement != 0 row i is the logit of the reverse complement of window i.  Positions outside
 * the sequence read as N.  No host synchronisation, no allocation; windows run in sub-batches of the
 * context's max_batch.  Like every eval entry point it ends a pending train forward, rebuilds the folded
 * tables only when params->version moved, and leaves no staged batch behind (x == NULL afterwards is
 * EXPLAINN_E_STATE).  Dense input mode: EXPLAINN_E_UNSUPPORTED.  mode:
 *   EXPLAINN_SCAN_WINDOWS  every sub-batch is staged with explainn_stage_windows and run through the
 *                          ordinary eval forward; any stride >= 1; needs no workspace.
 *   EXPLAINN_SCAN_SHARED   stride must be a multiple of 7 (else EXPLAINN_E_ARG; the context stays
 *                          usable).  MaxPool1d(7,7) then pools every window on one grid, so the filter
 *                          bank runs ONCE over the region, on tiles placed 7n apart, and every window's
 *                          pooled vector is a slice of that track; the FC and the
 *                          head run per window as always.  Same logits as WINDOWS, bit for bit.  The
 *                          track lives in `workspace`: device memory, 256-byte aligned, of at least
 *                          explainn_scan_workspace_bytes(ctx, n_windows, stride, mode) bytes (one
 *                          filter-bank output array per max_batch tiles).
 *   EXPLAINN_SCAN_AUTO     SHARED where it is legal and was measured faster, else WINDOWS; the size
 *                          query resolves the same way.
 * explainn_scan_workspace_bytes returns the negative error code for a bad argument. */
#define EXPLAINN_SCAN_AUTO 0
#define EXPLAINN_SCAN_WINDOWS 1
#define EXPLAINN_SCAN_SHARED 2
int explainn_stage_windows(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len, int64_t start0,
                           int64_t step, int B, int reverse_complement, void* stream);
int64_t explainn_scan_workspace_bytes(const explainn_ctx* ctx, int64_t n_windows, int64_t stride, int mode);
int explainn_scan(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len, int64_t start, int64_t n_windows,
                  int64_t stride, int reverse_complement, const explainn_params* p, float* logits, int mode,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* Scoring sequence variants: the batch rows are windows of ONE device-resident sequence at arbitrary
 * starts, each with at most one edit (an SNV, MNV, insertion, deletion or any ref -> alt replacement)
 * spliced in on the device -- what a user of the reference does by building both haplotype windows of
 * every variant on the host.  All pointers of explainn_edits are device pointers.
 *
 * Row b is defined by row_start[b] (int64, signed) and row_edit[b] (int32: an index into the edit
 * table, negative = no edit, a plain reference window).  Edit e has pos[e] (int64, 0-based, reference
 * coordinates), ref_len[e] >= 0, alt_len[e] >= 0 and alt_off[e], an offset into the byte pool `alt` of
 * base codes (alt_bytes of them, < 2^31).  The haplotype is
 *     H = seq[:pos] + alt[alt_off : alt_off + alt_len] + seq[pos + ref_len:]
 * and row b is H[row_start : row_start + L]: row_start counts in haplotype coordinates, which equal
 * reference coordinates whenever row_start <= pos.  For output position q, g = row_start + q, the base is
 *     seq[g]                        when g < pos,
 *     alt[alt_off + g - pos]        when g < pos + alt_len,
 *     seq[g - alt_len + ref_len]    otherwise.
 * A source index outside [0, seq_len) reads as N and raises no flag, as in explainn_stage_windows.  A
 * byte above 4, in seq inside the range or in alt, reads as N and raises bit 0 of explainn_input_flags.
 * The tables are never read by the host, so the kernel stays memory-safe on a bad one: a row whose
 * row_edit >= n_edits, or whose edit has a negative length or an alt run that leaves the pool
 * (alt_off < 0 or alt_off + alt_len > alt_bytes), reads as N throughout and raises bit 0.
 * reverse_complement != 0 reverse-complements the row after the edit.  One edit per row: a haplotype
 * of several variants goes through explainn_haplotypes below.
 *
 * explainn_stage_edited_windows stages rows row0 .. row0 + B - 1 of the tables.  The context then holds
 * exactly what explainn_stage_codes would hold for the materialised (B,L) matrix: every entry point
 * that takes x == NULL runs on it, train mode included.
 *
 * explainn_score_edits: the eval-mode results of rows 0 .. n_rows-1, in sub-batches of the context's
 * max_batch: logits fp32 (n_rows,T) -- (n_rows,G,T) on a bank context -- and / or outs, the per-unit
 * outputs of explainn_unit_outputs, fp32 (n_rows,units), units = G*U on a bank.  Either may be NULL, not
 * both (EXPLAINN_E_ARG; the context stays usable).  Row by row the results are those of
 * explainn_stage_edited_windows followed by explainn_forward_eval / explainn_unit_outputs, bit for bit.
 * No host synchronisation, no allocation.  Like every eval entry point it ends a pending train
 * forward, rebuilds the folded tables only when params->version moved, and leaves no staged batch
 * behind.  Dense input mode: EXPLAINN_E_UNSUPPORTED. */
typedef struct explainn_edits {
    const int64_t* row_start;
    const int32_t* row_edit;
    const int64_t* pos;
    const int32_t* ref_len;
    const int32_t* alt_len;
    const int32_t* alt_off;
    const uint8_t* alt;
    int64_t n_edits;
    int64_t alt_bytes;
} explainn_edits;
int explainn_stage_edited_windows(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len,
                                  const explainn_edits* edits, int64_t row0, int B, int reverse_complement,
                                  void* stream);
int explainn_score_edits(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len, const explainn_edits* edits,
                         int64_t n_rows, int reverse_complement, const explainn_params* p,
                         float* logits /* (n_rows,[G,]T) or NULL */, float* outs /* (n_rows,units) or NULL */,
                         void* stream);

/* Scoring haplotypes: as above, but a row carries a RUN of edits -- two variants in one window, a
 * phased genotype over a region, two insertions at a varying distance.  All pointers of
 * explainn_haplotypes are device pointers.
 *
 * The edit table (pos, ref_len, alt_len, alt_off, the pool alt of alt_bytes < 2^31 base codes; n_edits
 * records) is that of explainn_edits: one record per variant.  A haplotype is a list of int32 indices
 * into it, so a carried variant costs 4 bytes per haplotype: row b has row_start[b] (int64, signed),
 * row_first[b] (int64, an index into edit_index) and row_count[b] (int32, >= 0), and its edits are
 *     e_i = edit_index[row_first[b] + i],   i < row_count[b],   in list order.
 * The run must be ordered and non-overlapping: pos[e_i] + ref_len[e_i] <= pos[e_{i+1}].  Abutting edits
 * are legal; so are two insertions (ref_len 0) at one position, which apply in list order.  With
 * pos_i, ref_i, alt_i the fields of e_i and c = row_count[b] the haplotype is
 *     H = seq[:pos_0] + alt_0 + seq[pos_0 + ref_0 : pos_1] + alt_1 + ... + seq[pos_{c-1} + ref_{c-1}:]
 * and row b is H[row_start : row_start + L]: row_start counts in the coordinates of that H, which equal
 * reference coordinates up to the run's first edit.  In closed form, with
 *     shift_i = sum_{m<i} (alt_len_m - ref_len_m),   hstart_i = pos_i + shift_i   (nondecreasing in i),
 * for output position q, g = row_start + q, the base is
 *     seq[g]                           when g < hstart_0,
 *     alt[alt_off_i + g - hstart_i]    when hstart_i <= g < hstart_i + alt_len_i,
 *     seq[g - shift_{i+1}]             otherwise, i the last edit with hstart_i <= g
 * in wrapping 64-bit arithmetic.  reverse_complement != 0 reverse-complements the row after the edits.
 * A source index outside [0, seq_len) reads as N and raises no flag; a byte above 4, in seq inside the
 * range or in alt, reads as N and raises bit 0 of explainn_input_flags.  row_count == 0 is a plain
 * reference window, and a run of one edit stages bit for bit what explainn_stage_edited_windows stages
 * for that edit.
 *
 * The tables are never read by the host, so the kernel stays memory-safe on a bad one: no index becomes
 * an address before it is range-checked, and a row with row_count < 0, row_first < 0 or row_first +
 * row_count > n_index, an edit_index outside [0, n_edits), an edit with a negative length or an alt run
 * that leaves the pool (alt_off < 0 or alt_off + alt_len > alt_bytes), or a run that violates the
 * ordering rule reads as N throughout and raises bit 0; the other rows of the batch are unaffected.
 *
 * row_count has no cap, but a row's whole run is walked (and validated) by every 64-position tile of
 * the row, 64 edits at a time, so the cost of a row grows with its run length: start a run near the
 * window -- at the first variant at or right of row_start -- not at the chromosome's start.
 *
 * explainn_stage_haplotype_windows stages rows row0 .. row0 + B - 1.  The context then holds exactly what
 * explainn_stage_codes would hold for the materialised (B,L) matrix: every entry point that takes
 * x == NULL runs on it, train mode included; a pending train forward is dropped.
 *
 * explainn_score_haplotypes is explainn_score_edits on these rows: logits fp32 (n_rows,T) --
 * (n_rows,G,T) on a bank context -- and / or outs fp32 (n_rows,units); either may be NULL, not both
 * (EXPLAINN_E_ARG; the context stays usable).  Sub-batches of max_batch, no host synchronisation, no
 * allocation, no staged batch left behind.  Dense input mode: EXPLAINN_E_UNSUPPORTED. */
typedef struct explainn_haplotypes {
    const int64_t* row_start;
    const int64_t* row_first;
    const int32_t* row_count;
    const int32_t* edit_index;
    const int64_t* pos;
    const int32_t* ref_len;
    const int32_t* alt_len;
    const int32_t* alt_off;
    const uint8_t* alt;
    int64_t n_index;
    int64_t n_edits;
    int64_t alt_bytes;
} explainn_haplotypes;
int explainn_stage_haplotype_windows(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len,
                                     const explainn_haplotypes* haps, int64_t row0, int B,
                                     int reverse_complement, void* stream);
int explainn_score_haplotypes(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len,
                              const explainn_haplotypes* haps, int64_t n_rows, int reverse_complement,
                              const explainn_params* p, float* logits /* (n_rows,[G,]T) or NULL */,
                              float* outs /* (n_rows,units) or NULL */, void* stream);

/* Calling motif sites: every (unit, start position) of a device-resident sequence of base codes
 * (0..3 = ACGT, 4 = N, as explainn_scan takes it) whose eval-mode activation, rounded to float16 as
 * the reference stores it, exceeds the unit's threshold -- the positions np.where finds in the dense
 * float16 activation array (interpret.py:375-429), without that array.  For unit u and start p
 *     a16(u,p) = float16(exp(alpha[u] * sum_{j<k} w[u][j][seq[p+j]] + shift[u]))
 * (the value model.linears[:3] gives at that position of any window that holds the k-mer, bit for
 * bit; N contributes 0), and (u,p) is a site when a16 > thresholds[u].  The call covers the starts
 * p = start .. start + n_positions - 1.  With reverse_complement != 0 the activation at p is that of
 * the filter on the reverse complement of seq[p : p+k] -- what the forward pass gives at position
 * len-k-p of the reverse-complemented sequence; positions stay in forward coordinates.  period > 0:
 * seq is a concatenation of records of `period` bases, and a start with p mod period > period - k (its
 * k-mer would cross a record boundary) is never a site.  A byte above 4 reads as N and raises bit 0 of
 * explainn_input_flags.
 *
 * units = the context's filter-bank width (G*U on a bank context); thresholds: fp32 [units], device.
 * offsets: int64 [units+1], device, always written: the exclusive scan of the FULL per-unit site
 * counts.  pos (int32, start-relative) and score (a16 as fp32; may be NULL): record offsets[u] + r is
 * the r-th site of unit u in ascending position; records with index >= capacity are not written
 * (offsets still tells the truth).  pos == NULL: count only.  The order is a function of the input
 * alone (counts and scans; no rank depends on the arrival order of an atomic).
 * workspace: device memory, 256-byte aligned, of explainn_call_sites_workspace_bytes(ctx, n_positions)
 * bytes.  No host synchronisation, no allocation.  EXPLAINN_E_ARG unless 0 <= start,
 * start + n_positions + k - 1 <= seq_len and n_positions + k < 2^31.  Like every eval entry point it
 * ends a pending train forward, rebuilds the folded tables only when params->version moved, and
 * leaves no staged batch behind.  Dense input mode: EXPLAINN_E_UNSUPPORTED.
 * EXPLAINN_SITES_TILE: start positions per workgroup (tests place their sequence ends around it). */
#define EXPLAINN_SITES_TILE 1024
int64_t explainn_call_sites_workspace_bytes(const explainn_ctx* ctx, int64_t n_positions);
int explainn_call_sites(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len, int64_t start,
                        int64_t n_positions, int64_t period, int reverse_complement,
                        const explainn_params* p, const float* thresholds, int64_t* offsets, int32_t* pos,
                        float* score, int64_t capacity, void* workspace, int64_t workspace_bytes,
                        void* stream);

/* The empirical null of the activations explainn_call_sites thresholds (csrc/actnull.hip, DESIGN.md
 * section 8, "Calibrated sites").  a16(u,p) above is float16(exp(.)), never negative: its bit pattern is
 * one of EXPLAINN_ACT_BINS = 32768 values that sort in the order of the values they encode (0x7C00 =
 * +inf, the NaN patterns above it), so a unit's null is held exactly as an integer histogram.
 *
 * explainn_activation_histogram: for every unit u of the context (G*U on a bank context) and every live
 * start p in [start, start + n_positions):  hist[u][bits(a16(u,p)) & 0x7FFF] += 1, with a16 the value of
 * explainn_call_sites bit for bit.  "Live" as there: with period > 0 a start with p mod period >
 * period - k is not counted, so every live start adds exactly one count to every unit's row.
 * hist: device uint64 [units][EXPLAINN_ACT_BINS], ADDED INTO (the caller zeroes it once and may
 * accumulate any number of calls, strands and chunks).  The reverse strand, N, bytes above 4 (read as N,
 * bit 0 of explainn_input_flags), the argument checks (EXPLAINN_E_ARG), the eval-mode table handling
 * and dense input mode (EXPLAINN_E_UNSUPPORTED) are those of explainn_call_sites.  n_positions == 0
 * launches nothing.  No host synchronisation, no allocation, no workspace.  All additions are integer:
 * the result is a function of the input alone.
 * EXPLAINN_ACT_SPAN: start positions a workgroup takes at a time; a unit's spans are dealt round robin
 * to its workgroups (tests place their sequence ends around it).
 *
 * explainn_activation_null: from hist [units][EXPLAINN_ACT_BINS] (device),
 *     total[u]   = sum_b hist[u][b]
 *     tail[u][b] = sum_{b' >= b} hist[u][b']        the null activations >= the value with pattern b
 *     thresholds[u] = the float16 value, as fp32, of the smallest pattern b <= 0x7C00 with
 *                     tail[u][b+1] <= m,  m = (uint64) floor(alpha * (double) total[u])
 * (0x7C00 if there is none; +inf when total[u] == 0).  explainn_call_sites compares with a strict >, so
 * at this threshold it calls at most m of the null's positions, and more than m one float16 value
 * lower.  tail and thresholds may be NULL; total is required.  0 <= alpha <= 1, else EXPLAINN_E_ARG.
 * No context, no workspace, no allocation, no host synchronisation. */
#define EXPLAINN_ACT_BINS 32768
#define EXPLAINN_ACT_SPAN 8192
int explainn_activation_histogram(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len, int64_t start,
                                  int64_t n_positions, int64_t period, int reverse_complement,
                                  const explainn_params* p, uint64_t* hist, void* stream);
int explainn_activation_null(const uint64_t* hist, int units, double alpha, uint64_t* tail, uint64_t* total,
                             float* thresholds, void* stream);

/* Motif spacing (csrc/spacing.hip): which filters' sites occur together, and
 * at what distance.  Sites come as explainn_call_sites lists them: pos holds int64 forward-strand starts,
 * and offsets2, int64 [2U+1], cuts it into one list per (unit, strand): unit u's '+' sites are
 * [offsets2[2u], offsets2[2u+1]), its '-' sites [offsets2[2u+1], offsets2[2u+2]), each in ascending start.
 * For every ordered pair of DISTINCT records i, j (distinct by index, not by position), with a, b their
 * units and s_i, s_j = +-1 their strands:
 *     d = (pos[j] - pos[i]) * s_i        where the partner lies in the anchor's own orientation
 *     o = 0 if s_i == s_j, else 1
 *     |d| <= max_distance:  hist[a][b][o][d + max_distance] += 1
 * so hist[a][b][0][D+d] == hist[b][a][0][D-d] and hist[a][b][1][D+d] == hist[b][a][1][D+d].
 * anchors (A), partners (P): int32 unit indices on the device, in any order, overlapping or not; NULL means
 * all units in order (A, P must then equal U); an index outside [0,U) counts nothing.  hist: device int64
 * [A][P][2][2 max_distance + 1], ADDED INTO: the caller zeroes it once and accumulates any number of calls.
 * The entry point knows nothing of records: the caller keeps sequences apart by spacing their coordinates
 * more than max_distance apart.  Coordinates are int64; differences must fit int64.  A list that is not
 * ascending gives wrong counts, never an access outside its own range; offsets2 is trusted.  A workgroup
 * counts in 32-bit bins: lists of distinct starts, as explainn_call_sites gives them, cannot overflow one.
 * All additions are integer: the result is a function of the input alone.  No context, no workspace, no
 * allocation, no host synchronisation.  A, P, U < 0, A > 65535, a NULL set whose size is not U, or
 * max_distance outside [0, EXPLAINN_SPACING_MAX_DISTANCE]: EXPLAINN_E_ARG, nothing launched.  A == 0 or
 * P == 0 launches nothing.
 *
 * explainn_spacing_test: SpaMo's test of a preferred spacing, one result per (a, b, o), all [A][P][2] on
 * the device.  The admissible bins are min_distance <= |d| <= max_distance with the counts c_d of hist,
 * except where anchor and partner are the same unit (compared as unit indices): for o = 0 every unordered
 * pair sits once at +d and once at -d, and only the bins d >= max(min_distance, 1) are taken; for o = 1
 * every unordered pair sits twice in one bin, and every count is halved.  With m admissible bins:
 *     total = n = sum c_d;  best_count = c = max c_d;  best_distance = the d of the lowest bin that holds c
 *     pvalue = min(1, m P[Binomial(n, 1/m) >= c])      a uniform null over the bins, Bonferroni over them
 * the tail summed in fp64 from x = c upwards as exp(lgamma(n+1) - lgamma(x+1) - lgamma(n-x+1) + x log(1/m)
 * + (n-x) log1p(-1/m)) until a term no longer changes the sum; m == 1 gives 1.  n < max(min_count, 1) or
 * m == 0: pvalue 1, best_count 0, best_distance 0 (total is still n).  Outputs are OVERWRITTEN.
 * min_distance, min_count < 0 and the size checks above: EXPLAINN_E_ARG.  No host synchronisation. */
#define EXPLAINN_SPACING_MAX_DISTANCE 1024
int explainn_site_spacing(const int64_t* pos, const int64_t* offsets2, int U, const int32_t* anchors, int A,
                          const int32_t* partners, int P, int max_distance, int64_t* hist, void* stream);
int explainn_spacing_test(const int64_t* hist, int A, int P, const int32_t* anchors, const int32_t* partners,
                          int max_distance, int min_distance, int64_t min_count, int64_t* total,
                          int32_t* best_distance, int64_t* best_count, double* pvalue, void* stream);

/* Motif enrichment (csrc/enrich.hip, DESIGN.md section 8, "Enrichment"): which filters' best sites score
 * higher in a primary set of records than in a control set, and at what score threshold.
 *
 * explainn_record_best: seq holds device base codes as explainn_call_sites takes them; rec_offsets, device
 * int64 [n_records + 1], cuts it into records: record r is seq[rec_offsets[r] : rec_offsets[r+1]].  For every
 * unit u of the context (G*U on a bank context) and every record r
 *     best_bits[u][r] (uint16) = max over the record's live starts p and the requested strands of
 *                                bits(a16(u,p)) & 0x7FFF
 * with a16 the value explainn_call_sites compares, bit for bit (from 0.f, taps in j order, fp32, the folded
 * BatchNorm1 and exp, rounded to float16; N contributes 0); a start is live when its k-mer lies inside the
 * record; strands: 1 = forward only, 2 = both, the reverse strand as in explainn_call_sites (the filter on
 * the reverse complement of seq[p : p+k], reported at the forward start p).
 *     best_site[u][r] (int32; may be NULL) = (p_rel << 1) | is_minus  of the maximising site, p_rel its
 *                                forward start relative to the record
 * Among equal maxima the lowest start wins, and at one start '+' before '-'.  A record shorter than k has no
 * live start: bits 0, site -1.  A record whose offsets descend or leave [0, seq_len], or of 2^30 bases or
 * more (its starts would not fit the site word), reads as having no live start and raises bit 0 of
 * explainn_input_flags; it is never a read outside seq.  A byte above 4 inside a record reads as N and
 * raises bit 0.  Both outputs are unit-major [units][n_records] and OVERWRITTEN.  The result is a maximum
 * over integer keys (bits, then ~start, then strand): a function of the input alone.  EXPLAINN_E_ARG unless
 * seq_len >= 0, 0 <= n_records < 2^31 and strands is 1 or 2; the eval-mode table handling and dense input
 * mode (EXPLAINN_E_UNSUPPORTED) are those of explainn_call_sites.  n_records == 0 launches nothing.  No
 * host synchronisation, no allocation, no workspace.
 * EXPLAINN_BEST_SPAN: starts a wavefront takes per pass over its record (tests place their record lengths
 * around it).
 *
 * explainn_enrichment_test: from best_bits [units][n_records] (device uint16, read & 0x7FFF) and labels
 * (device uint8 [n_records]: 1 = primary, 0 = control, anything else leaves the record out), per unit, with
 * Np / Nc the primary / control records and N = Np + Nc:
 *     a_t = primary records with bits >= t,  b_t = control records with bits >= t       (t = 0 .. 32767)
 *     the thresholds are the m patterns t that an included record holds; at each, with n = a_t + b_t,
 *     logp(t) = 0 unless a_t N > n Np (integers), else min(0, ln P[X >= a_t]), X ~ Hypergeometric(N, Np, n):
 *     in fp64, ln of the first term from nine lgammas, plus ln of 1 + the following terms relative to it,
 *     each from the ratio (Np-x)(n-x) / ((x+1)(Nc-n+x+1)) of its predecessor, x = a_t upwards, until x
 *     reaches min(Np, n) or a term no longer changes the sum (explainn_spacing_test's rule; a threshold that
 *     is not enriched is given p = 1, not evaluated)
 * Outputs, each [units] on the device and OVERWRITTEN:
 *     n_thresholds (int32) m;  best_pattern (int32) the threshold of smallest logp, among equal values the
 *     highest pattern (0 when m == 0);  tp, fp (int64) a and b at it;  log_pvalue (double) its logp;
 *     log_padj (double) ln(1 - (1 - p)^m), computed as log(-expm1(m log1p(-p))), and as min(0, ln m +
 *     log_pvalue) when log_pvalue < -30 -- there the two differ by (m - 1) p / 2 in ln at the most: less than
 *     1e-13 relative to the value while m <= 50, and less than 1.6e-9 absolute (8e-11 relative) at the
 *     largest m = 32768; 0 when m == 0;
 *     u2 (int64) twice the Mann-Whitney U of primary over control, sum over the patterns of
 *     primary_at(t) (2 control_below(t) + control_at(t)), an exact integer;  auroc (double) u2 / (2 Np Nc).
 * counts: int64 [2], Np and Nc.  Np == 0 or Nc == 0: no threshold is enriched, the log values are 0, tp / fp
 * as counted at the highest held pattern, auroc NaN.  tails: NULL, or uint32 [units][2][32768] receiving a_t
 * and b_t.  workspace: device memory, 256-byte aligned, of explainn_enrichment_workspace_bytes(units,
 * n_records) bytes (128 KiB per workgroup of the call, not per unit).  All counts are 32-bit integer LDS
 * operations and every logp is computed by one lane: the result is a function of the input alone.  No
 * context, no allocation, no host synchronisation.  units < 0 or n_records outside [0, 2^31):
 * EXPLAINN_E_ARG (the workspace query returns 0).  units == 0 launches nothing. */
#define EXPLAINN_BEST_SPAN 256
int explainn_record_best(explainn_ctx* ctx, const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets,
                         int64_t n_records, int strands, const explainn_params* p, uint16_t* best_bits,
                         int32_t* best_site, void* stream);
int64_t explainn_enrichment_workspace_bytes(int units, int64_t n_records);
int explainn_enrichment_test(const uint16_t* best_bits, const uint8_t* labels, int units, int64_t n_records,
                             int32_t* n_thresholds, int32_t* best_pattern, int64_t* tp, int64_t* fp,
                             double* log_pvalue, double* log_padj, int64_t* u2, double* auroc, int64_t* counts,
                             uint32_t* tails, void* workspace, int64_t workspace_bytes, void* stream);

/* Motif centrality (csrc/central.hip, DESIGN.md section 3 item 19, section 8 "Centrality"): where in records
 * of one length the best sites of every unit sit, and CentriMo's test of a region that holds more of them
 * than its width explains.
 *
 * explainn_site_positions: best_bits (device uint16 [units][n_records], read & 0x7FFF) and best_site (device
 * int32 [units][n_records]: (start << 1) | is_minus, negative = no site) are explainn_record_best's outputs;
 * labels as explainn_enrichment_test takes them (1 = primary, 0 = control, anything else leaves the record
 * out); thresholds: device float [units][T], as explainn_call_sites takes them; M: the live starts of every
 * record, L - k + 1.  For every unit u, threshold t and included record r with a site,
 *     a16(u,r) > thresholds[u][t]  and  0 <= start < M:   hist[u][t][set][start] += 1
 * with a16 the float16 value of the bit pattern, compared as a float with the float threshold -- the
 * comparison of explainn_call_sites, so the record counts where call_sites with that threshold calls its
 * best site (a NaN pattern or a NaN threshold never counts) -- and set = 0 for primary, 1 for control.
 * hist: device int32 [units][T][2][M], ADDED INTO: the caller zeroes it once and accumulates calls over
 * chunks of records; a bin must stay below 2^31.  A site below 0 or a start >= M is not counted: it is never
 * a write outside hist.  counts: device int64 [2], OVERWRITTEN with (Np, Nc), the records of this call with
 * label 1 / 0, with or without a site (the caller adds them up over its calls).  The [T][2][M] histogram of
 * a workgroup sits in LDS: 1 <= T <= EXPLAINN_CENTRALITY_MAX_THRESHOLDS, M >= 1 and T*2*M*4 <= 65536 bytes,
 * else EXPLAINN_E_ARG (the caller splits the thresholds); so is units < 0 or n_records outside [0, 2^31).
 * units == 0 or n_records == 0 launches no kernel (counts is still zeroed, by a memset on the stream).  All
 * additions are integer: the result is a function of the input alone, whatever the slicing.  No context, no
 * workspace, no allocation, no host synchronisation.
 *
 * explainn_centrality_test: reads hist and counts (the sums over the calls that filled hist).  A region is a
 * range of starts [lo, hi] of w = hi - lo + 1 bins, w < M (the whole record has null probability 1 and is
 * never a region):
 *     mode 0 (centred): the regions [j, M-1-j], j >= 1;      mode 1 (local): every 0 <= lo <= hi <= M-1
 * both restricted to min_width <= w <= max_width (max_width above M - 1 reads as M - 1).  Per unit, with
 * n_t the sum of the primary row of threshold t: thresholds with n_t < max(min_sites, 1) are not tried.  For
 * a tried threshold and a region, with c the primary sites inside it,
 *     logp = 0 unless c M > n_t w (integers), else min(0, ln P[X >= c]), X ~ Binomial(n_t, q), q = w / M:
 *     in fp64, ln of the first term as lgamma(n+1) - lgamma(c+1) - lgamma(n-c+1) + c ln q + (n-c) log1p(-q),
 *     plus ln of 1 + the following terms relative to it, each its predecessor times
 *     ((n-x) / (x+1)) * (q / (1-q)), x = c upwards, until x reaches n or a term no longer changes the sum
 * (a region that is not enriched is given p = 1, not evaluated: explainn_enrichment_test's rule).  logp is a
 * function of (n_t, c, w, M) alone, so equal counts give equal bits.  Outputs, each [units] on the device and
 * OVERWRITTEN:
 *     best_t, best_lo, best_width (int32): the (threshold, region) of smallest logp; among equal values the
 *     narrower region, then the lower lo, then the lower threshold index;
 *     sites (int64) n_t and count (int64) c there;  n_tests (int64) m = tried thresholds x admissible regions;
 *     log_pvalue (double) its logp;  log_padj (double) ln(1 - (1 - p)^m), by the two branches of
 *     explainn_enrichment_test with the same switch point (log_pvalue < -30: min(0, ln m + log_pvalue));
 *     ctrl_sites, ctrl_count (int64): the sum of the control row of best_t, and its part inside the region;
 *     log_fisher (double): with (Np, Nc) = counts, ln P[X >= count], X ~ Hypergeometric(Np + Nc, Np, count +
 *     ctrl_count), summed as explainn_enrichment_test sums it, where count Nc > ctrl_count Np (integers) and
 *     Nc > 0; otherwise 0 -- also where count > Np or ctrl_count > Nc, counts that do not belong to hist.  It
 *     is evaluated at the region the binomial test chose only (CentriMo's --neg).
 * No threshold tried, or no admissible region (M == 1, or the widths leave none): best_t = best_lo =
 * best_width = 0, sites = count = n_tests = ctrl_sites = ctrl_count = 0 and the three log values 0.
 * Row sums must stay below 2^31.  One lane evaluates one (threshold, region) and the best is a minimum over
 * keys: the result is a function of the input alone.  EXPLAINN_E_ARG: the shape limits above, mode not 0 or
 * 1, min_width < 1, max_width < min_width, min_sites < 0, and in local mode more than
 * EXPLAINN_CENTRALITY_MAX_REGIONS admissible regions per unit (M (M+1) / 2 - 1 without a width limit:
 * M up to 2895 fits; the caller narrows max_width) -- the bound keeps one unit's evaluation, a lane per
 * (threshold, region), to a few milliseconds.  units == 0 launches nothing.  No context, no workspace, no
 * allocation, no host synchronisation. */
#define EXPLAINN_CENTRALITY_MAX_THRESHOLDS 16
#define EXPLAINN_CENTRALITY_MAX_REGIONS 4194304
int explainn_site_positions(const uint16_t* best_bits, const int32_t* best_site, const uint8_t* labels,
                            const float* thresholds, int units, int64_t n_records, int T, int M, int32_t* hist,
                            int64_t* counts, void* stream);
int explainn_centrality_test(const int32_t* hist, const int64_t* counts, int units, int T, int M, int mode,
                             int min_width, int max_width, int64_t min_sites, int32_t* best_t, int32_t* best_lo,
                             int32_t* best_width, int64_t* sites, int64_t* count, int64_t* n_tests,
                             double* log_pvalue, double* log_padj, int64_t* ctrl_sites, int64_t* ctrl_count,
                             double* log_fisher, void* stream);

/* The fp32 one-hot packed into the context ahead of the forward: like explainn_stage_codes, the
 * entry points then take x == NULL.  Lets the caller read explainn_input_flags BEFORE anything
 * depends on the batch -- and route a batch that is not one-hot to the dense kernels (next entry)
 * instead of running it as if its soft columns were N. */
int explainn_stage_onehot(explainn_ctx* ctx, const float* x, int B, void* stream);

/* Soft inputs.  The reference's forward takes ANY float (B,4,L) tensor (architectures/__init__.py:111
 * feeds x to a grouped Conv1d); the fast path here needs one-hot columns.  enable != 0 makes every
 * following entry point read x as a general dense tensor (csrc/dense.hip: dense input moments,
 * dense filter bank + pooling, dense filter-gradient scatter, dense activations; everything behind
 * the pooled activations is the regular pipeline) -- same results, to rounding, as the fast path
 * gives on one-hot x.  x must stay valid until the backward of a train forward has been enqueued.
 * The filter -> PWM export (explainn_filter_*) has no dense form: EXPLAINN_E_UNSUPPORTED. */
int explainn_dense_input(explainn_ctx* ctx, int enable);

/* PWM scan: the reference's `PWM` module forward (architectures/__init__.py:157-168).
 * x: fp32 (B,4,L) rows A,C,G,T; pwms: fp32 (G,4,k); scores: fp32 (B,G) = max (EXPLAINN_PWM_MAX) or
 * sum (EXPLAINN_PWM_SUM) of the window scores over both strands.  No context needed. */
#define EXPLAINN_PWM_SUM 0
#define EXPLAINN_PWM_MAX 1
int explainn_pwm_scan(const float* x, int B, int L, const float* pwms, int G, int k, int scoring,
                      float* scores, void* stream);

/* Dinucleotide-preserving shuffles (csrc/shuffle.hip).
 * out[i][r][:] = r-th dinucleotide-preserving shuffle of codes[i][:]: the same first and last symbol and
 * the same count of every ordered pair of adjacent symbols; every distinct such arrangement equally
 * likely.  codes: device uint8 (N,L), 0..3 = A,C,G,T, anything else = N, a fifth symbol, written back
 * as 4.  out: device uint8 (N,R,L), OVERWRITTEN.  The result is a pure function of
 * (seed, row0 + i, r, the row's codes): independent of N, R, launch geometry and of how a caller
 * splits its rows into calls.  capped: device uint8 (N,R) or NULL; 1 where the tree sampler reached
 * max_rounds and the row's own last exits were used (still a valid shuffle, not a uniform one).
 * max_rounds <= 0 means the default 64*L.  L < 3 copies the row.  N < 0, L < 1, R < 1: EXPLAINN_E_ARG.
 * N = 0 launches nothing.  More than 2^37 (row, r) pairs in one call: EXPLAINN_E_UNSUPPORTED (split the
 * rows).  No context, no workspace, no allocation, no host synchronisation. */
int explainn_dinucleotide_shuffle(const uint8_t* codes, int64_t N, int L, int R, uint64_t seed,
                                  int64_t row0, int max_rounds, uint8_t* out, uint8_t* capped,
                                  void* stream);

/* Motif comparison (csrc/motifs.hip): the best ungapped alignment of every query
 * motif with every target motif by width-normalised Pearson correlation, the score RSAT compare-matrices
 * and matrix-clustering call Ncor.
 * A set of M motifs: fp32 (M,wmax,4), rows A,C,G,T per column, non-negative counts or probabilities, and
 * int32 widths[M], 0 <= w <= wmax <= EXPLAINN_MOTIF_MAX_WIDTH; columns from w on are ignored.
 * Per column f[a] = (c[a] + pc/4) / (sum c + pc), 0.25 where that denominator is 0; d = f - 0.25;
 * n = sum_a d[a]^2.  An alignment (s, o): strand s = 1 takes the target's reverse complement; query column
 * i meets target column i + o; over the overlap of size w, XY = sum d_q.d_t, SX = sum n_q, SY = sum n_t,
 * cor = XY / sqrt(SX SY) (0 when SX or SY is below EXPLAINN_MOTIF_VAR_FLOOR), Ncor = cor w / (wq + wt - w).
 * Admissible: w >= 1 and w >= min(min_overlap, wq, wt).  The best alignment is the admissible one with the
 * largest Ncor, ties to strand 0, then to the smaller offset; a pair with a width of 0 gives zeros.
 * both_strands == 0 searches strand 0 only.
 * ncor, cor: fp32 (Q,T); align: int16 (Q,T,3) = offset, strand, overlap.  Outputs are OVERWRITTEN; cor and
 * align may be NULL.  t == NULL compares the queries with themselves (T must then equal Q; t_widths is
 * not read).  workspace: device memory, 16-byte aligned, of explainn_motif_compare_workspace_bytes(Q,T,wmax)
 * bytes, dead after the call.  No context, no allocation, no host synchronisation; the same input gives the
 * same bits on every call.  Q, T < 0, wmax < 1, min_overlap < 1, pseudocount < 0: EXPLAINN_E_ARG;
 * wmax > EXPLAINN_MOTIF_MAX_WIDTH: EXPLAINN_E_UNSUPPORTED; a width outside [0,wmax] is found on the device
 * and makes that motif one of width 0.  Q == 0 or T == 0 launches nothing. */
#define EXPLAINN_MOTIF_MAX_WIDTH 64
#define EXPLAINN_MOTIF_VAR_FLOOR 1e-6f
int64_t explainn_motif_compare_workspace_bytes(int Q, int T, int wmax);
int explainn_motif_compare(const float* q, const int32_t* q_widths, int Q, const float* t,
                           const int32_t* t_widths, int T, int wmax, float pseudocount, int min_overlap,
                           int both_strands, float* ncor, float* cor, int16_t* align, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* Motif significance (csrc/motifs.hip): the p-value of the best alignment of
 * every query with every target under the null of Gupta et al. 2007 (Tomtom with incomplete scores, column
 * similarity Pearson).  Motif sets, pseudocount, strands, offsets, overlap and admissibility are those of
 * explainn_motif_compare.  A column's unit vector is u = d / sqrt(n) (0 where n < EXPLAINN_MOTIF_VAR_FLOOR);
 * the score of two columns is c = u_q.u_t in [-1,1], quantised to b = clamp(floor((c + 1) bins/2 + 0.5), 0,
 * bins).  The database is every column of every target of width > 0, and of its reverse complement when
 * both_strands; N columns.  h[q][i][b] is the share of database columns that score b against query column i;
 * the null of the sum over query columns [lo, lo+w) is the convolution of their h, SF its upper tail
 * (clamped to 1).  An alignment scores S = sum of b over its overlap and p_align = SF_{lo,w}(S).  The pair's
 * alignment is the admissible one with the smallest p_align, ties to strand 0, then to the smaller offset;
 * pvalue = 1 - (1 - p_align)^n_align over the n_align admissible alignments of the pair (both strands
 * counted), computed as -expm1(n_align log1p(-p_align)).  A pair with a width of 0 gives pvalue 1 and zeros.
 * The score range is fixed at [-1,1] (not rescaled per query as the MEME program does), everything after the
 * quantisation is fp64, and a p-value below the fp64 range is reported as 0.
 * pvalue: double (Q,T); align: int16 (Q,T,3) = offset, strand, overlap; score: int32 (Q,T) = S.  For checks
 * of the stages: colscore: uint8 (Q,wmax,S,wmax,T), S = 2 with both_strands else 1 -- query column i of q
 * against column j of the strand-s view of target t, EXPLAINN_MOTIF_NO_SCORE where either column does not
 * exist (every entry is written); hist: int32 (Q,wmax,bins+1), the counts N h (zeros past a query's width).
 * Outputs are OVERWRITTEN; align, score, colscore and hist may be NULL and are then not written.
 * t == NULL takes the queries as the database (T must then equal Q).  workspace: device memory, 16-byte
 * aligned, of explainn_motif_significance_workspace_bytes(Q,T,wmax,bins,both_strands) bytes (0 for arguments
 * the call would refuse), dead after the call; it grows with Q, and the null depends on the targets alone,
 * so a caller short of memory splits the queries and gets the same bits.  No context, no allocation, no host
 * synchronisation; the same input gives the same bits on every call.  Errors as explainn_motif_compare's,
 * and bins outside [2, EXPLAINN_MOTIF_MAX_BINS]: EXPLAINN_E_ARG.  Q == 0 or T == 0 launches nothing. */
#define EXPLAINN_MOTIF_MAX_BINS 128
#define EXPLAINN_MOTIF_NO_SCORE 255
int64_t explainn_motif_significance_workspace_bytes(int Q, int T, int wmax, int bins, int both_strands);
int explainn_motif_significance(const float* q, const int32_t* q_widths, int Q, const float* t,
                                const int32_t* t_widths, int T, int wmax, float pseudocount, int min_overlap,
                                int both_strands, int bins, double* pvalue, int16_t* align, int32_t* score,
                                uint8_t* colscore, int32_t* hist, void* workspace, int64_t workspace_bytes,
                                void* stream);

/* Motif tree and merged cluster motifs (csrc/motiftree.hip, DESIGN.md section 3, "Motif tree"): agglomerate
 * the M motifs of a self-comparison, cut the tree, place every member in its cluster's frame and pool the
 * placed matrices.  Context-free; no allocation, no host synchronisation; integer-exact, so the same input
 * gives the same bits on every call.
 * Input: ncor fp32 (M,M) and align int16 (M,M,3) as explainn_motif_compare writes them (the upper triangle is
 * read: q[i][j] = (int32) rintf(ncor[i][j] 2^20), (offset, strand) of the pair for i < j) and int32 widths[M],
 * taken as they are.  Linkage of two clusters over their leaf pairs: SINGLE max q, COMPLETE min q, AVERAGE
 * (double) sum q / (double) pairs.  A cluster's slot is its smallest leaf; of the live pairs lo < hi the one with
 * the largest linkage merges into slot lo, ties to the smaller lo, then the smaller hi; M - 1 steps.  The best
 * leaf pair (i < j) of a step is the one with the largest q across the two clusters, ties to the smaller i, then
 * j.  Placement: leaf x at (f, h) has column c of rc^f(m_x) in frame column h + c; the pair's (s, o) says that
 * in a frame where i is (0,0), j is (s,-o); a step keeps cluster lo and sends every leaf of hi through
 * f ^= F, h = (F ? -(h + w) : h) + H so that the best pair meets as compared.
 * explainn_motif_tree writes log int32 (M-1,8) = lo, hi, leaves of the merged cluster, leaf_i, leaf_j, F, H, 0;
 * link int64 (M-1,2) = sum, pairs ((q, 1) for SINGLE and COMPLETE; height = sum / pairs / 2^20); gone int32 [M],
 * the step that merged slot c away (-1: never); flips, shifts int32 [M], every leaf in the root's frame.
 * workspace: 16-byte aligned, explainn_motif_tree_workspace_bytes(M, linkage) bytes (two M x M matrices of 8
 * bytes; 0 for arguments the call refuses), dead after the call.  One workgroup runs the M - 1 steps.
 * M < 0, an unknown linkage, a short workspace: EXPLAINN_E_ARG; M > EXPLAINN_MOTIF_TREE_MAX_LEAVES:
 * EXPLAINN_E_UNSUPPORTED.  M == 0 launches nothing.
 * explainn_motif_tree_cut: a step is above the cut when sum >= threshold pairs (threshold = ceil(min_ncor 2^20),
 * at least 1, else EXPLAINN_E_ARG).  Per leaf: labels = the slot of its cluster at the cut, flips and shifts in
 * that cluster's frame, the shifts moved so that the smallest of a cluster is 0; per slot that is a cluster,
 * slot_hi - slot_lo is the cluster's span (other slots hold INT32_MAX, INT32_MIN).  All int32 [M], overwritten.
 * explainn_motif_tree_pool: x fp32 (M,wmax,4) and widths as explainn_motif_compare's (a width outside
 * [0,wmax] is a width of 0), labels / flips / shifts as the cut wrote them, cluster_slots int32 [C] the slots of
 * the clusters to pool; merged double (C,span,4): per (column, base) the sum over the members in ascending leaf
 * order of the placed entries, plain fp64 adds; support int32 (C,span): members covering the column.  Columns
 * at or past span are dropped.  Overwritten.  M, C, span < 0, C > M, wmax outside [1, EXPLAINN_MOTIF_MAX_WIDTH]:
 * EXPLAINN_E_ARG.  C == 0 or span == 0 launches nothing. */
#define EXPLAINN_LINKAGE_SINGLE 0
#define EXPLAINN_LINKAGE_COMPLETE 1
#define EXPLAINN_LINKAGE_AVERAGE 2
#define EXPLAINN_MOTIF_TREE_MAX_LEAVES 12288
int64_t explainn_motif_tree_workspace_bytes(int M, int linkage);
int explainn_motif_tree(const float* ncor, const int16_t* align, const int32_t* widths, int M, int linkage,
                        int32_t* log, int64_t* link, int32_t* gone, int32_t* flips, int32_t* shifts,
                        void* workspace, int64_t workspace_bytes, void* stream);
int explainn_motif_tree_cut(const int32_t* log, const int64_t* link, const int32_t* gone, const int32_t* widths,
                            int M, int threshold, int32_t* labels, int32_t* flips, int32_t* shifts,
                            int32_t* slot_lo, int32_t* slot_hi, void* stream);
int explainn_motif_tree_pool(const float* x, const int32_t* widths, const int32_t* labels, const int32_t* flips,
                             const int32_t* shifts, const int32_t* cluster_slots, int M, int wmax, int C, int span,
                             double* merged, int32_t* support, void* stream);

/* Known-motif sites (csrc/pwmsites.hip, DESIGN.md section 8, "Known-motif sites"): where the motifs of a
 * database occur in a sequence, at an exact p-value cutoff -- what FIMO lists.  A motif is an integer score
 * table: scores, device int16 (M,wmax,4), rows A,C,G,T per column, every entry in [0, bins], and int32
 * widths[M]; a width outside [1, wmax] is found on the device and makes the motif EMPTY (no sites).  The host
 * quantises log-odds to these integers (explainn_amd/pwmsites.py); 1 <= wmax <= EXPLAINN_MOTIF_MAX_WIDTH and
 * 1 <= bins <= EXPLAINN_MOTIF_MAX_BINS, so a site's score is at most 8192.
 *
 * explainn_pwm_null: per motif m of width w, the distribution of the score of a random w-mer drawn iid from
 * the background (bg_a .. bg_t, each in (0,1]; the caller makes them sum to 1), column by column in fp64:
 *     pdf_0 = [1];   pdf_{j+1}[s] = sum_{a = A,C,G,T in this order} bg[a] pdf_j[s - scores[m][j][a]]
 *     tail[m][s] = sum_{s' >= s} pdf_w[s']            for 0 <= s <= w bins, 0 beyond
 *     thresholds[m] = the smallest s with tail[m][s] <= pcut;  w bins + 1 if there is none
 * All terms are non-negative and every sum has a fixed order (no atomics on floats): the same input gives the
 * same bits.  An empty motif has an all-zero tail row and thresholds[m] = 1 (0 bins + 1).  tail: device double
 * [M][wmax bins + 2], may be NULL; thresholds: device int32 [M].  pcut outside [0,1] (or NaN), a background
 * frequency outside (0,1], M < 0 or wmax / bins outside their ranges: EXPLAINN_E_ARG.  M == 0 launches nothing.
 *
 * explainn_pwm_sites: seq, seq_len, start, n_positions and period as explainn_call_sites takes them, except
 * that the call may end at the sequence's end: it needs start + n_positions <= seq_len only, and reads the
 * bases [start, min(start + n_positions + wmax - 1, seq_len)).  Codes 0..3 = ACGT; 4 and every byte above it = N.
 * Rows r = 2m + (strand is '-'):
 *     row 2m    at start p scores  sum_{j<w} scores[m][j][seq[p+j]]
 *     row 2m+1  at start p scores  sum_{j<w} scores[m][j][3 - seq[p+w-1-j]]    (the reverse complement of
 *               seq[p : p+w]; the same forward coordinate p); empty when both_strands == 0
 * A start is not live for motif m when its w bases run past the bases the call reads, when its window holds
 * an N, or, with period > 0, when p mod period > period - w (the rule of explainn_call_sites with the
 * motif's own width).  A live start with score >= thresholds[m] is a site.
 * offsets: int64 [2M+1], device, always written: the exclusive scan of the FULL per-row counts -- the
 * offsets2 layout explainn_site_spacing reads.  pos (int32, start-relative), score (int32, may be NULL) and
 * pvalue (double, may be NULL, needs tail: tail[m][score] of explainn_pwm_null's table with the same wmax and
 * bins): record offsets[r] + i is the i-th site of row r in ascending position; records with index >= capacity
 * are not written.  pos == NULL: count only.  Order and bits are a function of the input alone (counts, scans
 * and ballots in position order).  workspace: device memory, 256-byte aligned, of
 * explainn_pwm_sites_workspace_bytes(M, n_positions) bytes.  No context, no allocation, no host
 * synchronisation.  EXPLAINN_E_ARG unless 0 <= start, start + n_positions <= seq_len, n_positions + wmax < 2^31,
 * period >= 0, capacity >= 0 and 0 <= M <= 65535 EXPLAINN_PWM_GROUP.  M == 0 or n_positions == 0 zeroes offsets.
 * EXPLAINN_PWM_GROUP: motifs per workgroup (tests place their motif counts around it). */
#define EXPLAINN_PWM_GROUP 16
int explainn_pwm_null(const int16_t* scores, const int32_t* widths, int M, int wmax, int bins, double bg_a,
                      double bg_c, double bg_g, double bg_t, double pcut, double* tail, int32_t* thresholds,
                      void* stream);
int64_t explainn_pwm_sites_workspace_bytes(int M, int64_t n_positions);
int explainn_pwm_sites(const uint8_t* seq, int64_t seq_len, int64_t start, int64_t n_positions, int64_t period,
                       int both_strands, const int16_t* scores, const int32_t* widths, int M, int wmax,
                       const int32_t* thresholds, const double* tail, int bins, int64_t* offsets, int32_t* pos,
                       int32_t* score, double* pvalue, int64_t capacity, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* The observed score histogram of known motifs (csrc/pwmsites.hip, DESIGN.md section 8, "Site q-values"): every
 * test explainn_pwm_sites would make, counted by its integer score -- the sites and all the windows that are none.
 *
 * explainn_pwm_score_histogram: seq, seq_len, start, n_positions, period and both_strands, and scores, widths, M,
 * wmax and bins, as explainn_pwm_sites takes them.  For every motif m and every start p that is live for m there
 * (its w bases inside the bases the call reads, no N, inside its record):
 *     hist[m][score of row 2m at p] += 1,   and with both_strands != 0   hist[m][score of row 2m+1 at p] += 1
 * (each strand is a test).  An empty motif counts nothing, so sum_s hist[m][s] grows by the number of tests of m.
 * hist: device int64 [M][wmax bins + 2], the row stride of explainn_pwm_null's tail, ADDED INTO: the caller zeroes
 * it once and may accumulate any number of calls, chunks, records and files.  A score outside the row -- possible
 * only with a table entry outside [0, bins] -- is not counted.  All additions are integer (32-bit counters in LDS,
 * flushed with 64-bit atomics): the result is a function of the input alone, whatever the grid, and whatever
 * chunks a caller cuts.  A workgroup holds as many motifs' rows as the 160 KB of LDS allow beside their tables and
 * a tile's codes (EXPLAINN_PWM_GROUP at the most, four for the largest row) and takes at most
 * EXPLAINN_PWM_HIST_SLICE starts, two counts each, so no 32-bit counter overflows.  No context, no workspace, no
 * allocation, no host synchronisation.  EXPLAINN_E_ARG as explainn_pwm_sites (geometry, 0 <= start, start +
 * n_positions <= seq_len, n_positions + wmax < 2^31, period >= 0).  M == 0 or n_positions == 0 launches nothing. */
#define EXPLAINN_PWM_HIST_SLICE (1 << 30)
int explainn_pwm_score_histogram(const uint8_t* seq, int64_t seq_len, int64_t start, int64_t n_positions,
                                 int64_t period, int both_strands, const int16_t* scores, const int32_t* widths,
                                 int M, int wmax, int bins, int64_t* hist, void* stream);

/* Site q-values (csrc/siteq.hip, DESIGN.md section 8, "Site q-values"): the Benjamini-Hochberg q-value of every
 * score bin of every unit, for filter sites (bins = EXPLAINN_ACT_BINS bit patterns) and known-motif sites (bins =
 * wmax bins + 2 integer scores) alike.  obs: device int64 [units][bins], the tests of unit u that scored in bin b
 * (all of them: explainn_activation_histogram / explainn_pwm_score_histogram of the scanned sequences), none
 * negative; p: device double [units][bins], the p-value of the bin, not NaN, which the caller's null makes
 * non-increasing in b.  With N = sum_b obs[u][b] and R[b] = sum_{b' >= b} obs[u][b']:
 *     q[u][b]  = min(1, min over b' <= b with R[b'] > 0 of (p[u][b'] * (double) N) / (double) R[b'])     (1 if none)
 *     total[u] = N
 *     first[u] = the number of b with q[u][b] > alpha = the smallest b with q[u][b] <= alpha (bins if none)
 * Bins of equal p need no tie rule: the lower one has the larger R and lies inside the minimum.  This is BH over
 * all N tests of the unit -- it does not depend on a p-value cutoff, as a q-value estimated from a truncated site
 * list does.  Every term is one fp64 multiply and one fp64 divide, every sum is an integer sum and a minimum is
 * exact: the same input gives the same bits, those of the expression above evaluated in IEEE double.
 * q: device double [units][bins]; total: device int64 [units]; first: device int32 [units], may be NULL.
 * EXPLAINN_E_ARG unless units >= 0, 1 <= bins <= EXPLAINN_SITEQ_MAX_BINS and 0 <= alpha <= 1.  units == 0 launches
 * nothing.  No context, no workspace, no allocation, no host synchronisation, no atomics on floats. */
#define EXPLAINN_SITEQ_MAX_BINS 32768
int explainn_site_qvalues(const int64_t* obs, const double* p, int units, int bins, double alpha, double* q,
                          int64_t* total, int32_t* first, void* stream);

/* Known-motif enrichment and centrality (csrc/pwmbest.hip, DESIGN.md section 3 item 21, section 8 "Known-motif
 * enrichment"): explainn_record_best for the score tables of explainn_pwm_sites in place of a model's filters.
 *
 * explainn_pwm_record_best: seq, seq_len, rec_offsets and n_records as explainn_record_best takes them (device
 * base codes; device int64 [n_records + 1]; record r is seq[rec_offsets[r] : rec_offsets[r+1]]); scores, widths, M
 * and wmax as explainn_pwm_sites takes them (int16 (M,wmax,4), entries in [0, bins]; a width outside [1, wmax]
 * makes the motif EMPTY).  Codes 0..3 = ACGT; 4 and every byte above it = N.  For motif m of width w, record r
 * and a start p relative to the record:
 *     '+' scores  sum_{j<w} scores[m][j][seq[p+j]]
 *     '-' scores  sum_{j<w} scores[m][j][3 - seq[p+w-1-j]]     (row 2m+1 of explainn_pwm_sites: the reverse
 *                 complement of the same w bases, reported at the same forward p); not taken when both_strands == 0
 * A start is live when its w bases lie inside the record and hold no N.
 *     best_bits[m][r] (uint16) = the largest score over the record's live starts and the requested strands
 *     best_site[m][r] (int32; may be NULL) = (p << 1) | is_minus of the maximum
 * Among equal maxima the lowest start wins, and at one start '+' before '-' (explainn_record_best's key: score,
 * then ~start, then is_plus).  No live start -- a record shorter than w, a record with an N in every window, an
 * empty motif --: bits 0, site -1.  A record whose offsets descend or leave [0, seq_len], or of 2^30 bases or more,
 * reads as having no live start for every motif and ORs bit 0 into *flags (device int32, may be NULL; never
 * cleared here); the check is a compare before any read of seq.  Both outputs are unit-major [M][n_records] and
 * OVERWRITTEN: the layout explainn_enrichment_test and explainn_site_positions read (a score is at most 8192: a
 * 15-bit pattern that sorts like the score).  The result is a maximum over integer keys: a function of the
 * input alone.  EXPLAINN_E_ARG unless seq_len >= 0, 0 <= n_records < 2^31, 0 <= M <= 65535 EXPLAINN_PWM_GROUP and
 * 1 <= wmax <= EXPLAINN_MOTIF_MAX_WIDTH.  M == 0 or n_records == 0 launches nothing.  No context, no workspace,
 * no allocation, no host synchronisation.
 * EXPLAINN_PWM_BEST_SPAN: starts a wavefront takes per pass over its record (tests place their record lengths
 * around it). */
#define EXPLAINN_PWM_BEST_SPAN 256
int explainn_pwm_record_best(const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets, int64_t n_records,
                             int both_strands, const int16_t* scores, const int32_t* widths, int M, int wmax,
                             uint16_t* best_bits, int32_t* best_site, int32_t* flags, void* stream);

/* Variant effects on known motifs (csrc/pwmvariants.hip, DESIGN.md section 3 item 25, section 8 "Variant effects
 * on known motifs"): explainn_pwm_record_best for the two haplotypes of every variant, restricted to the windows
 * the allele touches; neither haplotype is materialised.
 *
 * explainn_pwm_variant_best: seq / seq_len are device base codes; pos (int64), ref_len, alt_len, alt_off (int32) and
 * alt (uint8, alt_bytes of them) are the edit table of explainn_edits, one record per variant, all on the device;
 * scores, widths, M and wmax as explainn_pwm_record_best takes them.  For variant v and allele A -- index 0 the
 * reference with l = ref_len[v], index 1 the alternative with l = alt_len[v] -- the haplotype is
 *     H_A = seq[:pos] + allele + seq[pos + ref_len:]          of n_A = seq_len - ref_len + l bases
 * and a motif of live width w has the starts s = pos - w + 1 + i, i = 0 .. w + l - 2: with l >= 1 the windows that
 * overlap the allele, with l == 0 the w - 1 windows that span the junction (none for w == 1).  A start is live when
 * 0 <= s, s + w <= n_A and the window holds no N.  '+' and '-' score as in explainn_pwm_record_best.
 *     best_bits[m][v][A] (uint16) = the largest score over the live starts and the requested strands, 0 without one
 *     best_site[m][v][A] (int32; may be NULL) = (i << 1) | is_minus of the maximum, -1 without a live start
 * Among equal maxima the lowest i wins, and at one start '+' before '-' (explainn_record_best's key with i in place
 * of the start): a maximum over integer keys, the same bits for any grid.  Both outputs are [M][n_variants][2] and
 * OVERWRITTEN.  The host never reads the tables, so the kernel stays inside its arrays on bad ones: a source index
 * outside [0, seq_len) reads as N; a byte above 4 reads as N and ORs bit 0 into *flags (device int32, may be NULL;
 * never cleared here) when it lies in seq within wmax - 1 bases of an allele or in the alt allele itself; a variant
 * with pos < 0, a negative length, pos + ref_len > seq_len, alt_off < 0, alt_off + alt_len > alt_bytes or an
 * allele longer than EXPLAINN_PWM_VARIANT_MAX_ALLELE ORs bit 1 into *flags and has no site on either allele for
 * every motif -- compares only, before any byte of its alleles is read.  EXPLAINN_E_ARG unless seq_len >= 0,
 * alt_bytes >= 0, 0 <= n_variants < 2^30, 0 <= M <= 65535 EXPLAINN_PWM_GROUP and 1 <= wmax <=
 * EXPLAINN_MOTIF_MAX_WIDTH.  M == 0 or n_variants == 0 launches nothing.  No context, no workspace, no allocation,
 * no host synchronisation, no atomics but the flags. */
#define EXPLAINN_PWM_VARIANT_MAX_ALLELE 128
int explainn_pwm_variant_best(const uint8_t* seq, int64_t seq_len, const int64_t* pos, const int32_t* ref_len,
                              const int32_t* alt_len, const int32_t* alt_off, const uint8_t* alt, int64_t alt_bytes,
                              int64_t n_variants, int both_strands, const int16_t* scores, const int32_t* widths,
                              int M, int wmax, uint16_t* best_bits, int32_t* best_site, int32_t* flags, void* stream);

/* De novo word discovery (csrc/words.hip, DESIGN.md section 3 item 26, section 8 "Word discovery"): which k-mers
 * occur in more records of a primary set than of a control set, and the sites of the best one widened by its
 * enriched one-mismatch neighbours -- the three device steps of explainn_amd/discover.py's DREME-style loop.
 * seq, seq_len, rec_offsets and n_records as explainn_pwm_record_best takes them.
 *
 * Word code.  Base codes are A,C,G,T = 0..3, and any byte >= 4 is "not a base".  A k-mer's code is
 * sum b_i 4^(k-1-i), first base most significant; rc(code) is the code of the reverse complement.  With both
 * strands a word is indexed by its canonical code min(code, rc(code)), and non-canonical entries of a table stay
 * 0; with both_strands == 0 it is indexed by code.  EXPLAINN_WORD_MIN_WIDTH <= k <= EXPLAINN_WORD_MAX_WIDTH.
 * Live start.  Start s of record r is live when the k bases s .. s+k-1 lie inside the record and all are < 4.
 *
 * explainn_word_counts: presence counts.  counts[w] (int32 [4^k], ADDED INTO, so files accumulate) grows by the
 * number of records with at least one live start whose (canonical) code is w: a record counts once however often
 * the word occurs in it.
 *
 * explainn_word_test: for the counts a = pos[w], b = neg[w] (int32 [n_words]) and the record totals Np, Nc
 *     logp[w] = hypergeom_logsf(a, a+b, Np, Nc) (csrc/tails.h: ln P[X >= a], X ~ Hypergeometric(Np+Nc, Np, a+b))
 *               when a >= min_count and the primary set is enriched, a (Np+Nc) > (a+b) Np in integers;
 *               otherwise exactly 0.0 (also for an entry outside 0 <= a <= Np, 0 <= b <= Nc)
 *     best[0] = the word of the smallest logp, ties to the lowest code; -1 when no entry is below 0
 *     best[1] = n_tested, the number of entries with a + b > 0
 *     best_logp[0] = that smallest logp, 0.0 without one
 * logp (double [n_words]), best (int64 [2]) and best_logp (double [1]) are OVERWRITTEN.  Equal counts give
 * bit-equal values, and the minimum and the tie rule are integer atomics: the same answer for any grid.
 *
 * explainn_word_sites: the sites of the pattern (k, seed, accept) in one set.  accept is a bit mask with bit
 * 4 i + b for motif position i (0 = first base) and base b.  A window with code c MATCHES when its Hamming
 * distance to seed is 0, or when it is 1 with the differing position i holding base b and bit 4i+b of accept set.
 * A start is a SITE when it is live and its window matches ('+'), or, with both strands, when rc(window) matches
 * ('-'); a start that matches both ways is one '+' site.
 *     totals[0] += nsites, the number of sites (overlapping sites all count)
 *     totals[1] += nrecords, the number of records with at least one site          (int64 [2], ADDED INTO)
 *     pfm[i][b] += the sites with base b at motif position i, a '-' site contributing 3 - base[start + k-1-i]
 *                                                                (int64 [k][4], ADDED INTO; may be NULL)
 *     seq_out[0 .. seq_len) = seq with every base covered by at least one site replaced by 4 and every other
 *                             byte copied (may be NULL; another array than seq).  It is decided on the input
 *                             alone, in gather form, one output byte per lane, so overlaps cannot race.
 *
 * flags (device int32, may be NULL; ORed into, never cleared here) of word_counts and word_sites: bit 0 = a byte
 * above 4 was read (it reads as N; every byte of a record of at least k bases is read); bit 1 = a record whose
 * offsets are not 0 <= o[r] <= o[r+1] <= seq_len was skipped -- a compare before any byte of it is read; it
 * contributes nothing.  EXPLAINN_E_ARG, without a launch, for k outside its range, negative sizes, Np + Nc >=
 * 2^31, n_words > 4^EXPLAINN_WORD_MAX_WIDTH, a seed outside [0, 4^k), an accept bit from 4k on and null required
 * pointers.  n_records == 0 counts nothing (word_sites still copies seq).  No context, no workspace, no
 * allocation, no host synchronisation; every sum is an integer atomic, so the results are functions of the input.
 * EXPLAINN_WORD_SPAN: starts a workgroup takes per pass over its record (tests place repeats around it). */
#define EXPLAINN_WORD_MIN_WIDTH 3
#define EXPLAINN_WORD_MAX_WIDTH 10
#define EXPLAINN_WORD_SPAN 256
int explainn_word_counts(const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets, int64_t n_records, int k,
                         int both_strands, int32_t* counts, int32_t* flags, void* stream);
int explainn_word_test(const int32_t* pos, const int32_t* neg, int64_t n_words, int64_t Np, int64_t Nc,
                       int64_t min_count, double* logp, int64_t* best, double* best_logp, void* stream);
int explainn_word_sites(const uint8_t* seq, int64_t seq_len, const int64_t* rec_offsets, int64_t n_records, int k,
                        int both_strands, int64_t seed, uint64_t accept, uint8_t* seq_out, int64_t* pfm,
                        int64_t* totals, int32_t* flags, void* stream);

/* One Adam step over n_tensors parameter tensors in a single launch -- torch.optim.Adam(params, lr)
 * with its defaults, the optimiser the reference builds (architectures/__init__.py:463-464) and
 * steps at selene/__init__.py:291.  params/grads/exp_avg/exp_avg_sq: HOST arrays of n_tensors
 * device pointers (fp32, contiguous), sizes: HOST array of element counts; step: 1 for the first
 * update; the hyper-parameters are doubles because torch derives 1-beta and the bias corrections
 * from Python floats (1.f - 0.999f is off by 5e-5).  No context needed. */
int explainn_adam_step(int n_tensors, float* const* params, const float* const* grads,
                       float* const* exp_avg, float* const* exp_avg_sq, const int64_t* sizes,
                       int64_t step, double lr, double beta1, double beta2, double eps, void* stream);

/* Input validation result of every pack since the last call: bit 0 set = some column of x was
 * neither one-hot nor all-zero (such columns were treated as N); bit 1 (EXPLAINN_FLAG_BN1_TIMEOUT)
 * set = a train forward's BatchNorm1 statistics, computed inside the filter-bank launch, gave up
 * waiting for the input moments (bounded wait: that step's BatchNorm1 fold was skipped and its
 * results are invalid).  Synchronises `stream`, writes the flags to *flags_host and clears them. */
#define EXPLAINN_FLAG_BN1_TIMEOUT 2
int explainn_input_flags(explainn_ctx* ctx, int* flags_host, void* stream);

/* Measurement aid (bench.py's per-kernel roofline; the reference only logs steps per second,
 * selene/__init__.py:296-304): with timing enabled every stage of the training step is bracketed
 * by HIP events on the launch stream; explainn_stage_times synchronises the device and returns
 * the microseconds of each stage of the LAST step (-1 for stages that did not run), in the order
 * of explainn_stage_name(0 .. explainn_stage_count()-1).  Off by default: the events cost a few
 * microseconds per stage. */
int explainn_stage_timing(explainn_ctx* ctx, int enable);
int explainn_stage_count(void);
const char* explainn_stage_name(int i);
int explainn_stage_times(explainn_ctx* ctx, float* us, int cap);

/* Test aid for the built-in dropout generator (architectures/__init__.py:92 nn.Dropout(0.3); the
 * reference exposes no mask either -- torch draws it inside the op).  After a train-mode forward
 * of B sequences, copies the per-(unit, sequence) 100-bit words "pre-activation > 0 AND kept by
 * dropout" the backward will use into out: device, uint32 (U, B, 4), channel r = bit (r & 31) of
 * word r >> 5.  With BatchNorm2's weight = 0 and bias > 0 every pre-activation is positive and the
 * words ARE the keep mask (tests/test_gpu_parity.py measures its rate, scaling and independence
 * that way).  EXPLAINN_E_STATE without a train forward of that batch size in flight. */
int explainn_debug_keep_bits(explainn_ctx* ctx, int B, uint32_t* out, void* stream);

/* Sync-BN: a training step over R shards of one batch that computes what one
 * device computes on the concatenated batch -- every BatchNorm takes the WHOLE batch's statistics.
 * The step runs as EXPLAINN_SYNC_PHASES phases.  Phase i writes this rank's contribution to the
 * exchange X_i (exchange_out: explainn_sync_exchange_elems(ctx, i) fp64, device; 0 = the phase
 * writes none); the caller SUMS X_i over the ranks in place, in the same order on every rank, and
 * hands the sum to the next phase that runs (exchange_in).  The layout of X_i depends on the
 * context's shape only, never on B_local, so uneven shards add.  Phases: 1 pack + input moments,
 * 2 BatchNorm1 + filter bank + q moments, 3 BatchNorm2 + FC, 4 BatchNorm3 + combiner (logits: the
 * forward ends here), 5 loss gradient + head sums, 6 BatchNorm3 backward + passA, 7 mid + passB +
 * filter-gradient sums, 8 the filter / BatchNorm1 gradients.  After phase 8 all 14 gradients are
 * those of the whole batch on every rank: no gradient all-reduce follows.
 *   B_local >= 1 sequences of this rank, B_global >= 2 of all ranks (the normaliser of every mean);
 *   x: one-hot (B_local,4,L) or NULL for staged codes (phase 1); keep_mask / dropout_p / seed as in
 *   explainn_forward_train (phase 3); logits: (B_local,T) out (phase 4, read again by phase 5);
 *   phase 5 either takes dlogits (the caller's d loss / d logits, multiplied by dl_scale -- the
 *   autograd path passes B_local/B_global to turn a shard-mean loss into the global mean) or, with
 *   dlogits == NULL, computes the gradient of the global mean loss of kind loss_kind from targets;
 *   the loss value (loss_out, device float) then comes out of phase 6.
 * Soft (dense) input is not supported (EXPLAINN_E_UNSUPPORTED). */
#define EXPLAINN_SYNC_PHASES 8
typedef struct explainn_sync_args {
    const float* x;
    const float* targets;
    const float* dlogits;
    float dl_scale;
    int B_local, B_global;
    const explainn_params* params;
    const explainn_grads* grads;
    int loss_kind;
    float dropout_p;
    uint64_t seed;
    const uint8_t* keep_mask;
    int freeze_top_n_filters;
    float* logits;
    float* loss_out;
} explainn_sync_args;
int64_t explainn_sync_exchange_elems(const explainn_ctx* ctx, int phase);
int explainn_sync_phase(explainn_ctx* ctx, int phase, const explainn_sync_args* args,
                        const double* exchange_in, double* exchange_out, void* stream);

/* Evaluation metrics on the device (the reference's test.py::_get_performances and the callables of
 * architectures.get_metrics, which run scikit-learn / scipy on host copies).  y (targets) and s
 * (scores): contiguous row-major fp32 (N,T) device arrays.  mode EXPLAINN_METRICS_PER_TASK: T
 * results, one per column of length N; EXPLAINN_METRICS_GLOBAL: one result over all N*T values (the
 * Trainer's flatten()).  A column may hold at most 2^26 values (EXPLAINN_E_ARG beyond; the size query
 * returns the negative code).  Results are fp64 on the device (1 or T values each); no host
 * synchronisation, no allocation: all scratch is the caller's workspace of at least
 * explainn_metrics_workspace_bytes(N, T, mode, kind) bytes.  Same input, same bits, on every call.
 *   binary: auroc = Mann-Whitney statistic with ties counted one half (NaN for a one-class column),
 *           ap = average precision as scikit-learn defines it (0 for a column without a positive),
 *           counts = int64 (positives, negatives) per result.  Both come from ONE sort.
 *   linear: pearson (two fp64 passes) and spearman (Pearson of the average ranks); NaN for a
 *           constant column.
 * status (one device word, OR-ed into, never cleared here): bit 0 = a NaN or +-Inf in y or s,
 * bit 1 = a binary target other than exactly 0 or 1.  The results are meaningless when it is set.
 * -0.0 and +0.0 are one score; denormals are distinct values.  No context needed. */
#define EXPLAINN_METRICS_GLOBAL 0
#define EXPLAINN_METRICS_PER_TASK 1
#define EXPLAINN_METRICS_BINARY 0
#define EXPLAINN_METRICS_LINEAR 1
#define EXPLAINN_METRICS_NONFINITE 1
#define EXPLAINN_METRICS_NOT_BINARY 2
int64_t explainn_metrics_workspace_bytes(int64_t N, int T, int mode, int kind);
int explainn_metrics_binary(const float* y, const float* s, int64_t N, int T, int mode, double* auroc,
                            double* ap, int64_t* counts, unsigned int* status, void* workspace,
                            int64_t workspace_bytes, void* stream);
int explainn_metrics_linear(const float* y, const float* s, int64_t N, int T, int mode, double* pearson,
                            double* spearman, unsigned int* status, void* workspace,
                            int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EXPLAINN_HIP_H */
