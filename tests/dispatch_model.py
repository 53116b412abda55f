"""Which compiled kernel forms the host code picks for a model shape, restated from the launchers in
explainn_amd/csrc (api.hip, convpool.hip, bwd.hip, fc.hip, head.hip, prep.hip, dense.hip), and the
case list of the dispatch sweep (tests/test_gpu_dispatch_sweep.py) built from it.

The tuning constants and tables are read from the sources with regular expressions, not copied:
a retuned constant or a new bucket moves the model with it, and tests/test_dispatch_coverage.py
then fails on CPU until the sweep reaches the new form.

forms(U, k, L, T, B, max_batch, path) returns a set of tuples, one per choice the host code makes:

  ("NQ", NQ)                      pooled-length bucket (nq_bucket): passA/passB/qmom/prep2/fc_fwd <NQ>
  ("nq_edge", NQ, "lower"|"upper")  n = nq_lower(NQ) + 1 or n = NQ
  ("qmom", "small"|"big")         qmom_kernel (NQ <= 32) or qmom_big_kernel
  ("fc_fwd", "bf16"|"fp32")       fc_fwd_bf_kernel (NQ <= FC_BF_MAXN) or the fp32-MFMA fc_fwd_kernel
  ("pa_ng", g)                    passA row groups (grid z)
  ("mid", "fused"|"big")          mid_fused_kernel (n <= 72) or mid_big_kernel
  ("conv_pool", ksteps, UT)       conv_pool_mm_kernel<KS, UT>
  ("conv_bwd", K)                 conv_bwd_mm_kernel<K>
  ("conv_bwd_images", K)          ... with more than one LDS image per workgroup (wper > CBM_CHUNK)
  ("dense", ...)                  the soft-input kernels (dense.hip) instead of the two above
  ("head_fwd", branch)            logits_bn | regs<HEAD_RB> | regs<16> | loop (head_fwd_train_kernel)
  ("logits", "bn"|"kernel"|"gemm")
  ("head_bwd", branch)            passA_dl | passA_loss | fused_loss | deferred_loss | kernel
  ("head_bwd_body", body)         inreg | loop | gemm: the branch inside head_bwd_kernel
  ("QCH", q), ("qch_per", s)      q-moment chunks and sequences per chunk
  ("ACH", a), ("ach_per", s)      passA chunks and sequences per chunk
  ("eval_logits", "kernel"|"gemm")  the eval-mode combiner

head_forms(U, T, B, path, G) with G > 1 is the head of a model bank of G members of U units: every form
is tagged ("bank", ...), so that a bank's run of a kernel never counts for the single model's.

The entry points that came after the train step have launchers of their own (ism.hip, inputgrad.hip):

ism_forms(U, k, L, T, B), in-silico mutagenesis
  ("ism_nw", NW)                  ism_units_kernel<NW>, NW = ism_nw(k)
  ("ism_k_edge", NW, "lower"|"upper")  the smallest / largest kernel size of that NW
  ("ism_sum", TC, "full"|"ragged"|"several")  ism_sum_kernel<TC>: the last task chunk full or not, more than one
  ("ism_sum_trips", TC, 1|2|3, "full"|"ragged")  task chunks of ism_sum_kernel (3: one neither first nor last)
  ("ism_subbatches", "one"|"several")  trips of launch_ism's sub-batch loop
  ("ism_tail", r)                 positions behind the last pooled window's reach, L - (7n + k - 1)
  ("ism_n", 1)                    one pooled window

ig_forms(U, k, L, T, B, mode), the input gradient; mode eval | train | train_dense
  ("ig", mode)                    input_grad_kernel<TRAIN, DENSE>
  ("ig_ng", NG)                   train: row groups of passB's S12p partials that ig_coef_kernel sums
  ("ig_chunks", "several"[, "big_n"])  train: QCH or ACH > 1 (big_n: at a pooled length of the large-n kernels)
  ("ig_units", "partial_wave"|"partial_pass"|"several_passes")   units against IG_UT and a wave's share
  ("ig_units_edge", mode, U)      U = a wave's share, IG_UT, and one more
  ("ig_batch", B)                 B = 2, the 64-sequence tile and IG_DY_THREADS, and one more
  ("ig_wmax", mode, k)            some tile of IG_POS positions needs the largest window count of that k
  ("ig_k", mode, k)               the smallest / largest kernel size
  ("ig_tail", mode, r)            (L - k + 1) % POOLW
  ("ig_pos", "ragged")            L is no multiple of IG_POS
  ("ig_wc", "ragged"|"several")   eval: pooled positions against ig_eval_dy's register chunk IG_WC
  ("ig_n", mode, 1)               one pooled window
"""
import collections
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "explainn_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^\s*#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, "#define %s not found" % name
    return int(m.group(1))


def _one(pattern, text, what):
    m = re.search(pattern, text, re.S)
    assert m, "%s not found in the sources (pattern %r)" % (what, pattern)
    return m


def _ints(s):
    return [int(v) for v in re.findall(r"\d+", s)]


def parse_sources():
    """Every constant and table the dispatch depends on, read from csrc."""
    common, api, bwd = _src("common.h"), _src("api.hip"), _src("bwd.hip")
    head, conv, dense, fc = _src("head.hip"), _src("convpool.hip"), _src("dense.hip"), _src("fc.hip")
    c = {}
    for name in ("MAX_K", "MAX_NQ", "HEAD_RB", "HEAD_GEMM_MIN_T", "PA_HEAD_MAX_T", "FC_BF_MAXN", "POOLW"):
        c[name] = _define(common, name)
    c["CBM_CHUNK"] = _define(bwd, "CBM_CHUNK")
    c["DENSE_BWD_SEQS"] = _define(dense, "DENSE_BWD_SEQS")
    body = _one(r"static inline int nq_bucket\(int n\)\s*\{.*?b\[\]\s*=\s*\{([^}]*)\}", common, "nq_bucket table").group(1)
    c["buckets"] = _ints(body)
    body = _one(r"constexpr int nq_lower\(int NQ\)\s*\{.*?b\[\]\s*=\s*\{([^}]*)\}", common, "nq_lower table").group(1)
    c["nq_lower_table"] = _ints(body)
    body = _one(r"#define NQ_DISPATCH\(NQv, CALL\)(.*?)default:", common, "NQ_DISPATCH").group(1)
    c["nq_dispatch"] = [int(v) for v in re.findall(r"case (\d+):", body)]
    body = _one(r"#define KB_DISPATCH\(Kv, CALL\)(.*?)default:", bwd, "KB_DISPATCH").group(1)
    c["kb_dispatch"] = [int(v) for v in re.findall(r"case (\d+):", body)]
    # the filter bank: k-steps of 4 taps, two 32-unit tiles per wave up to CONV_UT2_MAX_KS k-steps
    m = _one(r"inline int conv_ksteps\(int k\)\s*\{\s*return \(k \+ (\d+)\) / (\d+);", common, "conv_ksteps")
    c["CONV_KSTEP"] = int(m.group(2))
    assert int(m.group(1)) == c["CONV_KSTEP"] - 1
    c["CONV_UT2_MAX_KS"] = int(_one(r"inline int conv_ut\(int k\)\s*\{\s*return conv_ksteps\(k\) <= (\d+) \? 2 : 1;",
                                    common, "conv_ut").group(1))
    body = _one(r"switch \(conv_ksteps\(c->k\)\)\s*\{(.*?)default:", conv, "launch_conv_pool_mm switch").group(1)
    c["cpm_cases"] = {int(ks): ("CALLUT" if kind == "CALLUT" else "UT1")
                      for ks, kind in re.findall(r"case (\d+): \{ (CALLUT|CALLKS)\(", body)}
    # conv_bwd: windows cut in P parts from n >= CBM_SPLIT_MIN_N on
    m = _one(r"static int conv_bwd_mm_split\(const explainn_ctx\* c\)\s*\{\s*int P = c->n >= (\d+) \? (\d+) : 1;",
             bwd, "conv_bwd_mm_split")
    c["CBM_SPLIT_MIN_N"], c["CBM_SPLIT"] = int(m.group(1)), int(m.group(2))
    c["MID_FUSED_MAX_N"] = int(_one(r"int launch_mid_bwd\(.*?if \(c->n <= (\d+)\)", bwd, "launch_mid_bwd").group(1))
    c["QMOM_SMALL_MAX_N"] = int(_one(r"int launch_qmoments\(.*?if constexpr \(\(N\) <= (\d+)\)", _src("prep.hip"),
                                     "launch_qmoments").group(1))
    # api.hip: chunk counts
    m = _one(r"int q = \(max_batch \+ (\d+)\) / (\d+);\s*const int64_t per = \(int64_t\)c->U \* c->NS \* c->NS \* (\d+);"
             r"\s*const int cap = \(int\)\(\(int64_t\)\((\d+) << (\d+)\)", api, "QCH rule")
    c["QCH_SEQS"], c["QCH_BYTES_PER"], c["QCH_CAP_BYTES"] = int(m.group(2)), int(m.group(3)), int(m.group(4)) << int(m.group(5))
    c["QCH_MAX"] = int(_one(r"if \(q > (\d+)\) q = \1;", api, "QCH max").group(1))
    m = _one(r"int a = \(max_batch \+ (\d+)\) / (\d+);.*?if \(a > (\d+)\) a = \3;", api, "ACH rule")
    c["ACH_SEQS"], c["ACH_MAX"] = int(m.group(2)), int(m.group(3))
    # head
    m = _one(r"bool head_rides_in_passA\(.*?return c->T <= PA_HEAD_MAX_T && B <= (\d+);", api, "head_rides_in_passA")
    c["PA_HEAD_MAX_B"] = int(m.group(1))
    c["FUSED_LOSS_MAX_T"] = int(_one(r"if \(c->T <= (\d+)\) \{\s*// few tasks: the loss gradient is recomputed",
                                     api, "fused-loss branch").group(1))
    m = _one(r"c->T <= HEAD_GEMM_MIN_T && !outs && \(size_t\)c->U \* \(sizeof\(float4\) \+ sizeof\(float\)\) <= (\d+) \* (\d+)"
             r" \* \(size_t\)G\)", head, "logits_bn LDS test (per member)")
    c["LOGITS_BN_LDS"] = int(m.group(1)) * int(m.group(2))
    c["LOGITS_BN_BYTES_PER_UNIT"] = 16 + 4
    m = _one(r"\} else if \(B <= (\d+) \* (\d+)\) \{\s*head_fwd_train_regs<(\d+)>", head, "head_fwd regs<16> branch")
    assert int(m.group(1)) == int(m.group(3))
    c["HEAD_FWD_REGS2"], c["HEAD_THREADS"] = int(m.group(1)), int(m.group(2))
    c["HEAD_INREG_MAX_T"] = int(_one(r"const bool inreg = !GEMMED && T <= (\d+) && B <= RB \* 256;", head,
                                     "head_bwd inreg").group(1))
    # fc.hip passA row groups: pa_nw16 = (NQ + 1 + 15) / 16 (the dz column is one more row)
    _one(r"constexpr int pa_nw16\(int NQ\) \{ return \(NQ \+ 1 \+ 15\) / 16; \}", fc, "pa_nw16")
    _one(r"constexpr int pa_wgt\(int NQ\) \{ return pa_nw16\(NQ\) <= 2 \? pa_nw16\(NQ\) : 3; \}", fc, "pa_wgt")
    c["PA_MAX_NG"] = int(_one(r"static_assert\(pa_ng\(NQ\) <= (\d+)", fc, "passA row-group limit").group(1))
    # prep.hip: the train-mode prep2 keeps C (n x n) and V1 (100 x (n + 1)) of a unit in LDS;
    # explainn_create refuses a pooled length whose tables exceed a workgroup's LDS
    _one(r"static size_t prep2_lds\(int n, int NS\) \{\s*return \(size_t\)NS \* sizeof\(double\) \+ "
         r"\(\(size_t\)n \* n \+ \(size_t\)FC_H \* \(n \+ 1\)\) \* sizeof\(float\);", _src("prep.hip"), "prep2_lds")
    # a bank (Gm > 1): never in passA, never the GEMM combiner, a loss kernel of its own; units per
    # trip of the combiner kernels' unit loops; the unit count a bank may have
    _one(r"bool head_rides_in_passA\(const explainn_ctx\* c, int B\) \{\s*if \(c->Gm > 1\) return false;", api,
         "a bank never rides in passA")
    _one(r"const bool gemm = c->Gm == 1 && c->T > HEAD_GEMM_MIN_T;", head, "head_bwd GEMM rule")
    _one(r"if \(logits && G == 1 && T > HEAD_GEMM_MIN_T\)", head, "head_fwd GEMM rule")
    _one(r"int launch_loss\(.*?\{\s*if \(c->Gm > 1\) \{\s*hipLaunchKernelGGL\(bank_loss_kernel", head, "bank_loss route")
    _one(r"int launch_loss_deferred\(.*?if \(c->Gm > 1\) return launch_loss\(", head, "bank_loss route (deferred)")
    c["LOGITS_UNITS_TRIP"] = int(_one(r"void logits_kernel\(.*?for \(int u0 = wv; u0 < U; u0 \+= (\d+)\)", head,
                                      "logits_kernel unit loop").group(1))
    m = _one(r"void logits_bn_kernel\(.*?constexpr int LQ = (\d+);.*?for \(int u0 = wv; u0 < U; u0 \+= (\d+) \* LQ\)",
             head, "logits_bn_kernel unit loop")
    c["LOGITS_BN_UNITS_TRIP"] = int(m.group(1)) * int(m.group(2))
    c["BANK_MAX_UNITS"] = _define(api, "BANK_MAX_UNITS")
    _one(r"if \(groups > 1 && \(int64_t\)groups \* units_per_member > BANK_MAX_UNITS\)", api, "bank unit limit")
    # ism.hip
    ism, ig = _src("ism.hip"), _src("inputgrad.hip")
    m = _one(r"inline int ism_nw\(int k\) \{ return \(k \+ (\d+)\) / (\d+) \+ (\d+); \}", ism, "ism_nw")
    c["ISM_NW_RULE"] = tuple(int(v) for v in m.groups())
    body = _one(r"switch \(ism_nw\(c->k\)\) \{(.*?)default:", ism, "launch_ism switch").group(1)
    c["ism_nw_cases"] = [int(v) for v in re.findall(r"case (\d+):", body)]
    m = _one(r"if \(c->T == (\d+)\) hipLaunchKernelGGL\(\(ism_sum_kernel<(\d+)>\), ISM_SUM_ARGS\);\s*"
             r"else if \(c->T <= (\d+)\) hipLaunchKernelGGL\(\(ism_sum_kernel<(\d+)>\), ISM_SUM_ARGS\);\s*"
             r"else hipLaunchKernelGGL\(\(ism_sum_kernel<(\d+)>\), ISM_SUM_ARGS\);", ism, "ism_sum dispatch")
    t1, tc1, t2, tc2, tc3 = (int(v) for v in m.groups())
    assert t1 == 1
    c["ism_sum_rules"] = [(t1, tc1), (t2, tc2), (None, tc3)]      # (largest T, TC), in order
    c["ISM_WS_CAP"] = 1 << int(_one(r"#define ISM_WS_CAP \(1LL << (\d+)\)", ism, "ISM_WS_CAP").group(1))
    m = _one(r"int ism_sub_batch\(.*?per = \(int64_t\)c->U \* 4 \* c->L \* \(int64_t\)sizeof\(float\);\s*"
             r"int64_t s = ISM_WS_CAP / per / (\d+) \* \1;\s*if \(s < \1\) s = \1;", ism, "ism_sub_batch")
    c["ISM_SUB_STEP"] = int(m.group(1))
    _one(r"inline int ism_pend\(int k, int n, int L\) \{ return min\(L, POOLW \* n \+ k - 1\); \}", ism, "ism_pend")
    # inputgrad.hip
    for name in ("IG_POS", "IG_UT", "IG_WMAX", "IG_DY_THREADS", "IG_WC"):
        c[name] = _define(ig, name)
    _one(r"int wlo = P0 - k - 5;\s*wlo = wlo <= 0 \? 0 : \(wlo \+ 6\) / 7;\s*"
         r"const int whi = min\(n - 1, \(P0 \+ IG_POS - 1\) / POOLW\);", ig, "input_grad window range")
    _one(r"const int ub = u0 \+ \(IG_UT / 4\) \* wave", ig, "input_grad wave share")
    c["IG_SEQS"] = int(_one(r"const dim3 grid\(\(B \+ (\d+)\) / (\d+), \(c->L \+ IG_POS - 1\) / IG_POS\);", ig,
                            "input_grad grid").group(2))
    # common.h: passB's row groups
    m = _one(r"constexpr int fc_nw16\(int NQ\) \{ return \(NQ \+ (\d+)\) / (\d+); \}", common, "fc_nw16")
    assert int(m.group(1)) == int(m.group(2)) - 1
    c["FC_TILE"] = int(m.group(2))
    m = _one(r"constexpr int fc_wgt\(int NQ\) \{ return fc_nw16\(NQ\) <= (\d+) \? fc_nw16\(NQ\) : (\d+); \}", common, "fc_wgt")
    c["FC_WGT_SMALL"], c["FC_WGT"] = int(m.group(1)), int(m.group(2))
    _one(r"constexpr int fc_ng\(int NQ\) \{ return \(fc_nw16\(NQ\) \+ fc_wgt\(NQ\) - 1\) / fc_wgt\(NQ\); \}", common, "fc_ng")
    _one(r"hipLaunchKernelGGL\(ig_coef_kernel,.*?c->igcoef, fc_ng\(c->NQ\),", ig, "ig_coef row groups")
    return c


C = parse_sources()
LDS_PER_WORKGROUP = 160 * 1024        # MI355X (gfx950): LDS per CU, all of it available to one workgroup


class Unsupported(Exception):
    """explainn_create refuses the shape (EXPLAINN_E_UNSUPPORTED)."""


def pooled_len(L, k):
    return (L - k + 1) // C["POOLW"]


def nq_bucket(n):
    for b in C["buckets"]:
        if b >= n:
            return b
    return 0


def nq_lower(NQ):
    b = [0] + C["buckets"]
    return b[b.index(NQ) - 1]


def conv_ksteps(k):
    return (k + C["CONV_KSTEP"] - 1) // C["CONV_KSTEP"]


def conv_ut(k):
    return 2 if conv_ksteps(k) <= C["CONV_UT2_MAX_KS"] else 1


def pa_ng(NQ):
    nw16 = (NQ + 1 + 15) // 16
    wgt = nw16 if nw16 <= 2 else 3
    return (nw16 + wgt - 1) // wgt


def ns_stride(NQ):
    cc = (NQ + 35) // 36
    cl = (((NQ + cc - 1) // cc) + 3) & ~3
    return cc * cl


def chunks(U, NQ, max_batch, qch=None, ach=None):
    """(QCH, ACH) of explainn_create, EXPLAINN_QCH / EXPLAINN_ACH overrides included."""
    q = (max_batch + C["QCH_SEQS"] - 1) // C["QCH_SEQS"]
    per = U * ns_stride(NQ) ** 2 * C["QCH_BYTES_PER"]
    cap = C["QCH_CAP_BYTES"] // max(per, 1)
    q = max(1, min(q, C["QCH_MAX"], cap))
    if qch is not None and 1 <= qch <= cap and qch <= C["QCH_MAX"]:
        q = qch
    a = max(1, min((max_batch + C["ACH_SEQS"] - 1) // C["ACH_SEQS"], C["ACH_MAX"]))
    if ach is not None and 1 <= ach <= C["ACH_MAX"]:
        a = ach
    return q, a


def prep2_lds(n):
    return ns_stride(nq_bucket(n)) * 8 + (n * n + 100 * (n + 1)) * 4


def max_legal_n():
    """The largest pooled length explainn_create accepts."""
    return max(n for n in range(1, C["MAX_NQ"] + 1) if prep2_lds(n) <= LDS_PER_WORKGROUP)


def check_supported(U, k, L, T):
    n = pooled_len(L, k)
    if k < 2 or k > C["MAX_K"]:
        raise Unsupported("kernel_size %d" % k)
    if n < 1:
        raise ValueError("sequence too short")
    if nq_bucket(n) == 0:
        raise Unsupported("pooled length %d" % n)
    if prep2_lds(n) > LDS_PER_WORKGROUP:
        raise Unsupported("pooled length %d: prep2 needs %d bytes of LDS" % (n, prep2_lds(n)))
    return n


def bank_head_forms(Um, T, B, path, G):
    """The head of a bank of G > 1 members of Um units (launch_head_fwd, train_step_front,
    launch_head_bwd with Gm > 1): never in passA, never a GEMM, a loss kernel of its own."""
    f = set()
    regs = C["HEAD_RB"] * C["HEAD_THREADS"]
    # the LDS test reads c->U = G * Um against G times the limit: one member's share
    if T <= C["HEAD_GEMM_MIN_T"] and G * Um * C["LOGITS_BN_BYTES_PER_UNIT"] <= C["LOGITS_BN_LDS"] * G:
        f |= {("bank", "head_fwd", "logits_bn"), ("bank", "logits", "bn")}
        if Um > C["LOGITS_BN_UNITS_TRIP"]:
            f.add(("bank_units_trip", "logits_bn", "several"))
    else:
        if B <= regs:
            f.add(("bank", "head_fwd", "regs%d" % C["HEAD_RB"]))
        elif B <= C["HEAD_FWD_REGS2"] * C["HEAD_THREADS"]:
            f.add(("bank", "head_fwd", "regs%d" % C["HEAD_FWD_REGS2"]))
        else:
            f.add(("bank", "head_fwd", "loop"))
        f.add(("bank", "logits", "kernel"))
        if Um > C["LOGITS_UNITS_TRIP"]:
            f.add(("bank_units_trip", "logits", "several"))
    if path != "step":
        branch = "kernel"
    elif T <= C["FUSED_LOSS_MAX_T"]:
        branch = "fused_loss"
    else:
        branch = "bank_loss"
    body = "inreg" if T <= C["HEAD_INREG_MAX_T"] and B <= regs else "loop"
    f |= {("bank", "head_bwd", branch), ("bank", "head_bwd_body", body), ("bank", "head_bwd", branch, body)}
    # the task thresholds themselves, at a batch below one block of threads (rows of the register
    # paths that no sequence fills) or not, with one trip of the combiner's unit loop or several
    if T in bank_task_edges():
        trips = "several_trips" if any(v[0] == "bank_units_trip" for v in f) else "one_trip"
        f.add(("bank", "t_edge", T, "lt_block" if B < C["HEAD_THREADS"] else "ge_block", trips))
    if B in (regs, regs + 1, C["HEAD_FWD_REGS2"] * C["HEAD_THREADS"] + 1):
        f.add(("bank", "b_edge", B))
    if G * Um == C["BANK_MAX_UNITS"]:
        f.add(("bank", "units", "limit"))
    return f


def bank_task_edges():
    return sorted({C["FUSED_LOSS_MAX_T"], C["FUSED_LOSS_MAX_T"] + 1, C["HEAD_INREG_MAX_T"], C["HEAD_INREG_MAX_T"] + 1,
                   C["HEAD_GEMM_MIN_T"], C["HEAD_GEMM_MIN_T"] + 1})


def head_forms(U, T, B, path, G=1):
    """The head's forward and backward branches of a train step (path "autograd": forward_train +
    explainn_backward; "step": explainn_train_step).  G > 1: a bank of G members of U units each."""
    if G > 1:
        return bank_head_forms(U, T, B, path, G)
    f = set()
    if T <= C["HEAD_GEMM_MIN_T"] and U * C["LOGITS_BN_BYTES_PER_UNIT"] <= C["LOGITS_BN_LDS"]:
        f.add(("head_fwd", "logits_bn"))
        f.add(("logits", "bn"))
    else:
        if B <= C["HEAD_RB"] * C["HEAD_THREADS"]:
            f.add(("head_fwd", "regs%d" % C["HEAD_RB"]))
        elif B <= C["HEAD_FWD_REGS2"] * C["HEAD_THREADS"]:
            f.add(("head_fwd", "regs%d" % C["HEAD_FWD_REGS2"]))
        else:
            f.add(("head_fwd", "loop"))
        f.add(("logits", "gemm" if T > C["HEAD_GEMM_MIN_T"] else "kernel"))
    passA = T <= C["PA_HEAD_MAX_T"] and B <= C["PA_HEAD_MAX_B"]
    if passA:
        f.add(("head_bwd", "passA_dl" if path == "autograd" else "passA_loss"))
        return f
    if path == "step" and T <= C["FUSED_LOSS_MAX_T"]:
        branch = "fused_loss"
    elif path == "step":
        branch = "deferred_loss"
    else:
        branch = "kernel"
    if T > C["HEAD_GEMM_MIN_T"]:
        body = "gemm"
    elif T <= C["HEAD_INREG_MAX_T"] and B <= C["HEAD_RB"] * C["HEAD_THREADS"]:
        body = "inreg"
    else:
        body = "loop"
    f |= {("head_bwd", branch), ("head_bwd_body", body), ("head_bwd", branch, body)}
    return f


def forms(U, k, L, T, B, max_batch=None, paths=("autograd",), dense=False, qch=None, ach=None):
    """The kernel forms one train step per entry point in `paths` (and the eval forward after it)
    of this shape run."""
    n = check_supported(U, k, L, T)
    max_batch = max(B, max_batch or B)
    NQ = nq_bucket(n)
    f = {("NQ", NQ), ("pa_ng", pa_ng(NQ))}
    if n == nq_lower(NQ) + 1:
        f.add(("nq_edge", NQ, "lower"))
    if n == min(NQ, max_legal_n()):
        f.add(("nq_edge", NQ, "upper"))
    f.add(("qmom", "small" if NQ <= C["QMOM_SMALL_MAX_N"] else "big"))
    f.add(("fc_fwd", "bf16" if NQ <= C["FC_BF_MAXN"] else "fp32"))
    f.add(("mid", "fused" if n <= C["MID_FUSED_MAX_N"] else "big"))
    if dense:
        f.add(("dense", "conv_pool"))
        f.add(("dense", "k", k))
        f.add(("dense", "n", n))
        nparts = (B + C["DENSE_BWD_SEQS"] - 1) // C["DENSE_BWD_SEQS"]
        f.add(("dense", "partials", "several" if nparts > 1 else "one"))
        if B % C["DENSE_BWD_SEQS"]:
            f.add(("dense", "ragged"))
    else:
        ks = conv_ksteps(k)
        assert ks in C["cpm_cases"], "conv_pool_mm has no case for %d k-steps" % ks
        f.add(("conv_pool", ks, conv_ut(k)))
        f.add(("conv_bwd", k))
        P = C["CBM_SPLIT"] if n >= C["CBM_SPLIT_MIN_N"] else 1
        wper = (n + P - 1) // P
        if wper > C["CBM_CHUNK"]:
            f.add(("conv_bwd_images", k))
    for path in paths:
        f |= head_forms(U, T, B, path)
    f.add(("eval_logits", "gemm" if T > C["HEAD_GEMM_MIN_T"] else "kernel"))
    q, a = chunks(U, NQ, max_batch, qch, ach)
    f.add(("QCH", q))
    f.add(("ACH", a))
    f.add(("qch_per", ((((B + q - 1) // q) + 63) // 64) * 64))
    f.add(("ach_per", ((((B + a - 1) // a) + 127) // 128) * 128))
    return f


# ---- the sweep --------------------------------------------------------------------------------
# paths: the entry points the case runs, "autograd" (forward_train + explainn_backward, with a
# dropout keep-mask when it is the only one) and / or "step" (explainn_train_step, no dropout)
Case = collections.namedtuple("Case", "id group U k L T B paths max_batch qch ach dense seed")
BOTH = ("autograd", "step")


def _case(group, U, k, L, T, B, paths=("autograd",), max_batch=None, qch=None, ach=None, dense=False, tag=""):
    cid = "%s-U%d-k%d-L%d-T%d-B%d%s%s%s%s%s" % (
        group, U, k, L, T, B, "" if paths == ("autograd",) else "-" + "+".join(paths),
        "-mb%d" % max_batch if max_batch else "", "-qch%d" % qch if qch else "", "-ach%d" % ach if ach else "",
        "-dense" if dense else "") + tag
    return Case(cid, group, U, k, L, T, B, paths, max_batch, qch, ach, dense, (U * 131 + k * 17 + L + B) % 10007)


# (U, k, L, T, B, n_frac) of tests/test_gpu_parity.py::test_train_step_vs_oracle: the sweep does not
# repeat these shapes, and the coverage test counts them
ORACLE_STEP_SHAPES = [
    (5, 19, 61, 3, 24, 0.05),       # tail = 1, N bases, B < 64
    (7, 19, 200, 1, 130, 0.0),      # B not a multiple of 64, U not a multiple of 4
    (4, 7, 75, 2, 64, 0.1),
    (9, 26, 300, 4, 200, 0.01),     # n = 39 -> bucket 40 (zero-padded weights)
    (3, 19, 1000, 2, 70, 0.0),      # n = 140 (config C4's pooled length)
    (2, 19, 600, 5, 66, 0.02),      # n = 83  -> bucket 84 (config C5's pooled length)
    (37, 19, 61, 50, 70, 0.02),     # T = 50 (C3/C4): combiner forward/backward as MFMA GEMMs
    (70, 9, 40, 164, 131, 0.0),     # T = 164 (C5), ragged tiles in every GEMM dimension
    (3, 5, 33, 9, 5, 0.0),          # smallest GEMM case: one partly filled tile
    (6, 32, 120, 1, 40, 0.03),      # largest instantiated kernel size (two code words per window)
    (5, 2, 40, 2, 33, 0.05),        # smallest kernel size
    (4, 31, 260, 1, 20, 0.02),      # odd kernel size next to the maximum, two staging chunks (n = 32+)
    # large-n kernels over SEVERAL batch chunks (QCH / ACH > 1, ragged last chunk): qmom_big,
    # mid_big, passB<140>/<84>, fc_fwd<NQ > 32> -- the code paths configs C4 / C5 run
    (3, 19, 1000, 2, 300, 0.01),    # n = 140, 3 chunks of 128 (last one 44 sequences)
    (2, 19, 600, 5, 700, 0.02),     # n = 83, 6 chunks (last one 60)
    (3, 19, 450, 1, 90, 0.0),       # n = 61 -> bucket 64: two 32-wide k-steps of the bf16 fc_fwd
    (4, 19, 61, 2, 600, 0.0),       # few tasks, batch > 512: the per-unit head backward kernel (smaller
                                    # batches run it inside passA)
    (1100, 5, 40, 2, 70, 0.0),      # more units than threads in the combiner block that finishes BatchNorm3
    # the lower edge of a pooled-length bucket (n = previous bucket + 1): passA and qmom decide at
    # compile time which rows always / never exist inside the bucket (csrc/common.h: nq_lower)
    (3, 19, 109, 1, 70, 0.0),       # n = 13 -> bucket 16
    (3, 19, 165, 1, 70, 0.02),      # n = 21 -> bucket 24
    (3, 19, 186, 2, 70, 0.0),       # n = 24 = bucket 24's upper edge
    (3, 19, 193, 1, 70, 0.0),       # n = 25 -> bucket 26 (C2's kernels, one row short)
    (3, 19, 207, 1, 70, 0.0),       # n = 27 -> bucket 28
    (3, 19, 249, 1, 70, 0.0),       # n = 33 -> bucket 40 (first size with two row groups in passA)
    (3, 19, 305, 1, 70, 0.0),       # n = 41 -> bucket 48
    (2, 19, 529, 1, 70, 0.0),       # n = 73 -> bucket 84: the first n of the large-n kernels
    # the filter-bank GEMM's edges: one pooling window (a wave's first window is its last), the
    # widest kernel with one window, unit counts that leave a 32-unit tile / a two-tile group partly empty
    (3, 19, 25, 1, 9, 0.0),         # n = 1, Lo = 7
    (2, 32, 38, 1, 7, 0.0),         # k = 32, n = 1
    (33, 19, 32, 1, 31, 0.0),       # 33 units: tile 1 holds one unit
    (65, 4, 200, 1, 100, 0.02),     # 65 units: three tiles, the second group half empty; k = 4 is one k-step
]


def _length(n, k, r):
    return C["POOLW"] * n + k - 1 + r


def build_cases():
    cases = []
    done_n = {pooled_len(L, k) for (U, k, L, T, B, _) in ORACLE_STEP_SHAPES}
    # A. every bucket at n = nq_lower(NQ) + 1 and n = NQ; ragged last windows (r = 0..6)
    i = 0
    n_top = max_legal_n()
    for NQ in C["buckets"]:
        for n in sorted({nq_lower(NQ) + 1, min(NQ, n_top)}):
            if n in done_n:
                continue
            k = (19, 7, 26, 12)[i % 4]
            r = i % C["POOLW"]
            B = 70 if n <= C["MID_FUSED_MAX_N"] else 300
            cases.append(_case("A", 3, k, _length(n, k, r), 1 + i % 3, B))
            i += 1
    n_max, k_max = n_top, C["MAX_K"]
    cases.append(_case("A", 3, k_max, _length(n_max, k_max, C["POOLW"] - 1), 2, 300, tag="-longest"))
    # B. every kernel size with two window parts (n >= CBM_SPLIT_MIN_N); the ends and the k-step
    # class boundaries again with several LDS images per workgroup
    for k in range(2, k_max + 1):
        n = C["CBM_SPLIT_MIN_N"] + k % 5
        cases.append(_case("B", 5, k, _length(n, k, k % C["POOLW"]), 1 + k % 2, 40 + k))
    n_img = C["CBM_SPLIT"] * C["CBM_CHUNK"] + 1
    for k in (2, 4 * C["CONV_UT2_MAX_KS"] - 4, 4 * (C["CONV_UT2_MAX_KS"] + 1), k_max):
        cases.append(_case("B", 5, k, _length(n_img, k, 3), 2, 70, tag="-images"))
    # C. unit tiles: 32-unit tiles / tile pairs of the filter bank, 16-unit tiles of conv_bwd, at a
    # kernel size with two tiles per wave and one with one
    for k in (4 * (C["CONV_UT2_MAX_KS"] - 1), 4 * (C["CONV_UT2_MAX_KS"] + 1)):
        for U in (16, 17, 31, 32, 63, 64, 96, 97):
            cases.append(_case("C", U, k, _length(4, k, U % 7), 2, 24))
    U_big = C["LOGITS_BN_LDS"] // C["LOGITS_BN_BYTES_PER_UNIT"] + 1     # the logits_bn LDS test fails
    cases.append(_case("C", U_big, 5, _length(2, 5, 0), 2, 16))
    # D. batch and task edges, through both entry points
    for T in (C["PA_HEAD_MAX_T"], C["PA_HEAD_MAX_T"] + 1, C["HEAD_GEMM_MIN_T"], C["HEAD_GEMM_MIN_T"] + 1):
        for B in (C["PA_HEAD_MAX_B"], C["PA_HEAD_MAX_B"] + 1):
            cases.append(_case("D", 4, 19, 200, T, B, BOTH))
    regs_max = C["HEAD_RB"] * C["HEAD_THREADS"]
    loop_min = C["HEAD_FWD_REGS2"] * C["HEAD_THREADS"] + 1
    for B in (regs_max + 1, loop_min, 6000):
        for T in (2, 50):
            cases.append(_case("D", 8, 19, 200, T, B, BOTH))
    cases.append(_case("D", 8, 19, 1000, 2, loop_min, BOTH))
    # E. chunk counts through the EXPLAINN_QCH / EXPLAINN_ACH overrides, and one capped QCH without
    for L in (1000, 600):
        cases.append(_case("E", 8, 19, L, 2, 1024, ("step",), qch=1, ach=3))
        cases.append(_case("E", 8, 19, L, 2, 1024, ("step",), qch=2, ach=1))
    cases.append(_case("E", 100, 5, _length(n_max, 5, 2), 2, 200, ("step",), max_batch=1024, tag="-capped"))
    # F. the soft-input kernels
    for U, k, n, B in ((5, 2, 1, 129), (5, 2, 80, 300), (5, 2, n_max, 300),
                       (33, k_max, 1, 300), (33, k_max, 80, 129), (5, k_max, n_max, 129)):
        cases.append(_case("F", U, k, _length(n, k, (n + k) % C["POOLW"]), 2, B, dense=True))
    return cases


CASES = build_cases()

# H. sizes explainn_create refuses: (U, k, L, T)
UNSUPPORTED = [(3, 1, 40, 1), (3, C["MAX_K"] + 1, 80, 1), (3, 19, _length(C["MAX_NQ"] + 1, 19, 0), 1)]
if max_legal_n() < C["MAX_NQ"]:
    UNSUPPORTED.append((3, 19, _length(max_legal_n() + 1, 19, 0), 1))


def case_forms(c):
    return forms(c.U, c.k, c.L, c.T, c.B, c.max_batch, c.paths, c.dense, c.qch, c.ach)


def all_forms(cases=None, with_existing=True):
    got = set()
    for c in (CASES if cases is None else cases):
        got |= case_forms(c)
    if with_existing:
        for (U, k, L, T, B, _) in ORACLE_STEP_SHAPES:
            got |= forms(U, k, L, T, B)
    return got


# ---- in-silico mutagenesis (csrc/ism.hip) -------------------------------------------------------
def ism_nw(k):
    add, div, plus = C["ISM_NW_RULE"]
    return (k + add) // div + plus


def ism_sum_tc(T):
    for tmax, tc in C["ism_sum_rules"]:
        if tmax is None or T <= tmax:
            return tc


def ism_sub_batch(U, L, B):
    step = C["ISM_SUB_STEP"]
    s = max(C["ISM_WS_CAP"] // (U * 4 * L * 4) // step * step, step)
    return min(s, (B + step - 1) // step * step)


def ism_workspace_bytes(U, L, B):
    return U * 4 * L * ism_sub_batch(U, L, B) * 4


def ism_pend(k, n, L):
    return min(L, C["POOLW"] * n + k - 1)


def ism_k_range(NW):
    ks = [k for k in range(2, C["MAX_K"] + 1) if ism_nw(k) == NW]
    return ks[0], ks[-1]


def ism_forms(U, k, L, T, B):
    n = check_supported(U, k, L, T)
    NW = ism_nw(k)
    assert NW in C["ism_nw_cases"], "launch_ism has no case for NW = %d" % NW
    f = {("ism_nw", NW), ("ism_tail", L - ism_pend(k, n, L))}
    lo, hi = ism_k_range(NW)
    if k == lo:
        f.add(("ism_k_edge", NW, "lower"))
    if k == hi:
        f.add(("ism_k_edge", NW, "upper"))
    TC = ism_sum_tc(T)
    f.add(("ism_sum", TC, "ragged" if T % TC else "full"))
    if T > TC:
        f.add(("ism_sum", TC, "several"))
    f.add(("ism_sum_trips", TC, min(3, (T + TC - 1) // TC), "ragged" if T % TC else "full"))
    f.add(("ism_subbatches", "several" if B > ism_sub_batch(U, L, B) else "one"))
    if n == 1:
        f.add(("ism_n", 1))
    return f


IsmCase = collections.namedtuple("IsmCase", "id U k L T B ref seed")      # ref: "oracle" | "device"


def _ism_case(U, k, L, T, B, ref="oracle"):
    return IsmCase("ism-U%d-k%d-L%d-T%d-B%d" % (U, k, L, T, B), U, k, L, T, B, ref, (U * 131 + k * 17 + L + T) % 10007)


def build_ism_cases():
    cases = []
    # both kernel sizes at every change of NW, three windows, tails 0..6, the task counts below the
    # first ism_sum threshold and at it
    i = 0
    for NW in C["ism_nw_cases"]:
        lo, hi = ism_k_range(NW)
        for k in (lo, hi):
            if k in (2, C["MAX_K"]):
                continue                    # the ends come with one window below
            cases.append(_ism_case(3 + i % 3, k, _length(3, k, i % C["POOLW"]), 1 + i % 3, 3))
            i += 1
    # the task chunks of ism_sum: both sides of every threshold, of the widest chunk, and three chunks
    tmid, tc_max = C["ism_sum_rules"][1][0], C["ism_sum_rules"][-1][1]
    for T in (tmid, tmid + 1, tc_max, tc_max + 1, 2 * tc_max + 1):
        cases.append(_ism_case(4, 5, _length(2, 5, T % C["POOLW"]), T, 3))
    # one window, smallest and largest kernel
    cases.append(_ism_case(3, 2, _length(1, 2, 3), 2, 3))
    cases.append(_ism_case(3, C["MAX_K"], _length(1, C["MAX_K"], 5), 1, 3))
    # two trips of the sub-batch loop: the smallest U x L whose sub-batch is one step, a batch of one
    # step and a ragged second trip
    U, step = 1100, C["ISM_SUB_STEP"]
    L = C["ISM_WS_CAP"] // (16 * 2 * step) // U + 1
    cases.append(_ism_case(U, 5, L, 2, step + 6, ref="device"))
    return cases


ISM_CASES = build_ism_cases()


# ---- the input gradient (csrc/inputgrad.hip) ----------------------------------------------------
def fc_ng(NQ):
    nw16 = (NQ + C["FC_TILE"] - 1) // C["FC_TILE"]
    wgt = nw16 if nw16 <= C["FC_WGT_SMALL"] else C["FC_WGT"]
    return (nw16 + wgt - 1) // wgt


def ig_windows(P0, k, n):
    """How many pooled windows input_grad_kernel loads for the tile of IG_POS positions at P0."""
    w = C["POOLW"]
    wlo = P0 - k - (w - 2)
    wlo = 0 if wlo <= 0 else (wlo + w - 1) // w
    whi = min(n - 1, (P0 + C["IG_POS"] - 1) // w)
    return whi - wlo + 1


def ig_max_windows(k):
    """The largest window count any tile can need at kernel size k (n unbounded)."""
    period = C["POOLW"] * C["IG_POS"]
    return max(ig_windows(P0, k, 10 ** 6) for P0 in range(0, 4 * period + C["IG_POS"] * k, C["IG_POS"]))


def ig_unit_edges():
    return (C["IG_UT"] // 4, C["IG_UT"] // 4 + 1, C["IG_UT"], C["IG_UT"] + 1)


def ig_batch_edges():
    return (2, C["IG_SEQS"], C["IG_SEQS"] + 1, C["IG_DY_THREADS"], C["IG_DY_THREADS"] + 1)


def ig_forms(U, k, L, T, B, mode):
    assert mode in ("eval", "train", "train_dense")
    n = check_supported(U, k, L, T)
    f = {("ig", mode), ("ig_tail", mode, (L - k + 1) % C["POOLW"])}
    if mode != "eval":
        NQ = nq_bucket(n)
        f.add(("ig_ng", fc_ng(NQ)))
        if n == nq_lower(NQ) + 1:
            f.add(("ig_ng_edge", fc_ng(NQ), "lower"))
        q, a = chunks(U, NQ, B)
        if q > 1 or a > 1:
            f.add(("ig_chunks", "several"))
            if n > C["MID_FUSED_MAX_N"]:
                f.add(("ig_chunks", "several", "big_n"))
    else:
        if n % C["IG_WC"]:
            f.add(("ig_wc", "ragged"))
        if n > C["IG_WC"]:
            f.add(("ig_wc", "several"))
    if U % (C["IG_UT"] // 4):
        f.add(("ig_units", "partial_wave"))
    if U % C["IG_UT"]:
        f.add(("ig_units", "partial_pass"))
    if U > C["IG_UT"]:
        f.add(("ig_units", "several_passes"))
    if U in ig_unit_edges():
        f.add(("ig_units_edge", mode, U))
    if B in ig_batch_edges():
        f.add(("ig_batch", B))
    if k in (2, C["MAX_K"]):
        f.add(("ig_k", mode, k))
    if max(ig_windows(P0, k, n) for P0 in range(0, L, C["IG_POS"])) == ig_max_windows(k):
        f.add(("ig_wmax", mode, k))
    if L % C["IG_POS"]:
        f.add(("ig_pos", "ragged"))
    if n == 1:
        f.add(("ig_n", mode, 1))
    return f


IgCase = collections.namedtuple("IgCase", "id U k L T B mode seed")


def _ig_case(U, k, L, T, B, mode, bump=0):
    return IgCase("ig-%s-U%d-k%d-L%d-T%d-B%d" % (mode, U, k, L, T, B), U, k, L, T, B, mode,
                  (U * 131 + k * 17 + L + B) % 10007 + bump)


def _ig_wmax_length(k, r):
    """The shortest L with tail r at which some tile needs ig_max_windows(k) windows."""
    for n in range(1, max_legal_n() + 1):
        L = C["POOLW"] * n + k - 1 + r
        if max(ig_windows(P0, k, n) for P0 in range(0, L, C["IG_POS"])) == ig_max_windows(k):
            return L + (1 if L % C["IG_POS"] == 0 and r < C["POOLW"] - 1 else 0)
    raise AssertionError("no pooled length reaches %d windows at k = %d" % (ig_max_windows(k), k))


def build_ig_cases():
    cases = []
    k_max = C["MAX_K"]
    for mode in ("train", "eval"):
        for U in ig_unit_edges():
            cases.append(_ig_case(U, 5, _length(2 + U % 3, 5, U % C["POOLW"]), 2, 6, mode))
        # the widest filter with the longest tail, and the narrowest: the shortest sequence at which a
        # tile needs the largest window count of that kernel size
        cases.append(_ig_case(5, k_max, _ig_wmax_length(k_max, C["POOLW"] - 1), 2, 6, mode))
        cases.append(_ig_case(5, 2, _ig_wmax_length(2, 3), 2, 6, mode))
        cases.append(_ig_case(3, 5, _length(1, 5, 2), 1, 6, mode))                  # n = 1
    # train: the first bucket of every fc_ng value past 1 at its lower edge (ig_ng 1 is every small case)
    seen = {1}
    for NQ in C["buckets"]:
        if fc_ng(NQ) not in seen and nq_lower(NQ) + 1 <= max_legal_n():
            seen.add(fc_ng(NQ))
            cases.append(_ig_case(3, 5, _length(nq_lower(NQ) + 1, 5, fc_ng(NQ)), 1, 6, "train"))
    # several batch chunks at a pooled length of the large-n kernels (inside its bucket: the lower
    # edges are the cases above)
    B_chunks = max(C["QCH_SEQS"], C["ACH_SEQS"]) + 5
    cases.append(_ig_case(3, 5, _length(C["MID_FUSED_MAX_N"] + 2, 5, 1), 2, B_chunks, "train"))
    for B in ig_batch_edges():
        cases.append(_ig_case(4, 5, _length(3, 5, B % C["POOLW"]), 2, B, "train"))
    # eval: pooled positions one past ig_eval_dy's register chunk
    cases.append(_ig_case(3, 5, _length(C["IG_WC"] + 1, 5, 4), 2, 6, "eval"))
    cases.append(_ig_case(4, k_max, _ig_wmax_length(k_max, C["POOLW"] - 1), 2, 6, "train_dense"))
    return cases


IG_CASES = build_ig_cases()


# ---- the head of a model bank (csrc/head.hip with Gm > 1) ---------------------------------------
BankCase = collections.namedtuple("BankCase", "id G U k L T B paths seed")


def _bank_case(G, U, T, B, paths=("step",), k=5, n=2):
    L = _length(n, k, (T + B) % C["POOLW"])
    return BankCase("bank-G%d-U%d-T%d-B%d-%s" % (G, U, T, B, "+".join(paths)), G, U, k, L, T, B, paths,
                    (G * 977 + U * 131 + T * 17 + B) % 10007)


def build_bank_cases():
    regs = C["HEAD_RB"] * C["HEAD_THREADS"]
    regs2 = C["HEAD_FWD_REGS2"] * C["HEAD_THREADS"]
    t_in, t_gemm = C["HEAD_INREG_MAX_T"], C["HEAD_GEMM_MIN_T"]
    cases = [
        _bank_case(2, 4, 2, regs + 1, BOTH),              # looped body: fused loss and dlogits given
        _bank_case(2, 4, t_in, regs, BOTH),               # the largest register-path batch
    ]
    for T in bank_task_edges():
        cases.append(_bank_case(2, 4, T, 70))
    cases.append(_bank_case(2, 4, t_gemm + 1, regs + 1))  # head_fwd_train regs<16>
    cases.append(_bank_case(2, 4, t_gemm + 1, regs2 + 1))  # head_fwd_train's loop
    cases.append(_bank_case(2, C["LOGITS_UNITS_TRIP"] + 1, t_gemm + 1, 70))
    cases.append(_bank_case(2, C["LOGITS_BN_UNITS_TRIP"] + 1, 2, 70))
    return cases


BANK_CASES = build_bank_cases()
# a bank at the unit limit, checked against its members on the single-model path: (G, Um, k, L, T, B)
BANK_LIMIT = (C["BANK_MAX_UNITS"] // 8, 8, 5, _length(2, 5, 3), 1, 70)


def bank_case_forms(c):
    f = set()
    for path in c.paths:
        f |= head_forms(c.U, c.T, c.B, path, c.G)
    return f


def entry_forms(ism=None, ig=None, bank=None, limit=True):
    """The forms the ISM, input-gradient and bank case lists reach."""
    got = set()
    for c in (ISM_CASES if ism is None else ism):
        got |= ism_forms(c.U, c.k, c.L, c.T, c.B)
    for c in (IG_CASES if ig is None else ig):
        got |= ig_forms(c.U, c.k, c.L, c.T, c.B, c.mode)
    for c in (BANK_CASES if bank is None else bank):
        got |= bank_case_forms(c)
    if limit:
        G, Um, _, _, T, B = BANK_LIMIT
        got |= head_forms(Um, T, B, "step", G)
    return got
