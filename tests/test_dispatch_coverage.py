"""The dispatch sweep (tests/test_gpu_dispatch_sweep.py) reaches every compiled kernel form.  CPU only:
tests/dispatch_model.py reads the bucket table, the kernel-size dispatch and the tuning constants from
the sources, so a bucket, kernel size or branch added later without a sweep case fails here."""
import pytest

import dispatch_model as dm

C = dm.C
GOT = dm.all_forms()


def _missing(want):
    return sorted(set(want) - GOT, key=repr)


def test_source_tables_agree():
    """The bucket table, nq_lower's table and NQ_DISPATCH list the same buckets; KB_DISPATCH and the
    filter bank's k-step switch cover every kernel size 2..MAX_K, and nothing beyond it."""
    assert C["buckets"] == sorted(C["buckets"]) and C["buckets"][-1] == C["MAX_NQ"]
    assert C["nq_lower_table"] == [0] + C["buckets"]
    assert C["nq_dispatch"] == C["buckets"]
    assert C["kb_dispatch"] == list(range(2, C["MAX_K"] + 1))
    ks = {dm.conv_ksteps(k) for k in range(2, C["MAX_K"] + 1)}
    assert set(C["cpm_cases"]) == ks
    for s, kind in C["cpm_cases"].items():
        assert (kind == "CALLUT") == (s <= C["CONV_UT2_MAX_KS"]), s
    assert {dm.pa_ng(NQ) for NQ in C["buckets"]} == set(range(1, C["PA_MAX_NG"] + 1))


def test_every_bucket_at_both_edges():
    want = [("nq_edge", NQ, edge) for NQ in C["buckets"] for edge in ("lower", "upper")]
    assert not _missing(want), _missing(want)


def test_every_kernel_size_and_filter_bank_form():
    ks = range(2, C["MAX_K"] + 1)
    want = [("conv_bwd", k) for k in ks] + [("conv_pool", dm.conv_ksteps(k), dm.conv_ut(k)) for k in ks]
    assert not _missing(want), _missing(want)
    # several LDS images per conv_bwd workgroup, at the smallest and largest kernel and at both
    # sides of the change from two unit tiles per wave to one
    imaged = {f[1] for f in GOT if f[0] == "conv_bwd_images"}
    assert {2, C["MAX_K"]} <= imaged, imaged
    assert {dm.conv_ut(k) for k in imaged} == {1, 2}, imaged


def test_fc_passA_qmom_and_mid_forms():
    want = [("pa_ng", g) for g in range(1, C["PA_MAX_NG"] + 1)]
    want += [("fc_fwd", "bf16"), ("fc_fwd", "fp32"), ("mid", "fused"), ("mid", "big"),
             ("qmom", "small"), ("qmom", "big")]
    # the edges of the fc_fwd and mid choices themselves
    want += [("nq_edge", C["FC_BF_MAXN"], "upper"), ("nq_edge", dm.nq_bucket(C["FC_BF_MAXN"] + 1), "lower")]
    assert dm.nq_bucket(C["MID_FUSED_MAX_N"]) == C["MID_FUSED_MAX_N"]
    want += [("nq_edge", C["MID_FUSED_MAX_N"], "upper"), ("nq_edge", dm.nq_bucket(C["MID_FUSED_MAX_N"] + 1), "lower")]
    assert not _missing(want), _missing(want)


def test_every_head_branch():
    """Every branch the head's launchers can take -- found by evaluating them over the edges of their
    own thresholds -- is reached by some case."""
    regs = C["HEAD_RB"] * C["HEAD_THREADS"]
    regs2 = C["HEAD_FWD_REGS2"] * C["HEAD_THREADS"]
    Ts = {1, C["PA_HEAD_MAX_T"], C["PA_HEAD_MAX_T"] + 1, C["FUSED_LOSS_MAX_T"] + 1, C["HEAD_INREG_MAX_T"] + 1,
          C["HEAD_GEMM_MIN_T"], C["HEAD_GEMM_MIN_T"] + 1}
    Bs = {2, C["PA_HEAD_MAX_B"], C["PA_HEAD_MAX_B"] + 1, regs, regs + 1, regs2, regs2 + 1}
    Us = {1, C["LOGITS_BN_LDS"] // C["LOGITS_BN_BYTES_PER_UNIT"] + 1}
    want = set()
    for T in Ts:
        for B in Bs:
            for U in Us:
                for path in ("autograd", "step"):
                    want |= dm.head_forms(U, T, B, path)
    for branch in ("logits_bn", "regs%d" % C["HEAD_RB"], "regs%d" % C["HEAD_FWD_REGS2"], "loop"):
        assert ("head_fwd", branch) in want
    assert not _missing(want), _missing(want)
    assert not _missing([("eval_logits", "kernel"), ("eval_logits", "gemm")])


def test_chunk_counts():
    qch = {f[1] for f in GOT if f[0] == "QCH"}
    assert 1 in qch and C["QCH_MAX"] in qch and any(1 < q < C["QCH_MAX"] for q in qch), qch
    # a QCH below ceil(max_batch / 128) because of the scratch cap, without an override
    capped = [c for c in dm.CASES if c.qch is None
              and dm.chunks(c.U, dm.nq_bucket(dm.pooled_len(c.L, c.k)), c.max_batch or c.B)[0]
              < min(C["QCH_MAX"], -(-(c.max_batch or c.B) // C["QCH_SEQS"]))]
    assert capped, "no case reaches a QCH capped by the scratch rule"
    # ACH at its maximum with chunks longer than two 128-sequence waves
    assert any(("ACH", C["ACH_MAX"]) in f and any(g[0] == "ach_per" and g[1] > 2 * 128 for g in f)
               for f in map(dm.case_forms, dm.CASES))
    # the overrides themselves: QCH 1 and 2, ACH 1 and 3, at a large-n bucket on each fc_fwd form
    over = {(c.qch, c.ach, dm.nq_bucket(dm.pooled_len(c.L, c.k)) > C["FC_BF_MAXN"]) for c in dm.CASES if c.qch}
    assert {q for q, _, _ in over} >= {1, 2} and {a for _, a, _ in over} >= {1, 3}
    assert {big for _, _, big in over} == {True, False}


def test_dense_path_shapes():
    want = [("dense", "k", 2), ("dense", "k", C["MAX_K"]), ("dense", "n", 1), ("dense", "n", dm.max_legal_n()),
            ("dense", "partials", "several"), ("dense", "ragged")]
    assert not _missing(want), _missing(want)
    units = {c.U for c in dm.CASES if c.dense}
    assert any(u % 4 for u in units) and any(u > 32 for u in units), units


@pytest.mark.parametrize("U,k,L,T", dm.UNSUPPORTED)
def test_unsupported_sizes_are_refused(U, k, L, T):
    with pytest.raises(dm.Unsupported):
        dm.forms(U, k, L, T, 4)


def test_unsupported_cases_cover_every_limit():
    ks = {k for _, k, _, _ in dm.UNSUPPORTED}
    ns = {dm.pooled_len(L, k) for _, k, L, _ in dm.UNSUPPORTED}
    assert {1, C["MAX_K"] + 1} <= ks and C["MAX_NQ"] + 1 in ns
    assert dm.max_legal_n() == C["MAX_NQ"] or dm.max_legal_n() + 1 in ns


def test_sweep_ids_are_unique_and_shapes_are_legal():
    ids = [c.id for c in dm.CASES]
    assert len(ids) == len(set(ids))
    for c in dm.CASES:
        dm.case_forms(c)                        # raises for a shape the library refuses
        assert c.B >= 2 and dm.pooled_len(c.L, c.k) >= 1


# ---- the entry points with launchers of their own: ISM, input gradient, the head of a bank --------
ENTRY = dm.entry_forms()


def _missing_entry(want):
    return sorted(set(want) - ENTRY, key=repr)


def test_ism_source_tables_agree():
    ks = range(2, C["MAX_K"] + 1)
    assert sorted({dm.ism_nw(k) for k in ks}) == C["ism_nw_cases"]
    assert [tc for _, tc in C["ism_sum_rules"]] == sorted(tc for _, tc in C["ism_sum_rules"])
    # every tile of input_grad_kernel finds its windows in IG_WMAX slots
    assert max(dm.ig_max_windows(k) for k in ks) <= C["IG_WMAX"]
    assert {dm.fc_ng(NQ) for NQ in C["buckets"]} == set(range(1, max(dm.fc_ng(NQ) for NQ in C["buckets"]) + 1))


def test_every_ism_form():
    want = [("ism_nw", NW) for NW in C["ism_nw_cases"]]
    want += [("ism_k_edge", NW, e) for NW in C["ism_nw_cases"] for e in ("lower", "upper")]
    # every task chunk at both sides of the thresholds and of the widest chunk, found by evaluating the rule
    tc_max = C["ism_sum_rules"][-1][1]
    Ts = {1, 2 * tc_max + 1}
    for tmax, _ in C["ism_sum_rules"]:
        Ts |= {tmax, tmax + 1} if tmax else {tc_max, tc_max + 1}
    for T in Ts:
        want += [f for f in dm.ism_forms(4, 5, 40, T, 3) if f[0] in ("ism_sum", "ism_sum_trips")]
    assert {f[1] for f in want if f[0] == "ism_sum"} == {tc for _, tc in C["ism_sum_rules"]}
    want += [("ism_subbatches", "one"), ("ism_subbatches", "several"), ("ism_n", 1)]
    want += [("ism_tail", r) for r in range(C["POOLW"])]
    assert not _missing_entry(want), _missing_entry(want)
    # the second trip of the sub-batch loop is ragged and the sub-batch is the smallest one
    sub = [c for c in dm.ISM_CASES if c.B > dm.ism_sub_batch(c.U, c.L, c.B)]
    assert any(dm.ism_sub_batch(c.U, c.L, c.B) == C["ISM_SUB_STEP"] and c.B % C["ISM_SUB_STEP"] for c in sub)


def test_every_input_grad_form():
    want = [("ig", mode) for mode in ("eval", "train", "train_dense")]
    ngs = sorted({dm.fc_ng(NQ) for NQ in C["buckets"] if dm.nq_lower(NQ) + 1 <= dm.max_legal_n()})
    want += [("ig_ng", g) for g in ngs] + [("ig_ng_edge", g, "lower") for g in ngs]
    want += [("ig_chunks", "several"), ("ig_chunks", "several", "big_n")]
    want += [("ig_units", e) for e in ("partial_wave", "partial_pass", "several_passes")]
    want += [("ig_batch", B) for B in dm.ig_batch_edges()]
    want += [("ig_pos", "ragged"), ("ig_wc", "ragged"), ("ig_wc", "several")]
    for mode in ("eval", "train"):
        want += [("ig_units_edge", mode, U) for U in dm.ig_unit_edges()]
        want += [("ig_k", mode, k) for k in (2, C["MAX_K"])] + [("ig_wmax", mode, k) for k in (2, C["MAX_K"])]
        want += [("ig_n", mode, 1), ("ig_tail", mode, C["POOLW"] - 1)]
    want += [("ig_k", "train_dense", C["MAX_K"]), ("ig_wmax", "train_dense", C["MAX_K"])]
    assert not _missing_entry(want), _missing_entry(want)
    # the widest filter meets the longest tail in one case, per mode
    for mode in ("eval", "train"):
        assert any({("ig_wmax", mode, C["MAX_K"]), ("ig_tail", mode, C["POOLW"] - 1)}
                   <= dm.ig_forms(c.U, c.k, c.L, c.T, c.B, c.mode) for c in dm.IG_CASES), mode


def _bank_wanted():
    """Every head form a bank can take, found by evaluating the rules over the edges of their own
    thresholds, at the member sizes a bank of two can have under the unit limit."""
    regs = C["HEAD_RB"] * C["HEAD_THREADS"]
    regs2 = C["HEAD_FWD_REGS2"] * C["HEAD_THREADS"]
    Ts = {1} | set(dm.bank_task_edges())
    Bs = {2, regs, regs + 1, regs2, regs2 + 1}
    Us = {1, C["LOGITS_UNITS_TRIP"] + 1, C["LOGITS_BN_UNITS_TRIP"] + 1, C["BANK_MAX_UNITS"] // 2}
    want = set()
    for T in Ts:
        for B in Bs:
            for U in Us:
                for path in ("autograd", "step"):
                    want |= dm.head_forms(U, T, B, path, G=2)
    return want


def test_every_bank_head_branch():
    want = _bank_wanted()
    assert all(f[0] in ("bank", "bank_units_trip") for f in want), "a bank form is not tagged"
    # a bank never rides in passA and never takes a GEMM
    assert not [f for f in want if "gemm" in f or any(str(v).startswith("passA") for v in f)]
    for branch in ("logits_bn", "regs%d" % C["HEAD_RB"], "regs%d" % C["HEAD_FWD_REGS2"], "loop"):
        assert ("bank", "head_fwd", branch) in want
    pairs = {f[2:] for f in want if f[:2] == ("bank", "head_bwd") and len(f) == 4}
    assert {b for b, _ in pairs} == {"fused_loss", "bank_loss", "kernel"} and {b for _, b in pairs} == {"inreg", "loop"}
    # t_edge carries the batch class of the case list: both sides of every task threshold below one block
    want = {f for f in want if f[:2] != ("bank", "t_edge")}
    want |= {("bank", "t_edge", T, "lt_block", "one_trip") for T in dm.bank_task_edges()}
    want |= {("bank", "units", "limit"), ("bank_units_trip", "logits", "several"),
             ("bank_units_trip", "logits_bn", "several")}
    assert not _missing_entry(want), _missing_entry(want)


def test_bank_logits_bn_lds_test_cannot_fail():
    """Unreachable, and reported as such: logits_bn_kernel's LDS test compares ONE member's statistics
    with the limit, and under BANK_MAX_UNITS no member of a bank (G >= 2) is large enough to fail it.
    So with few tasks a bank always takes logits_bn_kernel; head_fwd_train + logits_kernel is reached
    through T > HEAD_GEMM_MIN_T alone.  Raising the unit limit past this makes the branch live."""
    um_fail = C["LOGITS_BN_LDS"] // C["LOGITS_BN_BYTES_PER_UNIT"] + 1
    assert 2 * um_fail > C["BANK_MAX_UNITS"], "a bank can now fail the logits_bn LDS test: add a case"
    few = {f for f in _bank_wanted() if f[:2] == ("bank", "head_fwd")}
    for T in range(1, C["HEAD_GEMM_MIN_T"] + 1):
        for Um in (1, C["BANK_MAX_UNITS"] // 2):
            assert ("bank", "head_fwd", "logits_bn") in dm.head_forms(Um, T, 70, "step", G=2)
    assert few                                                  # (the set the loop above narrows)


def test_every_entry_case_is_needed():
    """Taking any one case out of the ISM, input-gradient or bank lists loses a form."""
    for name, cases in (("ism", dm.ISM_CASES), ("ig", dm.IG_CASES), ("bank", dm.BANK_CASES)):
        ids = [c.id for c in cases]
        assert len(ids) == len(set(ids)), name
        for i, c in enumerate(cases):
            rest = cases[:i] + cases[i + 1:]
            lost = ENTRY - dm.entry_forms(**{name: rest})
            assert lost, "%s adds no form of its own" % c.id
