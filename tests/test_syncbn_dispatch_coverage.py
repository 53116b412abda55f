"""The sync-BN sweep (tests/test_gpu_syncbn_sweep.py) reaches every producer form, shard edge, input,
loss and backward a sync-BN step can run.  CPU only: tests/syncbn_dispatch_model.py builds the forms from
tests/dispatch_model.py, which reads the constants from the sources.  The last test checks, from the fp64
reference alone, the condition that keeps the sweep's gradient comparison honest."""
import numpy as np
import pytest

import dispatch_model as dm
import syncbn_dispatch_model as sm
from oracle import explainn_oracle as orc
from parity_util import knife_masks

C = dm.C
GOT = sm.all_forms()


def _missing(want, got=GOT):
    return sorted(set(want) - got, key=repr)


def _wanted():
    """Every tuple the sweep has to reach, none of it read from sm.CASES."""
    t_min = C["HEAD_GEMM_MIN_T"]
    want = [("sync_logits", "kernel"), ("sync_logits", "gemm")]
    # both sides of the combiner threshold by a step with nothing else special; one task; many tasks
    want += [("sync_T", 1), ("sync_T_plain", t_min), ("sync_T_plain", t_min + 1), ("sync_T", 50)]
    want += [("sync_shard", tag) for tag in ("one", "below16", "at16", "above16", "below64", "at64", "above64",
                                              "uneven", "ranks8", "all_N_rank")]
    # one sequence as half of the smallest batch, next to a larger shard and between two; the shards around
    # qs0's 16 sequences as the first and the last rank; the even splits at 16 and at the 64-sequence tile
    want += [("sync_shard_at", "one", "first", "even"), ("sync_shard_at", "one", "first", "uneven"),
             ("sync_shard_at", "one", "middle", "uneven")]
    want += [("sync_shard_at", tag, pos, "uneven") for tag in ("below16", "above16") for pos in ("first", "last")]
    want += [("sync_shard_at", "at16", "first", "even"), ("sync_shard_at", "at64", "first", "even"),
             ("sync_shard_at", "below64", "first", "uneven"), ("sync_shard_at", "above64", "last", "uneven")]
    want += [("sync_chunks", "differ"), ("sync_chunks", "mostly_empty"), ("sync_chunks", "qch_filled"),
             ("sync_chunks", "ach_filled"),
             ("sync_chunks_order", "more_first"), ("sync_chunks_order", "more_last")]
    want += [("sync_input", v) for v in sm.INPUTS]
    want += [("sync_loss", v) for v in sm.LOSSES] + [("sync_backward", v) for v in sm.BACKWARDS]
    for form in ("kernel", "gemm"):
        want += [("sync_loss", "mse", form), ("sync_backward", "dlogits_shard_mean", form),
                 ("sync_backward", "dlogits_free", form)]
    want += [("sync_freeze", 2), ("sync_mask", "keep"), ("sync_n", 1, "one_unit"), ("sync_n", 1, "several_units")]
    # the producers whose partial buffers the combine kernels read with other strides or loop counts
    want += [("sync", f) for f in (("qmom", "small"), ("qmom", "big"), ("mid", "fused"), ("mid", "big"),
                                   ("fc_fwd", "bf16"), ("fc_fwd", "fp32"))]
    # (passA's row groups up to those of C4's pooled length, 140; the plain sweep holds the one bucket beyond)
    want += [("sync", ("pa_ng", g)) for g in range(1, dm.pa_ng(140) + 1)]
    want += [("sync", ("conv_bwd", 2)), ("sync", ("conv_bwd", C["MAX_K"])), ("sync", ("NQ", C["buckets"][0])),
             ("sync", ("NQ", C["buckets"][-2]))]
    return want


def test_sweep_reaches_every_sync_form():
    assert not _missing(_wanted()), _missing(_wanted())
    assert any(f[0] == "sync" and f[1][0] == "conv_bwd_images" for f in GOT), \
        "no sync case with several LDS images per conv_bwd workgroup"
    # several chunks on one rank next to one chunk on another
    qch = {f[1][1] for f in GOT if f[0] == "sync" and f[1][0] == "QCH"}
    ach = {f[1][1] for f in GOT if f[0] == "sync" and f[1][0] == "ACH"}
    assert min(qch) == 1 and max(qch) > 2 and min(ach) == 1 and max(ach) > 1, (qch, ach)


def test_sync_forms_are_the_producers_only():
    """The head forms of the plain step do not run under sync and are not counted."""
    for f in GOT:
        if f[0] == "sync":
            assert f[1][0] in sm.PRODUCER, f
    assert not [f for f in GOT if f[0] == "sync" and f[1][0].startswith(("head", "logits", "eval"))]


def test_batch_dependent_producer_forms_of_the_plain_sweep():
    """Every producer form that moves with the batch and that the plain sweep's batch / chunk groups (D, E)
    reach at B <= 400 is reached by a sync case, on a rank that is one of several."""
    ref = [c for c in dm.CASES if c.group in ("D", "E") and c.B <= 400]
    assert ref, "the plain sweep has no D / E case at B <= 400 any more"
    want = {("sync", f) for c in ref for f in dm.case_forms(c) if f[0] in sm.B_DEPENDENT}
    assert want
    assert all(len(c.shards) >= 2 for c in sm.CASES)
    assert not _missing(want), _missing(want)


def test_every_case_is_needed():
    """Taking any one case out of the list loses a form that the sweep has to reach."""
    ids = [c.id for c in sm.CASES]
    assert len(ids) == len(set(ids))
    want = set(_wanted())
    for i, c in enumerate(sm.CASES):
        lost = _missing(want, sm.all_forms(sm.CASES[:i] + sm.CASES[i + 1:]))
        assert lost, "%s reaches no wanted form of its own" % c.id


def test_cases_are_legal():
    for c in sm.CASES:
        n = dm.check_supported(c.U, c.k, c.L, c.T)
        assert n >= 1 and sum(c.shards) >= 2 and min(c.shards) >= 1, c.id
        assert c.freeze < c.U
        for b, mb in sm.rank_batches(c.shards, c.max_batches):
            assert mb >= b


@pytest.mark.parametrize("case", sm.CASES, ids=[c.id for c in sm.CASES])
def test_knife_edges_stay_an_exception(case):
    """compare_grads gives knife-edge rows only the loose bound and has no cap on how many rows that is.  So
    for every sync case the fp64 oracle on the concatenated batch must leave at least half of the units
    outside knife_masks -- all of them when U <= 2 -- and mask under 2 % of the channels."""
    d = sm.inputs(case)
    _, cache, _ = orc.forward(d["sd"], d["x"], training=True, dropout_mask=d["keep"], return_cache=True,
                              dtype=np.float64)
    ch, un = knife_masks(cache, case.U)
    clean = int((~un).sum())
    assert ch.mean() < 0.02, (case.id, float(ch.mean()))
    assert 2 * clean >= case.U, (case.id, clean)
    if case.U <= 2:
        assert clean == case.U, (case.id, clean)


def test_two_sequence_batch_is_resolved():
    """B_global = 2: a BatchNorm over the batch outputs +-1 / sqrt(1 + eps / var) and passes backwards only the
    eps residual, eps / (var + eps) of the difference of its two gradients.  Where a channel's batch variance
    is near eps that residual is set by the rounding of the statistics, whatever the fp32 arithmetic, and a
    comparison would measure that instead of the kernels: every batch variance of BatchNorm2 and BatchNorm3
    (from the fp64 oracle) is at least 100 eps in the two-sequence case."""
    eps = 1e-5
    two = [c for c in sm.CASES if sum(c.shards) == 2]
    assert two, "no case with two sequences in all"
    for c in two:
        d = sm.inputs(c)
        _, cache, _ = orc.forward(d["sd"], d["x"], training=True, return_cache=True, dtype=np.float64)
        for inv in (cache["inv2"], cache["inv3"]):
            assert (1.0 / np.asarray(inv) ** 2 - eps).min() >= 100 * eps, c.id
