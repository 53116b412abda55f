"""Which kernel forms a sync-BN step (csrc/syncbn.hip, engine.sync_phases, parallel.VirtualRanks) runs on
its ranks, and the case list of the sync-BN sweep (tests/test_gpu_syncbn_sweep.py).  Built on
tests/dispatch_model.py: every constant and bucket comes from dm.C and dm.forms, nothing is derived here
a second time.  tests/test_syncbn_dispatch_coverage.py checks on CPU that the cases reach every form.

Under sync-BN each rank launches the producers of the plain step at its own B_local (in a context sized
by its own max_batch) while prep1_stats, prep2 and mid normalise by B_global, and combine / distribute
kernels read the producers' partial buffers with the context's strides.  The head of the plain step does
not run: phase 4 is sync_bn3_fwd + the combiner, phases 5 and 6 are sync_loss / sync_head_sums /
sync_head_apply.

sync_forms(U, k, L, T, shards, max_batches, input, loss, backward, ...) returns a set of tuples:

  ("sync", f)                 f a producer form of dm.forms(U, k, L, T, B_r, max_batch_r, ("step",)) of some
                              rank r: NQ, nq_edge, qmom, fc_fwd, pa_ng, mid, conv_pool, conv_bwd,
                              conv_bwd_images, QCH, qch_per, ACH, ach_per
  ("sync_logits", "kernel"|"gemm")   phase 4's combiner: logits_kernel or gemm32_kernel (T > HEAD_GEMM_MIN_T)
  ("sync_T", T)
  ("sync_n", 1, "one_unit"|"several_units")   one pooled window: the smallest per-unit stride of every exchange
  ("sync_T_plain", T)         ... of a case with nothing else special: one-hot input, BCE on targets, no mask,
                              no frozen filters
  ("sync_shard", tag)         one (B_r = 1), below16 / at16 / above16 (1 < B_r < 16, 16, 17: the sequences
                              behind qs0's per-shard shift), below64 / at64 / above64 (63, 64, 65: the tile),
                              uneven, ranks8 (R >= 8), all_N_rank (a rank that holds only N)
  ("sync_shard_at", tag, "first"|"middle"|"last", "even"|"uneven")   where that edge shard sits among the
                              ranks (rank 0 opens every exchange sum and holds the first rows of the batch),
                              again of a case with nothing else special
  ("sync_chunks", "differ")   two ranks with different QCH or ACH (contexts of different max_batch)
  ("sync_chunks_order", "more_first"|"more_last")   ... and which end has more chunks
  ("sync_chunks", "mostly_empty")   a rank whose B_r fills fewer chunks than its context's QCH or ACH
  ("sync_chunks", "qch_filled"|"ach_filled")   a rank whose B_r fills more than one chunk: the distribute
                              kernels must clear what the producers left in the chunks behind the first
  ("sync_input", "onehot"|"codes"|"codes_rc")   phase 1: pack_tables_kernel on the caller's fp32 batch, or
                              launch_pack(nullptr) + prep1_tables on staged base codes
  ("sync_loss", "bce"|"mse"), ("sync_loss", loss, "kernel"|"gemm")
  ("sync_backward", "targets"|"dlogits_shard_mean"|"dlogits_free"), ("sync_backward", b, "kernel"|"gemm")
  ("sync_freeze", f)          freeze_top_n_filters = f > 0 (phase 8)
  ("sync_mask", "keep")       a recorded dropout keep mask split over the ranks
"""
import collections

import numpy as np

import dispatch_model as dm

C = dm.C
PRODUCER = ("NQ", "nq_edge", "qmom", "fc_fwd", "pa_ng", "mid", "conv_pool", "conv_bwd", "conv_bwd_images",
            "QCH", "qch_per", "ACH", "ach_per")
B_DEPENDENT = ("qch_per", "ach_per")        # producer forms that move with B at a fixed max_batch
SHARD_EDGES = {"below16": lambda b: 1 < b < 16, "at16": lambda b: b == 16, "above16": lambda b: b == 17,
               "below64": lambda b: b == 63, "at64": lambda b: b == 64, "above64": lambda b: b == 65,
               "one": lambda b: b == 1}
INPUTS = ("onehot", "codes", "codes_rc")
LOSSES = ("bce", "mse")
BACKWARDS = ("targets", "dlogits_shard_mean", "dlogits_free")


def rank_batches(shards, max_batches=None):
    """Per rank (B_r, max_batch of its context)."""
    mbs = max_batches or (None,) * len(shards)
    assert len(mbs) == len(shards)
    return [(b, max(b, mb or b)) for b, mb in zip(shards, mbs)]


def rank_chunks(U, k, L, shards, max_batches=None):
    """Per rank (QCH, ACH, chunks of QCH its B_r fills, chunks of ACH it fills)."""
    out = []
    for b, mb in rank_batches(shards, max_batches):
        f = dm.forms(U, k, L, 1, b, mb, ("step",))
        g = {v[0]: v[1] for v in f if v[0] in ("QCH", "qch_per", "ACH", "ach_per")}
        out.append((g["QCH"], g["ACH"], -(-b // g["qch_per"]), -(-b // g["ach_per"])))
    return out


def sync_forms(U, k, L, T, shards, max_batches=None, input="onehot", loss="bce", backward="targets",
               freeze=0, mask=False, n_rank=None):
    assert input in INPUTS and loss in LOSSES and backward in BACKWARDS
    assert len(shards) >= 2 and min(shards) >= 1
    f = set()
    for b, mb in rank_batches(shards, max_batches):
        f |= {("sync", v) for v in dm.forms(U, k, L, T, b, mb, ("step",)) if v[0] in PRODUCER}
    logits = "gemm" if T > C["HEAD_GEMM_MIN_T"] else "kernel"
    f |= {("sync_logits", logits), ("sync_T", T)}
    if dm.pooled_len(L, k) == 1:
        f.add(("sync_n", 1, "one_unit" if U == 1 else "several_units"))
    plain = (input, loss, backward, freeze, mask, n_rank) == ("onehot", "bce", "targets", 0, False, None)
    if plain:
        f.add(("sync_T_plain", T))
    R = len(shards)
    even = "even" if len(set(shards)) == 1 else "uneven"
    for r, b in enumerate(shards):
        pos = "first" if r == 0 else "last" if r == R - 1 else "middle"
        for tag, hit in SHARD_EDGES.items():
            if hit(b):
                f.add(("sync_shard", tag))
                if plain:
                    f.add(("sync_shard_at", tag, pos, even))
    if even == "uneven":
        f.add(("sync_shard", "uneven"))
    if R >= 8:
        f.add(("sync_shard", "ranks8"))
    if n_rank is not None:
        assert 0 <= n_rank < R
        f.add(("sync_shard", "all_N_rank"))
    ch = rank_chunks(U, k, L, shards, max_batches)
    if len({c[0] for c in ch}) > 1 or len({c[1] for c in ch}) > 1:
        f.add(("sync_chunks", "differ"))
        f.add(("sync_chunks_order", "more_first" if ch[0][:2] > ch[-1][:2] else "more_last"))
    if any(c[2] < c[0] or c[3] < c[1] for c in ch):
        f.add(("sync_chunks", "mostly_empty"))
    if any(c[2] > 1 for c in ch):
        f.add(("sync_chunks", "qch_filled"))
    if any(c[3] > 1 for c in ch):
        f.add(("sync_chunks", "ach_filled"))
    f |= {("sync_input", input), ("sync_loss", loss), ("sync_loss", loss, logits),
          ("sync_backward", backward), ("sync_backward", backward, logits)}
    if freeze > 0:
        f.add(("sync_freeze", freeze))
    if mask:
        f.add(("sync_mask", "keep"))
    return f


# ---- the sweep --------------------------------------------------------------------------------
# shards: B_r per rank; max_batches: the ranks' context sizes where they differ from B_r; n_rank: the rank
# whose rows are all N; bump: added to the seed (what the coverage test requires of the oracle's step)
SyncCase = collections.namedtuple(
    "SyncCase", "id group U k L T shards max_batches input loss backward freeze mask n_rank seed")


def _case(group, U, k, L, T, shards, max_batches=None, input="onehot", loss="bce", backward="targets",
          freeze=0, mask=False, n_rank=None, bump=0):
    shards = tuple(shards)
    if len(shards) > 4 and len(set(shards)) == 1:
        split = "%dx%d" % (shards[0], len(shards))
    else:
        split = "+".join(str(b) for b in shards)
    cid = "%s-U%d-k%d-L%d-T%d-%s%s%s%s%s%s%s%s" % (
        group, U, k, L, T, split, "-mb" + "+".join(str(b) for b in max_batches) if max_batches else "",
        "" if input == "onehot" else "-" + input, "" if loss == "bce" else "-" + loss,
        "" if backward == "targets" else "-" + backward, "-freeze%d" % freeze if freeze else "",
        "-mask" if mask else "", "-N%d" % n_rank if n_rank is not None else "")
    seed = (U * 131 + k * 17 + L + T * 29 + sum(shards) * 7 + len(shards)) % 10007 + bump
    return SyncCase(cid, group, U, k, L, T, shards, tuple(max_batches) if max_batches else None, input, loss,
                    backward, freeze, mask, n_rank, seed)


def build_cases():
    base = (5, 19, 200)
    t_gemm = C["HEAD_GEMM_MIN_T"] + 1
    cases = []
    # S. shard sizes at the edges the kernels care about
    # (two sequences in all: a BatchNorm over the batch outputs +-1 / sqrt(1 + eps / var), and what passes it
    # backwards is the eps residual.  A channel whose batch variance is near eps then has a gradient that the
    # rounding of its statistics sets, in any fp32 arithmetic; the seed is the first one at which every batch
    # variance of BatchNorm2 and BatchNorm3 is at least 100 eps -- the coverage test checks it on the oracle)
    cases.append(_case("S", *base, 2, (1, 1), bump=161))
    for shards in ((1, 40), (15, 17), (16, 16), (17, 15), (63, 65), (64, 64), (65, 1, 64), (2,) * 8):
        cases.append(_case("S", *base, 2, shards))
    # C. ranks whose contexts differ, and contexts larger than their shards
    cases.append(_case("C", *base, 2, (130, 70)))
    cases.append(_case("C", *base, 2, (70, 130)))
    cases.append(_case("C", *base, 2, (33, 31), max_batches=(400, 400)))
    # (several filled passA chunks, the last of one sequence: 256 + 1, and 128 + 128 + 1 of qmom's)
    cases.append(_case("C", *base, 2, (257, 257)))
    # N. the large-n kernels with small and uneven shards; the widest filter; one pooled window
    cases.append(_case("N", 5, 19, 1000, 2, (65, 64, 1)))
    cases.append(_case("N", 4, 32, 381, C["HEAD_GEMM_MIN_T"], (3, 64)))
    cases.append(_case("N", 3, 19, 25, 1, (17, 16)))
    cases.append(_case("N", 1, 2, 8, 1, (2, 1)))
    # T. the GEMM combiner one past its threshold and with a ragged 32-unit tile
    cases.append(_case("T", *base, t_gemm, (66, 64)))
    cases.append(_case("T", 33, 5, 61, 50, (65, 64)))
    # L. MSE through both combiners
    cases.append(_case("L", *base, 1, (33, 31), loss="mse"))
    cases.append(_case("L", *base, t_gemm, (33, 31), loss="mse"))
    # I. phase 1 on staged base codes; a rank whose pair counts are all zero
    cases.append(_case("I", *base, 2, (65, 63), input="codes"))
    cases.append(_case("I", *base, 2, (65, 63), input="codes_rc"))
    cases.append(_case("I", *base, 2, (65, 63), n_rank=1))
    # F. frozen filters (phase 8)
    cases.append(_case("F", *base, 2, (33, 31), freeze=2))
    # M. a recorded keep mask whose rows are split over uneven ranks
    cases.append(_case("M", *base, t_gemm, (40, 1, 23), mask=True))
    # D. the caller's dlogits: every rank's own shard-mean loss (dl_scale = B_r / B_global), and a free matrix
    for T in (2, t_gemm):
        for backward in ("dlogits_shard_mean", "dlogits_free"):
            cases.append(_case("D", *base, T, (5, 64, 1), backward=backward))
    return cases


CASES = build_cases()


def case_forms(c):
    return sync_forms(c.U, c.k, c.L, c.T, c.shards, c.max_batches, c.input, c.loss, c.backward, c.freeze,
                      c.mask, c.n_rank)


def all_forms(cases=None):
    got = set()
    for c in (CASES if cases is None else cases):
        got |= case_forms(c)
    return got


def bounds(c):
    """Row range [lo, hi) of every rank in the concatenated batch."""
    out, lo = [], 0
    for b in c.shards:
        out.append((lo, lo + b))
        lo += b
    return out


def to_codes(x):
    """Base codes 0..3 of a one-hot batch (B,4,L), 4 where the column is N."""
    codes = x.argmax(axis=1).astype(np.uint8)
    codes[x.sum(axis=1) == 0] = 4
    return codes


def inputs(c):
    """The case's inputs, as _inputs of the dispatch sweep builds them: a dict with
      sd     the state dict (|gamma1| in [0.6, 1.4], alternating sign)
      x      the ORACLE's input: the concatenated one-hot batch (of the reverse-complemented rows for codes_rc)
      codes  the device's input for the base-code cases (before any reverse complement), else None
      y      targets (binary for BCE, real for MSE)
      keep   the recorded keep mask (B, 100 U) or None
      D      the free dlogits matrix (B, T) or None"""
    from oracle import explainn_oracle as orc
    rng = np.random.default_rng(c.seed)
    B = sum(c.shards)
    sd = orc.random_state_dict(c.U, c.k, c.L, c.T, seed=c.seed)
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, c.U) * np.where(np.arange(c.U) % 2, 1, -1)).astype(np.float32)
    x = orc.random_onehot(B, c.L, seed=c.seed + 1, n_frac=0.01)
    if c.n_rank is not None:
        lo, hi = bounds(c)[c.n_rank]
        x[lo:hi] = 0
    codes = None
    if c.input != "onehot":
        codes = to_codes(x)
        if c.input == "codes_rc":
            x = np.ascontiguousarray(x[:, ::-1, ::-1])
    if c.loss == "mse":
        y = rng.standard_normal((B, c.T)).astype(np.float32)
    else:
        y = (rng.random((B, c.T)) > 0.5).astype(np.float32)
    keep = (rng.random((B, 100 * c.U)) > 0.3).astype(np.uint8) if c.mask else None
    D = None
    if c.backward == "dlogits_free":
        D = (rng.standard_normal((B, c.T)) / (B * c.T)).astype(np.float32)     # a loss gradient's scale
    return dict(sd=sd, x=x, codes=codes, y=y, keep=keep, D=D)
