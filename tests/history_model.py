"""The call-history walk of tests/test_gpu_call_history.py, as plain data (numpy only, no device).

A model object owns one device context: one allocation carved into scratch arrays that every entry
point shares, plus state that lives from call to call (the eval tables and their version, the
pending-work marks, the staged batch, the input mode, the sticky flag, tickets and per-chunk partial
sums sized by max_batch).  The property under test is HISTORY INDEPENDENCE: a call on a context that
has been through any earlier sequence of calls returns, bit for bit, what it returns on a fresh
context of the same geometry and max_batch.

This module says what "any earlier sequence" is:

  OP_CLASSES   one name per way of driving a context, with the C entry points it drives;
               header_gaps() reads include/explainn_hip.h and names every declared function that takes
               a context and is neither driven by a class or an event nor listed in EXEMPT.
  POINT_EVENTS things that happen between two ops and are ops of their own: one failed call per error
               family that returns after touching context state, and a switch of input mode.
  MODIFIERS    things that happen to an op: it runs inside an eval_cache() scope between two eval
               forwards (with or without a parameter change, CACHE_ROUTES), with a deferred bad
               batch's validation flag still pending, or at a batch above max_batch (the context is
               closed and re-created; with a train forward pending across it).
  GEOMETRIES   the three shapes, each with its classes, capacity and batch cycle.

walk(geometry) is a deterministic list of Items: an Eulerian circuit of the complete digraph on the
geometry's classes (every ordered pair of classes, self-pairs included, is adjacent once), then, for
every class X, every point event followed by X and X under every modifier.  The batch size cycles
through the geometry's list along the walk.  segments(geometry) cuts the walk into runs that overlap
by one item, each run driven from a fresh model; audit(geometry, items) lists what a walk lacks.

The chunk thresholds come from tests/dispatch_model.py, which reads them out of the sources.
"""
import collections
import os
import re

import numpy as np

import dispatch_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "explainn_hip.h")

# ---- op classes -------------------------------------------------------------------------------
# what every call through the Python layer's _stage may drive, whatever the class
STAGING = ("explainn_dense_input", "explainn_stage_onehot", "explainn_stage_codes", "explainn_input_flags")

# name -> (the entry points the class must be seen to call, what it is)
OP_CLASSES = collections.OrderedDict([
    ("step_fused", (("explainn_train_step",), "StepEngine.step: forward + loss + backward in one call")),
    ("step_split", (("explainn_train_step_fc", "explainn_train_step_conv"), "StepEngine.step in its two halves")),
    ("train_mask", (("explainn_forward_train", "explainn_backward"),
                    "autograd train forward + backward, replayed dropout keep-mask")),
    ("train_seed", (("explainn_forward_train", "explainn_backward"),
                    "autograd train forward + backward, built-in dropout at a fixed seed")),
    ("train_dx", (("explainn_forward_train", "explainn_backward_input"),
                  "autograd train forward + backward with x.grad")),
    ("train_nograd", (("explainn_forward_train", "explainn_debug_keep_bits"),
                      "train forward under no_grad, and the keep bits it left")),
    ("eval_onehot", (("explainn_forward_eval",), "eval forward from fp32 one-hot")),
    ("eval_codes", (("explainn_forward_eval", "explainn_stage_codes"), "eval forward from BaseCodes, both strands")),
    ("eval_soft", (("explainn_forward_eval", "explainn_dense_input"), "eval forward of soft input, dense kernels")),
    ("input_grad", (("explainn_forward_eval_keep", "explainn_input_grad"), "eval-keep forward + input_gradient")),
    ("ism", (("explainn_ism",), "in_silico_mutagenesis")),
    ("ig_zero", (("explainn_integrated_gradients",), "integrated_gradients, zero baseline")),
    ("ig_shuffle", (("explainn_integrated_gradients",), "integrated_gradients, dinucleotide-shuffle baseline")),
    ("scan", (("explainn_scan",), "scan of SequenceWindows, staged windows and the shared track")),
    ("score_edits", (("explainn_score_edits",), "EditedWindows scoring")),
    ("score_haplotypes", (("explainn_score_haplotypes",), "HaplotypeWindows scoring")),
    ("call_sites", (("explainn_call_sites",), "site calling")),
    ("record_best", (("explainn_record_best",), "best site per record")),
    ("act_histogram", (("explainn_activation_histogram",), "activation histogram")),
    ("unit_outputs", (("explainn_unit_outputs",), "model.linears(x)")),
    ("unit_activations", (("explainn_unit_activations",), "model.linears[:3](x)")),
    ("filter_export", (("explainn_filter_act_max", "explainn_filter_sites"), "filter_act_max + filter_sites")),
    ("sync_step", (("explainn_sync_phase",), "one-rank sync-BN step through StepEngine.sync_phases")),
    ("staged_raw", (("explainn_stage_windows", "explainn_stage_edited_windows", "explainn_stage_haplotype_windows",
                     "explainn_forward_eval", "explainn_unit_outputs", "explainn_forward_train",
                     "explainn_loss_grad", "explainn_backward"),
                    "the three window stagers at the C ABI, each followed by an x == NULL call")),
])

TRAIN_CLASSES = ("step_fused", "step_split", "train_mask", "train_seed", "train_dx", "train_nograd", "sync_step",
                 "staged_raw")
# classes whose size is not a batch of the context (they take a sequence, not B rows)
NO_BATCH = ("call_sites", "record_best", "act_histogram")
# classes whose Python entry reads the validation flag before computing, whatever validate_input says
# (VALIDATE_FIRST / ONEHOT_ONLY in architectures.ExplaiNN._stage): a flag left pending by an earlier
# deferred batch is read, checked and cleared right before them, not after
READS_FLAG_FIRST = ("train_dx", "input_grad", "ism", "ig_zero")
# what a bank refuses (EXPLAINN_E_UNSUPPORTED / ValueError in the Python layer)
MEMBER_ONLY = ("train_dx", "input_grad", "ism", "ig_zero", "ig_shuffle", "sync_step")
# the classes whose kernels depend on the pooled length
LARGE_N_CLASSES = ("step_fused", "train_mask", "eval_onehot", "input_grad", "ism", "ig_zero", "scan")

# ---- events -----------------------------------------------------------------------------------
# (a) failed calls + (c) the mode switch: ops of their own, compared like any other op
POINT_EVENTS = collections.OrderedDict([
    ("err_arg", (("explainn_scan_workspace_bytes",),
                 "an argument error after the front half ran: a shared-track scan at a stride that is no multiple of 7")),
    ("err_state_conv", (("explainn_train_step_conv",), "E_STATE: a _conv half without its _fc half")),
    ("err_state_backward", (("explainn_forward_train", "explainn_forward_eval", "explainn_backward"),
                            "E_STATE: a backward after an eval call, in Python and at the C ABI")),
    ("err_unsupported", ((), "E_UNSUPPORTED: the member-only entry points on a bank; the filter export in dense "
                             "input mode on a single model")),
    ("err_not_onehot", (("explainn_stage_onehot", "explainn_input_flags"),
                        "a batch that is not one-hot under dense_input=False")),
    ("mode_switch", (("explainn_dense_input", "explainn_stage_codes", "explainn_input_flags"),
                     "soft/dense -> base codes -> fp32 one-hot, then the sticky flag read and cleared")),
])
ERROR_FAMILIES = ("err_arg", "err_state_conv", "err_state_backward", "err_unsupported", "err_not_onehot")
# on a bank err_unsupported calls these and expects E_UNSUPPORTED from each
BANK_UNSUPPORTED = ("explainn_forward_eval_keep", "explainn_input_grad", "explainn_backward_input", "explainn_ism",
                    "explainn_integrated_gradients", "explainn_sync_phase")

# (b) routes by which parameters change inside an eval_cache() scope: those of
# tests/test_gpu_parity.py::test_eval_tables_follow_parameter_changes
CACHE_ROUTES = ("inplace", "train_step", "adam", "load_state_dict", "reassign", "data_invalidate")
# (b), (c) and (d) as things that happen to the op they precede
MODIFIERS = collections.OrderedDict([
    ("cache_none", "inside eval_cache(), between two eval forwards, no parameter change: the second uses cached tables"),
    ("cache_change", "inside eval_cache(), between two eval forwards, parameters changed by one of CACHE_ROUTES"),
    ("pending_flag", "a deferred, unvalidated bad batch ran before; its flag is pending when the op runs"),
    ("growth", "the op's batch is max_batch + 1: the context is closed and re-created"),
    ("growth_pending", "as growth, with a train forward awaiting its backward: the backward must raise stale"),
])
EVENTS = tuple(POINT_EVENTS) + tuple(MODIFIERS)

# ---- the header -------------------------------------------------------------------------------
# declared functions that take a context and are in no class: why
EXEMPT = {
    "explainn_create": "makes the context",
    "explainn_create_bank": "makes the context",
    "explainn_destroy": "ends the context",
    "explainn_groups": "reads a constant of the context",
    "explainn_scratch_bytes": "reads a constant of the context",
    "explainn_ism_workspace_bytes": "size query: reads the geometry, writes nothing",
    "explainn_integrated_gradients_workspace_bytes": "size query: reads the geometry, writes nothing",
    "explainn_scan_workspace_bytes": "size query (err_arg calls it for its error code)",
    "explainn_call_sites_workspace_bytes": "size query: reads the geometry, writes nothing",
    "explainn_sync_exchange_elems": "size query: reads the geometry, writes nothing",
    "explainn_stage_timing": "measurement aid: brackets stages with events, changes no result",
    "explainn_stage_times": "measurement aid: reads the events",
}


def context_functions(text=None):
    """Names of the functions include/explainn_hip.h declares with an explainn_ctx parameter."""
    if text is None:
        with open(HEADER) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(explainn_\w+)\s*\(([^;{}]*?)\)\s*;", text, re.S):
        if re.search(r"\bexplainn_ctx\s*\*", m.group(2)):
            out.append(m.group(1))
    return out


def driven(classes=None, events=None):
    """Every entry point some class or point event declares it drives."""
    got = set(STAGING)
    for name, (fns, _) in OP_CLASSES.items():
        if classes is None or name in classes:
            got |= set(fns)
    for name, (fns, _) in POINT_EVENTS.items():
        if events is None or name in events:
            got |= set(fns)
    if events is None or "err_unsupported" in events:
        got |= set(BANK_UNSUPPORTED)
    return got


def header_gaps(text=None, classes=None, events=None, exempt=None):
    """Context-taking functions of the header that no class drives and EXEMPT does not list."""
    exempt = EXEMPT if exempt is None else exempt
    have = driven(classes, events)
    return [f for f in context_functions(text) if f not in have and f not in exempt]


# ---- geometries -------------------------------------------------------------------------------
Geometry = collections.namedtuple("Geometry", "name G U k L T cap batches classes env segment")

_ALL = tuple(OP_CLASSES)
GEOMETRIES = collections.OrderedDict((g.name, g) for g in (
    # the smallest single model with two unit quads (one padded), a pooling tail, three q chunks and two
    # passA chunks.  Every shrink of the cycle follows 300 or 257.  A grid this small keeps BatchNorm1's
    # statistics in launches of their own (convpool.hip, conv_pool_bn1_workgroups); EXPLAINN_BN1_AUX = 8k,
    # the count the large grids take, moves them into the filter-bank launch, whose workgroups meet at
    # the context's bn1_ticket: state that must be re-armed per call.  The other two geometries keep the
    # separate launches.
    Geometry("small", 1, 6, 9, 74, 2, 300, (300, 1, 257, 2, 300, 64, 257, 70, 300, 128, 257, 129, 300), _ALL,
             {"EXPLAINN_BN1_AUX": "72"}, 250),
    # n = 140: qmom_big, passB<140>, the fp32 fc_fwd
    Geometry("large_n", 1, 3, 19, 1000, 2, 300, (300, 1, 257, 2, 300, 64, 257, 70, 300, 128, 257, 129, 300),
             LARGE_N_CLASSES, {}, 100),
    # three members of 4 units, T = 5 (the looped head bodies).  max_batch 200 gives one passA chunk:
    # EXPLAINN_ACH=2 makes it two, for the context under test and its fresh twin alike.
    Geometry("bank", 3, 4, 9, 74, 5, 200, (200, 1, 129, 2, 200, 64, 129, 70, 200, 128, 129),
             tuple(c for c in _ALL if c not in MEMBER_ONLY), {"EXPLAINN_ACH": "2"}, 220),
))


def pooled(g):
    return dm.pooled_len(g.L, g.k)


def chunk_counts(g, cap=None):
    """(QCH, ACH) of a context of this geometry at max_batch `cap`, the geometry's overrides included."""
    ach = int(g.env["EXPLAINN_ACH"]) if "EXPLAINN_ACH" in g.env else None
    qch = int(g.env["EXPLAINN_QCH"]) if "EXPLAINN_QCH" in g.env else None
    return dm.chunks(g.G * g.U, dm.nq_bucket(pooled(g)), g.cap if cap is None else cap, qch, ach)


def filled(g, B, cap=None):
    """(q chunks, passA chunks) a train call of B sequences produces; the others are gathered unproduced."""
    key = (g.name, B, cap)
    if key not in _FILLED:
        _FILLED[key] = _filled(g, B, cap)
    return _FILLED[key]


_FILLED = {}


def _filled(g, B, cap):
    f = dict((v[0], v[1]) for v in dm.forms(g.G * g.U, g.k, g.L, 1, B, max_batch=g.cap if cap is None else cap,
                                              qch=chunk_counts(g, cap)[0], ach=chunk_counts(g, cap)[1])
             if v[0] in ("qch_per", "ach_per"))
    return -(-B // f["qch_per"]), -(-B // f["ach_per"])


def is_big(g, B):
    q, a = filled(g, B)
    return q >= 2 and a >= 2


def is_small(g, B):
    return filled(g, B) == (1, 1)


def edge_batches(g):
    """Batch sizes the cycle must hold: 1, 2, the capacity, the 64-sequence tile and a ragged second tile,
    the q chunk size and one more, one more than the passA chunk size (where the capacity allows)."""
    tile = dm.C["IG_SEQS"]
    want = {1, 2, g.cap, tile, tile + 6}
    for b in (dm.C["QCH_SEQS"], dm.C["QCH_SEQS"] + 1, dm.C["ACH_SEQS"] + 1):
        if b <= g.cap:
            want.add(b)
    return sorted(want)


# ---- the walk ---------------------------------------------------------------------------------
# pos: index in the walk; cls: an op class or a point event; B: the batch (the cycle's, before a growth
# modifier raises it); mod: a modifier or None; route: the parameter-change route of cache_change;
# seed: what the input builder is seeded with
Item = collections.namedtuple("Item", "pos cls B mod route seed")


def euler_circuit(n):
    """Node indices of an Eulerian circuit of the complete digraph with self-loops on n nodes: n*n + 1
    entries, every ordered pair adjacent exactly once (Hierholzer, successors tried in a fixed order)."""
    used = [0] * n
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if used[v] < n:
            w = (v + used[v]) % n
            used[v] += 1
            stack.append(w)
        else:
            out.append(stack.pop())
    out.reverse()
    assert len(out) == n * n + 1
    return out


def _coverage(g, runs, cset):
    """What audit() counts: (pairs, event -> class, modifier x class, class x batch, routes, classes that
    shrink after a big batch, train classes that shrink after a big batch of a train class)."""
    pairs, after, under, sizes, route_seen, shrink, train_shrink = set(), set(), set(), set(), set(), set(), set()
    for run in runs:
        prev = None
        for it in run:
            if it.cls in cset:
                sizes.add((it.cls, it.B))
                if it.mod:
                    under.add((it.mod, it.cls))
                    if it.route:
                        route_seen.add(it.route)
                if prev is not None and prev.cls in cset:
                    # a modifier wraps the op in calls of its own: the pair counts only without one
                    if it.mod is None and prev.mod is None:
                        pairs.add((prev.cls, it.cls))
                        if is_small(g, it.B) and is_big(g, prev.B):
                            shrink.add(it.cls)
                            if prev.cls in TRAIN_CLASSES and it.cls in TRAIN_CLASSES:
                                train_shrink.add(it.cls)
                elif prev is not None and it.mod is None:
                    after.add((prev.cls, it.cls))
            prev = it
    return pairs, after, under, sizes, route_seen, shrink, train_shrink


def walk(g, classes=None, point_events=None, modifiers=None, batches=None, routes=None):
    """The walk of geometry g; the other arguments replace the module's lists (the model's own test
    removes one name at a time and asks audit() what was lost).

    1. the Eulerian circuit of the classes; 2. per class, every point event followed by the class, and
    the class under every modifier; 3. what the batch cycle, blind to the classes, left out: a class at
    a batch size it has not met, and a class at the largest one-chunk batch right after a train class
    at the largest batch."""
    classes = list(g.classes if classes is None else classes)
    point_events = list(POINT_EVENTS if point_events is None else point_events)
    modifiers = list(MODIFIERS if modifiers is None else modifiers)
    batches = list(g.batches if batches is None else batches)
    routes = list(CACHE_ROUTES if routes is None else routes)
    seq = [(classes[i], None, None, None) for i in euler_circuit(len(classes))] if classes else []
    for ci, cls in enumerate(classes):
        for ev in point_events:
            seq.append((ev, None, None, None))
            seq.append((cls, None, None, None))
        for mod in modifiers:
            if mod == "cache_change" and not routes:
                continue
            seq.append((cls, mod, routes[ci % len(routes)] if mod == "cache_change" else None, None))
    if "cache_change" in modifiers and classes:              # every route, whatever the class count
        for r in routes[len(classes):]:
            seq.append((classes[0], "cache_change", r, None))

    def items_of(seq):
        out = []
        for pos, (cls, mod, route, B) in enumerate(seq):
            if B is None:
                B = batches[pos % len(batches)] if batches else 0
            if mod in ("growth", "growth_pending") and batches:
                B = max(batches)          # (the executor adds what it takes to exceed the context's max_batch)
            out.append(Item(pos, cls, B, mod, route, 1000 + pos))
        return out

    if classes and batches:
        _, _, _, sizes, _, shrink, train_shrink = _coverage(g, [items_of(seq)], set(classes))
        small = [B for B in batches if is_small(g, B)]
        lead = [c for c in classes if c in TRAIN_CLASSES] or classes
        for cls in classes:
            if cls in NO_BATCH:
                continue
            for B in sorted(set(batches)):
                if (cls, B) not in sizes:
                    seq.append((cls, None, None, B))
            if small and (cls not in shrink or (cls in TRAIN_CLASSES and cls not in train_shrink)):
                seq.append((lead[0], None, None, max(batches)))
                seq.append((cls, None, None, max(small)))
    return items_of(seq)


_WALKS = {}


def segments(g, items=None):
    """The walk in runs of at most g.segment + 1 items; run i + 1 starts with the last item of run i, so
    every adjacent pair of the walk is adjacent in some run.  Each run is driven from a fresh model."""
    if items is None:
        if g.name not in _WALKS:
            _WALKS[g.name] = walk(g)
        items = _WALKS[g.name]
    out, i = [], 0
    while i < len(items) - 1:
        out.append(items[i:i + g.segment + 1])
        i += g.segment
    return out


def audit(g, runs, classes=None, point_events=None, modifiers=None, batches=None, routes=None):
    """What the runs (lists of Items, as segments() gives them) lack of the properties the GPU test
    relies on, as a list of sentences that name what is missing; empty when all hold."""
    classes = list(g.classes if classes is None else classes)
    point_events = list(POINT_EVENTS if point_events is None else point_events)
    modifiers = list(MODIFIERS if modifiers is None else modifiers)
    batches = sorted(set(g.batches if batches is None else batches))
    routes = list(CACHE_ROUTES if routes is None else routes)
    pairs, after, under, sizes, route_seen, shrink, train_shrink = _coverage(g, runs, set(classes))
    lost = []
    for a in classes:
        for b in classes:
            if (a, b) not in pairs:
                lost.append("pair %s -> %s is in no run" % (a, b))
    for ev in point_events:
        for c in classes:
            if (ev, c) not in after:
                lost.append("class %s never follows event %s" % (c, ev))
    for mod in modifiers:
        for c in classes:
            if (mod, c) not in under:
                lost.append("class %s never runs under %s" % (c, mod))
    if "cache_change" in modifiers:
        for r in routes:
            if r not in route_seen:
                lost.append("cache route %s changes no parameters inside a scope" % r)
    for c in classes:
        if c in NO_BATCH:
            continue
        for B in batches:
            if (c, B) not in sizes:
                lost.append("class %s never runs at batch size %d" % (c, B))
        if c not in shrink:
            lost.append("class %s never runs a one-chunk batch right after one that filled two q and two passA chunks" % c)
        if c in TRAIN_CLASSES and c not in train_shrink:
            lost.append("train class %s never shrinks right after a train class filled two q and two passA chunks" % c)
    for B in edge_batches(g):
        if B not in batches:
            lost.append("batch size %d is not in the cycle" % B)
    cyc = list(g.batches)
    for i, B in enumerate(cyc):
        nxt = cyc[(i + 1) % len(cyc)]
        if nxt < B and not is_big(g, B):
            lost.append("the cycle shrinks %d -> %d from a batch that did not fill two q and two passA chunks" % (B, nxt))
    # the chunk structure the walk relies on must survive every growth of a run (max_batch + 1 each time)
    for run in runs:
        grown = g.cap + sum(1 for it in run if it.mod in ("growth", "growth_pending"))
        if chunk_counts(g, grown) != chunk_counts(g) or min(chunk_counts(g)) < 2:
            lost.append("chunk counts %s at max_batch %d (%s at %d)" % (chunk_counts(g, grown), grown,
                                                                      chunk_counts(g), g.cap))
            break
    return lost


# ---- inputs -----------------------------------------------------------------------------------
def onehot(codes):
    x = np.zeros((codes.shape[0], 4, codes.shape[1]), dtype=np.float32)
    for a in range(4):
        x[:, a, :] = codes == a
    return x


def build_inputs(g, B, seed):
    """Every input an op of B sequences may take, as numpy arrays, from `seed` alone."""
    rng = np.random.default_rng(seed)
    U, L, T = g.G * g.U, g.L, g.T
    codes = rng.integers(0, 4, size=(B, L)).astype(np.uint8)
    codes[rng.random((B, L)) < 0.02] = 4
    soft = rng.random((B, 4, L)).astype(np.float32) + 0.05
    soft /= soft.sum(1, keepdims=True)
    S = 7 * B + L + 40
    seq = rng.integers(0, 4, size=S).astype(np.uint8)
    seq[rng.random(S) < 0.02] = 4
    d = {
        "codes": codes, "x": onehot(codes), "soft": soft,
        "y": (rng.random((B, T)) > 0.5).astype(np.float32),
        "dl": rng.standard_normal((B, g.G, T) if g.G > 1 else (B, T)).astype(np.float32),
        "mask": (rng.random((B, 100 * U)) > 0.3).astype(np.uint8),
        "select": (rng.random(B) > 0.2).astype(np.uint8),
        "seq": seq,
        "rec_offsets": np.append(np.arange(0, S, 50), S).astype(np.int64),
        "thresholds": np.full(U, 1.0, dtype=np.float32),
    }
    # one edit per row (explainn_edits)
    E = 8
    alt_len = rng.integers(0, 4, E).astype(np.int32)
    d["edits"] = {
        "row_start": rng.integers(-5, S - L + 5, B).astype(np.int64),
        "row_edit": rng.integers(-1, E, B).astype(np.int32),
        "pos": rng.integers(0, S, E).astype(np.int64),
        "ref_len": rng.integers(0, 4, E).astype(np.int32),
        "alt_len": alt_len,
        "alt_off": (np.cumsum(alt_len) - alt_len).astype(np.int32),
        "alt": rng.integers(0, 4, max(int(alt_len.sum()), 1)).astype(np.uint8),
    }
    # runs of up to two ordered, non-overlapping edits per row (explainn_haplotypes)
    E = S // 10
    alt_len = rng.integers(0, 4, E).astype(np.int32)
    count = rng.integers(0, 3, B).astype(np.int32)
    first_edit = rng.integers(0, E - 2, B)
    d["haps"] = {
        "row_start": rng.integers(-5, S - L + 5, B).astype(np.int64),
        "row_first": (np.cumsum(count) - count).astype(np.int64),
        "row_count": count,
        "edit_index": np.concatenate([np.arange(f, f + c) for f, c in zip(first_edit, count)] + [np.zeros(1)]).astype(np.int32),
        "pos": (10 * np.arange(E) + 3).astype(np.int64),
        "ref_len": rng.integers(0, 4, E).astype(np.int32),
        "alt_len": alt_len,
        "alt_off": (np.cumsum(alt_len) - alt_len).astype(np.int32),
        "alt": rng.integers(0, 4, max(int(alt_len.sum()), 1)).astype(np.uint8),
    }
    return d
