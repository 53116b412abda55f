"""The call-history walk (tests/history_model.py) has what tests/test_gpu_call_history.py relies on: every
ordered pair of op classes, every event in front of every class, the shrinks after batches that filled
several chunks, every context-taking function of the header placed -- and losing any name of its lists
is noticed, by name.  CPU only."""
import pytest

import history_model as hm

# What the walk must hold, restated here on purpose: deleting a name from history_model fails this file.
CLASSES = ["step_fused", "step_split", "train_mask", "train_seed", "train_dx", "train_nograd", "eval_onehot",
           "eval_codes", "eval_soft", "input_grad", "ism", "ig_zero", "ig_shuffle", "scan", "score_edits",
           "score_haplotypes", "call_sites", "record_best", "act_histogram", "unit_outputs", "unit_activations",
           "filter_export", "sync_step", "staged_raw"]
POINT_EVENTS = ["err_arg", "err_state_conv", "err_state_backward", "err_unsupported", "err_not_onehot", "mode_switch"]
MODIFIERS = ["cache_none", "cache_change", "pending_flag", "growth", "growth_pending"]
ROUTES = ["inplace", "train_step", "adam", "load_state_dict", "reassign", "data_invalidate"]
BATCHES = {"small": [1, 2, 64, 70, 128, 129, 257, 300], "large_n": [1, 2, 64, 70, 128, 129, 257, 300],
           "bank": [1, 2, 64, 70, 128, 129, 200]}
LARGE_N = ["step_fused", "train_mask", "eval_onehot", "input_grad", "ism", "ig_zero", "scan"]
MEMBER_ONLY = ["train_dx", "input_grad", "ism", "ig_zero", "ig_shuffle", "sync_step"]

GEOMS = list(hm.GEOMETRIES.values())
IDS = [g.name for g in GEOMS]


def test_the_lists_hold_every_name():
    for what, want, have in (("op class", CLASSES, hm.OP_CLASSES), ("point event", POINT_EVENTS, hm.POINT_EVENTS),
                             ("modifier", MODIFIERS, hm.MODIFIERS), ("cache route", ROUTES, hm.CACHE_ROUTES)):
        lost = [n for n in want if n not in have]
        assert not lost, "%s lost from history_model: %s" % (what, ", ".join(lost))
    assert sorted(hm.GEOMETRIES) == sorted(BATCHES)
    for g in GEOMS:
        lost = [B for B in BATCHES[g.name] if B not in g.batches]
        assert not lost, "batch size lost from the %s cycle: %s" % (g.name, lost)
    assert list(hm.GEOMETRIES["small"].classes) == CLASSES
    assert list(hm.GEOMETRIES["large_n"].classes) == LARGE_N
    assert list(hm.GEOMETRIES["bank"].classes) == [c for c in CLASSES if c not in MEMBER_ONLY]
    assert set(hm.ERROR_FAMILIES) == set(POINT_EVENTS) - {"mode_switch"}


def test_the_geometries_are_the_smallest_with_their_structures():
    s, n, b = (hm.GEOMETRIES[k] for k in ("small", "large_n", "bank"))
    assert (s.G, s.U, s.k, s.L, s.T, s.cap) == (1, 6, 9, 74, 2, 300)
    assert hm.pooled(s) == 9 and (s.L - s.k + 1) % hm.dm.C["POOLW"] == 3           # pooling tail 3
    # no chunk override; BatchNorm1's in-launch workgroups at their default count of 8 per tap
    assert hm.chunk_counts(s) == (3, 2) and s.env == {"EXPLAINN_BN1_AUX": str(8 * s.k)}
    assert (n.G, n.U, n.k, n.L, n.T, n.cap) == (1, 3, 19, 1000, 2, 300) and hm.pooled(n) == 140
    forms = hm.dm.forms(n.U, n.k, n.L, n.T, n.cap)
    assert {("qmom", "big"), ("fc_fwd", "fp32"), ("NQ", 140)} <= forms
    assert hm.chunk_counts(n) == (3, 2) and not n.env
    assert (b.G, b.U, b.k, b.L, b.T, b.cap) == (3, 4, 9, 74, 5, 200)
    assert ("bank", "head_bwd_body", "loop") in hm.dm.head_forms(b.U, b.T, b.cap, "step", b.G)
    # 200 sequences give one passA chunk: the override is needed, and only that one
    assert hm.dm.chunks(b.G * b.U, hm.dm.nq_bucket(hm.pooled(b)), b.cap) == (2, 1)
    assert hm.chunk_counts(b) == (2, 2) and b.env == {"EXPLAINN_ACH": "2"}


def test_every_context_function_of_the_header_is_placed():
    fns = hm.context_functions()
    assert len(fns) >= 40 and "explainn_forward_eval" in fns and "explainn_scan_workspace_bytes" in fns
    assert "explainn_adam_step" not in fns and "explainn_activation_null" not in fns      # take no context
    gaps = hm.header_gaps()
    assert not gaps, "declared in include/explainn_hip.h, driven by no op class and not exempt: %s" % ", ".join(gaps)
    stale = [f for f in hm.EXEMPT if f not in fns]
    assert not stale, "exempt but not declared with a context: %s" % ", ".join(stale)
    for f, why in hm.EXEMPT.items():
        assert why.strip(), f
    unknown = sorted(hm.driven() - set(fns))
    assert not unknown, "a class claims to drive what the header does not declare: %s" % ", ".join(unknown)


def test_a_new_entry_point_cannot_stay_outside_the_walk():
    with open(hm.HEADER) as f:
        text = f.read()
    new = "\nint explainn_new_thing(explainn_ctx* ctx, const float* x, int B, void* stream);\n"
    assert hm.header_gaps(text + new) == ["explainn_new_thing"]
    const = "\nint64_t explainn_new_query(const explainn_ctx* ctx,\n    int B);\n"
    assert hm.header_gaps(text + const) == ["explainn_new_query"]
    assert hm.header_gaps(text + "\nint explainn_no_context(const float* x, void* stream);\n") == []
    # a class that leaves takes its entry points with it
    for cls, (fns, _) in hm.OP_CLASSES.items():
        others = hm.driven([c for c in hm.OP_CLASSES if c != cls])
        own = [f for f in fns if f not in others]
        assert hm.header_gaps(classes=[c for c in hm.OP_CLASSES if c != cls]) == [f for f in hm.context_functions()
                                                                                 if f in own]


def test_the_circuit_holds_every_ordered_pair_once():
    for n in (1, 2, 3, 7, 18, 24):
        c = hm.euler_circuit(n)
        pairs = list(zip(c, c[1:]))
        assert len(pairs) == n * n and len(set(pairs)) == n * n and c[0] == c[-1]


@pytest.mark.parametrize("g", GEOMS, ids=IDS)
def test_the_walk_has_every_pair_event_and_shrink(g):
    runs = hm.segments(g)
    lost = hm.audit(g, runs)
    assert not lost, "\n".join(lost)
    # the runs are the walk, overlapping by one item, and none longer than the geometry allows
    items = hm.walk(g)
    assert [it.pos for it in items] == list(range(len(items)))
    assert all(len(r) <= g.segment + 1 for r in runs)
    assert all(a[-1] == b[0] for a, b in zip(runs, runs[1:]))
    assert [it for r in runs for it in r[1:]] == items[1:] and runs[0][0] == items[0]
    # growth: the context must really be exceeded, so no batch of the cycle is above the capacity
    assert max(g.batches) == g.cap
    # train-mode B = 1 (a raise, which is the op) and B = 2 reach every class that takes a batch
    for cls in g.classes:
        if cls not in hm.NO_BATCH:
            assert {1, 2} <= {it.B for it in items if it.cls == cls}, cls


@pytest.mark.parametrize("g", GEOMS, ids=IDS)
def test_the_walk_is_the_same_on_every_run(g):
    assert hm.walk(g) == hm.walk(g)
    a = hm.build_inputs(g, 3, 11)
    b = hm.build_inputs(g, 3, 11)
    flat = lambda d: [(k, v) for k, v in sorted(d.items()) if not isinstance(v, dict)] + \
        [(k + "/" + kk, vv) for k, v in sorted(d.items()) if isinstance(v, dict) for kk, vv in sorted(v.items())]
    for (ka, va), (kb, vb) in zip(flat(a), flat(b)):
        assert ka == kb and va.dtype == vb.dtype and (va == vb).all(), ka


@pytest.mark.parametrize("g", GEOMS, ids=IDS)
def test_losing_a_name_is_noticed_by_name(g):
    """A walk built without one op class, event, cache route or batch size fails the audit against the
    full lists, and the audit names what was lost."""
    classes = list(g.classes)
    for cls in classes:
        rest = [c for c in classes if c != cls]
        lost = hm.audit(g, hm.segments(g, hm.walk(g, classes=rest)))
        assert lost and all(cls in line for line in lost), (cls, lost[:3])
    for ev in hm.POINT_EVENTS:
        lost = hm.audit(g, hm.segments(g, hm.walk(g, point_events=[e for e in hm.POINT_EVENTS if e != ev])))
        assert len(lost) == len(classes) and all(line.endswith("event " + ev) for line in lost), (ev, lost[:3])
    for mod in hm.MODIFIERS:
        lost = hm.audit(g, hm.segments(g, hm.walk(g, modifiers=[m for m in hm.MODIFIERS if m != mod])))
        want = len(classes) + (len(hm.CACHE_ROUTES) if mod == "cache_change" else 0)
        assert len(lost) == want and all(mod in line or "cache route" in line for line in lost), (mod, lost[:3])
    for route in hm.CACHE_ROUTES:
        lost = hm.audit(g, hm.segments(g, hm.walk(g, routes=[r for r in hm.CACHE_ROUTES if r != route])))
        assert lost == ["cache route %s changes no parameters inside a scope" % route]
    for B in sorted(set(g.batches)):
        lost = hm.audit(g, hm.segments(g, hm.walk(g, batches=[b for b in g.batches if b != B])))
        assert lost and any("batch size %d" % B in line for line in lost), (B, lost[:3])


def test_the_audit_sees_a_pair_a_segment_boundary_cuts():
    g = hm.GEOMETRIES["large_n"]
    items = hm.walk(g)
    at = len(g.classes) ** 2 // 2                           # inside the circuit, where every pair occurs once
    cut = [items[:at], items[at:]]                          # no overlap: the pair across the cut is in no run
    a, b = items[at - 1], items[at]
    assert a.mod is None and b.mod is None and a.cls in g.classes and b.cls in g.classes
    assert "pair %s -> %s is in no run" % (a.cls, b.cls) in hm.audit(g, cut)
    assert not hm.audit(g, [items[:at + 1], items[at:]])


def test_the_chunk_arithmetic_is_the_launchers():
    g = hm.GEOMETRIES["small"]
    # a chunk is the call's batch over the chunk count, rounded up to 64 (q) or 128 (passA) sequences:
    # 300 -> 3 x 128 and 2 x 256; 129 -> 3 x 64 and 2 x 128; 128 -> 2 x 64 and 1 x 128; up to 64 one of each
    assert hm.filled(g, 300) == (3, 2) and hm.filled(g, 257) == (3, 2) and hm.filled(g, 129) == (3, 2)
    assert hm.filled(g, 128) == (2, 1) and hm.filled(g, 70) == (2, 1)
    assert hm.filled(g, 64) == (1, 1) and hm.filled(g, 2) == (1, 1)
    assert all(hm.is_big(g, B) for B in (300, 257, 129)) and all(hm.is_small(g, B) for B in (64, 2, 1))
    assert not hm.is_big(g, 128) and not hm.is_small(g, 70)
    # the cycle shrinks only from a batch that filled two chunks of both kinds
    for geo in GEOMS:
        cyc = list(geo.batches)
        for B, nxt in zip(cyc, cyc[1:] + cyc[:1]):
            assert nxt >= B or hm.is_big(geo, B), (geo.name, B, nxt)
