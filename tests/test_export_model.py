"""CPU: the export case lists of tests/export_model.py are fair and reach what they claim, judged on the
fp64 reference alone -- chunk counts, where the cap lands, the overflowing and underflowing units,
the selection pattern -- and hold no float16 knife edge at the delta computed here from the fp32 and
fp64 oracles.  Taking a case out of the list fails test_every_property_is_reached with the name of
what was lost."""
import numpy as np
import pytest

import export_model as em
from oracle import interpret_oracle as io

NAMES = [c["name"] for c in em.CASES]


def _first_capped(counts_u, cap):
    """(selected sequence, chunk) in which the running site count of one unit reaches cap."""
    run = 0
    for s in range(counts_u.shape[0]):
        for ch in range(counts_u.shape[1]):
            run += int(counts_u[s, ch])
            if run >= cap:
                return s, ch
    return None


def _sites_in_chunk(c, ref, ch):
    return ref["counts"][:, :, ch].sum() > 0


def check_lo256(c, ref):
    assert c["L"] - c["k"] + 1 == em.SITE_T and em.chunks(c) == 1
    assert (ref["acts16"][ref["rows"]][:, :, 255] > ref["thresholds"][None, :]).any(), "no site on the last thread"


def check_lo257(c, ref):
    assert c["L"] - c["k"] + 1 == em.SITE_T + 1 and em.chunks(c) == 2
    assert (ref["acts16"][ref["rows"]][:, :, 256] > ref["thresholds"][None, :]).any(), "no site at position 256"


def check_chunks3_ragged(c, ref):
    Lo = c["L"] - c["k"] + 1
    assert Lo == 582 and em.chunks(c) == 3 and Lo % em.SITE_T != 0
    assert _sites_in_chunk(c, ref, 2)


def check_chunks4(c, ref):
    assert c["L"] - c["k"] + 1 == 982 and em.chunks(c) == 4
    assert all(_sites_in_chunk(c, ref, ch) for ch in range(4))


def check_k2(c, ref):
    assert c["k"] == 2 and em.chunks(c) >= 2 and _sites_in_chunk(c, ref, 1)


def check_k32(c, ref):
    assert c["k"] == 32 and em.chunks(c) >= 2 and _sites_in_chunk(c, ref, 1)


def _check_units(c, ref, U):
    assert c["U"] == U and em.chunks(c) >= 2
    assert (ref["nsites"] > 0).all() and _sites_in_chunk(c, ref, 1)


def check_U1(c, ref):
    _check_units(c, ref, 1)


def check_U2(c, ref):
    _check_units(c, ref, 2)


def check_U3(c, ref):
    _check_units(c, ref, 3)


def check_cap_in_later_chunk(c, ref):
    """Some unit reaches the cap strictly inside a chunk >= 2 of a later sequence, after sites of that
    sequence in earlier chunks: there the count carried across chunks decides which sites are kept."""
    assert c["mode"] == "sites" and ref["cap"] < io.SITE_CAP
    found = []
    for u in range(c["U"]):
        cnt = ref["counts"][u]
        at = _first_capped(cnt, ref["cap"])
        if at is None:
            continue
        s, ch = at
        before = cnt[:s].sum() + cnt[s, :ch].sum()
        if s >= 1 and ch >= 1 and cnt[s, :ch].sum() > 0 and before < ref["cap"] < before + cnt[s, ch]:
            found.append(u)
    assert found, "no unit reaches the cap inside a later chunk"
    # dense: about half the positions of the selected sequences are sites
    total = ref["counts"].sum(axis=(1, 2))
    assert (total > 0.25 * len(ref["rows"]) * (c["L"] - c["k"] + 1)).all()


def check_cap_in_batch1(c, ref):
    b = c["batch_sizes"][0]
    S = len(ref["rows"])
    assert len(c["batch_sizes"]) == 1 and -(-S // b) >= 3 and c["sel"] == "all"
    per_seq = ref["counts"].sum(axis=2)
    assert (per_seq[:, :b].sum(axis=1) >= ref["cap"]).all(), "a unit is below the cap after batch 1"
    assert (per_seq[:, b:] > 0).all(), "later batches hold no site that could be added by mistake"
    assert (ref["nsites"] == ref["cap"]).all()
    # and the cap is reached past the first chunk of a sequence that is not the first
    for u in range(c["U"]):
        s, ch = _first_capped(ref["counts"][u], ref["cap"])
        assert s >= 1 and ch >= 1, (u, s, ch)


def check_cap_on_reverse(c, ref):
    assert c["rc"] and c["N"] == 16
    n_fwd = len(ref["rows"]) // 2
    per_seq = ref["counts"].sum(axis=2)
    fwd, total = per_seq[:, :n_fwd].sum(axis=1), per_seq.sum(axis=1)
    assert ((fwd < ref["cap"]) & (ref["cap"] < total)).any(), "no unit reaches the cap on the reverse strand"
    assert (ref["nsites"] == np.minimum(total, ref["cap"])).all()


def check_selection_runs(c, ref):
    _, codes, idxs = em.inputs(c)
    sel = np.zeros(len(codes), dtype=bool)
    sel[idxs] = True
    assert not sel[0] and not sel[-1], "unselected first and last"
    assert (~sel[1:-2] & ~sel[2:-1]).any(), "a run of unselected in the middle"
    all_n = (codes == 4).all(axis=1)
    assert all_n.sum() == 1 and sel[all_n].all(), "one selected sequence of only N"
    frac = (codes[~all_n] == 4).mean()
    assert 0.01 < frac < 0.03, frac
    # the unselected sequences would have added sites
    a16, thr = ref["acts16"], ref["thresholds"]
    assert (a16[~sel] > thr[None, :, None]).any()
    assert not ref["hit"][~sel].any()


def _check_extreme(c, ref, u, value):
    a = ref["acts16"][ref["rows"], u]
    assert (a == value).all(), "unit %d is not %s at every position" % (u, value)
    assert ref["thresholds"][u] == np.float16(value) and ref["nsites"][u] == 0 and not ref["hit"][:, u].any()
    mates = [v for v in range(4 * (u // 4), min(4 * (u // 4) + 4, c["U"])) if v not in c["extremes"]]
    assert mates and all(ref["nsites"][v] > 0 and np.isfinite(ref["thresholds"][v]) for v in mates)


def check_inf_unit(c, ref):
    _check_extreme(c, ref, c["extremes"][0], np.inf)
    # finite in fp32: only the float16 store overflows
    assert ref["acts64"][:, c["extremes"][0]].max() < 1e30


def check_zero_unit(c, ref):
    _check_extreme(c, ref, c["extremes"][1], 0.0)
    assert ref["acts64"][:, c["extremes"][1]].min() > 1e-30


def check_batch1(c, ref):
    assert 1 in c["batch_sizes"]


def check_batch65(c, ref):
    b = em.SCAN_LANES + 1
    assert b in c["batch_sizes"] and c["N"] > b and c["sel"] == "all" and not c["rc"]
    # the one live lane of the second trip has sites, and so has the sequence after the batch: both
    # offsets come from the total carried out of the first trip
    per_seq = ref["counts"].sum(axis=2)
    assert (per_seq[:, em.SCAN_LANES] > 0).all() and (per_seq[:, b:] > 0).any()


def test_every_property_is_reached():
    claimed = {t for c in em.CASES for t in c["tags"]}
    lost = [t for t in em.REQUIRED if t not in claimed]
    assert not lost, "no case reaches: " + "; ".join("%s (%s)" % (t, em.REQUIRED[t]) for t in lost)
    assert claimed <= set(em.REQUIRED)
    assert len(set(NAMES)) == len(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_what_it_claims(name):
    c = em.case(name)
    ref = em.reference(c)
    for tag in c["tags"]:
        globals()["check_" + tag](c, ref)
    # no case is empty, and the reference is the oracle's bookkeeping applied to float16 activations
    assert ref["nsites"].sum() > 0 and ref["acts16"].dtype == np.float16
    assert ref["thresholds"].dtype == np.float16
    assert (ref["pfm"].sum(axis=2) <= ref["nsites"][:, None]).all()
    if c["cap"] is None:
        assert (ref["nsites"] == ref["counts"].sum(axis=(1, 2))).all()


@pytest.mark.parametrize("name", NAMES)
def test_case_has_no_knife_edge(name):
    """delta from the two oracles on this very case; no selected activation within it of a float16
    boundary at the unit's maximum or across its threshold."""
    c = em.case(name)
    ref = em.reference(c)
    d = em.delta(c)
    assert em.DELTA_FLOOR <= d < 2.0 ** -14, d         # far below float16's spacing (2^-11)
    n = em.knife_edges(ref["acts64"][ref["rows"]], ref["thresholds"], d, at_max=c["mode"] == "pwms")
    assert n == 0, "%d knife edges at delta %.2e: pick another seed" % (n, d)


def test_knife_edge_rule_sees_a_planted_edge():
    """An activation one part in 10^7 under the float16 midpoint above the threshold is an edge; the same
    activation well inside the float16 cell is none."""
    thr = np.array([np.float16(1.5)])
    mid = 0.5 * (1.5 + float(np.nextafter(np.float16(1.5), np.float16(2))))
    a = np.array([[[0.7, mid * (1 - 1e-7), 2.9]]])
    assert em.knife_edges(a, thr, 2.0 ** -20, at_max=False) == 1
    a[0, 0, 1] = 1.5
    assert em.knife_edges(a, thr, 2.0 ** -20, at_max=False) == 0
    # at the maximum: 2.9 is clean, a value next to a boundary at the top is not
    top = 0.5 * (3.0 + float(np.nextafter(np.float16(3.0), np.float16(4))))
    a[0, 0, 2] = top * (1 + 1e-7)
    assert em.knife_edges(a, np.array([np.float16(0.1)]), 2.0 ** -20, at_max=True) == 1
