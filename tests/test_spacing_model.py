"""CPU: the numpy model of motif spacing (tests/spacing_model.py) against itself -- two independent forms,
the symmetries, the same-filter folds, the record gap rule -- its binomial tail against scipy, and the
argument checks of explainn_amd.spacing that need no device.

BINOM_TAIL_DEVIATION is the yardstick of tests/test_gpu_spacing.py: the largest relative deviation of the
model's tail (math.lgamma terms summed from c upwards) from scipy.stats.binom.sf over the grid below,
measured as 1.78e-10 (at n = 10^5, where lgamma(n+1) ~ 10^6 carries an absolute error of ~1e-10 into the
exponent); the constant is that figure and test_tail_matches_scipy holds the model to it."""
import math
import os
import re

import numpy as np
import pytest

import spacing_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINOM_TAIL_DEVIATION = 1.78e-10


def _random(U=4, n=150, span=400, seed=0):
    return sm.random_sites(U, n, span, seed)


@pytest.mark.parametrize("D", [0, 1, 7, 30])
def test_two_forms_agree(D):
    for seed in range(3):
        unit, start, strand = _random(seed=seed)
        a, b = sm.brute(unit, start, strand, 4, D), sm.per_pair(unit, start, strand, 4, D)
        assert np.array_equal(a, b)
        assert a.sum() > 0 or D == 0
    unit, start, strand = _random(U=5, seed=9)
    kw = dict(anchors=[4, 1], partners=[0, 1, 3])
    assert np.array_equal(sm.brute(unit, start, strand, 5, D, **kw), sm.per_pair(unit, start, strand, 5, D, **kw))
    assert np.array_equal(sm.brute(unit, start, strand, 5, D, **kw),
                          sm.brute(unit, start, strand, 5, D)[[4, 1]][:, [0, 1, 3]])


def test_symmetries():
    D = 12
    unit, start, strand = _random(seed=3)
    h = sm.brute(unit, start, strand, 4, D)
    assert np.array_equal(h[:, :, 0, :], h.transpose(1, 0, 2, 3)[:, :, 0, ::-1])
    assert np.array_equal(h[:, :, 1, :], h.transpose(1, 0, 2, 3)[:, :, 1, :])


def test_same_filter_folds():
    D = 15
    unit, start, strand = _random(seed=4)
    h = sm.brute(unit, start, strand, 4, D)
    for u in range(4):
        assert np.all(h[u, u, 1] % 2 == 0)
        plus, minus = start[(unit == u) & (strand > 0)], start[(unit == u) & (strand < 0)]
        # unordered pairs on one strand within D (starts are distinct inside a list: none at d = 0)
        same = sum(int(np.sum((np.abs(p[:, None] - p[None, :]) <= D) & (p[:, None] < p[None, :]))) for p in (plus, minus))
        assert h[u, u, 0, D] == 0 and h[u, u, 0, D + 1:].sum() == same == h[u, u, 0, :D].sum()
        opposite = int(np.sum(np.abs(plus[:, None] - minus[None, :]) <= D))
        assert h[u, u, 1].sum() == 2 * opposite
    total, _, _, _ = sm.test_stats(h, np.arange(4), np.arange(4), D, 0, 0)
    for u in range(4):
        assert total[u, u, 0] == h[u, u, 0, D + 1:].sum() and total[u, u, 1] == h[u, u, 1].sum() // 2


def test_same_position_counts():
    """Two filters on one position count at d = 0; one filter on both strands of one position counts in
    orientation 1 at d = 0, once per ordered pair; a record never meets itself."""
    unit, start, strand = sm.in_order([0, 1, 0], [10, 10, 10], [1, 1, -1])
    h = sm.brute(unit, start, strand, 2, 3)
    assert h[0, 1, 0, 3] == 1 and h[1, 0, 0, 3] == 1 and h[0, 1, 1, 3] == 1 and h[1, 0, 1, 3] == 1
    assert h[0, 0, 1, 3] == 2 and h[0, 0, 0].sum() == 0 and h[1, 1].sum() == 0
    assert np.array_equal(h, sm.per_pair(unit, start, strand, 2, 3))


def test_minus_anchor_flips_the_distance():
    unit, start, strand = sm.in_order([0, 1], [20, 23], [-1, -1])
    h = sm.brute(unit, start, strand, 2, 5)
    assert h[0, 1, 0, 5 - 3] == 1 and h[1, 0, 0, 5 + 3] == 1 and h.sum() == 2


@pytest.mark.parametrize("D", [3, 20])
def test_gap_rule_equals_per_record_sum(D):
    L = 50
    unit, start, strand = _random(U=3, n=200, span=8 * L, seed=5)
    start = np.concatenate([start, [L - 1, L, 2 * L - 1, 2 * L]])        # sites on both sides of two boundaries
    unit, strand = np.concatenate([unit, [0, 1, 2, 0]]), np.concatenate([strand, [1, 1, -1, -1]])
    unit, start, strand = sm.in_order(unit, start, strand)
    want = sm.by_record(sm.brute, unit, start, strand, start // L, 3, D)
    assert np.array_equal(sm.brute(unit, sm.gap(start, L, D), strand, 3, D), want)
    assert not np.array_equal(sm.brute(unit, start, strand, 3, D), want)     # the boundary pairs are real


def test_tail_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    worst = 0.0
    for n in (1, 10, 1000, 10 ** 5):
        for m in (2, 21, 201):
            lo = -(-n // m)
            sd = math.sqrt(n * (1.0 / m) * (1 - 1.0 / m))
            for c in sorted({min(n, max(lo, 1) + int(round(z * sd)) + j) for z in (0, 1, 3, 6, 10, 20) for j in (0, 1)}):
                ref = float(stats.binom.sf(c - 1, n, 1.0 / m))
                if ref <= 1e-300:
                    continue
                got = sm.binom_tail(n, m, c)
                worst = max(worst, abs(got - ref) / ref)
    print("largest relative deviation of the tail from scipy: %.3g" % worst)
    assert worst <= BINOM_TAIL_DEVIATION


def test_statistics_conventions():
    D = 4
    hist = np.zeros((2, 2, 2, 2 * D + 1), dtype=np.int64)
    hist[0, 1, 0, D - 3] = hist[0, 1, 0, D + 2] = 9                      # a tie: the lower bin index wins
    hist[0, 1, 0, D] = 50                                                # d = 0 < min_distance: not admissible
    hist[0, 0, 0, D + 2] = hist[0, 0, 0, D - 2] = 12
    hist[0, 0, 1, D - 4] = 30
    hist[1, 0, 1, D + 1] = 3
    total, best_d, best_c, p = sm.test_stats(hist, [0, 1], [0, 1], D, 1, 5)
    assert (total[0, 1, 0], best_d[0, 1, 0], best_c[0, 1, 0]) == (18, -3, 9)
    assert (total[0, 0, 0], best_d[0, 0, 0], best_c[0, 0, 0]) == (12, 2, 12)
    assert (total[0, 0, 1], best_d[0, 0, 1], best_c[0, 0, 1]) == (15, -4, 15)
    assert (total[1, 0, 1], best_d[1, 0, 1], best_c[1, 0, 1], p[1, 0, 1]) == (3, 0, 0, 1.0)       # n < min_count
    assert p[0, 0, 0] == pytest.approx(4 * 0.25 ** 12) and p[0, 0, 1] == pytest.approx(8 * 0.125 ** 15)
    total, best_d, best_c, p = sm.test_stats(hist, [0, 1], [0, 1], D, D + 1, 0)                   # m = 0
    assert not total.any() and not best_c.any() and np.all(p == 1.0)
    total, _, best_c, p = sm.test_stats(hist, [0, 1], [0, 1], D, D, 0)                            # m = 1 where a == b, o = 0
    assert p[0, 0, 0] == 1.0 and best_c[0, 0, 0] == 0 and total[0, 0, 0] == 0
    q, tested = sm.qvalues(*sm.test_stats(hist, [0, 1], [0, 1], D, 1, 5)[::3], [0, 1], [0, 1], D, 1, 5)
    assert tested.sum() == 3 and np.all(q[~tested] == 1.0)


# ---------------------------------------------------------------- explainn_amd.spacing without a device
def _calls(seed=0, U=3):
    return sm.calls_of(*sm.random_sites(U, 60, 300, seed), U)


def test_site_lists_offsets_and_gap():
    from explainn_amd import spacing as sp
    calls = _calls()
    start, off2, k = sp.site_lists(calls, 10)
    assert k == 5 and np.array_equal(start, calls.start) and off2[-1] == len(calls)
    for u in range(3):
        _, strand, _ = calls.unit(u)
        assert off2[2 * u + 1] - off2[2 * u] == np.sum(strand > 0) and off2[2 * u] == calls.offsets[u]
    start, _, _ = sp.site_lists(calls, 10, period=50)
    assert np.array_equal(start, sm.gap(calls.start, 50, 10))
    # a list of records of unequal lengths: the model record by record
    recs = [(_calls(1), 300), (_calls(2), 340), (_calls(3), 301)]
    start, off2, _ = sp.site_lists(recs, 10)
    unit = np.repeat(np.arange(6) // 2, np.diff(off2))
    strand = np.repeat(np.where(np.arange(6) % 2 == 0, 1, -1), np.diff(off2))
    want = sum(sm.of_calls(sm.brute, c, 10) for c, _ in recs)
    assert np.array_equal(sm.brute(unit, start, strand, 3, 10), want)
    assert start.max() == max(recs[2][0].start) + 300 + 340 + 2 * 11


def test_argument_checks_need_no_device():
    import torch
    from explainn_amd import _lib, spacing as sp
    from explainn_amd.sites import SiteCalls
    calls = _calls()
    for bad in (-1, sp.MAX_DISTANCE + 1, 2.5):
        with pytest.raises(ValueError, match="max_distance"):
            sp.spacing(calls, bad)
    lo, hi = calls.offsets[0], calls.offsets[1]
    start = calls.start.copy()
    start[lo:hi] = start[lo:hi][::-1]                                    # unit 0: '+' and '-' runs reversed
    with pytest.raises(ValueError, match="ascending"):
        sp.spacing(SiteCalls(calls.offsets, start, calls.strand, calls.score, 5), 10)
    with pytest.raises(ValueError, match=r"'\+' sites must come before"):
        sp.spacing(SiteCalls(calls.offsets, calls.start, -calls.strand, calls.score, 5), 10)
    with pytest.raises(ValueError, match="anchors=.*partners=.*smaller max_distance"):
        sp.spacing(calls, 100, max_bytes=3 * 3 * 2 * 201 * 8 - 1)
    big = sm.calls_of([], [], [], 6000)
    with pytest.raises(ValueError, match="more than max_bytes"):
        sp.spacing(big, 100)                                             # 6000^2 x 2 x 201 x 8 bytes > 2 GiB
    with pytest.raises(IndexError):
        sp.spacing(calls, 10, anchors=[3])
    held = sp.SpacingCounts(torch.zeros(3, 3, 2, 21, dtype=torch.int64), None, None, 10, 5, np.zeros((3, 2)))
    with pytest.raises(ValueError, match="out="):
        sp.spacing(calls, 11, out=held)
    with pytest.raises(ValueError, match="out="):
        sp.spacing(calls, 10, anchors=[0, 1], out=held)
    with pytest.raises(ValueError, match="out="):
        sp.spacing(sm.calls_of(*sm.random_sites(3, 60, 300, 0), 3, k=7), 10, out=held)
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert int(re.search(r"#define EXPLAINN_SPACING_MAX_DISTANCE (\d+)", text).group(1)) == \
        _lib.SPACING_MAX_DISTANCE == sp.MAX_DISTANCE == 1024


def test_planted_spacing_stands_out_in_the_model():
    """The planted case of the GPU test, on the model: the margin by which (0, 1, same) at +7 wins."""
    unit, start, strand, rec, U, L = planted()
    D = 20
    hist = sm.brute(unit, sm.gap(start + rec * L, L, D), strand, U, D)
    total, best_d, best_c, p = sm.test_stats(hist, np.arange(U), np.arange(U), D, 5, 10)
    q, tested = sm.qvalues(total, p, np.arange(U), np.arange(U), D, 5, 10)
    assert best_d[0, 1, 0] == 7 and best_d[1, 0, 0] == -7 and best_c[0, 1, 0] >= 200
    others = np.ones(p.shape, dtype=bool)
    others[0, 1, 0] = others[1, 0, 0] = False
    assert p[0, 1, 0] < 1e-100 and p[others].min() > 1e-6
    assert q[0, 1, 0] == q.min() and q[others].min() > 1e-4


def planted(records=400, L=200, U=4, seed=7):
    """400 records of 200 positions: unit 0 once per record; unit 1 follows it at +7 on the same strand in
    60 % of the records and sits anywhere otherwise; units 2, 3 uniform.  Returns SiteCalls-ordered
    (unit, start within the record, strand, record) and U, L."""
    g = np.random.default_rng(seed)
    rows = []
    for r in range(records):
        s0, p0 = g.choice([1, -1]), int(g.integers(30, L - 30))
        rows.append((0, p0, s0, r))
        if g.random() < 0.6:
            rows.append((1, p0 + 7 * s0, s0, r))
        else:
            rows.append((1, int(g.integers(0, L)), g.choice([1, -1]), r))
        for u in (2, 3):
            rows.append((u, int(g.integers(0, L)), g.choice([1, -1]), r))
    unit, start, strand, rec = (np.array(c, dtype=np.int64) for c in zip(*rows))
    order = np.lexsort((start + rec * L, strand < 0, unit))
    return unit[order], start[order], strand[order], rec[order], U, L
