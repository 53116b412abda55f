"""CPU: the numpy model of the activation null (tests/actnull_model.py) against brute force on small
float16 arrays -- sort, count `> t` for every candidate t, take the minimal t -- and the Python surface
that needs no device (SiteCalls.pvalue, bed_rows, the binding constants)."""
import numpy as np
import pytest

import actnull_model as am


def _candidates():
    """Every non-negative float16 value including +inf, ascending."""
    return np.arange(am.INF + 1, dtype=np.uint16).view(np.float16)


def _brute_threshold(row, alpha):
    """The smallest float16 t >= 0 with #(row > t) <= floor(alpha * n); +inf for an empty row."""
    row = np.sort(np.asarray(row, dtype=np.float16))
    if len(row) == 0:
        return np.float32(np.inf)
    m = int(np.floor(np.float64(alpha) * np.float64(len(row))))
    cand = _candidates()
    # values > t for every candidate t: what is right of t's last occurrence in the sorted row
    above = len(row) - np.searchsorted(row.astype(np.float64), cand.astype(np.float64), side="right")
    assert above[-1] == 0 and int((row > cand[1000]).sum()) == above[1000]
    return np.float32(cand[np.flatnonzero(above <= m)[0]])


def _rows(seed):
    g = np.random.default_rng(seed)
    rows = [
        np.exp(g.normal(0, 2, size=200)).astype(np.float16),                     # spread
        g.choice(np.array([0.25, 0.5, 0.5, 1.0, 3.0], np.float16), size=150),     # heavy ties
        np.concatenate([np.zeros(40, np.float16), np.full(7, np.inf, np.float16),
                        np.exp(g.normal(0, 1, size=60)).astype(np.float16)]),     # 0 and +inf present
        np.zeros(0, np.float16),                                                  # an empty row
        np.full(30, 2.5, np.float16),                                             # one value only
        np.array([6.1e-5, 5.96e-8, 0.0, 65504.0], np.float16),                    # subnormals and the largest finite
    ]
    return rows


def _hist(rows):
    return np.stack([np.bincount(am.bins(r), minlength=am.BINS) for r in rows]).astype(np.int64)


def test_bins_sort_like_values():
    v = _candidates()
    assert np.all(np.diff(v.astype(np.float64)[:-1]) > 0) and np.isinf(v[-1])
    assert np.array_equal(am.bins(v), np.arange(am.INF + 1))
    assert np.isnan(am.bin_values()[am.INF + 1:]).all()
    assert am.bins(np.array([-0.0], np.float16))[0] == 0


@pytest.mark.parametrize("seed", [0, 1])
def test_tail_total_against_brute_force(seed):
    rows = _rows(seed)
    h = _hist(rows)
    assert np.array_equal(am.histogram(np.stack([rows[0], rows[0]])), np.stack([h[0], h[0]]))
    assert np.array_equal(am.total(h), [len(r) for r in rows])
    t = am.tail(h)
    g = np.random.default_rng(seed + 10)
    for u, r in enumerate(rows):
        for b in np.concatenate([[0, 1, am.INF, am.INF + 1, am.BINS - 1], g.integers(0, am.INF, size=40),
                                 am.bins(r)[:20]]):
            want = int((am.bins(r) >= b).sum())
            assert t[u, b] == want, (u, b)


@pytest.mark.parametrize("alpha", [0.0, 1e-3, 0.01, 0.05, 0.3, 0.5, 1.0])
@pytest.mark.parametrize("seed", [0, 1])
def test_threshold_rule_against_brute_force(alpha, seed):
    rows = _rows(seed)
    h = _hist(rows)
    thr = am.thresholds(h, alpha)
    assert thr.dtype == np.float32
    for u, r in enumerate(rows):
        assert thr[u] == _brute_threshold(r, alpha), (u, alpha)
    # what the rule promises: at most m above the threshold, more than m one float16 step lower
    m = am.allowed(h, alpha)
    above = am.count_above(h, thr)
    assert np.all(above <= m)
    tb = am.threshold_bins(h, alpha)
    for u, r in enumerate(rows):
        if len(r) and tb[u] > 0:
            lower = am.bin_values()[tb[u] - 1]
            assert int((r > np.float16(lower)).sum()) > m[u], (u, alpha)


def test_threshold_special_cases():
    rows = _rows(0)
    h = _hist(rows)
    t0, t1 = am.thresholds(h, 0.0), am.thresholds(h, 1.0)
    for u, r in enumerate(rows):
        if len(r):
            assert t0[u] == np.float32(r.max())          # alpha 0: the largest observed value
            assert t1[u] == 0.0                          # alpha 1: everything may be called
        else:
            assert np.isinf(t0[u]) and np.isinf(t1[u])   # no null: never a site
    assert np.isinf(t0[2])                               # +inf present and none may exceed the threshold


def test_pvalue_against_brute_force():
    rows = _rows(1)
    h = _hist(rows)
    g = np.random.default_rng(5)
    for u, r in enumerate(rows):
        scores = np.concatenate([r[:10].astype(np.float32), np.exp(g.normal(0, 2, size=10)).astype(np.float32),
                                 np.array([0.0, np.inf, 1e-9, 6e4], np.float32)])
        s16 = scores.astype(np.float16)
        want = np.array([(1.0 + (r >= s).sum()) / (1.0 + len(r)) for s in s16], dtype=np.float64)
        got = am.pvalue(h, np.full(len(scores), u), scores)
        assert got.dtype == np.float64 and np.array_equal(got, want), u
    assert am.pvalue(h, [3], [1.0])[0] == 1.0            # the empty row


def test_site_calls_pvalue_and_bed_rows():
    """SiteCalls carries an optional pvalue; bed_rows appends a seventh column only then."""
    from explainn_amd import sites
    offsets, start, strand, score = [0, 2, 3], [5, 9, 1], [1, -1, 1], [0.5, 2.0, 1.25]
    plain = sites.SiteCalls(offsets, start, strand, score, 4)
    assert plain.pvalue is None
    rows = sites.bed_rows("chr", plain)
    assert rows == ["chr\t1\t5\tfilter1\t1.25\t+\n", "chr\t5\t9\tfilter0\t0.5\t+\n", "chr\t9\t13\tfilter0\t2\t-\n"]
    withp = sites.SiteCalls(offsets, start, strand, score, 4, pvalue=[0.5, 1e-4, 0.25])
    assert withp.pvalue.dtype == np.float64
    rows7 = sites.bed_rows("chr", withp)
    assert [r.rstrip("\n").rsplit("\t", 1)[0] + "\n" for r in rows7] == rows
    assert [r.rstrip("\n").split("\t")[6] for r in rows7] == ["0.25", "0.5", "0.0001"]
    with pytest.raises(ValueError):
        sites.SiteCalls(offsets, start, strand, score, 4, pvalue=[0.5])


def test_binding_constants_match_the_header():
    import os
    import re
    from explainn_amd import _lib, sites
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "explainn_hip.h")).read()
    assert int(re.search(r"#define EXPLAINN_ACT_BINS (\d+)", text).group(1)) == _lib.ACT_BINS == sites.ACT_BINS == am.BINS
    assert int(re.search(r"#define EXPLAINN_ACT_SPAN (\d+)", text).group(1)) == _lib.ACT_SPAN
    for name, nargs in (("explainn_activation_histogram", 10), ("explainn_activation_null", 7)):
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == nargs
