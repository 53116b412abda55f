"""Numpy model of motif spacing (csrc/spacing.hip, explainn_amd/spacing.py).

Sites are three arrays in SiteCalls order: unit (int64), start (int64), strand (+1 / -1).  For an ordered pair
of distinct records i, j:  d = (start_j - start_i) * strand_i,  o = 0 if strand_i == strand_j else 1, and
|d| <= D adds 1 to hist[a][b][o][d + D].  Two independent forms:

  brute(...)      every record against every record (the definition, read off as written);
  per_pair(...)   per (anchor unit, strand) x (partner unit, strand) lists, np.searchsorted for the window.

The test statistics are pure Python with math.lgamma for the binomial tail."""
import math

import numpy as np


def _sets(U, anchors, partners):
    a = np.arange(U) if anchors is None else np.asarray(anchors, dtype=np.int64)
    p = np.arange(U) if partners is None else np.asarray(partners, dtype=np.int64)
    return a, p


def brute(unit, start, strand, U, D, anchors=None, partners=None):
    """hist int64 (A, P, 2, 2D+1): every record i of an anchor unit against every record j != i of a partner
    unit, the whole i x j table (in slabs of rows), no order assumed; counted per (unit, unit) and then
    picked out by the unit sets."""
    unit, start, strand = (np.asarray(x, dtype=np.int64) for x in (unit, start, strand))
    an, pa = _sets(U, anchors, partners)
    full = np.zeros((U, U, 2, 2 * D + 1), dtype=np.int64)
    rows, cols = np.flatnonzero(np.isin(unit, an)), np.flatnonzero(np.isin(unit, pa))
    for r0 in range(0, len(rows), 128):
        i = rows[r0:r0 + 128]
        d = (start[None, cols] - start[i, None]) * strand[i, None]
        near = (np.abs(d) <= D) & (i[:, None] != cols[None, :])
        ri, cj = np.nonzero(near)
        ii, jj = i[ri], cols[cj]
        np.add.at(full, (unit[ii], unit[jj], (strand[ii] != strand[jj]).astype(np.int64), d[ri, cj] + D), 1)
    return full[an][:, pa]


def per_pair(unit, start, strand, U, D, anchors=None, partners=None):
    """The same histogram from sorted per-(unit, strand) lists: for every anchor site the partners inside
    [start - D, start + D] by two binary searches; a pair of a list with itself drops the site itself."""
    unit, start, strand = (np.asarray(x, dtype=np.int64) for x in (unit, start, strand))
    an, pa = _sets(U, anchors, partners)
    lists = {(u, s): np.sort(start[(unit == u) & (strand == s)]) for u in range(U) for s in (1, -1)}
    hist = np.zeros((len(an), len(pa), 2, 2 * D + 1), dtype=np.int64)
    for ai, a in enumerate(an):
        for bi, b in enumerate(pa):
            for sa in (1, -1):
                for sb in (1, -1):
                    xs, ys = lists[(a, sa)], lists[(b, sb)]
                    lo, hi = np.searchsorted(ys, xs - D, "left"), np.searchsorted(ys, xs + D, "right")
                    for x, l, h in zip(xs, lo, hi):
                        d = (ys[l:h] - x) * sa
                        np.add.at(hist[ai, bi, int(sa != sb)], d + D, 1)
                    if a == b and sa == sb:            # every site met itself at d = 0
                        hist[ai, bi, 0, D] -= len(xs)
    return hist


def of_calls(fn, calls, D, **kw):
    """brute / per_pair on a SiteCalls."""
    return fn(calls.unit_ids(), calls.start, calls.strand, calls.units, D, **kw)


def gap(start, period, D):
    """The coordinates that keep records of `period` bases apart: p + (p // period) (D + 1)."""
    start = np.asarray(start, dtype=np.int64)
    return start + (start // period) * (D + 1)


def by_record(fn, unit, start, strand, record, U, D, **kw):
    """The model run record by record and summed (record: the record index of every site)."""
    unit, start, strand, record = (np.asarray(x, dtype=np.int64) for x in (unit, start, strand, record))
    total = None
    for r in np.unique(record):
        m = record == r
        h = fn(unit[m], start[m], strand[m], U, D, **kw)
        total = h if total is None else total + h
    return total


# ------------------------------------------------------------------------------------------- the test
def binom_tail(n, m, c):
    """P[Binomial(n, 1/m) >= c] as the device sums it: the terms from x = c upwards until one no longer
    changes the sum (c >= n/m: they fall from the start)."""
    q = 1.0 / m
    logq, log1mq = math.log(q), math.log1p(-q)
    total = 0.0
    for x in range(c, n + 1):
        t = math.exp(math.lgamma(n + 1.0) - math.lgamma(x + 1.0) - math.lgamma(n - x + 1.0) + x * logq +
                     (n - x) * log1mq)
        if total + t == total:
            break
        total += t
    return total


def admissible(D, min_distance, same, o):
    """The distances d of the admissible bins of an entry, in ascending bin order."""
    if same and o == 0:
        return [d for d in range(max(min_distance, 1), D + 1)]
    return [d for d in range(-D, D + 1) if abs(d) >= min_distance]


def test_stats(hist, anchors, partners, D, min_distance, min_count):
    """(total, best_distance, best_count, pvalue), each (A, P, 2), of a histogram (A, P, 2, 2D+1)."""
    A, P = hist.shape[:2]
    total = np.zeros((A, P, 2), dtype=np.int64)
    best_distance = np.zeros((A, P, 2), dtype=np.int32)
    best_count = np.zeros((A, P, 2), dtype=np.int64)
    pvalue = np.ones((A, P, 2), dtype=np.float64)
    for a in range(A):
        for b in range(P):
            same = int(anchors[a]) == int(partners[b])
            for o in (0, 1):
                ds = admissible(D, min_distance, same, o)
                cs = [int(hist[a, b, o, d + D]) for d in ds]
                if same and o == 1:
                    assert all(c % 2 == 0 for c in cs)
                    cs = [c // 2 for c in cs]
                n, m = sum(cs), len(ds)
                total[a, b, o] = n
                if m == 0 or n < max(min_count, 1):
                    continue
                c = max(cs)
                best_count[a, b, o] = c
                best_distance[a, b, o] = ds[cs.index(c)]          # the first: the lowest bin index
                pvalue[a, b, o] = 1.0 if m == 1 else min(1.0, m * binom_tail(n, m, c))
    return total, best_distance, best_count, pvalue


test_stats.__test__ = False       # a model function, not a test


def benjamini_hochberg(p):
    """q-values of a 1-D array of p-values (stable order for ties)."""
    p = np.asarray(p, dtype=np.float64)
    T = len(p)
    order = np.argsort(p, kind="stable")
    adj = np.minimum(p[order] * T / np.arange(1, T + 1), 1.0)
    adj = np.minimum.accumulate(adj[::-1])[::-1]
    q = np.empty(T)
    q[order] = adj
    return q


def qvalues(total, pvalue, anchors, partners, D, min_distance, min_count):
    """(qvalue, tested): Benjamini-Hochberg over the tested entries in (a, b, o) order, 1 elsewhere."""
    A, P = total.shape[:2]
    tested = np.zeros(total.shape, dtype=bool)
    for a in range(A):
        for b in range(P):
            for o in (0, 1):
                m = len(admissible(D, min_distance, int(anchors[a]) == int(partners[b]), o))
                tested[a, b, o] = m > 0 and total[a, b, o] >= max(min_count, 1)
    q = np.ones(total.shape)
    q[tested] = benjamini_hochberg(pvalue[tested])
    return q, tested


def expected(site_counts, anchors, partners, D, min_distance, n_positions):
    """Pairs that independent placement puts into the admissible bins: m sum_s n_{a,s} n_{b,+-s} / n_positions,
    halved for the same filter on opposite strands (every unordered pair is counted once there)."""
    A, P = len(anchors), len(partners)
    out = np.zeros((A, P, 2))
    n = np.asarray(site_counts, dtype=np.float64)
    for a in range(A):
        for b in range(P):
            ua, ub = int(anchors[a]), int(partners[b])
            for o in (0, 1):
                m = len(admissible(D, min_distance, ua == ub, o))
                pairs = n[ua, 0] * n[ub, o] + n[ua, 1] * n[ub, 1 - o]
                if ua == ub and o == 1:
                    pairs /= 2
                out[a, b, o] = m * pairs / n_positions
    return out


# ------------------------------------------------------------------------------------------- inputs
def random_sites(U, n_sites, span, seed, offset=0):
    """(unit, start, strand) in SiteCalls order: per unit '+' ascending, then '-' ascending; starts are
    distinct inside a (unit, strand) list, as call_sites gives them."""
    g = np.random.default_rng(seed)
    unit, start, strand = [], [], []
    share = g.multinomial(n_sites, g.dirichlet(np.ones(2 * U)))
    for u in range(U):
        for s, n in ((1, share[2 * u]), (-1, share[2 * u + 1])):
            p = np.sort(g.choice(span, size=min(int(n), span), replace=False)).astype(np.int64) + offset
            unit += [u] * len(p)
            start += list(p)
            strand += [s] * len(p)
    return np.array(unit, dtype=np.int64), np.array(start, dtype=np.int64), np.array(strand, dtype=np.int64)


def calls_of(unit, start, strand, U, k=5):
    """A sites.SiteCalls of model arrays that are already in SiteCalls order."""
    from explainn_amd.sites import SiteCalls
    offsets = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(np.asarray(unit, dtype=np.int64), minlength=U), out=offsets[1:])
    return SiteCalls(offsets, start, np.asarray(strand, dtype=np.int8), np.zeros(len(start), np.float32), k)


def in_order(unit, start, strand):
    """Any (unit, start, strand) records sorted into SiteCalls order (stable)."""
    unit, start, strand = (np.asarray(x, dtype=np.int64) for x in (unit, start, strand))
    order = np.lexsort((start, strand < 0, unit))
    return unit[order], start[order], strand[order]
