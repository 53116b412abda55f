"""fp64 numpy / math.lgamma model of motif centrality (csrc/central.hip, explainn_amd/centrality.py; DESIGN.md
section 3 item 19 and section 8, "Centrality"), written from the definitions of include/explainn_hip.h.

Histograms: from the best sites of every (unit, record) -- bit pattern and (start << 1) | is_minus -- the labels
and the thresholds, hist[u][t][set][start] and the record counts.  The test: the admissible regions of both
modes, the binomial tail summed as the device sums it, the enriched-only rule, the tie rule, log_padj's two
branches (enrichment_model.log_padj: the same function) and the Fisher step
(enrichment_model.hypergeom_logsf).

LOGSF_DEVIATION: the largest absolute deviation of `binom_logsf` from scipy.stats.binom.logsf, in ln p, over
the grid of tests/test_centrality_model.py (q = w / M from 1 / M to (M - 1) / M for M = 2, 64 and 182), by the
grid's n (measured: 3.38e-14 at n = 40, 5.18e-13 at 400, 8.90e-12 at 4000, 1.04e-10 at 40000, 2.89e-9 at 10^6,
with at most 26, 82, 257, 807 and 3905 terms -- the growth is the cancellation of lgammas of size n ln n); the
constants are those figures rounded up to two digits and test_logsf_matches_scipy holds the model to them.
tests/test_gpu_centrality.py allows the device ten times the figure of its n, and at least 64 ulp of
lgamma(n + 1): the rule of enrichment_model.log_tolerance."""
import math

import numpy as np

import enrichment_model as em

LOGSF_DEVIATION = {40: 3.4e-14, 400: 5.2e-13, 4000: 9.0e-12, 40000: 1.1e-10, 10 ** 6: 2.9e-9}
# between the best ln p of a unit and the best one of a differing (n, c, w), wherever the GPU test demands the
# chosen (threshold, region) exactly: more than thirty times the largest tolerance of any case
# (log_tolerance(10^6) = 2.9e-8), and the value of enrichment_model.MIN_GAP
MIN_GAP = 1e-6
FIELDS = ("best_t", "best_lo", "best_width", "sites", "count", "n_tests", "log_pvalue", "log_padj", "ctrl_sites",
          "ctrl_count", "log_fisher")
LOG_FIELDS = ("log_pvalue", "log_padj", "log_fisher")


def deviation(n):
    """The recorded deviation of the smallest grid n that is at least n."""
    return LOGSF_DEVIATION[min(g for g in LOGSF_DEVIATION if g >= n)]


def log_tolerance(n):
    """What the device's log values may differ by from the model's at n sites (or records, for log_fisher):
    ten times the model's own deviation from scipy at that n, and at least 64 ulp of lgamma(n + 1)."""
    return max(10.0 * deviation(n), 64.0 * float(np.spacing(math.lgamma(n + 1.0))))


# ------------------------------------------------------------------------------------------- histograms
def passes(bits, thresholds):
    """bool (U, N, T): the float16 value of the pattern (& 0x7FFF), as a float, > the float32 threshold --
    the comparison of explainn_call_sites."""
    a = (np.ascontiguousarray(bits).view(np.uint16) & 0x7FFF).astype(np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return a[:, :, None] > np.asarray(thresholds, dtype=np.float32)[:, None, :]


def positions(bits, site, labels, thresholds, M):
    """(hist int32 (U, T, 2, M), counts int64 (2,)): hist[u][t][set][start] = included records whose best site
    of unit u passes threshold t and starts at `start`; a site below 0 or a start >= M counts nowhere."""
    site = np.asarray(site, dtype=np.int64)
    labels = np.asarray(labels)
    thresholds = np.asarray(thresholds, dtype=np.float32)
    U, T = thresholds.shape
    ok = passes(bits, thresholds)
    hist = np.zeros((U, T, 2, M), dtype=np.int64)
    start = site >> 1
    for s, lab in ((0, 1), (1, 0)):
        inc = (labels == lab)[None, :] & (site >= 0) & (start < M)
        for u in range(U):
            for t in range(T):
                sel = inc[u] & ok[u, :, t]
                hist[u, t, s] = np.bincount(start[u, sel], minlength=M)
    return hist.astype(np.int32), np.array([np.sum(labels == 1), np.sum(labels == 0)], dtype=np.int64)


def positions_brute(bits, site, labels, thresholds, M):
    """The same, record by record."""
    thresholds = np.asarray(thresholds, dtype=np.float32)
    U, T = thresholds.shape
    hist = np.zeros((U, T, 2, M), dtype=np.int32)
    pat = np.ascontiguousarray(bits).view(np.uint16) & 0x7FFF
    for u in range(U):
        for r, lab in enumerate(labels):
            if lab > 1 or site[u, r] < 0 or (int(site[u, r]) >> 1) >= M:
                continue
            a = np.float32(np.array(pat[u, r], np.uint16).view(np.float16))
            for t in range(T):
                if a > thresholds[u, t]:
                    hist[u, t, 0 if lab == 1 else 1, int(site[u, r]) >> 1] += 1
    return hist


# ------------------------------------------------------------------------------------------- the test
def regions(M, local=False, min_width=1, max_width=None):
    """[(lo, width), ...]: centred, the regions [j, M-1-j]; local, every lo <= hi; min_width <= width <=
    max_width and width < M."""
    hi = M - 1 if max_width is None else min(int(max_width), M - 1)
    if local:
        return [(lo, w) for w in range(max(int(min_width), 1), hi + 1) for lo in range(0, M - w + 1)]
    return [(j, M - 2 * j) for j in range(1, M) if max(int(min_width), 1) <= M - 2 * j <= hi]


def binom_logsf(n, c, w, M, return_terms=False):
    """ln P[X >= c], X ~ Binomial(n, w / M), as the device sums it: ln of the first term from three lgammas,
    plus ln of (1 + the following terms relative to it), each its predecessor times ((n-x) / (x+1)) * (q / (1-q)),
    until x reaches n or a term no longer changes the sum."""
    lg = math.lgamma
    q = float(w) / float(M)
    first = lg(n + 1.0) - lg(c + 1.0) - lg(n - c + 1.0) + c * math.log(q) + (n - c) * math.log1p(-q)
    odds = q / (1.0 - q)
    total, term, terms = 1.0, 1.0, 1
    for x in range(c, n):
        term *= (float(n - x) / float(x + 1)) * odds
        s = total + term
        if s == total:
            break
        total = s
        terms += 1
    out = min(0.0, first + math.log(total))
    return (out, terms) if return_terms else out


def logp(n, c, w, M, cache=None):
    """0 unless the region is enriched (c M > n w, in integers)."""
    if not c * M > n * w:
        return 0.0
    if cache is None:
        return binom_logsf(n, c, w, M)
    key = (n, c, w)
    if key not in cache:
        cache[key] = binom_logsf(n, c, w, M)
    return cache[key]


def log_fisher(count, ctrl_count, Np, Nc):
    """0 unless the primary share exceeds the control's (count Nc > ctrl_count Np) and there is a control."""
    if Nc <= 0 or count > Np or ctrl_count > Nc or not count * Nc > ctrl_count * Np:
        return 0.0
    return em.hypergeom_logsf(count, count + ctrl_count, Np, Nc)


def unit_stats(h, counts, local=False, min_width=1, max_width=None, min_sites=1):
    """One unit's outputs from its (T, 2, M) histogram, and `gap`: the distance from the best ln p to the
    smallest one of a differing (n, c, w) (inf without one, or when the best is the assigned 0: equal counts
    give equal bits on the device, so only differing counts can change places)."""
    h = np.asarray(h, dtype=np.int64)
    T, _, M = h.shape
    regs = regions(M, local, min_width, max_width)
    pre = np.concatenate([np.zeros((T, 1), np.int64), np.cumsum(h[:, 0], axis=1)], axis=1)
    need = max(int(min_sites), 1)
    tried = [t for t in range(T) if pre[t, M] >= need]
    out = dict(zip(FIELDS, (0, 0, 0, 0, 0, 0, 0.0, 0.0, 0, 0, 0.0)))
    out["gap"] = float("inf")
    if not tried or not regs:
        return out
    cache, best, items = {}, None, []
    for t in tried:
        n = int(pre[t, M])
        for lo, w in regs:
            c = int(pre[t, lo + w] - pre[t, lo])
            lp = logp(n, c, w, M, cache)
            items.append((lp, n, c, w))
            key = (lp, w, lo, t)
            if best is None or key < best:
                best = key
    lp, w, lo, t = best
    n, c = int(pre[t, M]), int(pre[t, lo + w] - pre[t, lo])
    if lp < 0.0:
        others = [x[0] for x in items if x[1:] != (n, c, w)]
        out["gap"] = min(others) - lp if others else float("inf")
    m = len(tried) * len(regs)
    cs, cc = int(h[t, 1].sum()), int(h[t, 1, lo:lo + w].sum())
    out.update(best_t=t, best_lo=lo, best_width=w, sites=n, count=c, n_tests=m, log_pvalue=lp,
               log_padj=em.log_padj(lp, m), ctrl_sites=cs, ctrl_count=cc,
               log_fisher=log_fisher(c, cc, int(counts[0]), int(counts[1])))
    return out


def test_stats(hist, counts, **kwargs):
    """Every unit's unit_stats, stacked: a dict of arrays over the units."""
    per = [unit_stats(h, counts, **kwargs) for h in np.asarray(hist)]
    return {f: np.array([p[f] for p in per]) for f in FIELDS + ("gap",)}


test_stats.__test__ = False       # a model function, not a test


def brute_count(starts, lo, w):
    """Sites with lo <= start < lo + w, read off the raw list."""
    starts = np.asarray(starts)
    return int(np.sum((starts >= lo) & (starts < lo + w)))


# ------------------------------------------------------------------------------------------- inputs
def best_case(units, n_records, T, M, seed, labels_upto=2):
    """Random best sites for the histogram tests: (bits uint16, site int32 (units, N), labels uint8 (N,),
    thresholds float32 (units, T)).  Scores in [0.25, 4), a few NaN patterns and a few with bit 15 set;
    thresholds inside that range, one of them met exactly by some scores (`>` is strict); one record in 16
    has no site (-1), one in 16 a forged start (>= M, up to the largest the site word holds); labels 0 ..
    labels_upto (above 1: left out)."""
    g = np.random.default_rng(seed)
    N = int(n_records)
    bits = g.integers(0x3400, 0x4400, size=(units, N)).astype(np.uint16)
    bits[g.random((units, N)) < 0.02] = 0x7E00
    bits[g.random((units, N)) < 0.1] |= 0x8000
    site = ((g.integers(0, M, size=(units, N)) << 1) | g.integers(0, 2, size=(units, N))).astype(np.int32)
    kind = g.integers(0, 16, size=(units, N))
    site[kind == 0] = -1
    forged = g.integers(M, max(M + 40, 2 * M), size=(units, N))
    forged[g.random((units, N)) < 0.3] = (1 << 30) - 1
    site = np.where(kind == 1, ((forged << 1) | 1).astype(np.int32), site)
    labels = g.integers(0, labels_upto + 1, size=N).astype(np.uint8)
    thr = g.integers(0x3400, 0x4400, size=(units, T)).astype(np.uint16).view(np.float16).astype(np.float32)
    if N and bits[0, 0] & 0x7FFF < 0x7C00:
        thr[0, 0] = np.float32(np.array(bits[0, 0] & 0x7FFF, np.uint16).view(np.float16))
    return bits, site, labels, np.sort(thr, axis=1)


def level_case(units, T, M, n_primary, n_control, seed, central=0.0, sd=3.0, keep=0.7):
    """A (hist, counts) of synthetic records: every record of every unit has one start -- with probability
    `central` drawn from a normal of `sd` bins around the middle start, else uniform -- and passes the first
    `level` thresholds, level falling off geometrically (`keep`); control records are uniform."""
    g = np.random.default_rng(seed)
    hist = np.zeros((units, T, 2, M), dtype=np.int32)
    for u in range(units):
        for s, n, frac in ((0, n_primary, central), (1, n_control, 0.0)):
            start = g.integers(0, M, size=n)
            mid = np.clip(np.rint((M - 1) / 2.0 + sd * g.standard_normal(n)), 0, M - 1).astype(np.int64)
            start = np.where(g.random(n) < frac, mid, start)
            level = np.minimum(g.geometric(1.0 - keep, size=n), T + 1) - 1          # 0 .. T
            for t in range(T):
                hist[u, t, s] = np.bincount(start[level > t], minlength=M)
    return hist, np.array([n_primary, n_control], dtype=np.int64)


def test_cases():
    """name -> (hist, counts, kwargs of the test): the inputs tests/test_gpu_centrality.py feeds straight to
    explainn_centrality_test and demands the chosen (threshold, region) on exactly."""
    cases = {}
    cases["M1"] = level_case(2, 2, 1, 30, 20, 1) + ({},)
    cases["M2_centred"] = level_case(2, 2, 2, 30, 20, 2) + ({},)
    cases["M2_local"] = level_case(3, 2, 2, 30, 20, 3) + ({"local": True},)
    cases["odd_centred"] = level_case(4, 3, 65, 300, 200, 4, central=0.3) + ({},)
    cases["even_centred"] = level_case(4, 3, 64, 300, 200, 5, central=0.3) + ({},)
    cases["odd_local"] = level_case(3, 2, 63, 200, 100, 6, central=0.3) + ({"local": True},)
    cases["even_local"] = level_case(3, 2, 64, 200, 100, 7, central=0.3) + ({"local": True},)
    cases["centred_widths"] = level_case(4, 3, 65, 300, 200, 8, central=0.3, sd=8.0) + ({"min_width": 5, "max_width": 31},)
    cases["local_widths"] = level_case(3, 2, 64, 200, 100, 9, central=0.3) + ({"local": True, "min_width": 3, "max_width": 10},)
    cases["wide_max"] = level_case(2, 2, 33, 100, 50, 10, central=0.2) + ({"max_width": 1000},)
    cases["min_sites"] = level_case(4, 4, 33, 120, 50, 11, central=0.4, keep=0.4) + ({"min_sites": 40},)
    hist, counts = level_case(3, 3, 33, 150, 80, 12, central=0.4)
    hist[:, 1] = 0                                                              # a threshold no site passes
    cases["empty_threshold"] = (hist, counts, {})
    cases["all_empty"] = (np.zeros((2, 3, 2, 33), np.int32), np.array([40, 30], np.int64), {})
    cases["no_control"] = level_case(3, 2, 33, 150, 0, 13, central=0.4) + ({},)
    cases["no_records"] = (np.zeros((2, 1, 2, 20), np.int32), np.zeros(2, np.int64), {"local": True})
    cases["planted"] = planted_case() + ({},)
    cases["planted_local"] = level_case(2, 2, 100, 1500, 1000, 15, central=0.5, sd=4.0) + ({"local": True, "max_width": 40},)
    cases["large_n"] = level_case(2, 2, 182, 100000, 100000, 16, central=0.05, sd=6.0, keep=0.8) + ({},)
    cases["many_units"] = level_case(300, 2, 33, 200, 100, 17, central=0.2) + ({},)
    return cases


test_cases.__test__ = False       # a model function, not a test


def planted_case():
    """2000 primary records of M = 182 starts, 60 % of them with the site within a few bins (sd 5) of the
    middle, the rest and the 2000 control records uniform: the chosen region is centred by construction and
    about +-2 sd wide."""
    return level_case(3, 3, 182, 2000, 2000, 14, central=0.6, sd=5.0)
