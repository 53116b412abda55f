"""CPU: the fp64 model of motif centrality (tests/centrality_model.py) against brute force and scipy, and the
host logic of explainn_amd.centrality that needs no device.

test_logsf_matches_scipy measures the model's binomial tail against scipy.stats.binom.logsf and holds it to
centrality_model.LOGSF_DEVIATION, the yardstick of tests/test_gpu_centrality.py."""
import math
import os
import re

import numpy as np
import pytest

import centrality_model as cm
import enrichment_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- histograms
def test_positions_equal_the_record_by_record_count():
    for units, n, T, M, seed in ((2, 50, 1, 1, 0), (3, 70, 3, 2, 1), (2, 200, 16, 65, 2), (1, 0, 2, 9, 3)):
        bits, site, labels, thr = cm.best_case(units, n, T, M, seed, labels_upto=4)
        hist, counts = cm.positions(bits, site, labels, thr, M)
        assert hist.shape == (units, T, 2, M) and hist.dtype == np.int32
        assert np.array_equal(hist, cm.positions_brute(bits, site, labels, thr, M))
        assert list(counts) == [int(np.sum(labels == 1)), int(np.sum(labels == 0))]
        # a site at every threshold it passes: the rows of ascending thresholds are nested
        assert np.all(hist[:, :-1] >= hist[:, 1:])
    bits, site, labels, thr = cm.best_case(2, 300, 2, 20, 4)
    assert np.any(site < 0) and np.any((site >> 1) >= 20) and np.any(bits & 0x8000) and np.any(labels > 1)
    hist, _ = cm.positions(bits, site, labels, thr, 20)
    inc = (labels <= 1)[None, :] & (site >= 0) & ((site >> 1) < 20)
    assert hist[:, 0].sum() <= inc.sum() and hist.sum() > 0
    # `>` is strict, and bit 15 is not read
    one = np.array([[0x3C00, 0xBC00, 0x3C01]], np.uint16)
    h, _ = cm.positions(one, np.array([[0, 2, 4]], np.int32), np.ones(3, np.uint8), np.array([[1.0]], np.float32), 3)
    assert h[0, 0, 0].tolist() == [0, 0, 1]
    # NaN patterns and NaN thresholds never count
    h, _ = cm.positions(np.array([[0x7E00, 0x3C00]], np.uint16), np.array([[0, 2]], np.int32), np.ones(2, np.uint8),
                        np.array([[0.0, np.nan]], np.float32), 2)
    assert h[0, :, 0].tolist() == [[0, 1], [0, 0]]


# ------------------------------------------------------------------------------------------- the test
def test_regions_of_both_modes():
    assert cm.regions(1) == [] and cm.regions(1, local=True) == [] and cm.regions(2) == []
    assert cm.regions(2, local=True) == [(0, 1), (1, 1)]
    assert cm.regions(5) == [(1, 3), (2, 1)] and cm.regions(6) == [(1, 4), (2, 2)]
    assert cm.regions(7, min_width=2, max_width=4) == [(2, 3)]
    assert cm.regions(6, max_width=100) == cm.regions(6) and cm.regions(6, min_width=5) == []
    for M in (2, 5, 8):
        loc = cm.regions(M, local=True)
        assert len(loc) == M * (M + 1) // 2 - 1 and len(set(loc)) == len(loc)
        assert all(0 <= lo and lo + w <= M and 1 <= w < M for lo, w in loc)
        assert set(cm.regions(M)) <= set(loc)
        assert all(lo + (lo + w - 1) == M - 1 for lo, w in cm.regions(M))     # centred: equally far from both ends
    assert [r for r in cm.regions(8, local=True, min_width=3, max_width=4)] == \
        [(lo, 3) for lo in range(6)] + [(lo, 4) for lo in range(5)]


def test_counts_and_the_chosen_region_against_brute_force():
    """Site lists, counted region by region: the model's prefix sums, its best (threshold, region) under the
    tie rule and n_tests."""
    g = np.random.default_rng(0)
    for trial in range(6):
        M, T, local = int(g.integers(2, 14)), int(g.integers(1, 4)), bool(trial % 2)
        starts = [g.integers(0, M, size=int(g.integers(0, 40))) for _ in range(T)]
        ctrl = [g.integers(0, M, size=int(g.integers(0, 40))) for _ in range(T)]
        h = np.stack([np.stack([np.bincount(s, minlength=M), np.bincount(c, minlength=M)]) for s, c in zip(starts, ctrl)])
        counts = np.array([60, 50])
        kw = {"local": local, "min_width": int(g.integers(1, 3)), "min_sites": int(g.integers(0, 10))}
        st = cm.unit_stats(h, counts, **kw)
        best = None
        tried = [t for t in range(T) if len(starts[t]) >= max(kw["min_sites"], 1)]
        regs = cm.regions(M, local, kw["min_width"])
        for t in tried:
            for lo, w in regs:
                key = (cm.logp(len(starts[t]), cm.brute_count(starts[t], lo, w), w, M), w, lo, t)
                best = key if best is None or key < best else best
        if best is None:
            assert st["best_width"] == 0 and st["n_tests"] == 0 and st["log_pvalue"] == 0.0 and st["sites"] == 0
            continue
        lp, w, lo, t = best
        assert (st["log_pvalue"], st["best_width"], st["best_lo"], st["best_t"]) == best
        assert st["sites"] == len(starts[t]) and st["count"] == cm.brute_count(starts[t], lo, w)
        assert st["ctrl_sites"] == len(ctrl[t]) and st["ctrl_count"] == cm.brute_count(ctrl[t], lo, w)
        assert st["n_tests"] == len(tried) * len(regs)
        assert st["log_padj"] == em.log_padj(lp, st["n_tests"])


def test_tie_rule():
    # two equal peaks: the narrower region, then the lower lo, then the lower threshold
    h = np.zeros((2, 2, 9), np.int64)
    h[:, 0, 1] = h[:, 0, 6] = 5
    h[:, 0] += 1
    st = cm.unit_stats(h, [100, 0], local=True)
    assert (st["best_t"], st["best_lo"], st["best_width"], st["count"]) == (0, 1, 1, 6)
    # nothing enriched anywhere: every ln p is the assigned 0, and the same rule decides
    flat = np.ones((2, 2, 8), np.int64)
    st = cm.unit_stats(flat, [8, 8])
    assert (st["log_pvalue"], st["best_width"], st["best_lo"], st["best_t"], st["gap"]) == (0.0, 2, 3, 0, np.inf)
    st = cm.unit_stats(flat, [8, 8], local=True)
    assert (st["best_width"], st["best_lo"], st["n_tests"]) == (1, 0, 2 * 35)
    assert cm.logp(10, 5, 4, 8) == 0.0 and cm.logp(10, 6, 4, 8) < 0.0             # c M > n w, strictly


def logsf_grid(n):
    """Enriched (n, c, w, M) around and far above the mean, q = w / M from 1 / M to (M - 1) / M."""
    out = set()
    for M in (2, 64, 182):
        for w in sorted({1, 2, M // 4, M // 2, M - 2, M - 1}):
            if not 1 <= w < M:
                continue
            q = w / M
            mean, sd = n * q, math.sqrt(n * q * (1 - q))
            for z in (0, 0.5, 1, 3, 6, 10, 20, 30):
                for j in (0, 1):
                    c = min(int(math.floor(mean)) + 1 + int(round(z * sd)) + j, n)
                    if c * M > n * w:
                        out.add((n, c, w, M))
    return sorted(out)


def test_logsf_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    for n, bound in cm.LOGSF_DEVIATION.items():
        worst, terms = 0.0, 0
        for _, c, w, M in logsf_grid(n):
            ref = float(stats.binom.logsf(c - 1, n, w / M))
            assert np.isfinite(ref)
            got, t = cm.binom_logsf(n, c, w, M, return_terms=True)
            worst, terms = max(worst, abs(got - ref)), max(terms, t)
        print("n = %d: largest |ln p - scipy| = %.3g over %d points, at most %d terms" % (
            n, worst, len(logsf_grid(n)), terms))
        assert len(logsf_grid(n)) >= 100
        assert worst <= bound, n
    assert cm.deviation(150) == cm.LOGSF_DEVIATION[400] and cm.deviation(100000) == cm.LOGSF_DEVIATION[10 ** 6]
    assert cm.log_tolerance(150) >= 64 * np.spacing(math.lgamma(151.0))
    assert 2 * max(cm.log_tolerance(n) for n in cm.LOGSF_DEVIATION) < cm.MIN_GAP


def test_pvalues_are_binomial_and_fisher():
    stats = pytest.importorskip("scipy.stats")
    hist, counts = cm.planted_case()
    for h in hist:
        st = cm.unit_stats(h, counts)
        assert st["log_pvalue"] < -700                  # past the range of a double p: scipy's logsf is -inf here
        a, b = st["count"], st["ctrl_count"]
        lf = stats.hypergeom.logsf(a - 1, counts.sum(), counts[0], a + b)
        assert st["log_fisher"] < -50 and st["log_fisher"] == pytest.approx(lf, rel=1e-10)
    hist, counts, kw = cm.test_cases()["odd_centred"]
    for h in hist:
        st = cm.unit_stats(h, counts, **kw)
        a, b = st["count"], st["ctrl_count"]
        p = stats.binom.sf(a - 1, st["sites"], st["best_width"] / h.shape[2])
        assert st["log_pvalue"] == pytest.approx(math.log(p), rel=1e-11)
        f = stats.fisher_exact([[a, counts[0] - a], [b, counts[1] - b]], alternative="greater")[1]
        assert st["log_fisher"] == (pytest.approx(math.log(f), rel=1e-10) if a * counts[1] > b * counts[0] else 0.0)
    assert cm.log_fisher(5, 5, 50, 50) == 0.0 and cm.log_fisher(6, 5, 50, 50) < 0.0 and cm.log_fisher(6, 0, 50, 0) == 0.0
    assert cm.log_fisher(60, 5, 50, 50) == 0.0                                   # counts that belong to no table


def test_planted_region_is_the_central_one():
    hist, counts = cm.planted_case()
    M = hist.shape[3]
    for h in hist:
        st = cm.unit_stats(h, counts)
        lo, hi = st["best_lo"], st["best_lo"] + st["best_width"] - 1
        assert lo + hi == M - 1 and 10 <= st["best_width"] <= 40               # centred, about +-2 sd of 5 bins
        assert st["count"] > 0.5 * st["sites"] and st["ctrl_count"] < 0.3 * st["ctrl_sites"]
    hist, counts, kw = cm.test_cases()["planted_local"]
    for h in hist:
        st = cm.unit_stats(h, counts, **kw)
        mid = (hist.shape[3] - 1) / 2.0
        assert st["best_lo"] < mid < st["best_lo"] + st["best_width"] - 1 and st["best_width"] <= 30


def test_gaps_and_branches_of_the_inputs_the_gpu_test_reuses():
    """The GPU test demands the chosen threshold and region exactly, of every unit of every case: each best
    ln p must stand clear of the best one of a differing (n, c, w) by more than MIN_GAP.  No unit is left out."""
    smallest, short, full, untried = np.inf, 0, 0, 0
    for name, (hist, counts, kw) in cm.test_cases().items():
        st = cm.test_stats(hist, counts, **kw)
        assert np.all(st["gap"] > cm.MIN_GAP), (name, st["gap"])
        smallest = min(smallest, st["gap"].min())
        short += int(np.sum(st["log_pvalue"] < -30.0))
        full += int(np.sum((st["log_pvalue"] >= -30.0) & (st["log_pvalue"] < 0.0)))
        untried += int(np.sum(st["best_width"] == 0))
        if name in ("M1", "M2_centred", "all_empty", "no_records"):
            assert not st["best_width"].any() and not st["n_tests"].any()
        if name == "empty_threshold":
            assert np.all(st["best_t"] != 1) and np.all(st["n_tests"] == 2 * len(cm.regions(33)))
        if name == "min_sites":
            assert np.any(st["n_tests"] < 4 * len(cm.regions(33))) and np.all(st["sites"] >= 40)
        if name == "no_control":
            assert not st["log_fisher"].any() and not st["ctrl_sites"].any()
        if name == "large_n":
            assert np.all(st["log_pvalue"] < -30.0) and np.all(st["sites"] > 50000)
    assert short > 0 and full > 0 and untried > 0                               # both log_padj branches are met
    print("smallest gap between the best ln p and the runner-up of other counts: %.3g" % smallest)


# ------------------------------------------------------------------------------------------- host logic
def test_region_coordinates_for_odd_and_even_m():
    from explainn_amd.centrality import region_coordinates
    # L = 27, k = 19: M = 9 starts; the centred region [3, 5] spans the bases [3, 24): the middle of the record
    s, e, c = region_coordinates([3, 0, 4], [3, 1, 0], 19, 27)
    assert s.tolist() == [3, 0, 0] and e.tolist() == [24, 19, 0]
    assert c[0] == 0.0 and c[1] == (0 + 0 + 19 - 27) / 2.0 and np.isnan(c[2])
    # even M = 10 (L = 28): [4, 5] is centred; [4, 4] sits half a base left of the centre
    s, e, c = region_coordinates([4, 4], [2, 1], 19, 28)
    assert e.tolist() == [24, 23] and c.tolist() == [0.0, -0.5]
    for M, k in ((9, 19), (10, 19), (182, 19), (59, 2)):
        L = M + k - 1
        for j, w in cm.regions(M):
            s, e, c = region_coordinates(j, w, k, L)
            assert c == 0.0 and s + e == L and e - s == w + k - 1               # every centred region: offset 0


def _result(units=5, seed=0, control=True):
    from explainn_amd.centrality import Centrality
    g = np.random.default_rng(seed)
    lp = -np.abs(g.standard_normal(units)) * 10
    lp[1] = lp[3]                                       # a tie: the lower filter comes first
    m = g.integers(1, 500, size=units)
    width = g.integers(1, 100, size=units)
    width[np.argmax(lp)] = 0                            # a unit for which nothing was tried
    lo = g.integers(0, 80, size=units)
    sites = g.integers(50, 90, size=units)
    thr = np.sort(g.random((units, 3)).astype(np.float32), axis=1)
    nc = 70 if control else 0
    return Centrality(g.integers(0, 3, size=units), lo, width, sites, sites // 2, m, lp,
                      [em.log_padj(x, int(k)) for x, k in zip(lp, m)], g.integers(0, 60, size=units) * bool(nc),
                      g.integers(0, 20, size=units) * bool(nc), -g.random(units) * bool(nc), [90, nc], thr, 19, 200, True, "fwd")


def test_table_rows_order_and_columns():
    from explainn_amd import centrality as ce
    res = _result()
    rows = ce.table_rows(res)
    assert [r[0] for r in rows] == sorted(range(5), key=lambda u: (res.log_pvalue[u], u))
    assert [r[0] for r in rows].index(1) + 1 == [r[0] for r in rows].index(3)
    u = rows[0][0]
    M = 200 - 19 + 1
    assert rows[0][1] == float(res.thresholds[u, res.best_t[u]]) and rows[0][2] == res.sites[u]
    assert rows[0][3] == res.best_lo[u] and rows[0][4] == res.best_lo[u] + res.best_width[u] - 1 + 19
    assert rows[0][5] == res.best_width[u] and rows[0][7] == res.count[u]
    assert rows[0][6] == (2 * res.best_lo[u] + res.best_width[u] - 1 + 19 - 200) / 2.0
    assert rows[0][8] == pytest.approx(res.sites[u] * res.best_width[u] / M)
    assert rows[0][11] == pytest.approx(math.exp(res.log_padj[u]) * 5)
    q = __import__("spacing_model").benjamini_hochberg(np.exp(res.log_pvalue))
    assert np.allclose(res.qvalue, q, rtol=1e-12, atol=0)
    assert len(rows[0]) == len(ce.COLUMNS) + 3 and rows[0][13:] == (res.ctrl_sites[u], res.ctrl_count[u], res.log_fisher[u])
    z = int(np.flatnonzero(res.best_width == 0)[0])
    assert z != u and np.isnan(res.center[z]) and res.region_end[z] == 0 and res.expected[z] == 0.0
    kept = ce.table_rows(res, max_evalue=float(np.sort(res.evalue)[1]))
    assert 0 < len(kept) < 5 and all(r[11] <= np.sort(res.evalue)[1] for r in kept)
    plain = ce.table_rows(_result(control=False))
    assert len(plain[0]) == len(ce.COLUMNS) and len(ce.table_rows(res, control=False)[0]) == len(ce.COLUMNS)

    class Sink(list):
        write = list.append
    out = Sink()
    ce.write_table(out, rows)
    assert out[0] == "\t".join(ce.COLUMNS + ce.CONTROL_COLUMNS) + "\n" and len(out) == 6
    assert out[1].startswith("filter%d\t" % u) and out[1].count("\t") == len(ce.COLUMNS) + 2
    out = Sink()
    ce.write_table(out, plain)
    assert out[0] == "\t".join(ce.COLUMNS) + "\n" and out[1].count("\t") == len(ce.COLUMNS) - 1
    assert ce.COLUMNS == ("Filter", "Threshold", "Sites", "RegionStart", "RegionEnd", "Width", "Center", "Count",
                          "Expected", "LogPvalue", "LogPadj", "Evalue", "Qvalue")
    assert ce.CONTROL_COLUMNS == ("CtrlSites", "CtrlCount", "LogFisher")


def test_save_and_load(tmp_path):
    from explainn_amd import centrality as ce
    res = _result(seed=2)
    res.save(tmp_path / "c.npz")
    back = ce.Centrality.load(tmp_path / "c.npz")
    for f in ce._FIELDS + ("counts", "thresholds", "threshold", "region_start", "region_end", "center", "expected",
                           "evalue", "qvalue", "fisher_evalue", "fisher_qvalue"):
        assert np.array_equal(getattr(back, f), getattr(res, f), equal_nan=True), f
    assert (back.kernel_size, back.length, back.local, back.strands) == (19, 200, True, "fwd")
    hist, counts = cm.level_case(3, 2, 12, 40, 30, 0)
    pos = ce.SitePositions(hist, counts, np.arange(6, dtype=np.float32).reshape(3, 2), 19, 30, "fwd")
    pos.save(tmp_path / "p.npz")
    p2 = ce.SitePositions.load(tmp_path / "p.npz")
    assert np.array_equal(p2.hist, hist) and p2.hist.dtype == np.int32 and np.array_equal(p2.counts, counts)
    assert np.array_equal(p2.thresholds, pos.thresholds) and (p2.kernel_size, p2.length, p2.strands) == (19, 30, "fwd")
    assert (p2.units, p2.starts) == (3, 12)
    with pytest.raises(ValueError, match="M = L - k"):
        ce.SitePositions(hist, counts, np.zeros((3, 2), np.float32), 19, 31)


def test_value_errors():
    from explainn_amd import ExplaiNN, centrality as ce
    from explainn_amd.enrichment import RecordBest
    model = ExplaiNN(4, 19, 200, 1).eval()
    thr = np.zeros(4, np.float32)
    recs = [np.zeros(40, np.uint8), np.zeros(41, np.uint8), np.zeros(5, np.uint8)]
    for fn in (ce.site_positions, ce.centrality):
        with pytest.raises(ValueError, match="fixed-width summit windows"):
            fn(model, recs, thr)
        with pytest.raises(ValueError, match="fixed-width summit windows"):
            fn(model, recs[:1], thr, control=recs[1:])
        with pytest.raises(ValueError, match="no primary"):
            fn(model, [], thr)
        with pytest.raises(ValueError, match="as long as the kernel"):
            fn(model, recs[2:], thr)
        with pytest.raises(ValueError, match="strands"):
            fn(model, recs[:1], thr, strands="rev")
        for bad in (np.zeros(3), np.zeros((4, 0)), np.zeros((2, 4)), np.zeros((4, 2, 1))):
            with pytest.raises(ValueError, match="thresholds must be"):
                fn(model, recs[:1], bad)
        with pytest.raises(ValueError, match="at most 16 thresholds"):
            fn(model, recs[:1], np.zeros((4, 17)))
    for kw in ({"min_width": 0}, {"min_width": 5, "max_width": 4}, {"min_sites": -1}):
        with pytest.raises(ValueError, match="min_width|min_sites"):
            ce.centrality(model, recs[:1], thr, **kw)
        with pytest.raises(ValueError, match="min_width|min_sites"):
            ce.test_positions(None, **kw)
    with pytest.raises(ValueError, match="SitePositions"):
        ce.test_positions(None)
    assert ce.common_length([40, 3, 40, 0], 19) == 40 and ce.check_thresholds(thr, 4).shape == (4, 1)
    assert ce.check_widths(1, None, 0) == (1, None, 0)
    # saved best sites of unequal lengths, and of another model
    rb = RecordBest(np.zeros((4, 2), np.float16), np.zeros((4, 2), np.int32), np.ones((4, 2), np.int8), [40, 41], 19)
    with pytest.raises(ValueError, match="fixed-width summit windows"):
        ce.positions_from_best(rb, thr)
    ok = RecordBest(np.zeros((4, 2), np.float16), np.zeros((4, 2), np.int32), np.ones((4, 2), np.int8), [40, 40], 19)
    other = RecordBest(np.zeros((3, 1), np.float16), np.zeros((3, 1), np.int32), np.ones((3, 1), np.int8), [40], 19)
    with pytest.raises(ValueError, match="control's best sites"):
        ce.positions_from_best(ok, thr, other)
    with pytest.raises(ValueError, match="RecordBest"):
        ce.positions_from_best(None, thr)


def test_cli_parser():
    from explainn_amd import centrality as ce
    a = ce._parser().parse_args(["m.pth", "p.fa", "-t", "t.tsv", "-o", "out.tsv"])
    assert (a.thresholds, a.control, a.local, a.min_width, a.max_width, a.min_sites, a.strands, a.max_evalue,
            a.save_positions) == (["t.tsv"], None, False, 1, None, 1, "both", 10.0, None)
    a = ce._parser().parse_args(["m.pth", "p.fa", "-t", "a.tsv", "-t", "b.tsv", "--control", "c.fa", "--local",
                                 "--min-width", "3", "--max-width", "50", "--min-sites", "20", "--strands", "fwd",
                                 "--max-evalue", "0.5", "--save-positions", "p.npz", "-o", "o.tsv"])
    assert (a.thresholds, a.control, a.local, a.min_width, a.max_width, a.min_sites, a.strands, a.max_evalue,
            a.save_positions, a.output_file) == (["a.tsv", "b.tsv"], "c.fa", True, 3, 50, 20, "fwd", 0.5, "p.npz", "o.tsv")
    with pytest.raises(SystemExit):
        ce._parser().parse_args(["m.pth", "p.fa", "-o", "o.tsv"])


def test_constants_agree_with_the_header():
    from explainn_amd import _lib, centrality as ce
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert int(re.search(r"#define EXPLAINN_CENTRALITY_MAX_THRESHOLDS (\d+)", text).group(1)) == \
        _lib.CENTRALITY_MAX_THRESHOLDS == ce.MAX_THRESHOLDS
    assert int(re.search(r"#define EXPLAINN_CENTRALITY_MAX_REGIONS (\d+)", text).group(1)) == _lib.CENTRALITY_MAX_REGIONS
    M = 2895
    assert M * (M + 1) // 2 - 1 <= _lib.CENTRALITY_MAX_REGIONS < (M + 1) * (M + 2) // 2 - 1
    assert len(cm.FIELDS) == len(ce._FIELDS) and cm.FIELDS == ce._FIELDS
