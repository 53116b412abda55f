"""CPU: the numpy model of site q-values (tests/siteq_model.py) against brute force and the textbook
Benjamini-Hochberg procedure, and the host code around it (signatures, SiteCalls.qvalue, bed columns)."""
import numpy as np
import pytest

import actnull_model as am
import pwmsites_model as pm
import siteq_model as qm
import sites_model as sm


def _tables(widths, seed, bins=100):
    S, w, scale, _ = pm.quantise(pm.dirichlet_motifs(widths, seed), pm.uniform(), 0.1, bins)
    return S, pm.live_widths(w, scale)


# ---------------------------------------------------------------- the histogram model
@pytest.mark.parametrize("period,both", [(0, True), (0, False), (50, True), (13, False)])
def test_histogram_loop_equals_vectorised_and_the_scan(period, both):
    S, lw = _tables([0, 1, 5, 12, 3], seed=1)
    codes = pm.random_codes(300, seed=2, n_frac=0.03)
    codes[100:106] = 4                                     # a run of N
    want = qm.score_histogram_loop(S, lw, 100, codes, period=period, both=both)
    assert np.array_equal(qm.score_histogram(S, lw, 100, codes, period=period, both=both), want)
    assert np.array_equal(want.sum(axis=1), qm.live_tests(lw, S.shape[1], codes, period, both))
    assert want[0].sum() == 0 and want[1:].sum(axis=1).min() > 0
    # the scan at threshold 0 lists every test: its scores are the histogram's
    off, _, isc = pm.scan(S, lw, np.zeros(len(lw), np.int32), codes, period=period, both=both)
    for m in range(len(lw)):
        got = np.bincount(isc[off[2 * m]:off[2 * m + 2]], minlength=want.shape[1])
        assert np.array_equal(got, want[m]), m
    # a sub-range of starts, and two halves that add up
    part = qm.score_histogram(S, lw, 100, codes, start=40, n_positions=150, period=period, both=both)
    assert np.array_equal(part, qm.score_histogram_loop(S, lw, 100, codes, start=40, n_positions=150, period=period,
                                                        both=both))
    if period == 0:
        wmax = S.shape[1]
        a = qm.score_histogram(S, lw, 100, codes[:150 + wmax - 1], n_positions=150, both=both)
        b = qm.score_histogram(S, lw, 100, codes[150:], both=both)
        assert np.array_equal(a + b, want)


# ---------------------------------------------------------------- the q-table model
def _random_table(U, B, seed, n=400, ties=False):
    """obs with empty bins and p non-increasing in the bin (with runs of equal p when ties)."""
    g = np.random.default_rng(seed)
    obs = np.zeros((U, B), dtype=np.int64)
    for u in range(U):
        obs[u] = np.bincount(np.minimum((g.exponential(B / 8.0, size=n)).astype(np.int64), B - 1), minlength=B)
    steps = g.random((U, B)) * (g.random((U, B)) < (0.3 if ties else 1.0))
    steps[:, -1] += 0.05                                    # every p is positive
    p = np.cumsum(steps[:, ::-1], axis=1)[:, ::-1]
    p = p / (p[:, :1] * (1.0 + g.random((U, 1))))          # in (0, 1), not on a grid
    return obs, p


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("B", [1, 7, 202])
def test_qtable_equals_sorted_bh_bit_for_bit(B, ties):
    obs, p = _random_table(3, B, seed=B + ties, ties=ties)
    q, total, _ = qm.qtable(obs, p)
    assert np.array_equal(total, obs.sum(axis=1))
    for u in range(3):
        bins, pv = qm.per_test(obs[u], p[u])
        assert len(pv) == total[u]
        assert np.array_equal(qm.bh_sorted(pv), q[u][bins]), (u, "per-test BH and the table differ")
        assert np.all(np.diff(q[u]) <= 0) and q[u].max() <= 1.0 and q[u].min() >= 0.0
    if ties and B > 1:
        assert any(len(np.unique(p[u][obs[u] > 0])) < int((obs[u] > 0).sum()) for u in range(3))


def test_qtable_edges():
    B = 50
    obs = np.zeros((4, B), dtype=np.int64)
    p = np.tile(np.linspace(1.0, 0.0, B), (4, 1))
    obs[1, :] = 3                                           # unit 0: no observations
    obs[2, :] = 1
    obs[3, 10] = 5
    p[2] = 1e-9 * np.linspace(1.0, 0.5, B)                  # every bin qualifies
    p[3] = 1.0                                              # none does
    q, total, first = qm.qtable(obs, p, alpha=0.05)
    assert np.all(q[0] == 1.0) and total[0] == 0 and first[0] == B
    assert first[2] == 0 and np.all(q[2] <= 0.05)
    assert first[3] == B and np.all(q[3] == 1.0)
    assert 0 < first[1] < B and np.all(q[1][first[1]:] <= 0.05) and np.all(q[1][:first[1]] > 0.05)
    # bins above the last observation keep the running minimum; bins below the first one are 1 or the minimum so far
    assert np.all(q[3][:10] == 1.0)
    # alpha = 1 takes every bin, alpha = 0 only a q of exactly 0 (p = 0 at an observed bin)
    assert np.all(qm.qtable(obs, p, 1.0)[2] == 0)
    assert qm.qtable(obs, p, 0.0)[2][1] == B - 1


def test_thresholds_list_exactly_the_sites_with_small_q():
    """Filter sites: activation > threshold(first) <=> q <= alpha.  PWM sites: score >= max(thr, first) likewise."""
    g = np.random.default_rng(5)
    U, P, alpha = 4, 3000, 0.1
    acts = np.exp(g.normal(0.0, 1.0, size=(U, P))).astype(np.float16)
    acts[0, :40] = np.float16(30.0)                         # a planted signal
    acts[1] = np.float16(0.0)                               # nothing ever
    null = np.exp(g.normal(0.0, 1.0, size=(U, 20000))).astype(np.float16)
    null[3] = np.float16(1e-3)                              # every observed value of unit 3 beats its null
    obs, p = am.histogram(acts), qm.empirical_p(am.histogram(null))
    assert np.array_equal(p[np.arange(U), am.bins(acts[:, 0])], am.pvalue(am.histogram(null), np.arange(U), acts[:, 0]))
    q, _, first = qm.qtable(obs, p, alpha)
    thr = qm.filter_thresholds(first)
    lists = sm.site_lists(acts, thr)
    for u in range(U):
        want = np.flatnonzero(q[u][am.bins(acts[u])] <= alpha)
        assert np.array_equal(lists[u][0], want), u
    assert len(lists[0][0]) >= 40 and len(lists[1][0]) == 0 and len(lists[3][0]) == P
    assert thr[3] == np.float32(np.float16(1e-3)) and np.isinf(thr[1])     # just above the null's only value
    assert np.array_equal(qm.filter_thresholds([0, 1, qm.ACT_INF, qm.ACT_INF + 1, qm.ACT_BINS]),
                          np.array([-1.0, 0.0, 65504.0, np.inf, np.inf], dtype=np.float32))
    # PWM
    mats = pm.dirichlet_motifs([8, 0, 11], seed=6, alpha=0.1)
    codes = pm.random_codes(3000, seed=7)
    for at in (100, 900, 2000):
        pm.plant(codes, mats[0], at)
        pm.plant(codes, mats[2], at + 300, reverse=True)
    c = pm.calls(mats, codes, 1e-2)
    S, w, scale, _ = pm.quantise(mats)
    lw = pm.live_widths(w, scale)
    hist = qm.score_histogram(S, lw, 100, codes)
    q, total, first = qm.qtable(hist, c["tail"], 0.05)
    off, pos, isc = pm.scan(S, lw, np.maximum(c["thresholds"], first), codes)
    keep = q[c["unit"], c["iscore"]] <= 0.05
    assert 6 <= keep.sum() < len(keep)
    assert np.array_equal(pos, c["start"][keep]) and np.array_equal(isc, c["iscore"][keep])
    assert total[1] == 0 and np.array_equal(total, qm.live_tests(lw, S.shape[1], codes))


# ---------------------------------------------------------------- host code
def test_signatures_and_constants():
    from explainn_amd import _lib
    for name, nargs in (("explainn_pwm_score_histogram", 13), ("explainn_site_qvalues", 9)):
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.SITEQ_MAX_BINS == qm.ACT_BINS == _lib.ACT_BINS and _lib.PWM_HIST_SLICE == 1 << 30


def test_sitecalls_carry_qvalues():
    from explainn_amd import pwmsites, sites
    a = sites.SiteCalls([0, 1, 2], [5, 9], [1, -1], [2.0, 3.0], 4, pvalue=[0.1, 0.2], qvalue=[0.3, 0.4])
    b = sites.SiteCalls([0, 1], [7], [1], [1.0], 6, pvalue=[0.5])
    assert sites.concat_units(a, b).qvalue is None and sites.concat_units(a, b).pvalue is not None
    both = sites.concat_units(a, a)
    assert np.array_equal(both.qvalue, [0.3, 0.4, 0.3, 0.4]) and both.qvalue.dtype == np.float64
    with pytest.raises(ValueError, match="qvalue"):
        sites.SiteCalls([0, 1], [7], [1], [1.0], 6, qvalue=[0.5, 0.5])
    rows = sites.bed_rows("chr1", a)
    assert rows == ["chr1\t5\t9\tfilter0\t2\t+\t0.1\t0.3\n", "chr1\t9\t13\tfilter1\t3\t-\t0.2\t0.4\n"]
    a.qvalue = None
    assert sites.bed_rows("chr1", a) == [r.rsplit("\t", 1)[0] + "\n" for r in rows]
    c = pwmsites.PwmCalls([0, 1], [3], [1], [1.5], [6], ["m"], [77], [1e-3], [0.02])
    assert pwmsites.bed_rows("s", c) == ["s\t3\t9\tm\t1.5\t+\t0.001\t0.02\n"]
    assert pwmsites.PwmCalls([0, 1], [3], [1], [1.5], [6], ["m"], [77], [1e-3]).qvalue is None
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            sites.check_qvalue(bad)


def test_cli_flag_checks():
    from explainn_amd import calibrate, pwmsites, sites
    with pytest.raises(SystemExit, match="--null"):
        sites.main(["m.pth", "x.fa", "-t", "t.tsv", "--qvalues"])
    with pytest.raises(SystemExit, match="--qvalues"):
        sites.main(["m.pth", "x.fa", "-t", "t.tsv", "--max-qvalue", "0.1"])
    with pytest.raises(SystemExit, match="--bg sequence"):
        pwmsites.main(["m.meme", "x.fa", "--qvalues", "--bg", "sequence"])
    with pytest.raises(SystemExit, match="--qvalues"):
        pwmsites.main(["m.meme", "x.fa", "--max-qvalue", "0.1"])
    with pytest.raises(SystemExit, match="go together"):
        calibrate.main(["m.pth", "x.fa", "-o", "t.tsv", "--qvalue", "0.1"])
