"""CPU: the numpy model of known-motif enrichment and centrality (tests/pwmbest_model.py) against brute
force, the integer-to-float16 bridge, and the host half of explainn_amd/pwmenrich.py (result assembly, tables)
fed from the model.  The planted case of tests/test_gpu_pwmbest.py meets its assertions here, in the model."""
import io
import os
import re

import numpy as np
import pytest

import centrality_model as cm
import pwmbest_model as bm
import pwmsites_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRIDGE_THRESHOLDS = (0, 1, 532, 1023, 1024, 1025, 8193)


def _palindrome(w=8, seed=3):
    """A motif equal to its own reverse complement: column j = column w-1-j with the bases reversed."""
    half = np.random.default_rng(seed).dirichlet(np.full(4, 0.3), size=w // 2)
    return np.concatenate([half, half[::-1, ::-1]])


# ---------------------------------------------------------------- best sites
@pytest.mark.parametrize("both", [False, True])
def test_vectorised_best_equals_brute_force(both):
    mats = pm.dirichlet_motifs([1, 4, 6, 9], seed=1) + [_palindrome(), np.full((5, 4), 0.25), np.zeros((0, 4))]
    tab = bm.tables(mats)
    assert tab["live"][-1] == 0 and tab["live"][-2] == 0          # an empty motif and a flat one
    g = np.random.default_rng(2)
    recs = [pm.random_codes(int(n), seed=int(n), n_frac=0.05) for n in (0, 1, 3, 4, 6, 9, 10, 40, 41, 97)]
    recs.append(np.full(30, 4, np.uint8))                         # all N
    recs.append(np.array([5, 255, 0, 1, 2, 3, 0, 1, 2, 3, 9], np.uint8))      # bytes above 4 read as N
    recs.append(np.zeros(50, np.uint8))                           # flat: every start ties, the lowest wins
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    flat = np.concatenate(recs)
    a = bm.record_best(tab["S"], tab["live"], flat, off, both)
    b = bm.record_best(tab["S"], tab["live"], flat, off, both, best=bm.best_brute)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 0
    bits, site = a[0], a[1]
    assert np.all(site[-1] == -1) and np.all(bits[-1] == 0) and np.all(site[-2] == -1)
    assert np.all(site[:-2, len(recs) - 3] == -1)                 # the all-N record
    assert np.all(site[:5, -1] >> 1 == 0)                         # the flat record: start 0 on the better strand
    assert site[4, -1] == 0                                       # (the palindrome: both strands alike, '+')
    assert np.all(site[2, [0, 1, 2, 3]] == -1)                    # shorter than w = 6
    if both:
        # the palindrome scores both strands alike everywhere: '+' wins every tie
        assert np.all(site[4][site[4] >= 0] & 1 == 0)
        assert np.any(site[:4] & 1 == 1)                          # the other motifs do use '-'


@pytest.mark.parametrize("both", [False, True])
def test_equal_length_form_equals_the_record_loop(both):
    tab = bm.tables(pm.dirichlet_motifs([4, 7, 13], seed=6) + [_palindrome(6), np.zeros((0, 4))])
    rows = pm.random_codes(300 * 12, seed=7, n_frac=0.05).reshape(300, 12)
    rows[5] = 4
    rows[6] = 0
    want = bm.record_best(tab["S"], tab["live"], rows.reshape(-1), np.arange(301) * 12, both)
    got = bm.record_best_equal(tab["S"], tab["live"], rows, both)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.all(got[1][2] == -1) and np.all(got[1][:, 5] == -1) and np.any(got[1][:2] >= 0)


def test_tie_rule_key_order():
    """Score first, then the lowest start, then '+': read off a hand-made table."""
    S = np.zeros((1, 2, 4), np.int16)
    S[0, 0] = [5, 0, 0, 3]                                        # A first: 5; T first: 3
    S[0, 1] = [0, 0, 0, 5]                                        # T second: 5
    for best in (bm.best_brute, bm.best_of_record):
        # AC: '+' = 5 + 0, '-' (its reverse complement GT) = 0 + 5: a tie at one start goes to '+'
        assert best(S[0], 2, np.array([0, 1]), True) == (5, 0)
        # CCAT: AT at start 2 scores 10 on both strands (it is its own reverse complement): start 2, '+'
        assert best(S[0], 2, np.array([1, 1, 0, 3]), True) == (10, 4)
        # GTCC: GT scores 5 on both strands at start 0, TC 3, CC 0: the maximum's only start, '+'
        assert best(S[0], 2, np.array([2, 3, 1, 1]), True) == (5, 0)
        # ACAC: AC (5, tied strands) at starts 0 and 2, CA ('-' = TG = 3) between: the lowest start
        assert best(S[0], 2, np.array([0, 1, 0, 1]), True) == (5, 0)
        # AA: '+' = 5, '-' (TT) = 3 + 5 = 8: a '-' winner; forward only: 5
        assert best(S[0], 2, np.array([0, 0]), True) == (8, 1)
        assert best(S[0], 2, np.array([0, 0]), False) == (5, 0)


def test_forged_offsets_in_the_model():
    tab = bm.tables(pm.dirichlet_motifs([4, 6], seed=4))
    codes = pm.random_codes(60, seed=5, n_frac=0.0)
    good = np.array([0, 20, 40, 60], dtype=np.int64)
    want = bm.record_best(tab["S"], tab["live"], codes, good)
    for forged in ([0, 20, 10, 60], [0, 20, 40, 61], [-1, 20, 40, 60]):
        got = bm.record_best(tab["S"], tab["live"], codes, np.array(forged, dtype=np.int64))
        assert got[2] == 1
        bad = [r for r in range(3) if not bm.record_ok(forged[r], forged[r + 1], 60)]
        assert bad and np.all(got[1][:, bad] == -1) and np.all(got[0][:, bad] == 0)
        same = [r for r in range(3) if forged[r] == good[r] and forged[r + 1] == good[r + 1]]
        assert np.array_equal(got[0][:, same], want[0][:, same]) and np.array_equal(got[1][:, same], want[1][:, same])
    assert not bm.record_ok(0, 1 << 30, 1 << 31) and bm.record_ok(0, (1 << 30) - 1, 1 << 31)


# ---------------------------------------------------------------- the bridge
def test_bridge_is_exact_for_every_score_and_threshold():
    from explainn_amd import pwmenrich
    isc = np.arange(0, 8194)
    pat = bm.bridge_pattern(isc)
    assert pat.min() == 0x400 and pat.max() == 0x2401             # all normal halves
    thr = bm.bridge_threshold(np.array(BRIDGE_THRESHOLDS))
    assert np.array_equal(thr, pwmenrich.bridge_thresholds(BRIDGE_THRESHOLDS)) and thr.dtype == np.float32
    got = cm.passes(pat[None, :], thr[None, :])[0]                # (scores, thresholds)
    want = isc[:, None] >= np.array(BRIDGE_THRESHOLDS)[None, :]
    assert np.array_equal(got, want)
    # the bridged values are normal halves: finite, increasing with the score, the smallest 2^-14
    v = pat.view(np.float16).astype(np.float64)
    assert np.all(np.diff(v) > 0) and v[0] == 2.0 ** -14
    with pytest.raises(ValueError):
        pwmenrich.bridge_thresholds([8194])
    with pytest.raises(ValueError):
        pwmenrich.bridge_thresholds([-1])


def test_width_groups():
    from explainn_amd import pwmenrich
    lw = np.array([12, 0, 6, 12, 19, 6, 0], dtype=np.int32)
    for groups in (bm.width_groups(lw), pwmenrich.width_groups(lw)):
        assert [w for w, _ in groups] == [6, 12, 19]
        assert [idx.tolist() for _, idx in groups] == [[2, 5], [0, 3], [4]]


# ---------------------------------------------------------------- the ABI
def test_abi_is_bound():
    from explainn_amd import _lib
    assert "explainn_pwm_record_best" in _lib.EXPORTS and len(_lib.SIGNATURES["explainn_pwm_record_best"][1]) == 13
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert int(re.search(r"#define EXPLAINN_PWM_BEST_SPAN (\d+)", text).group(1)) == _lib.PWM_BEST_SPAN
    assert "pwmbest.hip" in open(os.path.join(ROOT, "explainn_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------- the planted case, in the model
@pytest.fixture(scope="module")
def planted():
    mats, primary, control = bm.planted_case()
    return mats, primary, control, bm.enrichment(mats, primary, control), \
        bm.centrality(mats, primary, control, (1e-3,))


def _tab(mats):
    from explainn_amd import pwmenrich
    return pwmenrich._Tables(bm.named(mats), None, 0.1, 100)


def _enrichment_result(mats, e):
    from explainn_amd import enrichment, pwmenrich
    return pwmenrich.enrichment_result([e[f] for f in enrichment._FIELDS], e["counts"], _tab(mats),
                                       e["threshold_pvalue"], e["excluded"])


def _centrality_result(mats, c, pvalues=(1e-3,)):
    from explainn_amd import pwmenrich
    return pwmenrich.MotifCentrality([c[f] for f in cm.FIELDS], c["counts"], pvalues, c["iscore_thresholds"],
                                       _tab(mats), c["length"], int(np.sum(c["labels"] == 2)))


def test_planted_motif_leads_the_model_enrichment(planted):
    mats, primary, control, e, _ = planted
    print("ln p", np.round(e["log_pvalue"], 2), "tp", e["tp"], "fp", e["fp"], "gap", e["gap"])
    assert int(np.argmin(e["log_pvalue"])) == 3 and e["log_pvalue"][3] < -50.0
    assert e["gap"][3] > 1e-6 and np.array_equal(e["counts"], [120, 240]) and e["excluded"] == 0
    res = _enrichment_result(mats, e)
    assert res.qvalue[3] < 0.05 and res.evalue[3] < 1e-10
    assert np.array_equal(res.iscore_threshold, e["best_pattern"])
    assert np.allclose(res.threshold, e["threshold"], rtol=0, atol=0, equal_nan=True)
    assert 0.0 < res.threshold_pvalue[3] < 1e-3                   # a strong cutoff: few random 12-mers reach it
    assert res.threshold[3] > 0.0


def test_planted_motif_is_centred_in_the_model(planted):
    mats, primary, control, _, c = planted
    print("ln p", np.round(c["log_pvalue"], 2), "lo", c["best_lo"], "width", c["best_width"], "gap", c["gap"])
    assert int(np.argmin(c["log_pvalue"])) == 3 and c["log_pvalue"][3] < -50.0 and c["gap"][3] > 1e-6
    lo, width = int(c["best_lo"][3]), int(c["best_width"][3])
    assert lo <= 44 < lo + width and width <= 21                  # around the planted centre, and narrow
    res = _centrality_result(mats, c)
    assert res.qvalue[3] < 0.05
    assert res.region_start[3] == lo and res.region_end[3] == lo + width - 1 + 12 and abs(res.center[3]) <= 1.0
    assert res.starts.tolist() == [100 - w + 1 for w in bm.PLANTED_WIDTHS]
    assert res.iscore_threshold[3] == c["iscore_thresholds"][3, 0] and res.pvalue[3] == 1e-3


def test_tables_from_the_model(planted, tmp_path):
    from explainn_amd import pwmenrich
    mats, primary, control, e, c = planted
    res = _enrichment_result(mats, e)
    rows = pwmenrich.enrichment_rows(res)
    assert len(rows) == 8 and rows[0][:2] == ("MA0003.1", "name3")
    assert [r[9] for r in rows] == sorted(r[9] for r in rows)
    assert rows[0][4] == e["tp"][3] and rows[0][6] == e["fp"][3]
    assert len(pwmenrich.enrichment_rows(res, max_evalue=1e-6)) < 8
    res.save(str(tmp_path / "enr.npz"))
    back = pwmenrich.MotifEnrichment.load(str(tmp_path / "enr.npz"))
    assert pwmenrich.enrichment_rows(back) == rows and back.excluded == res.excluded and back.kernel_size == 19
    fh = io.StringIO()
    pwmenrich.write_enrichment_table(fh, rows)
    lines = fh.getvalue().splitlines()
    assert lines[0].split("\t") == list(pwmenrich.ENRICHMENT_COLUMNS) and len(lines) == 9
    assert lines[1].startswith("MA0003.1\tname3\t") and len(lines[1].split("\t")) == len(pwmenrich.ENRICHMENT_COLUMNS)
    cres = _centrality_result(mats, c)
    crows = pwmenrich.centrality_rows(cres, control=True)
    assert crows[0][:2] == ("MA0003.1", "name3") and len(crows[0]) == len(pwmenrich.CENTRALITY_COLUMNS) + 3
    fh = io.StringIO()
    pwmenrich.write_centrality_table(fh, crows)
    lines = fh.getvalue().splitlines()
    assert lines[0].split("\t")[:3] == ["Motif", "Name", "Threshold"] and lines[0].endswith("LogFisher")
    assert lines[1].startswith("MA0003.1\tname3\t") and len(lines[1].split("\t")) == len(lines[0].split("\t"))
    assert pwmenrich.CENTRALITY_COLUMNS[2:] == __import__("explainn_amd.centrality", fromlist=["x"]).COLUMNS[1:]


def test_motif_best_from_the_model(planted, tmp_path):
    from explainn_amd import pwmenrich
    mats, primary, _, e, _ = planted
    tab = e["tab"]
    isc, start, strand, site = bm.of_records(tab["S"], tab["live"], primary)
    best = pwmenrich.MotifBest.from_device(isc.view(np.uint16).view(np.int16), site, [len(r) for r in primary],
                                           tab["widths"], ["m%d" % i for i in range(8)], tab["scale"], tab["lo"])
    assert np.array_equal(best.start, start) and np.array_equal(best.strand, strand) and best.units == 8
    assert np.array_equal(best.bits, isc.view(np.uint16)) and np.array_equal(best.live_widths, tab["live"])
    want = isc / tab["scale"][:, None] + (tab["widths"] * tab["lo"])[:, None]
    assert np.array_equal(best.score, want) and best.score.dtype == np.float64
    # the planted records hold the consensus: the top score of the motif, w bins at most
    assert best.iscore[3].max() <= 12 * 100 and np.mean(best.iscore[3] == best.iscore[3].max()) >= 0.5
    path = tmp_path / "best.npz"
    best.save(str(path))
    back = pwmenrich.MotifBest.load(str(path))
    for f in ("iscore", "start", "strand", "lengths", "widths", "scale", "lo"):
        assert np.array_equal(getattr(back, f), getattr(best, f)), f
    assert back.names == best.names and back.ids is None
    with pytest.raises(ValueError):
        pwmenrich.MotifBest(isc, start[:, :5], strand, best.lengths, tab["widths"], best.names, tab["scale"], tab["lo"])


def test_empty_motif_in_the_assemblies():
    """An empty motif keeps the "no threshold tried" outputs and is not a row of the centrality table."""
    from explainn_amd import pwmenrich
    mats = pm.dirichlet_motifs([6, 8], seed=7) + [np.full((5, 4), 0.25)]
    g = np.random.default_rng(8)
    primary = [g.integers(0, 4, size=40).astype(np.uint8) for _ in range(30)] + [np.zeros(5, np.uint8)]
    control = [g.integers(0, 4, size=40).astype(np.uint8) for _ in range(20)]
    c = bm.centrality(mats, primary, control, (1e-2, 1e-3))
    assert np.sum(c["labels"] == 2) == 1 and c["length"] == 40
    assert c["n_tests"][2] == 0 and c["best_width"][2] == 0 and c["log_pvalue"][2] == 0.0
    tab = pwmenrich._Tables(mats, None, 0.1, 100)
    res = pwmenrich.MotifCentrality([c[f] for f in cm.FIELDS], c["counts"], (1e-2, 1e-3), c["iscore_thresholds"], tab,
                                      40, 1)
    assert res.qvalue[2] == 1.0 and np.isnan(res.threshold[2]) and np.isnan(res.center[2]) and res.starts[2] == 0
    assert len(pwmenrich.centrality_rows(res)) == 2 and res.excluded == 1
    assert np.array_equal(res.evalue[:2], np.exp(c["log_padj"][:2]) * 2)
    e = bm.enrichment(mats, primary, control)
    assert e["excluded"] == 1 and np.all(e["bits"][2] == 0) and e["n_thresholds"][2] == 1
    eres = pwmenrich.enrichment_result([e[f] for f in __import__("explainn_amd.enrichment", fromlist=["x"])._FIELDS],
                                       e["counts"], tab, e["threshold_pvalue"], e["excluded"])
    assert np.isnan(eres.threshold[2]) and eres.threshold_pvalue[2] == 0.0 and eres.excluded == 1
