"""CPU: the fp64 model of motif enrichment (tests/enrichment_model.py) against brute force and scipy, and the
host logic of explainn_amd.enrichment that needs no device.

test_logsf_matches_scipy measures the model's hypergeometric tail against scipy.stats.hypergeom.logsf and
holds it to enrichment_model.LOGSF_DEVIATION, the yardstick of tests/test_gpu_enrichment.py."""
import math
import os
import re

import numpy as np
import pytest

import enrichment_model as em
import sites_model as sm
from oracle import explainn_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- best sites
def test_best_site_vectorised_equals_brute_force_with_ties():
    g = np.random.default_rng(0)
    for trial in range(20):
        U, P = 4, int(g.integers(1, 40))
        # few distinct values: ties between starts and between strands are the rule
        f = g.integers(0, 4, size=(U, P)).astype(np.float16)
        r = g.integers(0, 4, size=(U, P)).astype(np.float16)
        for rev in (r, None):
            a, b = em.best_brute(f, rev), em.best_of_acts(f, rev)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    f = np.array([[1, 3, 3, 2], [0, 0, 0, 0], [np.inf, 1, np.inf, 0]], dtype=np.float16)
    r = np.array([[3, 3, 0, 0], [0, 0, 0, 0], [0, np.inf, 0, 0]], dtype=np.float16)
    bits, site = em.best_of_acts(f, r)
    assert list(site) == [(0 << 1) | 1, 0, 0]            # '-' at the lower start beats '+' later; all-equal: 0, '+'
    assert list(bits) == [0x4200, 0, 0x7C00]
    bits, site = em.best_of_acts(f, None)
    assert list(site) == [1 << 1, 0, 0]
    bits, site = em.best_of_acts(np.zeros((2, 0), np.float16))
    assert list(bits) == [0, 0] and list(site) == [-1, -1]


def test_record_best_on_kmer_activations():
    """Records of lengths around k on a real filter bank: short records have no site, a palindrome ties the
    strands, and the reverse strand is the forward strand of the reverse complement, mapped back."""
    U, k = 3, 6
    sd = orc.random_state_dict(U, k, 40, 1, seed=3)
    acts = lambda c, rev: sm.kmer_acts(sd, c, reverse=rev)
    g = np.random.default_rng(1)
    pal = g.integers(0, 4, size=10).astype(np.uint8)
    pal = np.concatenate([pal, sm.rc_codes(pal)])
    recs = [g.integers(0, 4, size=n).astype(np.uint8) for n in (k - 1, k, k + 1, 0, 33)] + [pal]
    codes = np.concatenate(recs)
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    bits, site = em.record_best(acts, codes, off, k)
    assert bits.shape == (U, len(recs))
    assert np.all(bits[:, [0, 3]] == 0) and np.all(site[:, [0, 3]] == -1)
    assert np.all(site[:, 1] >> 1 == 0)
    for r, rec in enumerate(recs):
        if len(rec) < k:
            continue
        f, v = acts(rec, False), acts(rec, True)
        assert np.array_equal(v, acts(sm.rc_codes(rec), False)[:, ::-1])
        want = em.best_brute(f, v)
        assert np.array_equal(bits[:, r], want[0]) and np.array_equal(site[:, r], want[1])
    # the palindrome: the reverse strand holds the forward strand's values mirrored, so the maximum is on both
    f, v = acts(pal, False), acts(pal, True)
    assert np.array_equal(f, v[:, ::-1]) and np.array_equal(bits[:, -1], em.to_bits(f).max(axis=1))
    fwd_only, _ = em.record_best(acts, codes, off, k, both=False)
    assert np.all(fwd_only <= bits) and np.any(fwd_only < bits)
    bad = off.copy()
    bad[2], bad[3] = off[3], off[2]                      # a descending pair: record 2 reads as empty
    b2, s2 = em.record_best(acts, codes, bad, k)
    assert np.all(b2[:, 2] == 0) and np.all(s2[:, 2] == -1) and np.array_equal(b2[:, 4:], bits[:, 4:])


# ------------------------------------------------------------------------------------------- the test
def _cases():
    out = {"half_normal_%d" % s: em.half_normal_case(seed=s) for s in range(5)}
    out.update(em.synthetic_cases())
    out["many_units"] = em.many_units_case()
    return out


def test_tails_thresholds_counts_and_u2_against_brute_force():
    for name, (bits, labels) in _cases().items():
        for col in bits:
            st = em.unit_stats(col, labels)
            inc = np.isin(labels, (0, 1))
            held = np.unique(col[inc].astype(np.int64) & 0x7FFF)
            assert np.array_equal(st["thresholds"], held), name
            assert st["n_thresholds"] == len(held)
            for t in list(held[:5]) + list(held[-5:]) + [0, 1, 0x7C00, 0x7FFF]:
                assert (st["a"][t], st["b"][t]) == em.brute_counts(col, labels, t), (name, t)
            assert (st["tp"], st["fp"]) == em.brute_counts(col, labels, st["best_pattern"])
            assert st["u2"] == em.brute_u2(col, labels), name
            assert (st["Np"], st["Nc"]) == (int(np.sum(labels == 1)), int(np.sum(labels == 0)))


def test_auroc_matches_mannwhitneyu():
    stats = pytest.importorskip("scipy.stats")
    for seed in range(3):
        bits, labels = em.half_normal_case(seed=seed)
        for col in bits:
            st = em.unit_stats(col, labels)
            x = col.view(np.float16).astype(np.float64)
            u = stats.mannwhitneyu(x[labels == 1], x[labels == 0]).statistic
            assert st["auroc"] == pytest.approx(u / (st["Np"] * st["Nc"]), rel=1e-14)
            assert st["auroc"] == st["u2"] / (2.0 * st["Np"] * st["Nc"])


def logsf_grid(N):
    """Enriched (a, n, Np, Nc) around and far above the mean, over several shapes of the 2 x 2 table."""
    out = set()
    shapes = [(fp, fn) for fp in (0.05, 0.4, 0.5, 0.9) for fn in (0.01, 0.1, 0.5, 0.97)]
    if N > 10 ** 5:
        shapes = [(0.05, 0.01), (0.4, 0.01), (0.5, 0.1), (0.9, 0.01)]        # the term count grows with sd
    for fp, fn in shapes:
        Np = max(1, int(round(fp * N)))
        Nc, n = N - Np, max(1, int(round(fn * N)))
        if Nc < 1:
            continue
        mean = n * Np / N
        sd = math.sqrt(max(n * (Np / N) * (1 - Np / N) * (N - n) / max(N - 1, 1), 1e-12))
        for z in (0, 0.5, 1, 3, 6, 10, 20, 50):
            for j in (0, 1):
                a = min(max(int(math.floor(mean)) + 1 + int(round(z * sd)) + j, max(0, n - Nc)), min(Np, n))
                if a * N > n * Np:
                    out.add((a, n, Np, Nc))
    return sorted(out)


def test_logsf_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    for N, bound in em.LOGSF_DEVIATION.items():
        worst, terms = 0.0, 0
        for a, n, Np, Nc in logsf_grid(N):
            ref = float(stats.hypergeom.logsf(a - 1, N, Np, n))
            got, t = em.hypergeom_logsf(a, n, Np, Nc, return_terms=True)
            worst, terms = max(worst, abs(got - ref)), max(terms, t)
        print("N = %d: largest |ln p - scipy| = %.3g over %d points, at most %d terms" % (
            N, worst, len(logsf_grid(N)), terms))
        assert len(logsf_grid(N)) >= 20
        assert worst <= bound, N
    assert em.deviation(150) == em.LOGSF_DEVIATION[400] and em.deviation(5002) == em.LOGSF_DEVIATION[40000]
    assert em.log_tolerance(150) >= 64 * np.spacing(math.lgamma(151.0))


def test_pvalue_is_fishers_exact_at_the_best_threshold():
    stats = pytest.importorskip("scipy.stats")
    for seed in range(3):
        bits, labels = em.half_normal_case(seed=seed)
        for col in bits:
            st = em.unit_stats(col, labels)
            a, b = st["tp"], st["fp"]
            p = stats.fisher_exact([[a, st["Np"] - a], [b, st["Nc"] - b]], alternative="greater")[1]
            if st["log_pvalue"] < 0:
                assert math.exp(st["log_pvalue"]) == pytest.approx(p, rel=1e-11)
            # the best threshold is the best: no held threshold has a smaller Fisher p
            assert st["log_pvalue"] == st["logp"].min()
    # not enriched: p = 1 by rule, whatever Fisher says
    assert em.logp(3, 10, 50, 50) == 0.0 and em.logp(5, 5, 50, 50) == 0.0 and em.logp(6, 5, 50, 50) < 0.0


def test_log_padj_branches_agree_at_the_seam():
    for m in (1, 2, 50, 3000, 32768):
        for lp in (-30.0, -30.000001, -29.999999, -35.0):
            full, short = em.log_padj(lp, m, "full"), em.log_padj(lp, m, "short")
            # ln(1 - (1-p)^m) = ln(m p) + ln(1 - (m-1) p / 2 + ...): the forms differ by (m-1) p / 2 at the most
            assert abs(full - short) <= 0.5 * m * math.exp(lp) + 4 * np.spacing(abs(short)), (m, lp)
            if m <= 50:
                assert abs(full - short) <= 1e-13 * abs(short)
    assert em.log_padj(-31.0, 7) == em.log_padj(-31.0, 7, "short")
    assert em.log_padj(-29.0, 7) == em.log_padj(-29.0, 7, "full")
    assert em.log_padj(0.0, 9) == 0.0 and em.log_padj(-5.0, 0) == 0.0
    assert em.log_padj(math.log(0.01), 1) == pytest.approx(math.log(0.01), rel=1e-13)
    assert em.log_padj(math.log(0.5), 2) == pytest.approx(math.log(0.75), rel=1e-13)


def test_gaps_of_the_inputs_the_gpu_test_reuses():
    """The GPU test demands best_pattern, tp and fp exactly: every unit's best logp must stand clear of its
    runner-up by more than MIN_GAP on every input it reuses (it asserts the same on the device's own bits)."""
    smallest = np.inf
    for name, (bits, labels) in _cases().items():
        gaps = em.test_stats(bits, labels)["gap"]
        assert np.all(gaps > em.MIN_GAP), (name, gaps)
        smallest = min(smallest, gaps.min())
    bits, labels = kmer_case()
    gaps = em.test_stats(bits, labels)["gap"]
    assert np.all(gaps > em.MIN_GAP), gaps
    print("smallest gap between the best and the runner-up logp: %.3g" % min(smallest, gaps.min()))


def kmer_case(n_primary=2000, n_control=3000, L=40, U=3, k=8, seed=11):
    """The 2000 + 3000 case on the host: 40-base records scored by a filter bank through sites_model.kmer_acts
    (the GPU test scores the same records on the device)."""
    sd = orc.random_state_dict(U, k, L, 1, seed=seed)
    codes = kmer_records(n_primary, n_control, L, sd, k, seed)
    bits = np.zeros((U, len(codes)), dtype=np.uint16)
    for r, c in enumerate(codes):
        bits[:, r] = em.best_of_acts(sm.kmer_acts(sd, c), sm.kmer_acts(sd, c, reverse=True))[0]
    return bits, em_labels(n_primary, n_control)


def em_labels(n_primary, n_control):
    return np.concatenate([np.ones(n_primary, np.uint8), np.zeros(n_control, np.uint8)])


def kmer_records(n_primary, n_control, L, sd, k, seed):
    """Random records; a third of the primary ones carry the k-mer that unit 0's taps like best."""
    g = np.random.default_rng(seed)
    codes = [g.integers(0, 4, size=L).astype(np.uint8) for _ in range(n_primary + n_control)]
    w = np.asarray(sd["linears.0.weight"])[0]                                # (4, k)
    a = float(np.asarray(sd["linears.1.weight"])[0])
    kmer = (np.argmax(w, axis=0) if a > 0 else np.argmin(w, axis=0)).astype(np.uint8)
    for r in range(0, n_primary, 3):
        p = int(g.integers(0, L - k + 1))
        codes[r][p:p + k] = kmer
    return codes


# ------------------------------------------------------------------------------------------- host logic
def _result(units=5, seed=0):
    from explainn_amd.enrichment import Enrichment
    g = np.random.default_rng(seed)
    lp = -np.abs(g.standard_normal(units)) * 10
    lp[1] = lp[3]                                       # a tie: the lower filter comes first
    m = g.integers(1, 50, size=units)
    return Enrichment(m, g.integers(0x3000, 0x4000, size=units), g.integers(0, 60, size=units),
                      g.integers(0, 90, size=units), lp, [em.log_padj(x, int(k)) for x, k in zip(lp, m)],
                      g.integers(0, 60 * 90 * 2, size=units), g.random(units), [60, 90], 19, "both", 2, 7)


def test_table_rows_order_and_columns():
    from explainn_amd import enrichment as en
    res = _result()
    rows = en.table_rows(res)
    assert [r[0] for r in rows] == sorted(range(5), key=lambda u: (res.log_pvalue[u], u))
    assert [r[0] for r in rows].index(1) + 1 == [r[0] for r in rows].index(3)
    u = rows[0][0]
    assert rows[0][1] == float(np.array(res.best_pattern[u], np.uint16).view(np.float16))
    assert rows[0][3] == pytest.approx(100.0 * res.tp[u] / 60) and rows[0][5] == pytest.approx(100.0 * res.fp[u] / 90)
    assert rows[0][6] == pytest.approx(((res.tp[u] + 1) / 61) / ((res.fp[u] + 1) / 91))
    assert rows[0][9] == pytest.approx(math.exp(res.log_padj[u]) * 5)
    q = __import__("spacing_model").benjamini_hochberg(np.exp(res.log_pvalue))
    assert np.allclose(res.qvalue, q, rtol=1e-12, atol=0)
    kept = en.table_rows(res, max_evalue=float(np.median(res.evalue)))
    assert 0 < len(kept) < 5 and all(r[9] <= np.median(res.evalue) for r in kept)

    class Sink(list):
        write = list.append
    out = Sink()
    en.write_table(out, rows)
    assert out[0] == "\t".join(en.COLUMNS) + "\n" and len(out) == 6
    assert out[1].startswith("filter%d\t" % u) and out[1].count("\t") == len(en.COLUMNS) - 1
    assert en.COLUMNS == ("Filter", "Threshold", "TP", "TPpct", "FP", "FPpct", "Enrichment", "LogPvalue", "LogPadj",
                          "Evalue", "Qvalue", "AUROC")


def test_labels_chunks_and_record_forms():
    from explainn_amd import enrichment as en
    lab = en.record_labels([19, 18, 40], [5, 19], 19)
    assert list(lab) == [1, 2, 1, 2, 0]
    assert en.record_chunks([10, 10, 10, 35, 5], 20) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert en.record_chunks([10, 10, 10], 1000) == [(0, 3)] and en.record_chunks([], 5) == []
    assert en.record_chunks([0, 0, 3], 2) == [(0, 2), (2, 3)]
    with pytest.raises(ValueError, match="chunk_bases"):
        en.record_chunks([3], 0)
    ids, codes = en.record_codes([("a", np.zeros(3, np.uint8)), np.ones(2, np.uint8)])
    assert ids == ["a", "1"] and [len(c) for c in codes] == [3, 2]
    with pytest.raises(ValueError, match="uint8"):
        en.record_codes([np.zeros(3, np.int64)])
    rb = en.RecordBest.from_device(np.array([[0x3C00, 0]], np.int16), np.array([[(7 << 1) | 1, -1]], np.int32), [30, 2], 19)
    assert rb.score[0, 0] == 1.0 and list(rb.start[0]) == [7, -1] and list(rb.strand[0]) == [-1, 0]
    assert rb.bits.dtype == np.uint16 and rb.bits[0, 0] == 0x3C00


def test_ragged_records_without_a_control_raise():
    from explainn_amd import ExplaiNN, enrichment as en
    model = ExplaiNN(4, 19, 200, 1).eval()
    recs = [np.zeros(40, np.uint8), np.zeros(41, np.uint8)]
    with pytest.raises(ValueError, match="one length"):
        en.enrichment(model, recs)
    with pytest.raises(ValueError, match="strands"):
        en.enrichment(model, recs, recs, strands="rev")
    with pytest.raises(ValueError, match="shuffles"):
        en.enrichment(model, recs[:1], shuffles=0)
    with pytest.raises(ValueError, match="no primary"):
        en.enrichment(model, [], recs)


def test_cli_parser():
    from explainn_amd import enrichment as en
    a = en._parser().parse_args(["m.pth", "p.fa", "-o", "out.tsv"])
    assert (a.control, a.shuffles, a.seed, a.strands, a.max_evalue, a.save_best) == (None, 1, 0, "both", 10.0, None)
    a = en._parser().parse_args(["m.pth", "p.fa", "--control", "c.fa", "--strands", "fwd", "--max-evalue", "0.5",
                                 "--save-best", "b.npz", "--shuffles", "3", "--seed", "9", "-o", "o.tsv"])
    assert (a.control, a.shuffles, a.seed, a.strands, a.max_evalue, a.save_best, a.output_file) == (
        "c.fa", 3, 9, "fwd", 0.5, "b.npz", "o.tsv")
    with pytest.raises(SystemExit):
        en._parser().parse_args(["m.pth", "p.fa"])


def test_save_and_load(tmp_path):
    from explainn_amd import enrichment as en
    res = _result(seed=2)
    res.save(tmp_path / "e.npz")
    back = en.Enrichment.load(tmp_path / "e.npz")
    for f in en._FIELDS + ("counts", "threshold", "enrichment", "evalue", "qvalue"):
        assert np.array_equal(getattr(back, f), getattr(res, f)), f
    assert (back.kernel_size, back.strands, back.shuffles, back.seed) == (19, "both", 2, 7)
    rb = en.RecordBest(np.array([[1.5, 0]], np.float16), [[3, -1]], [[1, 0]], [25, 4], 19, ids=["x", "y"])
    rb.save(tmp_path / "b.npz")
    b2 = en.RecordBest.load(tmp_path / "b.npz")
    assert np.array_equal(b2.score, rb.score) and np.array_equal(b2.start, rb.start) and b2.ids == ["x", "y"]
    assert np.array_equal(b2.strand, rb.strand) and np.array_equal(b2.lengths, rb.lengths) and b2.kernel_size == 19


def test_constants_agree_with_the_header():
    from explainn_amd import _lib
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert int(re.search(r"#define EXPLAINN_BEST_SPAN (\d+)", text).group(1)) == _lib.BEST_SPAN
    assert _lib.ACT_BINS == em.BINS
