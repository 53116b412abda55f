"""GPU: known-motif enrichment and centrality (csrc/pwmbest.hip through explainn_pwm_record_best,
explainn_amd/pwmenrich.py and `python -m explainn_amd.pwmenrich`) against the numpy model
tests/pwmbest_model.py.  Scores, sites, flags, counts, thresholds and regions are compared exactly
(array_equal); the log values of the two tests within enrichment_model.log_tolerance /
centrality_model.log_tolerance, and the chosen threshold / region exactly where the model's `gap` (best to
runner-up) is above MIN_GAP."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import centrality_model as cm  # noqa: E402
import enrichment_model as em  # noqa: E402
import pwmbest_model as bm  # noqa: E402
import pwmsites_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7


def _lib():
    from explainn_amd import _lib
    return _lib


def _span():
    return _lib().PWM_BEST_SPAN


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _offsets(recs):
    off = np.zeros(len(recs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in recs], out=off[1:])
    return off


def _flat(recs):
    return np.concatenate(list(recs) + [np.full(1, 4, np.uint8)]).astype(np.uint8)      # never an empty buffer


def _call(S, lw, codes, offsets, both=True, want_site=True, seq_len=None, want_flags=True):
    """One explainn_pwm_record_best call on host arrays: (bits uint16 (M,R), site int32 (M,R) or None, flags)."""
    lib = _lib()
    M, wmax, R = S.shape[0], S.shape[1], len(offsets) - 1
    Sd, wd, cd, od = _dev(S), _dev(np.asarray(lw, dtype=np.int32)), _dev(codes), _dev(np.asarray(offsets, dtype=np.int64))
    bits = torch.full((M, R), SENTINEL, dtype=torch.int16, device="cuda")
    site = torch.full((M, R), SENTINEL, dtype=torch.int32, device="cuda") if want_site else None
    flags = torch.zeros(1, dtype=torch.int32, device="cuda") if want_flags else None
    lib.check(lib.load().explainn_pwm_record_best(
        cd.data_ptr(), len(codes) if seq_len is None else seq_len, od.data_ptr(), R, int(both), Sd.data_ptr(),
        wd.data_ptr(), M, wmax, bits.data_ptr(), site.data_ptr() if want_site else None,
        flags.data_ptr() if want_flags else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return (bits.cpu().numpy().view(np.uint16), site.cpu().numpy() if want_site else None,
            int(flags.item()) if want_flags else None)


def _check(S, lw, recs, both=True):
    """bits, site and flag equal the model's on a list of records; returns (bits, site)."""
    codes, off = _flat(recs), _offsets(recs)
    want_bits, want_site, want_flag = bm.record_best(S, lw, codes, off, both)
    bits, site, flag = _call(S, lw, codes, off, both)
    assert np.array_equal(bits, want_bits) and np.array_equal(site, want_site) and flag == want_flag == 0
    return bits, site


def _tables(widths, seed, extra=()):
    tab = bm.tables(pm.dirichlet_motifs(widths, seed) + list(extra))
    return tab["S"], tab["live"]


def _palindrome(w=8, seed=3):
    half = np.random.default_rng(seed).dirichlet(np.full(4, 0.3), size=w // 2)
    return np.concatenate([half, half[::-1, ::-1]])


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
@pytest.mark.parametrize("n", ["SPAN-1", "SPAN", "SPAN+1", "2*SPAN+3"])
def test_start_counts_around_the_span(n, both):
    n = eval(n, {"SPAN": _span()})
    S, lw = _tables([1, 6, 19, 64], seed=1)
    # n starts for each width in turn, and a short neighbour between them
    recs = [pm.random_codes(n + w - 1, seed=n + w) for w in (1, 6, 19, 64)] + [pm.random_codes(70, seed=n)]
    bits, site = _check(S, lw, recs, both)
    assert np.all(site[:3, :] >= 0) and bits.max() > 0
    if both:
        assert np.any(site & 1 == 1) and np.any(site & 1 == 0)
    else:
        assert np.all(site[site >= 0] & 1 == 0)


@pytest.mark.parametrize("M", ["1", "GROUP", "GROUP+1"])
def test_motif_counts_around_the_group(M):
    M = eval(M, {"GROUP": _lib().PWM_GROUP})
    widths = list(np.random.default_rng(M).integers(4, 13, size=M))
    S, lw = _tables(widths, seed=7)
    recs = [pm.random_codes(int(n), seed=int(n)) for n in (300, 40, 11, 257, 5)]
    bits, site = _check(S, lw, recs)
    assert np.all(site[:, 0] >= 0) and np.all(bits[:, 0] > 0)


@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
def test_widths_and_record_edges(both):
    """Widths 0, 1, 6, 19, 64 and one past wmax; records that are empty, shorter than w, exactly w, or all N."""
    S, lw = _tables([8, 1, 6, 19, 64, 9], seed=2)
    lw = lw.copy()
    lw[0], lw[5] = 0, 65                                          # width 0; a width past wmax = 64: both empty
    recs = [np.zeros(0, np.uint8), np.full(40, 4, np.uint8)]
    recs += [pm.random_codes(n, seed=n, n_frac=0.0) for n in (1, 5, 6, 18, 19, 63, 64, 65)]
    bits, site = _check(S, lw, recs, both)
    assert np.all(site[[0, 5]] == -1) and np.all(bits[[0, 5]] == 0)
    assert np.all(site[:, :2] == -1)                              # the empty and the all-N record
    for m, w in ((1, 1), (2, 6), (3, 19), (4, 64)):
        for r, rec in enumerate(recs[2:], start=2):
            assert (site[m, r] >= 0) == (len(rec) >= w), (m, r)
            if len(rec) == w:
                assert site[m, r] >> 1 == 0


def test_n_runs_across_a_pass_and_bytes_above_four():
    span = _span()
    S, lw = _tables([6, 19, 12, 7], seed=3)
    long = pm.random_codes(2 * span + 90, seed=4, n_frac=0.0)
    long[span - 5:span + 8] = 4                                   # an N run across the pass boundary
    long[[20, span + 40, 2 * span + 10]] = [5, 255, 9]            # bytes above 4 read as N
    holes = pm.random_codes(span + 30, seed=5, n_frac=0.0)
    holes[np.arange(3, span + 30, 5)] = 4                         # an N every 5 bases: only width <= 4 would fit
    edge = pm.random_codes(span + 18, seed=6, n_frac=0.0)
    edge[span:] = 4                                               # live starts end before the pass does
    bits, site = _check(S, lw, [long, holes, edge, long[::-1].copy()])
    assert np.all(site[:, 1] == -1) and np.all(site[:, [0, 2, 3]] >= 0)


def test_tie_rules_palindrome_and_flat_region():
    S, lw = _tables([6, 9], seed=8, extra=[_palindrome(8), _palindrome(12, seed=4)])
    span = _span()
    recs = [np.zeros(span + 50, np.uint8), np.full(2 * span + 7, 2, np.uint8), pm.random_codes(300, seed=9, n_frac=0.0),
            np.tile(np.array([0, 3], np.uint8), span)]            # poly-A, poly-G, random, (AT)n
    bits, site = _check(S, lw, recs)
    assert np.all(site[:, :2] >> 1 == 0)                          # a flat region: the lowest start
    assert np.all(site[2:] & 1 == 0)                              # a palindrome: '+' wins the tie at every start
    assert np.all(site[:, 3] >> 1 <= 1)                           # period 2: the first or the second start


def test_more_records_than_the_grid_has_slices():
    """One motif group: the call has at most 16384 workgroups of four waves, so 66000 records make the waves of
    some workgroups take a second record."""
    S, lw = _tables([4, 7], seed=10)
    rows = pm.random_codes(66000 * 12, seed=11, n_frac=0.02).reshape(66000, 12)
    want_bits, want_site = bm.record_best_equal(S, lw, rows)
    for both in (True, False):
        if not both:
            want_bits, want_site = bm.record_best_equal(S, lw, rows, both=False)
        bits, site, flag = _call(S, lw, rows.reshape(-1), np.arange(66001, dtype=np.int64) * 12, both)
        assert np.array_equal(bits, want_bits) and np.array_equal(site, want_site) and flag == 0
    assert np.mean(site[0] >= 0) > 0.9 and np.any(site[1] == -1)


def test_null_site_null_flags_and_repeatability():
    S, lw = _tables([6, 10, 15], seed=12)
    recs = [pm.random_codes(int(n), seed=int(n)) for n in (100, 256, 300, 9, 700)]
    codes, off = _flat(recs), _offsets(recs)
    a, b = _call(S, lw, codes, off), _call(S, lw, codes, off)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    only, none, noflag = _call(S, lw, codes, off, want_site=False, want_flags=False)
    assert np.array_equal(only, a[0]) and none is None and noflag is None
    assert np.array_equal(a[0], bm.record_best(S, lw, codes, off)[0])


def test_forged_offsets_set_the_flag_and_stay_inside():
    S, lw = _tables([6, 10], seed=13)
    codes = pm.random_codes(400, seed=14, n_frac=0.0)
    good = np.array([0, 100, 200, 300, 400], dtype=np.int64)
    want = bm.record_best(S, lw, codes, good)
    for forged in ([0, 100, 50, 300, 400], [0, 100, 200, 300, 401], [-1, 100, 200, 300, 400],
                   [0, 100, 200, 1 << 40, 400], [0, -(1 << 40), 200, 300, 400]):
        forged = np.array(forged, dtype=np.int64)
        model = bm.record_best(S, lw, codes, forged)
        bits, site, flag = _call(S, lw, codes, forged)
        assert flag == model[2] == 1
        assert np.array_equal(bits, model[0]) and np.array_equal(site, model[1])
        bad = [r for r in range(4) if not bm.record_ok(int(forged[r]), int(forged[r + 1]), 400)]
        assert bad and np.all(site[:, bad] == -1) and np.all(bits[:, bad] == 0)
        same = [r for r in range(4) if forged[r] == good[r] and forged[r + 1] == good[r + 1]]
        assert same and np.array_equal(bits[:, same], want[0][:, same]) and np.array_equal(site[:, same], want[1][:, same])
    # a record of 2^30 bases has no int32 site word: refused by a compare, whatever seq_len claims
    # (every other record of the call lies inside the real buffer)
    huge = np.array([0, 100, 100 + (1 << 30)], dtype=np.int64)
    bits, site, flag = _call(S, lw, codes, huge, seq_len=1 << 31)
    assert flag == 1 and np.all(site[:, 1] == -1) and np.all(bits[:, 1] == 0)
    assert np.array_equal(site[:, 0], want[1][:, 0]) and np.array_equal(bits[:, 0], want[0][:, 0])
    # the flag is ORed into, never cleared; with flags == NULL the outputs are the same
    bits2, site2, _ = _call(S, lw, codes, np.array([0, 100, 50, 300, 400], dtype=np.int64), want_flags=False)
    assert np.all(site2[:, 1] == -1) and np.array_equal(site2[:, [0, 3]], want[1][:, [0, 3]])


def test_argument_errors_and_empty_calls():
    lib = _lib()
    L = lib.load()
    S, lw = _tables([6, 9], seed=15)
    codes = pm.random_codes(100, seed=16)
    Sd, wd, cd, od = _dev(S), _dev(lw), _dev(codes), _dev(np.array([0, 50, 100], dtype=np.int64))
    bits = torch.full((2, 2), SENTINEL, dtype=torch.int16, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(seq_len=100, R=2, M=2, wmax=9):
        return L.explainn_pwm_record_best(cd.data_ptr(), seq_len, od.data_ptr(), R, 1, Sd.data_ptr(), wd.data_ptr(), M,
                                          wmax, bits.data_ptr(), None, None, stream)

    for bad in (dict(seq_len=-1), dict(R=-1), dict(R=1 << 31), dict(M=-1), dict(M=65535 * lib.PWM_GROUP + 1),
                dict(wmax=0), dict(wmax=65)):
        assert call(**bad) == lib.E_ARG, bad
        assert b"pwm_record_best" in L.explainn_last_error()
    assert call(M=0) == lib.OK and call(R=0) == lib.OK
    torch.cuda.synchronize()
    assert np.all(bits.cpu().numpy() == SENTINEL)                 # nothing was launched
    assert call() == lib.OK
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy().view(np.uint16), bm.record_best(S, lw, codes, [0, 50, 100])[0])


# ---------------------------------------------------------------- best_motif_sites
def _mixed_records(seed, n=60):
    g = np.random.default_rng(seed)
    return [("rec%d" % i, pm.random_codes(int(L), seed=seed + i)) for i, L in enumerate(g.integers(0, 330, size=n))]


def test_best_motif_sites_chunking_and_device_codes():
    from explainn_amd import pwmenrich
    mats = pm.dirichlet_motifs([6, 12, 9, 20], seed=30, alpha=0.2) + [np.full((5, 4), 0.25)]
    recs = _mixed_records(31)
    tab = bm.tables(mats)
    isc, start, strand, _ = bm.of_records(tab["S"], tab["live"], [c for _, c in recs])
    best = pwmenrich.best_motif_sites(bm.named(mats), recs)
    assert np.array_equal(best.iscore, isc) and np.array_equal(best.start, start) and np.array_equal(best.strand, strand)
    assert best.ids == [r[0] for r in recs] and best.names == ["MA%04d.1" % i for i in range(5)]
    assert np.array_equal(best.lengths, [len(c) for _, c in recs]) and np.all(best.start[4] == -1)
    ok = best.start[:4] >= 0
    want = isc[:4] / tab["scale"][:4, None] + (tab["widths"] * tab["lo"])[:4, None]
    assert np.array_equal(best.score[:4][ok], want[ok]) and np.all(np.isnan(best.score[:4][~ok]))
    small = pwmenrich.best_motif_sites(mats, recs, chunk_bases=500)
    on_device = pwmenrich.best_motif_sites(mats, [torch.from_numpy(c).cuda() for _, c in recs], chunk_bases=1777)
    for other in (small, on_device):
        for f in ("iscore", "start", "strand", "lengths"):
            assert np.array_equal(getattr(other, f), getattr(best, f)), f
    fwd = pwmenrich.best_motif_sites(mats, recs, strands="fwd")
    want_fwd = bm.of_records(tab["S"], tab["live"], [c for _, c in recs], both=False)
    assert np.array_equal(fwd.iscore, want_fwd[0]) and np.array_equal(fwd.start, want_fwd[1]) and np.all(fwd.strand >= 0)


def test_best_site_is_the_strongest_site_scan_motifs_lists():
    from explainn_amd import pwmenrich, pwmsites
    mats = pm.dirichlet_motifs([6, 12, 9], seed=32, alpha=0.2)
    recs = [pm.random_codes(n, seed=n, n_frac=0.01) for n in (150, 40, 260)]
    best = pwmenrich.best_motif_sites(mats, recs)
    for r, rec in enumerate(recs):
        calls = pwmsites.scan_motifs(mats, rec, pvalue=1.0)       # every live (start, strand)
        for m in range(3):
            start, strand, _ = calls.unit(m)
            isc = calls.iscore[calls.offsets[m]:calls.offsets[m + 1]]
            top = isc.max()
            first = np.lexsort((-strand[isc == top], start[isc == top]))[0]
            assert best.iscore[m, r] == top and best.start[m, r] == start[isc == top][first]
            assert best.strand[m, r] == strand[isc == top][first]


# ---------------------------------------------------------------- enrichment
def _assert_enrichment(res, want, n_records):
    for f in ("n_thresholds", "best_pattern", "tp", "fp", "u2", "counts"):
        assert np.array_equal(getattr(res, f), want[f]), f
    tol = em.log_tolerance(n_records)
    for f in ("log_pvalue", "log_padj"):
        worst = float(np.max(np.abs(getattr(res, f) - want[f])))
        print("%s: largest |device - model| = %.3g (allowed %.3g)" % (f, worst, tol))
        assert worst <= tol, f
    assert np.array_equal(res.auroc, want["u2"] / (2.0 * want["counts"][0] * want["counts"][1]))
    assert np.array_equal(res.threshold, want["threshold"], equal_nan=True) and res.excluded == want["excluded"]


def test_motif_enrichment_equals_the_model():
    from explainn_amd import pwmenrich, pwmsites
    mats = pm.dirichlet_motifs([6, 12, 9, 12], seed=33, alpha=0.2) + [np.full((5, 4), 0.25)]
    g = np.random.default_rng(34)
    primary = [pm.random_codes(60, seed=100 + i, n_frac=0.01) for i in range(70)] + [np.zeros(8, np.uint8)]
    control = [pm.random_codes(int(n), seed=300 + i, n_frac=0.01) for i, n in enumerate(g.integers(12, 90, size=110))]
    for i in range(0, 70, 2):
        pm.plant(primary[i], mats[1], 10 + i % 30, reverse=bool(i % 4))
    want = bm.enrichment(mats, primary, control)
    assert np.all(want["gap"][:4] > em.MIN_GAP), want["gap"]             # the chosen thresholds are then owed exactly
    assert want["excluded"] == 1 and int(np.argmin(want["log_pvalue"])) == 1
    res = pwmenrich.motif_enrichment(bm.named(mats), primary, control, chunk_bases=1500)
    _assert_enrichment(res, want, len(primary) + len(control))
    # the per-site p-value at the chosen cutoff: bit-equal to the device's own tail table, gathered
    null = pwmsites.score_null(mats, pvalue=1.0)
    tail = null.tail.cpu().numpy()
    assert np.array_equal(res.threshold_pvalue, tail[np.arange(5), res.best_pattern])
    live = want["tail"][np.arange(5), want["best_pattern"]] > 0
    assert np.all(np.abs(res.threshold_pvalue[live] / want["threshold_pvalue"][live] - 1.0) <= 1e-10)
    assert res.threshold_pvalue[4] == 0.0 and res.ids[1] == "MA0001.1" and res.names[1] == "name1"
    assert np.array_equal(res.qvalue <= 1.0, np.ones(5, bool)) and res.evalue[1] == np.exp(res.log_padj[1]) * 5


def test_shuffled_control_depends_on_the_seed():
    from explainn_amd import pwmenrich
    from explainn_amd.sequence import dinucleotide_shuffle_device
    mats, primary, _ = bm.planted_case()
    a = pwmenrich.motif_enrichment(mats, primary, shuffles=2, seed=0)
    again = pwmenrich.motif_enrichment(mats, primary, shuffles=2, seed=0, chunk_bases=2100)
    b = pwmenrich.motif_enrichment(mats, primary, shuffles=2, seed=1)
    assert np.array_equal(a.counts, [120, 240]) and a.shuffles == 2
    for f in ("fp", "u2", "tp", "best_pattern", "log_pvalue"):
        assert np.array_equal(getattr(a, f), getattr(again, f)), f
    assert not (np.array_equal(a.fp, b.fp) and np.array_equal(a.u2, b.u2))
    assert int(np.argmin(a.log_pvalue)) == 3 and a.log_pvalue[3] < -50.0
    # the control columns are the shuffles the shuffle entry point draws
    shuf = dinucleotide_shuffle_device(torch.from_numpy(np.stack(primary)).cuda(), 2, 0).reshape(-1, 100).cpu().numpy()
    want = bm.enrichment(mats, primary, list(shuf))
    for f in ("tp", "fp", "u2", "best_pattern", "n_thresholds"):
        assert np.array_equal(getattr(a, f), want[f]), f
    with pytest.raises(ValueError, match="one length"):
        pwmenrich.motif_enrichment(mats, primary + [np.zeros(7, np.uint8)])


# ---------------------------------------------------------------- centrality
def _assert_centrality(res, want, n):
    exact = want["gap"] > cm.MIN_GAP
    assert exact.sum() >= 1
    for f in ("best_t", "best_lo", "best_width", "sites", "count", "ctrl_sites", "ctrl_count"):
        assert np.array_equal(getattr(res, f)[exact], want[f][exact]), f
    assert np.array_equal(res.n_tests, want["n_tests"]) and np.array_equal(res.counts, want["counts"])
    assert np.array_equal(res.iscore_thresholds, want["iscore_thresholds"])
    tol = cm.log_tolerance(n)
    for f in ("log_pvalue", "log_padj"):
        worst = float(np.max(np.abs(getattr(res, f) - want[f])))
        print("%s: largest |device - model| = %.3g (allowed %.3g)" % (f, worst, tol))
        assert worst <= tol, f
    worst = float(np.max(np.abs(res.log_fisher[exact] - want["log_fisher"][exact])))
    assert worst <= tol


@pytest.mark.parametrize("local", [False, True], ids=["centred", "local"])
def test_motif_centrality_equals_the_model_per_width_group(local):
    from explainn_amd import pwmenrich
    mats, primary, control = bm.planted_case(n_primary=90, n_control=60, length=60)
    mats = mats + [np.full((5, 4), 0.25)]                         # an empty motif among three width-12 ones
    primary = primary + [np.zeros(10, np.uint8)]                  # shorter than the widest: left out
    pv = (1e-2, 1e-3)
    kw = dict(local=local, min_sites=3, max_width=20) if local else dict(local=False)
    want = bm.centrality(mats, primary, control, pv, **kw)
    res = pwmenrich.motif_centrality(mats, primary, pv, control, chunk_bases=900, **kw)
    _assert_centrality(res, want, len(primary) + len(control))
    assert res.excluded == 1 and res.length == 60 and res.n_tests[8] == 0 and res.best_width[8] == 0
    assert res.qvalue[8] == 1.0 and np.isnan(res.threshold[8])
    assert res.starts.tolist() == [60 - w + 1 for w in bm.PLANTED_WIDTHS] + [0]
    with pytest.raises(ValueError, match="one length"):
        pwmenrich.motif_centrality(mats, primary + [np.zeros(70, np.uint8)], pv)
    with pytest.raises(ValueError, match="pvalues"):
        pwmenrich.motif_centrality(mats, primary, (1e-3,) * 17)


# ---------------------------------------------------------------- the planted case, end to end
def _write_fasta(path, recs, prefix):
    with open(path, "wt") as fh:
        for i, c in enumerate(recs):
            fh.write(">%s%d\n%s\n" % (prefix, i, "".join("ACGTN"[v] for v in c)))


def test_planted_case_end_to_end(tmp_path):
    from explainn_amd import motifs as mo
    from explainn_amd import pwmenrich
    mats, primary, control = bm.planted_case()
    motifs = bm.named(mats)
    e = pwmenrich.motif_enrichment(motifs, primary, control)
    _assert_enrichment(e, bm.enrichment(mats, primary, control), 360)
    assert int(np.argmin(e.log_pvalue)) == 3 and e.log_pvalue[3] < -50.0 and e.qvalue[3] < 0.05
    c = pwmenrich.motif_centrality(motifs, primary, (1e-3,), control)
    _assert_centrality(c, bm.centrality(mats, primary, control, (1e-3,)), 360)
    assert int(np.argmin(c.log_pvalue)) == 3 and c.log_pvalue[3] < -50.0 and c.qvalue[3] < 0.05
    assert c.best_lo[3] <= 44 < c.best_lo[3] + c.best_width[3]
    # the CLI, through a MEME file (whose probabilities are rounded: only the ranking is asserted)
    meme, pfa, cfa = tmp_path / "db.meme", tmp_path / "p.fa", tmp_path / "c.fa"
    mo.write_meme(str(meme), motifs)
    _write_fasta(pfa, primary, "peak")
    _write_fasta(cfa, control, "ctrl")
    out, best = tmp_path / "enr.tsv", tmp_path / "best.npz"
    pwmenrich.main(["enrichment", str(meme), str(pfa), "--control", str(cfa), "--max-evalue", "1000", "--save-best",
                    str(best), "-o", str(out)])
    lines = open(out).read().splitlines()
    assert lines[0].split("\t") == list(pwmenrich.ENRICHMENT_COLUMNS) and len(lines) == 9
    lead = lines[1].split("\t")
    assert lead[0] == "MA0003.1" and int(lead[4]) >= 80 and int(lead[6]) <= 2 and float(lead[9]) < -50.0
    saved = pwmenrich.MotifBest.load(str(best))
    assert saved.iscore.shape == (8, 120) and saved.ids[0] == "peak0"
    out = tmp_path / "cen.tsv"
    pwmenrich.main(["centrality", str(meme), str(pfa), "--pvalue", "1e-3", "--control", str(cfa), "--max-evalue", "1000",
                    "-o", str(out)])
    lines = open(out).read().splitlines()
    assert lines[0].split("\t") == list(pwmenrich.CENTRALITY_COLUMNS) + ["CtrlSites", "CtrlCount", "LogFisher"]
    lead = lines[1].split("\t")
    assert lead[0] == "MA0003.1" and int(lead[4]) <= 44 and int(lead[5]) >= 44 + 12 and float(lead[10]) < -50.0


# ---------------------------------------------------------------- filters and motifs in one table
def test_filters_and_motifs_in_one_table():
    from explainn_amd import enrichment as en
    from explainn_amd import pwmenrich
    from test_gpu_sites import _net
    mats, primary, control = bm.planted_case(n_primary=60, n_control=80)
    net = _net(5, 19, 100, seed=3)
    res = pwmenrich.filters_and_motifs(en.best_sites(net, primary), pwmenrich.best_motif_sites(mats, primary),
                                       en.best_sites(net, control), pwmenrich.best_motif_sites(mats, control))
    alone_f, alone_m = en.enrichment(net, primary, control), pwmenrich.motif_enrichment(mats, primary, control)
    assert res.units == 13 and res.names[:5] == ["filter%d" % u for u in range(5)] and res.names[5] == "motif0"
    for f in ("best_pattern", "tp", "fp", "u2", "log_pvalue", "log_padj"):
        assert np.array_equal(getattr(res, f), np.concatenate([getattr(alone_f, f), getattr(alone_m, f)])), f
    assert np.array_equal(res.threshold[5:], alone_m.threshold) and int(np.argmin(res.log_pvalue)) == 5 + 3
    assert np.array_equal(res.threshold[:5], alone_f.threshold.astype(np.float64))
