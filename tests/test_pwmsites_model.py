"""CPU: the numpy model of known-motif sites (tests/pwmsites_model.py) against enumeration of every w-mer,
and the host half of explainn_amd/pwmsites.py (quantise, assembly, concat_units, the BED writer, argument
checks) against the model.  No device call is made."""
import os
import re

import numpy as np
import pytest

import pwmsites_model as pm
from explainn_amd import _lib, pwmsites, sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKEWED = np.array([0.1, 0.4, 0.3, 0.2])


@pytest.mark.parametrize("w", [1, 2, 5, 6])
@pytest.mark.parametrize("bins", [16, 100])
def test_null_equals_enumeration_of_every_kmer(w, bins):
    (m,) = pm.dirichlet_motifs([w], seed=10 + w)
    S, widths, scale, _ = pm.quantise([m], SKEWED, 0.1, bins)
    assert scale[0] > 0 and widths[0] == w
    pdf, want = pm.null_pdf(S[0, :w], SKEWED, bins), pm.enumerated_pdf(S[0, :w], SKEWED, bins)
    err = float(np.abs(pdf - want).max())
    print("w=%d bins=%d: max |pdf - enumeration| = %.3g" % (w, bins, err))
    assert err <= 1e-14
    tail = pm.tail_of(pdf)
    assert abs(tail[0] - 1.0) <= 1e-12 and np.all(np.diff(tail) <= 0)
    # every mass under this background is a multiple of 10^-w, w <= 6: cutoffs off that grid meet no tie
    for pcut in (0.3712345678, 0.0712345678, 0.0131234567, 2.3456789e-4):
        thr = pm.threshold_of(tail, pcut)
        mass = lambda t: float(want[max(t, 0):].sum())
        assert mass(thr) <= pcut * (1 + 1e-12)
        assert thr == 0 or mass(thr - 1) > pcut


def test_threshold_out_of_range_when_no_score_reaches_the_cutoff():
    (col,) = pm.dirichlet_motifs([1], seed=3)
    S, _, _, _ = pm.quantise([np.repeat(col, 2, axis=0)], None, 0.1, 100)      # both columns reach `bins`
    tail = pm.tail_of(pm.null_pdf(S[0], pm.uniform(), 100))
    assert tail[200] == 1 / 16                                   # the best 2-mer
    assert pm.threshold_of(tail, 1e-6) == 2 * 100 + 1
    t = pm.threshold_of(tail, 1 / 16)                            # the scores only the best 2-mer reaches
    assert t <= 200 and tail[t] == 1 / 16 and tail[t - 1] > 1 / 16
    assert pm.threshold_of(tail, 1.0) == 0
    (m,) = pm.dirichlet_motifs([2], seed=3)                      # the best 2-mer scores less than 2 bins:
    S, _, _, _ = pm.quantise([m], None, 0.1, 100)                # the threshold is the first score above it
    best = int(S[0].max(axis=1).sum())
    assert best < 200 and pm.threshold_of(pm.tail_of(pm.null_pdf(S[0], pm.uniform(), 100)), 1e-6) == best + 1


@pytest.mark.parametrize("bins", [1, 16, 100, 128])
def test_quantise_reaches_both_ends_and_equals_the_model(bins):
    mats = pm.dirichlet_motifs([1, 6, 19, 64], seed=1) + [np.zeros((0, 4)), np.full((5, 4), 0.25)]
    counts = np.random.default_rng(2).integers(0, 30, size=(8, 4)).astype(np.float64)
    counts[3] = 0                                                # a column without counts reads as uniform
    mats.append(counts)
    for bg in (None, SKEWED):
        S, widths, scale, lo = pwmsites.quantise(mats, bg, 0.1, bins)
        S2, widths2, scale2, lo2 = pm.quantise(mats, bg, 0.1, bins)
        assert S.dtype == np.int16 and S.shape == (7, 64, 4)
        assert np.array_equal(S, S2) and np.array_equal(widths, widths2)
        assert np.allclose(scale, scale2, rtol=1e-14, atol=0) and np.allclose(lo, lo2, rtol=1e-14, atol=0)
        for i, m in enumerate(mats):
            if scale[i] > 0:
                assert S[i, :len(m)].min() == 0 and S[i, :len(m)].max() == bins
            assert not S[i, len(m):].any()
        assert scale[4] == 0 and (bg is not None or scale[5] == 0)     # width 0; flat under a uniform background
        assert np.array_equal(pm.live_widths(widths, scale) == 0, scale == 0)


def test_real_score_is_the_log_odds_up_to_the_rounding_of_the_cells():
    (m,) = pm.dirichlet_motifs([8], seed=4)
    S, _, scale, lo = pwmsites.quantise([m], SKEWED, 0.1, 100)
    word = pm.consensus(m)
    exact = sum(np.log2((m[j, a] + 0.1 * SKEWED[a]) / 1.1 / SKEWED[a]) for j, a in enumerate(word))
    got = sum(int(S[0, j, a]) for j, a in enumerate(word)) / scale[0] + 8 * lo[0]
    assert abs(got - exact) <= 8 * 0.5 / scale[0] + 1e-12         # half a bin per column


def _model_case(seed=5, n=700, both=True, period=0):
    mats = pm.dirichlet_motifs([6, 11, 4], seed=seed)
    codes = pm.random_codes(n, seed + 1, n_frac=0.02)
    for at, (i, rev) in zip((40, 200, 333, 500), ((0, False), (1, True), (2, False), (0, True))):
        pm.plant(codes, mats[i], at, reverse=rev)
    return mats, codes


def test_reverse_hits_mirror_the_forward_hits_of_the_reverse_complement():
    mats, codes = _model_case()
    S, widths, scale, _ = pm.quantise(mats)
    lw = pm.live_widths(widths, scale)
    _, thr = pm.null_table(S, lw, 100, pm.uniform(), 1e-2)
    off, pos, isc = pm.scan(S, lw, thr, codes)
    off_rc, pos_rc, isc_rc = pm.scan(S, lw, thr, pm.rc_codes(codes))
    assert off[-1] > 20
    for m, w in enumerate(widths):
        minus = slice(off[2 * m + 1], off[2 * m + 2])
        plus_rc = slice(off_rc[2 * m], off_rc[2 * m + 1])
        assert len(pos[minus]) > 0
        assert np.array_equal(pos[minus], (len(codes) - w - pos_rc[plus_rc])[::-1])
        assert np.array_equal(isc[minus], isc_rc[plus_rc][::-1])
    # the vectorised scan against the definition read off one window at a time
    for m, w in enumerate(widths):
        for p in range(len(codes) - w + 1):
            win = codes[p:p + w].astype(int)
            fwd = None if (win >= 4).any() else sum(int(S[m, j, win[j]]) for j in range(w))
            got = pos[off[2 * m]:off[2 * m + 1]]
            assert (fwd is not None and fwd >= thr[m]) == (p in got)


def test_a_palindromic_motif_hits_both_strands_at_one_coordinate():
    half = pm.dirichlet_motifs([3], seed=6, alpha=0.05)[0]
    m = np.concatenate([half, half[::-1, ::-1]])                  # column j = the complement of column w-1-j
    codes = pm.random_codes(300, 7, n_frac=0.0)
    pm.plant(codes, m, 100)
    c = pm.calls([m], codes, 1e-3)
    plus, minus = c["start"][c["strand"] > 0], c["start"][c["strand"] < 0]
    assert 100 in plus and np.array_equal(plus, minus)
    assert np.array_equal(c["iscore"][c["strand"] > 0], c["iscore"][c["strand"] < 0])


def test_period_and_n_and_the_sequence_end_in_the_model():
    mats = [np.eye(4)[[0, 1, 2, 3, 0, 1]]]                        # ACGTAC
    codes = np.tile(np.array([0, 1, 2, 3], dtype=np.uint8), 10)
    c = pm.calls(mats, codes, 1e-3, both=False)
    assert np.array_equal(c["start"], np.arange(0, 35, 4))        # 32 fits (38 <= 40), 36 does not
    assert np.array_equal(pm.calls(mats, codes, 1e-3, both=False, period=10)["start"], [0, 4, 12, 20, 24, 32])
    codes[9] = 7                                                  # a byte above 4 reads as N
    assert np.array_equal(pm.calls(mats, codes, 1e-3, both=False)["start"], [0, 12, 16, 20, 24, 28, 32])


def test_sequence_background_pools_the_strands():
    codes = np.array([0, 0, 0, 1, 2, 2, 3, 4, 4], dtype=np.uint8)
    assert np.allclose(pwmsites.sequence_background(codes, "fwd"), [3 / 7, 1 / 7, 2 / 7, 1 / 7])
    got = pwmsites.sequence_background(codes, "both")
    assert np.allclose(got, pm.sequence_background(codes)) and got[0] == got[3] and got[1] == got[2]
    with pytest.raises(ValueError, match="every base"):
        pwmsites.sequence_background(np.array([0, 1, 2], dtype=np.uint8), "fwd")


def _pwm_calls(c, names):
    return pwmsites.PwmCalls(c["offsets"], c["start"], c["strand"], c["score"], c["widths"], names, c["iscore"],
                             c["pvalue"])


def _assembled(blocks, widths, scale, lo):
    """PwmCalls of site_blocks' blocks, as scan_motifs makes them."""
    offsets, start, strand, iscore, pvalue = sites.assemble(blocks, 3, (np.int32, np.float64))
    unit = np.repeat(np.arange(3), np.diff(offsets))
    return pwmsites.PwmCalls(offsets, start, strand, iscore / scale[unit] + widths[unit] * lo[unit], widths,
                             list("abc"), iscore, pvalue)


def test_assembly_of_chunks_equals_the_whole():
    mats, codes = _model_case()
    want = pm.calls(mats, codes, 1e-2)
    S, widths, scale, lo = pm.quantise(mats)
    lw = pm.live_widths(widths, scale)
    blocks = []
    for p0, cnt in sites.position_chunks(len(codes), 97):
        off, pos, isc = pm.scan(S, lw, want["thresholds"], codes[:p0 + cnt + S.shape[1] - 1], p0, cnt)
        row = np.repeat(np.arange(6), np.diff(off))
        blocks.append((p0, np.arange(6), off, pos, isc, want["tail"][row // 2, isc]))
    got = _assembled(blocks, widths, scale, lo)
    for key in ("offsets", "start", "strand", "iscore", "score", "pvalue"):
        assert np.array_equal(getattr(got, key), want[key]), key
    assert got.units == 3 and got.kernel_size == 11 and got.names == list("abc") and len(got) == len(want["start"])
    empty = _assembled([], widths, scale, lo)
    assert len(empty) == 0 and empty.units == 3 and empty.pvalue.shape == (0,)


def test_concat_units():
    mats, codes = _model_case()
    b = _pwm_calls(pm.calls(mats, codes, 1e-2), list("abc"))
    a = sites.SiteCalls([0, 2, 2, 3], [5, 9, 7], [1, -1, 1], [0.5, 0.25, 2.0], 19)
    both = sites.concat_units(a, b)
    assert type(both) is sites.SiteCalls and both.units == 6 and both.kernel_size == 19 and both.pvalue is None
    assert np.array_equal(both.offsets, np.concatenate([[0, 2, 2, 3], 3 + b.offsets[1:]]))
    for u in range(3):
        for x, y in zip(both.unit(u), a.unit(u)):
            assert np.array_equal(x, y)
        for x, y in zip(both.unit(3 + u), b.unit(u)):
            assert np.array_equal(x, y)
    a.pvalue = np.array([0.1, 0.2, 0.3])
    kept = sites.concat_units(b, a)
    assert kept.kernel_size == 19 and np.array_equal(kept.pvalue, np.concatenate([b.pvalue, a.pvalue]))
    assert np.array_equal(kept.unit(3)[0], [5, 9])


def test_bed_rows_equal_the_model():
    mats, codes = _model_case()
    c = pm.calls(mats, codes, 1e-2)
    names = ["MA0001.1", "MA0002.1", "x"]
    rows = pwmsites.bed_rows("chrT", _pwm_calls(c, names))
    assert rows == pm.bed_rows("chrT", c, names) and len(rows) == len(c["start"]) > 20
    fields = [r.rstrip("\n").split("\t") for r in rows]
    assert all(len(f) == 7 and f[0] == "chrT" and f[5] in "+-" for f in fields)
    width = dict(zip(names, c["widths"]))
    assert all(int(f[2]) - int(f[1]) == width[f[3]] for f in fields)
    assert [int(f[1]) for f in fields] == sorted(int(f[1]) for f in fields)


def test_argument_errors():
    (m,) = pm.dirichlet_motifs([5], seed=8)
    for bins in (0, 129, 2.5):
        with pytest.raises(ValueError, match="bins"):
            pwmsites.quantise([m], None, 0.1, bins)
    with pytest.raises(ValueError, match="wider"):
        pwmsites.quantise([np.full((65, 4), 0.25)])
    with pytest.raises(ValueError, match="pseudocount"):
        pwmsites.quantise([m], None, -1.0)
    with pytest.raises(ValueError, match="log-odds are not finite"):
        pwmsites.quantise([np.eye(4)], None, 0.0)
    with pytest.raises(ValueError, match="negative"):
        pwmsites.quantise([-m])
    for bg in ([0.5, 0.5, 0.0, 0.0], [0.3, 0.3, 0.3, 0.3], [0.5, 0.5], "genome"):
        with pytest.raises(ValueError, match="bg"):
            pwmsites.quantise([m], bg)
    codes = pm.random_codes(50, 9)
    with pytest.raises(ValueError, match="pvalue"):
        pwmsites.scan_motifs([m], codes, pvalue=1.5, device="cpu")
    with pytest.raises(ValueError, match="strands"):
        pwmsites.scan_motifs([m], codes, strands="rev", device="cpu")
    with pytest.raises(ValueError, match="1-D uint8"):
        pwmsites.scan_motifs([m], codes.astype(np.int64), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):    # there is no CPU path
        pwmsites.scan_motifs([m], codes, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pwmsites.score_null([m], device="cpu")


def test_motif_list_takes_named_and_bare_sets():
    mats = pm.dirichlet_motifs([4, 7], seed=11)
    names, got = pwmsites.motif_list([("MA1", "one", mats[0]), ("MA2", "", mats[1])])
    assert names == ["MA1", "MA2"] and all(np.array_equal(a, b) for a, b in zip(got, mats))
    names, got = pwmsites.motif_list(mats)
    assert names == ["motif0", "motif1"] and [len(g) for g in got] == [4, 7]
    assert np.allclose(got[1], mats[1], atol=1e-7)               # (packed sets travel as float32)


def test_cli_parsing_and_constants():
    a = pwmsites._parser().parse_args(["db.meme", "x.fa", "-o", "out.bed"])
    assert (a.pvalue, a.bg, a.pseudocount, a.bins, a.strands) == (1e-4, None, 0.1, 100, "both")
    a = pwmsites._parser().parse_args(["db.meme", "x.fa", "--bg", "0.3,0.2,0.2,0.3", "--strands", "fwd", "--bins", "64"])
    assert a.bg == [0.3, 0.2, 0.2, 0.3] and a.strands == "fwd" and a.bins == 64
    assert pwmsites._parser().parse_args(["db.meme", "x.fa", "--bg", "sequence"]).bg == "sequence"
    with pytest.raises(SystemExit):
        pwmsites._parser().parse_args(["db.meme", "x.fa", "--bg", "1,2,3"])
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert int(re.search(r"#define EXPLAINN_PWM_GROUP (\d+)", text).group(1)) == _lib.PWM_GROUP
    assert (pm.MAX_WIDTH, pm.MAX_BINS) == (_lib.MOTIF_MAX_WIDTH, _lib.MOTIF_MAX_BINS)
