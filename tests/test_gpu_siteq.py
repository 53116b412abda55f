"""GPU: site q-values -- the observed PWM score histogram (csrc/pwmsites.hip through
explainn_pwm_score_histogram and pwmsites.score_histogram), the Benjamini-Hochberg table (csrc/siteq.hip through
explainn_site_qvalues, sites.site_qtable, sites.SiteQvalues) and what the listers and command lines do with them
-- against the numpy model tests/siteq_model.py.  Every comparison is exact (array_equal): the histogram is
integer work, and every entry of the table is one fp64 multiply and one fp64 divide of the same inputs."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import actnull_model as am  # noqa: E402
import pwmsites_model as pm  # noqa: E402
import siteq_model as qm  # noqa: E402
from test_gpu_sites import _codes, _net  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = [6, 0, 19, 24, 1, 11]      # the default motif set: width 0 is an empty motif


def _lib():
    from explainn_amd import _lib
    return _lib


def _tile():
    return _lib().SITES_TILE


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tables(widths, seed, bins=100):
    S, w, scale, _ = pm.quantise(pm.dirichlet_motifs(widths, seed), pm.uniform(), 0.1, bins)
    return S, pm.live_widths(w, scale)


def _hist(S, lw, bins, codes, start=0, n_positions=None, period=0, both=True, hist=None):
    """One explainn_pwm_score_histogram call on host arrays; returns the device histogram."""
    lib = _lib()
    M, wmax = S.shape[0], S.shape[1]
    n = len(codes) - start if n_positions is None else n_positions
    Sd, wd, cd = _dev(S), _dev(np.asarray(lw, dtype=np.int32)), _dev(codes)
    if hist is None:
        hist = torch.zeros((M, wmax * bins + 2), dtype=torch.int64, device="cuda")
    lib.check(lib.load().explainn_pwm_score_histogram(
        cd.data_ptr(), len(codes), start, n, period, int(both), Sd.data_ptr(), wd.data_ptr(), M, wmax, bins,
        hist.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return hist


def _n_windows(lw, codes, n, both):
    """Per motif the tests among the first n starts that an N takes away."""
    isn = np.concatenate([[0], np.cumsum(np.asarray(codes) >= 4)])
    p = np.arange(n)
    return np.array([int((isn[p + w] != isn[p]).sum()) * (2 if both else 1) if w else 0 for w in lw], dtype=np.int64)


def _check_hist(S, lw, bins, codes, **kw):
    got = _hist(S, lw, bins, codes, **kw).cpu().numpy()
    want = qm.score_histogram(S, lw, bins, codes, **kw)
    assert np.array_equal(got, want)
    return got


# ---------------------------------------------------------------- the histogram
@pytest.mark.parametrize("both", [True, False], ids=["both", "fwd"])
@pytest.mark.parametrize("starts", [-1, 0, 1, 1025])
def test_histogram_around_the_tile(starts, both):
    """TILE - 1, TILE, TILE + 1 and 2 TILE + 1 starts: with the wmax - 1 bases behind the last one (every start
    is whole), and with the sequence ending at the last start (the last windows run out); 1 % N; every row sums to
    the number of live tests."""
    S, lw = _tables(WIDTHS, seed=1)
    wmax, n = S.shape[1], _tile() + starts
    codes = pm.random_codes(n + wmax - 1, seed=10 + starts)
    whole = _check_hist(S, lw, 100, codes, n_positions=n, both=both)
    assert np.array_equal(whole.sum(axis=1), (lw > 0) * n * (2 if both else 1) - _n_windows(lw, codes, n, both))
    got = _check_hist(S, lw, 100, codes[:n], both=both)
    assert np.array_equal(got.sum(axis=1), qm.live_tests(lw, wmax, codes[:n], 0, both))
    assert got[1].sum() == 0 and got.sum() > 3 * _tile()


@pytest.mark.parametrize("M", [1, 15, 16, 17, 33])
def test_histogram_motif_counts(M):
    """Around EXPLAINN_PWM_GROUP and around the 15 motifs of width <= 24 and 100 bins that share a workgroup."""
    g = np.random.default_rng(M)
    widths = [int(w) for w in g.integers(1, 25, size=M)]
    widths[-1] = 24
    S, lw = _tables(widths, seed=20 + M)
    _check_hist(S, lw, 100, pm.random_codes(_tile() + 300, seed=M))


def test_histogram_every_width_and_an_empty_motif():
    S, lw = _tables(list(range(0, 25)), seed=3)
    got = _check_hist(S, lw, 100, pm.random_codes(1200, seed=4))
    assert got[0].sum() == 0 and np.all(got[1:].sum(axis=1) > 0)


def test_histogram_largest_row():
    """wmax = 64 and 128 bins: rows of 8194 bins, four motifs to a workgroup, seven motifs."""
    S, lw = _tables([64, 1, 33, 0, 64, 17, 2], seed=5, bins=128)
    codes = pm.random_codes(_tile() + 200, seed=6)
    got = _check_hist(S, lw, 128, codes)
    assert got.shape[1] == 8194 and np.flatnonzero(got[0]).max() > 64 * 128 // 3


def test_histogram_one_bin():
    S, lw = _tables([5, 9, 3], seed=7, bins=1)
    got = _check_hist(S, lw, 1, pm.random_codes(1500, seed=8))
    assert got.shape[1] == 9 * 1 + 2


def test_histogram_runs_of_n_and_bytes_above_four():
    S, lw = _tables(WIDTHS, seed=9)
    codes = pm.random_codes(2500, seed=11, n_frac=0.0)
    for at, n in ((0, 1), (200, 5), (1000, 30), (1020, 10), (2499, 1)):
        codes[at:at + n] = 4
    got = _check_hist(S, lw, 100, codes)
    codes[202] = 9                                          # inside a run of N, and read as N
    assert np.array_equal(_hist(S, lw, 100, codes).cpu().numpy(), got)
    assert np.array_equal(got.sum(axis=1), qm.live_tests(lw, S.shape[1], codes))


@pytest.mark.parametrize("period,both", [(50, True), (200, False), (1024, True), (7, True)])
def test_histogram_period(period, both):
    """Windows that would cross a record boundary are not counted; a period shorter than a motif leaves it none."""
    S, lw = _tables(WIDTHS, seed=12)
    codes = pm.random_codes(period * (2100 // period + 1), seed=13)
    got = _check_hist(S, lw, 100, codes, period=period, both=both)
    assert np.array_equal(got.sum(axis=1), qm.live_tests(lw, S.shape[1], codes, period, both))
    assert got.sum() < _check_hist(S, lw, 100, codes, both=both).sum()


def test_histogram_subrange_and_accumulation():
    """start / n_positions inside a longer sequence (the bases behind the last start are read, no more); a call
    that ends at the sequence's end; two calls into one histogram add up."""
    S, lw = _tables(WIDTHS, seed=14)
    codes = pm.random_codes(3000, seed=15)
    _check_hist(S, lw, 100, codes, start=37, n_positions=1500)
    _check_hist(S, lw, 100, codes, start=2000, n_positions=1000, period=100)
    hist = _hist(S, lw, 100, codes)
    once = hist.cpu().numpy().copy()
    assert np.array_equal(_hist(S, lw, 100, codes, hist=hist).cpu().numpy(), 2 * once)
    # split at any start: the halves add up to the whole
    wmax = S.shape[1]
    parts = _hist(S, lw, 100, codes, start=0, n_positions=1111)
    _hist(S, lw, 100, codes, start=1111, n_positions=3000 - 1111, hist=parts)
    assert np.array_equal(parts.cpu().numpy(), once) and wmax == 24


def test_a_workgroup_takes_several_tiles():
    """4096 motifs of width 1 are 256 groups, so a call is cut into 4 slices and 9 tiles give a workgroup two or
    three; eight distinct motifs, repeated."""
    S8, lw8 = _tables([1] * 8, seed=16, bins=4)
    S, lw = np.tile(S8, (512, 1, 1)), np.tile(lw8, 512)
    codes = pm.random_codes(8 * _tile() + 100, seed=17)
    got = _hist(S, lw, 4, codes).cpu().numpy()
    assert np.array_equal(got, np.tile(qm.score_histogram(S8, lw8, 4, codes), (512, 1)))


def test_histogram_errors():
    lib = _lib()
    S, lw = _tables([6, 8], seed=18)
    codes = pm.random_codes(400, seed=19)
    with pytest.raises(lib.ExplainnError, match=r"code -1"):
        _hist(S, lw, 100, codes, start=0, n_positions=401)
    with pytest.raises(lib.ExplainnError, match=r"code -1"):
        _hist(S, lw, 100, codes, start=-1, n_positions=10)
    with pytest.raises(lib.ExplainnError, match=r"code -1"):
        _hist(S, lw, 100, codes, period=-1)
    with pytest.raises(lib.ExplainnError, match=r"code -1"):
        _hist(S, lw, 129, codes)
    assert int(_hist(S, lw, 100, codes, n_positions=0).sum()) == 0
    # a table entry outside [0, bins] may carry a score past the row: it is not counted, nothing else moves
    bad = S.copy()
    bad[0, 0, :] = 3000
    got = _hist(bad, lw, 100, codes).cpu().numpy()
    assert got[0].sum() == 0 and np.array_equal(got[1], qm.score_histogram(S, lw, 100, codes)[1])


def test_score_histogram_python():
    from explainn_amd import pwmsites
    mats = [("m%d" % i, "", m) for i, m in enumerate(pm.dirichlet_motifs([8, 0, 11, 24], seed=21))]
    codes = pm.random_codes(3000, seed=22)
    S, w, scale, _ = pm.quantise([m[2] for m in mats])
    want = qm.score_histogram(S, pm.live_widths(w, scale), 100, codes)
    one = pwmsites.score_histogram(mats, codes)
    assert one.dtype == torch.int64 and one.is_cuda and np.array_equal(one.cpu().numpy(), want)
    small = pwmsites.score_histogram(mats, torch.from_numpy(codes).cuda(), chunk_positions=1000)
    assert torch.equal(small, one)
    null = pwmsites.score_null(mats)
    twice = pwmsites.score_histogram(null, codes, out=pwmsites.score_histogram(null, codes, chunk_positions=333))
    assert np.array_equal(twice.cpu().numpy(), 2 * want)
    fwd = pwmsites.score_histogram(null, codes, strands="fwd", period=100)
    assert np.array_equal(fwd.cpu().numpy(), qm.score_histogram(S, pm.live_widths(w, scale), 100, codes, period=100,
                                                                 both=False))
    with pytest.raises(RuntimeError):
        pwmsites.score_histogram(null, codes, out=one[:2].contiguous())


# ---------------------------------------------------------------- the q-table
def _random_table(U, B, seed, n=2000, ties=True):
    g = np.random.default_rng(seed)
    obs = np.zeros((U, B), dtype=np.int64)
    for u in range(U):
        obs[u] = np.bincount(np.minimum((g.exponential(B / 8.0, size=n)).astype(np.int64), B - 1), minlength=B)
    steps = g.random((U, B)) * (g.random((U, B)) < (0.3 if ties else 1.0))
    steps[:, -1] += 0.05
    p = np.cumsum(steps[:, ::-1], axis=1)[:, ::-1]
    return obs, p / (p[:, :1] * (1.0 + g.random((U, 1))))


def _check_qtable(obs, p, alpha):
    from explainn_amd import sites
    q, total, first = sites.site_qtable(_dev(obs), _dev(p), alpha)
    wq, wtotal, wfirst = qm.qtable(obs, p, alpha)
    assert q.dtype == torch.float64 and first.dtype == torch.int32
    assert np.array_equal(q.cpu().numpy(), wq)
    assert np.array_equal(total.cpu().numpy(), wtotal) and np.array_equal(first.cpu().numpy(), wfirst)
    return wq, wfirst


@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("B", [1, 202, 255, 257, 2402])
def test_qtable_equals_model(U, B):
    """Bins below, at and above the 256 threads of a workgroup; tied p-values; three alphas."""
    obs, p = _random_table(U, B, seed=U * 1000 + B)
    for alpha in (0.0, 0.05, 1.0):
        _check_qtable(obs, p, alpha)


def test_qtable_edges():
    """A unit without observations, one whose every bin qualifies, one where none does, observations in one bin."""
    B = 300
    obs = np.zeros((5, B), dtype=np.int64)
    p = np.tile(np.linspace(1.0, 0.0, B), (5, 1))
    obs[1, :] = 3
    obs[2, :] = 1
    obs[3, 10] = 5
    obs[4, B - 1] = 1 << 40                                 # a count past 32 bits
    p[2] = 1e-9 * np.linspace(1.0, 0.5, B)
    p[3] = 1.0
    q, first = _check_qtable(obs, p, 0.05)
    assert np.all(q[0] == 1.0) and first[0] == B and first[2] == 0 and first[3] == B and 0 < first[1] < B
    assert q[4, B - 1] == 0.0 and np.array_equal(q[4], p[4])            # R = N in every bin: q is p


def test_qtable_errors():
    from explainn_amd import _lib, sites
    obs, p = _random_table(2, 50, seed=1)
    with pytest.raises(ValueError):
        sites.site_qtable(_dev(obs), _dev(p), 1.5)
    with pytest.raises(RuntimeError):
        sites.site_qtable(_dev(obs), _dev(p[:, :40]))
    with pytest.raises(RuntimeError):
        sites.site_qtable(_dev(obs).to(torch.int32), _dev(p))
    with pytest.raises(ValueError):
        sites.site_qtable(torch.zeros((1, _lib.SITEQ_MAX_BINS + 1), dtype=torch.int64, device="cuda"),
                          torch.zeros((1, _lib.SITEQ_MAX_BINS + 1), dtype=torch.float64, device="cuda"))
    q, total, first = sites.site_qtable(_dev(obs[:0]), _dev(p[:0]))
    assert q.shape == (0, 50) and total.shape == (0,)


# ---------------------------------------------------------------- filters, end to end
def _filter_case():
    """A tiny model, a background of 20000 bases, and 3000 bases that carry COPIES copies of the k-mer of the
    background that unit 0 likes best.  Its p-value is a few / 40000 and N about 6000, so with 58 copies its q-value
    is near 0.01."""
    from explainn_amd.sites import activation_null, call_sites
    U, k, L = 3, 8, 50
    net = _net(U, k, L, seed=3)
    background = _codes(20000, seed=40)
    codes = _codes(3000, seed=41)
    null = activation_null(net, background)
    best = call_sites(net, background, np.full(U, -1.0), strands="fwd").unit(0)
    word = background[int(best[0][np.argmax(best[2])]):][:k]
    for at in range(50, 2950, 50):
        codes[at:at + k] = word
    return net, null, codes, background


COPIES = 58


def test_site_qvalues_full_table_and_call_sites():
    from explainn_amd.sites import SiteQvalues, activation_null, call_sites, site_qvalues
    net, null, codes, background = _filter_case()
    observed = activation_null(net, codes)
    sq = site_qvalues(observed, null)
    assert isinstance(sq, SiteQvalues) and sq.q.shape == (3, am.BINS) and sq.units == 3
    obs, p = observed.hist.cpu().numpy(), qm.empirical_p(null.hist.cpu().numpy())
    alpha = 0.1
    wq, wtotal, wfirst = qm.qtable(obs, p, alpha)
    assert np.array_equal(sq.q.cpu().numpy(), wq)                     # B = 32768, and the p table has equal bits
    assert np.array_equal(sq.total.cpu().numpy(), wtotal) and np.array_equal(sq.first(alpha), wfirst)
    thr = sq.thresholds(alpha)
    assert thr.dtype == np.float32 and np.array_equal(thr, qm.filter_thresholds(wfirst))
    # every position of both strands, then those with q <= alpha: the FDR thresholds list exactly these
    full = call_sites(net, codes, np.full(3, -1.0), null=null, qvalues=sq)
    assert len(full) == 3 * 2 * (3000 - 8 + 1)
    unit = full.unit_ids()
    assert np.array_equal(full.qvalue, wq[unit, am.bins(full.score.astype(np.float16))])
    assert np.array_equal(full.pvalue, p[unit, am.bins(full.score.astype(np.float16))])
    keep = full.qvalue <= alpha
    assert keep[unit == 0].sum() >= COPIES and keep.sum() < len(keep) // 10
    called = call_sites(net, codes, thr, null=null, qvalues=sq)
    for name in ("start", "strand", "score", "pvalue", "qvalue"):
        assert np.array_equal(getattr(called, name), getattr(full, name)[keep]), name
    assert np.array_equal(np.diff(called.offsets), np.bincount(unit[keep], minlength=3))
    # without the new arguments: what it was
    plain = call_sites(net, codes, thr)
    assert plain.qvalue is None and plain.pvalue is None and np.array_equal(plain.start, called.start)
    assert np.array_equal(sq.qvalue(unit[:100], full.score[:100]), full.qvalue[:100])
    # mismatches are refused
    with pytest.raises(ValueError, match="strands"):
        site_qvalues(activation_null(net, codes, strands="fwd"), null)
    with pytest.raises(ValueError, match="shuffles"):
        site_qvalues(activation_null(net, codes.reshape(-1, 50), shuffles=1), null)
    with pytest.raises(ValueError, match="units"):
        call_sites(_net(4, 8, 50), codes, np.zeros(4), qvalues=sq)


# ---------------------------------------------------------------- known motifs, end to end
def _pwm_case():
    mats = pm.dirichlet_motifs([8, 5, 11, 20], seed=50, alpha=0.1)
    codes = pm.random_codes(3000, seed=51, n_frac=0.005)
    for i, at in enumerate(range(100, 2900, 200)):
        pm.plant(codes, mats[(0, 2, 3)[i % 3]], at, reverse=bool(i % 2))
    return [("MA%04d.1" % i, "name%d" % i, m) for i, m in enumerate(mats)], mats, codes


def _pwm_expect(mats, pieces, pcut, alpha, both=True):
    """The model's sites of every piece at pcut, their q-values over all the pieces (the device's own tail as the
    p table: its bits are not the model's, test_gpu_pwmsites.py holds them within 1e-10) and the q <= alpha mask."""
    from explainn_amd import pwmsites
    tail = pwmsites.score_null(mats, pcut).tail.cpu().numpy()
    S, w, scale, _ = pm.quantise(mats)
    lw = pm.live_widths(w, scale)
    hist = sum(qm.score_histogram(S, lw, 100, c, both=both) for c in pieces)
    q, _, _ = qm.qtable(hist, tail, alpha)
    out = []
    for c in pieces:
        want = pm.calls(mats, c, pcut, both=both)
        assert pm.min_relative_gap(want["tail"], lw, 100, pcut) > 1e-6
        qv = q[want["unit"], want["iscore"]] if len(want["unit"]) else np.zeros(0)
        out.append((want, qv, qv <= alpha))
    return out


def test_scan_motifs_qvalue():
    from explainn_amd import pwmsites
    motifs, mats, codes = _pwm_case()
    pcut, alpha = 1e-2, 0.05
    (want, qv, keep), = _pwm_expect(mats, [codes], pcut, alpha)
    assert 14 <= keep.sum() < len(keep)
    calls = pwmsites.scan_motifs(motifs, codes, pvalue=pcut, qvalue=alpha)
    for key in ("start", "strand", "iscore", "score"):
        assert np.array_equal(getattr(calls, key), want[key][keep]), key
    assert calls.qvalue.dtype == np.float64 and np.array_equal(calls.qvalue, qv[keep])
    assert np.array_equal(np.diff(calls.offsets), np.bincount(want["unit"][keep], minlength=4))
    # the chunking does not show; a histogram given beforehand is the one it would count
    other = pwmsites.scan_motifs(motifs, codes, pvalue=pcut, qvalue=alpha, chunk_positions=700,
                                 observed=pwmsites.score_histogram(mats, codes))
    for key in ("offsets", "start", "strand", "iscore", "qvalue", "pvalue"):
        assert np.array_equal(getattr(other, key), getattr(calls, key)), key
    # observed alone adds the column and filters nothing; without either the result is what it was
    column = pwmsites.scan_motifs(motifs, codes, pvalue=pcut, observed=pwmsites.score_histogram(mats, codes))
    plain = pwmsites.scan_motifs(motifs, codes, pvalue=pcut)
    assert plain.qvalue is None and np.array_equal(column.qvalue, qv)
    for key in ("offsets", "start", "strand", "iscore", "pvalue"):
        assert np.array_equal(getattr(column, key), getattr(plain, key)), key
    # one family of tests over two records: the q-values are over both
    two = [codes[:1800], codes[1800:]]
    hist = pwmsites.score_histogram(mats, two[1], out=pwmsites.score_histogram(mats, two[0]))
    for piece, (w2, q2, k2) in zip(two, _pwm_expect(mats, two, pcut, alpha)):
        got = pwmsites.scan_motifs(motifs, piece, pvalue=pcut, qvalue=alpha, observed=hist)
        assert np.array_equal(got.start, w2["start"][k2]) and np.array_equal(got.qvalue, q2[k2])
    fwd = pwmsites.scan_motifs(motifs, codes, pvalue=pcut, qvalue=0.2, strands="fwd")
    (w3, q3, k3), = _pwm_expect(mats, [codes], pcut, 0.2, both=False)
    assert np.array_equal(fwd.start, w3["start"][k3]) and np.array_equal(fwd.qvalue, q3[k3])
    with pytest.raises(ValueError):
        pwmsites.scan_motifs(motifs, codes, qvalue=1.5)


# ---------------------------------------------------------------- command lines
def _write_fasta(path, records):
    with open(path, "wt") as fh:
        for rid, c in records:
            fh.write(">%s\n%s\n" % (rid, "".join("ACGTN"[v] for v in c)))


def test_pwmsites_cli(tmp_path):
    from explainn_amd import motifs as mo
    from explainn_amd import pwmsites
    motifs, _, codes = _pwm_case()
    meme, fasta, out = (str(tmp_path / n) for n in ("db.meme", "x.fa", "out.bed"))
    mo.write_meme(meme, motifs)
    back = mo.read_meme(meme)
    mats, names = [b[2] for b in back], [b[0] for b in back]
    records = [("chrA", codes[:1800]), ("chrB", codes[1800:]), ("short", codes[:4])]
    _write_fasta(fasta, records)
    expect = _pwm_expect(mats, [c for _, c in records], 1e-2, 0.05)

    def rows(keep_all):
        """The model's rows (pwmsites_model.bed_rows: seven columns) with the q-value behind them."""
        want = []
        for (rid, _), (w, qv, keep) in zip(records, expect):
            k = np.ones(len(qv), bool) if keep_all else keep
            c = dict(w, **{key: w[key][k] for key in ("start", "unit", "strand", "score", "pvalue")})
            order = sorted(range(int(k.sum())), key=lambda i: (c["start"][i], c["unit"][i], -c["strand"][i]))
            want += [ln[:-1] + "\t%.6g\n" % qv[k][i] for ln, i in zip(pm.bed_rows(rid, c, names), order)]
        return want

    def got(*flags):
        pwmsites.main([meme, fasta, "--pvalue", "1e-2", "-o", out] + list(flags))
        return open(out).readlines()

    plain = got()
    assert plain and all(len(ln.split("\t")) == 7 for ln in plain)
    eight = got("--qvalues")
    assert eight == rows(True)
    assert [ln.rsplit("\t", 1)[0] + "\n" for ln in eight] == plain                  # the first seven: unchanged
    kept = got("--qvalues", "--max-qvalue", "0.05")
    assert 0 < len(kept) < len(eight) and kept == rows(False)


def test_sites_and_calibrate_cli(tmp_path):
    from explainn_amd import calibrate, sites
    net, null, codes, background = _filter_case()
    ckpt, bg, fa, tsv, qtsv, npz, bed = (str(tmp_path / n) for n in (
        "model.pth.tar", "bg.fa", "x.fa", "thresholds.tsv", "fdr.tsv", "null.npz", "sites.bed"))
    torch.save({"options": dict(net._options), "state_dict": {k: v.cpu() for k, v in net.state_dict().items()}}, ckpt)
    records = [("r0", codes[:1700]), ("r1", codes[1700:]), ("tiny", codes[:5])]
    _write_fasta(bg, [("bg", background)])
    _write_fasta(fa, records)
    calibrate.main([ckpt, bg, "-o", tsv, "--pvalue", "0.01", "--background", "sequence", "--save-null", npz])
    assert torch.equal(sites.ActivationNull.load(npz).hist, null.hist)
    observed = sites.records_null(net, [c for _, c in records])
    assert torch.equal(observed.hist, sum(sites.activation_null(net, c).hist for _, c in records[:2]))
    sq = sites.site_qvalues(observed, null)
    calibrate.main([ckpt, bg, "-o", qtsv, "--background", "sequence", "--qvalue", "0.1", "--target", fa])
    assert np.array_equal(sites.read_thresholds(qtsv, 3), sq.thresholds(0.1))
    thr = sites.read_thresholds(tsv, 3)

    def run(*flags):
        sites.main([ckpt, fa, "-t", tsv, "-o", bed] + list(flags))
        return open(bed).readlines()

    def want(thresholds):
        rows = []
        for rid, c in records:
            rows += sites.bed_rows(rid, sites.call_sites(net, c, thresholds, null=null, qvalues=sq))
        return rows

    seven = run("--null", npz)
    eight = run("--null", npz, "--qvalues")
    assert eight and eight == want(thr) and all(len(ln.split("\t")) == 8 for ln in eight)
    assert [ln.rsplit("\t", 1)[0] + "\n" for ln in eight] == seven                 # without the flag: unchanged
    kept = run("--null", npz, "--qvalues", "--max-qvalue", "0.1")
    assert kept == want(np.maximum(thr, sq.thresholds(0.1))) and 0 < len(kept) < len(eight)
    assert all(float(ln.split("\t")[7]) <= 0.1 for ln in kept)
    assert os.path.getsize(bed) > 0
