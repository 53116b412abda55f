"""GPU: known-motif sites (csrc/pwmsites.hip through explainn_pwm_null / explainn_pwm_sites,
explainn_amd/pwmsites.py and `python -m explainn_amd.pwmsites`) against the numpy model
tests/pwmsites_model.py.  Positions, integer scores, offsets and thresholds are compared exactly
(array_equal); fp64 tails within 1e-10 relative, the tolerance test_gpu_motifsig.py uses for fp64 tails (all
terms are positive: the true error is near 1e-14)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pwmsites_model as pm  # noqa: E402
import spacing_model as spm  # noqa: E402

pytestmark = pytest.mark.gpu

# a skewed background off the decimal grid: under (0.1, 0.4, 0.3, 0.2) the mass of AA is exactly the cutoff 1e-2
SKEWED = np.array([0.1371, 0.3629, 0.2913, 0.2087])
CUTOFFS = (1e-2, 1e-4, 1e-6)
TAIL_RTOL = 1e-10
GAP = 1e-6        # no model tail value this close (relative) to a cutoff: the device's threshold must be equal


def _lib():
    from explainn_amd import _lib
    return _lib


def _tile():
    return _lib().SITES_TILE


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _null(S, lw, bins, bg, pcut, want_tail=True):
    """explainn_pwm_null on host tables: (tail (M, wmax bins + 2) or None, thresholds) as numpy."""
    lib = _lib()
    M, wmax = S.shape[0], S.shape[1]
    Sd, wd = _dev(S), _dev(np.asarray(lw, dtype=np.int32))
    tail = torch.full((M, wmax * bins + 2), -1.0, dtype=torch.float64, device="cuda") if want_tail else None
    thr = torch.full((M,), -1, dtype=torch.int32, device="cuda")
    lib.check(lib.load().explainn_pwm_null(Sd.data_ptr(), wd.data_ptr(), M, wmax, bins, *[float(b) for b in bg],
                                           float(pcut), tail.data_ptr() if want_tail else None, thr.data_ptr(),
                                           _stream()))
    return (tail.cpu().numpy() if want_tail else None), thr.cpu().numpy()


class Scan:
    """One explainn_pwm_sites call on host arrays; buffers beyond `capacity` keep their sentinel."""
    SENTINEL = -7

    def __init__(self, S, lw, thr, codes, start=0, n_positions=None, period=0, both=True, capacity=None, tail=None,
                 bins=100, count_only=False, room=0):
        lib = _lib()
        L = lib.load()
        M, wmax = S.shape[0], S.shape[1]
        n = len(codes) - start if n_positions is None else n_positions
        Sd, wd, td, cd = _dev(S), _dev(np.asarray(lw, dtype=np.int32)), _dev(np.asarray(thr, dtype=np.int32)), _dev(codes)
        taild = _dev(tail) if tail is not None else None
        nbytes = int(L.explainn_pwm_sites_workspace_bytes(M, n))
        ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
        off = torch.full((2 * M + 1,), -1, dtype=torch.int64, device="cuda")

        def call(pos, score, pv, cap):
            lib.check(L.explainn_pwm_sites(
                cd.data_ptr(), len(codes), start, n, period, int(both), Sd.data_ptr(), wd.data_ptr(), M, wmax,
                td.data_ptr(), taild.data_ptr() if taild is not None else None, bins, off.data_ptr(),
                pos, score, pv, cap, ws.data_ptr(), nbytes, _stream()))

        call(None, None, None, 0)
        self.offsets = off.cpu().numpy()
        self.total = int(self.offsets[-1])
        if count_only:
            return
        cap = self.total if capacity is None else capacity
        size = max(self.total, cap) + room + 1
        pos = torch.full((size,), self.SENTINEL, dtype=torch.int32, device="cuda")
        isc = torch.full((size,), self.SENTINEL, dtype=torch.int32, device="cuda")
        pv = torch.full((size,), float(self.SENTINEL), dtype=torch.float64, device="cuda")
        off.fill_(-1)
        call(pos.data_ptr(), isc.data_ptr(), pv.data_ptr() if taild is not None else None, cap)
        self.offsets_emit = off.cpu().numpy()
        self.pos, self.iscore, self.pvalue = pos.cpu().numpy(), isc.cpu().numpy(), pv.cpu().numpy()


def _tables(widths, seed, bins=100, bg=None, pcut=1e-2):
    """Model tables of Dirichlet motifs: (S, live widths, thresholds at pcut, tail)."""
    bg = pm.uniform() if bg is None else bg
    S, w, scale, _ = pm.quantise(pm.dirichlet_motifs(widths, seed), bg, 0.1, bins)
    lw = pm.live_widths(w, scale)
    tail, thr = pm.null_table(S, lw, bins, bg, pcut)
    return S, lw, thr, tail


def _check_scan(S, lw, thr, codes, min_sites=1, **kw):
    """pos, iscore and offsets equal the model's; returns the Scan."""
    got = Scan(S, lw, thr, codes, **kw)
    model_kw = {k: kw[k] for k in ("start", "n_positions", "period", "both") if k in kw}
    off, pos, isc = pm.scan(S, lw, thr, codes, **model_kw)
    assert np.array_equal(got.offsets, off) and np.array_equal(got.offsets_emit, off)
    assert got.total == len(pos) >= min_sites
    assert np.array_equal(got.pos[:got.total], pos) and np.array_equal(got.iscore[:got.total], isc)
    assert np.all(got.pos[got.total:] == Scan.SENTINEL) and np.all(got.iscore[got.total:] == Scan.SENTINEL)
    return got


# ---------------------------------------------------------------- the null
NULL_WIDTHS = [0, 1, 2, 6, 19, 63, 64]


@pytest.mark.parametrize("bins", [1, 16, 100, 128])
@pytest.mark.parametrize("bg", [None, SKEWED], ids=["uniform", "skewed"])
def test_null_tail_and_thresholds(bins, bg):
    bgv = pm.uniform() if bg is None else bg
    mats = pm.dirichlet_motifs(NULL_WIDTHS, seed=20 + bins) + [np.full((5, 4), 0.25)]
    S, widths, scale, _ = pm.quantise(mats, bgv, 0.1, bins)
    lw = pm.live_widths(widths, scale)
    assert lw[0] == 0 and (bg is not None or lw[-1] == 0) and np.all(lw[1:-1] == NULL_WIDTHS[1:])
    for pcut in CUTOFFS:
        want_tail, want_thr = pm.null_table(S, lw, bins, bgv, pcut)
        gap = pm.min_relative_gap(want_tail, lw, bins, pcut)
        print("bins=%d pcut=%g: smallest relative gap of a model tail to the cutoff %.3g" % (bins, pcut, gap))
        assert gap > GAP                               # the condition under which the thresholds must be equal
        tail, thr = _null(S, lw, bins, bgv, pcut)
        live = want_tail > 0
        err = float(np.abs(tail[live] / want_tail[live] - 1.0).max())
        print("    max relative tail error %.3g" % err)
        assert err <= TAIL_RTOL
        for m, w in enumerate(lw):
            assert not tail[m, w * bins + 1:].any()    # zero past the motif's range; an empty motif: all zero
        assert np.array_equal(thr, want_thr)
        assert thr[0] == 1 and np.all(tail[0] == 0)
        _, thr_only = _null(S, lw, bins, bgv, pcut, want_tail=False)
        assert np.array_equal(thr_only, want_thr)


def test_null_argument_errors_and_bad_widths():
    lib = _lib()
    L = lib.load()
    S, lw, _, _ = _tables([6, 9], seed=1)
    Sd, thr = _dev(S), torch.full((2,), -5, dtype=torch.int32, device="cuda")
    wd = _dev(np.array([6, 9], dtype=np.int32))
    for pcut in (-0.1, 1.5, float("nan")):
        assert L.explainn_pwm_null(Sd.data_ptr(), wd.data_ptr(), 2, 9, 100, .25, .25, .25, .25, pcut, None,
                                   thr.data_ptr(), _stream()) == lib.E_ARG
        assert b"pcut" in L.explainn_last_error()
    for bad in dict(M=-1), dict(wmax=0), dict(wmax=65), dict(bins=0), dict(bins=129):
        a = dict(M=2, wmax=9, bins=100)
        a.update(bad)
        assert L.explainn_pwm_null(Sd.data_ptr(), wd.data_ptr(), a["M"], a["wmax"], a["bins"], .25, .25, .25, .25, 1e-3,
                                   None, thr.data_ptr(), _stream()) == lib.E_ARG
    assert L.explainn_pwm_null(Sd.data_ptr(), wd.data_ptr(), 2, 9, 100, .5, .5, 0.0, .25, 1e-3, None, thr.data_ptr(),
                               _stream()) == lib.E_ARG
    torch.cuda.synchronize()
    assert np.all(thr.cpu().numpy() == -5)             # nothing was launched
    # a width outside [1, wmax] is an empty motif, found on the device
    tail, got = _null(S, np.array([10, -3], dtype=np.int32), 100, pm.uniform(), 1e-3)
    assert np.array_equal(got, [1, 1]) and not tail.any()


# ---------------------------------------------------------------- the scan
@pytest.mark.parametrize("n", ["1", "TILE-1", "TILE", "TILE+1", "2*TILE+3"])
def test_scan_around_the_tile(n):
    n = eval(n, {"TILE": _tile()})
    S, lw, thr, tail = _tables([6, 19, 64], seed=2)
    codes = pm.random_codes(n + 80, seed=n)
    if n == 1:
        thr = np.zeros(3, dtype=np.int32)              # one start: make it a site of every motif it is live for
        codes[:64] = np.minimum(codes[:64], 3)
    got = _check_scan(S, lw, thr, codes, n_positions=n, tail=tail)
    row = np.repeat(np.arange(6), np.diff(got.offsets))
    assert np.array_equal(got.pvalue[:got.total], tail[row // 2, got.iscore[:got.total]])      # bit for bit
    assert np.all(got.pvalue[got.total:] == Scan.SENTINEL)
    for r in range(6):
        assert np.all(np.diff(got.pos[got.offsets[r]:got.offsets[r + 1]]) > 0)


def test_scan_from_a_start_and_to_the_sequence_end():
    S, lw, thr, _ = _tables([6, 19, 64], seed=3)
    codes = pm.random_codes(_tile() + 300, seed=4)
    _check_scan(S, lw, thr, codes, start=37, n_positions=_tile() + 5, min_sites=10)
    # to the very end: the last starts have fewer than w bases left and are not live
    got = _check_scan(S, lw, np.zeros(3, dtype=np.int32), codes, start=len(codes) - 100, n_positions=100)
    assert got.offsets[1] - got.offsets[0] <= 95 and got.offsets[5] - got.offsets[4] <= 37


def test_sequence_shorter_than_the_widest_motif():
    S, lw, _, _ = _tables([6, 64], seed=5)
    codes = pm.random_codes(30, seed=6, n_frac=0.0)
    got = _check_scan(S, lw, np.zeros(2, dtype=np.int32), codes)
    assert np.array_equal(np.diff(got.offsets), [25, 25, 0, 0])


@pytest.mark.parametrize("M", ["1", "GROUP", "GROUP+1"])
def test_motif_counts_around_the_group(M):
    M = eval(M, {"GROUP": _lib().PWM_GROUP})
    widths = list(np.random.default_rng(M).integers(4, 13, size=M))
    S, lw, thr, _ = _tables(widths, seed=7)
    got = _check_scan(S, lw, thr, pm.random_codes(_tile() + 200, seed=8), min_sites=M)
    assert np.all(np.diff(got.offsets).reshape(M, 2).sum(axis=1) > 0)      # every motif has sites


def test_empty_rows_n_runs_and_bytes_above_four():
    S, lw, thr, _ = _tables([8, 5, 12, 7, 9], seed=9)
    lw = lw.copy()
    lw[1], lw[3] = 0, 13                               # width 0; a width past wmax = 12: both rows empty
    codes = pm.random_codes(3000, seed=10, n_frac=0.0)
    codes[100:140] = 4
    codes[1020:1030] = 4                               # an N run across the tile boundary
    codes[[500, 1500, 2500]] = [5, 9, 255]             # bytes above 4 read as N
    codes[2990:] = 4
    got = _check_scan(S, lw, thr, codes, min_sites=20)
    cnt = np.diff(got.offsets).reshape(5, 2).sum(axis=1)
    assert cnt[1] == 0 and cnt[3] == 0 and np.all(cnt[[0, 2, 4]] > 0)
    # every live N-free start at threshold 0
    got = _check_scan(S, lw, np.zeros(5, dtype=np.int32), codes)
    free = lambda w: sum(1 for p in range(3000 - w + 1) if codes[p:p + w].max() < 4)
    assert np.array_equal(np.diff(got.offsets), [free(8)] * 2 + [0, 0] + [free(12)] * 2 + [0, 0] + [free(9)] * 2)


def test_period_with_motifs_up_to_and_past_the_record():
    S, lw, thr, _ = _tables([6, 50, 64], seed=11, pcut=1e-2)
    thr = np.array([thr[0], 0, 0], dtype=np.int32)     # width 50: one start per record; width 64: none
    codes = pm.random_codes(2000, seed=12, n_frac=0.0)
    got = _check_scan(S, lw, thr, codes, period=50, min_sites=40)
    assert np.array_equal(np.diff(got.offsets)[2:], [40, 40, 0, 0])
    assert np.array_equal(got.pos[got.offsets[2]:got.offsets[3]], np.arange(0, 2000, 50))
    assert np.all(got.pos[got.offsets[0]:got.offsets[2]] % 50 <= 44)
    _check_scan(S, lw, thr, codes, period=50, start=50, n_positions=1100, min_sites=20)


@pytest.mark.parametrize("both", [False, True])
def test_threshold_extremes_and_strands(both):
    S, lw, thr, _ = _tables([6, 10, 15], seed=13)
    codes = pm.random_codes(_tile() + 100, seed=14)
    bins = 100
    mixed = np.array([0, thr[1], lw[2] * bins + 1], dtype=np.int32)      # every start; the cutoff; nothing
    got = _check_scan(S, lw, mixed, codes, both=both)
    cnt = np.diff(got.offsets)
    assert cnt[0] > 900 and cnt[4] == 0 and cnt[5] == 0
    assert (cnt[1] == cnt[0] and cnt[3] > 0) if both else (cnt[1] == 0 and cnt[3] == 0)


def test_count_only_capacity_and_repeatability():
    S, lw, thr, tail = _tables([6, 9, 12], seed=15)
    codes = pm.random_codes(2 * _tile() + 50, seed=16)
    off, pos, isc = pm.scan(S, lw, thr, codes)
    total = len(pos)
    assert total > 60
    counted = Scan(S, lw, thr, codes, count_only=True)
    assert np.array_equal(counted.offsets, off)
    cap = total // 2
    cut = Scan(S, lw, thr, codes, capacity=cap, tail=tail, room=total)
    assert np.array_equal(cut.offsets_emit, off)                         # offsets still hold the full counts
    assert np.array_equal(cut.pos[:cap], pos[:cap]) and np.array_equal(cut.iscore[:cap], isc[:cap])
    assert np.all(cut.pos[cap:] == Scan.SENTINEL) and np.all(cut.iscore[cap:] == Scan.SENTINEL)
    assert np.all(cut.pvalue[cap:] == Scan.SENTINEL)
    a, b = Scan(S, lw, thr, codes, tail=tail), Scan(S, lw, thr, codes, tail=tail)
    for key in ("offsets", "pos", "iscore", "pvalue"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key


def test_scan_argument_errors():
    lib = _lib()
    L = lib.load()
    S, lw, thr, _ = _tables([6, 9], seed=17)
    codes = pm.random_codes(500, seed=18)
    Sd, wd, td, cd = _dev(S), _dev(lw), _dev(thr), _dev(codes)
    off = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty((int(L.explainn_pwm_sites_workspace_bytes(2, 500)),), dtype=torch.uint8, device="cuda")

    def call(start=0, n=500, period=0, M=2, wmax=9, bins=100, cap=0, nbytes=None, pv=None, seq_len=500):
        return L.explainn_pwm_sites(cd.data_ptr(), seq_len, start, n, period, 1, Sd.data_ptr(), wd.data_ptr(), M, wmax,
                                    td.data_ptr(), None, bins, off.data_ptr(), None, None, pv, cap, ws.data_ptr(),
                                    ws.numel() if nbytes is None else nbytes, _stream())

    assert call() == lib.OK
    for bad in (dict(start=-1), dict(n=501), dict(start=1), dict(period=-1), dict(cap=-1), dict(M=-1), dict(wmax=0),
                dict(wmax=65), dict(bins=0), dict(nbytes=8), dict(pv=off.data_ptr())):
        assert call(**bad) == lib.E_ARG, bad
    torch.cuda.synchronize()
    assert call(n=0) == lib.OK
    assert not off.cpu().numpy().any()                 # no positions: offsets zeroed


# ---------------------------------------------------------------- end to end
def _planted_case():
    mats = pm.dirichlet_motifs([6, 12, 9, 20], seed=30, alpha=0.2)
    codes = pm.random_codes(5000, seed=31, n_frac=0.005)
    g = np.random.default_rng(32)
    for at in range(60, 4900, 150):
        i = int(g.integers(0, 4))
        pm.plant(codes, mats[i], at, reverse=bool(g.integers(0, 2)))
    motifs = [("MA%04d.1" % i, "name%d" % i, m) for i, m in enumerate(mats)]
    return motifs, mats, codes


def _assert_calls(calls, want):
    for key in ("offsets", "start", "strand", "iscore", "score", "widths"):
        assert np.array_equal(getattr(calls, key), want[key]), key
    assert calls.score.dtype == np.float32 and calls.pvalue.dtype == np.float64
    assert np.all(np.abs(calls.pvalue / want["pvalue"] - 1.0) <= TAIL_RTOL)


def test_scan_motifs_end_to_end():
    from explainn_amd import pwmsites
    motifs, mats, codes = _planted_case()
    want = pm.calls(mats, codes, 1e-3)
    lw = pm.live_widths(want["widths"], np.ones(4))
    assert pm.min_relative_gap(want["tail"], lw, 100, 1e-3) > GAP
    assert np.all(want["strand"][:1] == 1) and {1, -1} <= set(want["strand"].tolist()) and len(want["start"]) > 30
    calls = pwmsites.scan_motifs(motifs, codes, pvalue=1e-3)
    _assert_calls(calls, want)
    assert calls.names == [m[0] for m in motifs] and calls.kernel_size == 20 and calls.units == 4
    assert np.all(calls.pvalue <= 1e-3)
    for u in range(4):                                 # per motif '+' ascending, then '-' ascending
        start, strand, _ = calls.unit(u)
        for s in (1, -1):
            assert np.all(np.diff(start[strand == s]) > 0)
        assert np.all(np.diff(strand.astype(int)) <= 0)
    # the chunking does not show: tiny chunks, device-resident codes, bare matrices
    small = pwmsites.scan_motifs(motifs, codes, pvalue=1e-3, chunk_positions=300)
    on_device = pwmsites.scan_motifs(mats, torch.from_numpy(codes).cuda(), pvalue=1e-3, chunk_positions=1777)
    for other in (small, on_device):
        for key in ("offsets", "start", "strand", "iscore", "score", "pvalue"):
            assert np.array_equal(getattr(other, key), getattr(calls, key)), key
    # forward strand only, a period, the sequence's own background
    fwd = pwmsites.scan_motifs(motifs, codes, pvalue=1e-3, strands="fwd", period=100)
    _assert_calls(fwd, pm.calls(mats, codes, 1e-3, both=False, period=100))
    bg = pm.sequence_background(codes)
    want_bg = pm.calls(mats, codes, 1e-3, bg=bg)
    assert pm.min_relative_gap(want_bg["tail"], lw, 100, 1e-3) > GAP
    _assert_calls(pwmsites.scan_motifs(motifs, codes, pvalue=1e-3, bg="sequence"), want_bg)
    with pytest.raises(ValueError, match="max_sites"):
        pwmsites.scan_motifs(motifs, codes, pvalue=1e-3, max_sites=5)
    empty = pwmsites.scan_motifs(motifs, codes[:0], pvalue=1e-3)
    assert len(empty) == 0 and empty.units == 4


def test_score_null_equals_the_model():
    from explainn_amd import pwmsites
    _, mats, _ = _planted_case()
    null = pwmsites.score_null(mats + [np.zeros((0, 4))], pvalue=1e-4, bg=SKEWED, bins=64)
    S, widths, scale, _ = pm.quantise(mats + [np.zeros((0, 4))], SKEWED, 0.1, 64)
    lw = pm.live_widths(widths, scale)
    tail, thr = pm.null_table(S, lw, 64, SKEWED, 1e-4)
    assert pm.min_relative_gap(tail, lw, 64, 1e-4) > GAP
    assert np.array_equal(null.thresholds.cpu().numpy(), thr) and np.array_equal(null.widths.cpu().numpy(), lw)
    assert np.array_equal(null.scores.cpu().numpy(), S) and null.wmax == 20
    got = null.tail.cpu().numpy()
    assert np.all(np.abs(got[tail > 0] / tail[tail > 0] - 1.0) <= TAIL_RTOL) and not got[tail == 0].any()


def test_spacing_of_filters_against_known_motifs():
    from explainn_amd import pwmsites
    from explainn_amd.sites import call_sites, concat_units
    from explainn_amd.spacing import spacing
    from test_gpu_sites import _dense, _net
    motifs, _, codes = _planted_case()
    net = _net(5, 19, 200, seed=3)
    flat = _dense(net, codes).astype(np.float32)
    thr = np.sort(flat, axis=1)[:, -40]                # some forty sites per filter and strand
    filter_calls = call_sites(net, codes, thr)
    pwm_calls = pwmsites.scan_motifs(motifs, codes, pvalue=1e-3)
    both = concat_units(filter_calls, pwm_calls)
    assert both.units == 9 and both.kernel_size == 20 and len(both) == len(filter_calls) + len(pwm_calls)
    got = spacing(both, 30).hist.cpu().numpy()
    want = spm.of_calls(spm.brute, both, 30)
    assert got.shape == want.shape == (9, 9, 2, 61) and np.array_equal(got, want)
    assert got[:5, 5:].sum() > 0                       # filter-versus-known-motif pairs were counted


def test_cli_reproduces_the_model_rows(tmp_path):
    from explainn_amd import motifs as mo
    from explainn_amd import pwmsites
    motifs, _, codes = _planted_case()
    meme, fasta, out = tmp_path / "db.meme", tmp_path / "x.fa", tmp_path / "out.bed"
    mo.write_meme(str(meme), motifs)
    back = mo.read_meme(str(meme))
    records = [("chrA", codes[:1800]), ("chrB", codes[1800:2500]), ("short", codes[2500:2504])]
    with open(fasta, "wt") as fh:
        for rid, c in records:
            text = "".join("ACGTN"[v] for v in c)
            fh.write(">%s some description\n" % rid)
            fh.writelines(text[i:i + 60] + "\n" for i in range(0, len(text), 60))
    pwmsites.main([str(meme), str(fasta), "--pvalue", "1e-3", "--bg", "0.3,0.2,0.2,0.3", "-o", str(out)])
    bg = np.array([0.3, 0.2, 0.2, 0.3])
    want = []
    for rid, c in records:
        m = pm.calls([b[2] for b in back], c, 1e-3, bg=bg)
        assert pm.min_relative_gap(m["tail"], pm.live_widths(m["widths"], np.ones(4)), 100, 1e-3) > GAP
        want += pm.bed_rows(rid, m, [b[0] for b in back])
    got = open(out).readlines()
    assert len(want) > 10 and got == want
