"""GPU: motif spacing (csrc/spacing.hip through explainn_site_spacing / explainn_spacing_test,
explainn_amd/spacing.py and `python -m explainn_amd.spacing`) against the brute-force numpy model
tests/spacing_model.py.  Histograms and the integer statistics are compared exactly (array_equal); the
p-value within ten times the deviation of the model's tail from scipy (test_spacing_model.py)."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import spacing_model as sm  # noqa: E402
from test_gpu_sites import _codes, _dense  # noqa: E402
from test_spacing_model import BINOM_TAIL_DEVIATION, planted  # noqa: E402

pytestmark = pytest.mark.gpu

PVALUE_RTOL = 10 * BINOM_TAIL_DEVIATION


def _spacing(sites, U, D, **kw):
    from explainn_amd.spacing import spacing
    return spacing(sm.calls_of(*sites, U), D, **kw)


def _check(sites, U, D, **kw):
    """spacing() of model-ordered sites equals the brute force; returns the host histogram."""
    got = _spacing(sites, U, D, **kw).hist.cpu().numpy()
    want = sm.brute(*sites, U, D, anchors=kw.get("anchors"), partners=kw.get("partners"))
    assert got.shape == want.shape and np.array_equal(got, want)
    return got


def _edge_sites():
    """5 units, ~200 sites on 2000 coordinates: positions shared between units, unit 0 on both strands of
    one position, unit 2 empty, unit 3 with '-' sites only, unit 4 with a single site."""
    unit, start, strand = sm.random_sites(2, 190, 2000, seed=1)
    g = np.random.default_rng(2)
    shared = start[(unit == 0) & (strand > 0)][:12]
    extra = [(1, p, 1) for p in shared[:6]] + [(1, p, -1) for p in shared[6:]]        # units 0 and 1 on one position
    extra += [(0, p, -1) for p in shared[:4]]                                        # unit 0 on both strands of it
    extra += [(3, int(p), -1) for p in g.choice(2000, 9, replace=False)] + [(4, int(shared[0]) + 3, 1)]
    u, p, s = (np.array(c, dtype=np.int64) for c in zip(*extra))
    unit, start, strand = np.concatenate([unit, u]), np.concatenate([start, p]), np.concatenate([strand, s])
    keep = np.unique(np.stack([unit, start, strand]), axis=1, return_index=True)[1]  # distinct records
    return sm.in_order(unit[keep], start[keep], strand[keep])


def test_edge_lists_equal_brute_force():
    sites = _edge_sites()
    unit, start, strand = sites
    assert np.sum(unit == 2) == 0 and np.all(strand[unit == 3] < 0) and np.sum(unit == 4) == 1
    h = _check(sites, 5, 10)
    assert h[0, 1, 0, 10] >= 6 and h[0, 1, 1, 10] >= 6 and h[0, 0, 1, 10] >= 8          # d = 0 is counted
    assert h[0, 0, 0, 10] == 0 and h[4, 4].sum() == 0 and h[2].sum() == 0 and h[:, 2].sum() == 0
    assert np.array_equal(h[:, :, 0, :], h.transpose(1, 0, 2, 3)[:, :, 0, ::-1])
    assert np.array_equal(h[:, :, 1, :], h.transpose(1, 0, 2, 3)[:, :, 1, :])
    assert np.all(h[np.arange(5), np.arange(5), 1] % 2 == 0)


@pytest.mark.parametrize("D", [0, 1])
def test_smallest_distances(D):
    assert _check(_edge_sites(), 5, D).sum() > 0


def test_distance_cap_and_beyond():
    from explainn_amd import _lib
    from explainn_amd.spacing import spacing
    cap = _lib.SPACING_MAX_DISTANCE
    sites = sm.random_sites(3, 50, 4000, seed=3)
    assert _check(sites, 3, cap).sum() > 0
    with pytest.raises(ValueError, match="max_distance"):
        spacing(sm.calls_of(*sites, 3), cap + 1)
    # the entry point itself: refused, nothing launched, the histogram untouched
    pos = torch.from_numpy(sites[1]).cuda()
    off2 = torch.from_numpy(np.arange(7, dtype=np.int64) * 0).cuda()
    hist = torch.zeros(3, 3, 2, 2 * (cap + 1) + 1, dtype=torch.int64, device="cuda")
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for D in (cap + 1, -1):
        assert lib.explainn_site_spacing(pos.data_ptr(), off2.data_ptr(), 3, None, 3, None, 3, D, hist.data_ptr(),
                                         stream) == _lib.E_ARG
    assert b"max_distance" in lib.explainn_last_error()
    assert lib.explainn_site_spacing(pos.data_ptr(), off2.data_ptr(), 3, None, 2, None, 3, 5, hist.data_ptr(),
                                     stream) == _lib.E_ARG                       # a null set means all units
    assert lib.explainn_spacing_test(hist.data_ptr(), 3, 3, None, None, cap + 1, 0, 0, hist.data_ptr(),
                                     hist.data_ptr(), hist.data_ptr(), hist.data_ptr(), stream) == _lib.E_ARG
    torch.cuda.synchronize()
    assert not bool(hist.any())


def test_long_list_against_short_list():
    """3000 sites against 3, in both roles: threads stride over the anchor's records and, with four pairs, the
    long list is split over the grid's slices."""
    g = np.random.default_rng(4)
    long = np.sort(g.choice(40000, 3000, replace=False))
    unit = np.concatenate([np.zeros(3000), np.ones(3)]).astype(np.int64)
    start = np.concatenate([long[:1700], long[1700:], long[[5, 1500]] + 3, long[[2999]] - 2])
    strand = np.concatenate([np.ones(1700), -np.ones(1300), [1, 1, -1]]).astype(np.int64)
    start[:1700], start[1700:3000] = np.sort(start[:1700]), np.sort(start[1700:3000])
    start[3000:3002] = np.sort(start[3000:3002])
    h = _check((unit, start, strand), 2, 25)
    assert h[0, 1].sum() == h[1, 0].sum() > 0 and h[0, 0].sum() > 3000
    for kw in (dict(anchors=[0], partners=[1]), dict(anchors=[1], partners=[0]), dict(anchors=[0], partners=[0])):
        _check((unit, start, strand), 2, 25, **kw)                             # one pair: the most slices


def test_dense_run():
    """300 consecutive positions on both strands in two units, D = 64: every anchor has more than 64 partners
    in range, and every lane of a wavefront counts into the same few bins."""
    p = np.arange(100, 400)
    sites = sm.in_order(np.repeat([0, 0, 1, 1], 300), np.tile(p, 4), np.repeat([1, -1, 1, -1], 300))
    h = _check(sites, 2, 64)
    assert h[0, 1, 0, 64] == 600 and h[0, 0, 0, 64] == 0 and h[0, 0, 1, 64] == 600


def test_coordinates_beyond_32_bits():
    unit, start, strand = _edge_sites()
    low = _check((unit, start, strand), 5, 10)
    assert np.array_equal(_check((unit, start + (1 << 33), strand), 5, 10), low)


def test_unit_sets_are_unit_ids():
    """A != P, unordered, overlapping: entry [1][1] is unit 1 with itself, entry [0][0] is unit 4 with unit 0."""
    sites = _edge_sites()
    full = _check(sites, 5, 10)
    h = _check(sites, 5, 10, anchors=[4, 1], partners=[0, 1, 3])
    assert np.array_equal(h, full[[4, 1]][:, [0, 1, 3]])
    counts = _spacing(sites, 5, 10, anchors=[4, 1], partners=[0, 1, 3])
    res = counts.test(min_distance=0, min_count=0)
    want = sm.test_stats(h, [4, 1], [0, 1, 3], 10, 0, 0)
    assert np.array_equal(res.total.cpu().numpy(), want[0])                     # [1][1] folded, [0][0] not
    assert want[0][1, 1, 0] == h[1, 1, 0, 11:].sum() and want[0][0, 0, 0] == h[0, 0, 0].sum()


def test_accumulation():
    from explainn_amd.spacing import spacing
    one, two = sm.random_sites(4, 150, 600, seed=5), sm.random_sites(4, 170, 700, seed=6)
    want = sm.brute(*one, 4, 12) + sm.brute(*two, 4, 12)
    acc = spacing(sm.calls_of(*one, 4), 12)
    out = spacing(sm.calls_of(*two, 4), 12, out=acc)
    assert out is acc and np.array_equal(acc.hist.cpu().numpy(), want)
    n1, n2 = (np.array([[np.sum((s[0] == u) & (s[2] == t)) for t in (1, -1)] for u in range(4)]) for s in (one, two))
    assert np.array_equal(acc.site_counts, n1 + n2)
    twice = spacing(sm.calls_of(*one, 4), 12)
    spacing(sm.calls_of(*one, 4), 12, out=twice)
    assert np.array_equal(twice.hist.cpu().numpy(), 2 * sm.brute(*one, 4, 12))
    with pytest.raises(ValueError, match="out="):
        spacing(sm.calls_of(*one, 4), 13, out=acc)


def test_records_are_kept_apart():
    from explainn_amd.spacing import spacing
    L, D = 50, 20
    unit, start, strand = sm.random_sites(3, 200, 8 * L, seed=7)
    edge = [(0, L - 1, 1), (1, L, 1), (2, 2 * L - 1, -1), (0, 2 * L, -1), (1, 3 * L - 2, 1), (1, 3 * L + 1, -1)]
    u, p, s = (np.array(c, dtype=np.int64) for c in zip(*edge))
    unit, start, strand = sm.in_order(np.concatenate([unit, u]), np.concatenate([start, p]), np.concatenate([strand, s]))
    want = sm.by_record(sm.brute, unit, start, strand, start // L, 3, D)
    assert not np.array_equal(sm.brute(unit, start, strand, 3, D), want)
    got = spacing(sm.calls_of(unit, start, strand, 3), D, period=L)
    assert np.array_equal(got.hist.cpu().numpy(), want)
    # the same records one by one, and records of unequal lengths
    for lengths in ([L] * 8, [70, 33, 120, 50, 127]):
        bounds = np.concatenate([[0], np.cumsum(lengths)])
        recs, want = [], 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            m = (start >= lo) & (start < hi)
            recs.append((sm.calls_of(unit[m], start[m] - lo, strand[m], 3), hi - lo))
            want = want + sm.brute(unit[m], start[m], strand[m], 3, D)
        assert np.array_equal(spacing(recs, D).hist.cpu().numpy(), want)


def test_same_input_same_bits():
    sites = sm.random_sites(4, 400, 900, seed=8)
    a, b = _spacing(sites, 4, 30), _spacing(sites, 4, 30)
    assert torch.equal(a.hist, b.hist)
    ra, rb = a.test(min_count=1), b.test(min_count=1)
    assert all(torch.equal(getattr(ra, f), getattr(rb, f)) for f in ("total", "best_distance", "best_count", "pvalue",
                                                                     "qvalue"))


# ------------------------------------------------------------------------------------------- the test
def _held(hist, anchors, partners, D, k=5, units=None, site_counts=None):
    from explainn_amd.spacing import SpacingCounts
    units = units if units is not None else int(max(max(anchors), max(partners))) + 1
    return SpacingCounts(torch.from_numpy(hist).cuda(), anchors, partners, D, k,
                         np.zeros((units, 2)) if site_counts is None else site_counts)


def _assert_test(res, hist, anchors, partners, D, min_distance, min_count):
    total, best_d, best_c, p = sm.test_stats(hist, anchors, partners, D, min_distance, min_count)
    assert np.array_equal(res.total.cpu().numpy(), total)
    assert np.array_equal(res.best_count.cpu().numpy(), best_c)
    assert np.array_equal(res.best_distance.cpu().numpy(), best_d)
    got = res.pvalue.cpu().numpy()
    big = p > 1e-300
    worst = float(np.max(np.abs(got[big] - p[big]) / p[big])) if big.any() else 0.0
    print("largest relative deviation of the device p-value from the model: %.3g (bound %.3g)" % (worst, PVALUE_RTOL))
    assert worst <= PVALUE_RTOL
    assert np.all(got[~big] < 1e-290)
    q, tested = sm.qvalues(total, p, anchors, partners, D, min_distance, min_count)
    assert np.array_equal(res.tested.cpu().numpy(), tested)
    assert np.allclose(res.qvalue.cpu().numpy(), q, rtol=1e-6, atol=0)
    return total, best_d, best_c, p


def test_statistics_of_constructed_histograms():
    D = 12
    g = np.random.default_rng(9)
    anchors, partners = [0, 1, 2], [2, 0, 1, 3]
    hist = g.poisson(g.choice([0.2, 3.0, 40.0, 4000.0], size=(3, 4, 2, 1)), size=(3, 4, 2, 2 * D + 1)).astype(np.int64)
    hist[0, 1, 0] = hist[0, 1, 0][::-1] + hist[0, 1, 0]                  # a == b, same strand: mirrored
    hist[1:, [2, 0], 1] *= 2                                             # a == b, opposite strands: even
    hist[0, 1, 1] *= 2
    hist[0, 0, 0] = 3                                                    # a tie over every bin: the lowest wins
    hist[0, 0, 0, [D - 7, D + 4]] = 11                                   # and a tie of two
    hist[1, 3, 1] = 5
    hist[1, 3, 1, D + 6] = 200                                           # a clear peak
    hist[2, 3, 0] = 0
    hist[2, 3, 0, D + 9] = 4                                             # n < min_count
    for md, mc in ((5, 10), (0, 0), (1, 10), (D, 1), (D + 1, 0)):
        res = _held(hist, anchors, partners, D).test(min_distance=md, min_count=mc)
        total, best_d, best_c, p = _assert_test(res, hist, anchors, partners, D, md, mc)
        if (md, mc) == (5, 10):
            assert best_d[0, 0, 0] == -7 and best_c[0, 0, 0] == 11 and best_d[1, 3, 1] == 6
            assert (total[2, 3, 0], best_c[2, 3, 0], p[2, 3, 0]) == (4, 0, 1.0)
            assert 0 < p[1, 3, 1] < 1e-20
        if md == D + 1:
            assert not total.any() and np.all(p == 1.0)
    # default min_distance: the kernel size
    res = _held(hist, anchors, partners, D, k=7).test()
    _assert_test(res, hist, anchors, partners, D, 7, 10)


def test_planted_spacing_is_found():
    from explainn_amd.spacing import spacing
    unit, start, strand, rec, U, L = planted()
    D = 20
    counts = spacing(sm.calls_of(unit, start + rec * L, strand, U), D, period=L)
    hist = counts.hist.cpu().numpy()
    assert np.array_equal(hist, sm.by_record(sm.brute, unit, start, strand, rec, U, D))
    n_positions = 400 * (L - 4)
    res = counts.test(min_distance=5, min_count=10, n_positions=n_positions)
    _assert_test(res, hist, np.arange(U), np.arange(U), D, 5, 10)
    q = res.qvalue.cpu().numpy()
    assert int(res.best_distance[0, 1, 0]) == 7 and int(res.best_distance[1, 0, 0]) == -7
    others = np.ones(q.shape, dtype=bool)
    others[0, 1, 0] = others[1, 0, 0] = False
    assert q[0, 1, 0] == q.min() and q[0, 1, 0] < 1e-100 and q[others].min() > 1e-4
    want = sm.expected(counts.site_counts, np.arange(U), np.arange(U), D, 5, n_positions)
    assert np.allclose(res.expected.cpu().numpy(), want, rtol=1e-12)
    ratio = res.ratio.cpu().numpy()
    # 240 planted pairs on top of the ~60 that two sites per record give any pair of filters
    assert ratio[0, 1, 0] > 2 * np.nanmax(np.where(others & (want > 0), ratio, np.nan))


def test_save_and_load(tmp_path):
    from explainn_amd.spacing import SpacingCounts
    counts = _spacing(_edge_sites(), 5, 10, anchors=[4, 1], partners=[0, 1, 3])
    path = os.path.join(tmp_path, "counts.npz")
    counts.save(path)
    back = SpacingCounts.load(path)
    assert torch.equal(back.hist, counts.hist) and back.max_distance == 10 and back.kernel_size == 5
    assert np.array_equal(back.anchors, [4, 1]) and np.array_equal(back.partners, [0, 1, 3])
    assert np.array_equal(back.site_counts, counts.site_counts)


# ------------------------------------------------------------------------------------------- end to end
def _model_calls(net, codes):
    from explainn_amd.sites import call_sites
    thr = np.median(_dense(net, codes).astype(np.float32), axis=1)
    return call_sites(net, codes, thr), thr


def test_end_to_end_model_and_bank():
    from explainn_amd import ExplaiNN, ExplaiNNBank
    from explainn_amd.spacing import spacing
    torch.manual_seed(11)
    a, b = ExplaiNN(8, 5, 50, 1), ExplaiNN(8, 5, 50, 1)
    bank = ExplaiNNBank.from_models([a, b]).cuda().eval()
    a, b = a.cuda().eval(), b.cuda().eval()
    codes = _codes(3000, seed=12, n_frac=0.003)
    calls, thr_a = _model_calls(a, codes)
    assert len(calls) > 10000
    got = spacing(calls, 20)
    assert np.array_equal(got.hist.cpu().numpy(), sm.of_calls(sm.brute, calls, 20))
    assert np.array_equal(got.site_counts.sum(axis=1), np.diff(calls.offsets)) and got.kernel_size == 5
    from explainn_amd.sites import call_sites
    _, thr_b = _model_calls(b, codes)
    both = call_sites(bank, codes, np.concatenate([thr_a, thr_b]))
    assert both.units == 16
    kw = dict(anchors=[9, 0, 15], partners=[0, 12, 9, 3])
    got = spacing(both, 20, **kw)
    assert np.array_equal(got.hist.cpu().numpy(), sm.of_calls(sm.brute, both, 20, **kw))


def test_cli(tmp_path):
    from explainn_amd import ExplaiNN, sites, spacing as sp
    torch.manual_seed(13)
    m = ExplaiNN(4, 5, 50, 1).cuda().eval()
    ckpt = os.path.join(tmp_path, "model.pth.tar")
    torch.save({"options": dict(m._options), "state_dict": {key: v.cpu() for key, v in m.state_dict().items()}}, ckpt)
    records = [("one", _codes(700, seed=14)), ("two", _codes(433, seed=15))]
    fa, tsv, out, npz = (os.path.join(tmp_path, n) for n in ("seqs.fa", "thr.tsv", "out.tsv", "counts.npz"))
    with open(fa, "w") as fh:
        for rid, codes in records:
            fh.write(">%s desc\n%s\n" % (rid, "".join("ACGTN"[c] for c in codes)))
    thr = np.quantile(_dense(m, records[0][1]).astype(np.float32), 0.9, axis=1)
    sites.write_thresholds(tsv, thr)
    sp.main([ckpt, fa, "-t", tsv, "-o", out, "-d", "15", "--max-qvalue", "1", "--min-count", "5", "--save-counts", npz])
    lines = open(out).read().splitlines()
    assert lines[0].split("\t") == list(sp.COLUMNS) == ["FilterA", "FilterB", "Orientation", "Distance", "Count", "Total",
                                                        "Expected", "Ratio", "Pvalue", "Qvalue"]
    per_record = [(sites.call_sites(m, codes, thr), len(codes)) for _, codes in records]
    counts = sp.spacing(per_record, 15)
    assert torch.equal(sp.SpacingCounts.load(npz).hist, counts.hist)
    want = sum(sm.of_calls(sm.brute, c, 15) for c, _ in per_record)
    assert np.array_equal(counts.hist.cpu().numpy(), want)
    res = counts.test(min_count=5, n_positions=sum(len(codes) - 4 for _, codes in records))
    tested = res.tested.cpu().numpy()
    rows = [ln.split("\t") for ln in lines[1:]]
    keys = [(int(r[0][6:]), int(r[1][6:]), ("same", "opposite").index(r[2])) for r in rows]
    assert sorted(keys) == sorted((a, b, o) for a, b, o in zip(*np.nonzero(tested)) if a <= b) and rows
    pv = [float(r[8]) for r in rows]
    assert pv == sorted(pv)
    for (a, b, o), r in zip(keys, rows):
        assert int(r[3]) == int(res.best_distance[a, b, o]) and int(r[4]) == int(res.best_count[a, b, o])
        assert int(r[5]) == int(res.total[a, b, o])
        for col, field in ((6, res.expected), (7, res.ratio), (8, res.pvalue), (9, res.qvalue)):
            assert float(r[col]) == float("%.6g" % float(field[a, b, o]))
    # a stricter q-value keeps a subset of the rows; the forward strand alone has no opposite orientation
    sp.main([ckpt, fa, "-t", tsv, "-o", out, "-d", "15", "--max-qvalue", "1", "--min-count", "5", "--strands", "fwd"])
    fwd = [ln.split("\t") for ln in open(out).read().splitlines()[1:]]
    assert fwd and all(r[2] == "same" for r in fwd)
