"""GPU: motif centrality (csrc/central.hip through explainn_site_positions / explainn_centrality_test and
explainn_amd/centrality.py).  The histograms are compared exactly with the model of tests/centrality_model.py;
the test is compared with it field by field: integers and the chosen (threshold, region) exactly, the three log
values within centrality_model.log_tolerance(n) (log_fisher: enrichment_model.log_tolerance(N)); end to end the model is applied to the dense recount of
float16(model.linears[:3]) under the tie rule of the best sites."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import centrality_model as cm  # noqa: E402
import enrichment_model as em  # noqa: E402
from test_gpu_enrichment import _recount, _saturate  # noqa: E402
from test_gpu_sites import _codes, _net  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 60), (5, 19, 200), (7, 32, 200)]


# ------------------------------------------------------------------------------------------- histograms
def _positions(bits, site, labels, thr, M, hist=None):
    from explainn_amd.centrality import positions_device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    h, c = positions_device(dev(bits.view(np.int16)), dev(site), dev(labels), dev(thr), M,
                            None if hist is None else dev(hist))
    return h.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 182])
def test_histograms_equal_the_model(M):
    """T = 1, 3, 16; 0, 1, 63, 65 records and enough for several slices of several chunks each; labels above 1,
    sites of -1, forged starts >= M (not counted, never a write outside hist), NaN patterns, bit 15."""
    for T, n, units in ((1, 0, 2), (3, 1, 2), (16, 63, 3), (3, 65, 5), (16, 40000, 3), (1, 3000, 300)):
        bits, site, labels, thr = cm.best_case(units, n, T, M, seed=1000 * M + n, labels_upto=3)
        want, want_counts = cm.positions(bits, site, labels, thr, M)
        got, counts = _positions(bits, site, labels, thr, M)
        assert got.dtype == np.int32 and np.array_equal(got, want), (T, n)
        assert np.array_equal(counts, want_counts), (T, n)
        if n >= 63:
            assert want.sum() > 0 and np.any(site < 0) and np.any((site >> 1) >= M) and np.any(labels > 1)
        # added into: a second call doubles the bins and overwrites the counts
        again, counts = _positions(bits, site, labels, thr, M, hist=got)
        assert np.array_equal(again, 2 * want) and np.array_equal(counts, want_counts)


def test_two_calls_equal_one_call_on_the_concatenation():
    M, T, units = 65, 3, 4
    bits, site, labels, thr = cm.best_case(units, 5000, T, M, seed=7)
    whole, counts = _positions(bits, site, labels, thr, M)
    cut = 1777
    part, c1 = _positions(bits[:, :cut].copy(), site[:, :cut].copy(), labels[:cut], thr, M)
    part, c2 = _positions(bits[:, cut:].copy(), site[:, cut:].copy(), labels[cut:], thr, M, hist=part)
    assert np.array_equal(part, whole) and np.array_equal(c1 + c2, counts)
    assert np.array_equal(whole, cm.positions(bits, site, labels, thr, M)[0])


def test_thresholds_past_one_call_go_over_in_groups():
    """M = 1024: a [T][2][M] histogram of 16 thresholds is 128 KiB, so the thresholds go in groups of 8; T = 8
    fills the 64 KiB of one call to the byte."""
    M, units = 1024, 2
    for T in (8, 16):
        bits, site, labels, thr = cm.best_case(units, 3000, T, M, seed=T)
        got, counts = _positions(bits, site, labels, thr, M)
        want, want_counts = cm.positions(bits, site, labels, thr, M)
        assert np.array_equal(got, want) and np.array_equal(counts, want_counts)
    from explainn_amd import _lib
    z = torch.zeros(16, dtype=torch.int32, device="cuda")
    rc = _lib.load().explainn_site_positions(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 1, 16, 1000,
                                             z.data_ptr(), z.data_ptr(), None)
    assert rc != 0 and "split the thresholds" in _lib.load().explainn_last_error().decode()
    rc = _lib.load().explainn_site_positions(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, 1, 17, 10,
                                             z.data_ptr(), z.data_ptr(), None)
    assert rc != 0


# ------------------------------------------------------------------------------------------- the test
def _check_test(name, hist, counts, kw):
    """One explainn_centrality_test call against the model, field by field; returns the worst deviations of
    the three log values."""
    from explainn_amd.centrality import test_device
    want = cm.test_stats(hist, counts, **kw)
    assert np.all(want["gap"] > cm.MIN_GAP), (name, want["gap"])         # exactness below is then owed
    out = test_device(torch.from_numpy(hist).cuda(), torch.from_numpy(counts).cuda(), **kw)
    got = {f: t.cpu().numpy() for f, t in out.items()}
    for f in cm.FIELDS:
        if f not in cm.LOG_FIELDS:
            assert np.array_equal(got[f], want[f]), (name, f)
    n = max(int(want["sites"].max(initial=1)), 1)
    N = max(int(counts.sum()), 1)
    worst = {f: float(np.max(np.abs(got[f] - want[f]), initial=0.0)) for f in cm.LOG_FIELDS}
    print("%s: n <= %d, N = %d, largest |log_pvalue - model| = %.3g, |log_padj - model| = %.3g (allowed %.3g), "
          "|log_fisher - model| = %.3g (allowed %.3g)" % (name, n, N, worst["log_pvalue"], worst["log_padj"],
                                                          cm.log_tolerance(n), worst["log_fisher"], em.log_tolerance(N)))
    assert worst["log_pvalue"] <= cm.log_tolerance(n) and worst["log_padj"] <= cm.log_tolerance(n), name
    assert worst["log_fisher"] <= em.log_tolerance(N), name         # the hypergeometric tail's own yardstick
    untried = want["best_width"] == 0
    for f in cm.LOG_FIELDS:
        assert np.all(got[f][untried] == 0.0) and np.all(got[f] <= 0.0), (name, f)
    return want


@pytest.mark.parametrize("name", sorted(cm.test_cases()))
def test_centrality_test_equals_the_model(name):
    hist, counts, kw = cm.test_cases()[name]
    want = _check_test(name, hist, counts, kw)
    if name == "large_n":
        assert np.all(want["log_pvalue"] < -30.0)                           # log_padj's short branch
    if name == "many_units":
        assert len(want["best_t"]) > 256                                    # more units than workgroups of a call
    if name == "planted":
        M = hist.shape[3]
        assert np.all(2 * want["best_lo"] + want["best_width"] - 1 == M - 1) and np.all(want["best_width"] <= 40)


def test_centrality_test_arguments():
    from explainn_amd.centrality import test_device
    hist, counts = cm.level_case(2, 2, 3000, 100, 50, 0)
    h, c = torch.from_numpy(hist).cuda(), torch.from_numpy(counts).cuda()
    with pytest.raises(RuntimeError, match="narrow max_width"):            # 3000 starts: 4501499 regions
        test_device(h, c, local=True)
    out = test_device(h, c, local=True, max_width=50)
    want = cm.test_stats(hist, counts, local=True, max_width=50)
    assert np.all(want["gap"] > cm.MIN_GAP)
    for f in ("n_tests", "best_lo", "best_width", "count"):
        assert np.array_equal(out[f].cpu().numpy(), want[f]), f
    with pytest.raises(ValueError, match="test fewer thresholds"):
        test_device(torch.zeros((1, 16, 2, 1000), dtype=torch.int32, device="cuda"), c)
    none = test_device(torch.zeros((0, 2, 2, 9), dtype=torch.int32, device="cuda"), c)
    assert none["best_t"].numel() == 0


# ------------------------------------------------------------------------------------------- end to end
def _records(k, L, n_primary, n_control, seed):
    prim = [_codes(L, seed + i) for i in range(n_primary)] + [_codes(k - 1, seed + 500)]
    ctrl = [_codes(L, seed + 1000 + i) for i in range(n_control)] + [_codes(k - 1, seed + 501)]
    return prim, ctrl


def _want(recount, n_primary, prim, ctrl, k, M, thr, kw):
    """The model on a dense recount (bits, site) of prim + all control records, of which `ctrl` are used."""
    from explainn_amd.enrichment import record_labels
    n = n_primary + len(ctrl)
    labels = record_labels([len(r) for r in prim], [len(r) for r in ctrl], k)
    hist, counts = cm.positions(recount[0][:, :n], recount[1][:, :n], labels, thr, M)
    return hist, counts, cm.test_stats(hist, counts, **kw)


def _thresholds(bits):
    """(U, 2) float32: half and three quarters of every unit's largest best activation; the saturated units
    0 (always +inf) and 1 (always 0) get thresholds every record passes."""
    top = (bits & 0x7FFF).max(axis=1).astype(np.uint16).view(np.float16).astype(np.float32)
    thr = np.stack([0.5 * top, 0.75 * top], axis=1).astype(np.float16).astype(np.float32)
    thr[0] = (1.0, 2.0)
    thr[1] = (-2.0, -1.0)
    return thr


def _compare(res, want, counts, name):
    for f in cm.FIELDS:
        if f in cm.LOG_FIELDS:
            tol = em.log_tolerance(max(int(counts.sum()), 1)) if f == "log_fisher" else \
                cm.log_tolerance(max(int(want["sites"].max(initial=1)), 1))
            assert np.all(np.abs(getattr(res, f) - want[f]) <= tol), (name, f)
        else:
            assert np.array_equal(getattr(res, f), want[f]), (name, f)


@pytest.mark.parametrize("U,k,L", SHAPES)
def test_end_to_end_equals_the_model_on_the_dense_recount(U, k, L):
    from explainn_amd import centrality as ce
    net = _saturate(_net(U, k, L, seed=U))
    prim, ctrl = _records(k, L, 60, 40, seed=10 * U)
    M = L - k + 1
    recount = {both: _recount(net, prim + ctrl, both) for both in (True, False)}
    thr = _thresholds(recount[True][0])
    for strands, control, kw in (("both", ctrl, {}), ("fwd", ctrl, {"local": True, "max_width": 20}),
                                 ("both", None, {"min_sites": 5}), ("fwd", None, {"local": True, "min_width": 2})):
        hist, counts, want = _want(recount[strands == "both"], len(prim), prim, control or [], k, M, thr, kw)
        assert np.all(want["gap"] > cm.MIN_GAP), (strands, want["gap"])
        pos = ce.site_positions(net, prim, thr, control, strands=strands)
        assert net.input_flags() == 0
        assert np.array_equal(pos.hist, hist) and np.array_equal(pos.counts, counts) and pos.starts == M
        assert list(counts) == [60, 40 if control is not None else 0]
        res = ce.centrality(net, prim, thr, control, strands=strands, **kw)
        _compare(res, want, counts, (U, strands))
        again = ce.test_positions(pos, **kw)
        for f in cm.FIELDS:
            assert np.array_equal(getattr(again, f), getattr(res, f)), f
        assert np.array_equal(res.threshold, thr[np.arange(U), want["best_t"]])
        assert np.array_equal(res.region_end - res.region_start, np.where(want["best_width"] > 0, want["best_width"] + k - 1, 0))
        # the saturated units: every start ties, so every best site is start 0 -- the pile the docstring warns of
        assert hist[0, :, 0, 0].tolist() == [60, 60] and hist[1, :, 0, 0].tolist() == [60, 60] and not hist[:2, :, :, 1:].any()
        if kw.get("local"):
            assert (res.best_lo[0], res.best_width[0], res.count[0]) == (0, kw.get("min_width", 1), 60)
    # any chunking gives the same bits; two calls into one `out` equal one call on all records
    for chunk in (1000, 1777):
        part = ce.site_positions(net, prim, thr, ctrl, chunk_bases=chunk)
        assert np.array_equal(part.hist, ce.site_positions(net, prim, thr, ctrl).hist)
    whole = ce.site_positions(net, prim, thr, ctrl)
    acc = ce.site_positions(net, prim[:25], thr, ctrl[:10])
    assert ce.site_positions(net, prim[25:], thr, ctrl[10:], out=acc) is acc
    assert np.array_equal(acc.hist, whole.hist) and np.array_equal(acc.counts, whole.counts)
    # saved best sites give the same histograms
    from explainn_amd.enrichment import best_sites
    saved = ce.positions_from_best(best_sites(net, prim), thr, best_sites(net, ctrl))
    assert np.array_equal(saved.hist, whole.hist) and np.array_equal(saved.counts, whole.counts)
    net.train()
    with pytest.raises(NotImplementedError, match="eval-mode"):
        ce.centrality(net, prim, thr)


def test_bank_equals_its_members():
    from explainn_amd import ExplaiNNBank, centrality as ce
    k, L = 19, 200
    a, b = _net(4, k, L, seed=6), _net(4, k, L, seed=7)
    bank = ExplaiNNBank.from_models([a.cpu(), b.cpu()]).cuda().eval()
    a, b = a.cuda().eval(), b.cuda().eval()
    prim, ctrl = _records(k, L, 50, 30, seed=300)
    g = np.random.default_rng(3)
    thr = (0.3 + 0.3 * g.random((8, 2))).astype(np.float32)
    got = ce.centrality(bank, prim, thr, ctrl)
    one, two = ce.centrality(a, prim, thr[:4], ctrl), ce.centrality(b, prim, thr[4:], ctrl)
    assert got.units == 8
    for f in cm.FIELDS:
        assert np.array_equal(getattr(got, f), np.concatenate([getattr(one, f), getattr(two, f)])), f
    pos = ce.site_positions(bank, prim, thr, ctrl)
    assert np.array_equal(pos.hist[:4], ce.site_positions(a, prim, thr[:4], ctrl).hist) and pos.hist.any()


def test_command_line(tmp_path):
    from explainn_amd import centrality as ce
    from explainn_amd.sites import write_thresholds
    k, L = 19, 100
    net = _net(6, k, L, seed=8)
    prim, ctrl = _records(k, L, 80, 50, seed=700)
    g = np.random.default_rng(8)
    thr = np.sort((0.2 + 0.5 * g.random((6, 2))).astype(np.float32), axis=1)
    ckpt, fa, cfa, out, npz, t0, t1 = (os.path.join(tmp_path, n) for n in (
        "model.pth.tar", "peaks.fa", "control.fa", "out.tsv", "pos.npz", "low.tsv", "high.tsv"))
    torch.save({"options": dict(net._options), "state_dict": {key: v.cpu() for key, v in net.state_dict().items()}}, ckpt)
    for path, recs in ((fa, prim), (cfa, ctrl)):
        with open(path, "w") as fh:
            for i, codes in enumerate(recs):
                fh.write(">r%d\n%s\n" % (i, "".join("ACGTN"[c] for c in codes)))
    write_thresholds(t0, thr[:, 0])
    write_thresholds(t1, thr[:, 1])
    ce.main([ckpt, fa, "-t", t0, "-t", t1, "--control", cfa, "--local", "--max-width", "30", "--min-sites", "3",
             "--max-evalue", "1e9", "--save-positions", npz, "-o", out])
    res = ce.centrality(net, prim, thr, ctrl, local=True, max_width=30, min_sites=3)

    class Sink(list):
        write = list.append
    want = Sink()
    ce.write_table(want, ce.table_rows(res, 1e9, True), True)
    assert open(out).read() == "".join(want) and len(want) == 7
    assert want[0].rstrip("\n").split("\t") == list(ce.COLUMNS + ce.CONTROL_COLUMNS)
    pos = ce.SitePositions.load(npz)
    assert np.array_equal(pos.hist, ce.site_positions(net, prim, thr, ctrl).hist) and list(pos.counts) == [80, 50]
