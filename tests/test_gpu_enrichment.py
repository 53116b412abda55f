"""GPU: motif enrichment (csrc/enrich.hip through explainn_record_best / explainn_enrichment_test and
explainn_amd/enrichment.py).  The best sites are compared exactly with a dense recount of
float16(model.linears[:3]) on the materialised windows under the model's tie rule; the test is compared
stage by stage with the fp64 model of tests/enrichment_model.py: integers exactly, the two log values within
enrichment_model.log_tolerance(N)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import enrichment_model as em  # noqa: E402
import sites_model as sm  # noqa: E402
from test_enrichment_model import em_labels, kmer_records  # noqa: E402
from test_gpu_sites import _codes, _dense, _net  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 60), (5, 19, 200), (7, 32, 200)]


def _span():
    from explainn_amd import _lib
    return _lib.BEST_SPAN


def _saturate(net):
    """Unit 0 always +inf, unit 1 always 0 (BatchNorm1's bias at +40 / -40): every start ties."""
    with torch.no_grad():
        net.linears[1].bias[0] = 40.0
        net.linears[1].bias[1] = -40.0
    return net


def _record_acts(net, rec, reverse):
    """float16 (U, len - k + 1) of one record of at least k bases: the record is padded with N to the model's
    window and only its own live starts are read."""
    o = net._options
    L, k = o["sequence_length"], o["kernel_size"]
    padded = np.concatenate([rec, np.full(max(L - len(rec), 0), 4, np.uint8)])
    P = len(rec) - k + 1
    if not reverse:
        return _dense(net, padded)[:, :P]
    # the forward activations of rc(record), padded behind it, mapped back to forward starts
    back = np.concatenate([sm.rc_codes(rec), np.full(max(L - len(rec), 0), 4, np.uint8)])
    return _dense(net, back)[:, :P][:, ::-1]


def _recount(net, recs, both):
    k = net._options["kernel_size"]
    codes = np.concatenate(recs + [np.zeros(0, np.uint8)])
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return em.record_best(lambda c, rev: _record_acts(net, c, rev), codes, off, k, both)


def _launch(net, recs, strands=2, offsets=None):
    flat = np.concatenate(recs + [np.full(1, 4, np.uint8)])
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64) if offsets is None else offsets
    bits, site = net._launch_record_best(torch.from_numpy(flat).cuda(), torch.from_numpy(np.asarray(off, np.int64)).cuda(),
                                         strands)
    return bits.cpu().numpy().view(np.uint16), site.cpu().numpy()


def _edge_records(k, seed):
    """k-1, k, k+1 bases; SPAN-1, SPAN, SPAN+1 and SPAN+k-1 starts; several passes; an empty record; records
    that end in N; a reverse palindrome.  1 % N throughout."""
    span = _span()
    g = np.random.default_rng(seed)
    starts = [span - 1, span, span + 1, span + k - 1, 3 * span + 17]
    recs = [_codes(n, seed + i) for i, n in enumerate([k - 1, k, k + 1, 0] + [s + k - 1 for s in starts])]
    recs[2][-1] = 4
    recs[5][-3:] = 4
    half = g.integers(0, 4, size=30).astype(np.uint8)
    recs.append(np.concatenate([half, sm.rc_codes(half)]))
    return recs


@pytest.mark.parametrize("U,k,L", SHAPES)
def test_dense_recount(U, k, L):
    from explainn_amd.enrichment import best_sites
    net = _saturate(_net(U, k, L, seed=U))
    recs = _edge_records(k, seed=10 * U)
    for both in (True, False):
        want_bits, want_site = _recount(net, recs, both)
        bits, site = _launch(net, recs, 2 if both else 1)
        assert net.input_flags() == 0
        assert np.array_equal(bits, want_bits), both
        assert np.array_equal(site, want_site), both
        rb = best_sites(net, [("r%d" % i, r) for i, r in enumerate(recs)], strands="both" if both else "fwd")
        assert np.array_equal(rb.bits, want_bits) and rb.ids[1] == "r1" and rb.kernel_size == k
        assert np.array_equal(rb.start, np.where(want_site < 0, -1, want_site >> 1))
        assert np.array_equal(rb.strand, np.where(want_site < 0, 0, 1 - 2 * (want_site & 1)))
        assert np.array_equal(rb.lengths, [len(r) for r in recs])
    # the saturated units: every start ties, the first one on '+' wins; short and empty records have none
    live = np.array([len(r) >= k for r in recs])
    assert np.all(bits[0, live] == 0x7C00) and np.all(bits[1] == 0)
    assert np.all(site[:2, live] == 0) and np.all(site[:, ~live] == -1) and np.all(bits[:, ~live] == 0)
    pal = recs[-1]
    f, r = _record_acts(net, pal, False), _record_acts(net, pal, True)
    assert np.array_equal(f, r[:, ::-1])                 # the palindrome: both strands hold the maximum


def test_bad_input_raises_the_flag_and_stays_inside():
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=3)
    recs = [_codes(n, 40 + i) for i, n in enumerate((50, 60, 70, 10))]
    good_bits, good_site = _launch(net, recs)
    assert net.input_flags() == 0
    dirty = [r.copy() for r in recs]
    dirty[1][25] = 9                                     # reads as N
    as_n = [r.copy() for r in recs]
    as_n[1][25] = 4
    bits, site = _launch(net, dirty)
    assert net.input_flags() & 1 and net.input_flags() == 0
    want = _launch(net, as_n)
    assert np.array_equal(bits, want[0]) and np.array_equal(site, want[1])
    dirty = [r.copy() for r in recs]
    dirty[3][2] = 200                                    # in a record shorter than the kernel
    _launch(net, dirty)
    assert net.input_flags() & 1
    # a descending pair, a pair past the end, a negative offset: those records read as empty, the others --
    # one of them overlapping its neighbours -- are what the model reads from the same offsets
    k = net._options["kernel_size"]
    flat = np.concatenate(recs + [np.full(1, 4, np.uint8)])
    total = len(flat) - 1
    for off in ([0, 50, 110, 100, total], [0, 50, 110, total + 5, total], [-3, 50, 110, 180, total]):
        bits, site = _launch(net, recs, offsets=off)
        assert net.input_flags() & 1
        want = em.record_best(lambda c, rev: _record_acts(net, c, rev), flat, off, k)
        assert np.array_equal(bits, want[0]) and np.array_equal(site, want[1])
        empty = [r for r in range(4) if not 0 <= off[r] <= off[r + 1] <= len(flat)]
        assert empty and np.all(bits[:, empty] == 0) and np.all(site[:, empty] == -1)
        assert np.array_equal(bits[:, 1], good_bits[:, 1]) and np.array_equal(site[:, 1], good_site[:, 1])
    assert np.array_equal(_launch(net, recs)[0], good_bits)


def test_many_units_many_records_per_workgroup():
    """300 units x 1500 records of 40-60 bases: 75 unit quads, several records per workgroup."""
    U, k, L = 300, 19, 60
    net = _net(U, k, L, seed=4)
    g = np.random.default_rng(4)
    recs = [_codes(int(n), 100 + i) for i, n in enumerate(g.integers(40, 61, size=1500))]
    pad = lambda r: np.concatenate([r, np.full(L - len(r), 4, np.uint8)])
    with torch.no_grad():
        fw = net.linears[:3](torch.from_numpy(sm.onehot(np.stack([pad(r) for r in recs]))).cuda())
        rv = net.linears[:3](torch.from_numpy(sm.onehot(np.stack([pad(sm.rc_codes(r)) for r in recs]))).cuda())
    fw, rv = (em.to_bits(x.cpu().numpy().astype(np.float16)).astype(np.int32) for x in (fw, rv))     # (R, U, Lo)
    want_bits = np.zeros((U, len(recs)), np.uint16)
    want_site = np.zeros((U, len(recs)), np.int32)
    for i, r in enumerate(recs):
        P = len(r) - k + 1
        f, v = fw[i, :, :P], rv[i, :, :P][:, ::-1]
        both = np.maximum(f, v)
        top = both.max(axis=1)
        p = np.argmax(both == top[:, None], axis=1)
        want_bits[:, i] = top
        want_site[:, i] = (p << 1) | (f[np.arange(U), p] != top)
    bits, site = _launch(net, recs)
    assert net.input_flags() == 0
    assert np.array_equal(bits, want_bits) and np.array_equal(site, want_site)
    assert (site & 1).any() and not (site & 1).all()


def test_chunking_does_not_change_the_result():
    from explainn_amd.enrichment import best_sites
    net = _net(5, 19, 200, seed=5)
    g = np.random.default_rng(5)
    recs = [_codes(int(n), 200 + i) for i, n in enumerate(g.integers(10, 400, size=40))]
    whole = best_sites(net, recs)
    assert (whole.start >= 0).any()
    for chunk in (1000, 1777):
        part = best_sites(net, recs, chunk_bases=chunk)
        for name in ("bits", "start", "strand", "lengths"):
            assert np.array_equal(getattr(part, name), getattr(whole, name)), (chunk, name)


def test_bank_equals_its_members():
    from explainn_amd import ExplaiNNBank
    from explainn_amd.enrichment import best_sites
    k, L = 19, 200
    a, b = _net(4, k, L, seed=6), _net(4, k, L, seed=7)
    bank = ExplaiNNBank.from_models([a.cpu(), b.cpu()]).cuda().eval()
    a, b = a.cuda().eval(), b.cuda().eval()
    recs = [_codes(n, 300 + n) for n in (18, 19, 150, 300, 77)]
    got, one, two = best_sites(bank, recs), best_sites(a, recs), best_sites(b, recs)
    assert got.score.shape == (8, 5)
    for name in ("bits", "start", "strand"):
        assert np.array_equal(getattr(got, name), np.concatenate([getattr(one, name), getattr(two, name)])), name


# ------------------------------------------------------------------------------------------- the test
def _check_test(bits, labels, name):
    """One explainn_enrichment_test call against the model, stage by stage; returns the worst deviations of
    the two log values."""
    from explainn_amd.enrichment import enrichment_test
    want = em.test_stats(bits, labels)
    assert np.all(want["gap"] > em.MIN_GAP), (name, want["gap"])         # exactness below is then owed
    dev = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()
    got = {f: t.cpu().numpy() for f, t in enrichment_test(dev, torch.from_numpy(labels).cuda(), want_tails=True).items()}
    assert np.array_equal(got["tails"], want["tails"]), name
    for f in ("n_thresholds", "best_pattern", "tp", "fp", "u2", "counts"):
        assert np.array_equal(got[f], want[f]), (name, f)
    Np, Nc = (int(c) for c in want["counts"])
    if Np > 0 and Nc > 0:
        assert np.array_equal(got["auroc"], want["u2"] / (2.0 * Np * Nc)), name
    else:
        assert np.all(np.isnan(got["auroc"])) and np.all(got["log_pvalue"] == 0) and np.all(got["log_padj"] == 0), name
    tol = em.log_tolerance(max(Np + Nc, 1))
    worst = [float(np.max(np.abs(got[f] - want[f]), initial=0.0)) for f in ("log_pvalue", "log_padj")]
    print("%s: N = %d, largest |log_pvalue - model| = %.3g, |log_padj - model| = %.3g (allowed %.3g)" % (
        name, Np + Nc, worst[0], worst[1], tol))
    assert worst[0] <= tol and worst[1] <= tol, name
    # without tails the outputs are the same
    again = enrichment_test(dev, torch.from_numpy(labels).cuda())
    for f in ("best_pattern", "tp", "log_pvalue", "log_padj"):
        assert np.array_equal(again[f].cpu().numpy(), got[f]), (name, f)
    return worst


@pytest.mark.parametrize("seed", range(5))
def test_enrichment_test_half_normal(seed):
    bits, labels = em.half_normal_case(seed=seed)
    _check_test(bits, labels, "60 + 90, seed %d" % seed)


def test_enrichment_test_synthetic():
    for name, (bits, labels) in em.synthetic_cases().items():
        _check_test(bits, labels, name)
    from explainn_amd.enrichment import enrichment_test
    # no record at all, and more units than workgroups of a call
    out = enrichment_test(torch.zeros((3, 0), dtype=torch.int16, device="cuda"),
                          torch.zeros(0, dtype=torch.uint8, device="cuda"))
    assert not out["n_thresholds"].any() and not out["best_pattern"].any() and torch.isnan(out["auroc"]).all()
    _check_test(*em.many_units_case(), "300 units")


def test_enrichment_test_on_device_scores():
    """2000 + 3000 records of 40 bases, scored on the device: the test's input is record_best's output."""
    from explainn_amd import ExplaiNN
    from explainn_amd.enrichment import _device_best
    U, k, L = 3, 8, 40
    sd = orc.random_state_dict(U, k, L, 1, seed=11)
    net = ExplaiNN(U, k, L, 1)
    net.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    net.cuda().eval()
    recs = kmer_records(2000, 3000, L, sd, k, 11)
    bits, _ = _device_best(net, recs, 2, None, False)
    assert net.input_flags() == 0
    bits = bits.cpu().numpy().view(np.uint16)
    labels = em_labels(2000, 3000)
    _check_test(bits, labels, "2000 + 3000")
    assert em.unit_stats(bits[0], labels)["log_pvalue"] < -50       # the planted k-mer of unit 0


# ------------------------------------------------------------------------------------------- end to end
def _planted(net, unit, n=300, L=100, seed=21):
    """Records of which 60 % carry the k-mer unit `unit` likes best (the argmax base of every tap)."""
    g = np.random.default_rng(seed)
    k = net._options["kernel_size"]
    w = net.linears[0].weight.detach().cpu().numpy()[unit]                   # (4, k)
    sign = float(net.linears[1].weight.detach().cpu().numpy()[unit])
    kmer = (np.argmax(w, axis=0) if sign > 0 else np.argmin(w, axis=0)).astype(np.uint8)
    recs = [g.integers(0, 4, size=L).astype(np.uint8) for _ in range(n)]
    for r in np.flatnonzero(g.random(n) < 0.6):
        p = int(g.integers(0, L - k + 1))
        recs[r][p:p + k] = kmer
    return recs


def test_planted_motif_end_to_end(tmp_path):
    from explainn_amd import enrichment as en
    net = _net(8, 19, 200, seed=8)
    unit = 5
    recs = _planted(net, unit)
    res = en.enrichment(net, recs, shuffles=2, seed=3)
    assert res.units == 8 and list(res.counts) == [300, 600]
    assert int(np.argmin(res.log_pvalue)) == unit and res.qvalue[unit] < 0.05 and res.auroc[unit] > 0.7
    assert res.log_pvalue[unit] < -50 and res.enrichment[unit] > 5
    again = en.enrichment(net, recs, shuffles=2, seed=3)
    for f in en._FIELDS + ("counts", "qvalue", "evalue", "threshold", "enrichment"):
        assert np.array_equal(getattr(again, f), getattr(res, f), equal_nan=f == "auroc"), f
    other = en.enrichment(net, recs, shuffles=2, seed=4)
    assert not np.array_equal(other.fp, res.fp) or not np.array_equal(other.u2, res.u2)
    # an explicit control of other lengths, with records too short to hold a site
    control = [_codes(n, 500 + n) for n in (150, 90, 18, 120)] * 20
    mixed = en.enrichment(net, recs + [np.zeros(5, np.uint8)], control)
    assert list(mixed.counts) == [300, 60] and int(np.argmin(mixed.log_pvalue)) == unit
    # the command line: the planted filter leads the table
    ckpt, fa, out, npz = (os.path.join(tmp_path, n) for n in ("model.pth.tar", "peaks.fa", "out.tsv", "best.npz"))
    torch.save({"options": dict(net._options), "state_dict": {key: v.cpu() for key, v in net.state_dict().items()}}, ckpt)
    with open(fa, "w") as fh:
        for i, codes in enumerate(recs):
            fh.write(">peak%d\n%s\n" % (i, "".join("ACGTN"[c] for c in codes)))
    en.main([ckpt, fa, "--shuffles", "2", "--seed", "3", "--save-best", npz, "-o", out])
    lines = open(out).read().splitlines()
    assert lines[0].split("\t") == list(en.COLUMNS)
    first = lines[1].split("\t")
    assert first[0] == "filter%d" % unit and int(first[2]) == int(res.tp[unit]) and int(first[4]) == int(res.fp[unit])
    assert float(first[7]) == float("%.6g" % res.log_pvalue[unit])
    lp = [float(ln.split("\t")[7]) for ln in lines[1:]]
    assert lp == sorted(lp)
    best = en.RecordBest.load(npz)
    assert np.array_equal(best.bits, en.best_sites(net, recs).bits) and best.ids[0] == "peak0"
