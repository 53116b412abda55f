"""GPU: the empirical null of the filter activations (csrc/actnull.hip through
explainn_activation_histogram / explainn_activation_null, sites.activation_null, sites.ActivationNull,
`python -m explainn_amd.calibrate` and `sites --null`) against a dense recount of
float16(model.linears[:3]) on the materialised windows and the numpy model tests/actnull_model.py.
Comparisons are exact (array_equal) unless a test says otherwise."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import actnull_model as am  # noqa: E402
import sites_model as sm  # noqa: E402
from test_gpu_sites import _codes, _dense, _net  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 60), (5, 19, 200), (7, 32, 200)]


def _span():
    from explainn_amd import _lib
    return _lib.ACT_SPAN


def _saturate(net):
    """Unit 0 always +inf (bin 0x7C00), unit 1 always 0 (bin 0): BatchNorm1's bias at +40 / -40."""
    with torch.no_grad():
        net.linears[1].bias[0] = 40.0
        net.linears[1].bias[1] = -40.0
    return net


def _zeros(units):
    return torch.zeros(units, am.BINS, dtype=torch.int64, device="cuda")


def _hist(net, codes, reverse=False, period=0, hist=None, **kw):
    """One explainn_activation_histogram call over a whole host sequence."""
    dev = torch.from_numpy(np.ascontiguousarray(codes)).cuda()
    hist = _zeros(net._units()) if hist is None else hist
    net._launch_activation_histogram(dev, hist, period=period, reverse_complement=reverse, **kw)
    return hist.cpu().numpy()


def _dense_rows(net, rows, reverse=False):
    """float16 (U, N*Lo) activations of the rows of an (N,L) matrix (of their reverse complements)."""
    x = sm.onehot(sm.rc_codes(rows) if reverse else rows)
    with torch.no_grad():
        a = net.linears[:3](torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float16)
    return a.transpose(1, 0, 2).reshape(a.shape[1], -1)


@pytest.mark.parametrize("U,k,L", SHAPES)
def test_histogram_equals_dense_recount(U, k, L):
    """Sequence ends just inside a span, k - 1 past it and in a fourth span; 1 % N; forward and reverse;
    one unit always +inf, one always 0; every row sums to the number of live positions."""
    span = _span()
    net = _saturate(_net(U, k, L, seed=U))
    for n_pos in (span - 1, span + k - 1, 3 * span + 17):
        codes = _codes(n_pos + k - 1, seed=n_pos)
        for reverse in (False, True):
            want = am.histogram(_dense(net, codes, reverse=reverse))
            got = _hist(net, codes, reverse=reverse)
            for u in range(U):
                assert np.array_equal(got[u], want[u]), (n_pos, reverse, u)
            assert np.array_equal(got.sum(axis=1), np.full(U, n_pos))
            assert got[0, am.INF] == n_pos and got[1, 0] == n_pos
    assert net.input_flags() == 0


@pytest.mark.parametrize("U,k,L", SHAPES)
def test_period_rows_equal_dense_recount(U, k, L):
    """An (N,L) matrix as one sequence with period = L: no k-mer crosses two rows; rows that end in N."""
    from explainn_amd.sites import activation_null
    net = _saturate(_net(U, k, L, seed=10 + U))
    N = (_span() + 3 * L) // L + 1                       # more than one span of starts
    rows = _codes(N * L, seed=31).reshape(N, L)
    rows[::3, -2:] = 4
    rows[1::5, -1] = 4
    Lo = L - k + 1
    fwd, rev = am.histogram(_dense_rows(net, rows)), am.histogram(_dense_rows(net, rows, reverse=True))
    for reverse, want in ((False, fwd), (True, rev)):
        got = _hist(net, rows.reshape(-1), reverse=reverse, period=L)
        assert np.array_equal(got, want), reverse
        assert np.array_equal(got.sum(axis=1), np.full(U, N * Lo))
    null = activation_null(net, rows)                    # (N,L): period = L, both strands
    assert np.array_equal(null.hist.cpu().numpy(), fwd + rev)
    assert np.array_equal(null.total.cpu().numpy(), np.full(U, 2 * N * Lo))


def test_a_block_takes_several_spans():
    """300 units x 6 spans: the spans of a unit are dealt to fewer workgroups than there are spans."""
    U, k, L = 300, 19, 200
    net = _net(U, k, L, seed=3)
    n_pos = 5 * _span() + 3
    codes = _codes(n_pos + k - 1, seed=13)
    got = _hist(net, codes)
    assert np.array_equal(got, am.histogram(_dense(net, codes)))
    assert np.array_equal(got.sum(axis=1), np.full(U, n_pos))


def test_accumulation_and_chunking():
    from explainn_amd.sites import activation_null
    span = _span()
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=1)
    n_pos = 3 * span + 17
    codes = _codes(n_pos + k - 1, seed=11)
    fwd, rev = _hist(net, codes), _hist(net, codes, reverse=True)
    # two halves, overlapping by k - 1 bases, into one histogram; then a range of one buffer
    half = n_pos // 2
    acc = _zeros(U)
    _hist(net, codes[:half + k - 1], hist=acc)
    assert np.array_equal(_hist(net, codes[half:], hist=acc), fwd)
    acc = _zeros(U)
    _hist(net, codes, hist=acc, start=0, n_positions=half)
    assert np.array_equal(_hist(net, codes, hist=acc, start=half, n_positions=n_pos - half), fwd)
    # added into, not overwritten
    pre = torch.full((U, am.BINS), 7, dtype=torch.int64, device="cuda")
    assert np.array_equal(_hist(net, codes, hist=pre), fwd + 7)
    # nothing to count: untouched
    pre = torch.full((U, am.BINS), 7, dtype=torch.int64, device="cuda")
    assert (torch.from_numpy(_hist(net, codes, hist=pre, start=5, n_positions=0)) == 7).all()
    whole = activation_null(net, codes)
    assert np.array_equal(whole.hist.cpu().numpy(), fwd + rev)
    assert np.array_equal(activation_null(net, codes, strands="fwd").hist.cpu().numpy(), fwd)
    for chunk in (span, span + 5):
        part = activation_null(net, torch.from_numpy(codes).cuda(), chunk_positions=chunk)
        assert torch.equal(part.hist, whole.hist), chunk


def test_agrees_with_call_sites_counts():
    """At the reference's 0.5 x max thresholds the count-only call_sites pass and the histogram's bins
    above the threshold count the same sites."""
    U, k, L = 7, 32, 200
    net = _net(U, k, L, seed=2)
    codes = _codes(2 * _span() + 40, seed=12)
    thr = (0.5 * _dense(net, codes).max(axis=1)).astype(np.float16).astype(np.float32)
    dev = torch.from_numpy(codes).cuda()
    for reverse in (False, True):
        off = net._launch_call_sites(dev, torch.from_numpy(thr).cuda(), reverse_complement=reverse)[0].cpu().numpy()
        counts = am.count_above(_hist(net, codes, reverse=reverse), thr)
        assert counts.sum() > 0
        assert np.array_equal(np.diff(off), counts), reverse


@pytest.mark.parametrize("U,k,L", SHAPES)
def test_numpy_model_within_two_ulps(U, k, L):
    """sites_model.kmer_acts uses another exp: the sorted bin lists of the two histograms differ by at
    most 2 bins entry by entry (the 2-ulp rule test_gpu_sites.py applies to the oracle)."""
    net = _net(U, k, L, seed=7)
    sd = {key: v.detach().cpu().numpy() for key, v in net.state_dict().items()}
    codes = _codes(_span() + 700, seed=16)
    for reverse in (False, True):
        want = np.sort(am.bins(sm.kmer_acts(sd, codes, reverse=reverse)), axis=1)
        got = _hist(net, codes, reverse=reverse)
        for u in range(U):
            mine = np.repeat(np.arange(am.BINS), got[u])
            assert len(mine) == want.shape[1]
            worst = int(np.abs(mine - want[u]).max())
            print("unit %d reverse %d: worst bin distance %d" % (u, reverse, worst))
            assert worst <= 2, (u, reverse)


def test_activation_null_kernel_equals_model():
    """tail, total and thresholds at alpha 0, 1e-3, 0.05 and 1, with an all-zero row appended."""
    from explainn_amd import _lib
    from explainn_amd.sites import _null_stats
    U, k, L = 5, 19, 200
    net = _saturate(_net(U, k, L, seed=4))
    codes = _codes(_span() + 500, seed=14)
    h = np.concatenate([_hist(net, codes) + _hist(net, codes, reverse=True), np.zeros((1, am.BINS), np.int64)])
    dev = torch.from_numpy(h).cuda()
    for alpha in (0.0, 1e-3, 0.05, 1.0):
        tail, total, thr = _null_stats(dev, alpha, want_tail=True, want_thresholds=True)
        assert np.array_equal(total.cpu().numpy(), am.total(h))
        assert np.array_equal(tail.cpu().numpy(), am.tail(h))
        want = am.thresholds(h, alpha)
        assert np.array_equal(thr.cpu().numpy(), want), alpha
        assert np.isinf(want[0]) == (alpha < 1.0) and want[1] == 0.0 and np.isinf(want[-1])
    _, total, _ = _null_stats(dev, 0.5)                  # totals alone
    assert np.array_equal(total.cpu().numpy(), am.total(h))
    with pytest.raises(_lib.ExplainnError, match=r"code -1"):
        _null_stats(dev, 1.5)


def test_calibration_is_tight():
    """On the background itself call_sites with thresholds(a) calls at most floor(a * total) positions
    per unit, and more than that with every threshold one float16 step lower."""
    from explainn_amd.sites import activation_null, call_sites
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=5)
    codes = _codes(_span() + 300, seed=15)
    null = activation_null(net, codes)
    total = null.total.cpu().numpy()
    assert np.array_equal(total, np.full(U, 2 * (len(codes) - k + 1)))
    for a in (1e-3, 0.05):
        thr = null.thresholds(a)
        assert thr.dtype == np.float32 and thr.shape == (U,)
        m = np.floor(a * total.astype(np.float64)).astype(np.int64)
        counts = np.diff(call_sites(net, codes, thr).offsets)
        assert np.all(counts <= m), (a, counts, m)
        bits = thr.astype(np.float16).view(np.uint16)
        pos = bits > 0                                   # a threshold of 0 has no float16 value below it
        assert pos.any()
        lower = np.where(pos, bits - 1, bits).astype(np.uint16).view(np.float16).astype(np.float32)
        counts = np.diff(call_sites(net, codes, lower).offsets)
        assert np.all(counts[pos] > m[pos]), (a, counts, m)


def test_shuffle_background():
    from explainn_amd.sequence import dinucleotide_shuffle_device
    from explainn_amd.sites import activation_null
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=6)
    rows = _codes(40 * L, seed=17).reshape(40, L)
    got = activation_null(net, rows, shuffles=3, seed=5)
    shuf = dinucleotide_shuffle_device(torch.from_numpy(rows).cuda(), 3, 5)
    want = activation_null(net, shuf.reshape(-1, L))
    assert torch.equal(got.hist, want.hist)
    assert np.array_equal(got.total.cpu().numpy(), np.full(U, 2 * 40 * 3 * (L - k + 1)))
    for chunk in (7 * L, 16 * L + 3):
        assert torch.equal(activation_null(net, rows, shuffles=3, seed=5, chunk_positions=chunk).hist, got.hist), chunk
    assert not torch.equal(activation_null(net, rows, shuffles=3, seed=6).hist, got.hist)
    with pytest.raises(ValueError):
        activation_null(net, rows.reshape(-1), shuffles=3)                 # no records to shuffle
    with pytest.raises(NotImplementedError):
        activation_null(net.train(), rows)
    net.eval()


def test_pvalues_and_save_load(tmp_path):
    from explainn_amd.sites import ActivationNull, activation_null, bed_rows, call_sites
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=8)
    codes = _codes(_span() + 100, seed=18)
    null = activation_null(net, _codes(3000, seed=19))
    thr = null.thresholds(0.01)
    calls = call_sites(net, codes, thr, null=null)
    assert len(calls) > 0
    h = null.hist.cpu().numpy()
    want = am.pvalue(h, calls.unit_ids(), calls.score)
    assert calls.pvalue.dtype == np.float64 and np.array_equal(calls.pvalue, want)
    assert want.min() >= 1.0 / (1.0 + h.sum(axis=1).max()) and want.max() <= 1.0
    rows = bed_rows("chr1", calls)
    assert all(len(r.rstrip("\n").split("\t")) == 7 for r in rows)
    # without a null: no p-value, and the six columns as ever
    plain = call_sites(net, codes, thr)
    assert plain.pvalue is None
    for name in ("offsets", "start", "strand", "score"):
        assert np.array_equal(getattr(plain, name), getattr(calls, name))
    unit = plain.unit_ids()
    order = np.lexsort((-plain.strand, unit, plain.start))
    assert bed_rows("chr1", plain) == [
        "%s\t%d\t%d\tfilter%d\t%.6g\t%s\n" % ("chr1", plain.start[i], plain.start[i] + k, unit[i], plain.score[i],
                                            "+" if plain.strand[i] > 0 else "-") for i in order]
    assert [r.rsplit("\t", 1)[0] + "\n" for r in rows] == bed_rows("chr1", plain)
    path = os.path.join(tmp_path, "null.npz")
    null.save(path)
    back = ActivationNull.load(path)
    assert torch.equal(back.hist, null.hist) and torch.equal(back.tail, null.tail)
    assert (back.kernel_size, back.strands, back.shuffles, back.seed) == (k, "both", 0, 0)
    with pytest.raises(ValueError):
        call_sites(_net(U + 1, k, L), codes, np.zeros(U + 1), null=null)
    # NaN bins mean non-finite parameters
    bad = null.hist.clone()
    bad[2, am.INF + 5] = 1
    with pytest.raises(ValueError, match="finite"):
        ActivationNull(bad, k)


def test_bank_equals_its_members():
    from explainn_amd import ExplaiNNBank
    from explainn_amd.sites import activation_null
    k, L = 19, 200
    a, b = _net(3, k, L, seed=5), _net(3, k, L, seed=6)
    bank = ExplaiNNBank.from_models([a.cpu(), b.cpu()]).cuda().eval()
    a, b = a.cuda().eval(), b.cuda().eval()
    codes = _codes(_span() + 500, seed=15)
    got = activation_null(bank, codes)
    assert got.units == 6
    for g, m in enumerate((a, b)):
        assert torch.equal(got.hist[3 * g:3 * g + 3], activation_null(m, codes).hist), g


def test_errors_and_input_flag():
    from explainn_amd import _lib
    U, k, L = 4, 5, 30
    net = _net(U, k, L, seed=8)
    codes = _codes(300, seed=17, n_frac=0.0)
    dev = torch.from_numpy(codes).cuda()
    hist = _zeros(U)
    with pytest.raises(_lib.ExplainnError, match=r"code -1"):
        net._launch_activation_histogram(dev, hist, start=0, n_positions=len(codes) - k + 2)   # overhangs by one
    with pytest.raises(_lib.ExplainnError, match=r"code -1"):
        net._launch_activation_histogram(dev, hist, start=-1, n_positions=10)
    with pytest.raises(RuntimeError):
        net._launch_activation_histogram(dev, hist[:3].contiguous())
    with pytest.raises(RuntimeError):
        net._launch_activation_histogram(dev, hist.to(torch.int32))
    with pytest.raises(NotImplementedError):
        net.train()._launch_activation_histogram(dev, hist)
    net.eval()
    assert int(hist.sum()) == 0
    assert net.input_flags() == 0
    bad = codes.copy()
    bad[150] = 9
    got = _hist(net, bad)
    assert net.input_flags() & 1
    bad[150] = 4
    assert np.array_equal(got, _hist(net, bad))          # the byte read as N
    assert net.input_flags() == 0


def test_clis(tmp_path):
    from explainn_amd import calibrate, sites
    U, k, L = 4, 8, 50
    m = _net(U, k, L, seed=9)
    ckpt = os.path.join(tmp_path, "model.pth.tar")
    torch.save({"options": dict(m._options), "state_dict": {key: v.cpu() for key, v in m.state_dict().items()}}, ckpt)
    rows = _codes(30 * L, seed=20).reshape(30, L)
    fa = os.path.join(tmp_path, "seqs.fa")
    with open(fa, "w") as fh:
        for i, row in enumerate(rows):
            fh.write(">s%d desc\n%s\n" % (i, "".join("ACGTN"[c] for c in row)))
    tsv, npz, bed = (os.path.join(tmp_path, n) for n in ("thresholds.tsv", "null.npz", "sites.bed"))
    calibrate.main([ckpt, fa, "-o", tsv, "--pvalue", "0.01", "--shuffles", "4", "--seed", "2", "--save-null", npz])
    null = sites.activation_null(m, rows, shuffles=4, seed=2)
    thr = sites.read_thresholds(tsv, U)
    assert np.array_equal(thr, null.thresholds(0.01))
    assert torch.equal(sites.ActivationNull.load(npz).hist, null.hist)
    calibrate.main([ckpt, fa, "-o", tsv, "--pvalue", "0.02", "--background", "sequence"])
    assert np.array_equal(sites.read_thresholds(tsv, U), sites.activation_null(m, rows).thresholds(0.02))
    sites.main([ckpt, fa, "-t", tsv, "-o", bed, "--null", npz])
    lines = open(bed).read().splitlines()
    assert lines and all(len(ln.split("\t")) == 7 for ln in lines)
    assert all(0.0 < float(ln.split("\t")[6]) <= 1.0 for ln in lines)
    sites.main([ckpt, fa, "-t", tsv, "-o", bed])
    six = open(bed).read().splitlines()
    assert six == [ln.rsplit("\t", 1)[0] for ln in lines]
    # records of unequal lengths: one null over all of them, no k-mer across two records
    ragged = [_codes(n, seed=21 + n) for n in (70, 333, k - 1, 120)]
    fa2 = os.path.join(tmp_path, "ragged.fa")
    with open(fa2, "w") as fh:
        for i, row in enumerate(ragged):
            fh.write(">r%d\n%s\n" % (i, "".join("ACGTN"[c] for c in row)))
    calibrate.main([ckpt, fa2, "-o", tsv, "--pvalue", "0.05", "--background", "sequence", "--save-null", npz])
    want = sum(sites.activation_null(m, row).hist for row in ragged)
    got = sites.ActivationNull.load(npz)
    assert torch.equal(got.hist, want)
    assert np.array_equal(sites.read_thresholds(tsv, U), got.thresholds(0.05))
    with pytest.raises(ValueError, match="period"):
        calibrate.main([ckpt, fa2, "-o", tsv])                       # shuffles need records of one length
