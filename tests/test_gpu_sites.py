"""GPU: motif-site calling (csrc/sites.hip through explainn_call_sites, explainn_amd/sites.py and
interpret.filter_site_list) against a dense recount of float16(model.linears[:3]) on the materialised
windows, the reference-fed PFM fixtures and the numpy oracle.  Comparisons are exact (array_equal)
unless a test says otherwise."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sites_model as sm  # noqa: E402
from test_interpret_oracle import PFM_CASES, load  # noqa: E402
from oracle import interpret_oracle as io  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 60), (5, 19, 200), (7, 32, 200)]


def _tile():
    from explainn_amd import _lib
    return _lib.SITES_TILE


def _net(U, k, L, seed=0):
    from explainn_amd import ExplaiNN
    torch.manual_seed(seed)
    return ExplaiNN(U, k, L, 1).cuda().eval()


def _codes(n, seed, n_frac=0.01):
    g = np.random.default_rng(seed)
    c = g.integers(0, 4, size=n).astype(np.uint8)
    c[g.random(n) < n_frac] = 4
    return c


def _windows(codes, L, k):
    """Window starts (stride Lo, the last one pulled back to end at the sequence's end) and the (W,L)
    window matrix: together the windows hold every k-mer of the sequence."""
    Lo = L - k + 1
    starts = sorted(set(list(range(0, len(codes) - L + 1, Lo)) + [len(codes) - L]))
    return np.array(starts), np.stack([codes[s:s + L] for s in starts])


def _flatten(starts, acts16, P):
    """(W,U,Lo) window activations -> (U,P) per sequence position; where windows overlap the values
    are the same bits (asserted)."""
    W, U, Lo = acts16.shape
    flat = np.zeros((U, P), dtype=np.float16)
    seen = np.zeros(P, dtype=bool)
    for s, a in zip(starts, acts16):
        old = seen[s:s + Lo]
        assert np.array_equal(flat[:, s:s + Lo][:, old], a[:, old])
        flat[:, s:s + Lo] = a
        seen[s:s + Lo] = True
    assert seen.all()
    return flat


def _dense(net, codes, reverse=False):
    """float16(linears[:3]) of the materialised windows of one sequence, per forward position; reverse:
    of the windows of the reverse-complemented sequence, mapped back (p = len - k - p')."""
    o = net._options
    L, k = o["sequence_length"], o["kernel_size"]
    seq = sm.rc_codes(codes) if reverse else codes
    starts, win = _windows(seq, L, k)
    with torch.no_grad():
        acts = net.linears[:3](torch.from_numpy(sm.onehot(win)).cuda()).cpu().numpy().astype(np.float16)
    flat = _flatten(starts, acts, len(codes) - k + 1)
    return flat[:, ::-1] if reverse else flat


def _thresholds(flat, special=True):
    thr = (0.5 * flat.max(axis=1)).astype(np.float16).astype(np.float32)
    if special:
        thr[0] = -1.0                       # a site everywhere
        thr[1] = np.inf                     # never a site
    return thr


def _expect(calls, fwd, rev, thr):
    """calls (SiteCalls) holds exactly the dense recount: per unit '+' ascending, then '-' ascending."""
    total = 0
    for u in range(len(thr)):
        start, strand, score = calls.unit(u)
        want = [(fwd, 1)] + ([(rev, -1)] if rev is not None else [])
        pos = [np.flatnonzero(f[u] > thr[u]) for f, _ in want]
        assert np.array_equal(start, np.concatenate(pos)), u
        assert np.array_equal(strand, np.concatenate([np.full(len(p), s, np.int8) for p, (_, s) in zip(pos, want)])), u
        assert np.array_equal(score, np.concatenate([f[u, p].astype(np.float32) for p, (f, _) in zip(pos, want)])), u
        total += len(start)
    assert len(calls) == total
    return total


@pytest.mark.parametrize("U,k,L", SHAPES)
def test_dense_recount_one_sequence(U, k, L):
    """Sequence ends just inside a tile, k - 1 past it and in a fourth tile; 1 % N; one unit a site
    everywhere, one never; both strands; sites whose k-mer straddles a tile boundary are present."""
    from explainn_amd.sites import call_sites
    tile = _tile()
    net = _net(U, k, L, seed=U)
    for n_pos in (tile - 1, tile + k - 1, 3 * tile + 17):
        codes = _codes(n_pos + k - 1, seed=n_pos)
        fwd, rev = _dense(net, codes), _dense(net, codes, reverse=True)
        thr = _thresholds(fwd)
        calls = call_sites(net, codes, thr)
        assert calls.units == U and calls.kernel_size == k
        _expect(calls, fwd, rev, thr)
        assert len(calls.unit(0)[0]) == 2 * n_pos and len(calls.unit(1)[0]) == 0
        if n_pos > tile:
            p = calls.unit(2)[0]
            assert ((p % tile) + k > tile).any(), "no site straddles a tile boundary"
        # forward strand alone
        _expect(call_sites(net, torch.from_numpy(codes).cuda(), thr, strands="fwd"), fwd, None, thr)


def test_chunking_equals_one_call():
    from explainn_amd.sites import call_sites
    tile = _tile()
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=1)
    codes = _codes(3 * tile + 17 + k - 1, seed=11)
    thr = _thresholds(_dense(net, codes))
    whole = call_sites(net, codes, thr)
    assert len(whole) > 0
    for chunk in (tile, tile + 5):
        part = call_sites(net, codes, thr, chunk_positions=chunk)
        for name in ("offsets", "start", "strand", "score"):
            assert np.array_equal(getattr(part, name), getattr(whole, name)), (chunk, name)


def test_capacity_truncates_and_leaves_the_rest_untouched():
    tile = _tile()
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=2)
    codes = _codes(2 * tile + 40, seed=12)
    dev = torch.from_numpy(codes).cuda()
    thr = torch.from_numpy(_thresholds(_dense(net, codes))).cuda()
    off, _, _ = net._launch_call_sites(dev, thr)
    total = int(off[-1])
    _, pos, score = net._launch_call_sites(dev, thr, capacity=total)
    cap = total // 2 + 3
    assert 0 < cap < total
    pos2 = torch.full((total,), -7, dtype=torch.int32).cuda()
    score2 = torch.full((total,), -7.0, dtype=torch.float32).cuda()
    off2, _, _ = net._launch_call_sites(dev, thr, capacity=cap, pos=pos2, score=score2)
    assert torch.equal(off2, off)
    assert torch.equal(pos2[:cap], pos[:cap]) and torch.equal(score2[:cap], score[:cap])
    assert (pos2[cap:] == -7).all() and (score2[cap:] == -7.0).all()
    # a sub-range: start-relative positions of the same sites
    s0, n = tile - 3, tile // 2
    o3, p3, _ = net._launch_call_sites(dev, thr, start=s0, n_positions=n, capacity=total)
    o3, p3, off_h, pos_h = o3.cpu().numpy(), p3.cpu().numpy(), off.cpu().numpy(), pos.cpu().numpy()
    for u in range(U):
        full = pos_h[off_h[u]:off_h[u + 1]]
        assert np.array_equal(p3[o3[u]:o3[u + 1]] + s0, full[(full >= s0) & (full < s0 + n)])


@pytest.mark.parametrize("name", PFM_CASES)
def test_golden_pfms_from_site_lists(name):
    """The period path against reference-generated numbers: the PFM and nsites recounted from
    filter_site_list equal the fixture's and filter_pwms' on the same model."""
    from explainn_amd import interpret as it
    from test_gpu_interpret import _model
    z, m = load(name)
    net = _model(z, m)
    x = sm.onehot(z["codes"])
    lists = it.filter_site_list(net, x, z["idxs"], z["thresholds"], m["rc"], site_cap=m["cap"])
    pfm, nsites = sm.pfm_from_lists(z["codes"], lists, m["k"], m["rc"])
    assert np.array_equal(nsites, z["nsites"]) and np.array_equal(pfm, z["pfm"])
    res = it.filter_pwms(net, x, z["idxs"], m["rc"], site_cap=m["cap"])
    assert np.array_equal(res["thresholds"], z["thresholds"])
    assert np.array_equal(nsites, res["nsites"]) and np.array_equal(pfm, res["pfm"])


def test_large_shape_several_tiles():
    """300 units x 4 000 positions: 75 unit quads, four tiles, the last one ragged."""
    from explainn_amd.sites import call_sites
    U, k, L = 300, 19, 200
    net = _net(U, k, L, seed=3)
    codes = _codes(4000 + k - 1, seed=13)
    fwd, rev = _dense(net, codes), _dense(net, codes, reverse=True)
    thr = _thresholds(fwd)
    total = _expect(call_sites(net, codes, thr), fwd, rev, thr)
    assert total > 2 * 4000


def test_ragged_last_quad():
    """A unit count that is no multiple of 4: the last workgroup row holds one live unit."""
    from explainn_amd.sites import call_sites
    U, k, L = 9, 19, 200
    net = _net(U, k, L, seed=4)
    codes = _codes(_tile() + 300, seed=14)
    fwd, rev = _dense(net, codes), _dense(net, codes, reverse=True)
    thr = _thresholds(fwd, special=False)
    assert _expect(call_sites(net, codes, thr), fwd, rev, thr) > 0


def test_bank_equals_its_members():
    from explainn_amd import ExplaiNNBank
    from explainn_amd.sites import call_sites
    k, L = 19, 200
    a, b = _net(5, k, L, seed=5), _net(5, k, L, seed=6)
    bank = ExplaiNNBank.from_models([a.cpu(), b.cpu()]).cuda().eval()
    a, b = a.cuda().eval(), b.cuda().eval()
    codes = _codes(_tile() + 500, seed=15)
    thr_a, thr_b = _thresholds(_dense(a, codes), special=False), _thresholds(_dense(b, codes), special=False)
    got = call_sites(bank, codes, np.concatenate([thr_a, thr_b]))
    assert got.units == 10
    for g, (m, thr) in enumerate(((a, thr_a), (b, thr_b))):
        one = call_sites(m, codes, thr)
        assert len(one) > 0
        for u in range(5):
            for x, y in zip(got.unit(5 * g + u), one.unit(u)):
                assert np.array_equal(x, y), (g, u)


@pytest.mark.parametrize("U,k,L", [(5, 19, 200), (7, 32, 200), (300, 19, 200)])
def test_classification_against_the_numpy_oracle(U, k, L):
    """Independent of the device's own dense export: the oracle's float16 activations
    (interpret_oracle.acts_outs_preds on the materialised windows) with thresholds at half the unit's
    maximum.  Every (unit, position) whose oracle activation differs from the threshold by more than
    2 float16 ulps is classified identically; positions within 2 ulps may fall either way and must be
    at most 1 % of all (0.2 - 0.3 % on these shapes, worked out on the CPU)."""
    from explainn_amd.sites import call_sites
    net = _net(U, k, L, seed=7)
    sd = {key: v.detach().cpu().numpy() for key, v in net.state_dict().items()}
    codes = _codes(_tile() + 700, seed=16)
    P = len(codes) - k + 1
    starts, win = _windows(codes, L, k)
    acts = io.acts_outs_preds(sd, sm.onehot(win))[0]
    flat = np.zeros((U, P), dtype=np.float16)
    for s, a in zip(starts, acts):
        flat[:, s:s + a.shape[1]] = a
    thr16 = (0.5 * flat.max(axis=1)).astype(np.float16)
    calls = call_sites(net, codes, thr16.astype(np.float32), strands="fwd")
    got = np.zeros((U, P), dtype=bool)
    got[calls.unit_ids(), calls.start] = True
    ulp = np.spacing(np.abs(thr16)).astype(np.float64)[:, None]
    decided = np.abs(flat.astype(np.float64) - thr16.astype(np.float64)[:, None]) > 2 * ulp
    share = 1.0 - decided.mean()
    print("undecided share %.4f %%, sites %d" % (100 * share, got.sum()))
    assert np.array_equal(got[decided], (flat > thr16[:, None])[decided])
    assert share <= 0.01
    assert got.any() and not got.all()


def test_errors_and_input_flag():
    from explainn_amd import _lib
    from explainn_amd.sites import call_sites
    U, k, L = 4, 5, 30
    net = _net(U, k, L, seed=8)
    codes = _codes(300, seed=17, n_frac=0.0)
    dev = torch.from_numpy(codes).cuda()
    thr = torch.full((U,), 0.5, dtype=torch.float32).cuda()
    with pytest.raises(_lib.ExplainnError, match=r"code -1"):
        net._launch_call_sites(dev, thr, start=0, n_positions=len(codes) - k + 2)      # overhangs by one
    with pytest.raises(_lib.ExplainnError, match=r"code -1"):
        net._launch_call_sites(dev, thr, start=-1, n_positions=10)
    off, _, _ = net._launch_call_sites(dev, thr, start=0, n_positions=len(codes) - k + 1)   # the last legal range
    assert off.shape == (U + 1,)
    with pytest.raises(RuntimeError):
        net._launch_call_sites(dev, thr[:3].contiguous())
    with pytest.raises(RuntimeError):
        call_sites(net, codes, np.zeros(U + 1))
    with pytest.raises(NotImplementedError):
        net.train()._launch_call_sites(dev, thr)
    with pytest.raises(NotImplementedError):
        call_sites(net, codes, np.zeros(U))
    net.eval()
    with pytest.raises(ValueError, match=r"max_sites.*filter\d+"):
        call_sites(net, codes, np.zeros(U), max_sites=100)             # threshold 0: every position
    assert net.input_flags() == 0
    bad = codes.copy()
    bad[150] = 9
    off_bad, _, _ = net._launch_call_sites(torch.from_numpy(bad).cuda(), thr)
    assert net.input_flags() & 1
    assert net.input_flags() == 0                                      # read and cleared
    # the byte read as N
    bad[150] = 4
    off_n, _, _ = net._launch_call_sites(torch.from_numpy(bad).cuda(), thr)
    assert torch.equal(off_bad, off_n)
    with pytest.raises(ValueError, match="one-hot|base codes"):
        bad[150] = 200
        call_sites(net, bad, thr.cpu().numpy())
    # a sequence shorter than the filter has no start at all
    empty = call_sites(net, codes[:k - 1], thr.cpu().numpy())
    assert len(empty) == 0 and np.array_equal(empty.offsets, np.zeros(U + 1, np.int64))


def test_eval_tables_follow_the_parameters():
    """Like every eval entry point the call rebuilds the folded tables when the parameters moved, and
    leaves the model usable for an ordinary forward."""
    from explainn_amd.sites import call_sites
    U, k, L = 5, 19, 200
    net = _net(U, k, L, seed=9)
    codes = _codes(_tile() + 100, seed=18)
    thr = _thresholds(_dense(net, codes), special=False)
    first = call_sites(net, codes, thr, strands="fwd")
    with torch.no_grad():
        net.linears[0].weight.mul_(1.5)
    fwd = _dense(net, codes)
    second = call_sites(net, codes, thr, strands="fwd")
    _expect(second, fwd, None, thr)
    assert not np.array_equal(first.offsets, second.offsets)
    x = torch.from_numpy(sm.onehot(_windows(codes, L, k)[1])).cuda()
    assert torch.isfinite(net(x)).all()
