"""GPU: the one promise of csrc/codescan.h, stated in one place -- a unit's eval-mode activation at a start
position is the same float16 bit pattern whichever kernel computes it: sites_kernel (call_sites),
act_hist_kernel (activation_histogram), record_best_kernel (record_best) and interpret.hip's site_kernel
(filter_act_max / filter_sites).  The kernels are compared with each other on one seeded input; everything
compared is an integer or a bit pattern, so every assertion is exact equality.  The fp64 oracle is used for
one thing: no activation of the input is 0, so a threshold of 0 makes every live start a site."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sites_model as sm  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDS = 37
CASES = [(5, 5, 23), (8, 19, 40)]          # (U, k, period): a ragged last quad and k < 7; the headline k


def make_input(U, k, period, seed=7):
    """(state dict, codes (RECORDS * period,) uint8 with about 5 % N).  BatchNorm1 is scaled so that
    alpha * sum + shift spreads over several units of e: the float16 patterns of exp(.) cover several
    binades, none of them 0 or inf."""
    g = np.random.default_rng(seed + 1000 * k)
    sd = orc.random_state_dict(U, k, period, 1, seed=seed)
    sd["linears.0.weight"] = g.normal(0.0, 0.3, size=(U, 4, k)).astype(np.float32)
    sd["linears.0.bias"] = g.normal(0.0, 0.2, size=U).astype(np.float32)
    sd["linears.1.weight"] = (g.uniform(0.5, 1.2, size=U) * g.choice([-1.0, 1.0], size=U)).astype(np.float32)
    sd["linears.1.bias"] = g.uniform(-1.0, 1.0, size=U).astype(np.float32)
    sd["linears.1.running_mean"] = g.normal(0.0, 0.3, size=U).astype(np.float32)
    sd["linears.1.running_var"] = g.uniform(0.8, 2.0, size=U).astype(np.float32)
    codes = g.integers(0, 4, size=RECORDS * period).astype(np.uint8)
    codes[g.random(codes.size) < 0.05] = 4
    return sd, codes


def oracle_acts(sd, codes, period):
    """fp64 (2, RECORDS, U, period - k + 1): the activations of the records and of their reverse complements."""
    rows = codes.reshape(RECORDS, period)
    return np.stack([orc.unit_activations(sd, sm.onehot(r).astype(np.float64), dtype=np.float64)
                     for r in (rows, sm.rc_codes(rows))])


def test_input_has_no_zero_activation():
    """(CPU arithmetic only.)  Every activation rounds to a finite, non-zero float16, with room to spare for
    the kernels' fp32 rounding, and the input spreads over many patterns."""
    for U, k, period in CASES:
        sd, codes = make_input(U, k, period)
        a = oracle_acts(sd, codes, period)
        assert a.min() > 2.0 ** -13 and a.max() < 2.0 ** 15, (k, a.min(), a.max())
        assert len(np.unique(a.astype(np.float16))) > 1000, k


def _bits(score):
    s16 = score.astype(np.float16)
    assert np.array_equal(s16.astype(np.float32), score)            # the scores are float16 values
    return s16.view(np.uint16)


@functools.lru_cache(maxsize=None)
def _run(U, k, period):
    """Every kernel once on the case's input; shared by the tests below and not modified by them."""
    from explainn_amd import ExplaiNN, _lib
    sd, codes = make_input(U, k, period)
    net = ExplaiNN(U, k, period, 1)
    net.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    net.cuda().eval()
    dev = torch.from_numpy(codes).cuda()
    n_pos = codes.size - k + 1
    live = np.flatnonzero(sm.period_mask(n_pos, period, k))
    zero = torch.zeros(U, device="cuda", dtype=torch.float32)
    out = {"net": net, "codes": dev, "live": live, "bits": {}, "hist": {}}
    for rc in (False, True):
        offsets, pos, score = net._launch_call_sites(dev, zero, period=period, reverse_complement=rc,
                                                     capacity=U * n_pos)
        offsets, pos, score = offsets.cpu().numpy(), pos.cpu().numpy(), score.cpu().numpy()
        # a threshold of 0: every live start of every unit, in ascending position
        assert np.array_equal(offsets, np.arange(U + 1) * len(live))
        assert np.array_equal(pos[:offsets[-1]].reshape(U, -1), np.tile(live, (U, 1)))
        out["bits"][rc] = _bits(score[:offsets[-1]]).reshape(U, RECORDS, period - k + 1)
        hist = torch.zeros(U, _lib.ACT_BINS, device="cuda", dtype=torch.int64)
        out["hist"][rc] = net._launch_activation_histogram(dev, hist, period=period, reverse_complement=rc).cpu().numpy()
    assert net.input_flags() == 0
    return out


@pytest.mark.parametrize("U,k,period", CASES)
def test_histogram_is_the_multiset_of_site_scores(U, k, period):
    r = _run(U, k, period)
    for rc in (False, True):
        bits = r["bits"][rc]
        assert bits.max() < 0x7C00 and bits.min() > 0
        for u in range(U):
            assert np.array_equal(r["hist"][rc][u], np.bincount(bits[u].ravel(), minlength=r["hist"][rc].shape[1])), (rc, u)


@pytest.mark.parametrize("U,k,period", CASES)
def test_record_best_is_the_maximum_of_site_scores(U, k, period):
    """Ties go to the lowest start, and '+' comes before '-'."""
    r = _run(U, k, period)
    off = torch.arange(RECORDS + 1, dtype=torch.int64, device="cuda") * period
    fwd, rev = r["bits"][False].astype(np.int64), r["bits"][True].astype(np.int64)      # (U, RECORDS, starts)
    for strands in (2, 1):
        bits, site = r["net"]._launch_record_best(r["codes"], off, strands)
        bits, site = bits.cpu().numpy().view(np.uint16), site.cpu().numpy()
        # per start the better strand ('+' on a tie), then the first start that holds the maximum
        both = np.maximum(fwd, rev) if strands == 2 else fwd
        minus = (rev > fwd).astype(np.int64) if strands == 2 else np.zeros_like(fwd)
        start = both.argmax(axis=2)
        assert np.array_equal(bits, both.max(axis=2)), strands
        assert np.array_equal(site, (start << 1) | np.take_along_axis(minus, start[..., None], axis=2)[..., 0]), strands


@pytest.mark.parametrize("U,k,period", CASES)
def test_batch_export_sees_the_same_activations(U, k, period):
    """The records as a (RECORDS, period) batch through interpret.hip's site_kernel: the per-unit maximum, and
    the site count at a threshold inside the unit's range, are those of call_sites."""
    from explainn_amd.architectures import BaseCodes
    r = _run(U, k, period)
    net, batch = r["net"], r["codes"].reshape(RECORDS, period)
    for rc in (False, True):
        bits = r["bits"][rc].reshape(U, -1)
        x = BaseCodes(batch, rc)
        umax = net.filter_act_max(x, torch.zeros(U, device="cuda", dtype=torch.float32)).cpu().numpy()
        assert np.array_equal(_bits(umax), bits.max(axis=1)), rc
        # an arbitrary in-range threshold: the unit's median score
        thr = np.sort(bits, axis=1)[:, bits.shape[1] // 2].astype(np.uint16).view(np.float16).astype(np.float32)
        thr_dev = torch.from_numpy(thr).cuda()
        offsets, _, _ = net._launch_call_sites(r["codes"], thr_dev, period=period, reverse_complement=rc)
        counts = np.diff(offsets.cpu().numpy())
        assert np.array_equal(counts, (bits > thr.astype(np.float16).view(np.uint16)[:, None]).sum(axis=1)), rc
        assert counts.min() > 0 and counts.max() < bits.shape[1]
        total = torch.zeros(U, device="cuda", dtype=torch.int32)
        pfm = torch.zeros(U, k, 4, device="cuda", dtype=torch.int32)
        net.filter_sites(x, thr_dev, total, pfm)
        assert np.array_equal(total.cpu().numpy(), counts), rc
    assert net.input_flags() == 0
