"""CPU, fp64: the sync-BN exchanges (tests/syncbn_model.py, the algebra of csrc/syncbn.hip) summed
over R shards -- uneven ones and shards of one sequence included -- give the full batch's BatchNorm
statistics to 1e-10 relative; the per-shard statistics do not."""
import numpy as np
import pytest

from conftest import Golden
from oracle import explainn_oracle as orc
import syncbn_model as sm


def _bounds(B, R):
    base, extra = divmod(B, R)
    out, lo = [], 0
    for r in range(R):
        hi = lo + base + (1 if r < extra else 0)
        out.append((lo, hi))
        lo = hi
    return out


def _full(name):
    g = Golden(name)
    sd = g.sd()
    x = g.onehot().astype(np.float64)
    _, cache, _ = orc.forward(sd, x, training=True, return_cache=True, dtype=np.float64)
    U = cache["V2"].shape[0]
    z = np.einsum("bur,ur->bu", cache["a"].reshape(x.shape[0], U, -1), cache["V2"])
    d3 = np.random.default_rng(0).standard_normal(z.shape) * (cache["y3"] > 0)
    return g, sd, x, cache, z, d3


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _truth(g, sd, x, cache, z, d3):
    B, L, k = x.shape[0], x.shape[2], g.k
    W = np.asarray(sd["linears.0.weight"], np.float64)
    cb = np.asarray(sd["linears.0.bias"], np.float64)
    c = cache["c"]                                   # conv output (B, U, Lo), bias included
    bn1 = [(c[:, u].mean() - cb[u], c[:, u].var()) for u in range(W.shape[0])]
    q = cache["q"]
    bn2 = [(q[:, u].mean(0), np.cov(q[:, u].T, bias=True)) for u in range(q.shape[1])]
    bn3 = (z.mean(0), z.var(0))
    head = (d3.sum(0), (d3 * cache["zhat"]).sum(0))
    return bn1, bn2, bn3, head, W, L - k + 1


def _derive(parts, W, B, Lo):
    X = sm.add(parts)
    bn1, bn2, bn3 = sm.statistics(X, B, Lo, W)
    return bn1, bn2, bn3, X["X4"]


CASES = [("tiny_u1_k5", 2), ("tiny_u3_k5_N", 3), ("small_u8_k19", 2), ("small_u8_k19", 3),
         ("small_u8_k19", 4), ("c1_u100_k19_L200", 3)]


@pytest.mark.parametrize("name,R", CASES)
def test_summed_exchanges_give_full_batch_statistics(name, R):
    g, sd, x, cache, z, d3 = _full(name)
    B = x.shape[0]
    bn1_t, bn2_t, bn3_t, head_t, W, Lo = _truth(g, sd, x, cache, z, d3)
    bounds = _bounds(B, R)
    if name == "tiny_u1_k5":
        assert min(hi - lo for lo, hi in bounds) == 1      # shards of one sequence
    parts = [sm.shard_exchanges(x[lo:hi], cache["q"][lo:hi], z[lo:hi], cache["zhat"][lo:hi],
                                d3[lo:hi], g.k) for lo, hi in bounds]
    bn1, bn2, bn3, head = _derive(parts, W, B, Lo)
    # the pair counts are integers: exact
    C, c = parts[0]["X1"]
    assert np.array_equal(C, np.rint(C)) and np.array_equal(c, np.rint(c))
    for (m, v), (mt, vt) in zip(bn1, bn1_t):
        assert abs(m - mt) <= 1e-10 * max(abs(mt), 1.0) and abs(v - vt) <= 1e-10 * vt
    for (m, cv), (mt, cvt) in zip(bn2, bn2_t):
        assert _rel(m, mt) < 1e-10 and _rel(cv, cvt) < 1e-10
    assert _rel(bn3[0], bn3_t[0]) < 1e-10 and _rel(bn3[1], bn3_t[1]) < 1e-10
    assert _rel(head[0], head_t[0]) < 1e-10 and _rel(head[1], head_t[1]) < 1e-10


def test_per_shard_statistics_do_not_match():
    """What per-shard BatchNorm uses -- each shard's own statistics -- is not the full batch's."""
    g, sd, x, cache, z, d3 = _full("small_u8_k19")
    B = x.shape[0]
    bn1_t, bn2_t, bn3_t, _, W, Lo = _truth(g, sd, x, cache, z, d3)
    lo, hi = _bounds(B, 2)[0]
    part = sm.shard_exchanges(x[lo:hi], cache["q"][lo:hi], z[lo:hi], cache["zhat"][lo:hi], d3[lo:hi], g.k)
    bn1, bn2, bn3, _ = _derive([part], W, hi - lo, Lo)
    assert max(abs(v - vt) / vt for (_, v), (_, vt) in zip(bn1, bn1_t)) > 1e-3
    assert max(_rel(cv, cvt) for (_, cv), (_, cvt) in zip(bn2, bn2_t)) > 1e-3
    assert _rel(bn3[1], bn3_t[1]) > 1e-3


def test_shift_conversion_is_an_identity():
    """Sums about different per-shard shifts cannot be added; converted to sums about zero they can."""
    rng = np.random.default_rng(3)
    q = rng.random((37, 6)) * 5 + 100.0
    parts = []
    for lo, hi in _bounds(37, 4):
        S1, S2 = sm.qmoments_about(q[lo:hi], q[lo])
        parts.append(sm.to_zero(S1, S2, q[lo], hi - lo))
    Sq = sum(p[0] for p in parts)
    Sqq = sum(p[1] for p in parts)
    assert _rel(Sq, q.sum(0)) < 1e-13 and _rel(Sqq, q.T @ q) < 1e-13
    # adding the raw shifted sums instead is wrong
    raw = sum(sm.qmoments_about(q[lo:hi], q[lo])[1] for lo, hi in _bounds(37, 4))
    mean = q.mean(0)
    assert _rel(raw / 37, (q - mean).T @ (q - mean) / 37) > 1e-2
