"""The Integrated Gradients algebra (tests/pathgrad_model.py: the path walked in conv-sum space)
against brute force in fp64 -- the mean over the nodes of autograd's x.grad of oracle/torch_ref.py at
the soft input x_a, times (x - x') -- and the host-side dinucleotide shuffle."""
import numpy as np
import pytest

from oracle import explainn_oracle as orc
import pathgrad_model as pm
from pathgrad_model import brute_force


def _case(U, k, L, T, B, seed, nfrac=0.05):
    sd = orc.random_state_dict(U, k, L, T, seed=seed, dtype=np.float64)
    sd["linears.1.weight"][::2] *= -1            # negative gamma1 -> min-pooling branch
    x = orc.random_onehot(B, L, seed=seed + 1, n_frac=nfrac, dtype=np.float64)
    xc = orc.random_onehot(B, L, seed=seed + 7, n_frac=nfrac, dtype=np.float64)
    codes = np.where(xc.sum(axis=1) > 0, xc.argmax(axis=1), 4).astype(np.uint8)
    dl = np.random.default_rng(seed + 2).standard_normal((B, T))
    return sd, x, codes, dl


@pytest.mark.parametrize("U,k,L,T,B,steps,kind", [
    (3, 5, 33, 2, 6, 4, "zero"),
    (5, 19, 61, 3, 8, 7, "codes"),
    (4, 2, 40, 1, 5, 3, "uniform"),
    (2, 7, 47, 2, 6, 1, "codes"),
])
def test_model_equals_brute_force_fp64(U, k, L, T, B, steps, kind):
    sd, x, codes, dl = _case(U, k, L, T, B, seed=U + k)
    base = codes if kind == "codes" else kind
    ig, lx, lb = pm.integrated_gradients(sd, x, base, dl, steps)
    ref, dF = brute_force(sd, x, pm.baseline_dense(base, x), dl, steps)
    assert np.abs(ref).max() > 0
    assert np.abs(ig - ref).max() < 1e-10 * np.abs(ref).max()
    assert np.abs((dl * (lx - lb)).sum(axis=1) - dF).max() < 1e-10 * max(1.0, np.abs(dF).max())
    if kind == "uniform":
        assert (np.abs(ig) > 0).all(axis=1).any()      # all four rows of a position carry attribution


def test_own_sequence_as_baseline_gives_exact_zero():
    sd, x, _, dl = _case(4, 9, 50, 2, 6, seed=3)
    own = np.where(x.sum(axis=1) > 0, x.argmax(axis=1), 4).astype(np.uint8)
    ig, lx, lb = pm.integrated_gradients(sd, x, own, dl, 5)
    assert (ig == 0).all() and np.array_equal(lx, lb)


def test_convergence_residual_shrinks_with_steps():
    sd, x, codes, dl = _case(6, 11, 80, 2, 16, seed=5)
    res = []
    for steps in (8, 64):
        ig, lx, lb = pm.integrated_gradients(sd, x, codes, dl, steps)
        res.append(np.abs(ig.sum(axis=(1, 2)) - (dl * (lx - lb)).sum(axis=1)).mean())
    assert res[1] < res[0], res


def _dinuc(row):
    m = np.zeros((5, 5), dtype=np.int64)
    np.add.at(m, (row[:-1], row[1:]), 1)
    return m


def test_dinucleotide_shuffle():
    from explainn_amd.sequence import dinucleotide_shuffle
    rng = np.random.default_rng(0)
    codes = rng.integers(0, 5, size=(5, 120)).astype(np.uint8)
    codes[1] = rng.integers(0, 4, size=120)            # no N
    codes[2, 10:90] = 2                                # low complexity
    sh = dinucleotide_shuffle(codes, n=3, seed=4)
    assert sh.shape == (5, 3, 120) and sh.dtype == np.uint8
    for i in range(5):
        for r in range(3):
            assert np.array_equal(_dinuc(sh[i, r]), _dinuc(codes[i]))
            assert sh[i, r, 0] == codes[i, 0] and sh[i, r, -1] == codes[i, -1]
    assert (sh[0, 0] != codes[0]).any() and (sh[0, 0] != sh[0, 1]).any()
    assert np.array_equal(sh, dinucleotide_shuffle(codes, n=3, seed=4))
    assert not np.array_equal(sh, dinucleotide_shuffle(codes, n=3, seed=5))
    one = dinucleotide_shuffle(codes[0], n=2, seed=4)
    assert one.shape == (2, 120) and np.array_equal(one, sh[0, :2])
    with pytest.raises(ValueError):
        dinucleotide_shuffle(np.full((2, 8), 7, np.uint8))
