"""The incremental in-silico mutagenesis algebra (tests/ism_model.py, the kernels' recipe) against
brute force through the fp64 oracle on every substituted sequence (CPU only)."""
import numpy as np
import pytest

from oracle import explainn_oracle as orc
from tests import ism_model


def _case(U, k, L, T, seed, n_frac=0.0, neg_units=()):
    sd = orc.random_state_dict(U, k, L, T, seed=seed, dtype=np.float64)
    for u in neg_units:
        sd["linears.1.weight"][u] = -abs(sd["linears.1.weight"][u]) - 0.3   # min-pooling units
    rng = np.random.default_rng(seed + 100)
    codes = rng.integers(0, 4, size=(2, L))
    if n_frac:
        codes[rng.random((2, L)) < n_frac] = 4
    return sd, codes


@pytest.mark.parametrize("k", [2, 5, 19, 32])
def test_incremental_matches_brute_force(k):
    L = k + 7 * 3 + 4                      # Lo mod 7 != 0: a dropped tail
    sd, codes = _case(3, k, L, 3, seed=k, n_frac=0.1, neg_units=(1,))
    logits, delta = ism_model.ism(sd, codes)
    base, ref = ism_model.brute_force(sd, codes)
    np.testing.assert_allclose(logits, base, rtol=1e-10, atol=1e-12)
    scale = np.abs(ref).max()
    assert scale > 1e-3
    assert np.abs(delta - ref).max() <= 1e-10 * scale


def test_exact_zeros():
    k, L = 5, 5 + 7 * 2 + 5
    sd, codes = _case(2, k, L, 3, seed=7, n_frac=0.15)
    _, delta = ism_model.ism(sd, codes)
    n = orc.pooled_len(L, k)
    pend = 7 * n + k - 1
    assert pend < L
    assert np.all(delta[:, :, :, pend:] == 0)
    for b in range(codes.shape[0]):
        for p in range(L):
            if codes[b, p] < 4:
                assert np.all(delta[b, :, codes[b, p], p] == 0)
    # at an N position every row is a real substitution
    bs, ps = np.nonzero(codes[:, :pend] == 4)
    assert len(bs) and np.any(delta[bs, :, :, ps] != 0)
