"""The tiling and unfold algebra of the shared scan (tests/scan_model.py) against the oracle's
eval-mode pooled values: for every window, the unfolded tile track equals the pooled vector of the
materialised window -- exactly, in fp64: the same products summed in the same order at every sequence
position, and the max picks the same element.  CPU only."""
import numpy as np
import pytest

from oracle import explainn_oracle as orc
import scan_model as sm
from explainn_amd import scan as scan_py          # (the feature's module: window count and starts)


def _pooled(sd, mat):
    """(B,U,n) eval-mode pooled values of a (B,L) code matrix, fp64."""
    _, cache, _ = orc.forward(sd, sm.onehot(mat), dtype=np.float64, return_cache=True)
    return cache["q"]


SHAPES = [(200, 19), (50, 5), (83, 7), (600, 32)]


@pytest.mark.parametrize("L,k", SHAPES)
@pytest.mark.parametrize("mname", ["1", "2", "3", "n", "n+2"])
def test_unfolded_tile_track_equals_window_pooling(L, k, mname):
    n = sm.pooled_len(L, k)
    m = {"1": 1, "2": 2, "3": 3, "n": n, "n+2": n + 2}[mname]
    stride = 7 * m
    U = 3
    sd = orc.random_state_dict(U, k, L, 1, seed=L + m)
    sd["linears.1.weight"] = np.array([0.9, -1.1, 0.7], dtype=np.float32)      # one unit pools the minimum
    for region in (L, L + 1, L + stride - 1, L + stride, 3000 + L):
        start = 5                                                           # not a multiple of 7
        seq = sm.random_codes(start + region + 11, seed=region + m, n_runs=6, tile=7 * n)
        W = len(scan_py.window_starts(region, L, stride))
        assert W == (region - L) // stride + 1 >= 1
        for rc in (False, True):
            windows = sm.window_matrix(seq, start, W, stride, L, rc)
            start0, step, J = sm.tile_plan(start, W, stride, L, k, rc)
            assert J == -(-(m * (W - 1) + n) // n) and abs(step) == 7 * n
            # no valid window reads a position the tiles pad past the region
            Leff = stride * (W - 1) + L
            assert sm.padded_reads(start, W, stride, L, k) < Leff
            # the tiles see the sequence only inside the region: everything else is N, as the padding is
            masked = np.full_like(seq, 4)
            masked[start:start + Leff] = seq[start:start + Leff]
            tiles = sm.window_matrix(masked, start0, J, step, L, rc)
            got = sm.unfold(_pooled(sd, tiles), m, W, rc)
            want = _pooled(sd, windows)
            assert got.shape == want.shape == (W, U, n)
            assert np.array_equal(got, want), (L, k, m, region, rc, np.abs(got - want).max())


def test_tile_count_small_cases():
    # one window: one tile; n windows at m = 1 reach into the second tile
    assert sm.n_tiles(26, 1, 1) == 1
    assert sm.n_tiles(26, 1, 2) == 2
    assert sm.n_tiles(26, 26, 3) == 3          # m = n: one tile per window
    assert sm.n_tiles(26, 28, 3) == 4          # m = n + 2: gaps, tiles cover them too
