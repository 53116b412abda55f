"""Shared by tests/test_shuffle_model.py (CPU) and tests/test_gpu_shuffle.py: the rows, the invariants and
the uniformity statistic that both hold a dinucleotide-preserving shuffle to."""
import collections
import statistics

import numpy as np

import shuffle_model as sm

# short rows for the uniformity statistic: K distinct arrangements by DFS.  CYCLIC's first picks hold the
# cycle A -> C -> A three times out of four, so its tree sampler has to pop cycles
UNIFORM_ROW = "AACGTCAGTCAG"          # K = 21
CYCLIC_ROW = "ACACCACAGCG"            # K = 28
DRAWS_PER_ARRANGEMENT = 2000
SEED = 17


def encode(s):
    return np.array(["ACGTN".index(ch) for ch in s], dtype=np.uint8)


def chi2_upper(df, p=1e-6):
    """The upper p quantile of chi-square(df): scipy where there is one, Wilson-Hilferty otherwise."""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(p, df))
    except ImportError:
        z = statistics.NormalDist().inv_cdf(1.0 - p)
        return df * (1.0 - 2.0 / (9.0 * df) + z * (2.0 / (9.0 * df)) ** 0.5) ** 3


def uniformity(row, draws):
    """Pearson's chi-square of `draws` (M, L) against the uniform law on the arrangements of `row`; every
    arrangement has to occur and nothing else.  Returns (statistic, K)."""
    arr = sm.arrangements(row)
    seen = collections.Counter(map(tuple, np.asarray(draws).tolist()))
    assert set(seen) == set(arr), "draws outside the enumeration, or an arrangement never drawn"
    expect = len(draws) / len(arr)
    return sum((seen[a] - expect) ** 2 / expect for a in arr), len(arr)


def assert_uniform(row, draws):
    stat, K = uniformity(row, draws)
    assert stat < chi2_upper(K - 1), (stat, chi2_upper(K - 1), K)


def assert_invariants(row, out):
    sym = np.minimum(np.asarray(row), 4).astype(np.int64)
    out = np.asarray(out).astype(np.int64)
    assert out.shape == sym.shape and out.max(initial=0) <= 4
    assert out[0] == sym[0] and out[-1] == sym[-1]
    assert np.array_equal(sm.pair_counts(out), sm.pair_counts(sym))


def mixed_rows(N, L, seed):
    """Row i by i mod 6: random with 2 % N, a homopolymer, (AC)^n G, A^n C^n G, all N, bytes 5..255."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 4, (N, L)).astype(np.uint8)
    rows[rng.random((N, L)) < 0.02] = 4
    for i in range(N):
        kind = i % 6
        if kind == 1:
            rows[i] = (i // 6) % 5
        elif kind == 2 and L >= 3:
            rows[i] = ([0, 1] * L)[:L - 1] + [2]
        elif kind == 3 and L >= 3:
            half = (L - 1) // 2
            rows[i] = [0] * (L - 1 - half) + [1] * half + [2]
        elif kind == 4:
            rows[i] = 4
        elif kind == 5:
            rows[i] = rng.integers(5, 256, L)
    return rows
