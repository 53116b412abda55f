"""The device shuffle's algorithm on the CPU (tests/shuffle_model.py, a restatement of DESIGN.md section 3
"Shuffles"): the invariants of a dinucleotide-preserving shuffle, uniformity over the enumerated
arrangements by Pearson's chi-square, and the fallback behind the cap.  tests/test_gpu_shuffle.py holds
csrc/shuffle.hip to this model byte for byte."""
import collections

import numpy as np

import shuffle_model as sm
from shuffle_util import (CYCLIC_ROW, DRAWS_PER_ARRANGEMENT, SEED, UNIFORM_ROW, assert_invariants, assert_uniform,
                          chi2_upper, encode, mixed_rows)


def test_arrangement_counts():
    assert len(sm.arrangements(encode(UNIFORM_ROW))) == 21
    assert len(sm.arrangements(encode(CYCLIC_ROW))) == 28
    assert sm.arrangements(encode("ACACACACG")) == [tuple(encode("ACACACACG"))]


def test_invariants():
    for L in (3, 4, 7, 16, 17, 61):
        rows = mixed_rows(12, L, seed=L)
        out, capped = sm.shuffle(rows, n=3, seed=5, row0=2)
        assert not capped.any()
        for i in range(len(rows)):
            for r in range(3):
                assert_invariants(rows[i], out[i, r])
    # N is kept as a symbol, and a byte above 4 is N
    row = np.array([0, 4, 1, 4, 4, 2, 200, 3, 4, 0], dtype=np.uint8)
    out, _ = sm.shuffle(row[None], n=20, seed=1)
    assert (out == 4).sum(axis=2).tolist() == [[5] * 20]
    assert len({tuple(o) for o in out[0].tolist()}) > 1


def test_short_rows_and_homopolymers():
    for row in ([3], [2, 7], [1, 1]):
        out, capped = sm.shuffle(np.array([row], dtype=np.uint8), n=2, seed=3)
        assert out.tolist() == [[[min(s, 4) for s in row]] * 2] and not capped.any()
    for sym in range(5):
        out, capped = sm.shuffle(np.full((1, 9), sym, dtype=np.uint8), n=2, seed=3)
        assert (out == sym).all() and not capped.any()


def test_pure_function_of_seed_row_and_shuffle():
    rows = mixed_rows(9, 23, seed=2)
    whole, _ = sm.shuffle(rows, n=4, seed=8)
    part, _ = sm.shuffle(rows[3:7], n=2, seed=8, row0=3)
    assert np.array_equal(part, whole[3:7, :2])
    assert not np.array_equal(whole, sm.shuffle(rows, n=4, seed=9)[0])
    assert not np.array_equal(whole[0], sm.shuffle(rows[:1], n=4, seed=8, row0=1)[0][0])


def test_lane_model_equals_plain_loops():
    for L in (1, 2, 3, 16, 33):
        rows = mixed_rows(13, L, seed=40 + L)
        for max_rounds in (0, 1):
            a = sm.shuffle(rows, n=3, seed=6, row0=5, max_rounds=max_rounds)
            b = sm.shuffle_lanes(rows, n=3, seed=6, row0=5, max_rounds=max_rounds)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_uniform_over_arrangements():
    row = encode(UNIFORM_ROW)
    M = DRAWS_PER_ARRANGEMENT * len(sm.arrangements(row))
    draws, capped = sm.shuffle_lanes(row[None], n=M, seed=SEED)
    assert not capped.any()
    assert_uniform(row, draws[0])


def test_uniform_when_cycles_are_popped():
    row = encode(CYCLIC_ROW)
    popped = [sm.shuffle_one_popped(row, SEED, 0, r)[2] for r in range(200)]
    assert np.mean(popped) > 0.5           # this row does exercise the popping
    M = DRAWS_PER_ARRANGEMENT * len(sm.arrangements(row))
    draws, capped = sm.shuffle_lanes(row[None], n=M, seed=SEED)
    assert not capped.any()
    assert_uniform(row, draws[0])


def test_statistic_on_the_host_shuffle():
    """The host sampler passes the same statistic on the same rows: a check of the test itself."""
    from explainn_amd.sequence import dinucleotide_shuffle
    for s in (UNIFORM_ROW, CYCLIC_ROW):
        row = encode(s)
        M = DRAWS_PER_ARRANGEMENT * len(sm.arrangements(row))
        assert_uniform(row, dinucleotide_shuffle(row, n=M, seed=SEED))


def test_statistic_rejects_a_biased_sampler():
    """... and does reject the walk that always takes the row's own last exits (the capped fallback)."""
    row = encode(CYCLIC_ROW)
    M = DRAWS_PER_ARRANGEMENT * len(sm.arrangements(row))
    draws, capped = sm.shuffle_lanes(row[None], n=M // 10, seed=SEED, max_rounds=1)
    assert capped.any()
    arr = sm.arrangements(row)
    seen = collections.Counter(map(tuple, draws[0].tolist()))
    expect = draws.shape[1] / len(arr)
    assert sum((seen[a] - expect) ** 2 / expect for a in arr) > chi2_upper(len(arr) - 1)


def test_fallback_at_the_cap():
    for n_rep in (2, 5, 20):
        row = np.array([0, 1] * n_rep + [2], dtype=np.uint8)
        out, capped = sm.shuffle(row[None], n=40, seed=4, max_rounds=1)
        # (AC)^n G: C's exit is G with probability 1/n at the first picks and again after the one pop
        assert capped.any() or n_rep == 2
        own = sm.own_last_exits(row.astype(np.int64))
        assert own == {0: 1, 1: 2}
        for r in range(40):
            assert_invariants(row, out[0, r])
            one, cap, popped = sm.shuffle_one_popped(row, 4, 0, r, max_rounds=1)
            assert cap == capped[0, r] and (popped == 1 if cap else popped <= 1)
            if cap:
                # the walk with the row's own last exits, on the draws that follow the tree sampler's:
                # A and C drew once each at the first picks and once each in the one popped cycle
                rng = sm.Stream(4, 0, r)
                rng.t = 4
                assert np.array_equal(out[0, r], sm.walk(row.astype(np.int64), own, rng))
    # with the default cap the same rows never reach it
    row = np.array([0, 1] * 20 + [2], dtype=np.uint8)
    assert not sm.shuffle(row[None], n=40, seed=4)[1].any()
