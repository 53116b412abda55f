"""Dinucleotide-preserving shuffles on the device (csrc/shuffle.hip) against tests/shuffle_model.py byte
for byte, the invariants and the uniformity statistic straight from the device output, and Integrated
Gradients with baselines="shuffle" against the same call with the device's shuffles passed explicitly."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from oracle import explainn_oracle as orc
from parity_util import model as make_model
import shuffle_model as sm
from shuffle_util import (CYCLIC_ROW, DRAWS_PER_ARRANGEMENT, SEED, UNIFORM_ROW, assert_invariants, assert_uniform,
                          encode, mixed_rows)

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 15, 16, 17, 60, 200, 257, 1000)
SHAPES = ((1, 1), (1, 65), (63, 3), (65, 64), (130, 5))
N_MAX, R_MAX = 130, 65
GUARD, FILL = 64, 0xAB
DEV_SEED, ROW0 = 12345, 7


def _rows(L):
    return mixed_rows(N_MAX, L, seed=L)


@functools.lru_cache(maxsize=None)
def _model(L, max_rounds):
    """The model's (out, capped) of all N_MAX rows x R_MAX shuffles, once per (L, max_rounds): every (N, R)
    of SHAPES is a slice of it, because a row's shuffles depend on (seed, row0 + i, r) alone."""
    out, capped = sm.shuffle_lanes(_rows(L), R_MAX, DEV_SEED, ROW0, max_rounds)
    out.setflags(write=False)
    capped.setflags(write=False)
    return out, capped


def _launch(rows, R, seed=DEV_SEED, row0=ROW0, max_rounds=0, want_capped=True, shift=(5, 3)):
    """explainn_dinucleotide_shuffle through ctypes, with codes and out at odd byte offsets of their
    buffers and a guard band around out and capped; checks the bands and that codes is untouched.
    Returns (out, capped or None) as numpy."""
    from explainn_amd import _lib
    lib = _lib.load()
    N, L = rows.shape
    src = torch.full((shift[0] + N * L,), FILL, dtype=torch.uint8, device="cuda")
    src[shift[0]:] = torch.from_numpy(np.ascontiguousarray(rows)).reshape(-1).cuda()
    before = src.clone()
    out = torch.full((shift[1] + N * R * L + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    cap = torch.full((N * R + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    rc = lib.explainn_dinucleotide_shuffle(
        src.data_ptr() + shift[0], N, L, R, seed, row0, max_rounds, out.data_ptr() + shift[1],
        cap.data_ptr() if want_capped else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == _lib.OK, lib.explainn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(src, before), "codes changed"
    assert (out[:shift[1]] == FILL).all() and (out[shift[1] + N * R * L:] == FILL).all(), "write outside out"
    assert (cap[N * R if want_capped else 0:] == FILL).all(), "write outside capped"
    got = out[shift[1]:shift[1] + N * R * L].reshape(N, R, L).cpu().numpy()
    return got, (cap[:N * R].reshape(N, R).cpu().numpy() if want_capped else None)


@pytest.mark.parametrize("max_rounds", [0, 1])
@pytest.mark.parametrize("L", LENGTHS)
def test_device_equals_model(L, max_rounds):
    want, want_cap = _model(L, max_rounds)
    rows = _rows(L)
    for N, R in SHAPES:
        got, cap = _launch(rows[:N], R, max_rounds=max_rounds)
        assert np.array_equal(got, want[:N, :R]), (N, R)
        assert np.array_equal(cap, want_cap[:N, :R]), (N, R)
    if max_rounds == 1 and L >= 15:
        assert want_cap[:63, :3].any() and not want_cap[:63, :3].all()      # the branch did run, and not only it
    got, cap = _launch(rows[:63], 3, max_rounds=max_rounds, want_capped=False)
    assert cap is None and np.array_equal(got, want[:63, :3])
    got, _ = _launch(rows[:63], 3, max_rounds=max_rounds, shift=(0, 0))      # aligned buffers too
    assert np.array_equal(got, want[:63, :3])


def test_split_independence():
    L = 60
    want, _ = _model(L, 0)
    rows = _rows(L)
    part, _ = _launch(rows[17:90], 7, row0=ROW0 + 17)
    assert np.array_equal(part, want[17:90, :7])
    assert np.array_equal(_launch(rows[17:90], 3, row0=ROW0 + 17)[0], part[:, :3])


def test_seeds():
    rows = _rows(60)[:63]
    a, _ = _launch(rows, 3)
    assert np.array_equal(a, _launch(rows, 3)[0])
    assert not np.array_equal(a, _launch(rows, 3, seed=DEV_SEED + 1)[0])
    assert not np.array_equal(a, _launch(rows, 3, row0=ROW0 + 1)[0])
    big = 2 ** 64 - 1                                          # the whole 64-bit seed is used
    assert np.array_equal(_launch(rows[:2], 2, seed=big)[0], sm.shuffle_lanes(rows[:2], 2, big, ROW0)[0])
    assert not np.array_equal(_launch(rows[:2], 2, seed=big)[0], _launch(rows[:2], 2, seed=2 ** 32 - 1)[0])


def test_invariants_from_device_output():
    """Straight from the device's bytes, in case the model shares a mistake with the kernel."""
    rows = _rows(1000)[:65]
    for max_rounds in (0, 1):
        got, _ = _launch(rows, 64, max_rounds=max_rounds)
        sym = np.minimum(rows, 4)
        assert got.max() <= 4
        assert (got[:, :, 0] == sym[:, None, 0]).all() and (got[:, :, -1] == sym[:, None, -1]).all()
        pair = got[:, :, :-1].astype(np.int64) * 5 + got[:, :, 1:]
        pair_in = sym[:, :-1].astype(np.int64) * 5 + sym[:, 1:]
        for q in range(25):
            assert ((pair == q).sum(axis=2) == (pair_in == q).sum(axis=1)[:, None]).all(), q
        if max_rounds == 0:
            assert (got[0] != sym[0]).any() and len({o.tobytes() for o in got[0]}) == 64
    for r in range(4):                                         # and once through the CPU test's own helper
        assert_invariants(rows[6], got[6, r])


@pytest.mark.parametrize("name", [UNIFORM_ROW, CYCLIC_ROW])
def test_uniform_over_arrangements(name):
    row = encode(name)
    M = DRAWS_PER_ARRANGEMENT * len(sm.arrangements(row))
    draws, capped = _launch(row[None], M, seed=SEED, row0=0)   # one row, R = M
    assert not capped.any()
    assert_uniform(row, draws[0])
    draws, capped = _launch(np.repeat(row[None], M, axis=0), 1, seed=SEED, row0=0)   # M copies, R = 1
    assert not capped.any()
    assert_uniform(row, draws[:, 0])


def test_python_wrapper():
    from explainn_amd.sequence import dinucleotide_shuffle_device
    rows = _rows(60)[:9]
    want, want_cap = _model(60, 1)
    dev = torch.from_numpy(rows).cuda()
    out, cap = dinucleotide_shuffle_device(dev, n=4, seed=DEV_SEED, row0=ROW0, max_rounds=1, return_capped=True)
    assert out.device == dev.device and out.dtype == torch.uint8 and tuple(out.shape) == (9, 4, 60)
    assert torch.equal(out.cpu(), torch.from_numpy(want[:9, :4].copy()))
    assert torch.equal(cap.cpu(), torch.from_numpy(want_cap[:9, :4].copy()))
    one = dinucleotide_shuffle_device(dev[0], n=4, seed=DEV_SEED, row0=ROW0, max_rounds=1)
    assert torch.equal(one, out[0])
    assert torch.equal(dev.cpu(), torch.from_numpy(rows))
    # a strided view is made contiguous, not misread
    assert torch.equal(dinucleotide_shuffle_device(dev[::2], 2, DEV_SEED),
                       dinucleotide_shuffle_device(dev[::2].contiguous(), 2, DEV_SEED))
    empty = dinucleotide_shuffle_device(dev[:0], n=3)
    assert tuple(empty.shape) == (0, 3, 60) and empty.device == dev.device
    e_out, e_cap = dinucleotide_shuffle_device(dev[:0], n=3, return_capped=True)
    assert tuple(e_out.shape) == (0, 3, 60) and tuple(e_cap.shape) == (0, 3)


def test_errors():
    from explainn_amd import _lib
    from explainn_amd.sequence import dinucleotide_shuffle_device
    lib = _lib.load()
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((256,), FILL, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for N, L, R in ((2, 8, 0), (2, 0, 2), (-1, 8, 2)):
        assert lib.explainn_dinucleotide_shuffle(src.data_ptr(), N, L, R, 0, 0, 0, out.data_ptr(), None,
                                                 stream) == _lib.E_ARG
    assert lib.explainn_dinucleotide_shuffle(src.data_ptr(), 0, 8, 2, 0, 0, 0, out.data_ptr(), None,
                                             stream) == _lib.OK
    torch.cuda.synchronize()
    assert (out == FILL).all()
    dev = src.reshape(8, 8)
    with pytest.raises(RuntimeError):
        dinucleotide_shuffle_device(dev.cpu())
    with pytest.raises(ValueError):
        dinucleotide_shuffle_device(dev.to(torch.int32))
    with pytest.raises(ValueError):
        dinucleotide_shuffle_device(dev.reshape(2, 4, 8))
    with pytest.raises(ValueError):
        dinucleotide_shuffle_device(dev, n=0)
    with pytest.raises(ValueError):
        dinucleotide_shuffle_device(dev.cpu().numpy())


# ---- Integrated Gradients with baselines="shuffle" ----
IG_SHAPE = (6, 9, 60, 2, 5)         # U, k, L, T, N


def _codes(x):
    return np.where(x.sum(axis=1) > 0, x.argmax(axis=1), 4).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _ig_setup():
    from explainn_amd.sequence import dinucleotide_shuffle_device
    U, k, L, T, N = IG_SHAPE
    sd = orc.random_state_dict(U, k, L, T, seed=12)
    x = orc.random_onehot(N, L, seed=13, n_frac=0.02).astype(np.float32)
    codes = _codes(x)
    m = make_model(sd, U, k, L, T).eval()
    shuf = dinucleotide_shuffle_device(torch.from_numpy(codes).cuda(), 2, 3).cpu().numpy()
    return m, x, codes, shuf


@pytest.mark.parametrize("onehot", [False, True])
@pytest.mark.parametrize("rc", [False, True])
def test_ig_shuffle_baseline(rc, onehot):
    from explainn_amd import interpret
    m, x, codes, shuf = _ig_setup()
    assert (shuf != codes[:, None]).any()
    Xs = x if onehot else codes
    kw = dict(steps=6, batch_size=3, return_delta=True, rev_complement=rc)
    got = interpret.integrated_gradients(m, Xs, "shuffle", n_shuffles=2, seed=3, **kw)
    ref = interpret.integrated_gradients(m, Xs, shuf, **kw)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.abs(got[0]).max() > 0
    # n_shuffles and seed are ignored for the other baselines
    kw["return_delta"] = False
    assert np.array_equal(interpret.integrated_gradients(m, Xs, "zero", n_shuffles=7, seed=9, **kw),
                          interpret.integrated_gradients(m, Xs, "zero", **kw))


def test_ig_shuffle_arguments():
    from explainn_amd import interpret
    m, x, codes, shuf = _ig_setup()
    with pytest.raises(ValueError):
        interpret.integrated_gradients(m, codes, "shuffle", n_shuffles=0)
    with pytest.raises(ValueError):                            # the model-level call keeps refusing the word
        m.integrated_gradients(torch.from_numpy(x).cuda(), torch.ones(len(x), IG_SHAPE[3], device="cuda"), "shuffle")
    # independent of the batch size
    a = interpret.integrated_gradients(m, codes, "shuffle", n_shuffles=2, seed=3, steps=6, batch_size=2)
    b = interpret.integrated_gradients(m, codes, shuf, steps=6, batch_size=5)
    assert np.array_equal(a, b)


def test_cli_device_shuffle(tmp_path):
    from explainn_amd import attribution, interpret
    m, x, codes, shuf = _ig_setup()
    ckpt = os.path.join(tmp_path, "model.pth.tar")
    torch.save({"options": dict(m._options), "state_dict": {key: v.cpu() for key, v in m.state_dict().items()}},
               ckpt)
    fa = os.path.join(tmp_path, "seqs.fa")
    with open(fa, "w") as fh:
        for i, row in enumerate(codes):
            fh.write(">s%d desc\n%s\n" % (i, "".join("ACGTN"[c] for c in row)))
    out = os.path.join(tmp_path, "ig.npz")
    attribution.main([ckpt, fa, "-o", out, "--baseline", "device-shuffle", "--n-shuffles", "2", "--seed", "3",
                      "--steps", "6", "-b", "3"])
    got = np.load(out)
    ref, delta = interpret.integrated_gradients(m, codes, shuf, steps=6, batch_size=3, return_delta=True)
    assert np.array_equal(got["ig"], ref) and np.array_equal(got["delta"], delta)
