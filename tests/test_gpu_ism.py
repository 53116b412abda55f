"""In-silico mutagenesis on the device (csrc/ism.hip): delta against brute force -- the fp64 oracle
on every substituted sequence for small shapes, the device forward on the materialised mutants for
full-size ones -- plus the exact zeros, bit-identical logits, input forms, errors and the CLI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import explainn_oracle as orc
from parity_util import model as make_model
from tests import ism_model

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _case(U, k, L, T, B, seed, n_frac=0.03, neg=True):
    sd = orc.random_state_dict(U, k, L, T, seed=seed)
    if neg:
        sd["linears.1.weight"][::3] = -np.abs(sd["linears.1.weight"][::3]) - 0.3   # min-pooling units
    rng = np.random.default_rng(seed + 1)
    codes = rng.integers(0, 4, size=(B, L)).astype(np.uint8)
    if n_frac:
        codes[rng.random((B, L)) < n_frac] = 4
    return sd, codes


def _onehot(codes):
    return torch.tensor(ism_model.onehot(codes), dtype=torch.float32, device="cuda")


def _ism(m, x):
    logits, delta = m.in_silico_mutagenesis(x)
    torch.cuda.synchronize()
    return logits.cpu().numpy(), delta.cpu().numpy()


def _device_brute(m, codes, rows=None):
    """delta from model(x) on all 4L substituted copies (reference rows come out 0); of the sequences
    `rows` only when given (the base logits are always those of every sequence)."""
    B, L = codes.shape
    out = []
    with torch.no_grad():
        base = m(torch.tensor(codes, device="cuda")).cpu().numpy()
        for b in (range(B) if rows is None else rows):
            mut = np.repeat(codes[b:b + 1], 4 * L, axis=0)
            for a in range(4):
                mut[a * L + np.arange(L), np.arange(L)] = a
            lg = m(torch.tensor(mut, device="cuda")).cpu().numpy()          # (4L, T)
            d = (lg - base[b]).reshape(4, L, -1).transpose(2, 0, 1)
            for p in range(L):
                if codes[b, p] < 4:
                    d[:, codes[b, p], p] = 0.0
            out.append(d)
    return base, np.stack(out)


@pytest.mark.parametrize("U,k,L,T,B", [
    (5, 2, 2 + 7 * 6 + 3, 1, 6), (6, 5, 5 + 7 * 5 + 4, 3, 9), (4, 19, 19 + 7 * 4 + 2, 3, 5),
    (3, 32, 32 + 7 * 3 + 6, 1, 7)])
def test_vs_oracle_small(U, k, L, T, B):
    sd, codes = _case(U, k, L, T, B, seed=10 + k)
    m = make_model(sd, U, k, L, T).eval()
    logits, delta = _ism(m, _onehot(codes))
    base, ref = ism_model.brute_force(sd, codes)
    err = np.abs(delta - ref).max()
    record_margin("ism_vs_oracle", err, TOL)
    assert err <= TOL, "k=%d: max |delta - oracle| = %.3g" % (k, err)
    assert np.abs(logits - base).max() <= TOL


def test_vs_oracle_c1_like():
    U, k, L, T, B = 100, 19, 200, 1, 8
    sd, codes = _case(U, k, L, T, B, seed=3)
    m = make_model(sd, U, k, L, T).eval()
    _, delta = _ism(m, _onehot(codes))
    _, ref = ism_model.brute_force(sd, codes)
    err = np.abs(delta - ref).max()
    record_margin("ism_vs_oracle", err, TOL)
    assert err <= TOL


@pytest.mark.parametrize("U,k,L,T,B", [
    (300, 19, 200, 1, 32),        # C2
    (40, 19, 200, 50, 8),         # T = 50
    (6, 19, 1000, 2, 4),          # n = 140
    (70, 9, 120, 3, 70)])         # U not a multiple of 64, B not a multiple of 64
def test_vs_device_brute_force(U, k, L, T, B):
    sd, codes = _case(U, k, L, T, B, seed=U + k)
    m = make_model(sd, U, k, L, T).eval()
    logits, delta = _ism(m, torch.tensor(codes, device="cuda"))
    base, ref = _device_brute(m, codes)
    err = np.abs(delta - ref).max()
    record_margin("ism_vs_device_brute_force", err, TOL)
    assert err <= TOL, "max |delta - brute force| = %.3g" % err
    assert np.array_equal(logits, base)


def test_exact_zeros_logits_and_determinism():
    U, k, L, T, B = 30, 7, 7 + 7 * 10 + 5, 3, 100
    sd, codes = _case(U, k, L, T, B, seed=5, n_frac=0.05)
    m = make_model(sd, U, k, L, T).eval()
    x = _onehot(codes)
    logits, delta = _ism(m, x)
    logits2, delta2 = _ism(m, x)
    assert np.array_equal(delta, delta2) and np.array_equal(logits, logits2)
    with torch.no_grad():
        assert np.array_equal(logits, m(x).cpu().numpy())
    pend = 7 * orc.pooled_len(L, k) + k - 1
    assert pend < L and np.all(delta[:, :, :, pend:] == 0)
    bs, ps = np.nonzero(codes < 4)
    assert np.all(delta[bs, :, codes[bs, ps], ps] == 0)
    bn, pn = np.nonzero(codes[:, :pend] == 4)
    assert np.any(delta[bn, :, :, pn] != 0)


def test_input_forms_and_interpret():
    from explainn_amd import interpret
    from explainn_amd.architectures import BaseCodes
    U, k, L, T, B = 12, 11, 80, 3, 20
    sd, codes = _case(U, k, L, T, B, seed=8)
    m = make_model(sd, U, k, L, T).eval()
    ct = torch.tensor(codes, device="cuda")
    l1, d1 = _ism(m, _onehot(codes))
    l2, d2 = _ism(m, BaseCodes(ct))
    assert np.array_equal(l1, l2) and np.array_equal(d1, d2)
    rc = np.where(codes < 4, 3 - codes, codes)[:, ::-1].copy()
    l3, d3 = _ism(m, BaseCodes(ct, reverse_complement=True))
    l4, d4 = _ism(m, _onehot(rc))
    assert np.array_equal(l3, l4) and np.array_equal(d3, d4)
    # rev_complement maps back onto the given strand: brute force on the reverse strand, flipped
    got = interpret.in_silico_mutagenesis(m, codes, batch_size=7, rev_complement=True)
    _, ref = _device_brute(m, rc)
    assert np.abs(got - ref[:, :, ::-1, ::-1]).max() <= TOL
    got1 = interpret.in_silico_mutagenesis(m, ism_model.onehot(codes).astype(np.float32), target=1)
    assert np.array_equal(got1, d1[:, 1])
    ab = interpret.in_silico_mutagenesis(m, codes, absolute=True)
    assert np.allclose(ab, l1[:, :, None, None] + d1, atol=0, rtol=0)
    assert m.training is False


def test_errors():
    from explainn_amd import _lib
    U, k, L, T, B = 8, 5, 40, 2, 6
    sd, codes = _case(U, k, L, T, B, seed=9)
    m = make_model(sd, U, k, L, T)
    x = _onehot(codes)
    m.train()
    with pytest.raises(RuntimeError):
        m.in_silico_mutagenesis(x)
    m.eval()
    soft = x * 0.5
    with pytest.raises(ValueError):
        m.in_silico_mutagenesis(soft)
    # C ABI: dense mode is unsupported; an ISM call ends a pending train forward
    dev = m._device()
    ctx = m._context(B, dev)
    ps, _ = m._params_struct(dev)
    lib, h, st = ctx.lib, ctx.handle, m._stream(dev)
    logits = torch.empty(B, T, device=dev)
    delta = torch.empty(B, T, 4, L, device=dev)
    nb = int(lib.explainn_ism_workspace_bytes(h, B))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    args = (x.data_ptr(), B, C.byref(ps), logits.data_ptr(), delta.data_ptr(), ws.data_ptr(), nb, st)
    _lib.check(lib.explainn_dense_input(h, 1))
    assert lib.explainn_ism(h, *args) == _lib.E_UNSUPPORTED
    _lib.check(lib.explainn_dense_input(h, 0))
    assert lib.explainn_ism(h, x.data_ptr(), B, C.byref(ps), logits.data_ptr(), delta.data_ptr(),
                            ws.data_ptr(), nb - 1, st) == _lib.E_ARG
    _lib.check(lib.explainn_forward_train(h, x.data_ptr(), B, C.byref(ps), None, 0.0, C.c_uint64(1),
                                          logits.data_ptr(), st))
    _lib.check(lib.explainn_ism(h, *args))
    dl = torch.ones(B, T, device=dev)
    assert lib.explainn_backward(h, dl.data_ptr(), B, C.byref(ps), C.byref(_lib.Grads()), 0, st) == _lib.E_STATE
    torch.cuda.synchronize()


def test_cli(tmp_path):
    from explainn_amd import interpret, mutagenesis
    U, k, L, T, B = 6, 9, 60, 2, 5
    sd, codes = _case(U, k, L, T, B, seed=12)
    m = make_model(sd, U, k, L, T).eval()
    ckpt = os.path.join(tmp_path, "model.pth.tar")
    torch.save({"options": dict(m._options), "state_dict": {key: v.cpu() for key, v in m.state_dict().items()}},
               ckpt)
    fa = os.path.join(tmp_path, "seqs.fa")
    with open(fa, "w") as fh:
        for i, row in enumerate(codes):
            fh.write(">s%d desc\n%s\n" % (i, "".join("ACGTN"[c] for c in row)))
    out = os.path.join(tmp_path, "ism.npz")
    mutagenesis.main([ckpt, fa, "-o", out, "-r", "-b", "3"])
    got = np.load(out)
    assert list(got["ids"]) == ["s%d" % i for i in range(B)]
    ref = interpret.in_silico_mutagenesis(m, codes, rev_complement=True)
    assert np.array_equal(got["delta"], ref)
    from explainn_amd.architectures import BaseCodes
    with torch.no_grad():
        lg = m(BaseCodes(torch.tensor(codes, device="cuda"), True)).cpu().numpy()
    assert np.array_equal(got["logits"], lg)
