"""Integrated Gradients on the device (csrc/pathgrad.hip: the path walked in conv-sum space) against
the fp64 brute-force Riemann sum -- autograd of oracle/torch_ref.py at every soft input, times
(x - x') (tests/pathgrad_model.brute_force) -- never against the algebra model or the code under test.
Bound as in tests/test_gpu_input_grad.py: relative to max|ref|, 5e-5 or 3x what the same brute force in
torch fp32 makes.  Sequences whose path holds a knife edge in the oracle's fp64 intermediates
(pathgrad_model.knife_rows) are left out; the exclusion is capped at a quarter of the batch."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import explainn_oracle as orc
from parity_util import KNIFE, TOL, model as make_model
import pathgrad_model as pm

pytestmark = pytest.mark.gpu

#        U,  k,   L, T,  B,  S, baseline
CASES = [(1, 2, 50, 1, 4, 4, "zero"), (3, 5, 60, 1, 64, 8, "codes"), (8, 19, 200, 3, 64, 16, "codes"),
         (33, 7, 100, 2, 70, 5, "uniform"), (8, 19, 200, 3, 64, 16, "zero"), (65, 32, 150, 1, 40, 3, "codes"),
         # case 0's one unit is closed along its whole path (an all-zero reference: exact zeros are what
         # it checks); the same shape again whose reference is not zero
         (1, 2, 50, 1, 4, 4, "codes")]


def _codes(x):
    return np.where(x.sum(axis=1) > 0, x.argmax(axis=1), 4).astype(np.uint8)


def _inputs(i, B=None, n_frac=0.02):
    U, k, L, T, B0, S, kind = CASES[i]
    B = B or B0
    sd = orc.random_state_dict(U, k, L, T, seed=i)
    x = orc.random_onehot(B, L, seed=i + 1, n_frac=n_frac)
    base = _codes(orc.random_onehot(B, L, seed=i + 7, n_frac=n_frac)) if kind == "codes" else kind
    dl = np.random.default_rng(i + 2).standard_normal((B, T)).astype(np.float32)
    return sd, x, base, dl


def _reference(sd, x, base, dl, S):
    """dict(ref, r32, dF, rows): the fp64 brute force, the same in fp32, F(x) - F(x'), the rows kept."""
    xb = pm.baseline_dense(base, x.astype(np.float64))
    ref, dF = pm.brute_force(sd, x, xb, dl, S, torch.float64)
    r32, _ = pm.brute_force(sd, x, xb, dl, S, torch.float32)
    return dict(ref=ref, r32=r32, dF=dF, rows=~pm.knife_rows(sd, x, xb, S, KNIFE))


@functools.lru_cache(maxsize=None)
def _case_reference(i):
    """Computed once per case and shared (read-only) by the tests that need it."""
    sd, x, base, dl = _inputs(i)
    return _reference(sd, x, base, dl, CASES[i][5])


def _within_cap(excluded):
    return excluded.sum() <= len(excluded) // 4 and (~excluded).sum() >= 2


def _bound(r):
    scale = np.abs(r["ref"]).max()
    rows = r["rows"]
    err32 = np.abs(r["r32"][rows] - r["ref"][rows]).max() / scale if scale > 0 else 0.0
    return scale, max(5e-5, 3 * err32), err32


def _check(got, r, what):
    rows = r["rows"]
    assert _within_cap(~rows), "%s: %d of %d sequences hold a knife edge" % (what, (~rows).sum(), len(rows))
    scale, bound, err32 = _bound(r)
    assert np.isfinite(got).all(), what
    if scale == 0:                 # every unit's ReLU closed along the path: the attribution is exactly zero
        assert np.abs(got).max() == 0, what
        return
    err = np.abs(got[rows] - r["ref"][rows]).max() / scale
    print("%s: error %.3g of max|ref|, bound %.3g (torch fp32 %.3g), %d of %d rows excluded" % (
        what, err, bound, err32, (~rows).sum(), len(rows)))
    record_margin("integrated gradients vs brute force", err, bound)
    assert err <= bound, "%s: ig error %.3g (torch fp32 %.3g)" % (what, err, err32)


def _run(m, x, base, dl, S, **kw):
    bl = torch.tensor(base, device="cuda") if not isinstance(base, str) else base
    ig, lx, lb = m.integrated_gradients(torch.tensor(x, device="cuda"), torch.tensor(dl, device="cuda"), bl, S, **kw)
    return ig.cpu().numpy(), lx.cpu().numpy(), lb.cpu().numpy()


@pytest.mark.parametrize("i", range(len(CASES)), ids=["U%d-k%d-L%d-T%d-B%d-S%d-%s" % c for c in CASES])
def test_vs_brute_force(i):
    U, k, L, T, B, S, kind = CASES[i]
    sd, x, base, dl = _inputs(i)
    m = make_model(sd, U, k, L, T).eval()
    ig, lx, lb = _run(m, x, base, dl, S)
    r = _case_reference(i)
    _check(ig, r, "case %d" % i)
    # endpoint logits: the model's own forward at both ends (the dense path's for a soft baseline)
    xb = pm.baseline_dense(base, x).astype(np.float32)
    with torch.no_grad():
        fx = m(torch.tensor(x, device="cuda")).cpu().numpy()
        m.dense_input = kind == "uniform" or None
        fb = m(torch.tensor(xb, device="cuda")).cpu().numpy()
        m.dense_input = None
    assert np.abs(lx - fx).max() <= TOL and np.abs(lb - fb).max() <= TOL, (np.abs(lx - fx).max(), np.abs(lb - fb).max())
    # column sums: within 4 L elementwise bounds of the reference's
    scale, bound, _ = _bound(r)
    rows = r["rows"]
    d = np.abs(ig[rows].sum(axis=(1, 2)) - r["ref"][rows].sum(axis=(1, 2))).max()
    assert d <= 4 * L * bound * scale, (d, 4 * L * bound * scale)
    # determinism
    ig2, lx2, lb2 = _run(m, x, base, dl, S)
    assert np.array_equal(ig, ig2) and np.array_equal(lx, lx2) and np.array_equal(lb, lb2)
    if kind == "uniform":
        assert (np.abs(ig) > 0).all(axis=1).any()
    pend = 7 * ((L - k + 1) // 7) + k - 1
    assert (ig[:, :, pend:] == 0).all()                # positions whose windows all fall in the dropped tail


def test_sub_batch_invariance():
    U, k, L, T, _, S, _ = CASES[2]
    B = 200
    sd, x, base, dl = _inputs(2, B)
    m = make_model(sd, U, k, L, T).eval()
    full = _run(m, x, base, dl, S)
    small = m.integrated_gradients_workspace_bytes(64)
    assert small < m.integrated_gradients_workspace_bytes(B)
    ws = torch.empty(small, dtype=torch.uint8, device="cuda")
    one = _run(m, x, base, dl, S, workspace=ws)
    h = B // 2
    halves = [_run(m, x[s], base[s], dl[s], S) for s in (slice(0, h), slice(h, B))]
    for a, b, c, d in zip(full, one, halves[0], halves[1]):
        assert np.array_equal(a, b), "result depends on the sub-batch split"
        assert np.array_equal(a, np.concatenate([c, d])), "result depends on the batch"
    with pytest.raises(RuntimeError):
        _run(m, x, base, dl, S, workspace=ws[:small - 1])


def test_identity_baseline_is_exact_zero():
    U, k, L, T, B, S, _ = CASES[2]
    sd, x, _, dl = _inputs(2)
    m = make_model(sd, U, k, L, T).eval()
    ig, lx, lb = _run(m, x, _codes(x), dl, S)
    assert (ig == 0).all() and np.array_equal(lx, lb)


def test_one_step():
    U, k, L, T, B, _, _ = CASES[1]
    sd, x, base, dl = _inputs(1)
    m = make_model(sd, U, k, L, T).eval()
    ig, _, _ = _run(m, x, base, dl, 1)
    _check(ig, _reference(sd, x, base, dl, 1), "steps = 1")


def test_errors():
    from explainn_amd import _lib
    U, k, L, T, B, S, _ = CASES[1]
    sd, x, base, dl = _inputs(1)
    m = make_model(sd, U, k, L, T)
    with pytest.raises(RuntimeError):
        _run(m, x, base, dl, S)                      # train mode
    m.eval()
    with pytest.raises(ValueError):
        _run(m, x, base, dl, 0)
    with pytest.raises(ValueError):
        _run(m, x, base[:, :-1], dl, S)
    with pytest.raises(ValueError):
        _run(m, x, base[:-1], dl, S)
    with pytest.raises(ValueError):
        _run(m, x, "shuffle", dl, S)
    with pytest.raises(ValueError):
        _run(m, x * 0.5, base, dl, S)                # not one-hot
    m.dense_input = True
    with pytest.raises(ValueError):
        _run(m, x, base, dl, S)
    m.dense_input = None
    # C ABI: dense mode is unsupported; steps < 1 and `codes` without codes are argument errors
    dev = m._device()
    ctx = m._context(B, dev)
    ps, _ = m._params_struct(dev)
    lib, h, st = ctx.lib, ctx.handle, m._stream(dev)
    xt, dlt, bt = torch.tensor(x, device=dev), torch.tensor(dl, device=dev), torch.tensor(base, device=dev)
    ig, lx, lb = torch.empty(B, 4, L, device=dev), torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)
    nb = int(lib.explainn_integrated_gradients_workspace_bytes(h, B))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def call(kind=_lib.IG_BASELINE_CODES, codes=bt.data_ptr(), steps=S):
        return lib.explainn_integrated_gradients(h, xt.data_ptr(), B, C.byref(ps), kind, codes, dlt.data_ptr(), steps,
                                                 ig.data_ptr(), lx.data_ptr(), lb.data_ptr(), ws.data_ptr(), nb, st)
    _lib.check(lib.explainn_dense_input(h, 1))
    assert call() == _lib.E_UNSUPPORTED
    _lib.check(lib.explainn_dense_input(h, 0))
    assert call(steps=0) == _lib.E_ARG
    assert call(codes=None) == _lib.E_ARG
    assert call(kind=7) == _lib.E_ARG
    _lib.check(call())
    torch.cuda.synchronize()
    assert np.array_equal(ig.cpu().numpy(), _run(m, x, base, dl, S)[0])


def test_state_rules():
    from explainn_amd import _lib
    U, k, L, T, B, S, _ = CASES[1]
    sd, x, base, dl = _inputs(1)
    m = make_model(sd, U, k, L, T).eval()
    xt = torch.tensor(x, device="cuda")
    with torch.no_grad():
        before = m(xt).clone()
    dev = m._device()
    ctx = m._context(B, dev)
    ps, _ = m._params_struct(dev)
    lib, h, st = ctx.lib, ctx.handle, m._stream(dev)
    logits = torch.empty(B, T, device=dev)
    _lib.check(lib.explainn_forward_train(h, xt.data_ptr(), B, C.byref(ps), None, 0.0, C.c_uint64(1),
                                          logits.data_ptr(), st))
    dlt, bt = torch.tensor(dl, device=dev), torch.tensor(base, device=dev)
    ig, lx, lb = torch.empty(B, 4, L, device=dev), torch.empty(B, T, device=dev), torch.empty(B, T, device=dev)
    nb = int(lib.explainn_integrated_gradients_workspace_bytes(h, B))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(lib.explainn_integrated_gradients(h, xt.data_ptr(), B, C.byref(ps), _lib.IG_BASELINE_CODES, bt.data_ptr(),
                                                 dlt.data_ptr(), S, ig.data_ptr(), lx.data_ptr(), lb.data_ptr(),
                                                 ws.data_ptr(), nb, st))
    assert lib.explainn_backward(h, dlt.data_ptr(), B, C.byref(ps), C.byref(_lib.Grads()), 0, st) == _lib.E_STATE
    torch.cuda.synchronize()
    # the train forward above moved the running statistics: a fresh model holds the parameters `before` saw
    m2 = make_model(sd, U, k, L, T).eval()
    with torch.no_grad():
        first = m2(xt).clone()
        m2.integrated_gradients(xt, dlt, bt, S)
        after = m2(xt)
    assert torch.equal(first, before) and torch.equal(after, before)


def test_reverse_complement_and_input_forms():
    from explainn_amd import interpret
    U, k, L, T, B, S, _ = CASES[2]
    sd, x, base, _ = _inputs(2)
    m = make_model(sd, U, k, L, T).eval()
    dl = np.zeros((B, T), np.float32); dl[:, 1] = 1
    for rc in (False, True):
        got = interpret.integrated_gradients(m, _codes(x), base, target=1, steps=S, batch_size=48, rev_complement=rc)
        xin = x[:, ::-1, ::-1].copy() if rc else x
        bin_ = np.where(base < 4, 3 - base, base)[:, ::-1].copy() if rc else base
        r = _reference(sd, xin, bin_, dl, S)
        if rc:
            r["ref"], r["r32"] = r["ref"][:, ::-1, ::-1], r["r32"][:, ::-1, ::-1]
        _check(got, r, "rev_complement=%s" % rc)
        onehot = interpret.integrated_gradients(m, x, base, target=1, steps=S, batch_size=48, rev_complement=rc)
        assert np.allclose(onehot, got, rtol=0, atol=1e-6 * np.abs(r["ref"]).max())
    with pytest.raises(ValueError):
        interpret.integrated_gradients(m, x, base[:, :-1], steps=S)


def test_several_baselines_and_delta():
    from explainn_amd import interpret
    U, k, L, T, B, S, _ = CASES[1]
    sd, x, _, _ = _inputs(1)
    m = make_model(sd, U, k, L, T).eval()
    bases = np.stack([_codes(orc.random_onehot(B, L, seed=40 + r, n_frac=0.02)) for r in range(3)], axis=1)
    got, delta = interpret.integrated_gradients(m, x, bases, steps=S, return_delta=True)
    single = [interpret.integrated_gradients(m, x, bases[:, r], steps=S, return_delta=True) for r in range(3)]
    mean = np.mean([s[0].astype(np.float64) for s in single], axis=0)
    assert np.abs(got - mean).max() <= 1e-6 * np.abs(mean).max()
    dmean = np.mean([s[1].astype(np.float64) for s in single], axis=0)
    assert np.abs(delta - dmean).max() <= 1e-5 * max(1.0, np.abs(dmean).max())
    # the delta is what its definition says, from the model's own forward
    with torch.no_grad():
        F = [m(torch.tensor(pm.codes_to_dense(c).astype(np.float32), device="cuda")).sum(dim=1).cpu().numpy()
             for c in (_codes(x), bases[:, 0])]
    d0 = single[0][0].sum(axis=(1, 2)) - (F[0] - F[1])
    assert np.abs(single[0][1] - d0).max() <= 4 * TOL


def test_cross_check_against_input_gradient_loop():
    from explainn_amd import interpret
    U, k, L, T, B, S, _ = CASES[4]
    sd, x, _, _ = _inputs(4, n_frac=0.0)
    m = make_model(sd, U, k, L, T).eval()
    got = interpret.integrated_gradients(m, x, "zero", steps=S)
    loop = np.zeros(x.shape, dtype=np.float64)
    for s in range(S):
        loop += interpret.input_gradients(m, (np.float32((s + 0.5) / S) * x).astype(np.float32), batch_size=B)
    loop *= x / S
    rows = ~pm.knife_rows(sd, x, np.zeros_like(x), S, KNIFE)
    assert _within_cap(~rows)
    err = np.abs(got[rows] - loop[rows]).max() / np.abs(loop).max()
    assert err <= 5e-5, err


def test_bank_member():
    from explainn_amd import ExplaiNNBank
    U, k, L, T, B, S, _ = CASES[1]
    sd, x, base, dl = _inputs(1)
    alone = [make_model(orc.random_state_dict(U, k, L, T, seed=50 + g), U, k, L, T).eval() for g in range(2)]
    bank = ExplaiNNBank.from_models(alone).cuda().eval()
    with pytest.raises(ValueError):
        bank.integrated_gradients(torch.tensor(x, device="cuda"), torch.tensor(dl, device="cuda"))
    for a, b in zip(_run(bank.member(1), x, base, dl, S), _run(alone[1], x, base, dl, S)):
        assert np.array_equal(a, b)


def test_cli(tmp_path):
    from explainn_amd import attribution, interpret
    from explainn_amd.sequence import dinucleotide_shuffle
    U, k, L, T, B = 6, 9, 60, 2, 5
    sd = orc.random_state_dict(U, k, L, T, seed=12)
    codes = _codes(orc.random_onehot(B, L, seed=13, n_frac=0.02))
    m = make_model(sd, U, k, L, T).eval()
    ckpt = os.path.join(tmp_path, "model.pth.tar")
    torch.save({"options": dict(m._options), "state_dict": {key: v.cpu() for key, v in m.state_dict().items()}},
               ckpt)
    fa = os.path.join(tmp_path, "seqs.fa")
    with open(fa, "w") as fh:
        for i, row in enumerate(codes):
            fh.write(">s%d desc\n%s\n" % (i, "".join("ACGTN"[c] for c in row)))
    out = os.path.join(tmp_path, "ig.npz")
    attribution.main([ckpt, fa, "-o", out, "--baseline", "shuffle", "--n-shuffles", "2", "--steps", "6",
                      "--target", "1", "-r", "-b", "3"])
    got = np.load(out)
    assert list(got["ids"]) == ["s%d" % i for i in range(B)]
    ref, delta = interpret.integrated_gradients(m, codes, dinucleotide_shuffle(codes, 2, 0), target=1, steps=6,
                                                rev_complement=True, return_delta=True)
    assert np.array_equal(got["ig"], ref) and np.array_equal(got["delta"], delta)
