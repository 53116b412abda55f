"""Input gradients on the device (csrc/inputgrad.hip): x.grad of the fused forward, eval and train
mode, against torch.autograd on the fp64 restatement of the reference forward (oracle/torch_ref.py).
Bound: relative to max|ref|, 5e-5 or 3x what torch_ref in fp32 makes on the same case
(tests/parity_util.py's rule).  Sequences with a ReLU knife edge in the fp64 intermediates (where two
correct fp32 implementations may take different branches) are left out of the comparison."""
import numpy as np
import pytest
import torch

from conftest import record_margin
from oracle import explainn_oracle as orc
from oracle import torch_ref
from parity_util import KNIFE, model as make_model

pytestmark = pytest.mark.gpu


def _ref_dx(sd, x, training, keep, dl, dtype):
    sdt = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in sd.items() if "tracked" not in k}
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    logits = torch_ref.forward(sdt, xt, training, 0.3 if keep is not None else 0.0,
                               None if keep is None else torch.tensor(keep, dtype=dtype))
    (logits * torch.tensor(dl, dtype=dtype)).sum().backward()
    return xt.grad.numpy().astype(np.float64)


def _knife_rows(sd, x, training, keep):
    _, cache, _ = orc.forward(sd, x, training=training, dropout_mask=keep, dtype=np.float64,
                              return_cache=True)
    B = x.shape[0]
    y2 = np.abs(np.asarray(cache["y2"]).reshape(B, -1)).min(axis=1)
    y3 = np.abs(np.asarray(cache["y3"]).reshape(B, -1)).min(axis=1)
    return (y2 < KNIFE) | (y3 < KNIFE)


def _within_cap(knife):
    """The knife-edge exclusion stays an exception: at most a quarter of the batch's sequences, and
    at least two are compared."""
    return knife.sum() <= len(knife) // 4 and (~knife).sum() >= 2


def _check(got, sd, x, training, keep, dl, what, cap=False):
    """cap: also require _within_cap of the excluded sequences (the cases of the entry sweep, whose
    unit counts keep the exclusion rare; the full-size shapes above exclude more)."""
    ref = _ref_dx(sd, x, training, keep, dl, torch.float64)
    r32 = _ref_dx(sd, x, training, keep, dl, torch.float32)
    # a flip moves its own sequence by a channel's share; in train mode it also moves every other
    # sequence through the batch statistics, by ~1/B of that: those stay in
    rows = ~_knife_rows(sd, x, training, keep)
    if cap:
        assert _within_cap(~rows), "%s: %d of %d sequences hold a knife edge" % (what, (~rows).sum(), len(rows))
    scale = np.abs(ref).max()
    if scale == 0:                 # every unit's ReLU closed: the gradient is exactly zero
        assert np.abs(got).max() == 0, what
        return
    err = np.abs(got[rows] - ref[rows]).max() / scale
    err32 = np.abs(r32[rows] - ref[rows]).max() / scale
    record_margin("input_grad %s vs oracle" % ("train" if training else "eval"), err, max(5e-5, 3 * err32))
    assert err <= max(5e-5, 3 * err32), "%s: dx error %.3g (torch fp32 %.3g)" % (what, err, err32)


def _case(U, k, L, T, B, seed, n_frac=0.02):
    sd = orc.random_state_dict(U, k, L, T, seed=seed)
    x = orc.random_onehot(B, L, seed=seed + 1, n_frac=n_frac)
    dl = np.random.default_rng(seed + 2).standard_normal((B, T)).astype(np.float32)
    return sd, x, dl


def _eval_dx(m, x, dl):
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    logits = m(xt)
    logits.backward(torch.tensor(dl, device="cuda"))
    return xt.grad.cpu().numpy(), logits.detach()


def _train_dx(m, x, dl, keep=None):
    m.train()
    if keep is not None:
        m.set_dropout_mask(torch.tensor(keep, device="cuda"))
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    logits = m(xt)
    logits.backward(torch.tensor(dl, device="cuda"))
    return xt.grad.cpu().numpy(), logits.detach()


EVAL = [(1, 2, 50, 1, 2), (3, 5, 60, 1, 64), (8, 19, 200, 50, 300), (100, 32, 150, 1, 256),
        (300, 19, 200, 1, 1024), (8, 19, 1000, 50, 128)]


@pytest.mark.parametrize("shape", EVAL, ids=["U%d-k%d-L%d-T%d-B%d" % s for s in EVAL])
def test_eval_input_grad_vs_oracle(shape):
    U, k, L, T, B = shape
    sd, x, dl = _case(U, k, L, T, B, seed=U + k)
    m = make_model(sd, U, k, L, T).eval()
    dx, logits = _eval_dx(m, x, dl)
    _check(dx, sd, x, False, None, dl, "eval %s" % (shape,))
    with torch.no_grad():
        plain = m(torch.tensor(x, device="cuda"))
    assert torch.equal(plain, logits), "eval-keep logits differ from plain eval"
    dx2, _ = _eval_dx(m, x, dl)
    assert np.array_equal(dx, dx2), "two runs differ"


TRAIN = [(3, 5, 60, 1, 64), (8, 19, 200, 50, 512), (8, 19, 200, 1, 1024), (100, 2, 100, 1, 200),
         (1, 32, 120, 1, 96), (300, 19, 200, 1, 1024), (8, 19, 1000, 50, 256)]


@pytest.mark.parametrize("shape", TRAIN, ids=["U%d-k%d-L%d-T%d-B%d" % s for s in TRAIN])
def test_train_input_grad_vs_oracle(shape):
    U, k, L, T, B = shape
    sd, x, dl = _case(U, k, L, T, B, seed=2 * U + k)
    keep = (np.random.default_rng(U).random((B, 100 * U)) > 0.3).astype(np.uint8)
    m = make_model(sd, U, k, L, T)
    dx, _ = _train_dx(m, x, dl, keep)
    _check(dx, sd, x, True, keep.astype(np.float64), dl, "train %s" % (shape,))


def test_train_gradients_bit_identical_with_and_without_dx():
    U, k, L, T, B = 8, 19, 200, 3, 256
    sd, x, dl = _case(U, k, L, T, B, seed=5)
    keep = (np.random.default_rng(1).random((B, 100 * U)) > 0.3).astype(np.uint8)
    outs = []
    for want in (False, True):
        m = make_model(sd, U, k, L, T).train()
        m.set_dropout_mask(torch.tensor(keep, device="cuda"))
        xt = torch.tensor(x, device="cuda", requires_grad=want)
        logits = m(xt)
        logits.backward(torch.tensor(dl, device="cuda"))
        outs.append((logits.detach().cpu(), [p.grad.cpu() for p in m.parameters()], xt.grad))
    (l0, g0, x0), (l1, g1, x1) = outs
    assert x0 is None and x1 is not None
    assert torch.equal(l0, l1)
    assert len(g0) == 14
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


def test_soft_input_and_autograd_grad():
    U, k, L, T, B = 8, 9, 100, 2, 128
    sd, _, dl = _case(U, k, L, T, B, seed=7)
    x = np.random.default_rng(3).random((B, 4, L)).astype(np.float32)
    m = make_model(sd, U, k, L, T).eval()
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    (g,) = torch.autograd.grad(m(xt), xt, torch.tensor(dl, device="cuda"))
    _check(g.cpu().numpy(), sd, x, False, None, dl, "eval soft")
    m2 = make_model(sd, U, k, L, T)
    m2.dropout_p = 0.0
    dx, _ = _train_dx(m2, x, dl)
    _check(dx, sd, x, True, None, dl, "train soft")


def test_staged_codes_reverse_complement():
    from explainn_amd import interpret
    U, k, L, T, B = 8, 19, 200, 2, 200
    sd, x, _ = _case(U, k, L, T, B, seed=11)
    codes = np.where(x.sum(axis=1) > 0, x.argmax(axis=1), 4).astype(np.uint8)
    m = make_model(sd, U, k, L, T).eval()
    for rc in (False, True):
        got = interpret.input_gradients(m, torch.tensor(codes), target=1, batch_size=64, rev_complement=rc)
        xin = x[:, ::-1, ::-1].copy() if rc else x
        dl = np.zeros((B, T), np.float32); dl[:, 1] = 1
        ref = _ref_dx(sd, xin, False, None, dl, torch.float64)
        if rc:
            ref = ref[:, ::-1, ::-1]
        rows = ~_knife_rows(sd, xin, False, None)
        err = np.abs(got[rows] - ref[rows]).max() / np.abs(ref).max()
        assert err < 5e-5, (rc, err)
        onehot = interpret.input_gradients(m, x, target=1, batch_size=64, rev_complement=rc)
        assert np.allclose(onehot, got, rtol=0, atol=1e-6 * np.abs(ref).max())


def test_integrated_gradients_riemann():
    U, k, L, T, B = 8, 19, 200, 1, 64
    sd, x, _ = _case(U, k, L, T, B, seed=13, n_frac=0.0)
    from explainn_amd import interpret
    m = make_model(sd, U, k, L, T).eval()
    steps = 16
    alphas = (np.arange(steps) + 0.5) / steps
    got = np.zeros_like(x, dtype=np.float64)
    ref = np.zeros_like(got)
    dl = np.ones((B, T), np.float32)
    for a in alphas:
        xa = (a * x).astype(np.float32)
        got += interpret.input_gradients(m, xa, target=0, batch_size=B)
        ref += _ref_dx(sd, xa, False, None, dl, torch.float64)
    got *= x / steps
    ref *= x / steps
    err = np.abs(got - ref).max() / np.abs(ref).max()
    assert err < 5e-5, err


def test_state_rules():
    U, k, L, T, B = 3, 5, 60, 1, 32
    sd, x, dl = _case(U, k, L, T, B, seed=17)
    m = make_model(sd, U, k, L, T).eval()
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    logits = m(xt)
    with torch.no_grad():
        m(torch.tensor(x, device="cuda"))           # another forward in between
    with pytest.raises(RuntimeError, match="stale"):
        logits.backward(torch.tensor(dl, device="cuda"))
