"""The scope of an eval-mode pass (strands.eval_pass / eval_mode) and the attribution drivers' common
scaffold in interpret.py.  The kernels have their own tests; here every comparison is between two runs
of the same kernels on the same batches, so every comparison is exact."""
import numpy as np
import pytest
import torch

from oracle import explainn_oracle as orc
from parity_util import model as make_model
from tests import ism_model

from explainn_amd import interpret
from explainn_amd.architectures import BaseCodes
from explainn_amd.predict import predict

pytestmark = pytest.mark.gpu

U, K, L, T, N = 6, 5, 5 + 7 * 5 + 4, 2, 5
BATCH = 2                                   # three batches, the last one ragged
FORMS = [(form, rc) for form in ("codes", "onehot") for rc in (False, True)]


def _model(seed=3):
    return make_model(orc.random_state_dict(U, K, L, T, seed=seed), U, K, L, T).eval()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def codes():
    c = np.random.default_rng(11).integers(0, 4, size=(N, L)).astype(np.uint8)
    c[1, 7] = c[4, L - 1] = 4               # an N inside a sequence and at its end
    return c


def _onehot(codes):
    return ism_model.onehot(codes).astype(np.float32)


def _by_hand(codes, form, rc, per_batch):
    """What a driver has to return: per_batch(xb, xin, i) on every batch -- xb the device batch as
    given, xin what the model takes for the strand -- its results on the host, concatenated."""
    Xs = torch.from_numpy(codes if form == "codes" else _onehot(codes))
    out = []
    with torch.no_grad():
        for i in range(0, N, BATCH):
            xb = Xs[i:i + BATCH].cuda()
            xin = BaseCodes(xb, rc) if form == "codes" else xb.flip(1, 2) if rc else xb
            out.append([t.cpu().numpy() for t in per_batch(xb, xin, i)])
    return [np.concatenate(parts) for parts in zip(*out)]


def _dlogits(B, target):
    dl = torch.zeros(B, T, device="cuda")
    dl[:, slice(None) if target is None else target] = 1.0
    return dl


def _given(codes, form):
    return codes if form == "codes" else _onehot(codes)


@pytest.mark.parametrize("form,rc", FORMS)
def test_input_gradients_equal_the_models_calls(model, codes, form, rc):
    def per_batch(xb, xin, i, target=None):
        dx = model.input_gradient(xin, _dlogits(len(xb), target))
        return (dx.flip(1, 2) if rc else dx,)

    ref, = _by_hand(codes, form, rc, per_batch)
    got = interpret.input_gradients(model, _given(codes, form), batch_size=BATCH, rev_complement=rc)
    assert got.dtype == np.float32 and got.shape == (N, 4, L)
    assert np.array_equal(got, ref)
    ref1, = _by_hand(codes, form, rc, lambda xb, xin, i: per_batch(xb, xin, i, target=1))
    got = interpret.input_gradients(model, _given(codes, form), target=1, batch_size=BATCH, rev_complement=rc,
                                    times_input=True)
    assert np.array_equal(got, ref1 * _onehot(codes))
    assert np.abs(ref1).max() > 0 and not np.array_equal(ref, ref1)


@pytest.mark.parametrize("form,rc", FORMS)
def test_integrated_gradients_equal_the_models_calls(model, codes, form, rc):
    base = np.random.default_rng(12).integers(0, 5, size=(N, L)).astype(np.uint8)
    for baselines in ("zero", base):
        def per_batch(xb, xin, i):
            dl, bl = _dlogits(len(xb), 1), baselines
            if not isinstance(bl, str):
                bl = torch.from_numpy(base[i:i + BATCH]).cuda()
                if rc and form == "onehot":     # codes are reverse-complemented with the staged batch
                    bl = torch.where(bl < 4, 3 - bl, bl).flip(1).contiguous()
            ig, lx, lb = model.integrated_gradients(xin, dl, bl, 8)
            return ig.flip(1, 2) if rc else ig, ig.sum(dim=(1, 2)) - (dl * (lx - lb)).sum(dim=1)

        ref, ref_delta = _by_hand(codes, form, rc, per_batch)
        got, delta = interpret.integrated_gradients(model, _given(codes, form), baselines, target=1, steps=8,
                                                    batch_size=BATCH, rev_complement=rc, return_delta=True)
        assert got.dtype == np.float32 and got.shape == (N, 4, L) and delta.shape == (N,)
        assert np.array_equal(got, ref) and np.array_equal(delta, ref_delta)
        assert np.abs(ref).max() > 0


@pytest.mark.parametrize("form,rc", FORMS)
def test_in_silico_mutagenesis_equals_the_models_calls(model, codes, form, rc):
    def per_batch(xb, xin, i):
        logits, delta = model.in_silico_mutagenesis(xin)
        return delta.flip(2, 3) if rc else delta, logits

    ref, logits = _by_hand(codes, form, rc, per_batch)
    got = interpret.in_silico_mutagenesis(model, _given(codes, form), batch_size=BATCH, rev_complement=rc)
    assert got.dtype == np.float32 and got.shape == (N, T, 4, L)
    assert np.array_equal(got, ref)
    got = interpret.in_silico_mutagenesis(model, _given(codes, form), target=1, batch_size=BATCH,
                                          rev_complement=rc, absolute=True)
    assert got.shape == (N, 4, L)
    assert np.array_equal(got, (ref + logits[:, :, None, None])[:, 1])


@pytest.mark.parametrize("rc", [False, True])
def test_return_logits(model, codes, rc):
    with torch.no_grad():
        fwd = model(BaseCodes(torch.from_numpy(codes).cuda(), rc)).cpu().numpy()
    for target in (None, 1):
        kwargs = dict(target=target, batch_size=BATCH, rev_complement=rc)
        delta, logits = interpret.in_silico_mutagenesis(model, codes, return_logits=True, **kwargs)
        assert logits.dtype == np.float32 and logits.shape == (N, T)
        assert np.array_equal(logits, fwd)
        assert np.array_equal(delta, interpret.in_silico_mutagenesis(model, codes, **kwargs))


def _restored(m):
    return m.training is True and m._rt.cache_depth == 0 and torch.is_grad_enabled()


def test_mode_and_scope_restored(codes):
    m = _model().train()
    x = _onehot(codes)
    for Xs in (codes, x):
        interpret.input_gradients(m, Xs, batch_size=BATCH)
        assert _restored(m)
        interpret.integrated_gradients(m, Xs, batch_size=BATCH, steps=4)
        assert _restored(m)
        interpret.in_silico_mutagenesis(m, Xs, batch_size=BATCH)
        assert _restored(m)
    res = interpret.filter_pwms(m, x, np.arange(N), batch_size=BATCH)
    assert _restored(m)
    interpret.filter_site_list(m, x, np.arange(N), res["thresholds"])
    assert _restored(m)


def test_mode_and_scope_restored_on_a_raise(codes):
    """The second batch is not one-hot: _stage refuses it (ONEHOT_ONLY) in the middle of the loop.  It read
    and cleared the flag to find that out, so nothing is left for a later check to report."""
    m = _model().train()
    x = _onehot(codes)
    x[3, :, 5] = 0.25
    with pytest.raises(ValueError, match="input is not one-hot: in-silico mutagenesis"):
        interpret.in_silico_mutagenesis(m, x, batch_size=BATCH)
    assert _restored(m)
    m.check_input()
    with pytest.raises(ValueError, match="input is not one-hot: in-silico mutagenesis"):
        interpret.integrated_gradients(m, x, batch_size=BATCH, steps=4)
    assert _restored(m)
    m.check_input()


def _used(m, codes):
    """`m` after more than two valid calls (of the model and of its replica): from here on a forward
    leaves the validation flag on the device for whoever closes the pass."""
    for _ in range(3):
        predict(m, codes)
    assert m.validate_input and not m._validate_now() and not m.eval_replica()._validate_now()
    return m


def test_two_strands_settles_both_contexts(codes):
    m = _used(_model(), codes)
    bad = codes.copy()
    bad[2, 9] = 7                           # both strands read it: the model's flag and the replica's are set
    with pytest.raises(ValueError, match="base codes must be 0..4"):
        predict(m, bad)
    assert m._rt.cache_depth == 0 and m.eval_replica()._rt.cache_depth == 0 and torch.is_grad_enabled()
    assert m.eval_replica().input_flags() == 0
    m.check_input()
    assert predict(m, codes).shape == (N, T, 4)


def test_input_gradients_settles(codes):
    """Base codes outside 0..4 are reported by the input_gradients call that was given them, as
    integrated_gradients and in_silico_mutagenesis report them.  (Before the drivers shared one scope this
    call returned, and the NEXT read of the flag -- here the check_input() below -- raised.)"""
    m = _used(_model(), codes)
    bad = codes.copy()
    bad[2, 9] = 9
    with pytest.raises(ValueError, match="base codes must be 0..4"):
        interpret.input_gradients(m, bad, batch_size=BATCH)
    assert not m.training and m._rt.cache_depth == 0
    m.check_input()
