"""Unit groups of the combiner launch that carries the head backward's batch sums
(EXPLAINN_HEAD_GROUPS; head.hip logits_bn_kernel<T> / head_sums / launch_head_fwd_sums): R blocks per
64 sequences repeat the logits; block 0 stores, the other R - 1 share the units of the batch sums.

Every sum keeps its order whatever R is -- the logits are summed by every group exactly as by the one
block of R = 1, and a (unit, block) row of the partials is formed by one thread group either way -- so
a step at R = 2, 4 or 8 must equal the step at R = 1 bit for bit: logits, loss, the whole flat
gradient and every buffer (BatchNorm3's running statistics among them).  The step's d loss / d logits
stays inside the context and has no accessor; passA forms dz of every (unit, sequence) from it and the
combiner's bias gradient is its sum, so it is held through the flat gradient.  The same cases at the
default R are checked against the fp64 oracle with the bounds of parity_util, which guards against
both forms being wrong together; the 1025-unit case has a test of its own (below), because the bar
parity_util sets for the tensors in front of the head is not a fixed number there.

Shapes (k = 9, L = 74: nine pooled positions, the smallest bucket): U = 3 (R = 4: one unit per unit
group; R = 8 clamped to that), U = 5 and 9 (uneven shares), U = 129 (all in one unit group at R = 2:
with four tasks a thread holds one unit per trip, so that group takes a second trip; 43 units each at
R = 4), U = 1025 (unit groups of 146 and 147 units at R = 8; 1025 at R = 2 and 341 / 342 at R = 4
against the 384 unit slots of one trip); B = 513 (the route's lower
edge: one live sequence in the last block), 577, 1024; T = 1 by default, T = 2 and 4 with
EXPLAINN_HEAD_PARTIALS=1; one case with N bases, one with the MSE loss.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import explainn_oracle as orc  # noqa: E402
import parity_util  # noqa: E402
from parity_util import check_grads, close, close_rel, compare_grads, GRAD_TOL_ORACLE, model, oracle_step, to_np  # noqa: E402

pytestmark = pytest.mark.gpu

K, L = 9, 74
# (U, T, B, loss, fraction of N bases)
CASES = [
    (3, 1, 513, "binary", 0.01),
    (5, 1, 577, "binary", 0.01),
    (9, 1, 1024, "binary", 0.01),
    (9, 1, 513, "binary", 0.2),
    (129, 1, 513, "binary", 0.01),
    (1025, 1, 577, "binary", 0.01),
    (9, 2, 577, "linear", 0.01),
    (5, 4, 1024, "binary", 0.01),
    (129, 4, 577, "binary", 0.01),
]
BIG = (1025, 1, 577, "binary", 0.01)


def _id(c):
    return "U%d_T%d_B%d_%s%s" % (c[0], c[1], c[2], c[3], "_N" if c[4] > 0.1 else "")


IDS = [_id(c) for c in CASES]
ORACLE_CASES = [c for c in CASES if c != BIG]
HEAD_KEYS = ("final.", "linears.10.", "linears.11.")   # the combiner, FC2, BatchNorm3: what the head backward produces

_INPUTS = {}


def _inputs(case):
    """(state dict, x, y) of a case, made once and never written to"""
    if case not in _INPUTS:
        U, T, B, loss, n_frac = case
        sd = orc.random_state_dict(U, K, L, T, seed=7 * U + T)
        x = orc.random_onehot(B, L, seed=B + T, n_frac=n_frac)
        rng = np.random.default_rng(B + 31 * U)
        y = (rng.random((B, T)) > 0.5).astype(np.float32) if loss == "binary" else rng.normal(0, 1, (B, T)).astype(np.float32)
        _INPUTS[case] = (sd, x, y)
    return _INPUTS[case]


def _engine(case, groups, monkeypatch, max_batch=None, partials="1"):
    """A fresh model, context and StepEngine; the knob is read when the context is made."""
    from explainn_amd.engine import StepEngine
    U, T, B, loss, _ = case
    monkeypatch.setenv("EXPLAINN_HEAD_PARTIALS", partials)
    if groups is None:
        monkeypatch.delenv("EXPLAINN_HEAD_GROUPS", raising=False)
    else:
        monkeypatch.setenv("EXPLAINN_HEAD_GROUPS", str(groups))
    m = model(_inputs(case)[0], U, K, L, T).train()
    m.dropout_p = 0.0
    return m, StepEngine(m, max_batch or B, loss=loss)


def _step(m, eng, x, y, per_unit=False):
    """One step; what it left: logits, loss, flat gradient, buffers.  per_unit: the route with the
    per-unit head backward launch (EXPLAINN_HEAD_PARTIALS=0) is expected, not the combiner's sums."""
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    eng.ctx.stage_timing(True)                         # the stages a step records show its route
    logits, ls = eng.step(xt, yt)
    torch.cuda.synchronize()
    stages = eng.ctx.stage_times()
    eng.ctx.stage_timing(False)
    assert "head_fwd" in stages and "passA" in stages and "loss" not in stages, stages
    assert ("head_bwd" in stages) == per_unit, stages
    out = {"logits": logits.detach().clone(), "loss": ls.detach().clone(), "flat_grad": eng.flat_grad.detach().clone()}
    for key, v in m.named_buffers():
        out["buffer " + key] = v.detach().clone()
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].shape == b[key].shape, (what, key)
        assert torch.isfinite(a[key].float()).all(), (what, key)
        if not torch.equal(a[key], b[key]):
            d = (a[key].double() - b[key].double()).abs()
            raise AssertionError("%s: %s differs in %d of %d elements, max|d| %.3e" % (
                what, key, int((d > 0).sum()), d.numel(), float(d.max())))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_groups_equal_one_group_bit_for_bit(case, monkeypatch):
    _, x, y = _inputs(case)
    one = _step(*_engine(case, 1, monkeypatch), x, y)
    assert any(k.endswith("running_var") for k in one) and float(one["flat_grad"].abs().max()) > 0
    for groups in (2, 4, 8):
        got = _step(*_engine(case, groups, monkeypatch), x, y)
        _same(got, one, "%d groups against one" % groups)


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[_id(c) for c in ORACLE_CASES])
def test_default_groups_vs_oracle(case, monkeypatch):
    """One step at the default R against the fp64 oracle, every gradient and buffer."""
    U, T, B, loss, _ = case
    sd, x, y = _inputs(case)
    ref_logits, ref_loss, ref_grads, nb = oracle_step(sd, x, y, kind=loss)
    m, eng = _engine(case, None, monkeypatch)
    got = _step(m, eng, x, y)
    close(to_np(got["logits"]), ref_logits, what="logits")
    close(float(got["loss"].item()), ref_loss, tol=1e-5, what="loss")
    check_grads([(key, v) for (key, _), v in zip(m.named_parameters(), eng.views)], ref_grads, "default groups ")
    for key, v in nb.items():
        if "tracked" in key:
            assert int(got["buffer " + key].item()) == int(v), key
        else:
            close_rel(to_np(got["buffer " + key]), v, tol=GRAD_TOL_ORACLE, what=key)


def test_1025_units_head_vs_oracle_and_front_vs_per_unit_route(monkeypatch):
    """U = 1025 at the default R, each half of the step against a reference that does not move.

    What the head backward produces -- logits, loss, the buffers, and the gradients of the combiner, FC2
    and BatchNorm3 -- against the fp64 oracle at the FIXED bound GRAD_TOL_ORACLE, with the oracle's
    knife-edge masks.  parity_util's other bar, three times the error of the stock-PyTorch fp32 CPU step,
    is not used here: at 1025 units x 100 channels x 577 sequences that step itself flips ReLU signs
    outside the mask, differently for each torch thread count, and the bar for linears.7.bias then lies
    anywhere between 5e-5 and 5e-2 (the device is 9e-4 from the oracle on that tensor, with the
    per-unit head backward as with the combiner's sums: DESIGN.md section 9 (0)).

    The gradients in front of the head against the same step with EXPLAINN_HEAD_PARTIALS=0: the
    per-unit head_bwd kernel, which shares nothing with head_sums or passA's prologue, feeding the same
    kernels behind it.  Both steps share the forward, hence its ReLU and pooling decisions, so no row
    can flip between them; they differ by how dz is rounded (fp64 batch sums added in another order,
    another expression for dz: an ulp of dz per element, 6e-8) where each route on its own is allowed
    GRAD_TOL_ORACLE for the dozens of such roundings per element that separate it from the truth.
    So they must agree within GRAD_TOL_ORACLE of the tensor's maximum (linears.1.bias, a near-null
    tensor: of its sibling's, as parity_util scales it)."""
    U, T, B, loss, _ = BIG
    sd, x, y = _inputs(BIG)
    ref_logits, _, nb = orc.forward(sd, x, training=True, return_cache=True)
    lg64, cache, _ = orc.forward(sd, x, training=True, return_cache=True, dtype=np.float64)
    ref_loss, _ = orc.bce_with_logits(ref_logits, y)
    _, dl = orc.bce_with_logits(lg64, y.astype(np.float64))
    ref_grads = orc.backward(cache, dl)

    m, eng = _engine(BIG, None, monkeypatch)
    got = _step(m, eng, x, y)
    grads = [(key, to_np(v)) for (key, _), v in zip(m.named_parameters(), eng.views)]
    close(to_np(got["logits"]), ref_logits, what="1025 units logits")
    close(float(got["loss"].item()), ref_loss, tol=1e-5, what="1025 units loss")
    for key, v in nb.items():
        if "tracked" in key:
            assert int(got["buffer " + key].item()) == int(v), key
        else:
            close_rel(to_np(got["buffer " + key]), v, tol=GRAD_TOL_ORACLE, what="1025 units " + key)
    head = [(key, g) for key, g in grads if key.startswith(HEAD_KEYS)]
    assert len(head) == 6, [key for key, _ in head]
    compare_grads(head, ref_grads, GRAD_TOL_ORACLE, cache, U, "1025 units head ")

    m0, eng0 = _engine(BIG, None, monkeypatch, partials="0")
    got0 = _step(m0, eng0, x, y, per_unit=True)
    assert torch.equal(got["logits"], got0["logits"]), "logits differ from the per-unit kernel's route"
    grads0 = {key: to_np(v) for (key, _), v in zip(m0.named_parameters(), eng0.views)}
    sib = float(np.abs(grads0["linears.1.weight"]).max())
    front = [(key, g) for key, g in grads if not key.startswith(HEAD_KEYS)]
    assert len(front) == 8, [key for key, _ in front]
    problems = []
    for key, g in front:
        g0 = grads0[key]
        assert np.isfinite(g).all(), key
        if key in parity_util.ZERO_GRAD:
            assert np.abs(g).max() < 1e-6 and np.abs(g0).max() < 1e-6, key
            continue
        scale = float(np.abs(g0).max())
        if key == parity_util.NEAR_NULL:
            scale = max(scale, sib)
        err = float(np.abs(g.astype(np.float64) - g0).max())
        print("%-18s max|d| %.3e = %.2e of scale %.3g (bound %.1e)" % (key, err, err / scale, scale, GRAD_TOL_ORACLE))
        if err > GRAD_TOL_ORACLE * scale + parity_util.GRAD_ABS_FLOOR:
            problems.append("%s: %.2e of scale %.3g" % (key, err / scale, scale))
    assert not problems, "in front of the head, against the per-unit route: " + "; ".join(problems)


@pytest.mark.parametrize("groups", [None, 8])
def test_smaller_batch_after_larger_equals_fresh_context(groups, monkeypatch):
    """A step of 1024 sequences, then one of 513 on the same context: the second equals a fresh
    context's bit for bit -- no row of hp / hb that the larger batch wrote leaks into it."""
    case = (9, 1, 1024, "binary", 0.01)
    _, x, y = _inputs(case)
    m, eng = _engine(case, groups, monkeypatch)
    _step(m, eng, x, y)
    used = _step(m, eng, x[:513], y[:513])
    m1, eng1 = _engine(case, groups, monkeypatch, max_batch=1024)
    fresh = _step(m1, eng1, x[:513], y[:513])
    for key in [k for k in used if k.startswith("buffer ")]:
        used.pop(key); fresh.pop(key)                  # (the used model's running statistics have two steps in them)
    _same(used, fresh, "second step against a fresh context")
