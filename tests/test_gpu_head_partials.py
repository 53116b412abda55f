"""The head backward's batch sums formed in the combiner launch and finished in passA
(EXPLAINN_HEAD_PARTIALS; head.hip logits_bn_kernel<T> / head_sums, fc.hip passA_kernel<NQ, 2|3>): the
route of explainn_train_step for a single model with T <= 4 tasks and more than 512 sequences.

Each case runs one StepEngine.step (dropout 0) with the route forced on and checks logits, loss, every
gradient and the BatchNorm buffers against the fp64 oracle; then the same step with the route forced
off (the per-unit head_bwd_kernel): equal logits, and the same oracle bounds on that route's
gradients.  The stages a step records show which route it took: no head_bwd stage with the route on,
one with it off.  Both routes' worst gradient errors are appended to profiles/r14_head_parity_margins.txt.
The two routes need not agree bit for bit behind the logits: the fp64 batch sums are added in a
different order (blocks of 64 sequences).  -m gpu."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import explainn_oracle as orc  # noqa: E402
import parity_util  # noqa: E402
from parity_util import check_grads, close, close_rel, GRAD_TOL_ORACLE, model, oracle_step, to_np  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGINS = os.path.join(ROOT, "profiles", "r14_head_parity_margins.txt")


def _dead_units(sd, U):
    """BatchNorm3 of units 3, 7, 20 shifted so far down that o = 0 for every sequence (|zhat| <=
    sqrt(B - 1) < 26): d3 = 0 everywhere, both batch sums exactly 0; unit 5 with gamma3 < 0."""
    g3 = np.array(sd["linears.11.weight"], dtype=np.float32)
    b3 = np.array(sd["linears.11.bias"], dtype=np.float32)
    for u in (3, 7, 20):
        g3[u], b3[u] = 1.0, -40.0
    g3[5] = -0.8
    sd["linears.11.weight"], sd["linears.11.bias"] = g3, b3
    fw = np.array(sd["final.weight"], dtype=np.float32)
    fw[0, 7] = -abs(fw[0, 7]) - 0.1
    fw[0, 5] = abs(fw[0, 5]) + 0.1
    sd["final.weight"] = fw
    return sd


# (U, k, L, T, B, loss, tweak)
CASES = [
    (5, 19, 61, 1, 520, "binary", None),        # just over the 512 gate: last block of 8 live sequences, U < 16 waves
    (330, 19, 61, 4, 577, "binary", None),      # second trip of the combiner's unit loop, four tasks, odd batch
    (17, 19, 61, 2, 1024, "linear", None),      # MSE, full blocks
    (33, 19, 61, 1, 640, "binary", _dead_units),  # units with o <= 0 everywhere, a negative gamma3
    (3, 19, 249, 1, 520, "binary", None),       # n = 33: two passA row groups, dz stored by group 0 alone
]


def _inputs(U, k, L, T, B, loss, tweak):
    sd = orc.random_state_dict(U, k, L, T, seed=U + T + B)
    if tweak:
        sd = tweak(sd, U)
    x = orc.random_onehot(B, L, seed=11, n_frac=0.01)
    rng = np.random.default_rng(12)
    y = (rng.random((B, T)) > 0.5).astype(np.float32) if loss == "binary" else rng.normal(0, 1, (B, T)).astype(np.float32)
    return sd, x, y


def _step(sd, U, k, L, T, B, loss, x, y, steps=1):
    from explainn_amd.engine import StepEngine
    m = model(sd, U, k, L, T).train()
    m.dropout_p = 0.0
    eng = StepEngine(m, B, loss=loss)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    losses = []
    eng.ctx.stage_timing(True)                         # which stages the step launched proves the route taken
    for _ in range(steps):
        logits, ls = eng.step(xt, yt)
        torch.cuda.synchronize()
        losses.append(float(ls.item()))
        stages = eng.ctx.stage_times()
        assert "head_fwd" in stages and "passA" in stages and "loss" not in stages, stages
        assert ("head_bwd" in stages) == (os.environ["EXPLAINN_HEAD_PARTIALS"] == "0"), stages
    eng.ctx.stage_timing(False)
    grads = [(key, v.detach().clone()) for (key, _), v in zip(m.named_parameters(), eng.views)]
    bufs = {key: v.detach().clone() for key, v in m.named_buffers()}
    return logits.detach().clone(), losses, grads, bufs


def _worst(grads, ref_grads):
    """worst max|d| / max|ref| over the gradient tensors, off the ReLU knife-edge rows (parity_util)"""
    cache, U, _, _ = parity_util._ORACLE_CACHES[id(ref_grads)]
    _, un = parity_util.knife_masks(cache, U)
    worst, where = 0.0, ""
    for key, g in grads:
        if key in parity_util.ZERO_GRAD or key == parity_util.NEAR_NULL:
            continue
        r = np.asarray(ref_grads[key], dtype=np.float64)
        err = np.abs(to_np(g).astype(np.float64).reshape(r.shape) - r)
        if key == "final.weight":
            err = err.T[~un]
        elif key.startswith(("linears.10.", "linears.11.")):
            err = err[~un]
        elif not key.startswith("final"):
            continue                                   # (rows in front of the head: covered by check_grads)
        e = float(err.max() / np.abs(r).max()) if err.size and np.abs(r).max() > 0 else 0.0
        if e >= worst:
            worst, where = e, key
    return worst, where


def _record(label, on, off):
    try:
        with open(MARGINS, "a") as f:
            f.write("%-28s partials %.3e (%s)   per-unit kernel %.3e (%s)   bound %.1e\n" % (
                label, on[0], on[1], off[0], off[1], GRAD_TOL_ORACLE))
    except OSError:
        pass                                           # (a read-only checkout: the assertions are the test)


def _check(label, logits, loss, grads, bufs, ref_logits, ref_loss, ref_grads, nb):
    close(to_np(logits), ref_logits, what=label + " logits")
    close(loss, ref_loss, tol=1e-5, what=label + " loss")
    check_grads(grads, ref_grads, label + " ")
    for key, v in nb.items():
        if "tracked" in key:
            assert int(bufs[key].item()) == int(v), key
        else:
            close_rel(to_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what=label + " " + key)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "U%d_L%d_T%d_B%d_%s%s" % (c[0], c[2], c[3], c[4], c[5], "_dead" if c[6] else ""))
def test_head_partials_vs_oracle_and_per_unit_kernel(case, monkeypatch):
    U, k, L, T, B, loss, tweak = case
    sd, x, y = _inputs(*case)
    ref_logits, ref_loss, ref_grads, nb = oracle_step(sd, x, y, kind=loss)

    monkeypatch.setenv("EXPLAINN_HEAD_PARTIALS", "1")
    logits, losses, grads, bufs = _step(sd, U, k, L, T, B, loss, x, y)
    _check("head partials", logits, losses[0], grads, bufs, ref_logits, ref_loss, ref_grads, nb)
    if tweak:
        g = dict(grads)
        for u in (3, 7, 20):                           # d3 = 0 for every sequence: exact zeros, not noise
            assert float(g["linears.11.weight"][u]) == 0.0 and float(g["linears.11.bias"][u]) == 0.0, u

    monkeypatch.setenv("EXPLAINN_HEAD_PARTIALS", "0")
    logits0, losses0, grads0, bufs0 = _step(sd, U, k, L, T, B, loss, x, y)
    assert torch.equal(logits, logits0), "logits differ from the per-unit kernel's route"
    for key in bufs:
        assert torch.equal(bufs[key], bufs0[key]), "%s differs from the per-unit kernel's route" % key
    _check("per-unit head_bwd", logits0, losses0[0], grads0, bufs0, ref_logits, ref_loss, ref_grads, nb)
    on, off = _worst(grads, ref_grads), _worst(grads0, ref_grads)
    print("head gradients, worst error / max|ref|: partials %.3e (%s), per-unit kernel %.3e (%s)" % (on + off))
    _record("U%d L%d T%d B%d %s" % (U, L, T, B, loss), on, off)
    assert on[0] <= GRAD_TOL_ORACLE, on


def test_head_partials_three_steps(monkeypatch):
    """Three steps on one batch, parameters untouched: every step's loss is the oracle's, the running
    statistics follow its update step by step, num_batches_tracked goes up by one per step, and the
    third step's gradients are those of a single step -- nothing in hp / hb / dlogits carries over."""
    case = CASES[0]
    U, k, L, T, B, loss, _ = case
    sd, x, y = _inputs(*case)
    _, ref_loss, ref_grads, _ = oracle_step(sd, x, y, kind=loss)
    monkeypatch.setenv("EXPLAINN_HEAD_PARTIALS", "1")
    steps = 3
    _, losses, grads, bufs = _step(sd, U, k, L, T, B, loss, x, y, steps=steps)
    for i, ls in enumerate(losses):
        close(ls, ref_loss, tol=1e-5, what="step %d loss" % i)
    assert losses[0] == losses[1] == losses[2], losses
    check_grads(grads, ref_grads, "third step ")
    sd_i = dict(sd)
    for _ in range(steps):
        _, _, nb_i = orc.forward(sd_i, x, training=True, return_cache=True)
        sd_i.update(nb_i)
    for key, v in nb_i.items():
        if "tracked" in key:
            assert int(bufs[key].item()) == int(sd[key]) + steps, key
        else:
            close_rel(to_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what="%d steps %s" % (steps, key))
