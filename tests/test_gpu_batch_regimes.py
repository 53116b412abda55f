"""One train step on the batches and parameters a trained model lives on (tests/regime_model.py), against
the fp64 oracle, by the routes of the dispatch sweep: StepEngine.step, autograd forward + backward
under a given keep mask, then the eval forward from the updated buffers.  The conditions that make
these fair cases are asserted on the CPU in tests/test_regime_model.py.

  out_*    one sequence carries the consensus k-mer of a unit.  BatchNorm2's statistics are SHIFTED
           fp32 sums over the batch (qmom / qmom_big in csrc/prep.hip): with the shift at an outlier
           every other sequence sits far from it and the variance is what survives the cancellation.
           Each case runs with the planted sequence first, at B//2 + 1 and last on the same rolled
           batch; the three results, un-rolled, must also agree with each other.
  scale_*  |gamma1| to 4 (__expf far from 0), FC1 x5 through the bf16-piece fc_fwd, logits to +-100
  scale_sat_*  max |logit| 90 .. 120: BCE value and gradient past expf's range, fused and deferred loss,
           and the MSE kind on targets x100
  degen_*  variance clamps and 1/sqrt(eps) amplification: a zero filter, zero FC1 rows, FC1 rows with
           BatchNorm2 variance ~ eps, a unit whose ReLU is dead for the whole batch

Bounds are the suite's own (parity_util): logits and loss `close`, gradients GRAD_TOL_ORACLE or 3x the
reference's fp32 error (check_grads; compare_masked from B = 2048 as in the sweep), buffers
GRAD_TOL_ORACLE against the fp64 oracle's (see Ref).  One refinement: a tensor-wide maximum hides exactly the rows under test (the
largest linears.7.running_var of out_n26 belongs to an unplanted unit; the zero FC1 rows' weight
gradient is 1e5 times the others'), so every planted unit and every degenerate row set is compared
once more RELATIVE TO ITS OWN max|ref|, by the same rule with the reference's fp32 error taken on
that slice.  Order independence: each placement is within its bound of one truth, so two placements
are within twice that bound of each other.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import regime_model as rm  # noqa: E402
from conftest import record_margin  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import (ABS_FLOOR, GRAD_ABS_FLOOR, GRAD_TOL_ORACLE, NEAR_NULL, TOL, ZERO_GRAD,  # noqa: E402
                         _ORACLE_CACHES, check_grads, close, close_rel, compare_masked, knife_masks, model,
                         oracle_step, to_np)

pytestmark = pytest.mark.gpu

MASKED_MIN_B = 2048       # as in the sweep: from here on gradients are compared with compare_masked
UNIT_GRADS = ("linears.0.weight", "linears.1.weight", "linears.6.weight", "linears.7.weight", "linears.7.bias")
ROW_GRADS = UNIT_GRADS[2:]
BUFS = ("linears.7.running_mean", "linears.7.running_var")
BUF_KEYS = tuple("linears.%d.running_%s" % (i, s) for i in (1, 7, 11) for s in ("mean", "var"))


class Ref:
    """The oracle's step on a case (planted sequence at index 0) for one keep mask: computed once.
    Logits and loss from the fp32 oracle, gradients from the fp64 oracle (parity_util.oracle_step), and
    the BatchNorm buffers from the fp64 oracle too: on degen_b640 the fp32 numpy oracle's own
    linears.11.running_mean is 3.3e-5 (7.8e-5 of the tensor's maximum) off the truth on the zero-filter
    unit -- its mean over 640 identical fp32 values of h is not that value, and 1/sqrt(eps) amplifies
    the residue -- while the device agrees with the fp64 buffers (measured on MI355X)."""
    _memo = {}

    def __init__(self, c, keep):
        inp = rm.inputs(c.id)
        self.U = c.U
        if c.B < MASKED_MIN_B:
            with rm.reference_threads():
                self.logits, self.loss, self.grads, self.nb = oracle_step(inp.sd, inp.x, inp.y, keep=keep, kind=c.loss)
            self.cache, _, self.ref_err, _ = _ORACLE_CACHES[id(self.grads)]
            self.masked = False
            _, _, self.nb = orc.forward(inp.sd, inp.x, training=True, dropout_mask=keep, return_cache=True,
                                        dtype=np.float64)
            self.grads32 = self._reference_grads(inp, c, keep)
        else:
            assert c.loss == "binary"
            self.logits, _, _ = orc.forward(inp.sd, inp.x, training=True, dropout_mask=keep, return_cache=True)
            lg64, self.cache, self.nb = orc.forward(inp.sd, inp.x, training=True, dropout_mask=keep, return_cache=True,
                                              dtype=np.float64)
            self.loss, _ = orc.bce_with_logits(self.logits, inp.y)
            _, dl = orc.bce_with_logits(lg64, inp.y.astype(np.float64))
            self.grads = orc.backward(self.cache, dl)
            self.ref_err, self.masked, self.grads32 = {}, True, None
        self.ch, self.un = knife_masks(self.cache, c.U)

    @staticmethod
    def _reference_grads(inp, c, keep):
        """The reference's own fp32 gradients (what reference_fp32_error takes the tensor-wide maximum
        of): its error on a slice sets that slice's bar."""
        from oracle import torch_ref
        sdt = {k: torch.tensor(np.array(v, dtype=np.float32)) for k, v in inp.sd.items() if "tracked" not in k}
        km = None if keep is None else torch.tensor(np.asarray(keep, dtype=np.float32))
        with rm.reference_threads():
            _, _, g = torch_ref.train_step(sdt, torch.tensor(inp.x), torch.tensor(inp.y), c.loss,
                                           0.3 if keep is not None else 0.0, km)
        return {k: v.detach().numpy().astype(np.float64) for k, v in g.items()}

    @classmethod
    def of(cls, c, route):
        keep = dict(rm.routes(c.id))[route]
        key = (c.U, c.k, c.L, c.T, c.B, c.seed, c.g1, c.fc, c.fin, c.planted, c.loss, c.yscale, keep is None)
        if key not in cls._memo:
            cls._memo[key] = cls(c, keep)
        return cls._memo[key]

    def tol(self, key):
        return max(GRAD_TOL_ORACLE, 3.0 * self.ref_err.get(key, 0.0))


def _slices(c):
    """{label: (keys, row index into each key's leading axis per key kind)}: the planted units and the
    degenerate row sets, plus -- where there are degenerate sets -- the ordinary units, so that what
    the large rows would hide is compared on its own scale too."""
    inp = rm.inputs(c.id)
    units = {"planted unit %d" % u: u for u in c.planted}
    rows = {}
    if inp.sets:
        units.update(inp.sets["units"])
        rows.update(inp.sets["rows"])
        for u in range(c.U):
            if u not in rm.DEGEN_UNITS.values():
                units["ordinary unit %d" % u] = u
        for name, rr in inp.sets["rows"].items():
            u = rr[0] // rm.FC_H
            rows["other rows of the %s unit" % name] = np.setdiff1d(np.arange(u * rm.FC_H, (u + 1) * rm.FC_H), rr)
    return units, rows


def _slice_problems(label, ref, got, bufs, c):
    """Every slice of _slices relative to ITS OWN max|ref|: gradients at GRAD_TOL_ORACLE or 3x the
    reference's fp32 error on that slice, buffers at GRAD_TOL_ORACLE."""
    units, rows = _slices(c)
    problems = []

    def one(what, key, idx, is_buf):
        full = np.asarray(ref.nb[key] if is_buf else ref.grads[key], dtype=np.float64)
        r = full.reshape(full.shape[0], -1)[idx]
        g = np.asarray(bufs[key] if is_buf else got[key], dtype=np.float64).reshape(full.shape[0], -1)[idx]
        scale = np.abs(r).max()
        t = GRAD_TOL_ORACLE
        if not is_buf and ref.grads32 is not None and scale > 0:
            r32 = ref.grads32[key].reshape(full.shape[0], -1)[idx]
            t = max(t, 3.0 * np.abs(r32 - r).max() / scale)
        bound = t * scale + (GRAD_ABS_FLOOR if is_buf else ABS_FLOOR)
        err = np.abs(g - r).max()
        record_margin("rel %s %s, %s" % (label, what, key), err / bound * t, t)
        if not np.isfinite(g).all() or err > bound:
            problems.append("%s %s: max|d| %.3e = %.2e of the slice's max|ref| %.3g (bound %.1e)" % (
                what, key, err, err / max(scale, 1e-300), scale, t))

    for what, u in units.items():
        assert not ref.un[u], what
        for key in UNIT_GRADS:
            idx = np.array([u]) if key in UNIT_GRADS[:2] else np.arange(u * rm.FC_H, (u + 1) * rm.FC_H)
            one(what, key, idx, False)
        for key in BUFS:
            one(what, key, np.arange(u * rm.FC_H, (u + 1) * rm.FC_H), True)
    for what, rr in rows.items():
        rr = rr[~ref.ch.reshape(-1)[rr]]
        for key in ROW_GRADS:
            one(what, key, rr, False)
        for key in BUFS:
            one(what, key, rr, True)
    return problems


def _check(c, label, ref, r, logits, loss, named, bufs):
    """One finished step (planted sequence at index r) against the oracle's (at index 0)."""
    close(np.roll(to_np(logits), -r, axis=0), ref.logits, what=label + " logits")
    close(float(loss), float(ref.loss), what=label + " loss")
    if ref.masked:
        rep = compare_masked(named, ref.grads, ref.cache, c.U, tight=GRAD_TOL_ORACLE)
        for name, (clean, _) in rep.items():
            record_margin("rel %s masked grad %s" % (label, name), clean, GRAD_TOL_ORACLE)
    else:
        check_grads(named, ref.grads, label + " ")
    for key, v in ref.nb.items():
        if "tracked" in key:
            assert int(bufs[key].item()) == int(v), key
        else:
            close_rel(to_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what=label + " " + key)
    got = {k: to_np(v) for k, v in named}
    problems = _slice_problems(label, ref, got, {k: to_np(bufs[k]) for k in BUFS}, c)
    assert not problems, "%s: rows under test differ on their own scale:\n  " % label + "\n  ".join(problems)
    out = dict(got)
    out["logits"] = np.roll(to_np(logits), -r, axis=0)
    out.update({k: to_np(bufs[k]) for k in BUF_KEYS})
    return out


def _step(c, route, x, y, keep, max_batch=None):
    """One train step by `route` on a fresh model: (model, logits, loss, named gradients)."""
    from explainn_amd.engine import StepEngine
    inp = rm.inputs(c.id)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m = model(inp.sd, c.U, c.k, c.L, c.T).train()
    names = [n for n, _ in m.named_parameters()]
    if route == "autograd":
        if keep is None:
            m.dropout_p = 0.0
        else:
            m.set_dropout_mask(torch.from_numpy(keep))
        logits = m(xt)
        fn = torch.nn.functional.binary_cross_entropy_with_logits if c.loss == "binary" else torch.nn.functional.mse_loss
        loss = fn(logits, yt)
        loss.backward()
        grads = [p.grad for p in m.parameters()]
    else:
        m.dropout_p = 0.0
        eng = StepEngine(m, max_batch or c.B, loss=c.loss)
        logits, loss = eng.step(xt, yt)
        grads = eng.views
        m._regime_engine = eng                           # the views live in the engine's flat buffer
    torch.cuda.synchronize()
    return m, logits.detach(), loss.detach(), list(zip(names, grads))


def _eval_check(label, m, c, ref, x, r):
    sd2 = dict(rm.inputs(c.id).sd)
    sd2.update({k: np.asarray(v, dtype=np.float32) for k, v in ref.nb.items() if "tracked" not in k})
    m.eval()
    with torch.no_grad():
        got = m(torch.from_numpy(x).cuda())
    close(np.roll(to_np(got), -r, axis=0), orc.forward(sd2, rm.inputs(c.id).x), what=label + " eval logits")


def _pair_problems(label, ref, a, b):
    """Two placements of one batch, un-rolled: each is within its bound of the same truth, so they
    are within twice that bound of each other -- knife-edge rows aside, as in the comparison with
    the truth."""
    problems = []
    sib = np.abs(ref.grads["linears.1.weight"]).max()
    for key in a:
        x, z = np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64)
        err = np.abs(x - z)
        if key == "logits":
            bound = 2 * TOL * max(1.0, np.abs(ref.logits).max())
        elif key in BUF_KEYS:
            bound = 2 * (GRAD_TOL_ORACLE * np.abs(ref.nb[key]).max() + GRAD_ABS_FLOOR)
        elif key in ZERO_GRAD:
            continue
        else:
            r = np.asarray(ref.grads[key], dtype=np.float64)
            scale = np.abs(r).max()
            if key == NEAR_NULL:
                if ref.masked:
                    continue
                scale = max(scale, sib)
            bound = 2 * (ref.tol(key) * scale + ABS_FLOOR)
            err = err.reshape(r.shape)
            if key.startswith(("linears.6.", "linears.7.")):
                err = err[~ref.ch.reshape(-1)]
            elif key.startswith(("linears.0.", "linears.1.", "linears.10.", "linears.11.")):
                err = err[~ref.un]
            elif key == "final.weight":
                err = err.T[~ref.un]
        worst = err.max() if err.size else 0.0
        record_margin("pair %s %s" % (label, key), worst, bound)
        if worst > bound:
            problems.append("%s: max|d| %.3e (bound %.3e)" % (key, worst, bound))
    return problems


def _run_outlier(c):
    for route, _ in rm.routes(c.id):
        ref = Ref.of(c, route)
        res = {}
        for where in rm.PLACEMENTS:
            x, y, keep, r = rm.placed(c.id, where)
            label = "%s %s %s" % (c.id, where, route)
            m, logits, loss, named = _step(c, route, x, y, keep if route == "autograd" else None)
            res[where] = _check(c, label, ref, r, logits, loss, named, dict(m.named_buffers()))
            if route == "step":
                _eval_check(label, m, c, ref, x, r)
        problems = []
        for i, wa in enumerate(rm.PLACEMENTS):
            for wb in rm.PLACEMENTS[i + 1:]:
                problems += ["%s vs %s, %s" % (wa, wb, p)
                             for p in _pair_problems("%s %s %s/%s" % (c.id, route, wa, wb), ref, res[wa], res[wb])]
        assert not problems, "%s %s: the step depends on the order of the batch:\n  " % (c.id, route) + \
            "\n  ".join(problems)


@pytest.mark.parametrize("cid", [c.id for c in rm.OUTLIER_CASES if not c.qch])
def test_outlier_led_batch(cid):
    _run_outlier(rm.BY_ID[cid])


def test_outlier_led_batch_two_chunks(monkeypatch):
    """out_n26 with the q moments in two batch chunks (EXPLAINN_QCH = 2, fixed when the context is
    created): the outlier lies in chunk 0 only, the partials of both chunks are about one shift."""
    from explainn_amd import _lib
    c = rm.BY_ID["out_qch2"]
    geom = (c.U, c.k, c.L, c.T)
    monkeypatch.delenv("EXPLAINN_QCH", raising=False)
    monkeypatch.delenv("EXPLAINN_ACH", raising=False)
    default = _lib.Context(*geom, max_batch=c.B, device=torch.cuda.current_device())
    default_bytes = default.scratch_bytes()
    default.close()
    monkeypatch.setenv("EXPLAINN_QCH", str(c.qch))
    over = _lib.Context(*geom, max_batch=c.B, device=torch.cuda.current_device())
    assert over.scratch_bytes() < default_bytes, "the EXPLAINN_QCH override was not applied"
    over.close()
    _run_outlier(c)


@pytest.mark.parametrize("cid", [c.id for c in rm.SCALE_CASES + rm.SAT_CASES + rm.DEGEN_CASES])
def test_trained_scale_and_degenerate_parameters(cid):
    c = rm.BY_ID[cid]
    inp = rm.inputs(cid)
    for route, keep in rm.routes(cid):
        ref = Ref.of(c, route)
        label = "%s %s" % (cid, route)
        m, logits, loss, named = _step(c, route, inp.x, inp.y, keep)
        _check(c, label, ref, 0, logits, loss, named, dict(m.named_buffers()))
        if route == "step":
            _eval_check(label, m, c, ref, inp.x, 0)


def test_saturated_loss_routes():
    """The saturated cases reach both loss forms of the fused step: recomputed inside the head's
    backward (T <= FUSED_LOSS_MAX_T) and in the loss kernel of its own (above)."""
    import dispatch_model as dm
    Ts = sorted(c.T for c in rm.SAT_CASES if c.loss == "binary")
    assert Ts[0] <= dm.C["FUSED_LOSS_MAX_T"] < Ts[-1], (Ts, dm.C["FUSED_LOSS_MAX_T"])


def test_outlier_in_a_bank_member():
    """A bank of two members of out_n26's size on out_n26's batch: the planted k-mers are the consensus
    of member 1's units, first in the batch.  Member by member against the oracle (rows under test on
    their own scale for member 1) and against the members run alone (tests/test_gpu_bank.py)."""
    import copy
    from explainn_amd import ExplaiNNBank
    from explainn_amd.engine import StepEngine
    from test_gpu_bank import Case as BankCase, _against_member, _member_grads
    c = rm.BY_ID["out_n26"]
    inp = rm.inputs(c.id)
    other = rm.sweep_device(orc.random_state_dict(c.U, c.k, c.L, c.T, seed=c.seed + 77),
                            np.random.default_rng(c.seed + 78))
    sds = [other, inp.sd]
    bank = ExplaiNNBank.from_models([model(sd, c.U, c.k, c.L, c.T) for sd in sds]).cuda().train()
    bank.dropout_p = 0.0
    before = copy.deepcopy(bank)
    xt, yt = torch.from_numpy(inp.x).cuda(), torch.from_numpy(inp.y).cuda()
    eng = StepEngine(bank, c.B, "binary")
    logits, loss = eng.step(xt, yt)
    torch.cuda.synchronize()
    assert logits.shape == (c.B, 2, c.T)
    bufs = dict(bank.named_buffers())
    ref = Ref.of(c, "step")
    named = _member_grads(bank, eng.views, 1)
    mb = {k: bank._member_view(k, v, 1) for k, v in bufs.items() if "tracked" not in k}
    mb.update({k: v for k, v in bufs.items() if "tracked" in k})
    _check(c, "out_bank member 1", ref, 0, logits[:, 1], loss[1], named, mb)
    ref_logits, ref_loss, ref_grads, nb = oracle_step(other, inp.x, inp.y)
    close(to_np(logits[:, 0]), ref_logits, what="out_bank member 0 logits")
    check_grads(_member_grads(bank, eng.views, 0), ref_grads, "out_bank member 0 ")
    for key, v in nb.items():
        if "tracked" not in key:
            close_rel(to_np(bank._member_view(key, bufs[key], 0)), v, tol=GRAD_TOL_ORACLE,
                      what="out_bank member 0 " + key)
    bc = BankCase("out_bank", 2, c.U, c.k, c.L, c.T, c.B, "binary", 0, 0.0, False, False)
    for g in range(2):
        _against_member(bc, "out_bank vs member %d alone" % g, before, g, xt, yt, logits, loss, eng.views)


def test_outlier_first_in_the_second_sync_bn_shard():
    """out_n26 over two virtual ranks with the planted sequence first in rank 1's shard: that rank's
    q moments are about a shard-local shift, which sync_qmom_combine undoes before the exchange.
    Against the oracle on the whole batch and against the one-device step."""
    from explainn_amd.parallel import shard_bounds
    from test_gpu_syncbn_train import _virtual_step
    c = rm.BY_ID["out_n26"]
    inp = rm.inputs(c.id)
    bounds = [shard_bounds(c.B, 2, r) for r in range(2)]
    r = bounds[1][0]
    x, y = rm.rotate(inp.x, inp.y, r)
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    ref = Ref.of(c, "step")
    sdt = {key: torch.from_numpy(np.asarray(v)) for key, v in inp.sd.items()}
    engines, logits, losses = _virtual_step(sdt, c.U, c.k, c.L, c.T, torch.from_numpy(x).cuda(),
                                            torch.from_numpy(y).cuda(), bounds)
    assert all(torch.equal(e.flat_grad, engines[0].flat_grad) for e in engines[1:])
    one_m, one_logits, one_loss, one_named = _step(c, "step", x, y, None)
    one = _check(c, "out_sync one device", ref, r, one_logits, one_loss, one_named, dict(one_m.named_buffers()))
    for i, e in enumerate(engines):
        names = [n for n, _ in e.model.named_parameters()]
        got = _check(c, "out_sync rank %d" % i, ref, r, logits, torch.tensor(losses[i]), list(zip(names, e.views)),
                     dict(e.model.named_buffers()))
        problems = _pair_problems("out_sync rank %d vs one device" % i, ref, got, one)
        assert not problems, "rank %d differs from the one-device step:\n  " % i + "\n  ".join(problems)
