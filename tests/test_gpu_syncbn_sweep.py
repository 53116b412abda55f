"""Sync-BN at its dispatch edges against the fp64 oracle: every case of tests/syncbn_dispatch_model.py
(shards of 1 / 16 / 64 sequences and their neighbours, eight ranks, contexts that differ or are mostly
empty, the large-n kernels on tiny shards, both combiners, MSE, base codes, a rank of N, frozen filters,
a recorded keep mask, the caller's dlogits) runs one step on virtual ranks and must reproduce the step
of the concatenated batch.  tests/test_syncbn_dispatch_coverage.py checks on CPU that the cases reach
every form.

Per case: logits at TOL, the loss at 1e-5 on every rank, the 14 gradients of every rank with check_grads'
bounds, every BatchNorm buffer of every rank at GRAD_TOL_ORACLE, identical bits on all ranks, and rank 0's
eval-mode logits from the updated buffers (a buffer that is wrong but equal on all ranks).  The fp32
batches go to the step by pointer (validate_input off: pack_tables_kernel, the steady state of a training
run; a fresh model's first steps stage the batch, as the golden tests do), base codes are staged.

The dlogits cases drive the autograd path's phases (1-4, the caller's dlogits, 5-8) on all ranks from
one thread in lockstep, as VirtualRanks.step does for the engine path.  -m gpu."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import parity_util  # noqa: E402
import syncbn_dispatch_model as sm  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import (GRAD_TOL_ORACLE, TOL, close, close_rel, compare_grads, model, oracle_step,  # noqa: E402
                         reference_fp32_error, to_np)
from test_gpu_syncbn import _floor  # noqa: E402

pytestmark = pytest.mark.gpu


class _Batch:
    """What _floor reads of a fixture."""

    def __init__(self, B):
        self.B = B


def _reference(c, d):
    """(logits, loss, gradients, buffers) of the step on the concatenated batch; the gradients are
    registered with parity_util's knife-edge cache and reference error, as oracle_step leaves them."""
    kind = "binary" if c.loss == "bce" else "mse"
    if c.backward != "dlogits_free":
        return oracle_step(d["sd"], d["x"], d["y"], freeze=c.freeze, keep=d["keep"], kind=kind)
    # a free dlogits matrix D: the knife-edge cache as _oracle of the dispatch sweep builds it, and the
    # gradients of D through it.  The reference's own fp32 error on this case comes from the same stock
    # PyTorch step with the MSE targets whose loss gradient is D (2 (logits - y) / (B T) = D)
    sd, x, D = d["sd"], d["x"], d["D"]
    ref_logits, _, nb = orc.forward(sd, x, training=True, return_cache=True)
    _, cache, _ = orc.forward(sd, x, training=True, return_cache=True, dtype=np.float64)
    grads = orc.backward(cache, D.astype(np.float64))
    y = (ref_logits - D * (D.size / 2.0)).astype(np.float32)
    ref_err = reference_fp32_error(sd, x, y, grads, "mse", cache=cache)
    parity_util._ORACLE_CACHES[id(grads)] = (cache, c.U, ref_err, grads)
    return ref_logits, None, grads, nb


def _check_grads(c, engine, grads, what):
    cache, U, ref_err, _ = parity_util._ORACLE_CACHES[id(grads)]
    names = [n for n, _ in engine.model.named_parameters()]
    compare_grads([(n, to_np(v)) for n, v in zip(names, engine.views)], grads, GRAD_TOL_ORACLE, cache, U, what,
                  ref_err, abs_floor=_floor(_Batch(sum(c.shards))))


def _engines(c, d):
    from explainn_amd.engine import StepEngine
    engines = []
    for b, mb in sm.rank_batches(c.shards, c.max_batches):
        m = model(d["sd"], c.U, c.k, c.L, c.T).train()
        m.validate_input = False
        if not c.mask:
            m.dropout_p = 0.0
        engines.append(StepEngine(m, mb, loss="binary" if c.loss == "bce" else "mse"))
    return engines


def _shards(c, d):
    """Per-rank device inputs: fp32 one-hot rows or BaseCodes, and targets."""
    from explainn_amd.architectures import BaseCodes
    xs, ys = [], []
    for lo, hi in sm.bounds(c):
        if c.input == "onehot":
            xs.append(torch.from_numpy(d["x"][lo:hi]).cuda())
        else:
            xs.append(BaseCodes(torch.from_numpy(d["codes"][lo:hi]).cuda(), c.input == "codes_rc"))
        ys.append(torch.from_numpy(d["y"][lo:hi]).cuda())
    return xs, ys


def _lockstep(gens):
    """Advance every rank's phases by one exchange at a time, summing each exchange in rank order."""
    while True:
        bufs = [next(g, None) for g in gens]
        if all(b is None for b in bufs):
            return
        assert all(b is not None for b in bufs), "ranks out of step"
        tot = bufs[0].clone()
        for b in bufs[1:]:
            tot += b
        for b in bufs:
            b.copy_(tot)


def _dlogits_step(c, d, engines, xs, ys):
    """The autograd path on every rank: phases 1-4, the caller's dlogits, phases 5-8."""
    from explainn_amd import _lib
    from explainn_amd.engine import sync_buffers, sync_run
    Bg = sum(c.shards)
    args, bufs = [], []
    for e, x in zip(engines, xs):
        xp, _ = e._front(x)
        bufs.append(sync_buffers(e.ctx, e.dev))
        args.append(_lib.SyncArgs(x=xp, targets=None, dlogits=None, dl_scale=1.0, B_local=int(x.shape[0]),
                                  B_global=Bg, params=ctypes.pointer(e.ps), grads=ctypes.pointer(e.gs),
                                  loss_kind=e.loss_kind, dropout_p=0.0, seed=0, keep_mask=None,
                                  freeze_top_n_filters=0, logits=e.logits.data_ptr(), loss_out=None))
    _lockstep([sync_run(e.ctx, a, b, range(1, 5)) for e, a, b in zip(engines, args, bufs)])
    keep, losses = [], []
    for e, a, y, (lo, hi) in zip(engines, args, ys, sm.bounds(c)):
        if c.backward == "dlogits_shard_mean":
            lg = e.logits[:hi - lo].detach().clone().requires_grad_()
            loss = torch.nn.functional.binary_cross_entropy_with_logits(lg, y)
            dl, = torch.autograd.grad(loss, lg)
            losses.append(float(loss.item()))
            a.dl_scale = float(hi - lo) / float(Bg)
        else:
            dl = torch.from_numpy(d["D"][lo:hi]).cuda()
            a.dl_scale = 1.0
        dl = dl.to(torch.float32).contiguous()
        keep.append(dl)
        a.dlogits = dl.data_ptr()
    _lockstep([sync_run(e.ctx, a, b, range(5, 9)) for e, a, b in zip(engines, args, bufs)])
    for e in engines:
        e.model._touched()
        e.model._rt.token += 1
    torch.cuda.synchronize()
    del keep
    logits = torch.cat([e.logits[:b] for e, b in zip(engines, c.shards)])
    return logits, losses


@pytest.mark.parametrize("case", sm.CASES, ids=[c.id for c in sm.CASES])
def test_sync_sweep_vs_oracle(case):
    from explainn_amd.parallel import VirtualRanks
    c = case
    d = sm.inputs(c)
    ref_logits, ref_loss, grads, nb = _reference(c, d)
    engines = _engines(c, d)
    xs, ys = _shards(c, d)
    label = "sync sweep %s" % c.group
    if c.backward == "targets":
        masks = None
        if c.mask:
            masks = [torch.from_numpy(d["keep"][lo:hi]).cuda() for lo, hi in sm.bounds(c)]
        out = VirtualRanks(engines).step(xs, ys, keep_masks=masks, freeze_top_n_filters=c.freeze)
        torch.cuda.synchronize()
        logits = torch.cat([lg for lg, _ in out])
        for _, ls in out:
            close(float(ls.item()), ref_loss, tol=1e-5, what=label + " loss")
    else:
        logits, losses = _dlogits_step(c, d, engines, xs, ys)
        if losses:
            # the ranks' own shard-mean losses, weighted by their shares, are the global mean
            mean = sum(ls * b for ls, b in zip(losses, c.shards)) / sum(c.shards)
            close(mean, ref_loss, tol=1e-5, what=label + " loss")
    close(to_np(logits), ref_logits, what=label + " logits")
    for e in engines:
        _check_grads(c, e, grads, label + " ")
        bufs = dict(e.model.named_buffers())
        for key, v in nb.items():
            if "tracked" in key:
                assert int(bufs[key].item()) == int(v), key
            else:
                close_rel(to_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what=label + " " + key)
    for e in engines[1:]:
        assert torch.equal(e.flat_grad, engines[0].flat_grad)
        for (key, a), (_, b) in zip(e.model.named_buffers(), engines[0].model.named_buffers()):
            assert torch.equal(a, b), key
    # eval mode from the buffers the step left, on the whole batch
    sd2 = dict(d["sd"])
    sd2.update(nb)
    m = engines[0].model.eval()
    with torch.no_grad():
        got = m(torch.from_numpy(d["x"]).cuda())
    close(to_np(got), orc.forward(sd2, d["x"]), tol=TOL, what=label + " eval logits")


def test_sync_dropout_seeds_reach_phase_3():
    """Two ranks holding the same rows, built-in dropout at 0.3: equal explicit seeds give bit-identical
    logits rows on both ranks, the default seeds (rank_seed: distinct per rank) different ones."""
    from explainn_amd.engine import StepEngine
    from explainn_amd.parallel import VirtualRanks
    U, k, L, T, B = 5, 19, 200, 2, 33
    sd = orc.random_state_dict(U, k, L, T, seed=21)
    x = torch.from_numpy(orc.random_onehot(B, L, seed=22, n_frac=0.01)).cuda()
    y = torch.from_numpy((np.random.default_rng(23).random((B, T)) > 0.5).astype(np.float32)).cuda()
    engines = []
    for _ in range(2):
        m = model(sd, U, k, L, T).train()
        m.dropout_p = 0.3
        engines.append(StepEngine(m, B))
    vr = VirtualRanks(engines)
    out = vr.step([x, x], [y, y], seeds=[77, 77])
    torch.cuda.synchronize()
    assert torch.isfinite(out[0][0]).all()
    assert torch.equal(out[0][0], out[1][0]), "equal seeds, equal rows: the ranks' logits differ"
    out = vr.step([x, x], [y, y])
    torch.cuda.synchronize()
    assert torch.isfinite(out[0][0]).all()
    assert not torch.equal(out[0][0], out[1][0]), "the default seeds gave both ranks the same dropout mask"
