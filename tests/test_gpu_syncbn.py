"""Sync-BN (parallel.sync_batchnorm): R shards of one batch, each a model
replica with its own context, driven as virtual ranks on one GPU, must reproduce the reference's
FULL-batch step -- concatenated logits, loss, all 14 gradients and the BatchNorm buffers -- at the
golden tolerances of test_gpu_parity.  The same shards without sync (per-shard BatchNorm) must miss
them, so the test tells the two semantics apart.  Needs an MI355X: -m gpu."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import GOLDEN_CASES, Golden  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import (GRAD_ABS_FLOOR, GRAD_TOL_GOLDEN, close as _close,  # noqa: E402
                         close_rel as _close_rel, compare_grads, model as _model, to_np as _np)

pytestmark = pytest.mark.gpu


def _shards(B, R):
    from explainn_amd.parallel import shard_bounds
    return [shard_bounds(B, R, r) for r in range(R)]


def _ranks(g, R, loss=None):
    from explainn_amd.engine import StepEngine
    engines = []
    for lo, hi in _shards(g.B, R):
        m = _model(g.sd(), g.U, g.k, g.L, g.T).train()
        engines.append(StepEngine(m, hi - lo, loss=loss or g.loss_kind))
    return engines


def _sync_step(g, R, keep=None):
    from explainn_amd.parallel import VirtualRanks
    engines = _ranks(g, R)
    x = torch.from_numpy(g.onehot()).cuda()
    y = torch.from_numpy(g.targets().astype(np.float32)).cuda()
    sh = _shards(g.B, R)
    if keep is None:
        for e in engines:
            e.model.dropout_p = 0.0
        masks = None
    else:
        masks = [torch.from_numpy(keep[lo:hi]).cuda() for lo, hi in sh]
    vr = VirtualRanks(engines)
    out = vr.step([x[lo:hi] for lo, hi in sh], [y[lo:hi] for lo, hi in sh], keep_masks=masks)
    torch.cuda.synchronize()
    logits = torch.cat([l for l, _ in out]).cpu().numpy()
    losses = [float(ls.item()) for _, ls in out]
    return engines, logits, losses


def _floor(g):
    return 1e-7 if g.B <= 2 else GRAD_ABS_FLOOR


def _cases():
    out = []
    for name in GOLDEN_CASES:
        B = int(Golden(name).B)
        out += [(name, R) for R in (2, 3, 4) if R <= B]
    return out


def _check(g, engines, logits, losses, prefix, keep=None):
    _close(logits, g.z[prefix + "/logits"], what="sync logits")
    for ls in losses:
        _close(ls, g.z[prefix + "/loss"], tol=1e-5, what="sync loss")
    _, cache, _ = orc.forward(g.sd(), g.onehot(), training=True, dropout_mask=keep, return_cache=True)
    ref = g.group(prefix + "/grad/")
    for e in engines:
        params = dict(zip([n for n, _ in e.model.named_parameters()], e.views))
        compare_grads([(k, _np(params[k])) for k in ref], ref, GRAD_TOL_GOLDEN, cache, g.U,
                      "sync golden ", abs_floor=_floor(g))
    if prefix == "train0":
        for e in engines:
            bufs = dict(e.model.named_buffers())
            for k, v in g.group("train0/buf/").items():
                if "tracked" in k:
                    assert int(bufs[k].item()) == int(v), k
                else:
                    _close_rel(_np(bufs[k]), v, what="buffer " + k)


@pytest.mark.parametrize("name,R", _cases())
def test_sync_bn_matches_full_batch_golden(name, R):
    g = Golden(name)
    engines, logits, losses = _sync_step(g, R)
    _check(g, engines, logits, losses, "train0")
    # every rank holds the same bits: gradients and BatchNorm buffers
    for e in engines[1:]:
        assert torch.equal(e.flat_grad, engines[0].flat_grad)
        for (k, a), (_, b) in zip(e.model.named_buffers(), engines[0].model.named_buffers()):
            assert torch.equal(a, b), k


@pytest.mark.parametrize("name,R", [c for c in _cases() if c[1] in (2, 3)])
def test_sync_bn_dropout_mask_golden(name, R):
    g = Golden(name)
    keep = g.keep_mask()
    engines, logits, losses = _sync_step(g, R, keep=keep)
    _check(g, engines, logits, losses, "drop", keep=keep)


def test_per_shard_bn_misses_the_full_batch():
    """The same shards through the default (per-shard) step: the logits of at least one fixture
    leave the golden bound that the sync step meets."""
    missed = []
    for name in ("small_u8_k19", "c1_u100_k19_L200"):
        g = Golden(name)
        engines = _ranks(g, 2)
        x = torch.from_numpy(g.onehot()).cuda()
        y = torch.from_numpy(g.targets().astype(np.float32)).cuda()
        parts = []
        for e, (lo, hi) in zip(engines, _shards(g.B, 2)):
            e.model.dropout_p = 0.0
            lg, _ = e.step(x[lo:hi], y[lo:hi], seed=1)
            parts.append(lg.clone())
        torch.cuda.synchronize()
        err = float(np.abs(torch.cat(parts).cpu().numpy() - g.z["train0/logits"]).max())
        missed.append(err > 1e-4)
    assert any(missed)


def test_sync_bn_one_rank_equals_plain_step():
    """One rank: sync and per-shard BatchNorm are the same function (to rounding)."""
    from explainn_amd.engine import StepEngine
    from explainn_amd.parallel import ProcessGroupReducer, sync_batchnorm
    g = Golden("c1_u100_k19_L200")
    x = torch.from_numpy(g.onehot()).cuda()
    y = torch.from_numpy(g.targets().astype(np.float32)).cuda()
    res = []
    for sync in (False, True):
        m = _model(g.sd(), g.U, g.k, g.L, g.T).train()
        m.dropout_p = 0.0
        if sync:
            sync_batchnorm(m, ProcessGroupReducer())
        e = StepEngine(m, g.B, loss=g.loss_kind)
        lg, ls = e.step(x, y, seed=3)
        torch.cuda.synchronize()
        res.append((_np(lg), float(ls.item()), _np(e.flat_grad)))
    _close(res[1][0], res[0][0], tol=1e-5, what="logits")
    assert abs(res[1][1] - res[0][1]) < 1e-6
    ref = res[0][2]
    assert np.abs(res[1][2] - ref).max() <= 1e-4 * np.abs(ref).max()


def test_sync_bn_errors():
    from explainn_amd import _lib
    from explainn_amd.engine import StepEngine
    from explainn_amd.parallel import ProcessGroupReducer, sync_batchnorm
    g = Golden("tiny_u1_k5")
    m = _model(g.sd(), g.U, g.k, g.L, g.T).train()
    sync_batchnorm(m, ProcessGroupReducer())
    x = torch.from_numpy(g.onehot()).cuda()
    # x.grad is out of scope in sync mode: refused, not computed with per-shard statistics
    with pytest.raises(NotImplementedError):
        m(x.clone().requires_grad_())
    # VirtualRanks drives its replicas itself; it is not a per-rank reducer
    from explainn_amd.parallel import VirtualRanks
    with pytest.raises(TypeError):
        sync_batchnorm(m, VirtualRanks([]))
    e = StepEngine(m, g.B)
    lib, h = e.ctx.lib, e.ctx.handle
    # out of order: phase 3 without phases 1 and 2
    a = _lib.SyncArgs(B_local=g.B, B_global=g.B, params=ctypes.pointer(e.ps),
                      grads=ctypes.pointer(e.gs))
    buf = torch.zeros(1 << 16, device="cuda", dtype=torch.float64)
    assert lib.explainn_sync_phase(h, 3, ctypes.byref(a), buf.data_ptr(), buf.data_ptr(),
                                   None) == _lib.E_STATE
    # one sequence in all is no batch statistic
    a.B_local, a.B_global = 1, 1
    assert lib.explainn_sync_phase(h, 1, ctypes.byref(a), None, buf.data_ptr(), None) == _lib.E_ARG
