"""Sync-BN beyond the golden fixtures: larger shapes against the fp64 oracle (several batch chunks
per rank, the big-n kernels), the autograd path, a short Adam run, the Trainer keyword and a real
two-process gloo group.  Needs an MI355X: -m gpu."""
import os
import socket
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import Golden  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import (GRAD_TOL_ORACLE, NEAR_NULL, ZERO_GRAD, check_grads, close as _close,  # noqa: E402
                         close_rel as _close_rel, model as _model, oracle_step, to_np as _np)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _virtual_step(sd, U, k, L, T, x, y, bounds):
    from explainn_amd.engine import StepEngine
    from explainn_amd.parallel import VirtualRanks
    engines = []
    for lo, hi in bounds:
        m = _model(sd, U, k, L, T).train()
        m.dropout_p = 0.0
        engines.append(StepEngine(m, hi - lo))
    out = VirtualRanks(engines).step([x[lo:hi] for lo, hi in bounds], [y[lo:hi] for lo, hi in bounds])
    torch.cuda.synchronize()
    return engines, torch.cat([lg for lg, _ in out]), [float(ls.item()) for _, ls in out]


def _bounds(B, R):
    from explainn_amd.parallel import shard_bounds
    return [shard_bounds(B, R, r) for r in range(R)]


# (U, k, L, T, B, R): 8 ranks of 128 (one batch chunk each); 3 uneven ranks of 342/341/341
# (qmom: 3 chunks, passA: 2 chunks, several filter-gradient partials and S1/S2 tiles per rank);
# L = 1000 (n = 140: qmom_big, mid_big, passB<140>) as 3 uneven ranks
SHAPES = [(24, 19, 200, 1, 1024, 8), (24, 19, 200, 2, 1024, 3), (6, 19, 1000, 2, 200, 3)]


@pytest.mark.parametrize("U,k,L,T,B,R", SHAPES)
def test_sync_bn_shapes_vs_oracle(U, k, L, T, B, R):
    sd = orc.random_state_dict(U, k, L, T, seed=11)
    xn = orc.random_onehot(B, L, seed=12, n_frac=0.01)
    yn = (np.random.default_rng(13).random((B, T)) > 0.5).astype(np.float32)
    ref_logits, ref_loss, grads, nb = oracle_step(sd, xn, yn)
    sdt = {key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()}
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    engines, logits, losses = _virtual_step(sdt, U, k, L, T, x, y, _bounds(B, R))
    _close(_np(logits), ref_logits, what="sync logits")
    for ls in losses:
        assert abs(ls - ref_loss) < 1e-5
    for e in engines:
        names = [n for n, _ in e.model.named_parameters()]
        check_grads(list(zip(names, e.views)), grads, "sync R=%d " % R)
        bufs = dict(e.model.named_buffers())
        for key, v in nb.items():
            if "tracked" in key:
                assert int(bufs[key].item()) == int(v), key
            else:
                _close_rel(_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what="sync R=%d %s" % (R, key))
    assert all(torch.equal(e.flat_grad, engines[0].flat_grad) for e in engines[1:])


def test_autograd_path_one_rank_equals_plain():
    """model(x) + loss.backward() with sync on (one-rank reducer): the same function as without."""
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
        lg = m(x)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(lg, y)
        loss.backward()
        torch.cuda.synchronize()
        res.append((_np(lg), [_np(p.grad) for p in m.parameters()],
                    [_np(b) for b in m.buffers()]))
    _close(res[1][0], res[0][0], tol=1e-5, what="logits")
    _close(res[1][0], g.z["train0/logits"], what="golden logits")
    for a, b in zip(res[1][1], res[0][1]):
        assert np.abs(a - b).max() <= 1e-4 * max(np.abs(b).max(), 1e-6)
    for a, b in zip(res[1][2], res[0][2]):
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-5 * max(np.abs(b).max(), 1.0)


def test_adam_two_virtual_ranks_follow_one_device():
    """5 StepEngine + Adam steps on 2 virtual ranks against the same 5 steps on one device over the
    whole batch.  Bound: for every tensor, the difference of the trajectories is at most 5 % of the
    distance the one-device run moved it.  The pre-BatchNorm biases and BatchNorm1's bias
    (ZERO_GRAD, NEAR_NULL: true gradient zero or ~0) are excluded from that: Adam normalises their
    rounding noise to full-size steps on either side, so they are bounded by 5 steps x 2 lr."""
    from explainn_amd.engine import StepEngine
    from explainn_amd.parallel import VirtualRanks
    g = Golden("c1_u100_k19_L200")
    x = torch.from_numpy(g.onehot()).cuda()
    y = torch.from_numpy(g.targets().astype(np.float32)).cuda()
    lr, steps = 0.003, 5
    one = _model(g.sd(), g.U, g.k, g.L, g.T).train()
    one.dropout_p = 0.0
    e1 = StepEngine(one, g.B)
    opt1 = torch.optim.Adam(one.parameters(), lr=lr)
    bounds = _bounds(g.B, 2)
    reps = []
    for lo, hi in bounds:
        m = _model(g.sd(), g.U, g.k, g.L, g.T).train()
        m.dropout_p = 0.0
        reps.append(StepEngine(m, hi - lo))
    opts = [torch.optim.Adam(e.model.parameters(), lr=lr) for e in reps]
    vr = VirtualRanks(reps)
    init = [p.detach().clone() for p in one.parameters()]
    for _ in range(steps):
        e1.step(x, y, seed=1)
        e1.attach_grads()
        opt1.step()
        vr.step([x[lo:hi] for lo, hi in bounds], [y[lo:hi] for lo, hi in bounds])
        for e, o in zip(reps, opts):
            e.attach_grads()
            o.step()
    torch.cuda.synchronize()
    for r in reps[1:]:
        for a, b in zip(r.model.parameters(), reps[0].model.parameters()):
            assert torch.equal(a, b)
    loose = set(ZERO_GRAD) | {NEAR_NULL}
    for (name, p), q, p0 in zip(one.named_parameters(), reps[0].model.parameters(), init):
        d = float((q - p).abs().max())
        if name in loose:
            assert d <= steps * 2 * lr, name
        else:
            moved = float((p - p0).abs().max())
            assert d <= 0.05 * moved + 1e-7, (name, d, moved)


@pytest.mark.parametrize("fused", [True, False])
def test_trainer_keyword_one_rank(tmp_path, fused):
    """A short Trainer run with sync_batchnorm=True (one rank: the same function) writes the same
    training losses as the run without it."""
    from torch.utils.data import DataLoader, TensorDataset
    from explainn_amd import ExplaiNN, get_loss, get_metrics, get_optimizer
    from explainn_amd.selene import Trainer
    from test_harness import _trainer_fixture
    z, (U, k, L, T, B, N), x, y, sd = _trainer_fixture()
    runs = []
    for sync in (False, True):
        model = ExplaiNN(U, k, L, T)
        model.load_state_dict(sd)
        model.dropout_p = 0.0
        loaders = {"train": DataLoader(TensorDataset(x[:N], y[:N]), B, shuffle=False),
                   "validation": DataLoader(TensorDataset(x[N:], y[N:]), B, shuffle=False)}
        crit = get_loss("binary") if fused else torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(1))
        spe = N // B
        out = tmp_path / ("sync" if sync else "plain")
        tr = Trainer(model, loaders, crit, get_metrics("binary"), get_optimizer(model.parameters(), 0.003),
                     max_steps=spe * 2, patience=spe * 10, report_stats_every_n_steps=spe,
                     output_dir=str(out), cpu_n_threads=1, use_cuda=True, logging_verbosity=0,
                     sync_batchnorm=sync)
        assert tr._fused_step_available() == fused
        tr.train_and_validate()
        runs.append(np.array([float(v) for v in open(out / "train.txt").read().split()[1:]]))
    assert np.abs(runs[1] - runs[0]).max() < 1e-5
    assert np.abs(runs[1] - z["train_txt"][:len(runs[1])]).max() < 1e-4


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _gloo_worker(r, ws, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import torch.distributed as dist
        from conftest import Golden as G
        from parity_util import model as mk
        from explainn_amd.engine import StepEngine
        from explainn_amd.parallel import ProcessGroupReducer, shard_batch, sync_batchnorm
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=r, world_size=ws)
        g = G("c1_u100_k19_L200")
        x = torch.from_numpy(g.onehot()).cuda()
        y = torch.from_numpy(g.targets().astype(np.float32)).cuda()
        xs, ys = shard_batch(x, y)
        out = {}
        # fused step
        m = mk(g.sd(), g.U, g.k, g.L, g.T).train()
        m.dropout_p = 0.0
        sync_batchnorm(m, ProcessGroupReducer())
        e = StepEngine(m, xs.shape[0])
        lg, loss = e.step(xs, ys, seed=5)
        out["fused"] = (lg.cpu().numpy(), float(loss.item()), e.flat_grad.cpu().numpy(),
                        [b.cpu().numpy() for b in m.buffers()])
        # autograd path (mean over the local rows; the backward rescales to the global mean)
        m2 = mk(g.sd(), g.U, g.k, g.L, g.T).train()
        m2.dropout_p = 0.0
        sync_batchnorm(m2, ProcessGroupReducer())
        lg2 = m2(xs)
        torch.nn.functional.binary_cross_entropy_with_logits(lg2, ys).backward()
        out["autograd"] = (lg2.detach().cpu().numpy(), None,
                           torch.cat([p.grad.reshape(-1) for p in m2.parameters()]).cpu().numpy(),
                           [b.cpu().numpy() for b in m2.buffers()])
        q.put((r, out))
        dist.barrier(); dist.destroy_process_group()
    except BaseException as exc:                    # report, do not hang the parent
        q.put((r, repr(exc)))
        raise


def test_process_group_gloo_world2_reproduces_full_batch():
    """Two spawned processes on one GPU, gloo (host-staged exchanges): both ranks reproduce the
    full-batch step of the c1 fixture, through StepEngine and through autograd."""
    from parity_util import GRAD_TOL_GOLDEN, compare_grads
    import torch.multiprocessing as mp
    g = Golden("c1_u100_k19_L200")
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    res = dict(q.get(timeout=240) for _ in range(2))
    for p in procs: p.join(timeout=60)
    for r in range(2):
        assert not isinstance(res[r], str), res[r]
    assert all(p.exitcode == 0 for p in procs)
    m = _model(g.sd(), g.U, g.k, g.L, g.T)
    names = [(n, p.numel(), tuple(p.shape)) for n, p in m.named_parameters()]
    bufnames = [n for n, _ in m.named_buffers()]
    _, cache, _ = orc.forward(g.sd(), g.onehot(), training=True, return_cache=True)
    ref = g.group("train0/grad/")
    for path in ("fused", "autograd"):
        lg = np.concatenate([res[0][path][0], res[1][path][0]])
        _close(lg, g.z["train0/logits"], what=path + " logits")
        if path == "fused":
            for r in range(2):
                _close(res[r][path][1], g.z["train0/loss"], tol=1e-5, what="loss")
        assert np.array_equal(res[0][path][2], res[1][path][2]), "identical gradients on both ranks"
        flat, off, named = res[0][path][2], 0, []
        for n, cnt, shp in names:
            named.append((n, flat[off:off + cnt].reshape(shp)))
            off += cnt
        compare_grads([(n, v) for n, v in named if n in ref], ref, GRAD_TOL_GOLDEN, cache, g.U,
                      "gloo %s " % path)
        want = g.group("train0/buf/")
        for n, b in zip(bufnames, res[0][path][3]):
            if n in want and "tracked" not in n:
                scale = max(float(np.abs(want[n]).max()), 1e-30)
                assert np.abs(b - want[n]).max() <= 2e-5 * scale, n
