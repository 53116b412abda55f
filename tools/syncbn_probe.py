"""Sync-BN cost at C2 (300 units, k 19, L 200, T 1, batch 1024).

Reports, on one GPU:
  plain_ms        the default (per-shard BatchNorm) StepEngine step on the whole batch
  sync1_ms        the sync-BN step in a one-rank group (the six exchanges are identities)
  virtual8_ms     8 virtual ranks of 128 sequences (VirtualRanks.step: 8 x 8 phases + 6 sums)
  phase_us        the device time of each sync phase of the one-rank step (HIP events)
  exchange_bytes  the size of each phase's exchange

usage: python tools/syncbn_probe.py [--steps K] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import ctypes as C
    import torch
    from explainn_amd import ExplaiNN, _lib
    from explainn_amd.engine import StepEngine, sync_run
    from explainn_amd.parallel import ProcessGroupReducer, VirtualRanks, shard_bounds, sync_batchnorm

    U, k, L, T, B, R = 300, 19, 200, 1, 1024, 8
    torch.manual_seed(0)
    x = torch.zeros(B, 4, L, device="cuda")
    x.scatter_(1, torch.randint(0, 4, (B, 1, L), device="cuda"), 1.0)
    y = (torch.rand(B, T, device="cuda") > 0.5).float()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    def fresh():
        torch.manual_seed(1)
        return ExplaiNN(U, k, L, T).cuda().train()

    plain = StepEngine(fresh(), B)
    res = {"workload": "C2: U=300, k=19, L=200, T=1, batch 1024, dropout 0.3",
           "plain_ms": timed(lambda: plain.step(x, y))}

    m1 = sync_batchnorm(fresh(), ProcessGroupReducer())
    e1 = StepEngine(m1, B)
    res["sync1_ms"] = timed(lambda: e1.step(x, y, global_batch=B))

    engines = [StepEngine(fresh(), hi - lo) for lo, hi in (shard_bounds(B, R, r) for r in range(R))]
    vr = VirtualRanks(engines)
    bounds = [shard_bounds(B, R, r) for r in range(R)]
    xs, ys = [x[lo:hi] for lo, hi in bounds], [y[lo:hi] for lo, hi in bounds]
    res["virtual8_ms"] = timed(lambda: vr.step(xs, ys))

    # device time per phase of the one-rank sync step: events around each explainn_sync_phase
    lib, h = e1.ctx.lib, e1.ctx.handle
    res["exchange_bytes"] = {str(i): 8 * int(lib.explainn_sync_exchange_elems(h, i))
                             for i in range(1, _lib.SYNC_PHASES + 1)}
    acc = [0.0] * _lib.SYNC_PHASES
    n = 10
    for _ in range(n):
        xp, _ = m1._stage(e1.ctx, x)
        args = _lib.SyncArgs(x=xp, targets=y.data_ptr(), dl_scale=1.0, B_local=B, B_global=B,
                             params=C.pointer(e1.ps), grads=C.pointer(e1.gs), loss_kind=e1.loss_kind,
                             dropout_p=float(m1.dropout_p), seed=7, logits=e1.logits.data_ptr(),
                             loss_out=e1.loss.data_ptr())
        for ph in range(1, _lib.SYNC_PHASES + 1):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _x in sync_run(e1.ctx, args, e1._xbufs, [ph]):
                pass
            ev1.record()
            torch.cuda.synchronize()
            acc[ph - 1] += ev0.elapsed_time(ev1) * 1e3 / n
        # (phases run one at a time here: sync_run reads the exchange of the last exchanging phase,
        # which the previous iteration left in e1._xbufs)
    res["phase_us"] = {str(i + 1): round(v, 2) for i, v in enumerate(acc)}
    res["steps"], res["warmup"] = a.steps, a.warmup
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
