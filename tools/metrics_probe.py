#!/usr/bin/env python3
"""Times the validation metrics on one GPU and its host: (a) the host path -- device tensors ->
.cpu().numpy() -> the architectures.get_metrics callables (scikit-learn / scipy) on the flattened
arrays, what selene.Trainer.validate does by default; (b) explainn_amd.metrics on the device, the
final read of the two scalars included.  Flattened sizes 1e4, 1e5, 1e6, 5e6 (global mode) and
(100000, 50) per task (host: the same callables column by column).  The legs alternate in one process
after a warm-up; times are wall clock, each call ends with its values on the host.  One JSON line per
(kind, size): median and spread (max - min over the timed calls) of both legs, their ratio, and at
the end the smallest size from which the device leg wins.

usage: metrics_probe.py [--reps R]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explainn_amd import get_metrics, metrics  # noqa: E402

SIZES = [(10 ** 4, 1, False), (10 ** 5, 1, False), (10 ** 6, 1, False), (5 * 10 ** 6, 1, False),
         (100000, 50, True)]


def host_leg(fns, y, s, per_task):
    yn, sn = y.cpu().numpy(), s.cpu().numpy()
    if per_task:
        return [[float(np.asarray(f(yn[:, t], sn[:, t])).reshape(-1)[0]) for t in range(yn.shape[1])]
                for f in fns.values()]
    return [float(np.asarray(f(yn.flatten(), sn.flatten())).reshape(-1)[0]) for f in fns.values()]


def device_leg(kind, y, s, per_task):
    return metrics.read(*metrics._run(kind, y, s, per_task))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(max(out) - min(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    rng = np.random.default_rng(0)
    for kind in ("binary", "linear"):
        fns = get_metrics(kind)
        crossover = None
        for n, t, per_task in SIZES:
            yv = (rng.random((n, t)) < 0.3) if kind == "binary" else rng.normal(size=(n, t))
            s = torch.from_numpy((rng.normal(size=(n, t)) + yv).astype(np.float32)).cuda()
            y = torch.from_numpy(yv.astype(np.float32)).cuda()
            reps = args.reps
            a = host_leg(fns, y, s, per_task)
            b = device_leg(kind, y, s, per_task)
            device_leg(kind, y, s, per_task)
            diff = float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())
            ha, da = [], []
            for _ in range(2):                       # alternate the legs
                ha.append(timed(lambda: host_leg(fns, y, s, per_task), reps // 2))
                da.append(timed(lambda: device_leg(kind, y, s, per_task), reps // 2))
            h_ms, d_ms = float(np.mean([v[0] for v in ha])), float(np.mean([v[0] for v in da]))
            h_sp, d_sp = max(v[1] for v in ha), max(v[1] for v in da)
            faster = d_ms + d_sp + h_sp < h_ms
            if not per_task:
                crossover = (n if crossover is None else crossover) if faster else None
            print(json.dumps({"kind": kind, "N": n, "T": t, "mode": "per_task" if per_task else "global",
                              "timed_calls_per_leg": 2 * (reps // 2), "host_ms": h_ms, "host_spread_ms": h_sp,
                              "device_ms": d_ms, "device_spread_ms": d_sp, "host_over_device": h_ms / d_ms,
                              "device_faster_beyond_spread": faster, "max_abs_diff": diff}), flush=True)
        print(json.dumps({"kind": kind, "device_wins_from_flattened_size": crossover}), flush=True)


if __name__ == "__main__":
    main()
