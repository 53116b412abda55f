#!/usr/bin/env python3
"""Times Integrated Gradients on one GPU, from host-resident base codes to a host-resident (N,4,L)
result, zero baseline, S midpoint nodes:
  (a) interpret.integrated_gradients -- one device pass along the path (csrc/pathgrad.hip);
  (b) the loop it replaces -- S soft batches a_s * x through interpret.input_gradients (the dense
      kernels, an eval_keep forward, an input-gradient launch and a copy back per node) and the
      host multiply-accumulate.
Shapes: 300 units / B 1024 and 100 units / B 100, both k 19, L 200, T 1, S 32.  The legs alternate in
one process after a warm-up of both; times are wall clock (the legs end in a device-to-host copy).
One JSON line per shape: the median, minimum and maximum of each leg, their ratio, and the largest
difference between the two results relative to the largest attribution.

  ig_probe.py [--reps R] [--out FILE]           time both legs, write FILE (a JSON list)
  ig_probe.py --only-new [--reps R]             run leg (a) alone: the command to put behind
                                                `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`
  ig_probe.py --kernel-stats DIR --out FILE     add the per-launch times of the pg_* kernels found in
                                                DIR's *kernel_stats.csv to FILE"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("U300-B1024", 300, 1024), ("U100-B100", 100, 100)]
K, L, T, STEPS = 19, 200, 1, 32


def build(U):
    import torch
    from explainn_amd import ExplaiNN
    from oracle import explainn_oracle as orc
    sd = orc.random_state_dict(U, K, L, T, seed=0)
    m = ExplaiNN(U, K, L, T)
    m.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    return m.cuda().eval()


def loop_route(m, x):
    from explainn_amd import interpret
    acc = np.zeros(x.shape, dtype=np.float64)
    for s in range(STEPS):
        acc += interpret.input_gradients(m, (np.float32((s + 0.5) / STEPS) * x), batch_size=len(x))
    return (acc * x / STEPS).astype(np.float32)


def run(name, U, B, reps, only_new):
    import torch
    from explainn_amd import interpret
    from explainn_amd.sequence import codes_to_one_hot
    m = build(U)
    codes = np.random.default_rng(1).integers(0, 4, size=(B, L)).astype(np.uint8)
    x = np.ascontiguousarray(codes_to_one_hot(codes), dtype=np.float32).reshape(B, 4, L)
    new = lambda: interpret.integrated_gradients(m, codes, "zero", steps=STEPS, batch_size=B)
    got = new()
    if only_new:
        for _ in range(reps):
            new()
        torch.cuda.synchronize()
        return None
    ref = loop_route(m, x)
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); new(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); loop_route(m, x); tb.append(time.perf_counter() - t0)
    st = lambda t: {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}
    rec = {"shape": name, "U": U, "k": K, "L": L, "T": T, "B": B, "steps": STEPS, "reps": reps,
           "integrated_gradients": st(ta), "input_gradient_loop": st(tb),
           "loop_over_new": float(np.median(tb) / np.median(ta)),
           "max_rel_diff": float(np.abs(got - ref).max() / np.abs(ref).max())}
    print(json.dumps(rec), flush=True)
    return rec


def kernel_stats(directory, out):
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Name"].replace("void ", "").split("(")[0]
            if name.startswith("pg_"):
                rows[name] = {"calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                              "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    if not rows:
        raise SystemExit("no pg_* kernels in %s/**/*kernel_stats.csv" % directory)
    doc = json.load(open(out)) if os.path.exists(out) else []
    doc.append({"kernel_times": rows, "note": "rocprofv3 --kernel-trace --stats over `ig_probe.py --only-new`: "
                "launches of both shapes, in shape order, pooled per kernel name"})
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    recs = [run(n, U, B, a.reps, a.only_new) for n, U, B in SHAPES if n in a.shapes.split(",")]
    if a.out and not a.only_new:
        json.dump(recs, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
