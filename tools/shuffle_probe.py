#!/usr/bin/env python3
"""Times dinucleotide-preserving shuffles, host against device, on one GPU.  L 200, R 10 shuffles per
sequence, N = 10^3 and 10^4 random sequences held on the host as base codes:
  (a) sequence.dinucleotide_shuffle on the host plus the copy of its (N,R,L) result to the device;
  (b) the copy of the codes to the device plus sequence.dinucleotide_shuffle_device (csrc/shuffle.hip);
      the kernel alone is timed with device events as well;
  (c) what `python -m explainn_amd.attribution` does after reading its input, end to end to a host-resident
      (N,4,L) result, 100 units, k 19, T 1, steps 32, batches of 1024: --baseline shuffle (host shuffles
      handed to interpret.integrated_gradients) against --baseline device-shuffle.
The legs alternate in one process after a warm-up of all of them at a small N; times are wall clock around
work that ends in a device synchronise or a device-to-host copy.  One JSON line per N: median, minimum and
maximum of every leg and the host/device ratios of the medians.

  shuffle_probe.py [--reps R] [--sizes 1000,10000] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

U, K, L, T, STEPS, R, BATCH = 100, 19, 200, 1, 32, 10, 1024


def build():
    import torch
    from explainn_amd import ExplaiNN
    from oracle import explainn_oracle as orc
    sd = orc.random_state_dict(U, K, L, T, seed=0)
    m = ExplaiNN(U, K, L, T)
    m.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    return m.cuda().eval()


def legs(m, codes):
    import torch
    from explainn_amd import interpret
    from explainn_amd.sequence import dinucleotide_shuffle, dinucleotide_shuffle_device

    def host():
        out = torch.from_numpy(dinucleotide_shuffle(codes, n=R, seed=0)).cuda()
        torch.cuda.synchronize()
        return out

    def device():
        out = dinucleotide_shuffle_device(torch.from_numpy(codes).cuda(), n=R, seed=0)
        torch.cuda.synchronize()
        return out

    def ig_host():
        return interpret.integrated_gradients(m, codes, dinucleotide_shuffle(codes, n=R, seed=0), steps=STEPS,
                                              batch_size=BATCH, return_delta=True)

    def ig_device():
        return interpret.integrated_gradients(m, codes, "shuffle", n_shuffles=R, seed=0, steps=STEPS,
                                              batch_size=BATCH, return_delta=True)

    return {"host_shuffle_and_copy": host, "device_shuffle": device, "attribution_shuffle": ig_host,
            "attribution_device_shuffle": ig_device}


def kernel_ms(codes, reps):
    import torch
    from explainn_amd.sequence import dinucleotide_shuffle_device
    dev = torch.from_numpy(codes).cuda()
    times = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dinucleotide_shuffle_device(dev, n=R, seed=0)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times[1:]


def stats(t):
    return {"median_ms": float(np.median(t)) * 1e3, "min_ms": min(t) * 1e3, "max_ms": max(t) * 1e3}


def run(m, N, reps):
    codes = np.random.default_rng(N).integers(0, 4, size=(N, L)).astype(np.uint8)
    fn = legs(m, codes)
    times = {name: [] for name in fn}
    for _ in range(reps):
        for name, f in fn.items():
            t0 = time.perf_counter()
            f()
            times[name].append(time.perf_counter() - t0)
    med = {name: float(np.median(t)) for name, t in times.items()}
    km = kernel_ms(codes, max(reps, 5))
    rec = {"N": N, "L": L, "R": R, "U": U, "k": K, "T": T, "steps": STEPS, "batch": BATCH, "reps": reps}
    rec.update({name: stats(t) for name, t in times.items()})
    rec["device_shuffle_kernel"] = {"median_ms": float(np.median(km)), "min_ms": min(km), "max_ms": max(km)}
    rec["host_over_device_shuffle"] = med["host_shuffle_and_copy"] / med["device_shuffle"]
    rec["attribution_shuffle_over_device_shuffle"] = med["attribution_shuffle"] / med["attribution_device_shuffle"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000,10000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m = build()
    warm = np.random.default_rng(0).integers(0, 4, size=(1100, L)).astype(np.uint8)
    for f in legs(m, warm).values():
        f()
    recs = [run(m, int(n), a.reps) for n in a.sizes.split(",")]
    if a.out:
        json.dump(recs, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
