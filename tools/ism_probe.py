#!/usr/bin/env python3
"""Times in-silico mutagenesis on one GPU at C2 (300 units, k 19, L 200, T 1) and C3 (T 50), 4096
sequences: (a) interpret.in_silico_mutagenesis, (b) brute force -- the 3L mutants of every sequence
as BaseCodes batches through model(x) in eval mode, built on the device.  The legs alternate in one
process after a warm-up; times are wall clock around a device synchronise.  One JSON line per config:
input sequences/s of each leg, their ratio and the max |difference| between the two deltas.

usage: ism_probe.py [--reps R] [--configs C2,C3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explainn_amd import ExplaiNN, interpret  # noqa: E402
from explainn_amd.architectures import BaseCodes  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402

N = 4096
CHUNK = 16           # sequences per brute-force pass: 16 x 3L = 9600 mutants


def brute(m, codes, L, want=None):
    """delta (N,T,4,L) on the device from the mutants' logits; with `want`, returns max |want - it|."""
    T = m._options["n_features"]
    p = torch.arange(L, device=codes.device).repeat(3)
    dd = torch.arange(1, 4, device=codes.device).repeat_interleave(L)
    err = 0.0
    with torch.no_grad():
        base = m(BaseCodes(codes))
        for i in range(0, codes.shape[0], CHUNK):
            c = codes[i:i + CHUNK]
            B = c.shape[0]
            mut = c.repeat_interleave(3 * L, dim=0).view(B, 3 * L, L)
            s = c[:, p].long()                                               # (B, 3L)
            a = torch.where(s < 4, (s + dd) & 3, dd % 4)                     # N: a = 1, 2, 3 (0 below)
            mut.scatter_(2, p.view(1, -1, 1).expand(B, -1, 1), a.to(torch.uint8).unsqueeze(2))
            lg = m(BaseCodes(mut.view(B * 3 * L, L))).view(B, 3 * L, T)
            d = lg - base[i:i + B, None, :]
            if want is not None:
                w = want[i:i + B]                                            # (B,T,4,L)
                got = w.permute(0, 3, 2, 1)[torch.arange(B, device=c.device)[:, None], p, a]   # (B,3L,T)
                err = max(err, float((got - d).abs().max()))
    torch.cuda.synchronize()
    return err


def run(cfg, T, reps):
    U, k, L = 300, 19, 200
    sd = orc.random_state_dict(U, k, L, T, seed=0)
    m = ExplaiNN(U, k, L, T)
    m.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    m.cuda().eval()
    codes_np = np.random.default_rng(1).integers(0, 4, size=(N, L)).astype(np.uint8)
    codes = torch.from_numpy(codes_np).cuda()

    def ism():
        with torch.no_grad(), m.eval_cache():
            return m.in_silico_mutagenesis(BaseCodes(codes))

    _, delta = ism(); torch.cuda.synchronize()
    err = brute(m, codes, L, want=delta)
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); ism(); torch.cuda.synchronize(); ta.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); brute(m, codes, L); tb.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); interpret.in_silico_mutagenesis(m, codes_np); t_api = time.perf_counter() - t0
    a, b = float(np.median(ta)), float(np.median(tb))
    print(json.dumps({"config": cfg, "U": U, "k": k, "L": L, "T": T, "sequences": N,
                      "ism_seq_per_s": N / a, "brute_force_seq_per_s": N / b, "speedup": b / a,
                      "interpret_api_seq_per_s_incl_host_copy": N / t_api,
                      "max_abs_diff": err, "ism_ms": a * 1e3, "brute_ms": b * 1e3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="C2,C3")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        run(cfg, {"C2": 1, "C3": 50}[cfg], a.reps)


if __name__ == "__main__":
    main()
