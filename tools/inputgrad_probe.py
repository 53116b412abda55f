#!/usr/bin/env python3
"""Times the input gradient at C2 (300 units, k 19, L 200, T 1) on one GPU: interpret.input_gradients
over 4096-sequence eval batches next to plain eval forwards of the same batches, and the train step
(forward + backward, dropout on) with and without x.grad at batch 1024.  One JSON line per figure.

usage: inputgrad_probe.py [--reps R]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from explainn_amd import ExplaiNN, interpret  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402


def timed(fn, reps):
    fn(); torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    U, k, L, T = 300, 19, 200, 1
    sd = orc.random_state_dict(U, k, L, T, seed=0)
    m = ExplaiNN(U, k, L, T)
    m.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    m.cuda().eval()
    N = 4096 * 4
    X = torch.from_numpy(orc.random_onehot(N, L, seed=1, n_frac=0.01)).cuda()
    dl = torch.ones(4096, T, device="cuda")

    def ig():
        with torch.no_grad(), m.eval_cache():
            for i in range(0, N, 4096):
                m.input_gradient(X[i:i + 4096], dl)

    def fwd():
        with torch.no_grad(), m.eval_cache():
            for i in range(0, N, 4096):
                m(X[i:i + 4096])

    t_ig, t_fwd = timed(ig, a.reps), timed(fwd, a.reps)
    print(json.dumps({"what": "eval input gradient, C2, batches of 4096 (device arrays)", "sequences": N,
                      "s": t_ig, "seq_per_s": N / t_ig, "eval_forward_s": t_fwd,
                      "eval_forward_seq_per_s": N / t_fwd}))
    Xh = X.cpu().numpy()
    t0 = time.perf_counter(); interpret.input_gradients(m, Xh, batch_size=4096); t_api = time.perf_counter() - t0
    print(json.dumps({"what": "interpret.input_gradients, host numpy in and out, C2", "sequences": N,
                      "s": t_api, "seq_per_s": N / t_api}))
    m.train()
    xb = X[:1024].clone()
    g = torch.ones(1024, T, device="cuda")

    def step(want):
        xt = xb.clone().requires_grad_(want)
        m(xt).backward(g)

    t_plain, t_dx = timed(lambda: step(False), a.reps * 10), timed(lambda: step(True), a.reps * 10)
    print(json.dumps({"what": "train step fwd+bwd via autograd, C2, batch 1024", "without_dx_ms": 1e3 * t_plain,
                      "with_dx_ms": 1e3 * t_dx}))


if __name__ == "__main__":
    main()
