#!/usr/bin/env python3
"""Time of a model-bank training step against the existing single-model training step, on one GPU.

At U = 100, L = 200, k = 19, T = 1 and B in {100, 1024}, for G in {1, 2, 5, 10, 20}, ms per step of
  (a) StepEngine + FusedAdam on an ExplaiNNBank of G members (resident batch),
  (b) the bank trainer loop (selene.BankTrainer.train) fed by a device-resident CodesLoader,
  (c) the existing selene.Trainer.train step on ONE 100-unit ExplaiNN fed by the same kind of loader
      -- the path a sequence of --initialize runs takes, untouched by the bank.
Windows of --steps steps end in a device synchronise; the legs alternate --repeats times in one
process after a warm-up.  Per leg: median window, spread (max - min), time per member-step = bank
step / G.  The check the bank has to pass is computed and printed: at G = 10, B = 100 the time per
member-step of (a) and of (b) is below (c) by more than the two spreads.  One JSON document.

usage: bank_probe.py [--steps 1000] [--repeats 5] [--out profiles/r09_bank_probe.json]
       bank_probe.py --trace-leg G B STEPS      (one bank leg alone, for a kernel trace)"""
import argparse
import json
import sys
import tempfile
import time

import os

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

U, K, L, T = 100, 19, 200, 1


def _data(B):
    from explainn_amd.loader import CodesLoader
    rng = np.random.default_rng(B)
    codes = rng.integers(0, 4, size=(B * 40, L)).astype(np.uint8)
    labels = (rng.random((B * 40, T)) > 0.5).astype(np.float32)
    return CodesLoader(codes, labels, B, True, False, "cuda"), codes, labels


def _window(step_fn):
    def window(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step_fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    return window


def engine_leg(G, B):
    from explainn_amd import ExplaiNN, ExplaiNNBank, get_optimizer
    from explainn_amd.engine import StepEngine
    torch.manual_seed(G)
    m = (ExplaiNN(U, K, L, T) if G == 1 else ExplaiNNBank(G, U, K, L, T)).cuda().train()
    eng = StepEngine(m, B, "binary")
    eng.attach_grads()
    opt = get_optimizer(m.parameters())
    _, codes, labels = _data(B)
    x = torch.from_numpy(codes[:B]).cuda()
    y = torch.from_numpy(labels[:B]).cuda()

    def step():
        eng.step(x, y)
        opt.step()
    return _window(step)


def bank_trainer_leg(G, B):
    from explainn_amd import ExplaiNNBank, get_optimizer
    from explainn_amd.selene import BankTrainer
    torch.manual_seed(G)
    bank = ExplaiNNBank(G, U, K, L, T)
    loader, _, _ = _data(B)
    tr = BankTrainer(bank, {"train": loader, "validation": loader}, "binary", {},
                     get_optimizer(bank.parameters()), report_stats_every_n_steps=10 ** 9,
                     output_dir=tempfile.mkdtemp(), logging_verbosity=0)

    def step():
        tr.step += 1
        tr.train()
    return _window(step)


def trainer_leg(B):
    from explainn_amd import ExplaiNN, get_loss, get_optimizer
    from explainn_amd.selene import Trainer
    torch.manual_seed(1)
    m = ExplaiNN(U, K, L, T)
    loader, _, _ = _data(B)
    tr = Trainer(m, {"train": loader, "validation": loader}, get_loss("binary"), {},
                 get_optimizer(m.parameters()), report_stats_every_n_steps=10 ** 9,
                 output_dir=tempfile.mkdtemp(), use_cuda=True, logging_verbosity=0)
    tr.step = 0

    def step():
        tr.step += 1
        tr.train()
        if len(tr._time_per_step) > 4096:        # (the Trainer empties these when it reports)
            tr._settle_train_loss()
            tr._time_per_step, tr._train_loss = [], []
    return _window(step)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace-leg":
        G, B, steps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
        engine_leg(G, B)(steps)
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 2, 5, 10, 20])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {"shape": {"U": U, "k": K, "L": L, "T": T}, "steps_per_window": a.steps, "windows": a.repeats,
           "legs": [], "checks": []}
    for B in (100, 1024):
        legs = {("c", 1): trainer_leg(B)}
        for G in a.groups:
            legs[("a", G)] = engine_leg(G, B)
            if G > 1:
                legs[("b", G)] = bank_trainer_leg(G, B)
        for w in legs.values():
            w(a.warmup)
        times = {key: [] for key in legs}
        for _ in range(a.repeats):
            for key, w in legs.items():           # alternating
                times[key].append(w(a.steps))
        stat = {}
        for (leg, G), t in times.items():
            stat[(leg, G)] = (float(np.median(t)), float(max(t) - min(t)))
            doc["legs"].append({"B": B, "leg": leg, "G": G, "ms_per_step_median": stat[(leg, G)][0],
                                "spread_ms": stat[(leg, G)][1], "windows_ms": t,
                                "ms_per_member_step": stat[(leg, G)][0] / G,
                                "member_step_spread_ms": stat[(leg, G)][1] / G})
        c_ms, c_sp = stat[("c", 1)]
        for leg in ("a", "b"):
            for G in a.groups:
                if (leg, G) not in stat or G == 1:
                    continue
                ms, sp = stat[(leg, G)]
                doc["checks"].append({"B": B, "leg": leg, "G": G, "member_step_ms": ms / G,
                                      "trainer_step_ms": c_ms, "spreads_ms": sp / G + c_sp,
                                      "below_by_more_than_the_spreads": bool(ms / G + sp / G + c_sp < c_ms)})
        del legs
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    for c in doc["checks"]:
        if c["G"] == 10 and c["B"] == 100:
            print("CHECK G=10 B=100 leg (%s): %.4f ms per member-step vs %.4f ms Trainer.train step, spreads %.4f: %s"
                  % (c["leg"], c["member_step_ms"], c["trainer_step_ms"], c["spreads_ms"],
                     "below" if c["below_by_more_than_the_spreads"] else "NOT below"))


if __name__ == "__main__":
    main()
