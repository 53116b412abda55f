#!/usr/bin/env python3
"""Time to list every motif site of a long sequence, on one GPU: the route a user had before
call_sites existed against call_sites.

A device-resident random sequence of --length bases (10^6), k 19, L 200, at 100 and 300 units of
random filters scaled by --filter-scale (3: see make_model);
thresholds are 0.5 x each unit's largest float16 activation on the sequence; both strands.  Legs:
  (a)  windows at stride Lo = L - k + 1 (they hold every k-mer once) cut on the device, through
       model.linears[:3] in batches, cast to float16, copied to the host, np.nonzero(acts > thr) --
       the reverse strand on the windows of the reverse-complemented sequence; transfers included;
  (b)  call_sites(model, seq_d, thresholds), the records read back (SiteCalls on the host).
One process; after a warm-up of both legs they alternate --repeats (5) times, every pass ending with
its result on the host.  Per leg: median and spread (max - min) in ms.  (b) beats (a) only when the
medians differ by more than the two spreads: `call_sites_beats_dense` is that verdict.  One JSON
document.  The two legs' site counts are compared before anything is timed.

usage: sites_probe.py [--length 1000000] [--repeats 5] [--filter-scale 3] [--out profiles/r12_sites_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, L, T = 19, 200, 1
LO = L - K + 1
SHAPES = {"C2_u300": 300, "default_u100": 100}
BATCH = 512                      # windows per linears[:3] call: 512 x 300 x 182 fp32 = 112 MB


def _rc(seq_d):
    r = seq_d.flip(0)
    return torch.where(r < 4, 3 - r, r)


def _window_matrix(seq_d):
    """(W,L) windows at stride Lo, the last one pulled back to the sequence's end."""
    n = seq_d.numel()
    starts = list(range(0, n - L + 1, LO))
    if starts[-1] != n - L:
        starts.append(n - L)
    idx = torch.tensor(starts, device=seq_d.device)[:, None] + torch.arange(L, device=seq_d.device)[None, :]
    return starts, seq_d[idx]


def dense_route(model, seq_d, thr16, want_max=False):
    """Leg (a).  Returns per strand the (window, unit, offset) index arrays of np.nonzero -- or, for the
    set-up pass, the per-unit float16 maxima."""
    out, umax = [], None
    thr = thr16[None, :, None] if thr16 is not None else None
    for strand_seq in (seq_d, _rc(seq_d)):
        starts, win = _window_matrix(strand_seq)
        hits = []
        with torch.no_grad():
            for i in range(0, len(win), BATCH):
                acts = model.linears[:3](win[i:i + BATCH]).to(torch.float16).cpu().numpy()
                if want_max:
                    m = acts.max(axis=(0, 2))
                    umax = m if umax is None else np.maximum(umax, m)
                else:
                    w, u, j = np.nonzero(acts > thr)
                    hits.append((w + i, u, j))
        out.append(hits)
        if want_max:
            break                                   # the thresholds come from the forward strand
    return umax if want_max else out


def count_dense(res, starts_n, n_pos):
    """Sites of leg (a) with the last window's overlap counted once."""
    total = 0
    for hits in res:
        for w, u, j in hits:
            last = w == starts_n - 1
            dup = last & (j < (starts_n - 1) * LO - (n_pos - LO)) if starts_n > 1 else np.zeros(len(w), bool)
            total += len(w) - int(dup.sum())
    return total


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def make_model(units, scale):
    """Random filters scaled by `scale`: with the default initialisation a third of all positions exceed
    half a unit's maximum; scaled by 3 a site is a rare event (a couple of hundred per unit and strand in 10^6 bases),
    as with trained filters."""
    from explainn_amd import ExplaiNN
    torch.manual_seed(units)
    m = ExplaiNN(units, K, L, T).cuda().eval()
    with torch.no_grad():
        m.linears[0].weight.mul_(scale)
    m.validate_input = False
    return m


def main():
    from explainn_amd.sites import call_sites
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--filter-scale", type=float, default=3.0)
    ap.add_argument("--out", default="profiles/r12_sites_probe.json")
    args = ap.parse_args()
    seq = np.random.default_rng(0).integers(0, 4, size=args.length).astype(np.uint8)
    seq_d = torch.from_numpy(seq).cuda()
    n_pos = args.length - K + 1
    doc = {"device": torch.cuda.get_device_name(0), "length": args.length, "repeats": args.repeats,
           "k": K, "L": L, "strands": "both", "threshold": "0.5 x unit max (float16)", "filter_scale": args.filter_scale,
           "results": []}
    for name, units in SHAPES.items():
        model = make_model(units, args.filter_scale)
        thr16 = (0.5 * dense_route(model, seq_d, None, want_max=True)).astype(np.float16)
        thr32 = thr16.astype(np.float32)
        fns = {"a_dense_nonzero": lambda: dense_route(model, seq_d, thr16),
               "b_call_sites": lambda: call_sites(model, seq_d, thr32)}
        res_a, res_b = fns["a_dense_nonzero"](), fns["b_call_sites"]()          # warm-up, and the same answer
        n_win = len(_window_matrix(seq_d)[0])
        sites_a, sites_b = count_dense(res_a, n_win, n_pos), len(res_b)
        if sites_a != sites_b:
            raise SystemExit("the legs disagree: %d sites dense, %d from call_sites" % (sites_a, sites_b))
        times = {leg: [] for leg in fns}
        for _ in range(args.repeats):
            for leg, fn in fns.items():                                         # alternating
                times[leg].append(timed(fn))
        row = {"shape": name, "units": units, "positions": n_pos, "sites": sites_b, "legs": {}}
        for leg, ts in times.items():
            row["legs"][leg] = {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts}
        a, b = row["legs"]["a_dense_nonzero"], row["legs"]["b_call_sites"]
        row["call_sites_beats_dense"] = bool(a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
        doc["results"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "legs"} |
                         {leg: [round(v["median_ms"], 2), round(v["spread_ms"], 2)] for leg, v in row["legs"].items()}),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
