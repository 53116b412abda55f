#!/usr/bin/env python3
"""Windows per second of scoring a long sequence, on one GPU: what a user could do before the scan
existed against the scan's two modes.

A device-resident random sequence of --length bases (10^6), both strands scored, two model shapes
(C2: 300 units, k 19, L 200, T 1; the reference default: 100 units), strides 7, 14, 49, 98, 203
(+ 50 for the legs that take any stride).  Legs:
  (a)  materialise every window on the host (numpy sliding window over the host copy of the
       sequence) and call predict() on the (W,L) code matrix, transfers included;
  (a') predict()'s loop on the window matrix already on the device (model + eval_replica, two streams);
  (b)  scan(mode="windows");   (c)  scan(mode="shared").
One process; after a warm-up of every leg the legs alternate --repeats (5) times, every window one
whole pass over the sequence ending in a device synchronise (the scan and predict() end in a copy to
the host, which synchronises).  Per leg: median and spread (max - min) in ms, windows/s from the
median.  A leg is faster than another only when the medians differ by more than the two spreads:
`shared_beats_windows` per (shape, stride) is that verdict, the AUTO rule's input.  One JSON document.

usage: scan_probe.py [--length 1000000] [--repeats 5] [--out profiles/r11_scan_probe.json]
       scan_probe.py --trace-leg LEG UNITS STRIDE    (one leg alone, for a kernel trace)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, L, T = 19, 200, 1
SHAPES = {"C2_u300": 300, "default_u100": 100}
STRIDES = [7, 14, 49, 98, 203, 50]


def _windows_host(seq, stride):
    v = np.lib.stride_tricks.sliding_window_view(seq, L)[::stride]
    return np.ascontiguousarray(v)


def _predict_device(model, mat_d):
    """predict()'s loop on a device-resident (W,L) code matrix."""
    from explainn_amd.architectures import BaseCodes
    rep = model.eval_replica()
    dev = mat_d.device
    cur = torch.cuda.current_stream(dev)
    if model._rt.side_stream is None:
        model._rt.side_stream = torch.cuda.Stream(dev)
    side = model._rt.side_stream
    outs = []
    with torch.no_grad(), model.eval_cache(), rep.eval_cache():
        for i in range(0, len(mat_d), 4096):
            xb = mat_d[i:i + 4096]
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                rev = rep(BaseCodes(xb, True))
            fwd = model(BaseCodes(xb))
            cur.wait_stream(side)
            outs.append(torch.stack((fwd, rev, (fwd + rev) / 2, torch.maximum(fwd, rev)), dim=2).cpu())
    return outs


def legs(model, seq, seq_d, stride):
    from explainn_amd.predict import predict
    from explainn_amd.scan import scan
    mat_d = torch.from_numpy(_windows_host(seq, stride)).cuda()
    out = {
        "a_host_predict": lambda: predict(model, _windows_host(seq, stride)),
        "a2_device_predict": lambda: _predict_device(model, mat_d),
        "b_scan_windows": lambda: scan(model, seq_d, stride=stride, mode="windows"),
    }
    if stride % 7 == 0:
        out["c_scan_shared"] = lambda: scan(model, seq_d, stride=stride, mode="shared")
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def make_model(units):
    from explainn_amd import ExplaiNN
    torch.manual_seed(units)
    m = ExplaiNN(units, K, L, T).cuda().eval()
    m.validate_input = False
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/r11_scan_probe.json")
    ap.add_argument("--trace-leg", nargs=3, metavar=("LEG", "UNITS", "STRIDE"))
    args = ap.parse_args()
    seq = np.random.default_rng(0).integers(0, 4, size=args.length).astype(np.uint8)
    seq_d = torch.from_numpy(seq).cuda()
    if args.trace_leg:
        leg, units, stride = args.trace_leg[0], int(args.trace_leg[1]), int(args.trace_leg[2])
        fn = legs(make_model(units), seq, seq_d, stride)[leg]
        fn()
        fn()
        torch.cuda.synchronize()
        return
    doc = {"device": torch.cuda.get_device_name(0), "length": args.length, "repeats": args.repeats,
           "k": K, "L": L, "T": T, "strands": "both", "results": []}
    for name, units in SHAPES.items():
        model = make_model(units)
        for stride in STRIDES:
            fns = legs(model, seq, seq_d, stride)
            W = (args.length - L) // stride + 1
            for fn in fns.values():
                fn()                                        # warm-up: contexts, allocator, tables
            times = {leg: [] for leg in fns}
            for _ in range(args.repeats):
                for leg, fn in fns.items():                 # alternating
                    times[leg].append(timed(fn))
            row = {"shape": name, "units": units, "stride": stride, "windows": W, "legs": {}}
            for leg, ts in times.items():
                med = float(np.median(ts))
                row["legs"][leg] = {"median_ms": med, "spread_ms": float(max(ts) - min(ts)),
                                    "windows_per_s": W / med * 1e3, "ms": ts}
            if "c_scan_shared" in times:
                b, c = row["legs"]["b_scan_windows"], row["legs"]["c_scan_shared"]
                row["shared_beats_windows"] = bool(b["median_ms"] - c["median_ms"] > b["spread_ms"] + c["spread_ms"])
                row["windows_beats_shared"] = bool(c["median_ms"] - b["median_ms"] > b["spread_ms"] + c["spread_ms"])
            doc["results"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "legs"} |
                             {leg: round(v["median_ms"], 2) for leg, v in row["legs"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
