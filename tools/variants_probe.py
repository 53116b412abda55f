#!/usr/bin/env python3
"""Variants per second of scoring SNVs and short indels, on one GPU: what a user could do before
score_variants existed against score_variants.

A device-resident random sequence of --length bases (10^6), --snvs (10^5) random SNVs plus --indels
(10^4) insertions and deletions of 1..10 bases, both strands, shifts=(0,), two model shapes (C2: 300
units, k 19, L 200, T 1; the reference default: 100 units).  Legs:
  (a)  materialise the ref and alt window of every variant on the host as base codes (numpy) and run
       predict() on the (2V,L) matrix, transfers included;
  (a') predict()'s loop on that matrix already on the device (model + eval_replica, two streams);
  (b)  score_variants() on the device-resident sequence.
The legs' outputs are asserted equal before anything is timed.  One process; after a warm-up of every
leg the legs alternate --repeats (5) times, every pass ending in a device synchronise (every leg ends
in a copy to the host).  Per leg: median and spread (max - min) in ms, variants/s from the median.  A
leg is faster than another only when the medians differ by more than the two spreads.  One JSON
document.

usage: variants_probe.py [--length 1000000] [--snvs 100000] [--indels 10000] [--repeats 5]
                         [--out profiles/r13_variants_probe.json]"""
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


def make_variants(seq, n_snv, n_indel, seed=1):
    rng = np.random.default_rng(seed)
    N = len(seq)
    pos = rng.integers(0, N - 10, size=n_snv + n_indel).astype(np.int64)
    ref_len = np.ones(n_snv + n_indel, dtype=np.int64)
    alts = [np.array([(seq[p] + 1 + rng.integers(0, 3)) % 4], dtype=np.uint8) for p in pos[:n_snv]]
    for i in range(n_indel):
        n = int(rng.integers(1, 11))
        if i % 2:
            ref_len[n_snv + i] = 0
            alts.append(rng.integers(0, 4, size=n).astype(np.uint8))
        else:
            ref_len[n_snv + i] = n
            alts.append(np.zeros(0, dtype=np.uint8))
    return pos, ref_len, alts


def host_matrix(seq, pos, ref_len, alts):
    """The (2V,L) code matrix of the ref and alt windows, row 2v and 2v+1: the work of a user without
    the device path (one padded copy of the sequence, fancy indexing for the reference rows, one
    splice per variant for the alt rows)."""
    from explainn_amd.variants import window_start
    V = len(pos)
    alt_len = np.fromiter((len(a) for a in alts), dtype=np.int64, count=V)
    start = window_start(pos, ref_len, alt_len, L)
    pad = L + 16
    padded = np.concatenate((np.full(pad, 4, np.uint8), seq, np.full(pad, 4, np.uint8)))
    mat = np.empty((2 * V, L), dtype=np.uint8)
    mat[0::2] = padded[(start + pad)[:, None] + np.arange(L)[None, :]]
    for v in range(V):
        s, p = int(start[v]) + pad, int(pos[v]) + pad
        hap = np.concatenate((padded[s:p], alts[v], padded[p + int(ref_len[v]):p + int(ref_len[v]) + L]))
        mat[2 * v + 1] = hap[:L]
    return mat


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
    return torch.cat(outs).numpy().astype(np.float64)


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
    ap.add_argument("--snvs", type=int, default=100000)
    ap.add_argument("--indels", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/r13_variants_probe.json")
    args = ap.parse_args()
    from explainn_amd.predict import predict
    from explainn_amd.variants import score_variants
    seq = np.random.default_rng(0).integers(0, 4, size=args.length).astype(np.uint8)
    seq_d = torch.from_numpy(seq).cuda()
    pos, ref_len, alts = make_variants(seq, args.snvs, args.indels)
    V = len(pos)
    mat_d = torch.from_numpy(host_matrix(seq, pos, ref_len, alts)).cuda()
    doc = {"device": torch.cuda.get_device_name(0), "length": args.length, "snvs": args.snvs,
           "indels": args.indels, "repeats": args.repeats, "k": K, "L": L, "T": T, "strands": "both",
           "shifts": [0], "results": []}
    for name, units in SHAPES.items():
        model = make_model(units)
        fns = {
            "a_host_predict": lambda: predict(model, host_matrix(seq, pos, ref_len, alts)),
            "a2_device_predict": lambda: _predict_device(model, mat_d),
            "b_score_variants": lambda: score_variants(model, seq_d, pos, ref_len, alts),
        }
        # warm-up (contexts, allocator, tables) and the equality of the legs' outputs
        a, a2, b = (fn() for fn in fns.values())
        pair = np.stack((b["ref"][:, 0], b["alt"][:, 0]), axis=1).reshape(2 * V, T, 4)
        assert np.array_equal(a, a2) and np.array_equal(a, pair), "the legs' outputs differ"
        times = {leg: [] for leg in fns}
        for _ in range(args.repeats):
            for leg, fn in fns.items():                     # alternating
                times[leg].append(timed(fn))
        row = {"shape": name, "units": units, "variants": V, "rows": 2 * V, "outputs_equal": True, "legs": {}}
        for leg, ts in times.items():
            med = float(np.median(ts))
            row["legs"][leg] = {"median_ms": med, "spread_ms": float(max(ts) - min(ts)),
                                "variants_per_s": V / med * 1e3, "ms": ts}
        for other in ("a_host_predict", "a2_device_predict"):
            o, b_ = row["legs"][other], row["legs"]["b_score_variants"]
            row["b_beats_" + other] = bool(o["median_ms"] - b_["median_ms"] > o["spread_ms"] + b_["spread_ms"])
            row[other + "_beats_b"] = bool(b_["median_ms"] - o["median_ms"] > o["spread_ms"] + b_["spread_ms"])
        doc["results"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "legs"} |
                         {leg: round(v["median_ms"], 2) for leg, v in row["legs"].items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
