#!/usr/bin/env python3
"""Windows per second of scoring haplotypes that carry many variants, on one GPU: what a user could do
before score_haplotypes existed against score_haplotypes.

A device-resident random sequence of --length bases (10^6), --variants (10^5) random variants (half
SNVs, a quarter each insertions and deletions of 1..10 bases; one per 10-base slot, so none overlap),
--haplotypes (8) each carrying a random half of them, --windows (10^4) window starts on slot boundaries
(so no variant straddles one), both strands, two model shapes (C2: 300 units, k 19, L 200, T 1; the
reference default: 100 units).  Rows: the reference windows, then every haplotype in every window.  Legs:
  (a)  build every haplotype on the host (one np.concatenate per haplotype), cut the windows out as base
       codes and run predict() on the (rows,L) matrix, transfers included;
  (a') predict()'s loop on that matrix already on the device (model + eval_replica, two streams);
  (b)  score_haplotypes() on the device-resident sequence;
  (b_tables) the host-side part of (b) alone: build_haplotype_tables.
The legs' outputs are asserted equal before anything is timed.  One process; after a warm-up of every
leg the legs alternate --repeats (5) times, every pass ending in a device synchronise.  Per leg: median
and spread (max - min) in ms, rows/s from the median.  A leg is faster than another only when the medians
differ by more than the two spreads.  One JSON document.

usage: haplotypes_probe.py [--length 1000000] [--variants 100000] [--haplotypes 8] [--windows 10000]
                           [--repeats 5] [--out profiles/r15_haplotypes_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.variants_probe import K, L, SHAPES, T, _predict_device, make_model, timed  # noqa: E402

SLOT = 10


def make_variants(seq, n, seed=1):
    """One variant per 10-base slot, at the slot's first base, REF alleles of at most 10 bases."""
    rng = np.random.default_rng(seed)
    slots = np.sort(rng.choice(np.arange(len(seq) // SLOT), size=n, replace=False))
    pos = (slots * SLOT).astype(np.int64)
    ref_len = np.ones(n, dtype=np.int64)
    alts = []
    for i, p in enumerate(pos):
        kind = i % 4
        if kind < 2:
            alts.append(np.array([(seq[p] + 1 + rng.integers(0, 3)) % 4], dtype=np.uint8))
        elif kind == 2:
            ref_len[i] = 0
            alts.append(rng.integers(0, 4, size=int(rng.integers(1, 11))).astype(np.uint8))
        else:
            ref_len[i] = int(rng.integers(1, 11))
            alts.append(np.zeros(0, dtype=np.uint8))
    return pos, ref_len, alts


def host_matrix(seq, pos, ref_len, alts, haps, starts):
    """The (R + H*R, L) code matrix: the work of a user without the device path.  Every haplotype is
    built once, whole; a window that starts at reference base s starts on it at s + the shift of the
    variants left of s."""
    pad = np.full(L + 16, 4, np.uint8)
    R = len(starts)
    mat = np.empty((R + len(haps) * R, L), dtype=np.uint8)
    padded = np.concatenate((pad, seq, pad))
    mat[:R] = padded[(starts + len(pad))[:, None] + np.arange(L)[None, :]]
    for h, carried in enumerate(haps):
        idx = np.sort(np.asarray(carried))                       # (pos is ascending)
        pieces, at = [pad], 0
        for i in idx:
            pieces += [seq[at:pos[i]], alts[i]]
            at = pos[i] + ref_len[i]
        pieces += [seq[at:], pad]
        hap = np.concatenate(pieces)
        alt_len = np.fromiter((len(alts[i]) for i in idx), dtype=np.int64, count=len(idx))
        shift = np.concatenate((np.zeros(1, np.int64), np.cumsum(alt_len - ref_len[idx])))
        hs = starts + shift[np.searchsorted(pos[idx], starts, side="left")] + len(pad)
        mat[R + h * R:R + (h + 1) * R] = hap[hs[:, None] + np.arange(L)[None, :]]
    return mat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=1000000)
    ap.add_argument("--variants", type=int, default=100000)
    ap.add_argument("--haplotypes", type=int, default=8)
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/r15_haplotypes_probe.json")
    args = ap.parse_args()
    from explainn_amd.predict import predict
    from explainn_amd.variants import build_haplotype_tables, score_haplotypes
    rng = np.random.default_rng(0)
    seq = rng.integers(0, 4, size=args.length).astype(np.uint8)
    seq_d = torch.from_numpy(seq).cuda()
    pos, ref_len, alts = make_variants(seq, args.variants)
    V, H, R = len(pos), args.haplotypes, args.windows
    haps = [np.sort(rng.permutation(V)[:V // 2]) for _ in range(H)]
    starts = (rng.integers(0, (args.length - L) // SLOT, size=R) * SLOT).astype(np.int64)
    mat_d = torch.from_numpy(host_matrix(seq, pos, ref_len, alts, haps, starts)).cuda()
    rows = R + H * R
    tab = build_haplotype_tables(pos, ref_len, alts, haps, starts, L)
    assert tab["straddling"].sum() == 0
    doc = {"device": torch.cuda.get_device_name(0), "length": args.length, "variants": V, "haplotypes": H,
           "windows": R, "rows": rows, "edits_per_row_mean": float(tab["row_count"].mean()),
           "edits_per_row_max": int(tab["row_count"].max()), "repeats": args.repeats, "k": K, "L": L, "T": T,
           "strands": "both", "results": []}
    for name, units in SHAPES.items():
        model = make_model(units)
        fns = {
            "a_host_predict": lambda: predict(model, host_matrix(seq, pos, ref_len, alts, haps, starts)),
            "a2_device_predict": lambda: _predict_device(model, mat_d),
            "b_score_haplotypes": lambda: score_haplotypes(model, seq_d, pos, ref_len, alts, haps, starts),
            "b_tables_host_only": lambda: build_haplotype_tables(pos, ref_len, alts, haps, starts, L),
        }
        # warm-up (contexts, allocator, tables) and the equality of the legs' outputs
        a, a2, b, _ = (fn() for fn in fns.values())
        both = np.concatenate((b["ref"], b["hap"].reshape(H * R, T, 4)))
        assert np.array_equal(a, a2) and np.array_equal(a, both), "the legs' outputs differ"
        times = {leg: [] for leg in fns}
        for _ in range(args.repeats):
            for leg, fn in fns.items():                     # alternating
                times[leg].append(timed(fn))
        row = {"shape": name, "units": units, "rows": rows, "outputs_equal": True, "legs": {}}
        for leg, ts in times.items():
            med = float(np.median(ts))
            row["legs"][leg] = {"median_ms": med, "spread_ms": float(max(ts) - min(ts)),
                                "rows_per_s": rows / med * 1e3, "ms": ts}
        legs = row["legs"]
        # (b) less its table building: the transfers of the tables, the device calls, the copies back
        row["b_device_calls_ms"] = legs["b_score_haplotypes"]["median_ms"] - legs["b_tables_host_only"]["median_ms"]
        for other in ("a_host_predict", "a2_device_predict"):
            o, b_ = legs[other], legs["b_score_haplotypes"]
            row["b_beats_" + other] = bool(o["median_ms"] - b_["median_ms"] > o["spread_ms"] + b_["spread_ms"])
            row[other + "_beats_b"] = bool(b_["median_ms"] - o["median_ms"] > o["spread_ms"] + b_["spread_ms"])
        doc["results"].append(row)
        print(json.dumps({k: v for k, v in row.items() if k != "legs"} |
                         {leg: round(v["median_ms"], 2) for leg, v in legs.items()}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
