#!/usr/bin/env python3
"""Time of the per-record best PWM site (csrc/pwmbest.hip) and of the two analyses built on it, on one GPU,
against the route a user had before.

Motifs: 300 and 2000 Dirichlet(0.3) matrices of width 6..24; records: 10^4 and 10^5 random records of 200
bases without N (the stock route below has no rule for N); both strands, uniform background, 100 bins.
Legs (each ends with its result synchronised):
  best_kernel   explainn_pwm_record_best on device-resident codes, offsets and tables: bits and sites of every
                (motif, record) (device events)
  enrichment    host records and matrices -> motif_enrichment(first half, second half as control) -> result on
                the host (host clock)
  centrality    host records and matrices -> motif_centrality(all records, p = 1e-4) -> result on the host
                (host clock)
  torch_route   stock torch on the same GPU, what the parent commit offers for the kernel's job: one-hot
                (R,4,200) fp32, per width group one torch.nn.functional.conv1d with the integer tables as weights
                and one with the reverse-complemented tables, the maximum of the two strands, amax per record;
                the records go over in pieces of --piece so that a group's (piece, motifs, starts) score array
                stays small (host clock, the device score matrix as the result).  Scores <= 8192 are exact in
                fp32.  It gives the scores only, not the sites.
Before timing the kernel's and the torch route's scores are compared: they must be equal.  Every (motifs,
records) runs in a process of its own under its own time limit; the first one that fails or runs out of time
ends the probe.  A warm-up pass, then --passes (3) timed passes: median and spread (max - min) in ms.
`kernel_beats_torch`: the medians differ by more than the two spreads.

usage: pwmbest_probe.py [--passes 3] [--limit 240] [--out profiles/r30_pwmbest_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MOTIFS = (300, 2000)
RECORDS = (10000, 100000)
LENGTH, PVALUE, BINS = 200, 1e-4, 100


def _child(M, R, passes, piece):
    import numpy as np
    import torch

    from explainn_amd import pwmenrich, pwmsites

    g = np.random.default_rng(M)
    widths = g.integers(6, 25, size=M)
    mats = [g.dirichlet(np.full(4, 0.3), size=int(w)).reshape(int(w), 4) for w in widths]
    rows = np.random.default_rng(0).integers(0, 4, size=(R, LENGTH)).astype(np.uint8)
    records = list(rows)
    S, w32, scale, lo = pwmsites.quantise(mats, np.full(4, 0.25), 0.1, BINS)
    live = np.where(scale > 0, w32, 0).astype(np.int32)
    scores, wd = torch.from_numpy(S).cuda(), torch.from_numpy(live).cuda()
    codes_d = torch.from_numpy(rows).cuda()
    flat = codes_d.reshape(-1)
    off = torch.arange(R + 1, device="cuda", dtype=torch.int64) * LENGTH

    def best_kernel():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        bits, site = pwmenrich.record_best_device(scores, wd, flat, off, True, True)
        b.record()
        b.synchronize()
        return bits, a.elapsed_time(b)

    def enrichment():
        t0 = time.perf_counter()
        res = pwmenrich.motif_enrichment(mats, records[:R // 2], records[R // 2:], bins=BINS)
        return res, (time.perf_counter() - t0) * 1e3

    def centrality():
        t0 = time.perf_counter()
        res = pwmenrich.motif_centrality(mats, records, (PVALUE,), bins=BINS)
        return res, (time.perf_counter() - t0) * 1e3

    groups = []                                            # per width: motif indices, fwd and rc weights
    for w in sorted(set(live.tolist()) - {0}):
        idx = np.flatnonzero(live == w)
        fwd = S[idx, :w].astype(np.float32).transpose(0, 2, 1)                    # (m, 4, w)
        rev = S[idx, :w][:, ::-1, ::-1].astype(np.float32).transpose(0, 2, 1)     # the table of the other strand
        groups.append((torch.from_numpy(idx).cuda(), torch.from_numpy(np.ascontiguousarray(fwd)).cuda(),
                       torch.from_numpy(np.ascontiguousarray(rev)).cuda()))

    def torch_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = torch.zeros((M, R), dtype=torch.int16, device="cuda")
        for r0 in range(0, R, piece):
            x = torch.nn.functional.one_hot(codes_d[r0:r0 + piece].to(torch.int64), 4).to(torch.float32).transpose(1, 2)
            for idx, fwd, rev in groups:
                top = torch.maximum(torch.nn.functional.conv1d(x, fwd), torch.nn.functional.conv1d(x, rev)).amax(dim=2)
                out[idx, r0:r0 + piece] = top.T.to(torch.int16)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    row = {"motifs": M, "records": R, "bases": LENGTH, "device": torch.cuda.get_device_name(0)}
    row["torch_route_equals_kernel"] = bool(torch.equal(best_kernel()[0], torch_route()[0]))
    if not row["torch_route_equals_kernel"]:
        raise SystemExit("the routes disagree: %r" % row)
    row["legs"] = {}
    for name, fn in (("best_kernel", best_kernel), ("torch_route", torch_route), ("enrichment", enrichment),
                     ("centrality", centrality)):
        fn()                                                                      # warm-up
        ts = [fn()[1] for _ in range(passes)]
        row["legs"][name] = {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per (motifs, records) process")
    ap.add_argument("--piece", type=int, default=4096, help="records per piece of the torch route")
    ap.add_argument("--out", default="profiles/r30_pwmbest_probe.json")
    ap.add_argument("--child", nargs=2, metavar=("MOTIFS", "RECORDS"))
    args = ap.parse_args()
    if args.child:
        return _child(int(args.child[0]), int(args.child[1]), args.passes, args.piece)
    doc = {"widths": "6..24", "strands": "both", "pvalue": PVALUE, "bins": BINS, "background": "uniform",
           "record_bases": LENGTH, "passes": args.passes, "torch_piece": args.piece, "results": []}
    ok = True
    for M in MOTIFS:
        for R in RECORDS:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--passes",
                   str(args.passes), "--piece", str(args.piece), "--child", str(M), str(R)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not rows:
                print("motifs %d records %d: exit %d (124 / 137: over its limit of %d s); the probe ends here\n%s" % (
                    M, R, out.returncode, args.limit, out.stderr[-2000:]), flush=True)
                ok = False
                break
            doc.setdefault("device", rows[0].pop("device"))
            rows[0].pop("device", None)
            doc["results"].append(rows[0])
            print(json.dumps({"motifs": M, "records": R, **{k: [round(v["median_ms"], 3), round(v["spread_ms"], 3)]
                                                            for k, v in rows[0]["legs"].items()}}), flush=True)
        if not ok:
            break
    doc["kernel_beats_torch"] = {}
    for r in doc["results"]:
        a, b = r["legs"]["torch_route"], r["legs"]["best_kernel"]
        doc["kernel_beats_torch"]["m%d_r%d" % (r["motifs"], r["records"])] = bool(
            a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
