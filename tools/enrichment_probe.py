#!/usr/bin/env python3
"""Time of motif enrichment on one GPU: the two device entry points, and the route a user had before them.

Device-resident random records of 200 bases, k 19, L 200, at 100 and 300 units, 10^4 and 10^5 records, both
strands; the first half of the records is the primary set.  Legs (each ends with its result synchronised):
  record_best      explainn_record_best alone: one call, bits and sites of every (unit, record)
  enrichment_test  explainn_enrichment_test alone, on record_best's bits
  dense_amax       the route of the parent commit to the same matrix: the records as windows ->
                   model.linears[:3] -> float16 -> amax over the positions, both strands, on the same GPU
  dense_fisher     the parent commit's test at ONE threshold per unit, the device's best one: counts by torch
                   on the float16 matrix, then scipy.stats.fisher_exact per unit on the host (the device
                   evaluates every threshold; a host search over them would cost this leg times their number)
Every (leg, units, records) runs in a process of its own under its own time limit; the first one that fails or
runs out of time ends the probe.  In a process: a warm-up pass, then --passes (3) timed passes; median and
spread (max - min) in ms.  Before timing, dense_amax is compared with record_best (the bit patterns must be
equal) and dense_fisher with enrichment_test (p-values within 1e-7 relative).  `device_beats_dense`: the
medians differ by more than the two spreads.  One JSON document.

usage: enrichment_probe.py [--passes 3] [--limit 240] [--out profiles/r22_enrichment_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, L, T = 19, 200, 1
UNITS = (100, 300)
RECORDS = (10000, 100000)
LEGS = ("record_best", "enrichment_test", "dense_amax", "dense_fisher")
PAIRS = {"dense_amax": "record_best", "dense_fisher": "enrichment_test"}
BATCH = 512                      # windows per linears[:3] call: 512 x 300 x 182 fp32 = 112 MB


def _child(leg, units, records, passes):
    import numpy as np
    import torch

    from explainn_amd import ExplaiNN
    from explainn_amd.enrichment import enrichment_test

    torch.manual_seed(units)
    model = ExplaiNN(units, K, L, T).cuda().eval()
    model.validate_input = False
    rows = torch.from_numpy(np.random.default_rng(0).integers(0, 4, size=(records, L)).astype(np.uint8)).cuda()
    flat = rows.view(-1)
    off = torch.arange(records + 1, device="cuda", dtype=torch.int64) * L
    labels = (torch.arange(records, device="cuda") < records // 2).to(torch.uint8)

    def record_best():
        with model.eval_cache():
            return model._launch_record_best(flat, off, 2)

    bits = record_best()[0]

    def test():
        return enrichment_test(bits, labels)

    def dense_amax():
        out = torch.empty((units, records), dtype=torch.float16, device="cuda")
        back = rows.flip(1)
        back = torch.where(back < 4, 3 - back, back)
        with torch.no_grad():
            for i in range(0, records, BATCH):
                f = model.linears[:3](rows[i:i + BATCH]).to(torch.float16).amax(dim=2)
                r = model.linears[:3](back[i:i + BATCH]).to(torch.float16).amax(dim=2)
                out[:, i:i + BATCH] = torch.maximum(f, r).t()
        return out

    best = test()

    def dense_fisher():
        from scipy.stats import fisher_exact
        score = bits.view(torch.float16)
        thr = best["best_pattern"].to(torch.int16).view(torch.float16)
        above = score >= thr[:, None]
        prim = labels == 1
        tp = (above & prim[None, :]).sum(dim=1).cpu().numpy()
        fp = (above & ~prim[None, :]).sum(dim=1).cpu().numpy()
        Np = int(prim.sum())
        Nc = records - Np
        return np.array([fisher_exact([[a, Np - a], [b, Nc - b]], alternative="greater")[1] for a, b in zip(tp, fp)])

    fn = {"record_best": record_best, "enrichment_test": test, "dense_amax": dense_amax,
          "dense_fisher": dense_fisher}[leg]
    res = fn()                                            # warm-up
    torch.cuda.synchronize()
    row = {"leg": leg, "units": units, "records": records, "device": torch.cuda.get_device_name(0)}
    if leg == "dense_amax":                               # the same answer, before anything is timed
        row["equal_to_kernel"] = bool(torch.equal(res.view(torch.int16), bits))
        if not row["equal_to_kernel"]:
            raise SystemExit("the dense route and record_best disagree")
    if leg == "dense_fisher":
        p = np.exp(best["log_pvalue"].cpu().numpy())
        enriched = p < 1.0                                # elsewhere the device assigns p = 1 by rule
        row["max_rel_dev"] = float(np.max(np.abs(res[enriched] - p[enriched]) / p[enriched], initial=0.0))
        row["thresholds_per_unit"] = float(best["n_thresholds"].double().mean())
        if row["max_rel_dev"] > 1e-7:
            raise SystemExit("scipy's Fisher test and enrichment_test disagree")
    ts = []
    for _ in range(passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    row.update(median_ms=float(np.median(ts)), spread_ms=float(max(ts) - min(ts)), ms=ts)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per (leg, units, records) process")
    ap.add_argument("--out", default="profiles/r22_enrichment_probe.json")
    ap.add_argument("--child", nargs=3, metavar=("LEG", "UNITS", "RECORDS"))
    args = ap.parse_args()
    if args.child:
        return _child(args.child[0], int(args.child[1]), int(args.child[2]), args.passes)
    doc = {"k": K, "L": L, "record_bases": L, "strands": "both", "passes": args.passes, "results": []}
    ok = True
    for units in UNITS:
        for records in RECORDS:
            for leg in LEGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--child", leg,
                       str(units), str(records)]
                try:
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    print("%s units %d records %d: over its limit of %d s; the probe ends here" % (
                        leg, units, records, args.limit), flush=True)
                    ok = False
                    break
                rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
                if out.returncode != 0 or not rows:
                    print("%s units %d records %d: exit %d; the probe ends here\n%s" % (
                        leg, units, records, out.returncode, out.stderr[-2000:]), flush=True)
                    ok = False
                    break
                doc.setdefault("device", rows[0].pop("device"))
                rows[0].pop("device", None)
                doc["results"].append(rows[0])
                print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rows[0].items()
                                  if k != "ms"}), flush=True)
            if not ok:
                break
        if not ok:
            break
    by = {(r["leg"], r["units"], r["records"]): r for r in doc["results"]}
    doc["device_beats_dense"] = {}
    for (leg, units, records), a in by.items():
        b = by.get((PAIRS.get(leg), units, records))
        if b:
            doc["device_beats_dense"]["%s_u%d_%d" % (PAIRS[leg], units, records)] = bool(
                a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
