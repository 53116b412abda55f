#!/usr/bin/env python3
"""Time of de novo word discovery (csrc/words.hip, explainn_amd/discover.py) on one GPU, against the route a user
had before.

Records: 10^4 and 10^5 primary records of 200 random bases, GATAAGCC planted in 30 % of them on a random strand, and
as many dinucleotide-shuffled controls (drawn on the device); both strands; widths 6, 7, 8 and 10.
Legs:
  counts        explainn_word_counts on the device-resident primary set into a zeroed table, per width (device
                events around REPS calls, divided by REPS)
  test          explainn_word_test on the two tables of that width (the same)
  torch_route   what the parent commit offers for the count kernel's job, on the same GPU and the same
                device-resident rows: torch unfold -> packed codes -> canonical -> unique of (record, code) ->
                bincount (host clock around one call that ends in a synchronise)
  discover      host records -> discover(control=None, widths=(6, 7, 8)) -> Discovery on the host, end to end
                (host clock)
Before anything is timed the kernel's and the route's tables are compared at every width: they must be equal.
Every record count runs in a process of its own under its own time limit; the first one that fails or runs out
of time ends the probe.  A warm-up pass, then --passes (3) timed passes: median and spread (max - min) in ms.
`kernel_beats_route`: the medians differ by more than the two spreads.

usage: discover_probe.py [--passes 3] [--limit 300] [--out profiles/r39_discover_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECORDS = (10000, 100000)
LENGTH, WIDTHS, LOOP_WIDTHS, PLANT, RATE, REPS = 200, (6, 7, 8, 10), (6, 7, 8), "GATAAGCC", 0.3, 20


def _child(R, passes):
    import numpy as np
    import torch

    from explainn_amd import discover as dv
    from explainn_amd.sequence import dinucleotide_shuffle_device

    g = np.random.default_rng(R)
    rows = g.integers(0, 4, size=(R, LENGTH)).astype(np.uint8)
    plant = np.array(["ACGT".index(ch) for ch in PLANT], dtype=np.uint8)
    for r in np.flatnonzero(g.random(R) < RATE):
        at = int(g.integers(0, LENGTH - len(plant) + 1))
        rows[r, at:at + len(plant)] = plant if g.random() < 0.5 else (3 - plant)[::-1]
    dev = torch.device("cuda", 0)
    prim = torch.from_numpy(rows).cuda()
    ctrl = dinucleotide_shuffle_device(prim, 1, 0).reshape(R, LENGTH)
    off = torch.arange(R + 1, dtype=torch.int64, device=dev) * LENGTH
    p_seq, c_seq = prim.reshape(-1), ctrl.reshape(-1).contiguous()

    def torch_counts(x, k):
        win = x.unfold(1, k, 1).to(torch.int64)                                   # (R, starts, k)
        pw = 4 ** torch.arange(k - 1, -1, -1, device=dev, dtype=torch.int64)
        code = torch.minimum((win * pw).sum(-1), ((3 - win) * pw.flip(0)).sum(-1))
        key = (torch.arange(R, device=dev)[:, None] * 4 ** k + code)[(win < 4).all(-1)]
        return torch.bincount(torch.unique(key) % 4 ** k, minlength=4 ** k).to(torch.int32)

    row = {"records": R, "length": LENGTH, "device": torch.cuda.get_device_name(0), "widths": {}}
    tables = {}
    for k in WIDTHS:
        pos, neg = dv.word_counts(p_seq, off, k), dv.word_counts(c_seq, off, k)
        if not (torch.equal(pos, torch_counts(prim, k)) and torch.equal(neg, torch_counts(ctrl, k))):
            raise SystemExit("width %d: the kernel's table and the torch route's differ" % k)
        tables[k] = (pos, neg)
    row["torch_route_equals_kernel"] = True

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / REPS

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def timed(fn):
        fn()                                                                      # warm-up
        ts = [fn() for _ in range(passes)]
        return {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts}

    for k in WIDTHS:
        out = torch.zeros(4 ** k, dtype=torch.int32, device=dev)
        pos, neg = tables[k]
        legs = {"counts": timed(lambda: events(lambda: dv.word_counts(p_seq, off, k, out=out))),
                "test": timed(lambda: events(lambda: dv.word_test(pos, neg, R, R, 5))),
                "torch_route": timed(lambda: clock(lambda: torch_counts(prim, k))[1])}
        legs["kernel_beats_route"] = bool(legs["torch_route"]["median_ms"] - legs["counts"]["median_ms"] >
                                          legs["torch_route"]["spread_ms"] + legs["counts"]["spread_ms"])
        row["widths"][str(k)] = legs
    records = list(rows)
    found = {}

    def loop():
        res, ms = clock(lambda: dv.discover(records, None, shuffles=1, seed=0, widths=LOOP_WIDTHS))
        found["res"] = res
        return ms

    row["discover"] = timed(loop)
    res = found["res"]
    row["discover"].update(motifs=len(res), first_word=res.word[0] if len(res) else None,
                           first_log_pvalue=float(res.log_pvalue[0]) if len(res) else None, flags=res.flags)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per record count's process")
    ap.add_argument("--out", default="profiles/r39_discover_probe.json")
    ap.add_argument("--child", type=int, metavar="RECORDS")
    args = ap.parse_args()
    if args.child:
        return _child(args.child, args.passes)
    doc = {"length": LENGTH, "widths": list(WIDTHS), "loop_widths": list(LOOP_WIDTHS), "strands": "both", "plant": PLANT,
           "plant_rate": RATE, "reps_per_event_window": REPS, "passes": args.passes, "results": []}
    ok = True
    for R in RECORDS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--passes",
               str(args.passes), "--child", str(R)]
        out = subprocess.run(cmd, capture_output=True, text=True)
        rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
        if out.returncode != 0 or not rows:
            print("records %d: exit %d (124 / 137: over its limit of %d s); the probe ends here\n%s" % (
                R, out.returncode, args.limit, out.stderr[-2000:]), flush=True)
            ok = False
            break
        doc.setdefault("device", rows[0].pop("device"))
        rows[0].pop("device", None)
        doc["results"].append(rows[0])
        print(json.dumps({"records": R, "discover": [round(rows[0]["discover"][f], 3) for f in ("median_ms", "spread_ms")],
                          **{k: {leg: round(v[leg]["median_ms"], 4) for leg in ("counts", "test", "torch_route")}
                             for k, v in rows[0]["widths"].items()}}), flush=True)
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
