#!/usr/bin/env python3
"""Time to build the empirical null of every filter's activation, on one GPU: the histogram kernel, the
Python route around it, and the route a user had before it existed.

Device-resident random base codes, k 19, L 200, at 300 and 100 units, 10^6 and 10^7 bases, both strands.
Legs (each ends with its result synchronised; where a leg's result lives on the host it is read back):
  kernel          explainn_activation_histogram alone: one call per strand into a zeroed histogram
  null_sequence   sites.activation_null(model, codes): chunks, both strands, tails and totals, the NaN check
  null_shuffle10  sites.activation_null(model, (N,200) rows, shuffles=10): ten dinucleotide shuffles of every
                  row drawn on the device and counted instead -- ten times the k-mers of null_sequence
  dense_bincount  the route of the parent commit: windows at stride Lo = L - k + 1 cut on the device ->
                  model.linears[:3] -> float16 -> bit patterns -> torch.bincount per unit (one bincount over
                  unit-offset indices, which is the per-unit count in one call) on the same GPU
Every (leg, units, length) runs in a process of its own under its own time limit; the first one that
fails or runs out of time ends the probe.  In a process: a warm-up pass, then --passes (3) timed passes;
median and spread (max - min) in ms.  Before timing, kernel, null_sequence and dense_bincount are
compared: the three histograms must be equal.  `kernel_beats_dense`: the medians differ by more than the
two spreads.  One JSON document.

usage: actnull_probe.py [--passes 3] [--limit 240] [--out profiles/r20_actnull_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, L, T = 19, 200, 1
LO = L - K + 1
UNITS = (300, 100)
LENGTHS = (1000000, 10000000)
LEGS = ("kernel", "null_sequence", "null_shuffle10", "dense_bincount")
BATCH = 512                      # windows per linears[:3] call: 512 x 300 x 182 fp32 = 112 MB
BINS = 32768


def _child(leg, units, length, passes):
    import numpy as np
    import torch

    from explainn_amd import ExplaiNN
    from explainn_amd.sites import activation_null

    torch.manual_seed(units)
    model = ExplaiNN(units, K, L, T).cuda().eval()
    model.validate_input = False
    length -= length % L                                  # whole rows for the shuffle leg
    seq_d = torch.from_numpy(np.random.default_rng(0).integers(0, 4, size=length).astype(np.uint8)).cuda()

    def rc(s):
        r = s.flip(0)
        return torch.where(r < 4, 3 - r, r)

    def kernel():
        hist = torch.zeros(units, BINS, dtype=torch.int64, device="cuda")
        with model.eval_cache():
            model._launch_activation_histogram(seq_d, hist)
            model._launch_activation_histogram(seq_d, hist, reverse_complement=True)
        return hist

    def null_sequence():
        return activation_null(model, seq_d).hist

    def null_shuffle10():
        return activation_null(model, seq_d.view(-1, L), shuffles=10).hist

    def dense_bincount():
        hist = torch.zeros(units * BINS, dtype=torch.int64, device="cuda")
        offs = (torch.arange(units, device="cuda", dtype=torch.int64) * BINS)[None, :, None]
        n_pos = length - K + 1
        for s in (seq_d, rc(seq_d)):
            starts = torch.arange(0, length - L + 1, LO, device="cuda")
            if int(starts[-1]) != length - L:
                starts = torch.cat([starts, torch.tensor([length - L], device="cuda")])
            # the last window is pulled back to the sequence's end: its first offsets repeat the one before
            dup = int(starts[-2]) + LO - int(starts[-1]) if len(starts) > 1 else 0
            with torch.no_grad():
                for i in range(0, len(starts), BATCH):
                    st = starts[i:i + BATCH]
                    win = s[st[:, None] + torch.arange(L, device="cuda")[None, :]]
                    bits = model.linears[:3](win).to(torch.float16).view(torch.int16).to(torch.int64) & 0x7FFF
                    bits = bits + offs
                    if i + BATCH >= len(starts) and dup > 0:
                        hist += torch.bincount(bits[:-1].reshape(-1), minlength=units * BINS)
                        hist += torch.bincount(bits[-1][:, dup:].reshape(-1), minlength=units * BINS)
                    else:
                        hist += torch.bincount(bits.reshape(-1), minlength=units * BINS)
        assert int(hist[:BINS].sum()) == 2 * n_pos
        return hist.view(units, BINS)

    fns = {"kernel": kernel, "null_sequence": null_sequence, "null_shuffle10": null_shuffle10,
           "dense_bincount": dense_bincount}
    fn = fns[leg]
    res = fn()                                            # warm-up
    torch.cuda.synchronize()
    row = {"leg": leg, "units": units, "bases": length, "device": torch.cuda.get_device_name(0),
           "counted_per_unit": int(res[0].sum())}
    if leg == "dense_bincount":                           # the same answer, before anything is timed
        row["equal_to_kernel"] = bool(torch.equal(res, kernel()) and torch.equal(res, null_sequence()))
        if not row["equal_to_kernel"]:
            raise SystemExit("the dense route and the kernel disagree")
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
    ap.add_argument("--limit", type=int, default=240, help="seconds per (leg, units, length) process")
    ap.add_argument("--out", default="profiles/r20_actnull_probe.json")
    ap.add_argument("--child", nargs=3, metavar=("LEG", "UNITS", "BASES"))
    args = ap.parse_args()
    if args.child:
        return _child(args.child[0], int(args.child[1]), int(args.child[2]), args.passes)
    doc = {"k": K, "L": L, "strands": "both", "passes": args.passes, "results": []}
    ok = True
    for units in UNITS:
        for length in LENGTHS:
            for leg in LEGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--child", leg,
                       str(units), str(length)]
                try:
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
                except subprocess.TimeoutExpired:
                    print("%s units %d bases %d: over its limit of %d s; the probe ends here" % (
                        leg, units, length, args.limit), flush=True)
                    ok = False
                    break
                rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
                if out.returncode != 0 or not rows:
                    print("%s units %d bases %d: exit %d; the probe ends here\n%s" % (
                        leg, units, length, out.returncode, out.stderr[-2000:]), flush=True)
                    ok = False
                    break
                doc.setdefault("device", rows[0].pop("device"))
                rows[0].pop("device", None)
                doc["results"].append(rows[0])
                print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in rows[0].items()
                                  if k != "ms"}), flush=True)
            if not ok:
                break
        if not ok:
            break
    by = {(r["leg"], r["units"], r["bases"]): r for r in doc["results"]}
    doc["kernel_beats_dense"] = {}
    for (leg, units, bases), a in by.items():
        b = by.get(("kernel", units, bases))
        if leg == "dense_bincount" and b:
            doc["kernel_beats_dense"]["u%d_%d" % (units, bases)] = bool(
                a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
