#!/usr/bin/env python3
"""Time of motif centrality on one GPU: the two device entry points, the end-to-end call, and the route a user
had before them.

Random records of 200 bases, k 19, L 200 (M = 182 starts), at 100 and 300 units, 10^4 and 10^5 records, both
strands; every record is in the primary set (no control: the parent commit's route has no Fisher step to
compare).  Thresholds: per unit the median of its best activations (T = 1) or their 20 / 40 / 60 / 80 %
quantiles (T = 4).  Legs, each for T = 1 and 4 (each ends with its result synchronised):
  site_positions   explainn_site_positions alone, on record_best's device output
  centrality_test  explainn_centrality_test alone, on that histogram; centred and local (all 16652 regions)
  end_to_end       centrality(model, records, thresholds): host records -> Centrality; centred and local
  host_route       the route of the parent commit: best_sites -> RecordBest on the host -> numpy histograms ->
                   scipy.stats.binom.logsf over the same regions, the enriched-only rule and the tie rule applied
                   in numpy; centred and local.  best_sites runs for all units; the numpy / scipy part runs on the
                   first HOST_UNITS units and its time is SCALED by units / HOST_UNITS (`host_scaled`: true) --
                   the full run would take minutes at 300 units in local mode.
Before timing, the host route is compared with the device on those units: histograms, chosen threshold and
region and counts equal, log_pvalue within 1e-9 relative.  Every (units, records) runs in a process of its own
under its own time limit; the first one that fails or runs out of time ends the probe.  In a process: a
warm-up pass, then --passes (3) timed passes; a pass repeats a call until it has run for 0.2 s and reports the
time per call; median and spread (max - min) in ms.  `device_beats_host`: end_to_end against host_route, the
medians differ by more than the two spreads.  One JSON document.

usage: centrality_probe.py [--passes 3] [--limit 400] [--out profiles/r23_centrality_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, L = 19, 200
M = L - K + 1
UNITS = (100, 300)
RECORDS = (10000, 100000)
THRESHOLDS = (1, 4)
HOST_UNITS = 8
MIN_PASS_S = 0.2


def _host_test(hist, local):
    """The parent commit's route from a (units, T, 2, M) primary histogram: scipy's binomial tail over the
    regions, the enriched-only rule, the tie rule.  Returns (best_t, best_lo, best_width, sites, count, logp)."""
    import numpy as np
    from scipy.stats import binom
    if local:
        regs = [(lo, w) for w in range(1, M) for lo in range(0, M - w + 1)]
    else:
        regs = [(j, M - 2 * j) for j in range(1, M) if M - 2 * j >= 1]
    lo = np.array([r[0] for r in regs], dtype=np.int64)
    w = np.array([r[1] for r in regs], dtype=np.int64)
    out = []
    for h in hist:
        best = None
        for t in range(h.shape[0]):
            pre = np.concatenate([[0], np.cumsum(h[t, 0].astype(np.int64))])
            n = int(pre[M])
            if n < 1:
                continue
            c = pre[lo + w] - pre[lo]
            lp = np.where(c * M > n * w, binom.logsf(c - 1, n, w / M), 0.0)
            i = np.lexsort((lo, w, lp))[0]
            key = (float(lp[i]), int(w[i]), int(lo[i]), t, n, int(c[i]))
            if best is None or key[:4] < best[:4]:
                best = key
        out.append((0, 0, 0, 0, 0, 0.0) if best is None else (best[3], best[2], best[1], best[4], best[5], best[0]))
    return [np.array(x) for x in zip(*out)]


def _child(units, records, passes):
    import numpy as np
    import torch

    from explainn_amd import ExplaiNN
    from explainn_amd import centrality as ce
    from explainn_amd.enrichment import best_sites

    torch.manual_seed(units)
    model = ExplaiNN(units, K, L, 1).cuda().eval()
    model.validate_input = False
    host_rows = np.random.default_rng(0).integers(0, 4, size=(records, L)).astype(np.uint8)
    recs = list(host_rows)
    prim = recs
    flat = torch.from_numpy(host_rows).cuda().view(-1)
    off = torch.arange(records + 1, device="cuda", dtype=torch.int64) * L
    labels = torch.ones(records, device="cuda", dtype=torch.uint8)
    with model.eval_cache():
        bits, site = model._launch_record_best(flat, off, 2)
    ranked = bits.sort(dim=1)[0].view(torch.float16).float()          # the patterns sort like the values
    quant = {1: (0.5,), 4: (0.2, 0.4, 0.6, 0.8)}
    thr = {T: ranked[:, [int(x * (records - 1)) for x in q]].contiguous() for T, q in quant.items()}
    device = torch.cuda.get_device_name(0)

    def timed(fn):
        fn()                                              # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps = max(1, min(200, int(MIN_PASS_S / max(time.perf_counter() - t0, 1e-6)) + 1))
        ts = []
        for _ in range(passes):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / reps)
        return {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts, "calls_per_pass": reps}

    def emit(leg, T, mode, extra, stats):
        row = {"leg": leg, "units": units, "records": records, "T": T, "mode": mode, "device": device}
        row.update(extra)
        row.update(stats)
        print("ROW " + json.dumps(row), flush=True)

    for T in THRESHOLDS:
        hist, counts = ce.positions_device(bits, site, labels, thr[T], M)
        emit("site_positions", T, None, {}, timed(lambda: ce.positions_device(bits, site, labels, thr[T], M)))
        thr_host = thr[T].cpu().numpy()
        for local in (False, True):
            mode = "local" if local else "centred"
            dev = {f: t.cpu().numpy() for f, t in ce.test_device(hist, counts, local).items()}
            emit("centrality_test", T, mode, {"n_tests": int(dev["n_tests"].max())},
                 timed(lambda: ce.test_device(hist, counts, local)))
            emit("end_to_end", T, mode, {}, timed(lambda: ce.centrality(model, prim, thr_host, local=local)))

            # the parent commit's route, compared with the device before it is timed
            def host_best():
                return best_sites(model, prim)

            def host_rest(rb):
                sub = slice(0, HOST_UNITS)
                a = rb.score[sub].astype(np.float32)
                h = np.zeros((HOST_UNITS, T, 2, M), dtype=np.int64)
                for u in range(HOST_UNITS):
                    for t in range(T):
                        ok = (rb.start[u] >= 0) & (a[u] > thr_host[u, t])
                        h[u, t, 0] = np.bincount(rb.start[u][ok], minlength=M)
                return h, _host_test(h, local)

            rb = host_best()
            h, got = host_rest(rb)
            if not np.array_equal(h[:, :, 0], hist[:HOST_UNITS, :, 0].cpu().numpy()):
                raise SystemExit("the host histograms and explainn_site_positions disagree")
            for name, x in zip(("best_t", "best_lo", "best_width", "sites", "count"), got):
                if not np.array_equal(x, dev[name][:HOST_UNITS]):
                    raise SystemExit("the host route and explainn_centrality_test disagree on " + name)
            lp = dev["log_pvalue"][:HOST_UNITS]
            rel = float(np.max(np.abs(got[5] - lp) / np.maximum(np.abs(lp), 1e-300), initial=0.0, where=lp < 0))
            if rel > 1e-9:
                raise SystemExit("scipy's binomial tail and explainn_centrality_test disagree: %g" % rel)
            t_best = timed(host_best)
            t_rest = timed(lambda: host_rest(rb))
            scale = units / HOST_UNITS
            ms = [a + b * scale for a, b in zip(t_best["ms"], t_rest["ms"])]
            emit("host_route", T, mode,
                 {"host_scaled": True, "host_units": HOST_UNITS, "max_rel_dev_log_pvalue": rel,
                  "best_sites_ms": t_best["median_ms"], "numpy_scipy_ms_on_host_units": t_rest["median_ms"]},
                 {"median_ms": float(np.median(ms)), "spread_ms": float(max(ms) - min(ms)), "ms": ms})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds per (units, records) process")
    ap.add_argument("--out", default="profiles/r23_centrality_probe.json")
    ap.add_argument("--child", nargs=2, metavar=("UNITS", "RECORDS"))
    args = ap.parse_args()
    if args.child:
        return _child(int(args.child[0]), int(args.child[1]), args.passes)
    doc = {"k": K, "L": L, "starts": M, "strands": "both", "passes": args.passes, "host_units": HOST_UNITS,
           "geometry": "untuned first choice (256-thread histogram blocks, 512-thread test workgroups)", "results": []}
    ok = True
    for units in UNITS:
        for records in RECORDS:
            cmd = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--child", str(units),
                   str(records)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print("units %d records %d: over its limit of %d s; the probe ends here" % (units, records, args.limit),
                      flush=True)
                ok = False
                break
            rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            for row in rows:
                doc.setdefault("device", row.pop("device"))
                row.pop("device", None)
                doc["results"].append(row)
                print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if k != "ms"}),
                      flush=True)
            if out.returncode != 0 or not rows:
                print("units %d records %d: exit %d; the probe ends here\n%s" % (units, records, out.returncode,
                                                                                 out.stderr[-2000:]), flush=True)
                ok = False
                break
        if not ok:
            break
    by = {(r["leg"], r["units"], r["records"], r["T"], r["mode"]): r for r in doc["results"]}
    doc["device_beats_host"] = {}
    for (leg, units, records, T, mode), a in by.items():
        b = by.get(("end_to_end", units, records, T, mode))
        if leg == "host_route" and b:
            doc["device_beats_host"]["u%d_%d_T%d_%s" % (units, records, T, mode)] = bool(
                a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
