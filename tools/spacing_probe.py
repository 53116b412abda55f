#!/usr/bin/env python3
"""Time of the motif-spacing histograms and their test, on one GPU, against the routes a user had before.

Site lists: a random ExplaiNN (k 19, L 200) of 300 and of 100 units, on 10^6 and 10^7 random bases, both
strands, called at null.thresholds(1e-4) of the sequence's own activation null.  max_distance 100.
Legs (each ends with its result synchronised; a leg whose result belongs on the host reads it back):
  kernel        explainn_site_spacing alone on device-resident starts and offsets, into a zeroed histogram
                (device events)
  test_kernel   explainn_spacing_test alone on that histogram (device events)
  end_to_end    host SiteCalls -> spacing() -> test(n_positions) -> total, best_distance, best_count,
                pvalue and qvalue back on the host (host clock)
  torch_route   stock torch on the same GPU: for every partner list (unit, strand) one torch.searchsorted
                pair over the starts of ALL anchor sites at once, the windows expanded with
                repeat_interleave, one torch.bincount over (anchor unit, orientation, distance) -- 2 U
                iterations, not 4 U^2: the strongest form of the searchsorted route (host clock, device
                histogram as the result)
  numpy_model   tests/spacing_model.py per_pair (np.searchsorted per list pair) on the host, timed on the
                pairs of ONE anchor unit with every partner and scaled by the number of units: "estimated"
Before timing, kernel and torch_route are compared: the histograms must be equal, and the numpy subset must
equal its rows.  Every (units, bases) runs in a process of its own under its own time limit; the first one
that fails or runs out of time ends the probe.  A warm-up pass, then --passes (3) timed passes: median and
spread (max - min) in ms.  `kernel_beats_torch`: the medians differ by more than the two spreads.

usage: spacing_probe.py [--passes 3] [--limit 300] [--out profiles/r21_spacing_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, L, T, D = 19, 200, 1, 100
UNITS = (300, 100)
LENGTHS = (1000000, 10000000)
PVALUE = 1e-4


def _child(units, length, passes):
    import ctypes as C

    import numpy as np
    import torch

    import spacing_model as sm
    from explainn_amd import ExplaiNN, _lib
    from explainn_amd.sites import activation_null, call_sites
    from explainn_amd.spacing import site_lists, spacing

    torch.manual_seed(units)
    model = ExplaiNN(units, K, L, T).cuda().eval()
    model.validate_input = False
    codes = np.random.default_rng(0).integers(0, 4, size=length).astype(np.uint8)
    thr = activation_null(model, codes).thresholds(PVALUE)
    calls = call_sites(model, codes, thr)
    n_positions = length - K + 1
    start, offsets2, _ = site_lists(calls, D)
    pos_d, off_d = torch.from_numpy(start).cuda(), torch.from_numpy(offsets2).cuda()
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = 2 * D + 1

    def kernel():
        hist = torch.zeros(units, units, 2, nb, dtype=torch.int64, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.explainn_site_spacing(pos_d.data_ptr(), off_d.data_ptr(), units, None, units, None, units, D,
                                             hist.data_ptr(), stream))
        b.record()
        b.synchronize()
        return hist, a.elapsed_time(b)

    hist_d = kernel()[0]
    outs = [torch.empty(units, units, 2, dtype=dt, device="cuda")
            for dt in (torch.int64, torch.int32, torch.int64, torch.float64)]

    def test_kernel():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _lib.check(lib.explainn_spacing_test(hist_d.data_ptr(), units, units, None, None, D, K, 10,
                                             *[o.data_ptr() for o in outs], stream))
        b.record()
        b.synchronize()
        return outs, a.elapsed_time(b)

    def end_to_end():
        t0 = time.perf_counter()
        res = spacing(calls, D).test(n_positions=n_positions)
        host = [getattr(res, f).cpu() for f in ("total", "best_distance", "best_count", "pvalue", "qvalue")]
        return host, (time.perf_counter() - t0) * 1e3

    unit_d = torch.from_numpy(calls.unit_ids()).cuda()
    strand_d = torch.from_numpy(calls.strand.astype(np.int64)).cuda()

    def torch_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hist = torch.zeros(units, units, 2, nb, dtype=torch.int64, device="cuda")
        index = torch.arange(len(pos_d), device="cuda")
        for lst in range(2 * units):
            lo, hi = int(offsets2[lst]), int(offsets2[lst + 1])
            if lo == hi:
                continue
            ys, sb = pos_d[lo:hi], 1 if lst % 2 == 0 else -1
            first = torch.searchsorted(ys, pos_d - D)
            count = torch.searchsorted(ys, pos_d + D, right=True) - first
            i = torch.repeat_interleave(index, count)
            j = first[i] + (torch.arange(len(i), device="cuda") - (torch.cumsum(count, 0) - count)[i])
            keep = (j + lo) != i                                           # a record does not meet itself
            i, j = i[keep], j[keep]
            d = (ys[j] - pos_d[i]) * strand_d[i]
            key = (unit_d[i] * 2 + (strand_d[i] != sb)) * nb + d + D
            hist[:, lst // 2] += torch.bincount(key, minlength=units * 2 * nb).view(units, 2, nb)
        torch.cuda.synchronize()
        return hist, (time.perf_counter() - t0) * 1e3

    model_anchors = [0]

    def numpy_model():
        t0 = time.perf_counter()
        h = sm.of_calls(sm.per_pair, calls, D, anchors=model_anchors)
        return h, (time.perf_counter() - t0) * 1e3 * units / len(model_anchors)

    sizes = np.diff(offsets2)
    row = {"units": units, "bases": length, "device": torch.cuda.get_device_name(0), "sites": int(len(calls)),
           "largest_list": int(sizes.max()), "pairs_counted": int(hist_d.sum())}
    got = torch_route()[0]
    row["torch_route_equals_kernel"] = bool(torch.equal(got, hist_d))
    row["numpy_subset_equals_kernel"] = bool(np.array_equal(numpy_model()[0], hist_d[model_anchors].cpu().numpy()))
    if not (row["torch_route_equals_kernel"] and row["numpy_subset_equals_kernel"]):
        raise SystemExit("the routes disagree: %r" % row)
    row["legs"] = {}
    for name, fn in (("kernel", kernel), ("test_kernel", test_kernel), ("end_to_end", end_to_end),
                     ("torch_route", torch_route), ("numpy_model", numpy_model)):
        fn()                                                               # warm-up
        ts = [fn()[1] for _ in range(passes)]
        row["legs"][name] = {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts}
    row["legs"]["numpy_model"]["estimated"] = "timed on the %d pairs of anchor unit 0, scaled by %d" % (units, units)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds per (units, bases) process")
    ap.add_argument("--out", default="profiles/r21_spacing_probe.json")
    ap.add_argument("--child", nargs=2, metavar=("UNITS", "BASES"))
    args = ap.parse_args()
    if args.child:
        return _child(int(args.child[0]), int(args.child[1]), args.passes)
    doc = {"k": K, "L": L, "strands": "both", "max_distance": D, "site_pvalue": PVALUE, "passes": args.passes,
           "results": []}
    ok = True
    for units in UNITS:
        for length in LENGTHS:
            cmd = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--child", str(units),
                   str(length)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print("units %d bases %d: over its limit of %d s; the probe ends here" % (units, length, args.limit),
                      flush=True)
                ok = False
                break
            rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not rows:
                print("units %d bases %d: exit %d; the probe ends here\n%s" % (units, length, out.returncode,
                                                                             out.stderr[-2000:]), flush=True)
                ok = False
                break
            doc.setdefault("device", rows[0].pop("device"))
            rows[0].pop("device", None)
            doc["results"].append(rows[0])
            print(json.dumps({"units": units, "bases": length, "sites": rows[0]["sites"],
                              **{k: [round(v["median_ms"], 3), round(v["spread_ms"], 3)]
                                 for k, v in rows[0]["legs"].items()}}), flush=True)
        if not ok:
            break
    doc["kernel_beats_torch"] = {}
    for r in doc["results"]:
        a, b = r["legs"]["torch_route"], r["legs"]["kernel"]
        doc["kernel_beats_torch"]["u%d_%d" % (r["units"], r["bases"])] = bool(
            a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
