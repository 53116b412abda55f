#!/usr/bin/env python3
"""Time of the site q-value kernels (csrc/pwmsites.hip: pwm_hist_kernel; csrc/siteq.hip: site_q_kernel) on one
GPU, against the routes a user had before.

Histogram shapes: 300 and 2000 Dirichlet(0.3) matrices of width 6..24, 100 bins, 10^6 and 10^7 random bases
without N (the stock route below has no rule for N), both strands.  Legs (each ends synchronised):
  hist_kernel   explainn_pwm_score_histogram on device-resident codes and tables (device events)
  count_call    explainn_pwm_sites' count call (p-value 1e-4) on the same input: the same windows walked, ranked
                instead of counted -- a large multiple of it points at the LDS atomics (device events)
  torch_route   stock torch on the same GPU, what the parent commit offers: one-hot (1,4,n) fp32, per width group
                one torch.nn.functional.conv1d with the integer tables as weights (and one with the
                reverse-complemented tables), then torch.bincount of score + motif * row length; the positions go
                over in pieces of --piece starts (host clock around a synchronise).  Scores <= 8192 are exact in
                fp32.  Timed once when its warm-up pass took more than 20 s.
  scan_q        host codes and matrices -> scan_motifs(pvalue=1e-4, qvalue=0.05) -> PwmCalls on the host
  scan_p        the same without qvalue: what the histogram pass and the table add end to end
Before timing, the kernel's and the torch route's histograms are compared: they must be equal.
Table shapes: 300 x 32768 and 2000 x 2402 (obs from an exponential, p falling with ties):
  q_kernel      explainn_site_qvalues (device events)
  numpy_model   tests/siteq_model.py qtable on the host (host clock); the tables must be equal bit for bit
Every shape runs in a process of its own under its own time limit; the first one that fails or runs out of time
ends the probe.  A warm-up pass, then --passes (3) timed passes: median and spread (max - min) in ms.

usage: siteq_probe.py [--passes 3] [--limit 240] [--out profiles/r37_siteq_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MOTIFS = (300, 2000)
LENGTHS = (1000000, 10000000)
TABLES = ((300, 32768), (2000, 2402))
PVALUE, QVALUE, BINS = 1e-4, 0.05, 100


def _timed(fn, passes, np):
    first = fn()[1]                                                               # warm-up
    ts = [fn()[1] for _ in range(passes if first < 20000 else 1)]
    return {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts, "warm_up_ms": first}


def _events(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def _hist_child(M, length, passes, piece):
    import ctypes as C

    import numpy as np
    import torch

    from explainn_amd import _lib, pwmsites

    g = np.random.default_rng(M)
    widths = g.integers(6, 25, size=M)
    mats = [g.dirichlet(np.full(4, 0.3), size=int(w)).reshape(int(w), 4) for w in widths]
    codes = np.random.default_rng(0).integers(0, 4, size=length).astype(np.uint8)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = pwmsites.score_null(mats, PVALUE, None, 0.1, BINS, "cuda")
    S, live = null.scores.cpu().numpy(), null.widths.cpu().numpy()
    wmax, stride = null.wmax, null.wmax * BINS + 2
    codes_d = torch.from_numpy(codes).cuda()
    hist = torch.zeros((M, stride), dtype=torch.int64, device="cuda")

    def hist_kernel():
        hist.zero_()
        return _events(torch, lambda: _lib.check(lib.explainn_pwm_score_histogram(
            codes_d.data_ptr(), length, 0, length, 0, 1, null.scores.data_ptr(), null.widths.data_ptr(), M, wmax, BINS,
            hist.data_ptr(), stream)))

    nbytes = int(lib.explainn_pwm_sites_workspace_bytes(M, length))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    offsets = torch.empty((2 * M + 1,), dtype=torch.int64, device="cuda")

    def count_call():
        return _events(torch, lambda: _lib.check(lib.explainn_pwm_sites(
            codes_d.data_ptr(), length, 0, length, 0, 1, null.scores.data_ptr(), null.widths.data_ptr(), M, wmax,
            null.thresholds.data_ptr(), None, BINS, offsets.data_ptr(), None, None, None, 0, ws.data_ptr(), nbytes,
            stream)))

    groups = []                                            # per width: motif indices, fwd and rc weights
    for w in sorted(set(live.tolist()) - {0}):
        idx = np.flatnonzero(live == w)
        fwd = S[idx, :w].astype(np.float32).transpose(0, 2, 1)                    # (m, 4, w)
        rev = S[idx, :w][:, ::-1, ::-1].astype(np.float32).transpose(0, 2, 1)     # the table of the other strand
        groups.append((w, (torch.from_numpy(idx).cuda() * stride)[:, None],
                       torch.from_numpy(np.ascontiguousarray(fwd)).cuda(),
                       torch.from_numpy(np.ascontiguousarray(rev)).cuda()))

    def torch_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = torch.zeros((M * stride,), dtype=torch.int64, device="cuda")
        for p0 in range(0, length, piece):
            part = codes_d[p0:p0 + piece + wmax - 1].to(torch.int64)
            x = torch.nn.functional.one_hot(part, 4).to(torch.float32).T[None]    # (1, 4, n)
            for w, base, fwd, rev in groups:
                if x.shape[2] < w:
                    continue
                for weight in (fwd, rev):
                    score = torch.nn.functional.conv1d(x, weight)[0, :, :piece].to(torch.int64)
                    out += torch.bincount((score + base).reshape(-1), minlength=M * stride)
        torch.cuda.synchronize()
        return out.view(M, stride), (time.perf_counter() - t0) * 1e3

    def scan_q():
        t0 = time.perf_counter()
        calls = pwmsites.scan_motifs(mats, codes, pvalue=PVALUE, bins=BINS, qvalue=QVALUE)
        return calls, (time.perf_counter() - t0) * 1e3

    def scan_p():
        t0 = time.perf_counter()
        calls = pwmsites.scan_motifs(mats, codes, pvalue=PVALUE, bins=BINS)
        return calls, (time.perf_counter() - t0) * 1e3

    row = {"motifs": M, "bases": length, "device": torch.cuda.get_device_name(0), "row_bins": stride}
    hist_kernel()
    tests = int(hist.sum())
    row["tests"] = tests
    row["torch_route_equals_kernel"] = bool(torch.equal(torch_route()[0], hist))
    if not row["torch_route_equals_kernel"]:
        raise SystemExit("the routes disagree: %r" % row)
    row["sites_q"], row["sites_p"] = len(scan_q()[0]), len(scan_p()[0])
    row["legs"] = {name: _timed(fn, passes, np) for name, fn in (
        ("hist_kernel", hist_kernel), ("count_call", count_call), ("torch_route", torch_route), ("scan_q", scan_q),
        ("scan_p", scan_p))}
    print("ROW " + json.dumps(row), flush=True)


def _table_child(U, B, passes):
    import numpy as np
    import torch

    import siteq_model as qm
    from explainn_amd import sites

    g = np.random.default_rng(U)
    obs = np.zeros((U, B), dtype=np.int64)
    for u in range(U):
        obs[u] = np.bincount(np.minimum(g.exponential(B / 8.0, size=100000).astype(np.int64), B - 1), minlength=B)
    steps = g.random((U, B)) * (g.random((U, B)) < 0.3)
    steps[:, -1] += 0.05
    p = np.cumsum(steps[:, ::-1], axis=1)[:, ::-1]
    p = np.ascontiguousarray(p / (p[:, :1] * 2.0))
    obs_d, p_d = torch.from_numpy(obs).cuda(), torch.from_numpy(p).cuda()

    def q_kernel():
        return _events(torch, lambda: sites.site_qtable(obs_d, p_d, QVALUE))

    def numpy_model():
        t0 = time.perf_counter()
        out = qm.qtable(obs, p, QVALUE)
        return out, (time.perf_counter() - t0) * 1e3

    (q, total, first), _ = q_kernel()
    wq, wtotal, wfirst = numpy_model()[0]
    row = {"units": U, "bins": B, "device": torch.cuda.get_device_name(0),
           "kernel_equals_numpy_bits": bool(np.array_equal(q.cpu().numpy(), wq) and np.array_equal(
               total.cpu().numpy(), wtotal) and np.array_equal(first.cpu().numpy(), wfirst))}
    if not row["kernel_equals_numpy_bits"]:
        raise SystemExit("the tables differ: %r" % row)
    row["legs"] = {"q_kernel": _timed(q_kernel, passes, np), "numpy_model": _timed(numpy_model, passes, np)}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape's process")
    ap.add_argument("--piece", type=int, default=1 << 17, help="start positions per piece of the torch route")
    ap.add_argument("--out", default="profiles/r37_siteq_probe.json")
    ap.add_argument("--child", nargs=3, metavar=("KIND", "A", "B"))
    args = ap.parse_args()
    if args.child:
        kind, a, b = args.child[0], int(args.child[1]), int(args.child[2])
        return _hist_child(a, b, args.passes, args.piece) if kind == "hist" else _table_child(a, b, args.passes)
    doc = {"widths": "6..24", "strands": "both", "pvalue": PVALUE, "qvalue": QVALUE, "bins": BINS,
           "background": "uniform", "passes": args.passes, "torch_piece": args.piece, "tables": [], "histograms": []}
    shapes = [("table", u, b) for u, b in TABLES] + [("hist", m, n) for n in LENGTHS for m in MOTIFS]
    ok = True
    for kind, a, b in shapes:
        cmd = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--piece", str(args.piece),
               "--child", kind, str(a), str(b)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("%s %d %d: over its limit of %d s; the probe ends here" % (kind, a, b, args.limit), flush=True)
            ok = False
            break
        rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
        if out.returncode != 0 or not rows:
            print("%s %d %d: exit %d; the probe ends here\n%s" % (kind, a, b, out.returncode, out.stderr[-2000:]),
                  flush=True)
            ok = False
            break
        doc.setdefault("device", rows[0].pop("device"))
        rows[0].pop("device", None)
        doc["tables" if kind == "table" else "histograms"].append(rows[0])
        print(json.dumps({"kind": kind, "shape": [a, b], **{k: [round(v["median_ms"], 3), round(v["spread_ms"], 3)]
                                                            for k, v in rows[0]["legs"].items()}}), flush=True)
    doc["kernel_beats_torch"] = {}
    for r in doc["histograms"]:
        t, k = r["legs"]["torch_route"], r["legs"]["hist_kernel"]
        doc["kernel_beats_torch"]["m%d_%d" % (r["motifs"], r["bases"])] = bool(
            t["median_ms"] - k["median_ms"] > t["spread_ms"] + k["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
