#!/usr/bin/env python3
"""Time of the known-motif scan (csrc/pwmsites.hip) on one GPU, against the routes a user had before.

Motifs: 300 and 2000 Dirichlet(0.3) matrices of width 6..24; sequence: 10^6 and 10^7 random bases without N
(the stock route below has no rule for N); both strands, p-value 1e-4, uniform background, 100 bins.
Legs (each ends with its result synchronised; a leg whose result belongs on the host reads it back):
  null_kernel   the upload of the integer tables and explainn_pwm_null: tails and thresholds of all motifs
                (device events)
  scan_kernels  explainn_pwm_sites on device-resident codes and tables: the count call and the emit call into
                buffers of the known size -- two count passes, four scans, one emit pass (device events)
  end_to_end    host codes and matrices -> scan_motifs() -> PwmCalls on the host (host clock)
  torch_route   stock torch on the same GPU, what the parent commit offers: one-hot (1,4,n) fp32, per width
                group one torch.nn.functional.conv1d with the integer tables as weights (and one with the
                reverse-complemented tables), `>= threshold`, torch.nonzero; the positions go over in pieces
                of --piece starts so that a group's (motifs, piece) score array stays small (host clock,
                device lists as the result).  Scores <= 8192 are exact in fp32.
  numpy_model   tests/pwmsites_model.py scan on the host, timed on FOUR motifs and at most 10^6 bases and
                scaled to the shape: "estimated"
Before timing the kernel's and the torch route's hits are compared as sorted (row, position) lists: they must
be equal.  Every (motifs, bases) runs in a process of its own under its own time limit; the first one that
fails or runs out of time ends the probe.  A warm-up pass, then --passes (3) timed passes: median and spread
(max - min) in ms.  `kernel_beats_torch`: the medians differ by more than the two spreads.

usage: pwmsites_probe.py [--passes 3] [--limit 240] [--out profiles/r26_pwmsites_probe.json]"""
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
PVALUE, BINS = 1e-4, 100


def _child(M, length, passes, piece):
    import ctypes as C

    import numpy as np
    import torch

    import pwmsites_model as pm
    from explainn_amd import _lib, pwmsites

    g = np.random.default_rng(M)
    widths = g.integers(6, 25, size=M)
    mats = [g.dirichlet(np.full(4, 0.3), size=int(w)).reshape(int(w), 4) for w in widths]
    codes = np.random.default_rng(0).integers(0, 4, size=length).astype(np.uint8)
    lib = _lib.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bg = np.full(4, 0.25)
    S, w32, scale, lo = pwmsites.quantise(mats, bg, 0.1, BINS)
    wmax = S.shape[1]
    live = np.where(scale > 0, w32, 0).astype(np.int32)

    def null_kernel():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        null = pwmsites._null(S, live, scale, lo, BINS, bg, PVALUE, torch.device("cuda", 0))
        b.record()
        b.synchronize()
        return null, a.elapsed_time(b)

    null = null_kernel()[0]
    codes_d = torch.from_numpy(codes).cuda()
    nbytes = int(lib.explainn_pwm_sites_workspace_bytes(M, length))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    offsets = torch.empty((2 * M + 1,), dtype=torch.int64, device="cuda")

    def call(pos, score, pv, cap):
        _lib.check(lib.explainn_pwm_sites(codes_d.data_ptr(), length, 0, length, 0, 1, null.scores.data_ptr(),
                                          null.widths.data_ptr(), M, wmax, null.thresholds.data_ptr(),
                                          null.tail.data_ptr(), BINS, offsets.data_ptr(), pos, score, pv, cap,
                                          ws.data_ptr(), nbytes, stream))

    call(None, None, None, 0)
    total = int(offsets[-1])
    pos = torch.empty((total,), dtype=torch.int32, device="cuda")
    isc = torch.empty((total,), dtype=torch.int32, device="cuda")
    pv = torch.empty((total,), dtype=torch.float64, device="cuda")

    def scan_kernels():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call(None, None, None, 0)
        call(pos.data_ptr(), isc.data_ptr(), pv.data_ptr(), total)
        b.record()
        b.synchronize()
        return (offsets, pos), a.elapsed_time(b)

    def end_to_end():
        t0 = time.perf_counter()
        calls = pwmsites.scan_motifs(mats, codes, pvalue=PVALUE, bins=BINS)
        return calls, (time.perf_counter() - t0) * 1e3

    thr_h = null.thresholds.cpu().numpy()
    groups = []                                            # per width: motif indices, fwd and rc weights, thresholds
    for w in sorted(set(live.tolist()) - {0}):
        idx = np.flatnonzero(live == w)
        fwd = S[idx, :w].astype(np.float32).transpose(0, 2, 1)                    # (m, 4, w)
        rev = S[idx, :w][:, ::-1, ::-1].astype(np.float32).transpose(0, 2, 1)     # the table of the other strand
        groups.append((w, torch.from_numpy(idx).cuda(), torch.from_numpy(np.ascontiguousarray(fwd)).cuda(),
                       torch.from_numpy(np.ascontiguousarray(rev)).cuda(),
                       torch.from_numpy(thr_h[idx].astype(np.float32)).cuda()[None, :, None]))

    def torch_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows, where = [], []
        for p0 in range(0, length, piece):
            part = codes_d[p0:p0 + piece + wmax - 1].to(torch.int64)
            x = torch.nn.functional.one_hot(part, 4).to(torch.float32).T[None]    # (1, 4, n)
            for w, idx, fwd, rev, thr in groups:
                if x.shape[2] < w:
                    continue
                for strand, weight in ((0, fwd), (1, rev)):
                    hit = torch.nonzero(torch.nn.functional.conv1d(x, weight)[:, :, :piece] >= thr)
                    rows.append(2 * idx[hit[:, 1]] + strand)
                    where.append(hit[:, 2] + p0)
        rows, where = torch.cat(rows), torch.cat(where)
        torch.cuda.synchronize()
        return (rows, where), (time.perf_counter() - t0) * 1e3

    sub, sub_len = list(range(4)), min(length, 1000000)

    def numpy_model():
        t0 = time.perf_counter()
        out = pm.scan(S[sub], live[sub], thr_h[sub], codes[:sub_len])
        return out, (time.perf_counter() - t0) * 1e3 * (M / len(sub)) * (length / sub_len)

    row = {"motifs": M, "bases": length, "device": torch.cuda.get_device_name(0), "sites": total,
           "workspace_bytes": nbytes}
    (off_k, pos_k), _ = scan_kernels()
    rows_k = torch.repeat_interleave(torch.arange(2 * M, device="cuda"), off_k[1:] - off_k[:-1])
    key_k = rows_k * length + pos_k.to(torch.int64)                               # already ascending
    (rows_t, where_t), _ = torch_route()
    key_t = torch.sort(rows_t * length + where_t).values
    row["torch_route_equals_kernel"] = bool(torch.equal(key_k, key_t))
    off_m, pos_m, _ = numpy_model()[0]
    want = [pos_k[int(off_k[r]):int(off_k[r + 1])].cpu().numpy() for r in range(2 * len(sub))]
    row["numpy_subset_equals_kernel"] = bool(sub_len < length or all(
        np.array_equal(pos_m[off_m[r]:off_m[r + 1]], want[r]) for r in range(2 * len(sub))))
    if not (row["torch_route_equals_kernel"] and row["numpy_subset_equals_kernel"]):
        raise SystemExit("the routes disagree: %r" % row)
    row["legs"] = {}
    for name, fn in (("null_kernel", null_kernel), ("scan_kernels", scan_kernels), ("end_to_end", end_to_end),
                     ("torch_route", torch_route), ("numpy_model", numpy_model)):
        fn()                                                                      # warm-up
        ts = [fn()[1] for _ in range(passes)]
        row["legs"][name] = {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts}
    row["legs"]["numpy_model"]["estimated"] = "timed on %d motifs and %d bases, scaled to the shape" % (len(sub), sub_len)
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per (motifs, bases) process")
    ap.add_argument("--piece", type=int, default=1 << 17, help="start positions per piece of the torch route")
    ap.add_argument("--out", default="profiles/r26_pwmsites_probe.json")
    ap.add_argument("--child", nargs=2, metavar=("MOTIFS", "BASES"))
    args = ap.parse_args()
    if args.child:
        return _child(int(args.child[0]), int(args.child[1]), args.passes, args.piece)
    doc = {"widths": "6..24", "strands": "both", "pvalue": PVALUE, "bins": BINS, "background": "uniform",
           "passes": args.passes, "torch_piece": args.piece, "results": []}
    ok = True
    for M in MOTIFS:
        for length in LENGTHS:
            cmd = [sys.executable, os.path.abspath(__file__), "--passes", str(args.passes), "--piece", str(args.piece),
                   "--child", str(M), str(length)]
            try:
                out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print("motifs %d bases %d: over its limit of %d s; the probe ends here" % (M, length, args.limit),
                      flush=True)
                ok = False
                break
            rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not rows:
                print("motifs %d bases %d: exit %d; the probe ends here\n%s" % (M, length, out.returncode,
                                                                              out.stderr[-2000:]), flush=True)
                ok = False
                break
            doc.setdefault("device", rows[0].pop("device"))
            rows[0].pop("device", None)
            doc["results"].append(rows[0])
            print(json.dumps({"motifs": M, "bases": length, "sites": rows[0]["sites"],
                              **{k: [round(v["median_ms"], 3), round(v["spread_ms"], 3)]
                                 for k, v in rows[0]["legs"].items()}}), flush=True)
        if not ok:
            break
    doc["kernel_beats_torch"] = {}
    for r in doc["results"]:
        a, b = r["legs"]["torch_route"], r["legs"]["scan_kernels"]
        doc["kernel_beats_torch"]["m%d_%d" % (r["motifs"], r["bases"])] = bool(
            a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
