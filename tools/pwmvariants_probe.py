#!/usr/bin/env python3
"""Time of variant effects on known motifs (csrc/pwmvariants.hip, explainn_amd/pwmvariants.py) on one GPU, against
the route a user had before.

Motifs: 300 and 2000 Dirichlet(0.3) matrices of width 6..24; variants: 10^4 and 10^5 on a random sequence of 10^7
bases without N, 90 % SNVs and 10 % indels / replacements with alleles of at most 10 bases; both strands, uniform
background, 100 bins, p = 1e-4.  The variants go over in the chunks motif_variants itself would use (dense
(M, chunk, 2) outputs under pwmvariants.OUTPUT_BYTES).
Legs (each ends with its result synchronised):
  kernel          explainn_pwm_variant_best on device-resident codes, edit table and score tables, chunk by chunk
                  into buffers allocated beforehand: bits and sites of every (motif, variant, allele) (device events
                  around all the chunks)
  motif_variants  host codes, host variant lists and matrices -> motif_variants(keep="hits") -> result on the host
                  (host clock)
  record_route    what the parent commit offers for the kernel's job, on the same GPU and the same device-resident
                  tables: per chunk and per width group w, one torch gather that splices the 2 w - 2 + l bases
                  around both alleles of every variant into records of one stride (N where the haplotype ends and
                  behind the record), then explainn_pwm_record_best on the group's motifs, scattered into the same
                  dense outputs (host clock around all the chunks, ending in a synchronise)
Before timing the two routes' bits and sites are compared on every chunk: they must be equal.  Every (motifs,
variants) runs in a process of its own under its own time limit; the first one that fails or runs out of time ends
the probe.  A warm-up pass, then --passes (3) timed passes: median and spread (max - min) in ms.
`kernel_beats_route`: the medians differ by more than the two spreads.

usage: pwmvariants_probe.py [--passes 3] [--limit 240] [--out profiles/r38_pwmvariants_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MOTIFS = (300, 2000)
VARIANTS = (10000, 100000)
BASES, PVALUE, BINS, MAX_INDEL = 10 ** 7, 1e-4, 100, 10


def _child(M, V, passes):
    import numpy as np
    import torch

    from explainn_amd import _lib, pwmenrich, pwmsites, pwmvariants
    from explainn_amd.variants import build_tables

    g = np.random.default_rng(M)
    widths = g.integers(6, 25, size=M)
    mats = [g.dirichlet(np.full(4, 0.3), size=int(w)).reshape(int(w), 4) for w in widths]
    motifs = [("m%d" % i, "m%d" % i, m) for i, m in enumerate(mats)]
    g = np.random.default_rng(V)
    codes = g.integers(0, 4, size=BASES).astype(np.uint8)
    snv = g.random(V) < 0.9
    ref_len = np.where(snv, 1, g.integers(0, MAX_INDEL + 1, size=V))
    alt_len = np.where(snv, 1, g.integers(0, MAX_INDEL + 1, size=V))
    pos = g.integers(0, BASES - MAX_INDEL, size=V)
    alts = [g.integers(0, 4, size=int(n)).astype(np.uint8) for n in alt_len]
    # trim=False below: the tables of both routes are these, as drawn
    tab = build_tables(pos, ref_len, alts, 0)
    S, w32, scale, lo = pwmsites.quantise(mats, np.full(4, 0.25), 0.1, BINS)
    live = np.where(scale > 0, w32, 0).astype(np.int32)
    wmax = S.shape[1]
    dev = torch.device("cuda", 0)
    scores, wd = torch.from_numpy(S).cuda(), torch.from_numpy(live).cuda()
    seq = torch.from_numpy(codes).cuda()
    edits = {k: torch.from_numpy(tab[k]).cuda() for k in ("pos", "ref_len", "alt_len", "alt_off", "alt")}
    chunk = max(1, pwmvariants.OUTPUT_BYTES // (12 * M))
    spans = [(v0, min(v0 + chunk, V)) for v0 in range(0, V, chunk)]
    cmax = max(b - a for a, b in spans)
    bits_k = torch.empty((M, cmax, 2), dtype=torch.int16, device=dev)
    site_k = torch.empty((M, cmax, 2), dtype=torch.int32, device=dev)
    bits_r, site_r = torch.empty_like(bits_k), torch.empty_like(site_k)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)

    def launch(a, b):
        """The kernel on variants [a, b) into the first b - a columns' worth of the flat buffers."""
        n = b - a
        _lib.call("explainn_pwm_variant_best", dev, seq, BASES, edits["pos"][a:b], edits["ref_len"][a:b],
                  edits["alt_len"][a:b], edits["alt_off"][a:b], edits["alt"], edits["alt"].shape[0], n, 1, scores, wd, M,
                  wmax, bits_k, site_k, flags)
        return bits_k.view(-1)[:M * n * 2].view(M, n, 2), site_k.view(-1)[:M * n * 2].view(M, n, 2)

    def kernel():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for v0, v1 in spans:
            launch(v0, v1)
        b.record()
        b.synchronize()
        return None, a.elapsed_time(b)

    groups = [(w, torch.from_numpy(np.flatnonzero(live == w)).cuda()) for w in sorted(set(live.tolist()) - {0})]
    tables = {w: (scores[idx].contiguous(), wd[idx].contiguous()) for w, idx in groups}
    source = torch.cat([seq, edits["alt"], torch.full((1,), 4, dtype=torch.uint8, device=dev)])   # the last byte: N
    n_at = BASES + edits["alt"].shape[0]

    def route_chunk(a, b):
        n = b - a
        p, rl = edits["pos"][a:b, None, None], edits["ref_len"][a:b, None, None].to(torch.int64)
        al, ao = edits["alt_len"][a:b, None, None].to(torch.int64), edits["alt_off"][a:b, None, None].to(torch.int64)
        l = torch.cat([rl, al], dim=1)                                            # (n, 2, 1)
        out_b, out_s = bits_r.view(-1)[:M * n * 2].view(M, n, 2), site_r.view(-1)[:M * n * 2].view(M, n, 2)
        for w, idx in groups:
            stride = 2 * w - 2 + MAX_INDEL
            t = torch.arange(stride, device=dev)[None, None, :]
            h = p - w + 1 + t                                                     # haplotype coordinate (n, 2, stride)
            inside = (t < l + 2 * w - 2) & (h >= 0) & (h < BASES - rl + l)
            in_allele = (h >= p) & (h < p + l)
            src = torch.where(h < p, h, h - l + rl)                               # seq on either side of the allele
            own = torch.cat([h[:, :1].expand(-1, 1, -1), (BASES + ao + h - p)[:, :1]], dim=1)      # ref: seq; alt: the pool
            at = torch.where(inside, torch.where(in_allele, own, src), torch.full_like(h, n_at))
            records = source[at.reshape(-1)]
            off = torch.arange(2 * n + 1, device=dev, dtype=torch.int64) * stride
            sc, wl = tables[w]
            bb, ss = pwmenrich.record_best_device(sc, wl, records, off, True, True)
            out_b[idx] = bb.view(len(idx), n, 2)
            out_s[idx] = ss.view(len(idx), n, 2)
        return out_b, out_s

    def record_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for v0, v1 in spans:
            route_chunk(v0, v1)
        torch.cuda.synchronize()
        return None, (time.perf_counter() - t0) * 1e3

    def motif_variants():
        t0 = time.perf_counter()
        res = pwmvariants.motif_variants(motifs, codes, pos, ref_len, alts, pvalue=PVALUE, bins=BINS, trim=False)
        return res, (time.perf_counter() - t0) * 1e3

    row = {"motifs": M, "variants": V, "bases": BASES, "chunk_variants": chunk, "device": torch.cuda.get_device_name(0)}
    same = True
    for v0, v1 in spans:
        kb, ks = launch(v0, v1)
        rb, rs = route_chunk(v0, v1)
        same = same and bool(torch.equal(kb, rb)) and bool(torch.equal(ks, rs))
    row["record_route_equals_kernel"] = same
    row["flags"] = int(flags.item())
    if not same or row["flags"]:
        raise SystemExit("the routes disagree or a flag is raised: %r" % row)
    row["legs"] = {}
    for name, fn in (("kernel", kernel), ("record_route", record_route), ("motif_variants", motif_variants)):
        res = fn()[0]                                                             # warm-up
        if name == "motif_variants":
            row["hits"] = len(res)
        ts = [fn()[1] for _ in range(passes)]
        row["legs"][name] = {"median_ms": float(np.median(ts)), "spread_ms": float(max(ts) - min(ts)), "ms": ts}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per (motifs, variants) process")
    ap.add_argument("--out", default="profiles/r38_pwmvariants_probe.json")
    ap.add_argument("--child", nargs=2, metavar=("MOTIFS", "VARIANTS"))
    args = ap.parse_args()
    if args.child:
        return _child(int(args.child[0]), int(args.child[1]), args.passes)
    doc = {"widths": "6..24", "strands": "both", "pvalue": PVALUE, "bins": BINS, "background": "uniform",
           "sequence_bases": BASES, "snv_fraction": 0.9, "max_indel": MAX_INDEL, "passes": args.passes, "results": []}
    ok = True
    for M in MOTIFS:
        for V in VARIANTS:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--passes",
                   str(args.passes), "--child", str(M), str(V)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not rows:
                print("motifs %d variants %d: exit %d (124 / 137: over its limit of %d s); the probe ends here\n%s" % (
                    M, V, out.returncode, args.limit, out.stderr[-2000:]), flush=True)
                ok = False
                break
            doc.setdefault("device", rows[0].pop("device"))
            rows[0].pop("device", None)
            doc["results"].append(rows[0])
            print(json.dumps({"motifs": M, "variants": V, **{k: [round(v["median_ms"], 3), round(v["spread_ms"], 3)]
                                                             for k, v in rows[0]["legs"].items()}}), flush=True)
        if not ok:
            break
    doc["kernel_beats_route"] = {}
    for r in doc["results"]:
        a, b = r["legs"]["record_route"], r["legs"]["kernel"]
        doc["kernel_beats_route"]["m%d_v%d" % (r["motifs"], r["variants"])] = bool(
            a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
