#!/usr/bin/env python3
"""Times the motif tree and the merged cluster motifs (csrc/motiftree.hip) on one GPU against the route without
them: the Ncor matrix copied to the host, scipy's linkage and fcluster there, and a numpy pooling loop.
Synthetic motifs, widths 6..24: families of five copies of a base (0-2 columns cut per end, every other one
reverse-complemented), so a cut at 0.6 leaves about M/5 clusters.  M = 300, 2000, 6000.
The comparison (motifs.compare) is computed once per size and stays on the device; it is not timed.  Legs,
alternating after a warm-up of all of them, three passes by default, median, minimum and maximum of each:
  tree_kernel  explainn_motif_tree alone between device events (quantisation + the one-workgroup loop)
  cut_pool     MotifTree.cut and the pooling of motifs.merge(tree=...), wall clock, ends on the host
  merge        motifs.tree + motifs.merge(tree=...) from the device comparison, wall clock, ends on the host
  scipy        ncor.cpu(), scipy.cluster.hierarchy.linkage(average) on 1 - q / 2^20, fcluster, and a numpy loop that
               pools the clusters with the placements the device found (scipy has none); the copy is included
The sorted heights of the two trees are compared (max abs difference), and the partitions when no height is within
2^-20 of the cut.  One JSON line per size.

  motiftree_probe.py [--reps R] [--sizes 300,2000,6000] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MIN_NCOR, SCALE = 0.6, 1 << 20


def make(M, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < M:
        base = rng.dirichlet([0.3] * 4, size=int(rng.integers(10, 25))) * 20.0
        for k in range(5):
            a, e = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            m = base[a:len(base) - e] * rng.uniform(0.9, 1.1, size=(len(base) - e - a, 4))   # no two copies alike
            out.append(np.ascontiguousarray(m[::-1, ::-1]) if k % 2 else m.copy())
    return out[:M]


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def kernel_ms(res, widths, reps):
    import torch
    from explainn_amd import _lib
    lib = _lib.load()
    M = len(widths)
    ncor = res.ncor.contiguous()
    align = torch.stack([res.offset, res.strand, res.overlap], dim=-1).contiguous()
    log = torch.empty((M - 1, 8), dtype=torch.int32, device="cuda")
    link = torch.empty((M - 1, 2), dtype=torch.int64, device="cuda")
    gone, flips, shifts = (torch.empty((M,), dtype=torch.int32, device="cuda") for _ in range(3))
    nbytes = int(lib.explainn_motif_tree_workspace_bytes(M, _lib.LINKAGE_AVERAGE))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.explainn_motif_tree(ncor.data_ptr(), align.data_ptr(), widths.data_ptr(), M,
                                           _lib.LINKAGE_AVERAGE, log.data_ptr(), link.data_ptr(), gone.data_ptr(),
                                           flips.data_ptr(), shifts.data_ptr(), ws.data_ptr(), nbytes, stream))
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times[1:]


def scipy_leg(res, x, w, placement):
    """(sorted heights, labels, pooled): the host route.  placement: (flips, shifts) per leaf from the device cut."""
    import scipy.cluster.hierarchy as hier
    ncor = res.ncor.cpu().numpy()
    M = len(w)
    iu = np.triu_indices(M, 1)
    q = np.rint(ncor[iu] * np.float32(SCALE)).astype(np.float64)
    Z = hier.linkage(1.0 - q / SCALE, method="average")
    labels = hier.fcluster(Z, t=1.0 - np.ceil(MIN_NCOR * SCALE) / SCALE, criterion="distance")
    flips, shifts = placement
    uniq, first = np.unique(labels, return_index=True)                       # number the clusters as the device does:
    rank = np.empty(labels.max() + 1, dtype=np.int64)                        # in the order of their smallest member
    rank[uniq[np.argsort(first)]] = np.arange(len(uniq))
    lab = rank[labels]
    span = int((shifts + w).max())
    pooled = np.zeros((len(uniq), span, 4))
    for y in range(M):
        m = x[y, :w[y]].astype(np.float64)
        pooled[lab[y], shifts[y]:shifts[y] + w[y]] += m[::-1, ::-1] if flips[y] else m
    return 1.0 - Z[:, 2], lab, pooled


def run(M, reps):
    import torch
    from explainn_amd import motifs
    mats = make(M, M)
    xt, wt = motifs.pack(mats)
    x, w = xt.numpy(), wt.numpy().astype(np.int64)
    res = motifs.compare((xt, wt))
    wd = wt.cuda()
    tree = motifs.tree(res, wd)
    merged = motifs.merge((xt, wt), tree=tree, min_ncor=MIN_NCOR)
    placement = (merged.flips, merged.shifts.astype(np.int64))
    heights, lab, pooled = scipy_leg(res, x, w, placement)                    # warm-up, and the results to compare
    timed = {"cut_pool": lambda: motifs.merge((xt, wt), tree=tree, min_ncor=MIN_NCOR),
             "merge": lambda: motifs.merge((xt, wt), tree=motifs.tree(res, wd), min_ncor=MIN_NCOR),
             "scipy": lambda: scipy_leg(res, x, w, placement)}
    times = {k: [] for k in timed}
    for _ in range(reps):
        for k, f in timed.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    rec = {"M": M, "widths": [int(w.min()), int(w.max())], "min_ncor": MIN_NCOR, "linkage": "average", "reps": reps,
           "clusters": len(merged)}
    rec.update({k: stats(v) for k, v in times.items()})
    rec["tree_kernel"] = stats(kernel_ms(res, wd, max(reps, 3)))
    rec["tree_kernel_us_per_step"] = rec["tree_kernel"]["median_ms"] * 1e3 / max(M - 1, 1)
    diff = np.abs(np.sort(heights) - np.sort(tree.heights))                  # equal unless tied pairs share a cluster:
    rec["max_abs_height_scipy_minus_device"] = float(diff.max())             # scipy breaks ties its own way
    rec["heights_differing"] = int((diff > 1e-9).sum())
    clear = bool(np.abs(tree.heights * SCALE - np.ceil(MIN_NCOR * SCALE)).min() > 1)
    rec["cut_clear_of_heights"] = clear
    if clear:
        rec["partitions_equal"] = bool(np.array_equal(lab, merged.labels))
        rec["max_abs_pooled_scipy_minus_device"] = float(np.abs(
            pooled[:, :merged.pfm.shape[1]] - merged.pfm[:, :pooled.shape[1]]).max()) if rec["partitions_equal"] else None
    rec["scipy_over_merge"] = rec["scipy"]["median_ms"] / rec["merge"]["median_ms"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="300,2000,6000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(64, 1)                                                               # warm-up of every leg
    recs = [run(int(m), a.reps) for m in a.sizes.split(",")]
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    main()
