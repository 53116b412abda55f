#!/usr/bin/env python3
"""Times motif significance (csrc/motifs.hip, explainn_motif_significance) on one GPU.  The synthetic
Dirichlet motifs and the two shapes of tools/motifs_probe.py:
  annotate  300 x 2000, widths 6..24, wmax 24   (one model's filters against a JASPAR-sized set)
  bank      2000 x 2000, width 19               (the filters of a model bank against themselves)
After a warm-up of every leg, three passes by default; median, minimum and maximum of each:
  device         motifs.significance from host-resident packed motifs to host-resident p- and q-values (both
                 copies, the workspace allocation and the torch q-value step included)
  device_kernel  explainn_motif_significance alone between device events, inputs, outputs and workspace
                 resident, one call per query chunk of the default workspace budget
  stages         the kernels of one such pass by name, from torch.profiler's device activity (absent when the
                 profiler reports no kernels)
  numpy_scaled   tests/motifsig_model.py (fp64 numpy) on the first `--model-queries` queries against the whole
                 database, its time multiplied by Q / that number: an estimate, labelled as one
The model's p-values on that subset are compared with the device's (the model rounds its own column scores, so
a pair whose null holds a column score that rounds the other way differs; the share of pairs within 1e-9
relative is reported beside the largest difference).  One JSON line per shape.

  motifsig_probe.py [--reps R] [--shapes annotate,bank] [--bins B] [--model-queries N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from motifs_probe import MIN_OVERLAP, SHAPES, make, stats  # noqa: E402

BUDGET = 512 << 20


def device_leg(q, qw, t, tw, bins):
    import torch
    from explainn_amd import motifs
    res = motifs.significance((torch.from_numpy(q), torch.from_numpy(qw)), (torch.from_numpy(t), torch.from_numpy(tw)),
                              min_overlap=MIN_OVERLAP, bins=bins, workspace_bytes=BUDGET)
    return res.pvalue.cpu().numpy(), res.qvalue.cpu().numpy()


class Resident:
    """Everything of the kernel leg on the device: one call per query chunk."""

    def __init__(self, q, qw, t, tw, bins):
        import torch
        from explainn_amd import _lib, motifs
        self.lib, self._lib, self.torch = _lib.load(), _lib, torch
        self.Q, self.T, self.wmax, self.bins = len(q), len(t), q.shape[1], bins
        self.q, self.qw, self.t, self.tw = (torch.from_numpy(a).cuda() for a in (q, qw, t, tw))
        self.p = torch.empty((self.Q, self.T), dtype=torch.float64, device="cuda")
        self.align = torch.empty((self.Q, self.T, 3), dtype=torch.int16, device="cuda")
        self.score = torch.empty((self.Q, self.T), dtype=torch.int32, device="cuda")
        self.step = motifs._query_chunk(self.lib, self.Q, self.T, self.wmax, bins, 1, BUDGET)
        self.nbytes = int(self.lib.explainn_motif_significance_workspace_bytes(self.step, self.T, self.wmax, bins, 1))
        self.ws = torch.empty((self.nbytes,), dtype=torch.uint8, device="cuda")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(self):
        for a in range(0, self.Q, self.step):
            n = min(self.step, self.Q - a)
            self._lib.check(self.lib.explainn_motif_significance(
                self.q[a:a + n].data_ptr(), self.qw[a:a + n].data_ptr(), n, self.t.data_ptr(), self.tw.data_ptr(),
                self.T, self.wmax, 0.0, MIN_OVERLAP, 1, self.bins, self.p[a:a + n].data_ptr(),
                self.align[a:a + n].data_ptr(), self.score[a:a + n].data_ptr(), None, None, self.ws.data_ptr(),
                self.nbytes, self.stream))

    def timed(self, reps):
        torch, times = self.torch, []
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.run()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return times[1:]

    def stages(self):
        """{kernel name: ms} of one pass, or None."""
        torch = self.torch
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                self.run()
                torch.cuda.synchronize()
            out = {}
            for ev in prof.key_averages():
                name = ev.key.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
                dev = getattr(ev, "device_time_total", None)
                if dev is None:
                    dev = getattr(ev, "cuda_time_total", 0.0)
                if name.startswith("motif_") and dev > 0:
                    out[name] = out.get(name, 0.0) + dev / 1e3
            return out or None
        except Exception as exc:                               # the split is a by-product: never fail the timing
            print("motifsig_probe: no stage split (%s)" % exc, file=sys.stderr)
            return None


def model_leg(q, qw, t, tw, bins, n):
    import motifsig_model as sm
    t0 = time.perf_counter()
    m = sm.significance(q[:n], qw[:n], t, tw, MIN_OVERLAP, 0.0, True, bins)
    return m, (time.perf_counter() - t0) * 1e3


def run(name, reps, bins, model_queries):
    Q, T, wlo, whi = SHAPES[name]
    q, qw = make(Q, wlo, whi, 1)
    t, tw = make(T, wlo, whi, 2)
    p, qv = device_leg(q, qw, t, tw, bins)                    # warm-up, and the result to compare
    res = Resident(q, qw, t, tw, bins)
    res.run()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        device_leg(q, qw, t, tw, bins)
        times.append((time.perf_counter() - t0) * 1e3)
    rec = {"shape": name, "Q": Q, "T": T, "widths": [wlo, whi], "wmax": whi, "min_overlap": MIN_OVERLAP, "bins": bins,
           "reps": reps, "workspace_budget_bytes": BUDGET, "query_chunk": res.step, "calls": -(-Q // res.step),
           "workspace_bytes": res.nbytes, "device": stats(times), "device_kernel": stats(res.timed(max(reps, 3)))}
    rec["stages_ms"] = res.stages()
    assert np.array_equal(res.p.cpu().numpy().view(np.uint64), p.view(np.uint64)), "the two legs disagree"
    rec["share_p_below_0.05"] = float((p < 0.05).mean())
    rec["share_q_below_0.05"] = float((qv < 0.05).mean())
    rec["smallest_p"] = float(p.min())
    if model_queries:
        n = min(model_queries, Q)
        m, ms = model_leg(q, qw, t, tw, bins, n)
        rel = np.abs(p[:n] - m["pvalue"]) / np.maximum(m["pvalue"], 1e-300)
        rec["numpy_scaled"] = {"queries": n, "measured_ms": ms, "scaled_to_all_queries_ms": ms * Q / n}
        rec["model_pairs_within_1e-9"] = float((rel <= 1e-9).mean())
        rec["model_largest_relative_difference"] = float(rel.max())
        rec["numpy_scaled_over_device_kernel"] = ms * Q / n / rec["device_kernel"]["median_ms"]
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="annotate,bank")
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--model-queries", type=int, default=8, help="0 skips the numpy leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run("warm", 1, a.bins, 2 if a.model_queries else 0)
    recs = [run(name, a.reps, a.bins, a.model_queries) for name in a.shapes.split(",")]
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    main()
