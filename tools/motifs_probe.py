#!/usr/bin/env python3
"""Times motif comparison (csrc/motifs.hip) on one GPU against the host and against stock torch on the same
GPU.  Synthetic Dirichlet motifs, two shapes:
  annotate  300 x 2000, widths 6..24, wmax 24   (one model's filters against a JASPAR-sized set)
  bank      2000 x 2000, width 19               (the filters of a model bank against themselves)
Legs, alternating in one process after a warm-up of all of them; wall clock around work that ends in a
device-to-host copy or a device synchronise; three passes by default; median, minimum and maximum of each:
  device         motifs.compare from host-resident packed motifs to a host-resident ncor (both copies included)
  device_kernel  explainn_motif_compare alone between device events, inputs, outputs and workspace resident
  numpy          the same scores on the host, vectorised over pairs, one (strand, offset) at a time, float32
  torch          the same scores with stock torch on the same GPU: padded unfold of the centred targets, one
                 einsum per strand for the products (and one each for SX, SY and the overlap), then the max
                 over (strand, offset); centred inputs resident, result left on the device
The torch leg is the reference for speed: `kernel_pays` is true when the device_kernel median is below the
torch median by more than the two legs' spreads (max - min) together.  The legs' results are compared as well
(max |ncor - ncor_device|).  One JSON line per shape.

  motifs_probe.py [--reps R] [--shapes annotate,bank] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"annotate": (300, 2000, 6, 24), "bank": (2000, 2000, 19, 19), "warm": (70, 130, 6, 12)}
MIN_OVERLAP, FLOOR = 5, 1e-6


def make(M, wlo, whi, seed):
    rng = np.random.default_rng(seed)
    widths = rng.integers(wlo, whi + 1, size=M).astype(np.int32)
    x = np.zeros((M, whi, 4), dtype=np.float32)
    for i, w in enumerate(widths):
        x[i, :w] = rng.dirichlet([0.5] * 4, size=w)
    return x, widths


def centred(x, widths):
    """(d, rc view, mask), float32: what every leg but the device's starts from."""
    M, wmax, _ = x.shape
    mask = (np.arange(wmax)[None, :] < widths[:, None]).astype(np.float32)
    f = x / np.maximum(x.sum(axis=2, keepdims=True), 1e-30)
    d = ((f - 0.25) * mask[:, :, None]).astype(np.float32)
    rc = np.zeros_like(d)
    for i, w in enumerate(widths):
        rc[i, :w] = d[i, :w][::-1, ::-1]
    return d, rc, mask


def numpy_leg(q, qw, t, tw):
    dq, _, mq = centred(q, qw)
    dt, rt, mt = centred(t, tw)
    nq = (dq * dq).sum(axis=2)
    Q, T, wmax = len(q), len(t), q.shape[1]
    tot = (qw[:, None] + tw[None, :]).astype(np.float32)
    need = np.minimum(MIN_OVERLAP, np.minimum(qw[:, None], tw[None, :])).astype(np.float32)
    best = np.full((Q, T), -np.inf, dtype=np.float32)
    for ds in (dt, rt):
        ns = (ds * ds).sum(axis=2)
        for o in range(-(wmax - 1), wmax):
            lo, hi = max(0, -o), min(wmax, wmax - o)
            xy = dq[:, lo:hi].reshape(Q, -1) @ ds[:, lo + o:hi + o].reshape(T, -1).T
            sx = nq[:, lo:hi] @ mt[:, lo + o:hi + o].T
            sy = mq[:, lo:hi] @ ns[:, lo + o:hi + o].T
            w = mq[:, lo:hi] @ mt[:, lo + o:hi + o].T
            ok = (sx >= FLOOR) & (sy >= FLOOR)
            ncor = np.where(ok, xy / np.sqrt(np.where(ok, sx * sy, 1.0)), 0.0) * w / np.maximum(tot - w, 1.0)
            np.maximum(best, np.where((w >= 1) & (w >= need), ncor, -np.inf), out=best)
    return np.where(np.isfinite(best), best, 0.0)


def torch_setup(q, qw, t, tw):
    import torch
    dq, _, mq = centred(q, qw)
    dt, rt, mt = centred(t, tw)
    wmax = q.shape[1]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    pad = lambda a: torch.nn.functional.pad(a, (0, 0, wmax - 1, wmax - 1) if a.dim() == 3 else (wmax - 1, wmax - 1))
    dq, mq, dt, rt, mt = dev(dq), dev(mq), dev(dt), dev(rt), dev(mt)
    return dict(dq=dq, nq=(dq * dq).sum(dim=2), mq=mq, qw=dev(qw.astype(np.float32)), tw=dev(tw.astype(np.float32)),
                strands=[(pad(d), pad((d * d).sum(dim=2))) for d in (dt, rt)], mt=pad(mt), wmax=wmax)


def torch_leg(s, chunk=512):
    """ncor (Q,T) on the device; queries in chunks of `chunk` to bound the (chunk, T, offsets) temporaries."""
    import torch
    wmax = s["wmax"]
    mtu = s["mt"].unfold(1, wmax, 1)                                   # (T, offsets, wmax)
    out = []
    for a in range(0, len(s["dq"]), chunk):
        dq, nq, mq, qw = s["dq"][a:a + chunk], s["nq"][a:a + chunk], s["mq"][a:a + chunk], s["qw"][a:a + chunk]
        w = torch.einsum("qi,tji->qtj", mq, mtu)
        sx = torch.einsum("qi,tji->qtj", nq, mtu)
        tot = (qw[:, None] + s["tw"][None, :])[:, :, None]
        need = torch.minimum(torch.full_like(tot, float(MIN_OVERLAP)), torch.minimum(qw[:, None], s["tw"][None, :])[:, :, None])
        adm = (w >= 1) & (w >= need)
        best = None
        for dt, nt in s["strands"]:
            xy = torch.einsum("qia,tjai->qtj", dq, dt.unfold(1, wmax, 1))   # windows (T, offsets, 4, wmax)
            sy = torch.einsum("qi,tji->qtj", mq, nt.unfold(1, wmax, 1))
            ok = (sx >= FLOOR) & (sy >= FLOOR)
            cor = torch.where(ok, xy / torch.sqrt(torch.where(ok, sx * sy, torch.ones_like(sx))), torch.zeros_like(xy))
            ncor = torch.where(adm, cor * w / torch.clamp(tot - w, min=1.0), torch.full_like(cor, float("-inf")))
            m = ncor.max(dim=2).values
            best = m if best is None else torch.maximum(best, m)
        out.append(torch.where(torch.isfinite(best), best, torch.zeros_like(best)))
    res = torch.cat(out)
    torch.cuda.synchronize()
    return res


def device_leg(q, qw, t, tw):
    import torch
    from explainn_amd import motifs
    res = motifs.compare((torch.from_numpy(q), torch.from_numpy(qw)), (torch.from_numpy(t), torch.from_numpy(tw)),
                         min_overlap=MIN_OVERLAP)
    return res.ncor.cpu().numpy()


def kernel_ms(q, qw, t, tw, reps):
    import torch
    from explainn_amd import _lib
    lib = _lib.load()
    Q, T, wmax = len(q), len(t), q.shape[1]
    dq, dqw, dt, dtw = (torch.from_numpy(a).cuda() for a in (q, qw, t, tw))
    ncor = torch.empty((Q, T), dtype=torch.float32, device="cuda")
    cor = torch.empty((Q, T), dtype=torch.float32, device="cuda")
    align = torch.empty((Q, T, 3), dtype=torch.int16, device="cuda")
    nbytes = int(lib.explainn_motif_compare_workspace_bytes(Q, T, wmax))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    times = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.explainn_motif_compare(dq.data_ptr(), dqw.data_ptr(), Q, dt.data_ptr(), dtw.data_ptr(), T, wmax,
                                              0.0, MIN_OVERLAP, 1, ncor.data_ptr(), cor.data_ptr(), align.data_ptr(),
                                              ws.data_ptr(), nbytes, stream))
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return times[1:]


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def run(name, reps, host=True):
    Q, T, wlo, whi = SHAPES[name]
    q, qw = make(Q, wlo, whi, 1)
    t, tw = make(T, wlo, whi, 2)
    ts = torch_setup(q, qw, t, tw)
    legs = {"device": lambda: device_leg(q, qw, t, tw), "torch": lambda: torch_leg(ts).cpu().numpy()}
    timed = {"device": lambda: device_leg(q, qw, t, tw), "torch": lambda: torch_leg(ts)}
    if host:
        legs["numpy"] = timed["numpy"] = lambda: numpy_leg(q, qw, t, tw)
    results = {k: f() for k, f in legs.items()}                      # warm-up, and the results to compare
    times = {k: [] for k in timed}
    for _ in range(reps):
        for k, f in timed.items():
            t0 = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t0) * 1e3)
    rec = {"shape": name, "Q": Q, "T": T, "widths": [wlo, whi], "wmax": whi, "min_overlap": MIN_OVERLAP, "reps": reps}
    rec.update({k: stats(v) for k, v in times.items()})
    rec["device_kernel"] = stats(kernel_ms(q, qw, t, tw, max(reps, 5)))
    for k in results:
        if k != "device":
            rec["max_abs_ncor_%s_minus_device" % k] = float(np.abs(results[k] - results["device"]).max())
    spread = lambda s: s["max_ms"] - s["min_ms"]
    rec["torch_over_device_kernel"] = rec["torch"]["median_ms"] / rec["device_kernel"]["median_ms"]
    rec["kernel_pays"] = bool(rec["torch"]["median_ms"] - rec["device_kernel"]["median_ms"]
                              > spread(rec["torch"]) + spread(rec["device_kernel"]))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="annotate,bank")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run("warm", 1, host=not a.no_host)
    recs = [run(name, a.reps, host=not a.no_host) for name in a.shapes.split(",")]
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    main()
