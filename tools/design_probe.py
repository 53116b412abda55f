#!/usr/bin/env python3
"""Time of greedy in-silico evolution (csrc/evolve.hip, ExplaiNN.evolve) on one GPU against the route a user
had before (the two legs share the ISM calls and differ in the selection), at 300 units x 1024 sequences and
100 units x 100 sequences (k 19, L 200, one task), 10 rounds, on one strand and on both.

Legs (device-resident codes in, device-resident results out, host clock around a device synchronise):
  evolve       model.evolve: per round and strand model.in_silico_mutagenesis, then one selection launch
               (explainn_evolve_pick) that reduces the maps, picks and edits
  torch_loop   what the parent commit offers on the same GPU: per round and strand
               model.in_silico_mutagenesis(BaseCodes(codes, rc)) (the dense (B,T,4,L) map), the reverse map
               flipped back, the same objective in fp64, the same admissibility, tie rule and locking as torch
               ops, the edit as a torch scatter; nothing goes to the host inside the loop
  select_kernel / select_torch   one round's selection alone on the first round's maps, held fixed: one
               explainn_evolve_pick launch against torch_loop's chain of torch ops; ms per selection, from two
               device events around 50 selections, a copy of the codes and a fresh mask included in both
Before timing the two legs' positions, bases, gains and final codes are compared: they must be equal.  Every
(shape, strands) runs in a process of its own under its own time limit; the first that fails or runs out of
time ends the probe.  A warm-up pass, then --passes (3) timed passes, the legs alternating: median and spread
(max - min) in ms.  `evolve_beats_loop`: the medians differ by more than the two spreads.

usage: design_probe.py [--passes 3] [--limit 240] [--out profiles/r35_design_probe.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((300, 1024), (100, 100))           # (units, sequences)
K, L, T, ROUNDS = 19, 200, 1, 10
SELECT_REPS = 50                            # selections per timed window of the selection-only legs


def _child(U, B, both, passes):
    import numpy as np
    import torch

    import ctypes as C

    from explainn_amd import ExplaiNN, _lib
    from explainn_amd.architectures import BaseCodes
    from oracle import explainn_oracle as orc

    sd = orc.random_state_dict(U, K, L, T, seed=0)
    m = ExplaiNN(U, K, L, T)
    m.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    m.cuda().eval()
    codes0 = torch.from_numpy(np.random.default_rng(1).integers(0, 4, size=(B, L)).astype(np.uint8)).cuda()
    w = torch.ones(T, device="cuda")
    rows = torch.arange(B, device="cuda")
    base = torch.arange(4, device="cuda").view(1, 4, 1)

    def evolve():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = codes0.clone()
        with torch.no_grad(), m.eval_cache():
            pos, ref, alt, gain, _ = m.evolve(codes, w, ROUNDS, None, both, True, 0.0)
        torch.cuda.synchronize()
        return (pos, alt, gain, codes), (time.perf_counter() - t0) * 1e3

    w64 = w.double()

    def torch_select(codes, open_, maps):
        """One round's selection as torch ops on the strands' maps (each in its own coordinates): the edit of
        codes and open_ in place, and (pos, alt, gain)."""
        gain = None
        for rc, delta in enumerate(maps):
            if rc:
                delta = delta.flip(2, 3)
            g = torch.zeros((B, 4, L), dtype=torch.float64, device="cuda")
            for t in range(T):
                g = g + w64[t] * delta[:, t].double()
            gain = g if gain is None else 0.5 * (gain + g)
        ok = (base != codes[:, None, :]) & open_[:, None, :] & (gain > 0)
        flat = torch.where(ok, gain, torch.full_like(gain, float("-inf"))).transpose(1, 2).reshape(B, 4 * L)
        top, best = flat.max(dim=1)
        # torch.max gives no promise about which of equal maxima it returns: take the first
        best = (flat == top[:, None]).to(torch.uint8).argmax(dim=1)
        moved = ok.flatten(1).any(dim=1)
        p, a = best // 4, (best % 4).to(torch.uint8)
        # (index_put with where, not a boolean mask: a mask's nonzero() would synchronise with the host)
        codes[rows, p] = torch.where(moved, a, codes[rows, p])
        open_[rows, p] = open_[rows, p] & ~moved
        return (torch.where(moved, p, torch.full_like(p, -1)).to(torch.int32),
                torch.where(moved, a, torch.full_like(a, 255)), torch.where(moved, top, torch.zeros_like(top)))

    def torch_loop():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codes = codes0.clone()
        open_ = torch.ones((B, L), dtype=torch.bool, device="cuda")
        log = ([], [], [])
        with torch.no_grad(), m.eval_cache():
            for _ in range(ROUNDS):
                maps = [m.in_silico_mutagenesis(BaseCodes(codes, rc))[1] for rc in ((False, True) if both else (False,))]
                for dst, v in zip(log, torch_select(codes, open_, maps)):
                    dst.append(v)
        out = (torch.stack(log[0]), torch.stack(log[1]), torch.stack(log[2]), codes)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    # the selection on its own: the first round's maps held fixed, SELECT_REPS selections between two device
    # events, each on a fresh copy of the codes and an all-open mask (the copies are inside both legs' times)
    with torch.no_grad():
        maps0 = [m.in_silico_mutagenesis(BaseCodes(codes0, rc))[1] for rc in ((False, True) if both else (False,))]
    lib = _lib.load()
    pos1 = torch.empty(B, dtype=torch.int32, device="cuda")
    ref1, alt1 = torch.empty(B, dtype=torch.uint8, device="cuda"), torch.empty(B, dtype=torch.uint8, device="cuda")
    gain1 = torch.empty(B, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def select_leg(kernel):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(SELECT_REPS):
            codes = codes0.clone()
            if kernel:
                mask = torch.ones((B, L), dtype=torch.uint8, device="cuda")
                _lib.check(lib.explainn_evolve_pick(
                    maps0[0].data_ptr(), maps0[1].data_ptr() if both else None, codes.data_ptr(), mask.data_ptr(),
                    w.data_ptr(), 0, B, T, L, 1, 0.0, pos1.data_ptr(), ref1.data_ptr(), alt1.data_ptr(),
                    gain1.data_ptr(), stream))
                out = (pos1, alt1, gain1, codes)
            else:
                out = torch_select(codes, torch.ones((B, L), dtype=torch.bool, device="cuda"), maps0) + (codes,)
        e1.record()
        e1.synchronize()
        return out, e0.elapsed_time(e1) / SELECT_REPS

    row = {"units": U, "sequences": B, "strands": 2 if both else 1, "device": torch.cuda.get_device_name(0)}
    a, b = evolve()[0], torch_loop()[0]                                           # (also the warm-up)
    row["loop_equals_evolve"] = bool(all(torch.equal(x, y) for x, y in zip(a, b)))
    row["moves"] = int((a[0] >= 0).sum())
    if not row["loop_equals_evolve"]:
        raise SystemExit("the routes disagree: %r" % row)
    a, b = select_leg(True)[0], select_leg(False)[0]                              # (also the warm-up)
    row["select_torch_equals_kernel"] = bool(all(torch.equal(x, y) for x, y in zip(a, b)))
    if not row["select_torch_equals_kernel"]:
        raise SystemExit("the selections disagree: %r" % row)
    ts = {"evolve": [], "torch_loop": [], "select_kernel": [], "select_torch": []}
    for _ in range(passes):
        ts["evolve"].append(evolve()[1])
        ts["torch_loop"].append(torch_loop()[1])
        ts["select_kernel"].append(select_leg(True)[1])
        ts["select_torch"].append(select_leg(False)[1])
    row["legs"] = {k: {"median_ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "ms": v}
                   for k, v in ts.items()}
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per (shape, strands) process")
    ap.add_argument("--out", default="profiles/r35_design_probe.json")
    ap.add_argument("--child", nargs=3, metavar=("UNITS", "SEQUENCES", "BOTH"))
    args = ap.parse_args()
    if args.child:
        return _child(int(args.child[0]), int(args.child[1]), bool(int(args.child[2])), args.passes)
    doc = {"kernel_size": K, "bases": L, "tasks": T, "rounds": ROUNDS, "lock": True, "min_gain": 0.0,
           "passes": args.passes, "results": []}
    ok = True
    for U, B in SHAPES:
        for both in (0, 1):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--passes",
                   str(args.passes), "--child", str(U), str(B), str(both)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            rows = [json.loads(ln[4:]) for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not rows:
                print("units %d sequences %d strands %d: exit %d (124 / 137: over its limit of %d s); the probe ends "
                      "here\n%s" % (U, B, both + 1, out.returncode, args.limit, out.stderr[-2000:]), flush=True)
                ok = False
                break
            doc.setdefault("device", rows[0].pop("device"))
            rows[0].pop("device", None)
            doc["results"].append(rows[0])
            print(json.dumps({"units": U, "sequences": B, "strands": both + 1, "moves": rows[0]["moves"],
                              **{k: [round(v["median_ms"], 3), round(v["spread_ms"], 3)]
                                 for k, v in rows[0]["legs"].items()}}), flush=True)
        if not ok:
            break
    for name, slow, fast in (("evolve_beats_loop", "torch_loop", "evolve"),
                             ("select_kernel_beats_torch", "select_torch", "select_kernel")):
        doc[name] = {}
        for r in doc["results"]:
            a, b = r["legs"][slow], r["legs"][fast]
            doc[name]["u%d_b%d_s%d" % (r["units"], r["sequences"], r["strands"])] = bool(
                a["median_ms"] - b["median_ms"] > a["spread_ms"] + b["spread_ms"])
    doc["complete"] = ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
