"""numpy restatement of greedy in-silico evolution (csrc/evolve.hip): one
round's selection from ISM maps, and the loop of rounds around a caller-supplied ISM function.  Every
step is fixed -- fp32 weights and deltas widened to fp64 (the products are exact), tasks added in
ascending order, the strands' mean as 0.5 * (f + r) -- so the device gives the same bits.
tests/test_design_model.py checks pick() against an enumeration of every candidate."""
import numpy as np

NO_BASE = 255


def objective(delta_f, delta_r, weights):
    """gain (B,4,L) fp64 of base a at position p in the forward strand's coordinates.  delta_f,
    delta_r: fp32 (B,T,4,L), the ISM maps of the sequences and of their reverse complements (each in its
    own strand's coordinates; delta_r None = one strand).  weights: fp32 (T,) or (B,T)."""
    delta_f = np.asarray(delta_f, dtype=np.float32)
    B, T = delta_f.shape[:2]
    w = np.broadcast_to(np.asarray(weights, dtype=np.float32), (B, T)).astype(np.float64)

    def fold(d):
        o = np.zeros((B,) + d.shape[2:], dtype=np.float64)
        for t in range(T):
            o = o + w[:, t, None, None] * d[:, t].astype(np.float64)
        return o
    gain = fold(delta_f)
    if delta_r is not None:
        # base a at p is base 3-a at L-1-p of the reverse strand
        gain = 0.5 * (gain + fold(np.asarray(delta_r, dtype=np.float32)[:, :, ::-1, ::-1]))
    return gain


def admissible(gain, codes, mask, min_gain):
    """(B,4,L) bool: a is not the base at p (at an N, any code above 3, all four are), the position is
    open, the gain exceeds min_gain (held as fp32, as the C ABI passes it)."""
    B, _, L = gain.shape
    ok = np.arange(4)[None, :, None] != codes[:, None, :]
    if mask is not None:
        ok = ok & (np.asarray(mask)[:, None, :] != 0)
    return ok & (gain > np.float64(np.float32(min_gain)))


def pick(delta_f, delta_r, codes, mask, weights, lock=True, min_gain=0.0):
    """One round.  Returns (pos int32, ref uint8, alt uint8, gain fp64, each (B), codes', mask'): per
    sequence the admissible candidate of the largest gain, ties to the lowest p, then the lowest a; -1,
    255, 255, 0 and unchanged codes where there is none.  mask None: every position open, and nothing
    to lock."""
    codes = np.array(codes, dtype=np.uint8)
    mask = None if mask is None else np.array(mask, dtype=np.uint8)
    B, L = codes.shape
    gain = objective(delta_f, delta_r, weights)
    ok = admissible(gain, codes, mask, min_gain)
    # position-major order, so that the first maximum is the lowest p, then the lowest a
    g = np.where(ok, gain, -np.inf).transpose(0, 2, 1).reshape(B, L * 4)
    best = g.argmax(axis=1)
    moved = ok.any(axis=(1, 2))
    rows = np.arange(B)
    p, a = best // 4, best % 4
    pos = np.where(moved, p, -1).astype(np.int32)
    ref = np.where(moved, codes[rows, p], NO_BASE).astype(np.uint8)
    alt = np.where(moved, a, NO_BASE).astype(np.uint8)
    out_gain = np.where(moved, g[rows, best], 0.0)
    codes[rows[moved], p[moved]] = a[moved]
    if lock and mask is not None:
        mask[rows[moved], p[moved]] = 0
    return pos, ref, alt, out_gain, codes, mask


def evolve(ism, codes, weights, rounds, mask=None, both_strands=False, lock=True, min_gain=0.0):
    """The loop.  ism(codes, reverse_complement) -> (logits (B,T), delta (B,T,4,L)) of the sequences or
    of their reverse complements, delta in the coordinates of the strand it ran on.  Returns a dict:
    pos, ref, alt, gain (B,rounds), codes (B,L) the result, rounds_codes [rounds+1] the codes before
    every round and at the end, logits (B,rounds+1,S,T)."""
    codes = np.array(codes, dtype=np.uint8)
    B, L = codes.shape
    if mask is not None:
        mask = np.array(np.broadcast_to(np.asarray(mask) != 0, (B, L)), dtype=np.uint8)
    elif lock:
        mask = np.ones((B, L), dtype=np.uint8)
    strands = (False, True) if both_strands else (False,)
    log = dict(pos=[], ref=[], alt=[], gain=[])
    seen, logits = [codes.copy()], []
    for r in range(rounds):
        res = [ism(codes, rc) for rc in strands]
        logits.append(np.stack([lg for lg, _ in res], axis=1))
        pos, ref, alt, gain, codes, mask = pick(res[0][1], res[1][1] if both_strands else None, codes, mask,
                                                weights, lock, min_gain)
        for key, v in zip(("pos", "ref", "alt", "gain"), (pos, ref, alt, gain)):
            log[key].append(v)
        seen.append(codes.copy())
    logits.append(np.stack([ism(codes, rc)[0] for rc in strands], axis=1))
    out = {key: np.stack(v, axis=1) for key, v in log.items()}
    out.update(codes=codes, rounds_codes=seen, logits=np.stack(logits, axis=1))
    return out
