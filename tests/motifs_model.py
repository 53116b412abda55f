"""Motif comparison restated in numpy ("Motif comparison"; csrc/motifs.hip): the
semantics the kernel, explainn_amd.motifs and the tests agree on.

  column:     f[a] = (c[a] + pc/4) / (sum c + pc), 0.25 where that denominator is 0; d = f - 0.25; n = sum d^2
  alignment:  (s, o); s = 1 takes the target's reverse complement t'[j][a] = t[wt-1-j][3-a]; query column i
              meets target column i + o; overlap i in [max(0,-o), min(wq, wt-o)), w its size; admissible when
              w >= 1 and w >= min(min_overlap, wq, wt)
  scores:     XY = sum d_q[i].d_t'[i+o], SX = sum n_q[i], SY = sum n_t'[i+o] over the overlap;
              cor = XY / sqrt(SX SY), 0 when SX or SY < VAR_FLOOR; Ncor = cor w / (wq + wt - w)
  best:       the admissible (s, o) with the largest Ncor, ties to s = 0, then to the smaller o; zeros when a
              width is 0

`best_loops` is that text as plain loops over one pair.  `all_alignments` is the same for two packed sets at
once, every (s, o) kept, in the dtype asked for: float64 is the model, float32 the "fp32 restatement" whose
distance from the model sets the tolerance of the device test."""
import numpy as np

VAR_FLOOR = 1e-6


def prepare(m, pc=0.0, dtype=np.float64):
    """(w,4) counts -> (d (w,4), n (w,))."""
    c = np.asarray(m, dtype=dtype).reshape(-1, 4)
    tot = c.sum(axis=1, keepdims=True) + dtype(pc)
    safe = np.where(tot == 0, dtype(1), tot)
    f = np.where(tot == 0, dtype(0.25), (c + dtype(pc) / dtype(4)) / safe)
    d = (f - dtype(0.25)).astype(dtype)
    return d, (d * d).sum(axis=1)


def revcomp(m):
    return np.asarray(m)[::-1, ::-1]


def alignments_loops(q, t, min_overlap=5, pc=0.0, both_strands=True):
    """Every admissible alignment of one pair: [(s, o, w, cor, ncor)] in the order of the tie rule."""
    dq, nq = prepare(q, pc)
    wq, wt = len(dq), len(np.asarray(t).reshape(-1, 4))
    out = []
    if wq == 0 or wt == 0:
        return out
    for s in ((0, 1) if both_strands else (0,)):
        dt, nt = prepare(revcomp(np.asarray(t).reshape(-1, 4)) if s else t, pc)
        for o in range(-(wq - 1), wt):
            lo, hi = max(0, -o), min(wq, wt - o)
            w = hi - lo
            if w < 1 or w < min(min_overlap, wq, wt):
                continue
            xy = sx = sy = 0.0
            for i in range(lo, hi):
                for a in range(4):
                    xy += dq[i, a] * dt[i + o, a]
                sx += nq[i]
                sy += nt[i + o]
            cor = 0.0 if (sx < VAR_FLOOR or sy < VAR_FLOOR) else xy / np.sqrt(sx * sy)
            out.append((s, o, w, cor, cor * w / (wq + wt - w)))
    return out


def best_loops(q, t, min_overlap=5, pc=0.0, both_strands=True):
    """(ncor, cor, offset, strand, overlap) of one pair."""
    best = None
    for s, o, w, cor, ncor in alignments_loops(q, t, min_overlap, pc, both_strands):
        if best is None or ncor > best[0]:
            best = (ncor, cor, o, s, w)
    return best if best is not None else (0.0, 0.0, 0, 0, 0)


def pack(mats, wmax=None):
    """list of (w,4) -> ((M,wmax,4) float32 zero padded, widths int32)."""
    mats = [np.asarray(m, dtype=np.float64).reshape(-1, 4) for m in mats]
    wmax = wmax or max([len(m) for m in mats] + [1])
    out = np.zeros((len(mats), wmax, 4), dtype=np.float32)
    for i, m in enumerate(mats):
        out[i, :len(m)] = m
    return out, np.array([len(m) for m in mats], dtype=np.int32)


def _prepare_set(x, widths, pc, dtype):
    M, wmax, _ = x.shape
    d = np.zeros((M, wmax, 4), dtype=dtype)
    rc = np.zeros((M, wmax, 4), dtype=dtype)
    for i, w in enumerate(widths):
        if 0 < w <= wmax:
            di, _ = prepare(x[i, :w], pc, dtype)
            d[i, :w] = di
            rc[i, :w] = di[::-1, ::-1]
    mask = (np.arange(wmax)[None, :] < np.where((widths < 0) | (widths > wmax), 0, widths)[:, None]).astype(dtype)
    return d, rc, mask


def all_alignments(q, qw, t, tw, min_overlap=5, pc=0.0, both_strands=True, dtype=np.float64):
    """Every (s, o) of every pair of two packed sets.  Returns dict(ncor, cor, w, adm (Q,T,2,2 wmax - 1), sx,
    sy, offsets): entry [.., s, j] is offset offsets[j] on strand s."""
    q, t = np.asarray(q), np.asarray(t)
    qw, tw = np.asarray(qw, dtype=np.int64), np.asarray(tw, dtype=np.int64)
    wmax = q.shape[1]
    dq, _, mq = _prepare_set(q, qw, pc, dtype)
    dt, rt, mt = _prepare_set(t, tw, pc, dtype)
    nq = (dq * dq).sum(axis=2)
    qw = mq.sum(axis=1).astype(np.int64)
    tw = mt.sum(axis=1).astype(np.int64)
    offsets = np.arange(-(wmax - 1), wmax)
    Q, T = len(q), len(t)
    shape = (Q, T, 2, len(offsets))
    XY, SX, SY = np.zeros(shape, dtype), np.zeros(shape, dtype), np.zeros(shape, dtype)
    W = np.zeros(shape, np.int64)
    for s in range(2):
        ds = rt if s else dt
        ns = (ds * ds).sum(axis=2)
        # the reverse-complement view of target t starts at column 0 as well: its mask is the forward one
        for j, o in enumerate(offsets):
            lo, hi = max(0, -o), min(wmax, wmax - o)
            XY[:, :, s, j] = dq[:, lo:hi].reshape(Q, -1) @ ds[:, lo + o:hi + o].reshape(T, -1).T
            SX[:, :, s, j] = nq[:, lo:hi] @ mt[:, lo + o:hi + o].T
            SY[:, :, s, j] = mq[:, lo:hi] @ ns[:, lo + o:hi + o].T
            W[:, :, s, j] = np.rint(mq[:, lo:hi] @ mt[:, lo + o:hi + o].T).astype(np.int64)
    floor = dtype(VAR_FLOOR)
    ok = (SX >= floor) & (SY >= floor)
    cor = np.where(ok, XY / np.sqrt(np.where(ok, SX * SY, dtype(1))), dtype(0)).astype(dtype)
    tot = (qw[:, None] + tw[None, :])[:, :, None, None] - W
    ncor = (cor * W.astype(dtype) / np.maximum(tot, 1).astype(dtype)).astype(dtype)
    need = np.minimum(min_overlap, np.minimum(qw[:, None], tw[None, :]))[:, :, None, None]
    adm = (W >= 1) & (W >= need)
    if not both_strands:
        adm[:, :, 1] = False
    return dict(ncor=ncor, cor=cor, w=W, adm=adm, sx=SX, sy=SY, offsets=offsets)


def best_of(al):
    """The best alignment of every pair from all_alignments' output: dict(ncor, cor, offset, strand, overlap,
    runner_up); runner_up is the second largest admissible Ncor of the pair (-inf where there is none)."""
    Q, T, _, nO = al["ncor"].shape
    score = np.where(al["adm"], al["ncor"].astype(np.float64), -np.inf).reshape(Q, T, 2 * nO)
    idx = score.argmax(axis=2)                       # the first maximum: s = 0 before s = 1, then the smaller o
    found = al["adm"].reshape(Q, T, -1).any(axis=2)
    take = lambda a: np.take_along_axis(a.reshape(Q, T, 2 * nO), idx[:, :, None], axis=2)[:, :, 0]
    part = np.sort(score, axis=2)
    return dict(ncor=np.where(found, take(al["ncor"]), 0), cor=np.where(found, take(al["cor"]), 0),
                offset=np.where(found, al["offsets"][idx % nO], 0), strand=np.where(found, idx // nO, 0),
                overlap=np.where(found, take(al["w"]), 0), found=found,
                runner_up=part[:, :, -2] if 2 * nO > 1 else np.full((Q, T), -np.inf))


def compare(q, qw, t=None, tw=None, min_overlap=5, pc=0.0, both_strands=True, dtype=np.float64):
    if t is None:
        t, tw = q, qw
    return best_of(all_alignments(q, qw, t, tw, min_overlap, pc, both_strands, dtype))
