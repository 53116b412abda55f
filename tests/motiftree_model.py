"""Motif tree, cut, placement and pooled cluster motifs restated in numpy ("Motif tree";
csrc/motiftree.hip): the semantics the kernels, explainn_amd.motifs and the tests agree on.

  input:     a self-comparison of M motifs (ncor, offset, strand; the upper triangle is read) and the widths w;
             q[i,j] = (int32) rint(float32 ncor[i,j] * 2^20) for leaves i < j
  linkage:   single = max q, complete = min q, average = (double) S / (double) (|A| |B|), S the int64 sum of q,
             over the leaf pairs across two clusters; (sum, pairs) is (q, 1) for single and complete
  step:      a cluster's slot is its smallest leaf; the live pair lo < hi with the largest linkage merges, ties to
             the smallest lo, then the smallest hi; the merged cluster keeps slot lo; M - 1 steps
  best pair: the leaf pair (i < j) across the two clusters with the largest q, ties to the smallest i, then j
  placement: leaf x at (f, h): frame column h + c holds column c of rc^f(m_x); see `transform`
  log:       int32 (M-1, 8) = lo, hi, leaves, leaf_i, leaf_j, F, H, 0; link int64 (M-1, 2) = sum, pairs;
             gone int32 [M]: the step at which slot c was merged away (-1: never); flips, shifts: every leaf
             in the root frame
  cut:       t = ceil(min_ncor 2^20); a step is above the cut when sum >= t pairs

`tree_brute` recomputes every linkage from the leaf pairs at every step; `tree` keeps the cluster matrices and
updates one row per step (a few seconds at M = 1000) -- test_motiftree_model.py holds the two equal."""
import math

import numpy as np

SCALE = 1 << 20
LINKAGES = {"single": 0, "complete": 1, "average": 2}
LOG_FIELDS = ("lo", "hi", "leaves", "leaf_i", "leaf_j", "F", "H")


def quantise(ncor):
    return np.rint(np.asarray(ncor, dtype=np.float32) * np.float32(SCALE)).astype(np.int32)


def rc(m):
    return np.asarray(m)[::-1, ::-1]


def placed(m, f):
    """rc^f(m)."""
    return rc(m) if f else np.asarray(m)


def transform(i, j, s, o, j_moves, f, h, w):
    """(F, H) of a step whose best leaf pair is (i < j) with compare's (s, o) for (i, j): in a frame where i is
    (0, 0), j is (s, -o).  j_moves: j is in the moved cluster."""
    if j_moves:
        a, m, ro = i, j, o
    else:
        a, m, ro = j, i, (int(w[i]) + o - int(w[j]) if s else -o)
    fa, ha, fm, hm = int(f[a]), int(h[a]), int(f[m]), int(h[m])
    ft = s ^ fa
    ht = ha + int(w[a]) + ro - int(w[m]) if fa else ha - ro
    F = ft ^ fm
    H = ht - (-(hm + int(w[m])) if F else hm)
    return F, H


def apply(F, H, f, h, w):
    """One leaf (or an array of leaves) through a step's transform."""
    return f ^ F, (-(h + w) if F else h) + H


def _empty(M):
    return dict(log=np.zeros((max(M - 1, 0), 8), np.int32), link=np.zeros((max(M - 1, 0), 2), np.int64),
                gone=np.full(M, -1, np.int32), flips=np.zeros(M, np.int32), shifts=np.zeros(M, np.int32))


def _record(out, t, lo, hi, leaves, s, n, i, j, F, H):
    out["log"][t, :7] = (lo, hi, leaves, i, j, F, H)
    out["link"][t] = (s, n)
    out["gone"][hi] = t


def tree_brute(ncor, offset, strand, widths, linkage="average"):
    kind = LINKAGES[linkage]
    w = np.asarray(widths, dtype=np.int64)
    M = len(w)
    q = quantise(ncor).astype(np.int64) if M else np.zeros((0, 0), np.int64)
    offset, strand = np.asarray(offset).astype(np.int64), np.asarray(strand).astype(np.int64)
    out = _empty(M)
    slot = list(range(M))
    f, h = [0] * M, [0] * M
    for t in range(M - 1):
        acc = {}
        for i in range(M):
            for j in range(i + 1, M):
                a, b = slot[i], slot[j]
                if a == b:
                    continue
                key = (min(a, b), max(a, b))
                v = int(q[i, j])
                e = acc.get(key)
                if e is None:
                    acc[key] = [v, 1, v, v, (v, -i, -j)]
                else:
                    e[0] += v
                    e[1] += 1
                    e[2] = max(e[2], v)
                    e[3] = min(e[3], v)
                    e[4] = max(e[4], (v, -i, -j))
        best = None
        for (lo, hi) in sorted(acc):
            s, n, vmax, vmin, _ = acc[(lo, hi)]
            s, n = ((vmax, 1), (vmin, 1), (s, n))[kind]
            val = np.float64(s) / np.float64(n)
            if best is None or val > best[0]:
                best = (val, lo, hi, s, n)
        _, lo, hi, s, n = best
        _, i, j = acc[(lo, hi)][4]
        i, j = -i, -j
        F, H = transform(i, j, int(strand[i, j]), int(offset[i, j]), slot[j] == hi, f, h, w)
        leaves = 0
        for y in range(M):
            if slot[y] == hi:
                f[y], h[y] = apply(F, H, f[y], h[y], int(w[y]))
                slot[y] = lo
            leaves += slot[y] == lo
        _record(out, t, lo, hi, leaves, s, n, i, j, F, H)
    out["flips"][:], out["shifts"][:] = f, h
    return out


def tree(ncor, offset, strand, widths, linkage="average"):
    kind = LINKAGES[linkage]
    w = np.asarray(widths, dtype=np.int64)
    M = len(w)
    out = _empty(M)
    if M < 2:
        return out
    offset, strand = np.asarray(offset), np.asarray(strand)
    ar = np.arange(M, dtype=np.int64)
    iu = np.triu_indices(M, 1)
    S = np.zeros((M, M), np.int64)
    S[iu] = quantise(ncor).astype(np.int64)[iu]
    S = S + S.T
    ii, jj = np.minimum.outer(ar, ar), np.maximum.outer(ar, ar)
    K = ((S + (1 << 31)).astype(np.uint64) << np.uint64(32)) | ((65535 - ii) << 16 | (65535 - jj)).astype(np.uint64)
    V = np.full((M, M), -np.inf)
    V[iu] = S[iu].astype(np.float64)
    size = np.ones(M, np.int64)
    alive = np.ones(M, bool)
    slot = ar.copy()
    f, h = np.zeros(M, np.int64), np.zeros(M, np.int64)
    combine = (np.maximum, np.minimum, np.add)[kind]
    for t in range(M - 1):
        lo, hi = divmod(int(V.argmax()), M)          # the first maximum: the smallest lo, then the smallest hi
        s = int(S[lo, hi])
        n = int(size[lo] * size[hi]) if kind == 2 else 1
        key = int(K[lo, hi])
        i, j = 65535 - ((key >> 16) & 65535), 65535 - (key & 65535)
        F, H = transform(i, j, int(strand[i, j]), int(offset[i, j]), slot[j] == hi, f, h, w)
        moved = slot == hi
        f[moved], h[moved] = apply(F, H, f[moved], h[moved], w[moved])
        slot[moved] = lo
        S[lo] = combine(S[lo], S[hi])
        S[:, lo] = S[lo]
        K[lo] = np.maximum(K[lo], K[hi])
        K[:, lo] = K[lo]
        size[lo] += size[hi]
        alive[hi] = False
        V[hi, :] = -np.inf
        V[:, hi] = -np.inf
        others = alive.copy()
        others[lo] = False
        pairs = (size[lo] * size).astype(np.float64) if kind == 2 else np.ones(M)
        val = np.where(others, S[lo].astype(np.float64) / pairs, -np.inf)
        V[lo, lo + 1:] = val[lo + 1:]
        V[:lo, lo] = val[:lo]
        _record(out, t, lo, hi, int(size[lo]), s, n, i, j, F, H)
    out["flips"][:], out["shifts"][:] = f, h
    return out


def heights(tr):
    return tr["link"][:, 0].astype(np.float64) / tr["link"][:, 1].astype(np.float64) / SCALE


def threshold(min_ncor):
    if not float(min_ncor) > 0:
        raise ValueError("min_ncor must be positive")
    return int(math.ceil(float(min_ncor) * SCALE))


def cut(tr, widths, min_ncor):
    """(labels int64 [M], flips int32 [M], shifts int32 [M], spans int32 [C], slots int64 [C])."""
    thr = threshold(min_ncor)
    w = np.asarray(widths, dtype=np.int64)
    M = len(w)
    hts = heights(tr)
    assert (np.diff(hts) <= 0).all(), "heights never increase"
    log, link, gone = tr["log"], tr["link"], tr["gone"]
    slot, f, h = np.zeros(M, np.int64), np.zeros(M, np.int32), np.zeros(M, np.int64)
    for y in range(M):
        c, fy, hy = y, 0, 0
        while gone[c] >= 0 and link[gone[c], 0] >= thr * link[gone[c], 1]:
            t = gone[c]
            fy, hy = apply(int(log[t, 5]), int(log[t, 6]), fy, hy, int(w[y]))
            c = int(log[t, 0])
        slot[y], f[y], h[y] = c, fy, hy
    slots = np.unique(slot)
    labels = np.searchsorted(slots, slot).astype(np.int64)
    spans = np.zeros(len(slots), np.int32)
    for c in range(len(slots)):
        mem = labels == c
        h[mem] -= h[mem].min()
        spans[c] = (h[mem] + w[mem]).max()
    return labels, f, h.astype(np.int32), spans, slots


def pool(x, widths, labels, flips, shifts, spans):
    """x: (M, wmax, 4) float32.  (merged float64 (C, span_max, 4), support int32 (C, span_max)): per column the
    fp64 sum over the members in ascending leaf order, plain adds."""
    x = np.asarray(x, dtype=np.float32)
    C = len(spans)
    smax = int(max(spans)) if C else 0
    merged = np.zeros((C, smax, 4), np.float64)
    support = np.zeros((C, smax), np.int32)
    for y in range(len(widths)):
        wy, c, hy = int(widths[y]), int(labels[y]), int(shifts[y])
        m = placed(x[y, :wy], int(flips[y])).astype(np.float64)
        for col in range(wy):
            for a in range(4):
                merged[c, hy + col, a] = merged[c, hy + col, a] + m[col, a]
            support[c, hy + col] += 1
    return merged, support


def overlap_of(hi_, wi, hj, wj):
    """The number of frame columns two placed leaves share."""
    return max(0, min(hi_ + wi, hj + wj) - max(hi_, hj))


def random_motif(rng, w, depth=20):
    if not w:
        return np.zeros((0, 4))
    return np.stack([rng.multinomial(depth, p) for p in rng.dirichlet([0.3] * 4, size=w)]).astype(np.float64)


def family_set(seed, bases=4, copies=10, widths=(12, 14)):
    """bases x copies count matrices, family-major: every copy is its base (widths[0] to widths[1] columns) with
    0 to 2 columns cut from each end, every other one reverse-complemented.  Returns (motifs, family index per
    motif)."""
    rng = np.random.default_rng(seed)
    out, fam = [], []
    for b in range(bases):
        base = random_motif(rng, widths[0] + b % (widths[1] - widths[0] + 1))
        for k in range(copies):
            a, e = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            m = base[a:len(base) - e]
            out.append(np.ascontiguousarray(rc(m)) if k % 2 else m.copy())
            fam.append(b)
    return out, np.array(fam)
