"""Motif significance restated in numpy (csrc/motifs.hip,
explainn_motif_significance): the statistic of Gupta et al. 2007 (Tomtom with incomplete scores, column
similarity Pearson) as the kernel, explainn_amd.motifs and the tests agree on.

  column:     d, n as in motifs_model.prepare (same pseudocount rule); u = d / sqrt(n), u = 0 where n < VAR_FLOOR
  col score:  c(qi, tj) = u_q[i] . u_t[j]   (in [-1,1]; the Pearson correlation of the two columns)
  quantised:  b = clamp(floor((c + 1) * bins/2 + 0.5), 0, bins), an integer; bins in [2,128]
  database:   the columns of all targets of width > 0, plus the columns of their reverse complements when
              both_strands; N of them
  null:       h[q][i][b] = #{database columns with b(q_i, column) = b} / N
  range null: for query columns [lo, lo+w): pmf = h[q][lo] * ... * h[q][lo+w-1] (convolution), support 0..w*bins;
              SF_{lo,w}(s) = min(1, sum_{s' >= s} pmf(s'))
  alignment:  (strand, offset, overlap [lo,hi), admissibility) exactly as in motifs_model; its score
              S = sum_i b(q_i, t'_{i+o}) over the overlap; p_align = SF_{lo,w}(S)
  pair:       the admissible alignment with the smallest p_align, ties to strand 0, then the smaller offset;
              n_align = number of admissible alignments of the pair (both strands counted);
              pvalue = -expm1(n_align * log1p(-p_align))   (1 when p_align = 1); pvalue = 1, alignment zeros when
              a width is 0 or N = 0
  row:        evalue = pvalue * T;  qvalue = Benjamini-Hochberg over the T targets of one query:
              q_(k) = min_{j>=k} min(1, p_(j) * T / j), p sorted ascending, stable

`pair_loops` is that text as plain loops over one (query, target) of a database.  `significance` is the same
for two packed sets at once; it takes the quantised column scores from outside when asked to (the device's
own integers), so that the later stages can be checked apart from the rounding of the first.

The layout of the column scores is the device's: colscore[q, i, s, j, t] (uint8) is query column i of query q
against column j of the strand-s view of target t, NONE (255) where either column does not exist."""
import numpy as np

import motifs_model as mm

VAR_FLOOR = mm.VAR_FLOOR
NONE = 255


def unit_columns(m, pc=0.0):
    """(w,4) counts -> (w,4) unit columns (zero where the column has no variance)."""
    d, n = mm.prepare(m, pc)
    ok = n >= VAR_FLOOR
    return np.where(ok[:, None], d / np.sqrt(np.where(ok, n, 1.0))[:, None], 0.0)


def unrounded(c, bins):
    """The column score in bin units before the rounding: b = clamp(floor(unrounded + 0.5), 0, bins)."""
    return (np.asarray(c, dtype=np.float64) + 1.0) * (bins / 2.0)


def quantise(c, bins):
    return np.clip(np.floor(unrounded(c, bins) + 0.5), 0, bins).astype(np.int64)


def range_sf(h_rows):
    """h_rows: (w, bins+1) pmfs of consecutive query columns -> [SF_1, ..., SF_w], SF_k over the first k rows."""
    out, pmf = [], None
    for h in h_rows:
        pmf = h.copy() if pmf is None else np.convolve(pmf, h)
        out.append(np.minimum(np.cumsum(pmf[::-1])[::-1], 1.0))
    return out


def sidak(p_align, n_align):
    p_align = np.asarray(p_align, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = -np.expm1(np.asarray(n_align, dtype=np.float64) * np.log1p(-np.minimum(p_align, 1.0)))
    return np.where(p_align >= 1.0, 1.0, p)


def bh_qvalues(p):
    """(Q,T) p-values -> (Q,T) Benjamini-Hochberg q-values, each row on its own."""
    p = np.asarray(p, dtype=np.float64)
    Q, T = p.shape
    if T == 0:
        return p.copy()
    order = np.argsort(p, axis=1, kind="stable")
    ranked = np.minimum(1.0, np.take_along_axis(p, order, axis=1) * T / np.arange(1, T + 1)[None, :])
    ranked = np.minimum.accumulate(ranked[:, ::-1], axis=1)[:, ::-1]
    out = np.empty_like(p)
    np.put_along_axis(out, order, ranked, axis=1)
    return out


# ---------------------------------------------------------------- plain loops, one pair
def pair_loops(q, targets, k, min_overlap=5, pc=0.0, both_strands=True, bins=100):
    """Query q against targets[k], the null from all of `targets`.  Returns dict(pvalue, offset, strand,
    overlap, score, p_align, n_align)."""
    strands = (0, 1) if both_strands else (0,)
    uq = unit_columns(q, pc)
    wq = len(uq)
    views = []                                             # every strand view of every target
    for t in targets:
        t = np.asarray(t, dtype=np.float64).reshape(-1, 4)
        views.append([unit_columns(mm.revcomp(t) if s else t, pc) for s in strands])
    N = sum(len(v[0]) for v in views) * len(strands)
    wt = len(views[k][0])
    none = dict(pvalue=1.0, offset=0, strand=0, overlap=0, score=0, p_align=1.0, n_align=0)
    if wq == 0 or wt == 0 or N == 0:
        return none
    h = np.zeros((wq, bins + 1))
    for i in range(wq):
        for v in views:
            for s in strands:
                for col in v[s]:
                    c = 0.0
                    for a in range(4):
                        c += uq[i, a] * col[a]
                    h[i, int(quantise(c, bins))] += 1
    h /= N
    best, n_align = None, 0
    for s in strands:
        ut = views[k][s]
        for o in range(-(wq - 1), wt):
            lo, hi = max(0, -o), min(wq, wt - o)
            w = hi - lo
            if w < 1 or w < min(min_overlap, wq, wt):
                continue
            S = 0
            for i in range(lo, hi):
                S += int(quantise(float(uq[i] @ ut[i + o]), bins))
            pmf = np.array([1.0])
            for i in range(lo, hi):
                new = np.zeros(len(pmf) + bins)
                for b in range(bins + 1):
                    for x in range(len(pmf)):
                        new[x + b] += pmf[x] * h[i, b]
                pmf = new
            p = min(1.0, float(sum(pmf[x] for x in range(len(pmf) - 1, S - 1, -1))))
            n_align += 1
            if best is None or p < best[0]:
                best = (p, o, s, w, S)
    p, o, s, w, S = best
    return dict(pvalue=float(sidak(p, n_align)), offset=o, strand=s, overlap=w, score=S, p_align=p, n_align=n_align)


# ---------------------------------------------------------------- packed sets
def _units(x, widths, pc):
    """(M,wmax,4), widths -> (unit columns (M,wmax,4), their reverse-complement view, clean widths)."""
    M, wmax, _ = x.shape
    widths = np.asarray(widths, dtype=np.int64)
    widths = np.where((widths < 0) | (widths > wmax), 0, widths)
    u, rc = np.zeros((M, wmax, 4)), np.zeros((M, wmax, 4))
    for i, w in enumerate(widths):
        if w:
            u[i, :w] = unit_columns(x[i, :w], pc)
            rc[i, :w] = u[i, :w][::-1, ::-1]
    return u, rc, widths


def column_scores(q, qw, t=None, tw=None, pc=0.0, both_strands=True, bins=100):
    """(colscore uint8 (Q,wmax,S,wmax,T), raw float64 of the same shape: the unrounded value in bin units, NaN
    where colscore is NONE)."""
    if t is None:
        t, tw = q, qw
    uq, _, qw = _units(np.asarray(q), qw, pc)
    ut, rt, tw = _units(np.asarray(t), tw, pc)
    wmax = uq.shape[1]
    views = np.stack([ut, rt] if both_strands else [ut])              # (S,T,wmax,4)
    raw = unrounded(np.einsum("qia,stja->qisjt", uq, views), bins)
    valid = ((np.arange(wmax)[None, :] < qw[:, None])[:, :, None, None, None]
             & (np.arange(wmax)[:, None] < tw[None, :])[None, None, None, :, :])
    valid = np.broadcast_to(valid, raw.shape)
    cs = np.where(valid, np.clip(np.floor(raw + 0.5), 0, bins), NONE).astype(np.uint8)
    return cs, np.where(valid, raw, np.nan)


def histograms(colscore, bins):
    """(Q,wmax,S,wmax,T) -> int64 (Q,wmax,bins+1): the count of every score along a query column's row."""
    Q, wmax = colscore.shape[:2]
    flat = colscore.reshape(Q * wmax, -1)
    out = np.zeros((Q * wmax, bins + 1), dtype=np.int64)
    for r in range(Q * wmax):
        out[r] = np.bincount(flat[r], minlength=256)[:bins + 1]
    return out.reshape(Q, wmax, bins + 1)


def significance(q, qw, t=None, tw=None, min_overlap=5, pc=0.0, both_strands=True, bins=100, colscore=None):
    """Every alignment of every pair and the best of each.  Returns dict(pvalue, evalue, qvalue, offset, strand,
    overlap, score, p_align, n_align, runner_up (Q,T); hist (Q,wmax,bins+1) int64; N; colscore; and per
    alignment, entry [.., s, j] being offset offsets[j] on strand s: p_all (1 on an inadmissible one), score_all,
    w_all, adm (Q,T,2,2 wmax - 1); offsets)."""
    if t is None:
        t, tw = q, qw
    q, t = np.asarray(q), np.asarray(t)
    Q, wmax, _ = q.shape
    T = len(t)
    qw = np.asarray(qw, dtype=np.int64)
    tw = np.asarray(tw, dtype=np.int64)
    qw = np.where((qw < 0) | (qw > wmax), 0, qw)
    tw = np.where((tw < 0) | (tw > wmax), 0, tw)
    S = 2 if both_strands else 1
    if colscore is None:
        colscore = column_scores(q, qw, t, tw, pc, both_strands, bins)[0]
    colscore = np.asarray(colscore).reshape(Q, wmax, S, wmax, T)
    hist = histograms(colscore, bins)
    N = int(tw.sum()) * S
    offsets = np.arange(-(wmax - 1), wmax)
    nO = len(offsets)
    score_all = np.zeros((Q, T, 2, nO), dtype=np.int64)
    w_all = np.zeros((Q, T, 2, nO), dtype=np.int64)
    present = colscore != NONE
    vals = np.where(present, colscore, 0).astype(np.int64)
    for s in range(S):
        for j, o in enumerate(offsets):
            i = np.arange(max(0, -o), min(wmax, wmax - o))
            score_all[:, :, s, j] = vals[:, i, s, i + o, :].sum(axis=1)
            w_all[:, :, s, j] = present[:, i, s, i + o, :].sum(axis=1)
    need = np.minimum(min_overlap, np.minimum(qw[:, None], tw[None, :]))[:, :, None, None]
    adm = (w_all >= 1) & (w_all >= need)
    adm[:, :, S:] = False
    p_all = np.ones((Q, T, 2, nO))
    for a in range(Q):
        if not qw[a] or not N:
            continue
        h = hist[a, :qw[a]] / float(N)
        for lo in range(qw[a]):
            sf = range_sf(h[lo:])                                     # sf[w-1] is SF_{lo,w}
            tab = np.ones((len(sf), len(sf[-1])))
            for k, v in enumerate(sf):
                tab[k, :len(v)] = v
            # the overlap of offset o starts at max(0, -o): lo > 0 is offset -lo alone, lo = 0 every o >= 0
            js = slice(wmax - 1 - lo, wmax - lo) if lo else slice(wmax - 1, nO)
            ok = adm[a, :, :S, js]
            got = tab[np.where(ok, w_all[a, :, :S, js] - 1, 0), np.where(ok, score_all[a, :, :S, js], 0)]
            p_all[a, :, :S, js] = np.where(ok, got, 1.0)
    masked = np.where(adm, p_all, np.inf).reshape(Q, T, 2 * nO)
    idx = masked.argmin(axis=2)                          # the first minimum: s = 0 before s = 1, then the smaller o
    found = adm.reshape(Q, T, -1).any(axis=2)
    take = lambda v: np.where(found, np.take_along_axis(v.reshape(Q, T, 2 * nO), idx[:, :, None], axis=2)[:, :, 0], 0)
    n_align = adm.reshape(Q, T, -1).sum(axis=2)
    p_align = np.where(found, take(p_all), 1.0)
    pvalue = np.where(found, sidak(p_align, n_align), 1.0)
    part = np.sort(masked, axis=2)
    return dict(pvalue=pvalue, evalue=pvalue * T, qvalue=bh_qvalues(pvalue), offset=np.where(found, offsets[idx % nO], 0),
                strand=np.where(found, idx // nO, 0), overlap=take(w_all), score=take(score_all), p_align=p_align,
                n_align=n_align, runner_up=part[:, :, 1] if 2 * nO > 1 else np.full((Q, T), np.inf), found=found,
                hist=hist, N=N, colscore=colscore, p_all=p_all, score_all=score_all, w_all=w_all, adm=adm,
                offsets=offsets)
