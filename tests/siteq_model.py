"""Numpy model of site q-values (csrc/pwmsites.hip: explainn_pwm_score_histogram; csrc/siteq.hip:
explainn_site_qvalues; sites.SiteQvalues, pwmsites.scan_motifs(qvalue=); DESIGN.md section 8, "Site q-values").

Written from the contract in include/explainn_hip.h: the observed score histogram by a brute-force window loop
over quantised tables, the q-table of (unit, bin) by its defining expression, and -- independently -- the
textbook Benjamini-Hochberg procedure on the expanded per-test p-values, which the table must equal bit for bit.
Everything is fp64 / integer numpy."""
import numpy as np

ACT_BINS, ACT_INF = 32768, 0x7C00


# ---------------------------------------------------------------- the observed PWM score histogram
def score_histogram(S, lwidths, bins, codes, start=0, n_positions=None, period=0, both=True):
    """score_histogram_loop with all the windows of a motif scored at once (the GPU tests' shapes would take the
    loop seconds); tests/test_siteq_model.py holds the two equal."""
    codes = np.minimum(np.asarray(codes, dtype=np.int64), 4)
    M, wmax = S.shape[0], S.shape[1]
    n_positions = len(codes) - start if n_positions is None else n_positions
    end = min(start + n_positions + wmax - 1, len(codes))
    hist = np.zeros((M, wmax * bins + 2), dtype=np.int64)
    for m in range(M):
        w = int(lwidths[m])
        if not 1 <= w <= wmax or end - start < w:
            continue
        p = np.arange(start, min(start + n_positions, end - w + 1))
        win = np.lib.stride_tricks.sliding_window_view(codes[:end], w)[p]
        live = ~np.any(win >= 4, axis=1)
        if period > 0:
            live &= p % period <= period - w
        win = win[live]
        cols = np.arange(w)[None, :]
        strands = [win, 3 - win[:, ::-1]] if both else [win]
        for x in strands:
            hist[m] += np.bincount(S[m, cols, x].astype(np.int64).sum(axis=1), minlength=hist.shape[1])
    return hist


def score_histogram_loop(S, lwidths, bins, codes, start=0, n_positions=None, period=0, both=True):
    """int64 (M, wmax bins + 2): [m][s] = the live windows of motif m, either requested strand, that score s.
    One window at a time: live = its w bases lie inside [start, min(start + n_positions + wmax - 1, len)), hold
    no code >= 4 and, with a period, do not cross a record boundary."""
    codes = np.minimum(np.asarray(codes, dtype=np.int64), 4)
    M, wmax = S.shape[0], S.shape[1]
    n_positions = len(codes) - start if n_positions is None else n_positions
    end = min(start + n_positions + wmax - 1, len(codes))
    hist = np.zeros((M, wmax * bins + 2), dtype=np.int64)
    for m in range(M):
        w = int(lwidths[m])
        if not 1 <= w <= wmax:
            continue
        for p in range(start, start + n_positions):
            win = codes[p:p + w]
            if p + w > end or win.max() >= 4 or (period > 0 and p % period > period - w):
                continue
            hist[m, int(sum(int(S[m, j, win[j]]) for j in range(w)))] += 1
            if both:
                hist[m, int(sum(int(S[m, j, 3 - win[w - 1 - j]]) for j in range(w)))] += 1
    return hist


def live_tests(lwidths, wmax, codes, period=0, both=True):
    """int64 (M,): the number of tests of every motif over the whole of `codes`, counted without scoring."""
    codes = np.minimum(np.asarray(codes, dtype=np.int64), 4)
    isn = np.concatenate([[0], np.cumsum(codes >= 4)])
    out = np.zeros(len(lwidths), dtype=np.int64)
    for m, w in enumerate(int(w) for w in lwidths):
        if 1 <= w <= wmax and len(codes) >= w:
            p = np.arange(len(codes) - w + 1)
            live = isn[p + w] == isn[p]
            if period > 0:
                live &= p % period <= period - w
            out[m] = int(live.sum()) * (2 if both else 1)
    return out


# ---------------------------------------------------------------- the q-table
def qtable(obs, p, alpha=0.0):
    """(q float64 (U,B), total int64 (U,), first int64 (U,)):
        q[u][b] = min(1, min over b' <= b with R[b'] > 0 of (p[u][b'] * N) / R[b']),  N = sum obs[u], R = its
    suffix sums; first[u] = the smallest b with q[u][b] <= alpha, B if none."""
    obs, p = np.asarray(obs, dtype=np.int64), np.asarray(p, dtype=np.float64)
    U, B = obs.shape
    q, first = np.ones((U, B)), np.full(U, B, dtype=np.int64)
    total = obs.sum(axis=1)
    for u in range(U):
        R = np.cumsum(obs[u, ::-1])[::-1]
        term = np.full(B, np.inf)
        has = R > 0
        term[has] = (p[u, has] * np.float64(total[u])) / R[has].astype(np.float64)
        q[u] = np.minimum(1.0, np.minimum.accumulate(term))
        ok = np.flatnonzero(q[u] <= alpha)
        if len(ok):
            first[u] = ok[0]
    return q, total, first


def bh_sorted(pvals):
    """Benjamini-Hochberg q-values of a 1-D array of p-values, by the book: sort ascending, (p_(j) * N) / j, a
    running minimum from the largest rank down, capped at 1; returned in the order of the input."""
    pvals = np.asarray(pvals, dtype=np.float64)
    n = len(pvals)
    order = np.argsort(pvals, kind="stable")
    ranked = (pvals[order] * np.float64(n)) / np.arange(1, n + 1, dtype=np.float64)
    qs = np.minimum(1.0, np.minimum.accumulate(ranked[::-1])[::-1])
    out = np.empty(n)
    out[order] = qs
    return out


def per_test(obs_row, p_row):
    """(bin of every test, its p-value): the histogram expanded to one entry per test."""
    b = np.repeat(np.arange(len(obs_row)), np.asarray(obs_row, dtype=np.int64))
    return b, np.asarray(p_row, dtype=np.float64)[b]


# ---------------------------------------------------------------- what the listers do with it
def filter_thresholds(first):
    """float32 thresholds for `activation > threshold`: the float16 value one pattern below `first`; +inf where no
    finite or infinite activation qualifies; -1 where pattern 0 does."""
    first = np.asarray(first, dtype=np.int64)
    vals = np.arange(ACT_BINS, dtype=np.uint16).view(np.float16).astype(np.float32)
    out = np.where(first - 1 >= ACT_INF, np.float32(np.inf), vals[np.clip(first - 1, 0, ACT_BINS - 1)])
    return np.where(first == 0, np.float32(-1.0), out).astype(np.float32)


def empirical_p(null_hist):
    """float64 (U, 32768): (1 + tail) / (1 + total) of an activation null's histogram."""
    h = np.asarray(null_hist, dtype=np.int64)
    tail = np.cumsum(h[:, ::-1], axis=1)[:, ::-1]
    return (1.0 + tail.astype(np.float64)) / (1.0 + h.sum(axis=1).astype(np.float64))[:, None]
