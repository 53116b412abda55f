"""Numpy restatement of the activation null ("Calibrated sites"): from float16
activation arrays to bins, histogram, tail, total, the threshold rule and the empirical p-value -- what
explainn_activation_histogram / explainn_activation_null (csrc/actnull.hip) and sites.ActivationNull
produce.  tests/test_actnull_model.py checks it against brute force; tests/test_gpu_actnull.py compares
the device with it."""
import numpy as np

BINS = 32768
INF = 0x7C00


def bins(acts16):
    """Bin of every float16 activation: its bit pattern without the sign.  For values >= 0 the patterns
    sort like the values (+inf = 0x7C00, NaNs above)."""
    a = np.ascontiguousarray(np.asarray(acts16, dtype=np.float16))
    return (a.view(np.uint16) & 0x7FFF).astype(np.int64)


def bin_values():
    """float32 (BINS,): the value of every pattern (NaN above 0x7C00)."""
    return np.arange(BINS, dtype=np.uint16).view(np.float16).astype(np.float32)


def histogram(acts16, mask=None):
    """int64 (U, BINS) from float16 (U, P) activations; mask (P,) bool selects the live positions."""
    acts16 = np.asarray(acts16, dtype=np.float16)
    if mask is not None:
        acts16 = acts16[:, mask]
    return np.stack([np.bincount(bins(row), minlength=BINS) for row in acts16]).astype(np.int64) \
        if len(acts16) else np.zeros((0, BINS), np.int64)


def total(hist):
    return np.asarray(hist, dtype=np.int64).sum(axis=1)


def tail(hist):
    """tail[u][b] = sum of hist[u][b'] over b' >= b."""
    return np.cumsum(np.asarray(hist, dtype=np.int64)[:, ::-1], axis=1)[:, ::-1]


def allowed(hist, alpha):
    """m = floor(alpha * total) per unit, one fp64 multiply."""
    return np.floor(np.float64(alpha) * total(hist).astype(np.float64)).astype(np.uint64).astype(np.int64)


def threshold_bins(hist, alpha):
    """Per unit the smallest pattern b <= 0x7C00 with tail[b + 1] <= m (0x7C00 if none, and for an empty row)."""
    t, m, tot = tail(hist), allowed(hist, alpha), total(hist)
    t1 = np.concatenate([t[:, 1:], np.zeros((len(t), 1), np.int64)], axis=1)      # tail[b + 1]
    out = np.full(len(t), INF, dtype=np.int64)
    for u in range(len(t)):
        ok = np.flatnonzero(t1[u, :INF + 1] <= m[u])
        if tot[u] > 0 and len(ok):
            out[u] = ok[0]
    return out


def thresholds(hist, alpha):
    """float32 (U,): the float16 value of threshold_bins."""
    return bin_values()[threshold_bins(hist, alpha)]


def pvalue(hist, unit_ids, scores):
    """float64: (1 + tail[u][bits(float16(score))]) / (1 + total[u])."""
    unit = np.asarray(unit_ids, dtype=np.int64)
    b = bins(np.asarray(scores, dtype=np.float32).astype(np.float16))
    return (1.0 + tail(hist)[unit, b].astype(np.float64)) / (1.0 + total(hist)[unit].astype(np.float64))


def count_above(hist, thr):
    """Per unit the null activations > thr[u] (thr finite or +inf, >= 0 or negative)."""
    vals = bin_values()[:INF + 1]
    h = np.asarray(hist, dtype=np.int64)
    return np.array([h[u, :INF + 1][vals > np.float32(thr[u])].sum() for u in range(len(h))], dtype=np.int64)
