"""numpy restatement of what csrc/metrics.hip computes, step for step: the order-preserving key of an
fp32 value (-0.0 canonicalised, denormals kept), a sort by that key, run boundaries, and per run

    AUROC    U2 = sum pos * (2 * negatives_strictly_below + neg), an integer;  U2 / (2 P Nneg)
    AP       sum (pos * cP) / (cA * P), cP / cA = positives / elements at or above the run's score
    Spearman d = 2 * rank - (n + 1) = start + end + 1 - n (integer, mean 0);  Pearson of d
    Pearson  fp64 means, centred sums

with the integer parts in exact Python / int64 arithmetic and every float sum through math.fsum, so
that the values returned are the exactly rounded references the device results are held against
(the role tests/ism_model.py plays for ISM).  What is rounded at all: one division per AP term (the
kernel performs the same division, so the terms are bit-identical), the centring and the products of
Pearson (a relative 2**-53 each), and the final division / square roots."""
import math

import numpy as np


def order_key(v):
    """uint32 whose unsigned order is the numeric order of the fp32 values; -0.0 == +0.0."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def runs(sorted_keys):
    """(start, end) of the run of equal keys each sorted position belongs to (end inclusive)."""
    n = len(sorted_keys)
    first = np.ones(n, dtype=bool)
    first[1:] = sorted_keys[1:] != sorted_keys[:-1]
    idx = np.arange(n, dtype=np.int64)
    start = np.maximum.accumulate(np.where(first, idx, 0))
    last = np.ones(n, dtype=bool)
    last[:-1] = first[1:]
    end = np.minimum.accumulate(np.where(last, idx, n)[::-1])[::-1]
    return start, end


def binary_parts(y, s):
    """One column: dict(P, Nneg, U2 (Python int), num, den (int64 arrays: the AP terms num/den))."""
    y = np.asarray(y, dtype=np.float32).ravel()
    key = order_key(np.asarray(s, dtype=np.float32).ravel())
    order = np.argsort(key, kind="stable")
    lab = (y[order] == 1.0).astype(np.int64)
    n = len(lab)
    start, end = runs(key[order])
    is_end = end == np.arange(n)
    cpos = np.cumsum(lab)                                  # positives at positions <= i
    a = start[is_end]
    e = np.nonzero(is_end)[0]
    Ca = np.where(a > 0, cpos[np.maximum(a - 1, 0)], 0)    # positives before the run
    pos = cpos[e] - Ca
    neg = (e + 1 - a) - pos
    P = int(cpos[-1])
    # pos * (2 negb + neg) < 2^53 per run; the total may pass 2^63 only beyond n = 2^31: Python ints anyway
    u2_terms = pos * (2 * (a - Ca) + neg)
    U2 = sum(int(x) for x in u2_terms.reshape(-1)) if n < 4096 else _int_sum(u2_terms)
    keep = pos > 0
    return dict(P=P, Nneg=n - P, U2=U2, num=(pos * (P - Ca))[keep], den=((n - a) * P)[keep])


def _int_sum(a):
    """Exact sum of a non-negative int64 array whose total may not fit 64 bits."""
    a = np.asarray(a, dtype=np.int64)
    hi, lo = a >> 32, a & 0xFFFFFFFF
    return (int(hi.sum()) << 32) + int(lo.sum())


def _signed_dot(a, b):
    """Exact sum a_i * b_i for int64 arrays with |a_i|, |b_i| < 2^27 (products < 2^54)."""
    p = a.astype(np.int64) * b.astype(np.int64)
    return _int_sum(np.where(p > 0, p, 0)) - _int_sum(np.where(p < 0, -p, 0))


def auroc(parts):
    """float(U2) / float(2 P Nneg): one correctly rounded division of exactly represented integers."""
    if parts["P"] == 0 or parts["Nneg"] == 0:
        return float("nan")
    return float(parts["U2"]) / float(2 * parts["P"] * parts["Nneg"])


def average_precision(parts):
    if parts["P"] == 0:
        return 0.0
    return math.fsum((parts["num"].astype(np.float64) / parts["den"].astype(np.float64)).tolist())


def rank_deviations(v):
    """d = 2 * average_rank - (n + 1) per element, int64 (scipy.stats.rankdata's 'average' ranks)."""
    key = order_key(np.asarray(v, dtype=np.float32).ravel())
    order = np.argsort(key, kind="stable")
    start, end = runs(key[order])
    d = np.empty(len(key), dtype=np.int64)
    d[order] = start + end + 1 - len(key)
    return d


def spearman(y, s):
    dy, ds = rank_deviations(y), rank_deviations(s)
    syy, sss, sys_ = _signed_dot(dy, dy), _signed_dot(ds, ds), _signed_dot(dy, ds)
    if syy == 0 or sss == 0:
        return float("nan")
    return float(sys_) / (math.sqrt(syy) * math.sqrt(sss))


def pearson(y, s):
    y = np.asarray(y, dtype=np.float32).ravel().astype(np.float64)
    s = np.asarray(s, dtype=np.float32).ravel().astype(np.float64)
    if (y == y[0]).all() or (s == s[0]).all():
        return float("nan")
    cy = y - math.fsum(y.tolist()) / len(y)
    cs = s - math.fsum(s.tolist()) / len(s)
    syy, sss, sys_ = math.fsum((cy * cy).tolist()), math.fsum((cs * cs).tolist()), math.fsum((cy * cs).tolist())
    return sys_ / (math.sqrt(syy) * math.sqrt(sss))


def columns(y, s, per_task):
    """The (targets, scores) columns a call works on: T of length N, or one of length N*T (flatten())."""
    y, s = np.asarray(y, dtype=np.float32), np.asarray(s, dtype=np.float32)
    if y.ndim == 1:
        y, s = y[:, None], s[:, None]
    if per_task:
        return [(y[:, t], s[:, t]) for t in range(y.shape[1])]
    return [(y.reshape(-1), s.reshape(-1))]
