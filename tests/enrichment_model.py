"""fp64 numpy / math.lgamma model of motif enrichment (csrc/enrich.hip, explainn_amd/enrichment.py; DESIGN.md
section 8, "Enrichment"), written from the definitions of include/explainn_hip.h.

Best sites: from float16 activation arrays (U, P) of the forward and the reverse strand of one record, the
largest bit pattern and (start << 1) | is_minus of the site that holds it -- the lowest start among equal
maxima, '+' before '-' at one start.  `best_brute` reads the rule off start by start; `best_of_acts` is the
vectorised form the GPU test uses.

The test: tails a_t, b_t of the two score lists, the thresholds, the hypergeometric tail summed as the device
sums it, the best threshold, log_padj's two branches, u2 and auroc.

LOGSF_DEVIATION: the largest absolute deviation of `hypergeom_logsf` from scipy.stats.hypergeom.logsf, in
ln p, over the grid of tests/test_enrichment_model.py, by the grid's N (measured: 3.53e-14 at N = 40, 9.09e-13
at 400, 1.46e-11 at 4000, 1.76e-10 at 40000, 6.43e-9 at 10^6, with at most 10, 41, 130, 407 and 1197 terms --
the growth is the cancellation of lgammas of size N ln N); the constants are those figures rounded up to two
digits and test_logsf_matches_scipy holds the model to them.
tests/test_gpu_enrichment.py allows the device ten times the figure of its N."""
import math

import numpy as np

BINS = 32768
LOGSF_DEVIATION = {40: 3.6e-14, 400: 9.1e-13, 4000: 1.5e-11, 40000: 1.8e-10, 10 ** 6: 6.5e-9}
MIN_GAP = 1e-6           # between the best and the runner-up logp of a unit, wherever the GPU test demands exactness


def deviation(N):
    """The recorded deviation of the smallest grid N that is at least N."""
    return LOGSF_DEVIATION[min(g for g in LOGSF_DEVIATION if g >= N)]


def log_tolerance(N):
    """What the device's log_pvalue / log_padj may differ by from the model's: ten times the model's own
    deviation from scipy at that N, and at least 64 ulp of lgamma(N + 1) (the two lgammas need not round
    alike)."""
    return max(10.0 * deviation(N), 64.0 * float(np.spacing(math.lgamma(N + 1.0))))


# ------------------------------------------------------------------------------------------- best sites
def to_bits(acts16):
    return np.ascontiguousarray(np.asarray(acts16, dtype=np.float16)).view(np.uint16) & 0x7FFF


def best_brute(fwd16, rev16=None):
    """(bits (U,), site (U,)) of one record from (U, P) float16 activations, start by start."""
    f = to_bits(fwd16)
    r = None if rev16 is None else to_bits(rev16)
    U, P = f.shape
    bits, site = np.zeros(U, dtype=np.uint16), np.full(U, -1, dtype=np.int32)
    for u in range(U):
        best = -1
        for p in range(P):
            for minus, arr in ((0, f), (1, r)):
                if arr is not None and int(arr[u, p]) > best:      # strictly: the first met wins a tie
                    best, site[u] = int(arr[u, p]), (p << 1) | minus
        bits[u] = max(best, 0)
    return bits, site


def best_of_acts(fwd16, rev16=None):
    """The same, vectorised: the first start that holds the maximum on either strand; '+' if it holds it."""
    f = to_bits(fwd16).astype(np.int64)
    U, P = f.shape
    if P == 0:
        return np.zeros(U, dtype=np.uint16), np.full(U, -1, dtype=np.int32)
    r = f if rev16 is None else to_bits(rev16).astype(np.int64)
    top = np.maximum(f, r).max(axis=1)
    p = np.argmax(np.maximum(f, r) == top[:, None], axis=1)
    minus = (f[np.arange(U), p] != top).astype(np.int64)
    return top.astype(np.uint16), ((p << 1) | minus).astype(np.int32)


def record_best(acts, codes, offsets, k, both=True):
    """(bits (U, R) uint16, site (U, R) int32) of the records codes[offsets[r] : offsets[r+1]].
    acts(codes, reverse) -> float16 (U, len - k + 1) activations of one record of at least k bases.  A record
    whose offsets descend or leave [0, len(codes)] has no live start."""
    R = len(offsets) - 1
    out_b, out_s = [], []
    for r in range(R):
        a, b = int(offsets[r]), int(offsets[r + 1])
        rec = codes[a:b] if 0 <= a <= b <= len(codes) else codes[:0]
        if len(rec) < k:
            bits, site = None, None
        else:
            bits, site = best_of_acts(acts(rec, False), acts(rec, True) if both else None)
        out_b.append(bits)
        out_s.append(site)
    U = next((len(b) for b in out_b if b is not None), 0)
    bits = np.stack([b if b is not None else np.zeros(U, np.uint16) for b in out_b], axis=1)
    site = np.stack([s if s is not None else np.full(U, -1, np.int32) for s in out_s], axis=1)
    return bits, site


# ------------------------------------------------------------------------------------------- the test
def tails(col, labels):
    """(a, b) int64 (32768,): primary (label 1) / control (label 0) records with bits >= t."""
    col = np.asarray(col).astype(np.int64) & 0x7FFF
    labels = np.asarray(labels)
    out = []
    for which in (1, 0):
        h = np.bincount(col[labels == which], minlength=BINS)
        out.append(np.cumsum(h[::-1])[::-1].astype(np.int64))
    return out[0], out[1]


def hypergeom_logsf(a, n, Np, Nc, return_terms=False):
    """ln P[X >= a], X ~ Hypergeometric(Np + Nc, Np, n), as the device sums it: ln of the first term from nine
    lgammas, plus ln of (1 + the following terms relative to it), each from the ratio of neighbouring terms,
    until x reaches min(Np, n) or a term no longer changes the sum."""
    lg = math.lgamma
    N, b = Np + Nc, n - a
    first = (lg(Np + 1.0) - lg(a + 1.0) - lg(Np - a + 1.0) + lg(Nc + 1.0) - lg(b + 1.0) - lg(Nc - b + 1.0)
             - lg(N + 1.0) + lg(n + 1.0) + lg(N - n + 1.0))
    total, term, terms = 1.0, 1.0, 1
    for x in range(a, min(Np, n)):
        term *= (float(Np - x) * float(n - x)) / (float(x + 1) * float(Nc - n + x + 1))
        s = total + term
        if s == total:
            break
        total = s
        terms += 1
    out = min(0.0, first + math.log(total))
    return (out, terms) if return_terms else out


def logp(a, b, Np, Nc):
    """0 unless the primary set is enriched at the threshold (a N > n Np, in integers)."""
    n = a + b
    return hypergeom_logsf(a, n, Np, Nc) if a * (Np + Nc) > n * Np else 0.0


def log_padj(lp, m, branch=None):
    """ln(1 - (1 - p)^m).  branch None: the device's choice (the short form below ln p = -30); "full" and
    "short" force one."""
    if m == 0:
        return 0.0
    if branch == "short" or (branch is None and lp < -30.0):
        return min(0.0, math.log(m) + lp)
    return min(0.0, math.log(-math.expm1(m * math.log1p(-math.exp(lp))))) if lp < 0.0 else 0.0


def unit_stats(col, labels):
    """One unit's outputs and what the tests need besides: a dict with tails a, b; Np, Nc; thresholds (the
    patterns held) and their logp; n_thresholds, best_pattern, tp, fp, log_pvalue, log_padj, u2, auroc; gap,
    the distance from the best logp to the runner-up (inf with fewer than two thresholds; 0 when the best
    value is held twice, inf when it is the assigned 0)."""
    a, b = tails(col, labels)
    Np, Nc = int(a[0]), int(b[0])
    a1, b1 = np.append(a[1:], 0), np.append(b[1:], 0)
    held = np.flatnonzero((a != a1) | (b != b1))
    lps = np.array([logp(int(a[t]), int(b[t]), Np, Nc) for t in held], dtype=np.float64)
    out = {"a": a, "b": b, "Np": Np, "Nc": Nc, "thresholds": held, "logp": lps, "n_thresholds": len(held)}
    if len(held):
        low = lps.min()
        best = int(held[np.flatnonzero(lps == low)[-1]])          # among equal values the highest pattern
        rest = np.sort(lps)
        # logp = 0 is assigned, not computed: equal zeros are equal on the device too, and the pattern decides
        out["gap"] = float(rest[1] - rest[0]) if len(rest) > 1 and low < 0.0 else float("inf")
    else:
        low, best = 0.0, 0
        out["gap"] = float("inf")
    out.update(best_pattern=best, tp=int(a[best]), fp=int(b[best]), log_pvalue=float(low),
               log_padj=log_padj(float(low), len(held)))
    prim, ctrl = a - a1, b - b1
    out["u2"] = int(np.sum(prim * (2 * (Nc - b) + ctrl)))
    out["auroc"] = out["u2"] / (2.0 * Np * Nc) if Np > 0 and Nc > 0 else float("nan")
    return out


def test_stats(bits, labels):
    """Every unit's unit_stats, stacked: a dict of arrays over the units (tails: (U, 2, 32768))."""
    per = [unit_stats(col, labels) for col in np.asarray(bits)]
    out = {f: np.array([p[f] for p in per]) for f in ("n_thresholds", "best_pattern", "tp", "fp", "log_pvalue",
                                                      "log_padj", "u2", "auroc", "gap")}
    out["tails"] = np.stack([np.stack([p["a"], p["b"]]) for p in per]) if per else np.zeros((0, 2, BINS), np.int64)
    lab = np.asarray(labels)
    out["counts"] = np.array([np.sum(lab == 1), np.sum(lab == 0)], dtype=np.int64)
    return out


test_stats.__test__ = False       # a model function, not a test


def brute_counts(col, labels, t):
    """(a_t, b_t) read off the raw score lists."""
    col = np.asarray(col).astype(np.int64) & 0x7FFF
    labels = np.asarray(labels)
    return int(np.sum((col >= t) & (labels == 1))), int(np.sum((col >= t) & (labels == 0)))


def brute_u2(col, labels):
    """Twice the Mann-Whitney U of primary over control: 2 per (primary > control) pair, 1 per tie."""
    col = np.asarray(col).astype(np.int64) & 0x7FFF
    labels = np.asarray(labels)
    p, c = col[labels == 1], col[labels == 0]
    return int(2 * np.sum(p[:, None] > c[None, :]) + np.sum(p[:, None] == c[None, :]))


# ------------------------------------------------------------------------------------------- inputs
def half_normal_case(n_primary=60, n_control=90, units=4, seed=0, shift=0.6):
    """The 60 + 90 case: (bits uint16 (units, N), labels uint8 (N,)) of half-normal scores rounded to float16,
    the primary records' scaled up in every unit but the last, with two records left out (label 2)."""
    g = np.random.default_rng(seed)
    N = n_primary + n_control + 2
    labels = np.concatenate([np.ones(n_primary, np.uint8), np.zeros(n_control, np.uint8), np.full(2, 2, np.uint8)])
    x = np.abs(g.standard_normal((units, N)))
    x[:-1, :n_primary] *= 1.0 + shift
    order = g.permutation(N)
    return x.astype(np.float16).view(np.uint16)[:, order].copy(), labels[order].copy()


def many_units_case():
    """More units than a call has workgroups: 300 units of the 60 + 90 case."""
    return half_normal_case(units=300, seed=9)


def synthetic_cases():
    """Named (bits, labels) matrices fed straight to the entry point: all-equal scores (m = 1), patterns in the
    NaN range, excluded labels, Np = 0, Nc = 0 and no included record at all."""
    g = np.random.default_rng(5)
    lab = (g.random(40) < 0.4).astype(np.uint8)
    cases = {"all_equal": (np.full((2, 40), 0x3C00, np.uint16), lab)}
    nan = g.integers(0x7BF0, 0x7E10, size=(3, 40)).astype(np.uint16)            # finite, +inf and NaN patterns
    nan[0, lab == 1] |= 0x7E00
    cases["nan_range"] = (nan, lab)
    mixed = g.integers(0, 6, size=40).astype(np.uint8)                            # labels 2..5 are left out
    cases["excluded"] = (g.integers(0x3000, 0x3040, size=(3, 40)).astype(np.uint16), mixed)
    some = g.integers(0x3000, 0x3400, size=(2, 40)).astype(np.uint16)
    cases["no_primary"] = (some, np.where(lab == 1, 3, 0).astype(np.uint8))
    cases["no_control"] = (some, np.where(lab == 0, 7, 1).astype(np.uint8))
    cases["nothing"] = (some, np.full(40, 2, np.uint8))
    cases["high_bit"] = (some | 0x8000, lab)                                      # bit 15 is not read
    return cases
