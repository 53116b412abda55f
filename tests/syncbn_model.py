"""fp64 model of the sync-BN exchanges (csrc/syncbn.hip), built from the
numpy oracle's train-mode intermediates exactly as the combine kernels define them:

  X1  the integer pair counts behind G, m of the window indicator (moments_kernel: G = count/(B Lo))
  X2  sum q, sum q q' -- from per-shard sums about the shard's own shift s = the geometric mean of q over its
      first 16 sequences,
      converted to sums about zero (sum q = S1 + B s, sum q q' = S2 + s S1' + S1 s' + B s s')
  X3  sum z, sum z^2 per unit
  X4  sum d3, sum d3 zhat per unit, the combiner gradients, the loss sum
  X5  EQ, Se per unit (with the global BN3 statistics -- the backward of the sync step)
  X6  S1, S2 per unit (the BatchNorm1 backward sums)

`shard_exchanges` gives one shard's contributions; summing them over shards and deriving the
statistics must give the full batch's."""
import numpy as np

EPS = 1e-5


def window_counts(x, k):
    """Pair counts of the window indicator: C[(a,j),(a',j')] = #{(b,p): x[b,a,p+j] x[b,a',p+j']},
    c[(a,j)] = #{(b,p): x[b,a,p+j]}, over the Lo = L-k+1 window starts."""
    B, _, L = x.shape
    Lo = L - k + 1
    W = np.stack([x[:, :, j:j + Lo] for j in range(k)], axis=2)      # (B, 4, k, Lo)
    F = W.transpose(0, 3, 1, 2).reshape(B * Lo, 4 * k).astype(np.float64)
    return F.T @ F, F.sum(0)


def bn1_stats(C, c, w, N):
    """Mean and biased variance of the raw conv sum of filter w (4k) from the counts of N windows."""
    G, m = C / N, c / N
    mu = w @ m
    return mu, w @ G @ w - mu * mu


def qmoments_about(q, s):
    """qmom's partials: sums about a shift s."""
    d = q - s
    return d.sum(0), d.T @ d


def to_zero(S1, S2, s, B):
    """The combine step: sums about s -> sums about zero (an identity)."""
    return S1 + B * s, S2 + np.outer(s, S1) + np.outer(S1, s) + B * np.outer(s, s)


def shard_exchanges(x, q, z, zhat, d3, k):
    """One shard's X1, X2, X3 and the BN3 part of X4.  x (B,4,L) one-hot, q (B,U,n) pooled
    activations, z (B,U) FC2 outputs, zhat (B,U), d3 (B,U) the head gradient at z's BatchNorm."""
    B = x.shape[0]
    C, c = window_counts(x, k)
    X2 = []
    for u in range(q.shape[1]):
        s = np.exp(np.log(q[:16, u]).mean(axis=0))    # this shard's own shift
        S1, S2 = qmoments_about(q[:, u], s)
        X2.append(to_zero(S1, S2, s, B))
    return {"X1": (C, c), "X2": X2, "X3": (z.sum(0), (z * z).sum(0)),
            "X4": (d3.sum(0), (d3 * zhat).sum(0))}


def add(parts):
    """The caller's reduction: element-wise sums in rank order."""
    out = {}
    for key in parts[0]:
        vals = [p[key] for p in parts]
        if key == "X2":
            out[key] = [tuple(sum(v[u][i] for v in vals) for i in range(2)) for u in range(len(vals[0]))]
        else:
            out[key] = tuple(sum(v[i] for v in vals) for i in range(len(vals[0])))
    return out


def statistics(X, B, Lo, conv_w):
    """BatchNorm statistics from (global) exchanges: BN1 mean/var per unit, BN2's input moments
    (mean of q, covariance) per unit, BN3 mean/var per unit."""
    C, c = X["X1"]
    bn1 = [bn1_stats(C, c, conv_w[u].reshape(-1), B * Lo) for u in range(conv_w.shape[0])]
    bn2 = []
    for Sq, Sqq in X["X2"]:
        mean = Sq / B
        bn2.append((mean, Sqq / B - np.outer(mean, mean)))
    s1, s2 = X["X3"]
    m3 = s1 / B
    return bn1, bn2, (m3, s2 / B - m3 * m3)
