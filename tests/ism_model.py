"""fp64 numpy restatement of the incremental in-silico mutagenesis algebra (DESIGN.md section 3,
item 11) that csrc/ism.hip implements: per unit, the raw conv sums g of the unmutated sequence, the
pooled extremes and y2 = A2 q + sh2 in eval mode; a substitution (p, a) changes g at j in
[p-k+1, p] by d_j = W[a, p-j] - W[s, p-j], hence only the windows those j fall in, hence
y2' = y2 + sum_w A2[:, w] dq_w.  tests/test_ism_model.py checks it against brute force through the
oracle's forward on every substituted sequence."""
import numpy as np

from oracle import explainn_oracle as orc

EPS = orc.BN_EPS
POOL = orc.POOL
H = orc.FC_HIDDEN


def eval_tables(sd):
    f = lambda key: np.asarray(sd[key], dtype=np.float64)
    W = f("linears.0.weight")
    U, _, k = W.shape
    alpha = f("linears.1.weight") / np.sqrt(f("linears.1.running_var") + EPS)
    shift = f("linears.1.bias") + alpha * (f("linears.0.bias") - f("linears.1.running_mean"))
    n = f("linears.6.weight").shape[1]
    V1 = f("linears.6.weight").reshape(U, H, n)
    inv2 = (f("linears.7.weight") / np.sqrt(f("linears.7.running_var") + EPS)).reshape(U, H)
    A2 = inv2[:, :, None] * V1
    sh2 = f("linears.7.bias").reshape(U, H) + inv2 * (f("linears.6.bias").reshape(U, H)
                                                      - f("linears.7.running_mean").reshape(U, H))
    inv3 = f("linears.11.weight") / np.sqrt(f("linears.11.running_var") + EPS)
    return dict(W=W, k=k, n=n, alpha=alpha, shift=shift, A2=A2, sh2=sh2,
                fc2=f("linears.10.weight").reshape(U, H), fc2_b=f("linears.10.bias"),
                inv3=inv3, rm3=f("linears.11.running_mean"), b3=f("linears.11.bias"),
                Wf=f("final.weight"), bf=f("final.bias"))


def _unit_out(tb, u, q):
    y2 = tb["sh2"][u] + tb["A2"][u] @ q
    z = tb["fc2"][u] @ np.maximum(y2, 0) + tb["fc2_b"][u]
    return max(tb["inv3"][u] * (z - tb["rm3"][u]) + tb["b3"][u], 0.0), y2


def _extreme(g, alpha):
    return g.max(axis=-1) if alpha >= 0 else g.min(axis=-1)


def ism(sd, codes):
    """codes (B,L) ints 0..3, 4 = N -> (logits (B,T), delta (B,T,4,L)), fp64."""
    tb = eval_tables(sd)
    W, k, n = tb["W"], tb["k"], tb["n"]
    U = W.shape[0]
    B, L = codes.shape
    T = tb["Wf"].shape[0]
    Wz = np.concatenate([W, np.zeros((U, 1, k))], axis=1)       # base 4 (N) contributes 0
    pend = min(L, POOL * n + k - 1)
    logits = np.zeros((B, T))
    delta = np.zeros((B, T, 4, L))
    for b in range(B):
        s = codes[b]
        dO = np.zeros((U, 4, L))
        o = np.zeros(U)
        for u in range(U):
            al, sh = tb["alpha"][u], tb["shift"][u]
            g = np.array([sum(Wz[u, s[j + t], t] for t in range(k)) for j in range(POOL * n)])
            ext = _extreme(g.reshape(n, POOL), al)
            q = np.exp(al * ext + sh)
            o[u], y2 = _unit_out(tb, u, q)
            for p in range(pend):
                jlo, jhi = max(0, p - k + 1), min(p, POOL * n - 1)
                ws = list(range(jlo // POOL, jhi // POOL + 1))
                for a in range(4):
                    if a == s[p]:
                        continue
                    gp = g.copy()
                    for j in range(jlo, jhi + 1):
                        gp[j] += Wz[u, a, p - j] - Wz[u, s[p], p - j]
                    dq = np.array([np.exp(al * _extreme(gp[POOL * w:POOL * w + POOL], al) + sh) - q[w]
                                   for w in ws])
                    y2p = y2 + tb["A2"][u][:, ws] @ dq
                    z = tb["fc2"][u] @ np.maximum(y2p, 0) + tb["fc2_b"][u]
                    dO[u, a, p] = max(tb["inv3"][u] * (z - tb["rm3"][u]) + tb["b3"][u], 0.0) - o[u]
        logits[b] = tb["Wf"] @ o + tb["bf"]
        delta[b] = np.einsum("tu,uap->tap", tb["Wf"], dO)
    return logits, delta


def onehot(codes):
    B, L = codes.shape
    x = np.zeros((B, 4, L))
    for a in range(4):
        x[:, a, :] = codes == a
    return x


def brute_force(sd, codes):
    """delta by running the oracle's fp64 forward on all 4L substituted copies of every sequence."""
    B, L = codes.shape
    x = onehot(codes)
    base = orc.forward(sd, x, dtype=np.float64)
    T = base.shape[1]
    delta = np.zeros((B, T, 4, L))
    for b in range(B):
        mut = np.repeat(x[b:b + 1], 4 * L, axis=0)
        for a in range(4):
            for p in range(L):
                mut[a * L + p, :, p] = 0
                mut[a * L + p, a, p] = 1
        out = orc.forward(sd, mut, dtype=np.float64)              # (4L, T)
        delta[b] = (out - base[b]).reshape(4, L, T).transpose(2, 0, 1)
        for p in range(L):
            if codes[b, p] < 4:
                delta[b, :, codes[b, p], p] = 0.0
    return base, delta
