"""The algebra of the Integrated Gradients pass (explainn_amd/csrc/pathgrad.hip) in numpy fp64.

The convolution is linear in x, so along x_a = x' + a (x - x') the raw conv sums are
g_a = g' + a (g - g'); only BatchNorm1 (affine in eval mode), exp, MaxPool(7,7), the per-unit FC and the
head are evaluated per node a_s = (s + 1/2)/S.  With D_a = dF/dg_a (non-zero at each pooled window's
argmax: first index on a tie, the minimum where BatchNorm1's scale is negative), F = sum_t dl logit_t:
    G  = (1/S) sum_s D_(a_s)
    IG = (x - x') * transposed_conv(W, G)
The model itself uses no torch and no autograd.  brute_force() below is the reference it is held
against (tests/test_pathgrad_model.py) and the GPU tests compare with: autograd at every soft input."""
import numpy as np

EPS = 1e-5
POOL = 7
FC_H = 100


def codes_to_dense(codes):
    """(B,L) codes -> (B,4,L) fp64: 0..3 one-hot, 4 an all-zero column, 5 a column of 0.25."""
    codes = np.asarray(codes)
    x = np.zeros((codes.shape[0], 4, codes.shape[1]))
    for a in range(4):
        x[:, a] = (codes == a) + 0.25 * (codes == 5)
    return x


def baseline_dense(kind, x):
    """'zero' / 'uniform' / a (B,L) code array -> the dense baseline of x's shape."""
    if isinstance(kind, str):
        return np.zeros_like(x) if kind == "zero" else np.full_like(x, 0.25)
    return codes_to_dense(kind)


def conv_sums(W, x):
    """g[b,u,j] = sum_(a,t) W[u,a,t] x[b,a,j+t] (no bias: BatchNorm1's shift carries it)."""
    win = np.lib.stride_tricks.sliding_window_view(x, W.shape[2], axis=2)      # (B,4,Lo,k)
    return np.einsum("bajt,uat->buj", win, W)


def _tables(sd):
    f = lambda key: np.asarray(sd[key], dtype=np.float64)
    W = f("linears.0.weight")
    U = W.shape[0]
    al = f("linears.1.weight") / np.sqrt(f("linears.1.running_var") + EPS)
    sh = f("linears.1.bias") + al * (f("linears.0.bias") - f("linears.1.running_mean"))
    V1 = f("linears.6.weight").reshape(U, FC_H, -1)
    s2 = (f("linears.7.weight") / np.sqrt(f("linears.7.running_var") + EPS)).reshape(U, FC_H)
    A2 = V1 * s2[:, :, None]
    sh2 = f("linears.7.bias").reshape(U, FC_H) + s2 * (f("linears.6.bias") - f("linears.7.running_mean")).reshape(U, FC_H)
    V2 = f("linears.10.weight").reshape(U, FC_H)
    s3 = f("linears.11.weight") / np.sqrt(f("linears.11.running_var") + EPS)
    sh3 = f("linears.11.bias") + s3 * (f("linears.10.bias") - f("linears.11.running_mean"))
    return W, al, sh, A2, sh2, V2, s3, sh3, f("final.weight"), f("final.bias")


def _node(tabs, g, dl):
    """Forward behind the convolution at conv sums g (B,U,Lo); returns (logits, D = dF/dg) with
    D = None when dl is None."""
    W, al, sh, A2, sh2, V2, s3, sh3, Wf, bf = tabs
    B, U, Lo = g.shape
    n = Lo // POOL
    gw = g[:, :, :POOL * n].reshape(B, U, n, POOL)
    sg = np.where(al < 0, -1.0, 1.0)[None, :, None, None]
    idx = (sg * gw).argmax(axis=3)                                   # first index on a tie
    ext = np.take_along_axis(gw, idx[..., None], axis=3)[..., 0]
    q = np.exp(al[None, :, None] * ext + sh[None, :, None])
    y2 = np.einsum("urw,buw->bur", A2, q) + sh2[None]
    z = np.einsum("ur,bur->bu", V2, np.maximum(y2, 0))
    y3 = s3[None] * z + sh3[None]
    logits = np.maximum(y3, 0) @ Wf.T + bf[None]
    if dl is None:
        return logits, None
    dz = (dl @ Wf) * (y3 > 0) * s3[None]
    e = dz[:, :, None] * V2[None] * (y2 > 0)
    dq = np.einsum("urw,bur->buw", A2, e)
    dy = al[None, :, None] * q * dq
    D = np.zeros((B, U, n, POOL))
    np.put_along_axis(D, idx[..., None], dy[..., None], axis=3)
    Dg = np.zeros_like(g)
    Dg[:, :, :POOL * n] = D.reshape(B, U, n * POOL)
    return logits, Dg


def integrated_gradients(sd, x, baseline, dl, steps):
    """x (B,4,L) one-hot fp64, baseline 'zero' / 'uniform' / (B,L) codes, dl (B,T).
    Returns (ig (B,4,L), logits_x, logits_base), fp64."""
    tabs = _tables(sd)
    W = tabs[0]
    x = np.asarray(x, dtype=np.float64)
    xb = baseline_dense(baseline, x)
    dl = np.asarray(dl, dtype=np.float64)
    g, gb = conv_sums(W, x), conv_sums(W, xb)
    G = np.zeros_like(g)
    for s in range(steps):
        a = (s + 0.5) / steps
        G += _node(tabs, gb + a * (g - gb), dl)[1]
    G /= steps
    B, _, L = x.shape
    k, Lo = W.shape[2], g.shape[2]
    dx = np.zeros((B, 4, L))
    for t in range(k):                                # dx[b,a,j+t] += sum_u W[u,a,t] G[b,u,j]
        dx[:, :, t:t + Lo] += np.einsum("ua,buj->baj", W[:, :, t], G)
    return (x - xb) * dx, _node(tabs, g, None)[0], _node(tabs, gb, None)[0]


# ---- the reference: brute force, never the algebra above ----
def brute_force(sd, x, xb, dl, steps, dtype=None):
    """(ig, F(x) - F(x')): the Riemann sum at the midpoint nodes, the mean over the nodes of autograd's
    x.grad of oracle/torch_ref.py at the soft input x_a times (x - x'), in torch `dtype` (fp64)."""
    import torch
    from oracle import torch_ref
    dtype = dtype or torch.float64
    npd = np.float64 if dtype == torch.float64 else np.float32
    sdt = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in sd.items() if "tracked" not in k}
    dlt = torch.tensor(np.asarray(dl), dtype=dtype)
    x, xb = np.asarray(x, dtype=npd), np.asarray(xb, dtype=npd)
    acc = np.zeros(x.shape)
    for s in range(steps):
        a = npd((s + 0.5) / steps)
        xt = torch.tensor(xb + a * (x - xb), dtype=dtype, requires_grad=True)
        (torch_ref.forward(sdt, xt, False, 0.0, None) * dlt).sum().backward()
        acc += xt.grad.numpy().astype(np.float64)
    with torch.no_grad():
        F = [(torch_ref.forward(sdt, torch.tensor(v, dtype=dtype), False, 0.0, None) * dlt).sum(dim=1).numpy()
             for v in (x, xb)]
    return acc / steps * (x.astype(np.float64) - xb), F[0].astype(np.float64) - F[1].astype(np.float64)


def knife_rows(sd, x, xb, steps, knife, gap=2e-6):
    """Sequences whose path holds a knife edge in the fp64 oracle's intermediates: at some node |y2| or
    |y3| below `knife` (a ReLU two correct fp32 implementations may open differently), or a pooled
    window whose two largest or two smallest conv sums differ by a non-zero amount below `gap` of the
    unit's largest |c| in the batch (an argmax two implementations may place differently; an exact
    tie follows the first-index rule and stays in)."""
    from oracle import explainn_oracle as orc
    x, xb = np.asarray(x, dtype=np.float64), np.asarray(xb, dtype=np.float64)
    B = x.shape[0]
    bad = np.zeros(B, dtype=bool)
    for s in range(steps):
        a = (s + 0.5) / steps
        _, cache, _ = orc.forward(sd, xb + a * (x - xb), dtype=np.float64, return_cache=True)
        bad |= np.abs(np.asarray(cache["y2"]).reshape(B, -1)).min(axis=1) < knife
        bad |= np.abs(np.asarray(cache["y3"]).reshape(B, -1)).min(axis=1) < knife
        c = np.asarray(cache["c"])
        U, n = c.shape[1], cache["n"]
        cs = np.sort(c[:, :, :POOL * n].reshape(B, U, n, POOL), axis=3)
        lim = gap * np.abs(c).max(axis=(0, 2))[None, :, None]
        for d in (cs[..., -1] - cs[..., -2], cs[..., 1] - cs[..., 0]):
            bad |= ((d > 0) & (d < lim)).any(axis=(1, 2))
    return bad
