"""CPU check of the input-gradient algebra the kernels use (csrc/inputgrad.hip, DESIGN.md section 3
item 10): an fp64 numpy restatement of the three terms -- the sparse term at the pooling argmax, the
constant table and the H_p tables of the train-mode g term -- against torch.autograd's x.grad on the
stock-PyTorch restatement of the reference forward (oracle/torch_ref.py) in float64.  Plus the C-ABI
declarations and exports of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import explainn_oracle as orc
from oracle import torch_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sd64(U, k, L, T, seed, neg_gamma):
    sd = orc.random_state_dict(U, k, L, T, seed=seed)
    sdt = {key: torch.tensor(np.asarray(v, dtype=np.float64)) for key, v in sd.items() if "tracked" not in key}
    if neg_gamma:
        sdt["linears.1.weight"][::2] *= -1          # every other unit pools the minimum
    return sdt


def _autograd(sdt, x, training, keep, dl):
    """x.grad of torch_ref.forward and dL/d(BatchNorm1 output), fp64."""
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    sd = {key: v.clone() for key, v in sdt.items()}
    store = {}
    orig = torch.nn.functional.batch_norm

    def bn_hook(t, *a, **kw):
        out = orig(t, *a, **kw)
        if "y1" not in store:                       # the first BatchNorm is BN1
            out.retain_grad()
            store["y1"] = out
        return out

    torch.nn.functional.batch_norm = bn_hook
    try:
        logits = torch_ref.forward(sd, xt, training, 0.3 if keep is not None else 0.0,
                                   None if keep is None else torch.tensor(keep))
    finally:
        torch.nn.functional.batch_norm = orig
    (logits * torch.tensor(dl)).sum().backward()
    return xt.grad.numpy(), store["y1"].grad.numpy()


def _model_dx(sdt, x, dy, training):
    """The kernels' algebra in numpy fp64: dy (B,U,Lo) nonzero at the argmax positions only."""
    W = sdt["linears.0.weight"].numpy(); cb = sdt["linears.0.bias"].numpy()
    g1 = sdt["linears.1.weight"].numpy()
    U, _, k = W.shape
    B, _, L = x.shape
    Lo = L - k + 1
    N = B * Lo
    # raw conv sum g (no bias)
    win = np.stack([x[:, :, t:t + Lo] for t in range(k)], axis=-1)            # (B,4,Lo,k)
    g = np.einsum("batk,uak->but", win, W)                                     # (B,U,Lo)
    if training:
        mu = g.mean(axis=(0, 2))
        sig = np.sqrt(g.var(axis=(0, 2)) + 1e-5)
    else:
        mu = sdt["linears.1.running_mean"].numpy() - cb
        sig = np.sqrt(sdt["linears.1.running_var"].numpy() + 1e-5)
    alpha = g1 / sig
    dx = np.zeros_like(x)
    # 1. sparse term: alpha dy W[u,:,t] at p* + t
    for t in range(k):
        dx[:, :, t:t + Lo] += np.einsum("buj,ua->baj", alpha[None, :, None] * dy, W[:, :, t])
    if not training:
        return dx
    chat = (g - mu[None, :, None]) / sig[None, :, None]
    S1 = dy.sum(axis=(0, 2)); S2 = (dy * chat).sum(axis=(0, 2))
    c = -alpha * S2 / (sig * N)
    kk = -alpha * S1 / N - c * mu
    D = 2 * k - 1
    P = np.zeros((D, 4, 4, k))                      # [d][a'][a][t]
    for d in range(D):
        for t in range(k):
            t2 = t + d - (k - 1)
            if 0 <= t2 < k:
                P[d, :, :, t] = np.einsum("u,ua,ub->ba", c, W[:, :, t], W[:, :, t2])
    R = np.einsum("u,uat->at", kk, W)
    for p in range(L):
        tlo, thi = max(0, p - Lo + 1), min(k - 1, p)
        # 2. the constant table, 3. the H_p table
        dx[:, :, p] += R[:, tlo:thi + 1].sum(axis=1)[None, :]
        H = P[:, :, :, tlo:thi + 1].sum(axis=-1)                              # [d][a'][a]
        for d in range(D):
            q = p + d - (k - 1)
            if 0 <= q < L:
                dx[:, :, p] += x[:, :, q] @ H[d]
    return dx


def _classes_are_distinct(k, L):
    Lo = L - k + 1
    pairs = {}
    for p in range(L):
        pr = (max(0, p - Lo + 1), min(k - 1, p))
        cls = pr[0] + pr[1]
        assert pairs.setdefault(cls, pr) == pr
    assert len(pairs) <= 2 * k - 1


CASES = [
    # U, k, L, T, B, seed, input kind
    (5, 7, 60, 2, 9, 0, "poly_a"),
    (3, 2, 40, 1, 6, 1, "n_bases"),
    (4, 19, 64, 3, 5, 2, "soft"),
    (2, 32, 50, 1, 4, 3, "onehot"),          # Lo = 19: Lo mod 7 != 0 and Lo < k
    (3, 5, 47, 2, 7, 4, "onehot"),           # Lo = 43: positions past 7n get only the dense terms
]


def _input(kind, B, L, seed):
    if kind == "soft":
        return np.random.default_rng(seed).random((B, 4, L))
    x = orc.random_onehot(B, L, seed=seed, n_frac=0.1 if kind == "n_bases" else 0.0).astype(np.float64)
    if kind == "poly_a":
        x[:, :, 10:40] = 0
        x[:, 0, 10:40] = 1
        x[:, :, 45:48] = 0                      # N run
    return x


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_three_terms_match_autograd(case, training):
    U, k, L, T, B, seed, kind = case
    torch.set_num_threads(4)
    sdt = _sd64(U, k, L, T, seed, neg_gamma=True)
    x = _input(kind, B, L, seed + 10)
    dl = np.random.default_rng(seed + 20).standard_normal((B, T))
    keep = None
    if training:
        keep = (np.random.default_rng(seed + 30).random((B, 100 * U)) > 0.3).astype(np.float64)
    ref, dy = _autograd(sdt, x, training, keep, dl)
    dx = _model_dx(sdt, x, dy, training)
    scale = np.abs(ref).max()
    assert scale > 0
    assert np.abs(dx - ref).max() <= 1e-10 * scale, (np.abs(dx - ref).max(), scale)
    _classes_are_distinct(k, L)


def test_header_declares_and_library_exports_input_grad():
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(explainn_[a-z_]+)\s*\(", text))
    new = ("explainn_forward_eval_keep", "explainn_input_grad", "explainn_backward_input")
    for name in new:
        assert name in declared, name
    import __graft_entry__ as g
    g.build()
    from explainn_amd import _lib
    lib = _lib.load()
    for name in new:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    from explainn_amd import interpret
    assert callable(interpret.input_gradients)
