"""mid_fused's per-bucket forms against the fp64 oracle, at the pooled lengths where its indexing can go
wrong.  The kernel writes T by destination (16-byte fragment rows of a 16-wide w tile and a 32-channel
k-step), the FC1 weight gradient on a [100][power of two] grid, and bounds its loops over w by the
bucket; so the cases sit on both sides of every w tile (15 / 16 / 17, 31 / 32 / 33, 48), on bucket
edges (26 = the flagship's, 31 -> 32, 33 -> 40), at one pooled position and at mid_fused's upper limit
72; n = 73 shows that mid_big takes over there.  U = 3 units, a ragged batch of 70, k = 5, one task.

Compared, with the helpers and bounds of parity_util (GRAD_TOL_ORACLE relative or 3x the reference's own
fp32 error, nothing looser): the gradient of the FC1 weights (linears.6.weight: mid writes it itself)
and the three that passB derives from mid's tables Ttf / Mff / k0' -- the filter gradient
(linears.0.weight) and BatchNorm1's weight and bias gradients (linears.1.*).  The CPU test checks,
on the oracle alone, that no compared row holds a ReLU knife edge, so every row gets the tight bound."""
import functools

import numpy as np
import pytest

import dispatch_model as dm
from oracle import explainn_oracle as orc
from parity_util import check_grads, close, knife_masks, model, oracle_step, _ORACLE_CACHES

U, K, T, B = 3, 5, 1, 70
POOLED = (1, 15, 16, 17, 26, 31, 32, 33, 48, 72, 73)
KEYS = ("linears.0.weight", "linears.1.weight", "linears.1.bias", "linears.6.weight")


def _length(n):
    return dm.C["POOLW"] * n + K - 1 + n % dm.C["POOLW"]      # ragged last window


@functools.lru_cache(maxsize=None)
def _case(n):
    """Inputs and the oracle's step for pooled length n, computed once and shared (read-only)."""
    # (seeds: 2800 + n, or 100 more where that one puts a pre-activation on a knife edge -- a choice made
    # on the oracle alone, which test_cases_are_what_they_claim re-checks)
    L, seed = _length(n), 2800 + n + (100 if n in (15, 48) else 0)
    rng = np.random.default_rng(seed)
    sd = orc.random_state_dict(U, K, L, T, seed=seed)
    # |gamma1| away from zero, one unit pooling the minimum (see tests/test_gpu_dispatch_sweep.py)
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, U) * np.where(np.arange(U) % 2, 1, -1)).astype(np.float32)
    x = orc.random_onehot(B, L, seed=seed + 1, n_frac=0.01)
    y = (rng.random((B, T)) > 0.5).astype(np.float32)
    ref_logits, ref_loss, grads, _ = oracle_step(sd, x, y)
    for a in (x, y, ref_logits):
        a.setflags(write=False)
    return sd, x, y, ref_logits, ref_loss, grads


@pytest.mark.parametrize("n", POOLED)
def test_cases_are_what_they_claim(n):
    """CPU: the shape gives the pooled length and the form, and the oracle alone leaves every compared
    row off the ReLU knife edges."""
    L = _length(n)
    assert dm.check_supported(U, K, L, T) == n and dm.pooled_len(L, K) == n
    assert (n <= dm.C["MID_FUSED_MAX_N"]) == (n != 73)
    grads = _case(n)[5]
    cache = _ORACLE_CACHES[id(grads)][0]
    ch, un = knife_masks(cache, U)
    assert not ch.any() and not un.any(), (n, int(ch.sum()), un)
    assert set(KEYS) <= set(grads)


@pytest.mark.gpu
@pytest.mark.parametrize("n", POOLED)
def test_mid_forms_vs_oracle(n):
    torch = pytest.importorskip("torch")
    from explainn_amd.engine import StepEngine
    sd, x, y, ref_logits, ref_loss, grads = _case(n)
    L = _length(n)
    m = model(sd, U, K, L, T).train()
    m.dropout_p = 0.0
    eng = StepEngine(m, B, loss="binary")
    logits, loss = eng.step(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda())
    torch.cuda.synchronize()
    label = "mid n=%d " % n
    close(logits.detach().cpu().numpy(), ref_logits, what=label + "logits")
    close(loss.item(), ref_loss, tol=1e-5, what=label + "loss")
    named = [(name, g) for (name, _), g in zip(m.named_parameters(), eng.views) if name in KEYS]
    assert sorted(name for name, _ in named) == sorted(KEYS)
    check_grads(named, grads, label)
