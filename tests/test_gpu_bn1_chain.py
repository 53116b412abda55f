"""BatchNorm1's statistics chain on the filter bank's auxiliary workgroups (convpool.hip, cpm_bn1) at
the edges of its dealing: phase 1 deals 8k items (gap d, base a, pair of partner bases) over `naux`
workgroups and scans several 64-position passes side by side; phase 2 folds two units per workgroup,
their scalars fetched up front and the two folds finished on lanes 0 and 1.

Each case runs one train step with the workgroups forced on (EXPLAINN_BN1_AUX = N) and the same step
with the separate moments / prep1_stats launches (EXPLAINN_BN1_AUX = 0) and asserts the same bits:
logits, every gradient, running_mean / running_var, num_batches_tracked.  The timeout bit of the
flags word must stay 0.  One case per kernel form is also held to the fp64 oracle.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import check_grads, close, close_rel, GRAD_TOL_ORACLE, model, oracle_step, to_np  # noqa: E402

pytestmark = pytest.mark.gpu

FLAG_BN1_TIMEOUT = 2       # include/explainn_hip.h: EXPLAINN_FLAG_BN1_TIMEOUT


def _case(U, k, L, B, aux=None, n_frac=0.01, staged=False, ut=None, oracle=False):
    return dict(U=U, k=k, L=L, B=B, aux=8 * k if aux is None else aux, n_frac=n_frac, staged=staged, ut=ut,
                oracle=oracle)


CASES = (
    # naux against the 8k items and the unit loop: one workgroup does everything, a count that divides
    # nothing, one short of the items, the default, the clamp
    [_case(40, k, 200, 96, aux=a) for k in (5, 19) for a in (1, 3, 8 * k - 1, 8 * k, 256)]
    + [
        # units per workgroup: one unit, fewer units than workgroups, not a multiple of 2 naux
        _case(1, 19, 200, 64),
        _case(5, 19, 200, 64),
        _case(45, 19, 200, 100, aux=8, n_frac=0.05),
        # position passes and where P(j - 1) and P(j + Lo - 1) fall
        _case(40, 32, 40, 96),            # Lo = 9 < k: both in the first pass
        _case(40, 19, 64, 96),
        _case(40, 19, 65, 96),
        _case(40, 19, 129, 96),
        _case(40, 19, 257, 96),
        # lane columns of phase 2: K4 = 8, 64 (exactly one column), 68, 128
        _case(40, 2, 200, 96, oracle=True),
        _case(40, 16, 200, 96),
        _case(40, 17, 200, 96),
        _case(40, 32, 200, 96),
        # kernel forms: two unit tiles per wave and one for k <= 20, the k > 20 forms
        _case(40, 19, 200, 130, ut=2, oracle=True),
        _case(40, 19, 200, 130, ut=1, oracle=True),
        _case(40, 5, 200, 64, ut=1),
        _case(40, 21, 200, 130, oracle=True),
        # many N bases; staged base codes
        _case(33, 20, 200, 100, n_frac=0.05),
        _case(40, 21, 200, 130, staged=True),
    ]
)


def _id(c):
    return "U%d_k%d_L%d_B%d_aux%d%s%s%s" % (c["U"], c["k"], c["L"], c["B"], c["aux"], "_ut%d" % c["ut"] if c["ut"] else "",
                                          "_codes" if c["staged"] else "", "_n05" if c["n_frac"] > 0.01 else "")


def _state(U, k, L, seed):
    rng = np.random.default_rng(seed)
    sd = orc.random_state_dict(U, k, L, 1, seed=seed)
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, U) * np.where(np.arange(U) % 2, 1, -1)).astype(np.float32)
    sd["linears.1.running_mean"] = rng.normal(0, 0.5, U).astype(np.float32)
    sd["linears.1.running_var"] = rng.uniform(0.5, 2.0, U).astype(np.float32)
    return sd


def _inputs(c, seed=7):
    x = orc.random_onehot(c["B"], c["L"], seed=seed, n_frac=c["n_frac"])
    y = (np.random.default_rng(seed + 3).random((c["B"], 1)) > 0.5).astype(np.float32)
    return x, y


def _step(m, x, y, staged):
    """one train step (no optimiser step) of m; logits, gradients, buffers and the flags word"""
    from explainn_amd.architectures import BaseCodes
    if staged:
        codes = x.argmax(axis=1).astype(np.uint8)
        codes[x.sum(axis=1) == 0] = 4
        xin = BaseCodes(torch.from_numpy(codes).cuda(), False)
    else:
        xin = torch.from_numpy(x).cuda()
    m.zero_grad(set_to_none=True)
    logits = m(xin)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(y).cuda()).backward()
    torch.cuda.synchronize()
    grads = [(name, p.grad.detach().clone()) for name, p in m.named_parameters()]
    bufs = {key: v.detach().clone() for key, v in m.named_buffers()}
    return logits.detach().clone(), grads, bufs, m.input_flags()


def _fresh(sd, c):
    m = model(sd, c["U"], c["k"], c["L"], 1).train()
    m.dropout_p = 0.0
    return m


def _same(got, ref, what):
    logits, grads, bufs, _ = got
    logits0, grads0, bufs0, _ = ref
    assert torch.equal(logits, logits0), "logits differ from " + what
    for (name, g), (_, g0) in zip(grads, grads0):
        assert torch.equal(g, g0), "%s gradient differs from %s" % (name, what)
    assert set(bufs) == set(bufs0)
    for key in bufs:
        assert torch.equal(bufs[key], bufs0[key]), "%s differs from %s" % (key, what)


_SEPARATE = {}     # the step with the separate launches, once per (shape, form)


def _separate(c, sd, x, y, monkeypatch):
    key = (c["U"], c["k"], c["L"], c["B"], c["n_frac"], c["staged"], c["ut"])
    if key not in _SEPARATE:
        monkeypatch.setenv("EXPLAINN_BN1_AUX", "0")
        _SEPARATE[key] = _step(_fresh(sd, c), x, y, c["staged"])
    return _SEPARATE[key]


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_bn1_chain(c, monkeypatch):
    sd = _state(c["U"], c["k"], c["L"], seed=c["U"] + c["k"] + c["B"])
    x, y = _inputs(c)
    if c["ut"]:
        monkeypatch.setenv("EXPLAINN_CPM_UT", str(c["ut"]))
    monkeypatch.setenv("EXPLAINN_BN1_AUX", str(c["aux"]))
    got = _step(_fresh(sd, c), x, y, c["staged"])
    assert got[3] & FLAG_BN1_TIMEOUT == 0, "BatchNorm1 workgroups timed out"
    _same(got, _separate(c, sd, x, y, monkeypatch), "the separate launches")
    if c["oracle"]:
        logits, grads, bufs, _ = got
        ref_logits, _, ref_grads, nb = oracle_step(sd, x, y)
        close(to_np(logits), ref_logits, what="logits")
        check_grads(grads, ref_grads, "bn1 chain ")
        for key, v in nb.items():
            if "tracked" in key:
                assert int(bufs[key].item()) == int(v), key
            else:
                close_rel(to_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what=key)


@pytest.mark.parametrize("k,ut", [(19, 2), (19, 1), (21, None)], ids=["k19_ut2", "k19_ut1", "k21"])
def test_bn1_chain_used_context(k, ut, monkeypatch):
    """Stale state of the context (the ticket, G, m, Gw): a second step with other inputs on a used
    model equals, bit for bit, that step on a fresh model started from the same parameters and buffers."""
    c = _case(45, k, 200, 100, n_frac=0.05, ut=ut)
    sd = _state(c["U"], c["k"], c["L"], seed=11)
    x1, y1 = _inputs(c, seed=7)
    x2, y2 = _inputs(c, seed=19)
    if ut:
        monkeypatch.setenv("EXPLAINN_CPM_UT", str(ut))
    monkeypatch.setenv("EXPLAINN_BN1_AUX", str(c["aux"]))
    used = _fresh(sd, c)
    first = _step(used, x1, y1, False)
    assert first[3] & FLAG_BN1_TIMEOUT == 0, "BatchNorm1 workgroups timed out"
    sd1 = {key: to_np(v).copy() for key, v in used.state_dict().items()}
    second = _step(used, x2, y2, False)
    assert second[3] & FLAG_BN1_TIMEOUT == 0, "BatchNorm1 workgroups timed out"
    fresh = _step(_fresh(sd1, c), x2, y2, False)
    assert fresh[3] & FLAG_BN1_TIMEOUT == 0, "BatchNorm1 workgroups timed out"
    _same(second, fresh, "a fresh context")
    assert not torch.equal(first[0], second[0])          # (the two steps did differ)
