"""BatchNorm1's batch statistics computed inside the filter-bank launch (convpool.hip, cpm_bn1): the
input moments and the BatchNorm1 fold of a one-hot train forward run on workgroups of their own in
the conv_pool_mm launch instead of in two launches in front of it.

Each case runs train steps with the workgroups forced on (EXPLAINN_BN1_AUX=8k, the default count)
and checks them against the fp64 oracle (logits, gradients, running statistics,
num_batches_tracked), then runs the same step with the separate launches (EXPLAINN_BN1_AUX=0) and
asserts that both give the same bits.  The timeout bit of the flags word
must stay 0.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import check_grads, close, close_rel, GRAD_TOL_ORACLE, model, oracle_step, to_np  # noqa: E402

pytestmark = pytest.mark.gpu

FLAG_BN1_TIMEOUT = 2       # include/explainn_hip.h: EXPLAINN_FLAG_BN1_TIMEOUT

# (U, k, L, B, n_frac, staged codes)
CASES = [
    (40, 2, 200, 96, 0.01, False),
    (40, 5, 200, 96, 0.01, False),
    (300, 19, 200, 256, 0.01, False),
    (45, 20, 200, 100, 0.05, False),      # U and B off the tile sizes, many N bases
    (40, 21, 200, 130, 0.01, True),       # staged base codes (x == NULL)
    (40, 32, 200, 96, 0.01, False),
    (33, 19, 1000, 64, 0.01, False),
    (2000, 19, 200, 128, 0.01, False),    # more workgroups than the chip holds at once
]


def _state(U, k, L, seed):
    rng = np.random.default_rng(seed)
    sd = orc.random_state_dict(U, k, L, 1, seed=seed)
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, U) * np.where(np.arange(U) % 2, 1, -1)).astype(np.float32)
    sd["linears.1.running_mean"] = rng.normal(0, 0.5, U).astype(np.float32)
    sd["linears.1.running_var"] = rng.uniform(0.5, 2.0, U).astype(np.float32)
    return sd


def _steps(sd, U, k, L, x, y, staged, n):
    """n train steps (no optimiser step) of a fresh model; returns logits, gradients, buffers of the
    last one and the flags word"""
    from explainn_amd.architectures import BaseCodes
    m = model(sd, U, k, L, 1).train()
    m.dropout_p = 0.0
    if staged:
        codes = x.argmax(axis=1).astype(np.uint8)
        codes[x.sum(axis=1) == 0] = 4
        xin = BaseCodes(torch.from_numpy(codes).cuda(), False)
    else:
        xin = torch.from_numpy(x).cuda()
    yt = torch.from_numpy(y).cuda()
    for _ in range(n):
        m.zero_grad(set_to_none=True)
        logits = m(xin)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, yt).backward()
    torch.cuda.synchronize()
    grads = [(name, p.grad.detach().clone()) for name, p in m.named_parameters()]
    bufs = {key: v.detach().clone() for key, v in m.named_buffers()}
    return m, logits.detach().clone(), grads, bufs, m.input_flags()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "U%d_k%d_L%d_B%d%s" % (c[0], c[1], c[2], c[3], "_codes" if c[5] else ""))
def test_bn1_in_filter_bank(case, monkeypatch):
    U, k, L, B, n_frac, staged = case
    sd = _state(U, k, L, seed=U + k + B)
    x = orc.random_onehot(B, L, seed=7, n_frac=n_frac)
    y = (np.random.default_rng(3).random((B, 1)) > 0.5).astype(np.float32)
    ref_logits, _, ref_grads, nb = oracle_step(sd, x, y)

    # (forced on: by default small grids keep the separate launches)
    monkeypatch.setenv("EXPLAINN_BN1_AUX", str(8 * k))
    m, logits, grads, bufs, flags = _steps(sd, U, k, L, x, y, staged, 1)
    assert flags & FLAG_BN1_TIMEOUT == 0, "BatchNorm1 workgroups timed out"
    close(to_np(logits), ref_logits, what="logits")
    check_grads(grads, ref_grads, "bn1-in-filter-bank ")
    for key, v in nb.items():
        if "tracked" in key:
            assert int(bufs[key].item()) == int(v), key
        else:
            close_rel(to_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what=key)

    # several steps on the same batch: the running statistics follow the oracle's update step by step,
    # num_batches_tracked goes up by exactly one per step
    steps = 3
    m3, logits3, grads3, bufs3, flags3 = _steps(sd, U, k, L, x, y, staged, steps)
    assert flags3 & FLAG_BN1_TIMEOUT == 0, "BatchNorm1 workgroups timed out"
    sd_i = dict(sd)
    for _ in range(steps):
        _, _, nb_i = orc.forward(sd_i, x, training=True, return_cache=True)
        sd_i.update(nb_i)
    for key, v in nb_i.items():
        if "tracked" in key:
            assert int(bufs3[key].item()) == int(sd[key]) + steps, key
        else:
            close_rel(to_np(bufs3[key]), v, tol=GRAD_TOL_ORACLE, what="%d steps %s" % (steps, key))

    # the separate moments / prep1_stats launches give the same bits
    monkeypatch.setenv("EXPLAINN_BN1_AUX", "0")
    _, logits0, grads0, bufs0, _ = _steps(sd, U, k, L, x, y, staged, 1)
    assert torch.equal(logits, logits0), "logits differ from the separate launches"
    for (name, g), (_, g0) in zip(grads, grads0):
        assert torch.equal(g, g0), "%s gradient differs from the separate launches" % name
    for key in bufs:
        assert torch.equal(bufs[key], bufs0[key]), "%s differs from the separate launches" % key
