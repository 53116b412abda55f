"""Size-independent properties of the HIP path at BASELINE.json's full C2 size (300 units, 200 bp,
batch 1024) -- where the numpy oracle would take minutes -- plus edge cases.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import compare_masked as _compare_masked  # noqa: E402

pytestmark = pytest.mark.gpu
U, K, L, T, B = 300, 19, 200, 1, 1024


def _c2_model(seed=0, T_=T):
    from explainn_amd import ExplaiNN
    torch.manual_seed(seed)
    m = ExplaiNN(U, K, L, T_).cuda()
    with torch.no_grad():                       # move BN parameters off their defaults
        g = torch.Generator().manual_seed(seed + 1)
        for i in (1, 7, 11):
            bn = m.linears[i]
            # |gamma| in [0.6, 1.4]: a unit with gamma1 ~ 0 has q ~ constant, BatchNorm2 then divides
            # by sqrt(eps) and amplifies rounding -- ill-conditioned in the reference as well
            bn.weight.copy_((0.6 + 0.8 * torch.rand(bn.weight.shape, generator=g)).cuda())
            bn.bias.copy_((0.2 * torch.randn(bn.bias.shape, generator=g)).cuda())
        m.linears[1].weight[::3] *= -1          # some units pool with min
    m.dropout_p = 0.0
    return m


def _batch(seed=1, n_frac=0.002):
    return torch.from_numpy(orc.random_onehot(B, L, seed=seed, n_frac=n_frac)).cuda()


def _grads(m, x, y, scale=1.0):
    m.train()
    m.zero_grad()
    logits = m(x)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y) * scale
    loss.backward()
    return logits.detach(), [p.grad.clone() for p in m.parameters()]


def test_c2_batch_permutation_equivariance():
    """Permuting the sequences of a batch permutes train-mode logits the same way and leaves
    every gradient unchanged (batch statistics and sums are order-independent up to rounding)."""
    m = _c2_model()
    x = _batch()
    y = (torch.rand(B, T, generator=torch.Generator().manual_seed(3)) > 0.5).float().cuda()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    lg1, g1 = _grads(m, x, y)
    m.load_state_dict(sd0)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(4)).cuda()
    lg2, g2 = _grads(m, x[perm], y[perm])
    assert (lg1[perm] - lg2).abs().max().item() < 1e-4
    # Among the 30.7 M ReLU pre-activations of a C2 batch some lie within rounding of zero; a
    # different lane/tile assignment changes fp32 summation order in the batch statistics and may
    # flip such a sign.  The oracle's forward says which channels / units those are; everything
    # else must agree to 2e-4 of the tensor's max.
    sd_np = {k: v.cpu().numpy() for k, v in sd0.items()}
    _, cache, _ = orc.forward(sd_np, x.cpu().numpy(), training=True, return_cache=True, dtype=np.float64)
    ref = {name: a.cpu().numpy() for (name, _), a in zip(m.named_parameters(), g1)}
    _compare_masked([(name, b) for (name, _), b in zip(m.named_parameters(), g2)], ref, cache, U)


def test_c2_backward_is_linear_in_the_loss_gradient():
    """backward(2*dlogits) == 2*backward(dlogits) for all 14 gradients (same forward state)."""
    m = _c2_model()
    x = _batch(seed=5)
    y = (torch.rand(B, T, generator=torch.Generator().manual_seed(6)) > 0.5).float().cuda()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    _, g1 = _grads(m, x, y, scale=1.0)
    m.load_state_dict(sd0)
    _, g2 = _grads(m, x, y, scale=2.0)
    for (name, _), a, b in zip(m.named_parameters(), g1, g2):
        scale = max(1e-6, a.abs().max().item())
        assert (2 * a - b).abs().max().item() <= 1e-4 * scale + 1e-7, name


def test_c2_train_mode_ignores_pre_batchnorm_biases():
    """A bias in front of a train-mode BatchNorm cancels exactly: shifting linears.{0,6,10}.bias
    changes no train-mode logit (their gradients are identically zero)."""
    m = _c2_model()
    x = _batch(seed=7)
    m.train()
    with torch.no_grad():
        a = m(x).clone()
        m.linears[0].bias += 0.37
        m.linears[6].bias -= 0.21
        m.linears[10].bias += 1.5
        b = m(x)
    assert (a - b).abs().max().item() < 1e-4


def test_c2_eval_facade_consistency():
    """model(x) == final(linears(x_rep)) and linears[:3] has the reference's shape, at full size
    (test.py:148-160); predict-style strand handling: forward of the reverse complement equals
    forward of the flipped tensor by construction."""
    m = _c2_model().eval()
    x = _batch(seed=8)[:256]
    with torch.no_grad():
        logits = m(x)
        outs = m.linears(x.repeat(1, U, 1))
        assert outs.shape == (256, U)
        assert (m.final(outs) - logits).abs().max().item() < 1e-4
        acts = m.linears[:3](x[:8].repeat(1, U, 1))
        assert acts.shape == (8, U, L - K + 1) and torch.isfinite(acts).all()
        # max-pool of the activations reproduces what the fused path pooled: compare through q
        pooled = torch.nn.functional.max_pool1d(acts, 7, 7)
        assert pooled.shape == (8, U, (L - K + 1) // 7)


def test_c2_step_is_deterministic():
    """Two identical steps from the same state give bitwise-identical gradients (fixed-order partial
    sums, no float atomics)."""
    m = _c2_model()
    x = _batch(seed=9)
    y = (torch.rand(B, T, generator=torch.Generator().manual_seed(10)) > 0.5).float().cuda()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    lg1, g1 = _grads(m, x, y)
    m.load_state_dict(sd0)
    lg2, g2 = _grads(m, x, y)
    assert torch.equal(lg1, lg2)
    for (name, _), a, b in zip(m.named_parameters(), g1, g2):
        assert torch.equal(a, b), name


def test_edge_cases_small():
    from explainn_amd import ExplaiNN
    sd = orc.random_state_dict(5, 19, 200, 2, seed=2)
    m = ExplaiNN(5, 19, 200, 2)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m = m.cuda().eval()
    x = orc.random_onehot(70, 200, seed=3)
    x[3] = 0                                    # an all-N sequence (all-zero columns)
    x[4, :, :50] = 0                            # a long N run
    ref = orc.forward(sd, x)
    with torch.no_grad():
        one = m(torch.from_numpy(x[:1]).cuda())            # batch of one in eval mode is fine
        assert np.abs(one.cpu().numpy() - ref[:1]).max() < 1e-4
        small = m(torch.from_numpy(x[:3]).cuda())
        big = m(torch.from_numpy(x).cuda())                # larger batch: the context grows
        assert np.abs(small.cpu().numpy() - ref[:3]).max() < 1e-4
        assert np.abs(big.cpu().numpy() - ref).max() < 1e-4
        again = m(torch.from_numpy(x[:3]).cuda())
        assert torch.equal(small, again)
    with pytest.raises(RuntimeError, match="shape"):
        m(torch.zeros(2, 4, 199).cuda())
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 4, 200))                          # host tensor, model on device


def test_empty_batch_follows_torch():
    from explainn_amd import ExplaiNN
    m = ExplaiNN(4, 5, 40, 2).cuda()
    x0 = torch.zeros(0, 4, 40).cuda()
    assert tuple(m.eval()(x0).shape) == (0, 2)
    with pytest.raises(ValueError):
        m.train()(x0)


def test_c2_full_size_against_fp64_oracle():
    """Train-mode logits and all gradients at the full C2 size against the numpy oracle in fp64
    (a few seconds of host time).  Logits within 1e-4; every gradient within 2e-4 of the tensor's
    max, except the rows the oracle itself marks as ReLU knife-edges (parity_util.knife_masks)."""
    m = _c2_model(seed=3)
    x = _batch(seed=11)
    y = (torch.rand(B, T, generator=torch.Generator().manual_seed(12)) > 0.5).float().cuda()
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    logits, grads = _grads(m, x, y)
    ref_logits, cache, nb = orc.forward(sd, x.cpu().numpy(), training=True, return_cache=True,
                                        dtype=np.float64)
    _, dl = orc.bce_with_logits(ref_logits, y.cpu().numpy().astype(np.float64))
    ref = orc.backward(cache, dl)
    assert np.abs(logits.cpu().numpy() - ref_logits).max() < 1e-4
    _compare_masked([(name, g) for (name, _), g in zip(m.named_parameters(), grads)], ref, cache, U)
    bufs = dict(m.named_buffers())
    for key, v in nb.items():
        if "tracked" not in key:
            assert np.abs(bufs[key].cpu().numpy() - v).max() < 1e-4, key


def test_c3_batch_and_tasks_against_fp64_oracle():
    """Config C3's batch and task count (B = 4096, T = 50) at 32 units: the many-task head (MFMA
    GEMMs for logits, d o and d Wf with K = 32 / 50 / 4096), the multi-block loss reduction
    (B*T = 204 800 elements -> 25 blocks) and explainn_train_step's T > 4 branch, against the
    numpy oracle in fp64.  Same tolerances as the C2 full-size test."""
    from explainn_amd import ExplaiNN
    from explainn_amd.engine import StepEngine
    U3, T3, B3 = 32, 50, 4096
    torch.manual_seed(21)
    m = ExplaiNN(U3, K, L, T3).cuda().train()
    m.dropout_p = 0.0
    x = torch.from_numpy(orc.random_onehot(B3, L, seed=22, n_frac=0.002)).cuda()
    y = (torch.rand(B3, T3, generator=torch.Generator().manual_seed(23)) > 0.5).float().cuda()
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    eng = StepEngine(m, B3, loss="binary")
    logits, loss = eng.step(x, y)
    torch.cuda.synchronize()
    ref_logits, cache, _ = orc.forward(sd, x.cpu().numpy(), training=True, return_cache=True,
                                       dtype=np.float64)
    ref_loss, dl = orc.bce_with_logits(ref_logits, y.cpu().numpy().astype(np.float64))
    ref = orc.backward(cache, dl)
    assert np.abs(logits.cpu().numpy() - ref_logits).max() < 1e-4
    assert abs(loss.item() - ref_loss) < 1e-5
    _compare_masked([(name, g) for (name, _), g in zip(m.named_parameters(), eng.views)], ref, cache, U3)
    # the autograd path (torch's own BCE, explainn_backward) lands on the same gradients
    m.zero_grad()
    out = m(x)
    torch.nn.functional.binary_cross_entropy_with_logits(out, y).backward()
    assert torch.allclose(out, logits, atol=0, rtol=0)
    for (name, p), g in zip(m.named_parameters(), eng.views):
        assert torch.allclose(p.grad, g, rtol=1e-4, atol=1e-6 * float(g.abs().max()) + 1e-12), name


def _shard_case(Uc, Lc, Tc, Bc, seed):
    """One per-GPU shard of configs C4 / C5 (BASELINE.json configs[3], [4]: B = 1024 per GPU) at a
    handful of units, through explainn_train_step, against the fp64 oracle."""
    from explainn_amd import ExplaiNN
    from explainn_amd.engine import StepEngine
    torch.manual_seed(seed)
    m = ExplaiNN(Uc, K, Lc, Tc).cuda().train()
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for i in (1, 7, 11):
            bn = m.linears[i]
            bn.weight.copy_((0.6 + 0.8 * torch.rand(bn.weight.shape, generator=g)).cuda())
            bn.bias.copy_((0.2 * torch.randn(bn.bias.shape, generator=g)).cuda())
        m.linears[1].weight[::3] *= -1
    m.dropout_p = 0.0
    x = torch.from_numpy(orc.random_onehot(Bc, Lc, seed=seed + 2, n_frac=0.002)).cuda()
    y = (torch.rand(Bc, Tc, generator=torch.Generator().manual_seed(seed + 3)) > 0.5).float().cuda()
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    eng = StepEngine(m, Bc, loss="binary")
    logits, loss = eng.step(x, y)
    torch.cuda.synchronize()
    ref_logits, cache, nb = orc.forward(sd, x.cpu().numpy(), training=True, return_cache=True,
                                        dtype=np.float64)
    ref_loss, dl = orc.bce_with_logits(ref_logits, y.cpu().numpy().astype(np.float64))
    ref = orc.backward(cache, dl)
    assert np.abs(logits.cpu().numpy() - ref_logits).max() < 1e-4
    assert abs(loss.item() - ref_loss) < 1e-5
    rep = _compare_masked([(name, g) for (name, _), g in zip(m.named_parameters(), eng.views)],
                          ref, cache, Uc)
    bufs = dict(m.named_buffers())
    for key, v in nb.items():
        if "tracked" not in key:
            assert np.abs(bufs[key].cpu().numpy() - v).max() < 1e-4 * max(1.0, np.abs(v).max()), key
    return rep


def test_c4_shard_shape_against_fp64_oracle():
    """Config C4's per-GPU shard: L = 1000 (n = 140), T = 50, B = 1024 -- qmom_big / mid_big /
    passB<140> / fc_fwd<140> with all 8 q-moment chunks and 8 passA chunks live."""
    _shard_case(8, 1000, 50, 1024, seed=31)


def test_c5_shard_shape_against_fp64_oracle():
    """Config C5's per-GPU shard: L = 600 (n = 83 -> bucket 84), T = 164, B = 1024."""
    _shard_case(8, 600, 164, 1024, seed=41)


@pytest.mark.parametrize("Bc", [128, 1024])
def test_c5_unit_count_determinism_and_unit_permutation(Bc):
    """U = 2000 (config C5): a grid of 2000 units and size_t offsets into ext / dy / partials.
    At Bc = 1024 this is the FULL per-GPU shard of config C5 (U = 2000, L = 600, T = 164,
    B = 1024; 2.7 GB of scratch): ext / dy are 2000 x 83 x 1088 x 4 B = 722 MB each and the
    passA partials U x ACH x 100 x NS floats, so element offsets times 4 exceed 2^31 bytes in
    several arrays -- the combination no oracle-sized test reaches.  Two identical steps are
    bitwise identical, and permuting the units (every per-unit parameter row together with its
    column of final.weight) permutes every per-unit gradient the same way and leaves the logits
    unchanged to 1e-4: a unit whose indexing wrapped or aliased another's scratch would break
    either property."""
    from explainn_amd import ExplaiNN
    from explainn_amd.engine import StepEngine
    Uc, Lc, Tc = 2000, 600, 164
    torch.manual_seed(51)
    m = ExplaiNN(Uc, K, Lc, Tc).cuda().train()
    m.dropout_p = 0.0
    x = torch.from_numpy(orc.random_onehot(Bc, Lc, seed=52, n_frac=0.002)).cuda()
    y = (torch.rand(Bc, Tc, generator=torch.Generator().manual_seed(53)) > 0.5).float().cuda()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    eng = StepEngine(m, Bc, loss="binary")
    lg1, _ = eng.step(x, y)
    lg1 = lg1.clone(); g1 = [v.clone() for v in eng.views]
    m.load_state_dict(sd0)
    lg2, _ = eng.step(x, y)
    assert torch.equal(lg1, lg2)
    for (name, _), a, b in zip(m.named_parameters(), g1, eng.views):
        assert torch.equal(a, b), name
        assert torch.isfinite(a).all(), name
    # unit permutation
    perm = torch.randperm(Uc, generator=torch.Generator().manual_seed(54)).cuda()
    n = m._n
    sdp = {}
    for key, v in sd0.items():
        if key.startswith("linears.6.") or key.startswith("linears.7."):
            if v.dim() == 0:
                sdp[key] = v.clone()
            else:
                sdp[key] = v.reshape((Uc, 100) + tuple(v.shape[1:]))[perm].reshape(v.shape).clone()
        elif key == "final.weight":
            sdp[key] = v[:, perm].clone()
        elif key == "final.bias" or v.dim() == 0:
            sdp[key] = v.clone()
        else:
            sdp[key] = v[perm].clone()
    m.load_state_dict(sdp)
    lg3, _ = eng.step(x, y)
    assert (lg1 - lg3).abs().max().item() < 1e-4
    for (name, _), a, b in zip(m.named_parameters(), g1, eng.views):
        if name.startswith(("linears.6.", "linears.7.")):
            ap = a.reshape((Uc, 100) + tuple(a.shape[1:]))[perm].reshape(a.shape)
        elif name == "final.weight":
            ap = a[:, perm]
        elif name == "final.bias":
            ap = a
        else:
            ap = a[perm]
        scale = max(1e-6, a.abs().max().item())
        # units are independent until `final`: a permuted unit sees exactly the same inputs, so its
        # gradients are bitwise those of the unpermuted run; only what sums over units (the logits,
        # hence dlogits and everything scaled by them) moves by rounding
        assert (ap - b).abs().max().item() <= 2e-4 * scale + 1e-9, name
