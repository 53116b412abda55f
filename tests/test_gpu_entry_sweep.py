"""The entry points that came after the train step, at their own dispatch edges: in-silico
mutagenesis (csrc/ism.hip), the input gradient (csrc/inputgrad.hip) and the head of a model bank
(csrc/head.hip with Gm > 1).  tests/dispatch_model.py builds the case lists from the constants it reads
in the sources, and tests/test_dispatch_coverage.py checks on CPU that they reach every form.

  ISM    both kernel sizes at every change of ism_units_kernel<NW>, the task chunks of ism_sum_kernel,
         one window, two trips of the sub-batch loop                         vs the fp64 oracle on every
         substituted sequence (TOL of tests/test_gpu_ism.py); the sub-batch case vs the device forward
  IG     fc_ng row groups of passB's partials, several batch chunks, unit / batch / kernel-size / tail
         edges, eval, train and soft input                  vs torch.autograd on the fp64 reference
         (the rule of tests/test_gpu_input_grad.py, with the knife-edge exclusion capped)
  bank   looped and register bodies of head_bwd_kernel, head_fwd_train's three branches, second trips of
         the combiner kernels' unit loops, the task thresholds            member by member vs the fp64
         oracle (parity_util's bounds; B >= 2048: compare_masked); the unit limit vs bank.member(g)

References are never the code under test."""
import copy

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dispatch_model as dm  # noqa: E402
import test_gpu_bank as bank_t  # noqa: E402
import test_gpu_dispatch_sweep as sweep  # noqa: E402
import test_gpu_input_grad as ig_t  # noqa: E402
import test_gpu_ism as ism_t  # noqa: E402
from conftest import record_margin  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import (GRAD_TOL_GOLDEN, GRAD_TOL_ORACLE, TOL, check_grads, close, close_rel,  # noqa: E402
                         compare_masked, model, to_np)
from tests import ism_model  # noqa: E402

gpu = pytest.mark.gpu


def _ids(cases):
    return [c.id for c in cases]


# ---- in-silico mutagenesis ------------------------------------------------------------------------
ISM_ORACLE = [c for c in dm.ISM_CASES if c.ref == "oracle"]
ISM_DEVICE = [c for c in dm.ISM_CASES if c.ref == "device"]


def _ism_exact_zeros(delta, codes, k):
    """Reference-base rows and the positions no pooled window reaches are exactly 0."""
    L = codes.shape[1]
    pend = min(L, dm.C["POOLW"] * dm.pooled_len(L, k) + k - 1)
    assert np.all(delta[:, :, :, pend:] == 0), "a position past the last pooled window's reach is not 0"
    bs, ps = np.nonzero(codes < 4)
    assert np.all(delta[bs, :, codes[bs, ps], ps] == 0), "a reference-base row is not 0"


@gpu
@pytest.mark.parametrize("c", ISM_ORACLE, ids=_ids(ISM_ORACLE))
def test_ism_edges_vs_oracle(c):
    sd, codes = ism_t._case(c.U, c.k, c.L, c.T, c.B, seed=c.seed)
    m = model(sd, c.U, c.k, c.L, c.T).eval()
    logits, delta = ism_t._ism(m, torch.tensor(codes, device="cuda"))
    base, ref = ism_model.brute_force(sd, codes)
    err = np.abs(delta - ref).max()
    print("%s: max |delta - oracle| = %.3e" % (c.id, err))
    record_margin("ism_vs_oracle", err, ism_t.TOL)
    assert err <= ism_t.TOL, "%s: max |delta - oracle| = %.3g" % (c.id, err)
    assert np.abs(logits - base).max() <= ism_t.TOL
    _ism_exact_zeros(delta, codes, c.k)


@gpu
@pytest.mark.parametrize("c", ISM_DEVICE, ids=_ids(ISM_DEVICE))
def test_ism_several_subbatches_vs_device_forward(c):
    """Two trips of launch_ism's sub-batch loop, the second with b0 > 0, fewer live sequences than the
    dout plane stride: the first and last sequence of either trip against the device forward on their
    materialised mutants."""
    S = dm.ism_sub_batch(c.U, c.L, c.B)
    assert S == dm.C["ISM_SUB_STEP"] < c.B < 2 * S
    sd, codes = ism_t._case(c.U, c.k, c.L, c.T, c.B, seed=c.seed)
    m = model(sd, c.U, c.k, c.L, c.T).eval()
    ctx = m._context(c.B, m._device())
    assert int(ctx.lib.explainn_ism_workspace_bytes(ctx.handle, c.B)) == dm.ism_workspace_bytes(c.U, c.L, c.B)
    logits, delta = ism_t._ism(m, torch.tensor(codes, device="cuda"))
    rows = [0, S - 1, S, c.B - 1]
    base, ref = ism_t._device_brute(m, codes, rows)
    err = np.abs(delta[rows] - ref).max()
    print("%s: max |delta - brute force| = %.3e" % (c.id, err))
    record_margin("ism_vs_device_brute_force", err, ism_t.TOL)
    assert err <= ism_t.TOL, "max |delta - brute force| = %.3g" % err
    assert np.array_equal(logits, base)
    _ism_exact_zeros(delta, codes, c.k)


# ---- the input gradient ---------------------------------------------------------------------------
def _ig_inputs(c):
    sd, x, dl = ig_t._case(c.U, c.k, c.L, c.T, c.B, seed=c.seed)
    rng = np.random.default_rng(c.seed + 3)
    keep = None
    if c.mode != "eval":
        keep = (rng.random((c.B, 100 * c.U)) > 0.3).astype(np.uint8)
    if c.mode == "train_dense":
        x = rng.dirichlet(np.ones(4) * 0.3, size=(c.B, c.L)).transpose(0, 2, 1).astype(np.float32)
        x = np.ascontiguousarray(x)
    return sd, x, dl, keep


@pytest.mark.parametrize("c", dm.IG_CASES, ids=_ids(dm.IG_CASES))
def test_input_grad_seeds_stay_inside_the_knife_edge_cap(c):
    """CPU, the oracle alone: the sequences the comparison leaves out (a ReLU knife edge in the fp64
    intermediates) are at most a quarter of the batch and leave at least two, for every case's seed."""
    sd, x, _, keep = _ig_inputs(c)
    knife = ig_t._knife_rows(sd, x, c.mode != "eval", None if keep is None else keep.astype(np.float64))
    assert ig_t._within_cap(knife), "%s: %d of %d sequences hold a knife edge" % (c.id, knife.sum(), c.B)


@gpu
@pytest.mark.parametrize("c", dm.IG_CASES, ids=_ids(dm.IG_CASES))
def test_input_grad_edges_vs_oracle(c):
    sd, x, dl, keep = _ig_inputs(c)
    m = model(sd, c.U, c.k, c.L, c.T)
    if c.mode == "eval":
        dx, _ = ig_t._eval_dx(m.eval(), x, dl)
        ig_t._check(dx, sd, x, False, None, dl, c.id, cap=True)
        pend = dm.C["POOLW"] * dm.pooled_len(c.L, c.k) + c.k - 1
        assert np.all(dx[:, :, pend:] == 0), "eval: a position no pooled window reaches has a gradient"
        return
    if c.mode == "train_dense":
        m.dense_input = True
    dx, _ = ig_t._train_dx(m, x, dl, keep)
    ig_t._check(dx, sd, x, True, keep.astype(np.float64), dl, c.id, cap=True)


# ---- the head of a model bank ---------------------------------------------------------------------
def _bank_inputs(c):
    """Member state dicts and the shared batch, by the dispatch sweep's _inputs (gamma1 bounded away
    from zero; from B = 1024 on BatchNorm2 / 3 shifted off zero, which keeps compare_masked's cap)."""
    base = dm.Case(c.id, "bank", c.U, c.k, c.L, c.T, c.B, ("step",), None, None, None, False, c.seed)
    _, x, y, _ = sweep._inputs(base)
    sds = [sweep._inputs(base._replace(seed=c.seed + 1 + 37 * g))[0] for g in range(c.G)]
    return sds, x, y


def _bank(c, sds):
    from explainn_amd import ExplaiNNBank
    return ExplaiNNBank.from_models([model(sd, c.U, c.k, c.L, c.T) for sd in sds]).cuda().train()


def _check_bank_member(c, label, bank, g, sd, x, y, keep_g, logits, loss, grads):
    ref_logits, ref_loss, ref_grads, nb, cache = sweep._oracle(c, sd, x, y, keep_g)
    close(to_np(logits[:, g]), ref_logits, what=label + " logits")
    close(float(loss[g]), float(ref_loss), what=label + " loss")
    named = bank_t._member_grads(bank, grads, g)
    if cache is None:
        check_grads(named, ref_grads, label + " ")
    else:
        rep = compare_masked(named, ref_grads, cache, c.U, tight=GRAD_TOL_ORACLE)
        for name, (clean, _) in rep.items():
            record_margin("rel %s masked grad %s" % (label, name), clean, GRAD_TOL_ORACLE)
    bufs = dict(bank.named_buffers())
    for key, v in nb.items():
        if "tracked" in key:
            assert int(bufs[key].item()) == int(v), key
        else:
            close_rel(to_np(bank._member_view(key, bufs[key], g)), v, tol=GRAD_TOL_GOLDEN, what=label + " " + key)


BANK_STEP = [c for c in dm.BANK_CASES if "step" in c.paths]
BANK_AUTOGRAD = [c for c in dm.BANK_CASES if "autograd" in c.paths]


@gpu
@pytest.mark.parametrize("c", BANK_STEP, ids=_ids(BANK_STEP))
def test_bank_head_step_vs_oracle(c):
    from explainn_amd.engine import StepEngine
    sds, x, y = _bank_inputs(c)
    bank = _bank(c, sds)
    bank.dropout_p = 0.0
    eng = StepEngine(bank, c.B, "binary")
    eng.ctx.stage_timing(True)
    logits, loss = eng.step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    stages = eng.ctx.stage_times()
    eng.ctx.stage_timing(False)
    assert "head_bwd" in stages and "head_fwd" in stages, stages        # never inside passA
    assert ("loss" in stages) == (c.T > dm.C["FUSED_LOSS_MAX_T"]), stages
    assert logits.shape == (c.B, c.G, c.T) and loss.shape == (c.G,)
    for g in range(c.G):
        _check_bank_member(c, "entry bank step m%d" % g, bank, g, sds[g], x, y, None, logits, loss, eng.views)


@gpu
@pytest.mark.parametrize("c", BANK_AUTOGRAD, ids=_ids(BANK_AUTOGRAD))
def test_bank_head_autograd_vs_oracle(c):
    """dlogits given (head_bwd_kernel<false, false>), under an explicit keep mask; member g against
    the oracle with its slice of the mask."""
    sds, x, y = _bank_inputs(c)
    bank = _bank(c, sds)
    keep = (np.random.default_rng(c.seed + 5).random((c.B, 100 * c.G * c.U)) > 0.3).astype(np.uint8)
    bank.set_dropout_mask(torch.from_numpy(keep))
    logits = bank(torch.from_numpy(x).cuda())
    yt = torch.from_numpy(y).cuda()
    losses = torch.stack([torch.nn.functional.binary_cross_entropy_with_logits(logits[:, g], yt)
                          for g in range(c.G)])
    losses.sum().backward()
    grads = [p.grad for p in bank.parameters()]
    for g in range(c.G):
        keep_g = np.ascontiguousarray(keep[:, 100 * c.U * g:100 * c.U * (g + 1)])
        _check_bank_member(c, "entry bank autograd m%d" % g, bank, g, sds[g], x, y, keep_g, logits.detach(),
                           losses.detach(), grads)


@gpu
def test_bank_at_the_unit_limit_vs_members():
    """A bank of BANK_MAX_UNITS units: its first, middle and last member against the stand-alone
    model's step (the existing single-model path) from the same parameters and batch."""
    from explainn_amd import ExplaiNNBank
    from explainn_amd.engine import StepEngine
    G, Um, k, L, T, B = dm.BANK_LIMIT
    assert G * Um == dm.C["BANK_MAX_UNITS"]
    c = bank_t.Case("limit", G, Um, k, L, T, B, "binary", 0, 0.0, False, False)
    torch.manual_seed(3)
    bank = ExplaiNNBank(G, Um, k, L, T).cuda().train()
    bank.dropout_p = 0.0
    before = copy.deepcopy(bank)
    x, y = bank_t._batch(c)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    eng = StepEngine(bank, B, "binary")
    logits, loss = eng.step(xt, yt)
    torch.cuda.synchronize()
    assert logits.shape == (B, G, T) and loss.shape == (G,)
    worst = 0.0
    for g in (0, G // 2, G - 1):
        w, _ = bank_t._against_member(c, "entry bank limit vs member %d" % g, before, g, xt, yt, logits, loss,
                                      eng.views)
        worst = max(worst, w)
    record_margin("entry bank at the unit limit vs single-model path, max |difference|", worst, TOL)
