"""Every compiled kernel form against the fp64 oracle.  Which template runs is chosen on the host from
(U, k, L, T, B, max_batch); tests/dispatch_model.py restates those rules from the sources and builds
this case list so that, between them, the cases reach every form (checked on CPU by
tests/test_dispatch_coverage.py):

  A  every pooled-length bucket at its lower edge (nq_lower + 1) and its upper edge, ragged last windows
  B  every kernel size 2..MAX_K; several LDS images per conv_bwd workgroup at the k-step class edges
  C  32-unit tiles / tile pairs of the filter bank and 16-unit tiles of conv_bwd; the head without
     logits_bn (U past its LDS test)
  D  batch and task edges of the head (passA / fused loss / deferred loss, register / looped
     BatchNorm3), through StepEngine.step and forward + backward
  E  chunk counts: EXPLAINN_QCH / EXPLAINN_ACH overrides and a QCH capped by the 64 MB rule
  F  the soft-input (dense.hip) kernels
  G  base codes: eval logits from uint8 codes equal the one-hot path bit for bit (group A shapes)
  H  sizes explainn_create refuses

The entry points with launchers of their own are swept in tests/test_gpu_entry_sweep.py from case lists
the same model builds (dm.ISM_CASES, dm.IG_CASES, dm.BANK_CASES, dm.BANK_LIMIT):

  ISM   ism_units_kernel<NW> at both kernel sizes of every NW, ism_sum_kernel's task chunks, one
        window, two trips of the sub-batch loop
  IG    input gradient: passB's fc_ng row groups, several batch chunks, unit / batch / kernel-size /
        tail edges in eval, train and soft-input mode
  bank  the head with Gm > 1: fused loss / bank_loss / given dlogits with register and looped bodies,
        head_fwd_train's branches, second trips of the combiner's unit loops, the 2000-unit limit

Each case runs one train step and the eval forward from the updated BatchNorm buffers.  Bounds are
the suite's own (parity_util): logits 1e-4 absolute, gradients GRAD_TOL_ORACLE relative or 3x the
error of the reference's fp32 arithmetic, buffers GRAD_TOL_ORACLE relative; B >= 2048 uses the
knife-edge masked comparison of the full-size property tests.  -m gpu."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dispatch_model as dm  # noqa: E402
from conftest import record_margin  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import (GRAD_TOL_ORACLE, check_grads, close, close_rel, compare_masked, model,  # noqa: E402
                         oracle_step, to_np)

pytestmark = pytest.mark.gpu

MASKED_MIN_B = 2048       # from here on the gradients are compared with compare_masked
SHIFTED_MIN_B = 1024      # from here on BatchNorm2 / 3 shift their outputs off zero (see _inputs)


def _inputs(c):
    rng = np.random.default_rng(c.seed)
    sd = orc.random_state_dict(c.U, c.k, c.L, c.T, seed=c.seed)
    # |gamma1| in [0.6, 1.4], half of them negative (those units pool the minimum).  A unit with
    # gamma1 ~ 0 has BatchNorm1 outputs ~ constant: its gradients are then cancellations of terms
    # hundreds of times their size (seen: 900x at gamma1 = 0.045), ill-conditioned in fp32 whatever the
    # summation order, and the comparison would measure that instead of the kernels
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, c.U) * np.where(np.arange(c.U) % 2, 1, -1)).astype(np.float32)
    if c.B >= SHIFTED_MIN_B:
        # Among B x 100 U ReLU pre-activations some land within rounding of zero, and the masked
        # comparison needs them to stay a small exception: BatchNorm2 / 3 shift their outputs away
        # from zero (|gamma| bounded away from 0, beta = 2.5 gamma), so a pre-activation crosses zero
        # only in the tail of its batch and few channels hold a knife-edge
        for key, shift in (("linears.7", 2.5), ("linears.11", 2.0)):
            g = rng.uniform(0.6, 1.4, sd[key + ".weight"].shape).astype(np.float32)
            sd[key + ".weight"] = g
            sd[key + ".bias"] = (shift * g).astype(np.float32)
    if c.dense:
        x = rng.dirichlet(np.ones(4) * 0.3, size=(c.B, c.L)).transpose(0, 2, 1).astype(np.float32)
        x[0] = 0                                         # an all-zero sequence
        x = np.ascontiguousarray(x)
    else:
        x = orc.random_onehot(c.B, c.L, seed=c.seed + 1, n_frac=0.01)
    y = (rng.random((c.B, c.T)) > 0.5).astype(np.float32)
    keep = None
    if c.paths == ("autograd",):
        keep = (rng.random((c.B, 100 * c.U)) > 0.3).astype(np.uint8)
    return sd, x, y, keep


def _oracle(c, sd, x, y, keep):
    if c.B < MASKED_MIN_B:
        ref_logits, ref_loss, grads, nb = oracle_step(sd, x, y, keep=keep)
        return ref_logits, ref_loss, grads, nb, None
    # large batches: the fp64 oracle's own intermediates give the knife-edge rows
    ref_logits, _, nb = orc.forward(sd, x, training=True, dropout_mask=keep, return_cache=True)
    lg64, cache, _ = orc.forward(sd, x, training=True, dropout_mask=keep, return_cache=True, dtype=np.float64)
    ref_loss, _ = orc.bce_with_logits(ref_logits, y)
    _, dl = orc.bce_with_logits(lg64, y.astype(np.float64))
    return ref_logits, ref_loss, orc.backward(cache, dl), nb, cache


def _check_step(c, label, m, logits, grads, ref_logits, ref_grads, nb, cache):
    close(to_np(logits), ref_logits, what=label + " logits")
    named = list(zip([n for n, _ in m.named_parameters()], grads))
    if cache is None:
        check_grads(named, ref_grads, label + " ")
    else:
        rep = compare_masked(named, ref_grads, cache, c.U, tight=GRAD_TOL_ORACLE)
        for name, (clean, _) in rep.items():
            record_margin("rel %s masked grad %s" % (label, name), clean, GRAD_TOL_ORACLE)
    bufs = dict(m.named_buffers())
    for key, v in nb.items():
        if "tracked" in key:
            assert int(bufs[key].item()) == int(v), key
        else:
            close_rel(to_np(bufs[key]), v, tol=GRAD_TOL_ORACLE, what=label + " " + key)


def _eval_checks(c, label, m, sd, nb, x):
    """Eval mode from the buffers the train step left; group A also checks the base-code input."""
    from explainn_amd.architectures import BaseCodes
    sd2 = dict(sd)
    sd2.update(nb)
    xt = torch.from_numpy(x).cuda()
    m.eval()
    with torch.no_grad():
        got = m(xt)
        close(to_np(got), orc.forward(sd2, x), what=label + " eval logits")
        if c.dense:
            xs = x[:8]
            xr = torch.from_numpy(xs).cuda().repeat(1, c.U, 1)
            close(to_np(m.linears[:3](xr)), orc.unit_activations(sd2, xs), what=label + " activations")
            close(to_np(m.linears(xr)), orc.unit_outputs(sd2, xs), what=label + " unit outputs")
        if c.group == "A":
            codes = x.argmax(axis=1).astype(np.uint8)
            codes[x.sum(axis=1) == 0] = 4
            ct = torch.from_numpy(codes).cuda()
            assert torch.equal(m(ct), got), "base codes differ from the one-hot path"
            assert torch.equal(m(BaseCodes(ct, True)), m(torch.flip(xt, dims=(1, 2)))), \
                "reverse-complement codes differ from the flipped one-hot"


def _run(c):
    from explainn_amd.engine import StepEngine
    sd, x, y, keep = _inputs(c)
    ref_logits, ref_loss, ref_grads, nb, cache = _oracle(c, sd, x, y, keep)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m = None
    for path in c.paths:
        label = "sweep %s %s" % (c.group, path)
        m = model(sd, c.U, c.k, c.L, c.T).train()
        if c.dense:
            m.dense_input = True
        if path == "autograd":
            if keep is None:
                m.dropout_p = 0.0
            else:
                m.set_dropout_mask(torch.from_numpy(keep))
            logits = m(xt)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, yt)
            loss.backward()
            grads = [p.grad for p in m.parameters()]
        else:
            m.dropout_p = 0.0
            eng = StepEngine(m, c.max_batch or c.B, loss="binary")
            logits, loss = eng.step(xt, yt)
            grads = eng.views
        torch.cuda.synchronize()
        close(loss.item(), ref_loss, tol=1e-5, what=label + " loss")
        _check_step(c, label, m, logits, grads, ref_logits, ref_grads, nb, cache)
    _eval_checks(c, "sweep %s" % c.group, m, sd, nb, x)


def _ids(cases):
    return [c.id for c in cases]


SWEEP = [c for c in dm.CASES if c.group != "E"]
CHUNKS = [c for c in dm.CASES if c.group == "E"]


@pytest.mark.parametrize("case", SWEEP, ids=_ids(SWEEP))
def test_dispatch_sweep_vs_oracle(case):
    _run(case)


@pytest.mark.parametrize("case", CHUNKS, ids=_ids(CHUNKS))
def test_chunk_counts_vs_oracle(case, monkeypatch):
    """QCH / ACH are fixed when the context is created: the overrides are set first and the model
    (hence its context) is built after them.  The override must have taken: QCH and ACH below the
    defaults shrink the q-moment and passA partial buffers of the scratch."""
    from explainn_amd import _lib
    geom = (case.U, case.k, case.L, case.T)
    mb = case.max_batch or case.B
    monkeypatch.delenv("EXPLAINN_QCH", raising=False)
    monkeypatch.delenv("EXPLAINN_ACH", raising=False)
    default = _lib.Context(*geom, max_batch=mb, device=torch.cuda.current_device())
    default_bytes = default.scratch_bytes()
    default.close()
    if case.qch:
        monkeypatch.setenv("EXPLAINN_QCH", str(case.qch))
    if case.ach:
        monkeypatch.setenv("EXPLAINN_ACH", str(case.ach))
    if case.qch or case.ach:
        over = _lib.Context(*geom, max_batch=mb, device=torch.cuda.current_device())
        assert over.scratch_bytes() < default_bytes, "the EXPLAINN_QCH / EXPLAINN_ACH override was not applied"
        over.close()
    _run(case)


def test_unsupported_sizes_raise_then_a_valid_model_still_matches():
    from explainn_amd import ExplaiNN
    msgs = {1: "kernel_size 1 unsupported", dm.C["MAX_K"] + 1: "kernel_size %d unsupported" % (dm.C["MAX_K"] + 1)}
    for U, k, L, T in dm.UNSUPPORTED:
        m = ExplaiNN(U, k, L, T).cuda()
        x = torch.from_numpy(orc.random_onehot(4, L, seed=3)).cuda()
        n = dm.pooled_len(L, k)
        match = msgs.get(k, "pooled length n=%d exceeds" % n if n > dm.C["MAX_NQ"] else "pooled length n=%d: .* LDS" % n)
        with pytest.raises(RuntimeError, match=match):
            m(x)
        m.eval()
        with pytest.raises(RuntimeError, match=match), torch.no_grad():
            m(x)
    # the library's state is clean after the refusals (no HIP error left behind for the next launch,
    # the library's or torch's): a valid model matches the oracle
    c = dm._case("H", 5, 19, 200, 2, 70)
    _run(c)
