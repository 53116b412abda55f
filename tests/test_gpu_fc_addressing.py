"""The FC kernels against the fp64 oracle at the shapes where fc_fwd's and passB's addressing can go wrong.
Those two reach a unit's rows ([n][Bs] of the pooled extremes and of dy, [Bs] of z, dz and the
ReLU bit words) through range-checked buffer descriptors bound to that unit alone: a row at or beyond
the pooled length n loads 0 and its store is dropped, the 16-sequence tile step is folded into the
instruction, and no device-side test of the batch stride is left.  So the cases are

  * pooled lengths on both sides of every 16-row group (15 / 16 / 17, 31 / 32 / 33, 48, 64, 96), at
    bucket edges (26 = the flagship's; 31 -> 32, 33 -> 40), with one pooled position, at one, two and
    three 32-wide k-steps of the bf16 fc_fwd, and n = 97 where the fp32 fc_fwd takes over;
  * U = 3 and U = 9: nine is one past the unit grid's multiple of 8, so padding blocks exit, and the last
    unit is the one with foreign memory behind its rows;
  * batches 1, 17, 70, 257 (a lone sequence -- eval mode only: BatchNorm refuses to train on one --,
    ragged tiles, more than one workgroup per unit), and one
    engine built for a larger batch than it is given, so that the batch stride exceeds the batch and
    the batch is no multiple of 16;
  * one step with a caller's keep mask (the dropout form whose mask address depends on the lane).

Compared, with the helpers and bounds of parity_util and nothing looser: the eval-mode logits, and of a
train step the logits, the loss and every gradient tensor.  The CPU test checks, on the oracle alone,
that the shapes are what they claim and that no compared row holds a ReLU knife edge."""
import functools

import numpy as np
import pytest

import dispatch_model as dm
from oracle import explainn_oracle as orc
from parity_util import check_grads, close, knife_masks, model, oracle_step, _ORACLE_CACHES

K, T = 5, 1
POOLED = (1, 15, 16, 17, 26, 31, 32, 33, 48, 64, 96, 97)
BATCHES = (1, 17, 70, 257)
# (n, U, B, max_batch): every pooled length with 3 units and the ragged batch 70, and with 9 units and the
# batches in turn; the flagship's bucket also at the two batches it would otherwise miss with 3 units, and
# in an engine built for 200 sequences that is given 17
CASES = ([(n, 3, 70, 70) for n in POOLED] +
         [(n, 9, BATCHES[i % len(BATCHES)], BATCHES[i % len(BATCHES)]) for i, n in enumerate(POOLED)] +
         [(26, 3, 1, 1), (26, 3, 257, 257), (26, 9, 17, 200)])
MASK_CASE = (26, 9, 70, 70)
_ID = lambda c: "n%d-U%d-B%d-of%d" % c


def _length(n):
    return dm.C["POOLW"] * n + K - 1 + n % dm.C["POOLW"]      # ragged last window


def _batch_stride(max_batch):
    """The batch stride a context of max_batch sequences uses: an odd multiple of 64."""
    bs = (max_batch + 63) // 64 * 64
    return bs + 64 if (bs // 64) % 2 == 0 else bs


# ((case, masked) -> what is added to the case's seed: the first multiple of 100 that leaves the oracle's
# pre-activations of all 257 sequences off the knife edges)
_SEED_SHIFT = {((17, 9, 257, 257), False): 700, ((33, 9, 257, 257), False): 400, ((97, 9, 257, 257), False): 300,
               ((26, 3, 257, 257), False): 100}


@functools.lru_cache(maxsize=None)
def _case(case, masked=False):
    """Inputs and the oracle's results for one case, computed once and shared (read-only)."""
    n, U, B, _ = case
    L = _length(n)
    # (seeds: a function of the case, moved on where the first choice puts a pre-activation on a knife
    # edge -- a choice made on the oracle alone, which test_cases_are_what_they_claim re-checks)
    seed = 3200 + 7 * n + U + B + _SEED_SHIFT.get((case, masked), 0)
    rng = np.random.default_rng(seed)
    sd = orc.random_state_dict(U, K, L, T, seed=seed)
    # |gamma1| away from zero, every other unit pooling the minimum (see tests/test_gpu_dispatch_sweep.py)
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, U) * np.where(np.arange(U) % 2, 1, -1)).astype(np.float32)
    x = orc.random_onehot(B, L, seed=seed + 1, n_frac=0.01)
    y = (rng.random((B, T)) > 0.5).astype(np.float32)
    keep = (rng.random((B, 100 * U)) > 0.3).astype(np.uint8) if masked else None
    # (a train step on ONE sequence has no reference: BatchNorm2 refuses it there and here; that batch
    # runs the eval-mode forward alone)
    ref_logits, ref_loss, grads = None, None, None
    if B > 1:
        ref_logits, ref_loss, grads, _ = oracle_step(sd, x, y, keep=keep)
    ref_eval = orc.forward(sd, x)
    for a in (x, y, ref_eval) + ((ref_logits,) if B > 1 else ()) + ((keep,) if masked else ()):
        a.setflags(write=False)
    return sd, x, y, keep, ref_logits, ref_loss, grads, ref_eval


@pytest.mark.parametrize("case", CASES + [MASK_CASE + (True,)], ids=lambda c: _ID(c[:4]) + ("-mask" if len(c) > 4 else ""))
def test_cases_are_what_they_claim(case):
    """CPU: the shape gives the pooled length, the bucket and the fc_fwd form; the unit and batch counts
    sit where the docstring says; and the oracle alone leaves every compared row off the ReLU knife edges."""
    masked = len(case) > 4
    case = case[:4]
    n, U, B, max_batch = case
    L = _length(n)
    assert dm.check_supported(U, K, L, T) == n and dm.pooled_len(L, K) == n
    f = dm.forms(U, K, L, T, B, max_batch, paths=("step",))
    NQ = dm.nq_bucket(n)
    assert dm.nq_lower(NQ) < n <= NQ and ("NQ", NQ) in f
    assert (("fc_fwd", "bf16") in f) == (n != 97) and (("fc_fwd", "fp32") in f) == (n == 97)
    assert U in (3, 9) and 9 % 8 == 1 and B in BATCHES and B <= max_batch
    bs = _batch_stride(max_batch)
    assert bs % 64 == 0 and bs >= max_batch
    if max_batch > B:
        assert bs > B + 64 and B % 16 != 0
    grads = _case(case, masked)[6]
    if B == 1:
        with pytest.raises(ValueError):
            oracle_step(*_case(case)[:3])
        return
    cache = _ORACLE_CACHES[id(grads)][0]
    ch, un = knife_masks(cache, U)
    assert not ch.any() and not un.any(), (case, int(ch.sum()), un)


def test_case_list_covers_the_issue():
    """CPU: every pooled length with both unit counts, every batch at the flagship's bucket, the three
    k-step counts of the bf16 fc_fwd and both sides of its upper limit."""
    assert {(n, U) for n, U, _, _ in CASES} >= {(n, U) for n in POOLED for U in (3, 9)}
    assert {B for n, _, B, _ in CASES if n == 26} == set(BATCHES)
    assert {B for _, _, B, _ in CASES} == set(BATCHES)
    assert {(dm.nq_bucket(n) + 31) // 32 for n in POOLED if n <= dm.C["FC_BF_MAXN"]} == {1, 2, 3}
    assert dm.C["FC_BF_MAXN"] in POOLED and dm.C["FC_BF_MAXN"] + 1 in POOLED
    assert any(mb > B for _, _, B, mb in CASES)


def _tensors(case, masked=False):
    import torch
    sd, x, y, keep, ref_logits, ref_loss, grads, ref_eval = _case(case, masked)
    n, U, B, _ = case
    m = model(sd, U, K, _length(n), T)
    return torch, m, torch.from_numpy(x.copy()).cuda(), torch.from_numpy(y.copy()).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_ID)
def test_fc_addressing_vs_oracle(case):
    """The eval-mode forward (fc_fwd without bit words), then one train step of the engine."""
    pytest.importorskip("torch")
    from explainn_amd.engine import StepEngine
    sd, x, y, keep, ref_logits, ref_loss, grads, ref_eval = _case(case)
    n, U, B, max_batch = case
    torch, m, xt, yt = _tensors(case)
    label = "fc %s " % _ID(case)
    m.eval()
    eng = StepEngine(m, max_batch, loss="binary")              # (the context of max_batch sequences serves both)
    with torch.no_grad():
        ev = m(xt)
    close(ev.detach().cpu().numpy(), ref_eval, what=label + "eval logits")
    if B == 1:
        return
    m.train()
    m.dropout_p = 0.0
    logits, loss = eng.step(xt, yt)
    torch.cuda.synchronize()
    close(logits.detach().cpu().numpy(), ref_logits, what=label + "logits")
    close(loss.item(), ref_loss, tol=1e-5, what=label + "loss")
    named = [(name, g) for (name, _), g in zip(m.named_parameters(), eng.views)]
    assert sorted(name for name, _ in named if name in grads) == sorted(grads)
    check_grads(named, grads, label)


@pytest.mark.gpu
def test_fc_addressing_keep_mask():
    """One train step with a caller's keep mask: the dropout form of fc_fwd that reads the mask at a
    lane-dependent address."""
    pytest.importorskip("torch")
    case = MASK_CASE
    sd, x, y, keep, ref_logits, ref_loss, grads, _ = _case(case, True)
    torch, m, xt, yt = _tensors(case, True)
    label = "fc %s mask " % _ID(case)
    m.train()
    m.set_dropout_mask(torch.from_numpy(keep.copy()))
    logits = m(xt)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, yt)
    loss.backward()
    torch.cuda.synchronize()
    close(logits.detach().cpu().numpy(), ref_logits, what=label + "logits")
    close(loss.item(), ref_loss, tol=1e-5, what=label + "loss")
    params = dict(m.named_parameters())
    check_grads([(key, params[key].grad) for key in grads], grads, label)
