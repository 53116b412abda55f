"""The filter gradient (bwd.hip conv_bwd_mm_kernel) at the shapes where its geometry can go wrong, after
the forms with at most five column tiles (k <= 20) were brought to five wavefronts per SIMD: the
offsets of the B fragments come from two registers and an immediate, the mask of the sequences past
the batch from one register, the next window's gradients are requested at the window's last position,
and the thread-derived values of the mask expansion and of the reduction are formed where they are used.

Every case is one train step against the fp64 oracle through the sweep's own runner and bounds
(tests/test_gpu_dispatch_sweep.py, parity_util): logits 1e-4 absolute, gradients -- conv_w, conv_b and
BatchNorm1's among them -- GRAD_TOL_ORACLE relative or 3x the error of the reference's fp32 arithmetic.

  pooled length n   1, 3 (fewer windows than wavefronts), 5 (P = 1, deal 2 1 1 1), 8 (P = 2, one window
                    per wavefront), 13 (halves of 7 and 6 windows), 26 (the headline: 13 per half, dealt
                    4 3 3 3), 29 (15 windows per half: a second LDS image of one window)
  batch             33 (a block with one live sequence: three of four lane groups dead, the fourth with
                    one sequence), 100 (a last block of four sequences: a lane group with half its
                    sequences)
  units             17 (a tile with one unit), 40 (a tile half filled)
  kernel size       3 (one column tile), 19 and 20 (five tiles: the new register bound; 19 clamps the last
                    tile's taps), 21 (six tiles: the old bound)

A context used at one batch and then at a smaller one must answer like a fresh one, bit for bit: the
partials of the sequence blocks that the larger batch wrote do not reach the smaller one's sums.  -m gpu."""
import pytest

torch = pytest.importorskip("torch")

import dispatch_model as dm  # noqa: E402
import test_gpu_dispatch_sweep as sweep  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import model  # noqa: E402

pytestmark = pytest.mark.gpu

POOLW = dm.C["POOLW"]


def _len(n, k, tail):
    return POOLW * n + k - 1 + tail


def _case(U, k, n, B, paths=("autograd",)):
    c = dm._case("R", U, k, _len(n, k, n % POOLW), 2, B, paths=paths, tag="-n%d" % n)
    assert dm.pooled_len(c.L, k) == n
    return c


# (units, kernel size, pooled length, batch): every value of every dimension, and each kernel size with
# a short, a split and a two-image pooled length
CASES = [
    _case(17, 19, 1, 33),
    _case(17, 19, 3, 100),
    _case(40, 19, 5, 33),
    _case(17, 19, 8, 100),
    _case(40, 19, 13, 33),
    _case(17, 19, 26, 100, paths=dm.BOTH),
    _case(40, 19, 26, 33),
    _case(40, 19, 29, 100),
    _case(17, 3, 1, 100),
    _case(17, 3, 13, 33),
    _case(40, 3, 29, 100),
    _case(40, 20, 5, 100),
    _case(17, 20, 26, 33),
    _case(17, 20, 29, 100),
    _case(17, 21, 3, 33),
    _case(40, 21, 26, 100),
    _case(17, 21, 29, 33),
]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_filter_gradient_vs_oracle(case):
    sweep._run(case)


def _step(eng, x, y):
    logits, loss = eng.step(x, y)
    torch.cuda.synchronize()
    return {"logits": logits.detach().clone(), "loss": loss.detach().clone(), "flat_grad": eng.flat_grad.detach().clone()}


@pytest.mark.parametrize("k,n", [(19, 26), (20, 29), (21, 13)])
def test_smaller_batch_after_larger_equals_fresh_context(k, n):
    from explainn_amd.engine import StepEngine
    import numpy as np
    U, T, B, B2 = 17, 2, 100, 33
    L = _len(n, k, 1)
    sd = orc.random_state_dict(U, k, L, T, seed=k + n)
    x = torch.from_numpy(orc.random_onehot(B, L, seed=n, n_frac=0.01)).cuda()
    y = torch.from_numpy((np.random.default_rng(k).random((B, T)) > 0.5).astype(np.float32)).cuda()

    def engine():
        m = model(sd, U, k, L, T).train()
        m.dropout_p = 0.0
        return StepEngine(m, B, loss="binary")

    used_engine = engine()
    first = _step(used_engine, x, y)
    assert float(first["flat_grad"].abs().max()) > 0
    used = _step(used_engine, x[:B2], y[:B2])
    fresh = _step(engine(), x[:B2], y[:B2])
    for key in used:
        assert torch.isfinite(used[key]).all(), key
        assert torch.equal(used[key], fresh[key]), "%s of the second step differs from a fresh context's" % key
