"""Inputs of the regime a trained model lives in, and the CPU checks that they are fair cases
(tests/test_regime_model.py states them; tests/test_gpu_batch_regimes.py runs them on the device).

Every other parity case is a uniform random one-hot batch on parameters at initialisation scale.
Here:

  outlier   one sequence of the batch carries the consensus k-mer of a unit (its pooled q is 50 .. 100
            standard deviations above the rest of the batch): a positive example.  BatchNorm2's batch
            statistics come from SHIFTED fp32 sums over the batch (qmom in csrc/prep.hip); the error
            of such sums grows with (distance of the batch from the shift / spread of the batch)^2, so
            the shift must not be an outlier itself.  The case is run with the planted sequence first,
            in the middle and last.
  scale     |gamma1| up to 4, heavy-tailed q, FC1 x5, non-negative final weights x30: logits to +-57
  sat       the same with the final weights scaled until max|logit| is 90 .. 120: past expf's range
  degen     a zero filter, zero FC1 rows, FC1 rows whose BatchNorm2 variance is of the order of eps,
            a unit whose ReLU is dead for the whole batch (BatchNorm3 variance 0)

Builders return numpy only; nothing here touches a torch device."""
import collections
import contextlib
import functools

import numpy as np

from oracle import explainn_oracle as orc

FC_H = 100
BN_EPS = 1e-5
POOL = 7
SHIFT_SEQS = 16            # sequences the q-moment kernels take their shift from

Case = collections.namedtuple("Case", "id kind U k L T B seed g1 fc fin planted qch loss yscale")


def _case(cid, kind, U, k, L, T, B, g1=1.0, fc=1.0, fin=1.0, planted=(), qch=None, loss="binary", yscale=1.0):
    return Case(cid, kind, U, k, L, T, B, (U * 131 + k * 17 + L + B) % 10007, g1, fc, fin, tuple(planted), qch,
                loss, yscale)


# ---- builders ----------------------------------------------------------------------------------
def consensus(sd, u):
    """The k-mer (base index per tap) that drives unit u's pooled q furthest up: with a negative
    gamma1 the exponential grows where the filter output is SMALLEST, so the sign matters."""
    W = np.asarray(sd["linears.0.weight"], dtype=np.float64)[u]            # (4, k)
    return np.argmax(np.sign(float(sd["linears.1.weight"][u])) * W, axis=0)


def planted_position(i):
    """Start of the i-th planted k-mer: the first tap of pooled window 3 + 4 i."""
    return POOL * (3 + 4 * i)


def plant_consensus(sd, x, units, index):
    """Writes the consensus k-mer of each listed unit into sequence `index` (in place; returns x)."""
    k = sd["linears.0.weight"].shape[2]
    for i, u in enumerate(units):
        p = planted_position(i)
        assert p + k <= x.shape[2], "planted k-mer %d does not fit" % i
        x[index, :, p:p + k] = 0
        x[index, consensus(sd, u), np.arange(p, p + k)] = 1
    return x


def rotate(x, y, r):
    """The batch with sequence i moved to index i + r (a planted sequence 0 lands on index r)."""
    return np.roll(x, r, axis=0), np.roll(y, r, axis=0)


def sweep_device(sd, rng, gamma1=True, bn23=True):
    """The parameter devices of tests/test_gpu_dispatch_sweep.py::_inputs: |gamma1| in [0.6, 1.4]
    with alternating sign (even units pool the minimum); BatchNorm2 / 3 gammas in [0.6, 1.4] and
    beta = 2.5 gamma / 2.0 gamma, which keeps ReLU knife-edges a rare exception at B >= 1024."""
    U = sd["linears.0.weight"].shape[0]
    if gamma1:
        sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, U) * np.where(np.arange(U) % 2, 1, -1)).astype(np.float32)
    if bn23:
        for key, shift in (("linears.7", 2.5), ("linears.11", 2.0)):
            g = rng.uniform(0.6, 1.4, sd[key + ".weight"].shape).astype(np.float32)
            sd[key + ".weight"] = g
            sd[key + ".bias"] = (shift * g).astype(np.float32)
    return sd


def trained_scale(sd, g1, fc, fin, rng):
    """Parameters at the scale training leaves them (in place; returns sd)."""
    U = sd["linears.0.weight"].shape[0]
    sd["linears.1.weight"] = (rng.uniform(0.7, 1.3, U) * g1 * np.where(np.arange(U) % 2, 1, -1)).astype(np.float32)
    sd["linears.1.bias"] = rng.uniform(-1, 1, U).astype(np.float32)
    sd["linears.0.weight"] = (sd["linears.0.weight"] * 8).astype(np.float32)
    sd["linears.6.weight"] = (sd["linears.6.weight"] * fc).astype(np.float32)
    sd["final.weight"] = np.clip(sd["final.weight"] * fin, 0, None).astype(np.float32)   # clamped at 0, as selene does
    return sd


DEGEN_UNITS = dict(zero_filter=0, zero_fc1=1, eps_fc1=2, dead_unit=3)
DEGEN_ROWS = (3, 40, 77)
EPS_TARGETS = (0.2, 1.0, 5.0)          # BatchNorm2 variances of the eps rows, in units of eps


def degenerate(sd, x):
    """Degenerate channels (in place).  Returns {"units": {name: unit}, "rows": {name: channel indices}}:
    zero_filter  unit 0's filter is all zeros: BatchNorm1 variance 0, q constant over the batch
    zero_fc1     three FC1 rows of unit 1 are exactly zero: BatchNorm2 variance 0
    eps_fc1      three FC1 rows of unit 2 scaled until the fp64 BatchNorm2 variance is 0.2, 1, 5 eps
    dead_unit    unit 3's BatchNorm2 channels at gamma 0.1, beta -5: ReLU dead for every sample (|hhat|
                 <= sqrt(B - 1) < 50), z constant, BatchNorm3 variance 0"""
    U, _, k = sd["linears.0.weight"].shape
    n = sd["linears.6.weight"].shape[1]
    assert U >= 5, "one ordinary unit has to remain"
    du = DEGEN_UNITS
    sd["linears.0.weight"][du["zero_filter"]] = 0
    zero_rows = np.array([du["zero_fc1"] * FC_H + r for r in DEGEN_ROWS])
    sd["linears.6.weight"][zero_rows] = 0
    eps_rows = np.array([du["eps_fc1"] * FC_H + r for r in DEGEN_ROWS])
    _, cache, _ = orc.forward(sd, x, training=True, return_cache=True, dtype=np.float64)
    q = cache["q"][:, du["eps_fc1"]]                                       # (B, n)
    for row, target in zip(eps_rows, EPS_TARGETS):
        v = np.asarray(sd["linears.6.weight"][row, :, 0], dtype=np.float64)
        var = (q @ v).var()
        sd["linears.6.weight"][row, :, 0] = (v * np.sqrt(target * BN_EPS / var)).astype(np.float32)
    dead = slice(du["dead_unit"] * FC_H, (du["dead_unit"] + 1) * FC_H)
    sd["linears.7.weight"][dead] = 0.1
    sd["linears.7.bias"][dead] = -5.0
    return {"units": {"zero_filter": du["zero_filter"], "dead_unit": du["dead_unit"]},
            "rows": {"zero_fc1": zero_rows, "eps_fc1": eps_rows}}


# ---- the cases ---------------------------------------------------------------------------------
PLACEMENTS = ("first", "middle", "last")


def placement_index(B, where):
    return {"first": 0, "middle": B // 2 + 1, "last": B - 1}[where]


OUTLIER_CASES = [
    _case("out_n26", "outlier", 6, 19, 200, 2, 1024, g1=2.0, planted=(0, 1)),
    _case("out_n50", "outlier", 5, 19, 368, 1, 768, g1=2.0, planted=(0, 1)),
    _case("out_n7", "outlier", 6, 9, 60, 1, 1024, g1=3.5, planted=(1,)),
    _case("out_b4096", "outlier", 4, 19, 200, 1, 4096, g1=1.5, planted=(0, 1)),
    _case("out_qch2", "outlier", 6, 19, 200, 2, 1024, g1=2.0, planted=(0, 1), qch=2),
]
SCALE_PARAMS = {"scale_g2": (2.0, 5.0, 10.0), "scale_g3": (3.0, 5.0, 30.0), "scale_g4": (4.0, 5.0, 30.0)}
SCALE_CASES = [_case("%s_b%d" % (name, B), "scale", 6, 19, 200, 2, B, g1=g1, fc=fc, fin=fin)
               for name, (g1, fc, fin) in SCALE_PARAMS.items() for B in (96, 640)]
SAT_FIN = {(2, 640): 25.0, (5, 96): 24.0, (2, 96): 34.0}      # set from the measured logits; see test_regime_model
SAT_CASES = [
    _case("scale_sat_t2_b640", "sat", 6, 19, 200, 2, 640, g1=3.0, fc=5.0, fin=SAT_FIN[(2, 640)]),
    _case("scale_sat_t5_b96", "sat", 6, 19, 200, 5, 96, g1=3.0, fc=5.0, fin=SAT_FIN[(5, 96)]),
    _case("scale_sat_mse_b96", "sat", 6, 19, 200, 2, 96, g1=3.0, fc=5.0, fin=SAT_FIN[(2, 96)], loss="linear",
          yscale=100.0),
]
DEGEN_CASES = [_case("degen_b%d" % B, "degen", 6, 19, 200, 2, B) for B in (96, 640)]
CASES = OUTLIER_CASES + SCALE_CASES + SAT_CASES + DEGEN_CASES
BY_ID = {c.id: c for c in CASES}

Inputs = collections.namedtuple("Inputs", "sd x y keep sets")


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """(sd, x, y, keep, sets) of a case; an outlier case has its planted sequence at index 0.
    `keep` is the dropout mask of the autograd route (None: dropout off); `sets` the row sets of
    degenerate()."""
    c = BY_ID[cid]
    rng = np.random.default_rng(c.seed)
    sd = orc.random_state_dict(c.U, c.k, c.L, c.T, seed=c.seed)
    x = orc.random_onehot(c.B, c.L, seed=c.seed + 1, n_frac=0.01)
    sets = None
    if c.kind == "outlier":
        sweep_device(sd, rng)
        # |gamma1| within 10 % of g1: the planted units' outlier ratios then stay near each other
        sd["linears.1.weight"] = (rng.uniform(0.9, 1.1, c.U) * c.g1 * np.where(np.arange(c.U) % 2, 1, -1)).astype(np.float32)
        plant_consensus(sd, x, c.planted, 0)
    elif c.kind in ("scale", "sat"):
        trained_scale(sd, c.g1, c.fc, c.fin, rng)
    else:
        sweep_device(sd, rng, bn23=False)
        sets = degenerate(sd, x)
    y = ((rng.random((c.B, c.T)) > 0.5) * c.yscale).astype(np.float32)
    keep = (rng.random((c.B, FC_H * c.U)) > 0.3).astype(np.uint8)
    if c.kind == "degen":
        # Dropout un-degenerates the case: under a keep mask z of the zero-filter unit is no longer
        # constant, and the reference's fp32 rounding noise in hhat (true value 0), amplified by
        # 1/sqrt(eps), reaches 2.5e-4 of the whole linears.7.weight gradient (B = 640; 5e-6 without
        # dropout).  That is the reference's limit, not a property of the kernels: the autograd route
        # of these cases runs with dropout off, as the sweep's two-route cases do.
        keep = None
    return Inputs(sd, x, y, keep, sets)


def placed(cid, where):
    """The outlier case with its planted sequence at the placement's index: (x, y, keep, r)."""
    c, inp = BY_ID[cid], inputs(cid)
    r = placement_index(c.B, where)
    x, y = rotate(inp.x, inp.y, r)
    return np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(np.roll(inp.keep, r, axis=0)), r


def routes(cid):
    """(route, keep mask) pairs a case runs: StepEngine.step without dropout, autograd with the mask."""
    return (("step", None), ("autograd", inputs(cid).keep))


REF_THREADS = 4


@contextlib.contextmanager
def reference_threads():
    """The reference's fp32 error depends on how ATen splits its batch reductions: with ONE thread
    its sequential sum leaves 1.0e-4 on out_n26's linears.7.bias gradient, with 4 or 8 threads 8e-6.
    The bar a case sets must not depend on what an earlier test left behind (a Trainer run leaves
    one thread): the reference is measured at REF_THREADS."""
    import torch
    before = torch.get_num_threads()
    torch.set_num_threads(REF_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(before)


# ---- the q-moment emulation --------------------------------------------------------------------
def shift_first(q):
    """The shift of the first implementation: q of sequence 0.  Kept as the counter-example."""
    return q[0]


def shift_geometric(q):
    """The shift the kernels use: q at the MEAN POOLED EXTREME of the batch's first SHIFT_SEQS
    sequences, exp(alpha mean(ext) + shift) -- the geometric mean of their q.  In the exponent an
    outlier is 3 .. 5 standard deviations off, not hundreds, so it moves this mean by a fraction of the
    batch's spread even when it is one of the 16."""
    m = min(SHIFT_SEQS, q.shape[0])
    return np.exp(np.log(q[:m].astype(np.float64)).mean(axis=0)).astype(np.float32)


def pooled_q(sd, x):
    """fp64 pooled q (B, U, n) of the train-mode forward."""
    _, cache, _ = orc.forward(sd, x, training=True, return_cache=True, dtype=np.float64)
    return cache["q"]


def emulated_var2_error(sd, x, shift, q=None, step=4):
    """BatchNorm2's variance as the device forms it, against the fp64 truth: (U,) the largest relative
    error over a unit's 100 channels.  q is rounded to fp32; d = q - s in fp32; S1 = sum d and
    S2 = sum d d' are fp32 accumulators that take `step` sequences at a time (one MFMA k-step: the
    products and their sum exact, one rounding into the accumulator); then prep2 in fp64:
    C = S2/B - (S1/B)(S1/B)' rounded to fp32, VC = V1 C rounded to fp32, var = sum_w VC[r,w] V1[r,w].
    shift: callable q (B, U, n) fp32 -> s (U, n)."""
    if q is None:
        q = pooled_q(sd, x)
    q32 = np.asarray(q, dtype=np.float32)
    B, U, n = q32.shape
    s = np.asarray(shift(q32), dtype=np.float32)
    d = (q32 - s[None]).astype(np.float32).astype(np.float64)
    S1 = np.zeros((U, n), dtype=np.float32)
    S2 = np.zeros((U, n, n), dtype=np.float32)
    for b0 in range(0, B, step):
        blk = d[b0:b0 + step]
        S1 = (S1 + blk.sum(axis=0)).astype(np.float32)
        S2 = (S2 + np.einsum("buw,buv->uwv", blk, blk)).astype(np.float32)
    qb = S1.astype(np.float64) / B
    Cs = (S2.astype(np.float64) / B - qb[:, :, None] * qb[:, None, :]).astype(np.float32)
    V1 = np.asarray(sd["linears.6.weight"], dtype=np.float64).reshape(U, FC_H, n)
    VC = np.einsum("urw,uwv->urv", V1, Cs.astype(np.float64)).astype(np.float32)
    var = np.maximum((VC.astype(np.float64) * V1).sum(axis=2), 0)
    truth = np.einsum("buw,urw->bur", q32.astype(np.float64), V1).var(axis=0)
    return (np.abs(var - truth) / np.maximum(truth, 1e-300)).max(axis=1)


def outlier_ratio(q, index, u):
    """q[index].max() / std(q of the other sequences) of unit u."""
    others = np.delete(q[:, u], index, axis=0)
    return float(q[index, u].max() / others.std())
