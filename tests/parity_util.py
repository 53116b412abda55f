"""Gradient comparison shared by the GPU parity tests: relative-to-the-tensor bounds, with the three
documented exceptions handled explicitly instead of by a slack absolute tolerance.

  * linears.{0,6,10}.bias sit in front of a train-mode BatchNorm: identically zero true gradient
    (we emit exact zeros, the reference emits rounding noise) -> absolute bound.
  * linears.1.bias is a near-null direction (a shift before exp scales q, which BatchNorm2
    normalises away up to eps): its value is a cancellation residual 3-4 orders below its sibling
    linears.1.weight, made of the same summands -> compared on the sibling's scale.
  * ReLU knife-edges: where a pre-activation is within KNIFE of zero for some sample, two correct
    fp32 implementations may take different branches; that moves the rows fed by that
    activation by one sample's share.  The affected rows (found from the ORACLE's intermediates at
    the same parameters, not from the product's) get the loose bound, every other row the tight one.
"""
import numpy as np

from conftest import record_margin

ZERO_GRAD = ("linears.0.bias", "linears.6.bias", "linears.10.bias")
NEAR_NULL = "linears.1.bias"
KNIFE = 5e-6
ABS_FLOOR = 2e-9          # both sides hold rounding noise where the true value is zero (B = 2 fixtures)

# Tolerance: 1e-4 absolute on logits (BASELINE.json north_star: "within 1e-4 fp32"); gradients and
# BatchNorm buffers RELATIVE to the largest entry of the reference tensor: 2e-5 against the
# reference's own numbers (golden fixtures), 5e-5 against the fp64 oracle on random cases.
TOL = 1e-4
GRAD_TOL_GOLDEN = 2e-5     # gradients / BatchNorm buffers vs the reference's own numbers, relative to max|ref|
# Absolute floor under the relative bounds: a tensor whose TRUE value is zero holds only rounding
# noise on both sides (fixture tiny_u1_k5 has B = 2: a train-mode BatchNorm over two samples outputs
# +-1 whatever its input, so every gradient in front of it is exactly zero and the reference's own
# numbers there are ~1e-9 noise).  Real gradient tensors of the fixtures peak at 1e-3 ... 1e-2, six
# orders above it.
GRAD_ABS_FLOOR = 2e-9
GRAD_TOL_ORACLE = 5e-5     # the same vs the fp64 numpy oracle on random cases


def close(a, b, tol=TOL, what=""):
    """Absolute bound (logits, losses, predictions: north_star's "within 1e-4 fp32")."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what + ": non-finite values"
    err = np.abs(a - b).max() if a.size else 0.0
    scale = max(1.0, np.abs(b).max() if b.size else 1.0)
    record_margin("abs " + what, err / scale, tol)
    assert err <= tol * scale, "%s: max|d|=%.3e (scale %.3g)" % (what, err, scale)


def close_rel(a, b, tol=GRAD_TOL_GOLDEN, what=""):
    """Relative to max|ref| of the tensor itself (gradients and buffers: a tensor whose entries
    are all of order 1e-3 must agree to tol of THAT, not of 1.0)."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what + ": non-finite values"
    err = np.abs(a - b).max() if a.size else 0.0
    scale = max(1e-12, np.abs(b).max() if b.size else 1.0)
    bound = tol * scale + GRAD_ABS_FLOOR
    record_margin("rel " + what, err / bound * tol, tol)
    assert err <= bound, "%s: max|d|=%.3e = %.3e of max|ref| %.3g (bound %.1e relative + %.0e)" % (
        what, err, err / scale, scale, tol, GRAD_ABS_FLOOR)


def model(sd, U, k, L, T):
    """An ExplaiNN on the device holding the numpy state dict `sd`."""
    import torch
    from explainn_amd import ExplaiNN
    m = ExplaiNN(U, k, L, T)
    m.load_state_dict({key: torch.from_numpy(np.array(v)) for key, v in sd.items()})
    return m.cuda()


def to_np(t):
    return t.detach().cpu().numpy()


def knife_masks(cache, U):
    """(channel mask (U,100), unit mask (U,)): rows a ReLU sign disagreement could move."""
    Bc = cache["y2"].shape[0]
    ch = np.abs(np.asarray(cache["y2"]).reshape(Bc, U, 100)).min(axis=0) < KNIFE
    un = (np.abs(np.asarray(cache["y3"]).reshape(Bc, U)).min(axis=0) < KNIFE) | ch.any(axis=1)
    return ch, un


def reference_fp32_error(sd, x, y, grads64, kind="binary", keep=None, p=0.3, freeze=0, cache=None):
    """How far the REFERENCE's own arithmetic (stock PyTorch fp32 CPU ops, oracle/torch_ref.py) lands
    from the fp64 truth on this very case: {key: max|torch_fp32 - fp64| / max|fp64|} over the rows
    that are not ReLU knife-edges.  Gradients through BatchNorm are cancellations; for some tensors
    (linears.1.weight above all) fp32 leaves 1e-4 relative however it is organised, so "as accurate
    as the reference" is the bar, not a fixed number."""
    import torch
    from oracle import torch_ref
    sdt = {k: torch.tensor(np.array(v, dtype=np.float32)).clone() for k, v in sd.items() if "tracked" not in k}
    km = None if keep is None else torch.tensor(np.asarray(keep, dtype=np.float32))
    threads = torch.get_num_threads()
    _, _, g = torch_ref.train_step(sdt, torch.tensor(np.asarray(x, dtype=np.float32)),
                                   torch.tensor(np.asarray(y, dtype=np.float32)), kind,
                                   p if keep is not None else 0.0, km)
    torch.set_num_threads(threads)
    U = sd["linears.0.weight"].shape[0]
    ch = un = None
    if cache is not None:
        ch, un = knife_masks(cache, U)
    out = {}
    for key, r in grads64.items():
        r = np.asarray(r, dtype=np.float64)
        t = g[key].detach().numpy().astype(np.float64).reshape(r.shape)
        if key == "linears.0.weight" and freeze:
            t[:freeze] = 0
        err = np.abs(t - r)
        if ch is not None:
            if key.startswith(("linears.6.", "linears.7.")):
                err = err[~ch.reshape(-1)]
            elif key.startswith(("linears.0.", "linears.1.", "linears.10.", "linears.11.")):
                err = err[~un]
            elif key == "final.weight":
                err = err.T[~un]
        scale = np.abs(r).max()
        out[key] = float(err.max() / scale) if err.size and scale > 0 else 0.0
    return out


def compare_grads(named, ref, tol, cache=None, U=None, what="", ref_err=None, abs_floor=ABS_FLOOR):
    """named: iterable of (state_dict key, array-like gradient); ref: {key: array}.  Collects every
    violation and raises once, so a failing run shows the whole picture.  ref_err (from
    reference_fp32_error, for comparisons against the fp64 oracle): a tensor passes when it is
    within `tol` of max|ref| outright OR within 3x the error the reference's own fp32 arithmetic
    makes on that tensor."""
    named = [(k, np.asarray(v, dtype=np.float64)) for k, v in named]
    ch = un = None
    B = None
    if cache is not None:
        ch, un = knife_masks(cache, U)
        B = np.asarray(cache["y3"]).shape[0]
    loose = max(5e-2, 2.0 / B) if B else None
    sib = ref.get("linears.1.weight")
    problems = []
    for key, got in named:
        if key not in ref:
            continue
        r = np.asarray(ref[key], dtype=np.float64)
        got = got.reshape(r.shape)
        if not np.isfinite(got).all():
            problems.append("%s: non-finite" % key)
            continue
        if key in ZERO_GRAD:
            if np.abs(got).max() >= 1e-6:
                problems.append("%s: |g| = %.2e, expected exact zeros" % (key, np.abs(got).max()))
            continue
        err = np.abs(got - r)
        scale = np.abs(r).max() if r.size else 0.0
        t = tol
        if ref_err is not None:
            t = max(tol, 3.0 * ref_err.get(key, 0.0))
        if key == NEAR_NULL and sib is not None:
            sib_scale = np.abs(np.asarray(sib)).max()
            if ref_err is not None and scale > 0:     # the reference's error was relative to this tensor's own max
                t = max(tol, 3.0 * ref_err.get(key, 0.0) * scale / max(sib_scale, scale))
            scale = max(scale, sib_scale)
        rows = None
        if ch is not None:
            if key.startswith(("linears.6.", "linears.7.")):
                rows = ch.reshape(-1)
            elif key.startswith(("linears.0.", "linears.1.", "linears.10.", "linears.11.")):
                rows = un
            elif key == "final.weight":
                err = err.T                        # (U, T): rows are units
                rows = un
        if rows is not None and rows.any():
            clean, masked = err[~rows], err[rows]
        else:
            clean, masked = err, err[:0]
        bound = t * scale + abs_floor
        worst = clean.max() if clean.size else 0.0
        record_margin("rel %sgrad %s" % (what, key), worst / bound * t, t)
        if worst > bound:
            problems.append("%s: clean rows max|d| %.3e = %.2e of scale %.3g (bound %.1e)" % (
                key, worst, worst / max(scale, 1e-300), scale, t))
        if masked.size and masked.max() > loose * scale + abs_floor:
            problems.append("%s: knife-edge rows max|d| %.3e = %.2e of scale %.3g (bound %.1e)" % (
                key, masked.max(), masked.max() / max(scale, 1e-300), scale, loose))
    assert not problems, "%sgradients differ:\n  " % what + "\n  ".join(problems)


_ORACLE_CACHES = {}       # id(reference gradient dict) -> (oracle cache, U): the knife-edge masks of that step


def oracle_step(sd, x, y, freeze=0, keep=None, kind="binary"):
    """Logits, loss and BatchNorm buffers from the fp32 oracle (compared with absolute bounds);
    gradients from the oracle in FP64 -- the truth -- together with the error the reference's own
    fp32 arithmetic makes on this case (reference_fp32_error), which sets the bar."""
    from oracle import explainn_oracle as orc
    ref_logits, _, nb = orc.forward(sd, x, training=True, dropout_mask=keep, return_cache=True)
    lg64, cache, _ = orc.forward(sd, x, training=True, dropout_mask=keep, return_cache=True, dtype=np.float64)
    loss_fn = orc.bce_with_logits if kind == "binary" else orc.mse
    ref_loss, _ = loss_fn(ref_logits, y)
    _, dl = loss_fn(lg64, y.astype(np.float64))
    grads = orc.backward(cache, dl, freeze_top_n_filters=freeze)
    ref_err = reference_fp32_error(sd, x, y, grads, kind, keep, freeze=freeze, cache=cache)
    _ORACLE_CACHES[id(grads)] = (cache, sd["linears.0.weight"].shape[0], ref_err, grads)
    return ref_logits, ref_loss, grads, nb


def check_grads(named, ref_grads, what=""):
    """compare_grads against gradients from oracle_step, at GRAD_TOL_ORACLE / 3x the reference's
    own fp32 error, with that step's knife-edge masks."""
    cache, U, ref_err, _ = _ORACLE_CACHES[id(ref_grads)]
    compare_grads([(key, to_np(got)) for key, got in named], ref_grads, GRAD_TOL_ORACLE, cache, U, what, ref_err)


def compare_masked(named_grads, ref, cache, U_, tight=5e-5, loose=5e-2):
    """Every gradient against the oracle: `tight` x max|ref| everywhere except the knife-edge
    channels / units of knife_masks, which only have to stay within `loose` (a flipped branch moves
    a row by one sample's share, which can be a percent of a small tensor's max: 1.1e-2 seen at
    T = 164).  Measured on MI355X: clean entries agree to 1e-6 .. 3e-6 of the tensor's max."""
    ch, un = knife_masks(cache, U_)
    # the masks must stay a small exception: under 2 % of the channels, and enough clean units left
    # for the tight comparison to mean something (an indexing bug hits every unit alike)
    assert ch.mean() < 0.02 and (~un).sum() >= max(2, U_ // 8), (ch.mean(), un.mean())
    report = {}
    for name, g in named_grads:
        r = ref[name].reshape(tuple(g.shape))
        got = g.detach().cpu().numpy()
        if name in ("linears.0.bias", "linears.6.bias", "linears.10.bias"):
            assert np.abs(got).max() < 1e-6, name           # identically zero
            continue
        if name == "linears.1.bias":
            continue                                       # near-null direction
        scale = np.abs(r).max()
        err = np.abs(got - r)
        if name.startswith(("linears.6.", "linears.7.")):
            rows = ch.reshape(-1)                           # channel index u*100 + r
        elif name.startswith(("linears.0.", "linears.1.", "linears.10.", "linears.11.")):
            rows = un
        else:
            rows = np.zeros(err.shape[0] if name != "final.weight" else 0, dtype=bool)
        if name == "final.weight":                          # (T, U): columns are units; o ~ 0 at a knife-edge
            masked, clean = err[:, un], err[:, ~un]
        elif rows.size:
            masked, clean = err[rows], err[~rows]
        else:
            masked, clean = err[:0], err
        report[name] = (clean.max() / scale if clean.size else 0.0, masked.max() / scale if masked.size else 0.0)
        assert clean.size == 0 or clean.max() <= tight * scale, (name, "clean", report[name])
        assert masked.size == 0 or masked.max() <= loose * scale, (name, "knife-edge", report[name])
    print("masked comparison: %.2f%% channels, %d/%d units masked; worst clean %.2e, worst masked %.2e" % (
        100 * ch.mean(), int(un.sum()), U_, max(v[0] for v in report.values()),
        max(v[1] for v in report.values())))
    return report
