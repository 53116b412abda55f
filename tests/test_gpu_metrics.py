"""Device-side evaluation metrics (csrc/metrics.hip, explainn_amd/metrics.py) against the exactly
rounded references of tests/metrics_model.py.

Bounds, derived and not measured:
  * AUROC is bit-equal to float(U2) / float(2 P Nneg) with the integers from the model: both sides are
    one correctly rounded division of integers that fp64 represents exactly (n <= 2**26).
  * AP, Pearson, Spearman: 1e-12 from the math.fsum reference -- relative for AP (all terms positive),
    absolute for the correlations (Cauchy-Schwarz: the sum of |terms| is at most the normaliser).  The
    kernels' longest sequential fp64 chain is 64 additions (16 per thread, 64 block partials per
    thread of the final block) plus trees of depth 8, far inside the (4096 + 30) * 2**-53 = 4.6e-13
    the bound allows for.
scikit-learn / scipy on the same arrays are computed too; their distance from the references is
recorded (conftest.record_margin) and must stay below 1e-9, a net for a wrong formula only."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_model as mm  # noqa: E402
from conftest import record_margin  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
NET = 1e-9
FMAX = np.finfo(np.float32).max

SMALL_N = [2, 63, 64, 65, 4097]
TASKS = [1, 3, 50]
BIG = [(1000003, 1), (1000003, 3), (100000, 50)]
BINARY_SCORES = ["distinct", "ties", "equal", "sep_up", "sep_down", "special"]
LINEAR_SCORES = ["distinct", "ties", "special"]


def _labels(n, t, rng):
    y = (rng.random((n, t)) < 0.3).astype(np.float32)
    y[0], y[1] = 0.0, 1.0                   # both classes in every column
    return y


def _scores(kind, y, rng):
    n, t = y.shape
    if kind == "distinct":
        return (rng.permutation(n * t).astype(np.float32) / np.float32(n * t) - np.float32(0.5)).reshape(n, t)
    if kind == "ties":
        return (np.round((rng.normal(size=(n, t)) + y) * 64) / 64).astype(np.float32)
    if kind == "equal":
        return np.full((n, t), -1.5, dtype=np.float32)
    if kind == "sep_up":
        return (y * 2 - 1) * (1 + rng.random((n, t)).astype(np.float32))
    if kind == "sep_down":
        return -(y * 2 - 1) * (1 + rng.random((n, t)).astype(np.float32))
    s = (rng.normal(size=(n, t)) + y).astype(np.float32)
    special = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, FMAX, -FMAX], dtype=np.float32)
    k = max(n * t // 3, 2)
    s.reshape(-1)[rng.integers(0, n * t, size=k)] = special[rng.integers(0, len(special), size=k)]
    s.reshape(-1)[:2] = [-0.0, 0.0]
    return s


def _close(what, got, ref, relative):
    """got within TOL of ref (relative to ref for AP); NaN only where the reference is NaN."""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    assert (np.isnan(got) == np.isnan(ref)).all(), what
    ok = ~np.isnan(ref)
    scale = np.abs(ref[ok]) if relative else np.ones(int(ok.sum()))
    err = np.abs(got[ok] - ref[ok]) / np.where(scale > 0, scale, 1.0)
    worst = float(err.max()) if err.size else 0.0
    print("%s: worst error %.3e (bound %.1e)" % (what, worst, TOL))
    record_margin(what, worst, TOL)
    assert worst <= TOL, "%s: %.3e" % (what, worst)


def _net(what, lib, ref):
    lib, ref = np.asarray(lib, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    ok = ~(np.isnan(lib) | np.isnan(ref))
    worst = float(np.abs(lib[ok] - ref[ok]).max()) if ok.any() else 0.0
    record_margin(what, worst, NET)
    assert worst <= NET, "%s: library and reference differ by %.3e" % (what, worst)


def _bits(a):
    return np.asarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def _binary_refs(y, s, per_task):
    parts = [mm.binary_parts(a, b) for a, b in mm.columns(y, s, per_task)]
    return parts, np.array([mm.auroc(p) for p in parts]), np.array([mm.average_precision(p) for p in parts])


def _check_binary(y, s, per_task, label, libs=True):
    from explainn_amd import metrics
    yt, st = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
    roc, ap = metrics.binary_metrics(yt, st, per_task)
    assert roc.dtype == torch.float64 and roc.is_cuda and tuple(roc.shape) == ((y.shape[1],) if per_task else ())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got_roc, got_ap = metrics.read(roc, ap)
    counts = metrics.class_counts(roc).cpu().numpy().reshape(-1, 2)
    parts, ref_roc, ref_ap = _binary_refs(y, s, per_task)
    assert [tuple(c) for c in counts] == [(p["P"], p["Nneg"]) for p in parts]
    assert (_bits(got_roc) == _bits(ref_roc)).all(), "%s: AUROC %r, integers give %r" % (label, got_roc, ref_roc)
    _close("metrics AP vs fsum " + label, got_ap, ref_ap, relative=True)
    if libs:
        from sklearn.metrics import average_precision_score, roc_auc_score
        cols = mm.columns(y, s, per_task)
        _net("sklearn roc_auc vs integers " + label, [roc_auc_score(a, b) for a, b in cols], ref_roc)
        _net("sklearn AP vs fsum " + label, [average_precision_score(a, b) for a, b in cols], ref_ap)
    return got_roc, got_ap


def _check_linear(y, s, per_task, label):
    from scipy.stats import pearsonr, spearmanr
    from explainn_amd import metrics
    yt, st = torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda()
    pe, sp = metrics.linear_metrics(yt, st, per_task)
    assert pe.dtype == torch.float64 and pe.is_cuda and tuple(pe.shape) == ((y.shape[1],) if per_task else ())
    got_pe, got_sp = metrics.read(pe, sp)
    cols = mm.columns(y, s, per_task)
    ref_pe = np.array([mm.pearson(a, b) for a, b in cols])
    ref_sp = np.array([mm.spearman(a, b) for a, b in cols])
    _close("metrics Pearson vs fsum " + label, got_pe, ref_pe, relative=False)
    _close("metrics Spearman vs exact ranks " + label, got_sp, ref_sp, relative=False)
    if len(cols[0][0]) > 2:
        _net("scipy pearsonr vs fsum " + label,
             [pearsonr(a.astype(np.float64), b.astype(np.float64))[0] for a, b in cols], ref_pe)
    _net("scipy spearmanr vs exact ranks " + label,
         [spearmanr(a.astype(np.float64), b.astype(np.float64))[0] for a, b in cols], ref_sp)
    return got_pe, got_sp


# ---------------------------------------------------------------- binary pair
@pytest.mark.parametrize("per_task", [False, True])
@pytest.mark.parametrize("kind", BINARY_SCORES)
@pytest.mark.parametrize("t", TASKS)
@pytest.mark.parametrize("n", SMALL_N)
def test_binary_small(n, t, kind, per_task):
    rng = np.random.default_rng(1000 * n + 10 * t + len(kind))
    y = _labels(n, t, rng)
    s = _scores(kind, y, rng)
    roc, ap = _check_binary(y, s, per_task, "(%d,%d) %s %s" % (n, t, kind, "per task" if per_task else "global"))
    cols = mm.columns(y, s, per_task)
    if kind == "equal":
        assert (np.asarray(roc).reshape(-1) == 0.5).all()
        assert (np.asarray(ap).reshape(-1) == np.array([float(a.sum()) / len(a) for a, _ in cols])).all()
    if kind == "sep_up":
        assert (np.asarray(roc).reshape(-1) == 1.0).all()
    if kind == "sep_down":
        assert (np.asarray(roc).reshape(-1) == 0.0).all()


@pytest.mark.parametrize("per_task", [False, True])
@pytest.mark.parametrize("kind", ["distinct", "ties"])
@pytest.mark.parametrize("n,t", BIG)
def test_binary_big(n, t, kind, per_task):
    rng = np.random.default_rng(n + t + len(kind))
    y = _labels(n, t, rng)
    s = _scores(kind, y, rng)
    _check_binary(y, s, per_task, "(%d,%d) %s %s" % (n, t, kind, "per task" if per_task else "global"))


@pytest.mark.parametrize("n,t", [(65, 3), (4097, 1), (1000003, 1)])
def test_single_positive_column(n, t):
    rng = np.random.default_rng(n)
    y = np.zeros((n, t), dtype=np.float32)
    y[rng.integers(0, n, size=t), np.arange(t)] = 1.0
    s = _scores("ties", y, rng)
    for per_task in (False, True):
        _check_binary(y, s, per_task, "(%d,%d) one positive per column" % (n, t))


# ---------------------------------------------------------------- linear pair
def _targets(s, ties, rng):
    z = s.astype(np.float64) / max(1.0, float(np.abs(s).max()))
    y = (0.5 * z + rng.normal(size=s.shape)).astype(np.float32)
    if ties:
        y = (np.round(y * 4) / 4).astype(np.float32)
    y[0], y[1] = -1.0, 1.0
    return y


@pytest.mark.parametrize("per_task", [False, True])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("kind", LINEAR_SCORES)
@pytest.mark.parametrize("t", TASKS)
@pytest.mark.parametrize("n", SMALL_N)
def test_linear_small(n, t, kind, ties, per_task):
    rng = np.random.default_rng(77 * n + 5 * t + len(kind) + ties)
    s = _scores(kind, np.zeros((n, t), dtype=np.float32), rng)
    s[0], s[1] = -0.5, 0.75                  # no constant column at n = 2
    y = _targets(s, ties, rng)
    _check_linear(y, s, per_task, "(%d,%d) %s%s %s" % (n, t, kind, " tied labels" if ties else "",
                                                       "per task" if per_task else "global"))


@pytest.mark.parametrize("per_task", [False, True])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n,t", BIG)
def test_linear_big(n, t, ties, per_task):
    rng = np.random.default_rng(n + t + ties)
    s = _scores("ties" if ties else "distinct", np.zeros((n, t), dtype=np.float32), rng)
    y = _targets(s, ties, rng)
    _check_linear(y, s, per_task, "(%d,%d)%s %s" % (n, t, " tied" if ties else "",
                                                    "per task" if per_task else "global"))


# ---------------------------------------------------------------- determinism, permutation, flatten
@pytest.mark.parametrize("n,t", [(4097, 3), (100000, 50)])
def test_determinism_permutation_flatten(n, t):
    from explainn_amd import metrics
    rng = np.random.default_rng(5)
    y = _labels(n, t, rng)
    s = _scores("ties", y, rng)
    yl = _targets(s, True, rng)
    perm = rng.permutation(n)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for per_task in (False, True):
        a = metrics.read(*metrics.binary_metrics(cu(y), cu(s), per_task))
        b = metrics.read(*metrics.binary_metrics(cu(y), cu(s), per_task))
        c = metrics.read(*metrics.binary_metrics(cu(y[perm]), cu(s[perm]), per_task))
        for u, v, w in zip(a, b, c):
            assert (_bits(u) == _bits(v)).all(), "two calls differ"
            assert (_bits(u) == _bits(w)).all(), "a row permutation changed AUROC / AP"
        a = metrics.read(*metrics.linear_metrics(cu(yl), cu(s), per_task))
        b = metrics.read(*metrics.linear_metrics(cu(yl), cu(s), per_task))
        c = metrics.read(*metrics.linear_metrics(cu(yl[perm]), cu(s[perm]), per_task))
        for u, v, w in zip(a, b, c):
            assert (_bits(u) == _bits(v)).all(), "two calls differ"
            # both are within TOL of the same exact value
            assert np.abs(np.asarray(u) - np.asarray(w)).max() <= 2 * TOL
    for fn, yy in ((metrics.binary_metrics, y), (metrics.linear_metrics, yl)):
        g = metrics.read(*fn(cu(yy), cu(s), False))
        f = metrics.read(*fn(cu(yy.reshape(-1, 1)), cu(s.reshape(-1, 1)), True))
        for u, v in zip(g, f):
            assert (_bits(u) == _bits(v)).all(), "global mode differs from per-task on the flattened data"


def test_single_metric_entry_points_and_host_input():
    from explainn_amd import metrics
    rng = np.random.default_rng(9)
    y = _labels(513, 2, rng)
    s = _scores("ties", y, rng)
    roc, ap = metrics.read(*metrics.binary_metrics(torch.from_numpy(y).cuda(), torch.from_numpy(s).cuda(), True))
    assert metrics.roc_auc(y, s, per_task=True).tolist() == roc               # numpy in
    assert metrics.average_precision(torch.from_numpy(y), torch.from_numpy(s), per_task=True).tolist() == ap
    pe, sp = metrics.read(*metrics.linear_metrics(s, y))
    assert metrics.pearson(s, y).item() == pe and float(metrics.spearman(s, y)) == sp
    fns = metrics.get_device_metrics("binary")
    assert fns["aucROC"](y.flatten(), s.flatten()) == metrics.roc_auc(y, s).item()
    assert isinstance(fns["aucPR"](y[:, 0], s[:, 0]), float)
    perf = metrics.performances(y, s, "binary")
    assert perf["aucROC"]["per_task"].tolist() == roc and perf["aucPR"]["global"] == metrics.average_precision(y, s).item()


# ---------------------------------------------------------------- degenerate and invalid input
def test_degenerate_columns():
    from explainn_amd import metrics
    rng = np.random.default_rng(11)
    s = rng.normal(size=(300, 3)).astype(np.float32)
    y = _labels(300, 3, rng)
    y[:, 1] = 0.0                            # no positive
    y[:, 2] = 1.0                            # no negative
    with pytest.warns(metrics.UndefinedMetricWarning):
        roc, ap = metrics.read(*metrics.binary_metrics(y, s, True))
    assert not np.isnan(roc[0]) and np.isnan(roc[1]) and np.isnan(roc[2])
    assert ap[1] == 0.0 and ap[2] == 1.0
    with pytest.warns(metrics.UndefinedMetricWarning):
        assert np.isnan(metrics.roc_auc(np.ones(10), np.arange(10.0)).item())
    yl = rng.normal(size=(300, 3)).astype(np.float32)
    yl[:, 1] = 0.1                           # 0.1f: the fp64 mean of 300 copies is not exact
    s2 = s.copy()
    s2[:, 2] = np.where(np.arange(300) % 2 == 0, 0.0, -0.0)
    with pytest.warns(metrics.UndefinedMetricWarning):
        pe, sp = metrics.read(*metrics.linear_metrics(yl, s2, True))
    assert not np.isnan(pe[0]) and not np.isnan(sp[0])
    assert np.isnan(pe[1]) and np.isnan(sp[1]) and np.isnan(pe[2]) and np.isnan(sp[2])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_input_raises(bad):
    from explainn_amd import metrics
    rng = np.random.default_rng(13)
    y = _labels(5000, 2, rng)
    s = rng.normal(size=(5000, 2)).astype(np.float32)
    for which in (0, 1):
        for fn in (metrics.binary_metrics, metrics.linear_metrics):
            arrs = [y.copy(), s.copy()]
            arrs[which][4321, 1] = bad
            with pytest.raises(ValueError, match="NaN or infinity"):
                metrics.read(*fn(arrs[0], arrs[1], True))


def test_non_binary_targets_raise():
    from explainn_amd import metrics
    rng = np.random.default_rng(14)
    y = _labels(700, 1, rng)
    y[5] = 0.5
    with pytest.raises(ValueError, match="exactly 0 or 1"):
        metrics.roc_auc(y, rng.normal(size=(700, 1)).astype(np.float32)).item()


def test_too_long_column_is_refused_before_allocating():
    from explainn_amd import metrics
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="2\\^26"):
        metrics.workspace_bytes((1 << 26) + 1, 1, True, metrics.BINARY)
    with pytest.raises(ValueError, match="2\\^26"):
        metrics.workspace_bytes((1 << 25) + 1, 2, False, metrics.LINEAR)
    assert metrics.workspace_bytes(1 << 26, 1, True, metrics.BINARY) > 0
    assert torch.cuda.memory_allocated() == before


# ---------------------------------------------------------------- Trainer switch
def _trainer_fixture():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trainer_run.npz"),
                allow_pickle=False)
    U, k, L, T, B, N = [int(v) for v in z["cfg"]]
    codes = z["codes"]
    x = np.zeros((codes.shape[0], 4, L), dtype=np.float32)
    for a in range(4):
        x[:, a, :] = codes == a
    sd = {key[3:]: torch.from_numpy(np.array(z[key])) for key in z.files if key.startswith("sd/")}
    return (U, k, L, T, B, N), torch.from_numpy(x), torch.from_numpy(z["y"]), sd


def _validate_once(tmp, model, loaders, kind, device_metrics):
    from explainn_amd import get_loss, get_metrics, get_optimizer
    from explainn_amd.selene import Trainer
    os.makedirs(tmp, exist_ok=True)
    tr = Trainer(model, loaders, get_loss(kind), get_metrics(kind), get_optimizer(model.parameters(), 0.003),
                 max_steps=4, report_stats_every_n_steps=1, output_dir=tmp, use_cuda=True,
                 logging_verbosity=0, device_metrics=device_metrics)
    tr.step = 1
    try:
        tr.validate()
        host = None if device_metrics else tr._evaluate_on_data("validation")
    finally:
        for lg in (tr.logger, tr._train_logger, tr._validation_logger):
            for h in list(lg.handlers):
                h.close()
            lg.handlers.clear()
    lines = open(os.path.join(tmp, "validation.txt")).read().strip().split("\n")
    return tr, lines, host


@pytest.mark.parametrize("kind", ["binary", "linear"])
def test_trainer_device_metrics_match_host(tmp_path, kind):
    from torch.utils.data import DataLoader, TensorDataset
    from explainn_amd import ExplaiNN
    (U, k, L, T, B, N), x, y, sd = _trainer_fixture()
    if kind == "linear":
        y = y + 0.25 * torch.randn(y.shape, generator=torch.Generator().manual_seed(1))
    model = ExplaiNN(U, k, L, T)
    model.load_state_dict(sd)
    loaders = {"train": DataLoader(TensorDataset(x[:N], y[:N]), B, shuffle=False),
               "validation": DataLoader(TensorDataset(x, y), B, shuffle=False)}
    th, lh, (_, preds, tgts) = _validate_once(str(tmp_path / "host"), model, loaders, kind, False)
    td, ld, _ = _validate_once(str(tmp_path / "device"), model, loaders, kind, True)
    assert lh[0] == ld[0] and len(lh) == len(ld) == 2                     # same header, one row each
    assert lh[1].split("\t")[0] == ld[1].split("\t")[0], "validation loss differs"
    assert list(th._validation_metrics) == list(td._validation_metrics)
    h, d = th._validation_metrics, td._validation_metrics
    assert all(isinstance(v, float) for v in d.values())
    assert [float(v) for v in ld[1].split("\t")[1:]] == list(d.values())
    if kind == "binary":
        for name in ("aucROC", "aucPR"):
            print("trainer %s: host %r device %r" % (name, h[name], d[name]))
            assert abs(h[name] - d[name]) <= 1e-12, name
    else:
        ref = mm.pearson(tgts.flatten(), preds.flatten())
        print("trainer Pearson: host (scipy, float32) %r device %r fsum %r" % (h["Pearson"], d["Pearson"], ref))
        assert abs(float(h["Pearson"]) - d["Pearson"]) <= 1e-6
        assert abs(d["Pearson"] - ref) <= 1e-12
        assert abs(d["Spearman"] - mm.spearman(tgts.flatten(), preds.flatten())) <= 1e-12
        assert abs(float(h["Spearman"]) - d["Spearman"]) <= 1e-6
    assert (th._best_step, th._min_loss) == (td._best_step, td._min_loss)   # the same checkpoint decision
    assert os.path.exists(tmp_path / "host" / "best_model.pth.tar")
    assert os.path.exists(tmp_path / "device" / "best_model.pth.tar")


# ---------------------------------------------------------------- evaluate CLI, end to end
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("kind", ["binary", "linear"])
def test_evaluate_cli_end_to_end(tmp_path, capsys, kind, rev):
    from explainn_amd import ExplaiNN, evaluate
    from explainn_amd.predict import _load_model, predict
    from explainn_amd.sequence import encode_codes_many
    from oracle import explainn_oracle as orc
    U, k, L, T, N = 6, 9, 60, 3, 203
    sd = orc.random_state_dict(U, k, L, T, seed=4)
    model = ExplaiNN(U, k, L, T)
    model.load_state_dict({key: torch.from_numpy(np.asarray(v)) for key, v in sd.items()})
    ck = str(tmp_path / "model.pth.tar")
    torch.save({"step": 1, "arch": "ExplaiNN", "options": model._options, "state_dict": model.state_dict(),
                "min_loss": 0.5, "optimizer": {}}, ck)
    rng = np.random.default_rng(21)
    seqs = ["".join(rng.choice(list("ACGT"), size=L)) for _ in range(N)]
    labels = (rng.random((N, T)) < 0.4).astype(np.float32) if kind == "binary" else \
        rng.normal(size=(N, T)).astype(np.float32)
    labels[0], labels[1] = 0.0, 1.0
    tsv = str(tmp_path / "data.tsv")
    with open(tsv, "wt") as fh:
        for i, (sq, row) in enumerate(zip(seqs, labels)):
            fh.write("s%d\t%s\t%s\n" % (i, sq, "\t".join(repr(float(v)) for v in row)))
    out = str(tmp_path / "out")
    evaluate.main([ck, tsv, "-o", out, "-b", "64"] + (["-r"] if rev else []))
    printed = capsys.readouterr().out
    text = open(os.path.join(out, "performance-metrics.tsv")).read()
    assert text in printed
    rows = [ln.split("\t") for ln in text.strip().split("\n")]
    assert rows[0] == ["metric", "global", "0", "1", "2"]
    logits = predict(_load_model(ck), encode_codes_many(seqs), 64)[:, :, 2 if rev else 0]
    if kind == "binary":
        from sklearn.metrics import average_precision_score, roc_auc_score
        fns = {"aucROC": roc_auc_score, "aucPR": average_precision_score}
    else:
        from scipy.stats import pearsonr, spearmanr
        fns = {"Pearson": lambda a, b: pearsonr(a, b)[0], "Spearman": lambda a, b: spearmanr(a, b)[0]}
    assert [r[0] for r in rows[1:]] == list(fns)
    y64 = labels.astype(np.float64)
    for r in rows[1:]:
        want = [fns[r[0]](y64.flatten(), logits.flatten())] + [fns[r[0]](y64[:, t], logits[:, t]) for t in range(T)]
        got = [float(v) for v in r[1:]]
        print("evaluate %s: table %r, libraries %r" % (r[0], got, [float(w) for w in want]))
        assert np.abs(np.array(got) - np.array(want, dtype=np.float64)).max() <= 1e-12, r[0]
