"""CPU checks of the metrics algebra (tests/metrics_model.py, the numpy restatement of
csrc/metrics.hip) against scikit-learn and scipy, and of the host-side layers around the device call:
results and their one-transfer read, the evaluate CLI's arguments and table, the Trainer's switch."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_model as mm  # noqa: E402


def _scores(kind, n, rng):
    if kind == "distinct":
        return rng.permutation(n).astype(np.float32) / np.float32(n) - np.float32(0.5)
    if kind == "ties":
        return np.round(rng.normal(size=n) * 64).astype(np.float32) / np.float32(64)
    if kind == "equal":
        return np.full(n, 0.25, dtype=np.float32)
    s = rng.normal(size=n).astype(np.float32)
    special = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.finfo(np.float32).max,
                        -np.finfo(np.float32).max, 1.0, -1.0], dtype=np.float32)
    s[rng.integers(0, n, size=max(n // 3, 4))] = special[rng.integers(0, len(special), size=max(n // 3, 4))]
    return s


def test_order_key_is_monotone_and_merges_zeros():
    v = np.array([-np.finfo(np.float32).max, -1.0, -1e-40, -1e-45, -0.0, 0.0, 1e-45, 1e-40, 1.0,
                  np.finfo(np.float32).max], dtype=np.float32)
    k = mm.order_key(v)
    assert k[4] == k[5]
    kk = np.delete(k, 4).astype(np.int64)
    assert (np.diff(kk) > 0).all()          # denormals stay distinct values, order is numeric


@pytest.mark.parametrize("kind", ["distinct", "ties", "equal", "special"])
@pytest.mark.parametrize("n", [2, 65, 4097, 200003])
def test_binary_formulas_match_sklearn(kind, n):
    from sklearn.metrics import average_precision_score, roc_auc_score
    rng = np.random.default_rng(n + len(kind))
    s = _scores(kind, n, rng)
    y = (rng.random(n) < 0.3).astype(np.float32)
    y[0], y[1] = 0.0, 1.0
    p = mm.binary_parts(y, s)
    assert p["P"] == int(y.sum()) and p["P"] + p["Nneg"] == n
    assert abs(mm.auroc(p) - roc_auc_score(y, s)) <= 1e-12
    assert abs(mm.average_precision(p) - average_precision_score(y, s)) <= 1e-12
    if kind == "equal":
        assert mm.auroc(p) == 0.5
        assert mm.average_precision(p) == p["P"] / n


def test_binary_extremes():
    y = np.array([0, 0, 1, 1, 1], dtype=np.float32)
    up = np.arange(5, dtype=np.float32)
    assert mm.auroc(mm.binary_parts(y, up)) == 1.0
    assert mm.auroc(mm.binary_parts(y, -up)) == 0.0
    assert mm.average_precision(mm.binary_parts(y, up)) == 1.0
    assert np.isnan(mm.auroc(mm.binary_parts(np.zeros(5), up)))
    assert mm.average_precision(mm.binary_parts(np.zeros(5), up)) == 0.0
    assert np.isnan(mm.auroc(mm.binary_parts(np.ones(5), up)))


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("kind", ["distinct", "ties", "special"])
@pytest.mark.parametrize("n", [2, 65, 4097, 200003])
def test_linear_formulas_match_scipy(kind, ties, n):
    from scipy.stats import pearsonr, spearmanr
    rng = np.random.default_rng(7 * n + len(kind) + ties)
    s = _scores(kind, n, rng)
    y = (0.5 * s.astype(np.float64) / max(1.0, float(np.abs(s).max())) + rng.normal(size=n)).astype(np.float32)
    if ties:
        y = np.round(y * 4).astype(np.float32) / np.float32(4)
    y[0], y[1] = -1.0, 1.0
    y64, s64 = y.astype(np.float64), s.astype(np.float64)
    if n > 2:           # scipy's two-point Pearson is +-1 by definition, as is the model's up to rounding
        assert abs(mm.pearson(y, s) - float(pearsonr(y64, s64)[0])) <= 1e-12
    else:
        assert abs(abs(mm.pearson(y, s)) - 1.0) <= 1e-12
    assert abs(mm.spearman(y, s) - float(spearmanr(y64, s64)[0])) <= 1e-12


def test_constant_columns_are_nan():
    c, v = np.full(9, 2.5, dtype=np.float32), np.arange(9, dtype=np.float32)
    assert np.isnan(mm.pearson(c, v)) and np.isnan(mm.spearman(c, v))
    assert np.isnan(mm.pearson(v, c)) and np.isnan(mm.spearman(v, c))
    z = np.array([0.0, -0.0, 0.0], dtype=np.float32)
    assert np.isnan(mm.spearman(z, v[:3]))


def test_rank_deviations_are_average_ranks():
    from scipy.stats import rankdata
    rng = np.random.default_rng(3)
    v = np.round(rng.normal(size=1001) * 8).astype(np.float32) / 8
    d = mm.rank_deviations(v)
    assert (d == np.round(2 * rankdata(v) - (len(v) + 1)).astype(np.int64)).all()
    assert d.sum() == 0


# ---- host-side layers, no device ----
def _fake_result(values, kind, status=0, counts=None):
    from explainn_amd import metrics
    t = torch.tensor(values, dtype=torch.float64)
    call = metrics._Call(kind, t, t, torch.tensor([status], dtype=torch.int32),
                         None if counts is None else torch.tensor(counts, dtype=torch.int64))
    return metrics._wrap(t, call, 0)


def test_read_settles_status_and_warns():
    from explainn_amd import metrics
    assert metrics.read(_fake_result(0.75, metrics.BINARY, counts=[3, 4])) == [0.75]
    assert _fake_result([0.5, 1.0], metrics.BINARY, counts=[[3, 4], [1, 2]]).tolist() == [0.5, 1.0]
    with pytest.raises(ValueError, match="NaN or infinity"):
        _fake_result(0.1, metrics.LINEAR, status=1).item()
    with pytest.raises(ValueError, match="exactly 0 or 1"):
        float(_fake_result(0.1, metrics.BINARY, status=2, counts=[1, 1]))
    with pytest.warns(metrics.UndefinedMetricWarning):
        assert np.isnan(_fake_result(float("nan"), metrics.BINARY, counts=[5, 0]).item())
    with pytest.warns(metrics.UndefinedMetricWarning):
        assert np.isnan(_fake_result(float("nan"), metrics.LINEAR).item())
    r = _fake_result(0.25, metrics.LINEAR)
    assert type(r + 1) is torch.Tensor          # derived values are plain tensors


def test_metric_names_and_kinds():
    from explainn_amd import metrics
    from explainn_amd.architectures import get_metrics
    for kind in ("binary", "linear"):
        assert list(metrics.get_device_metrics(kind)) == list(get_metrics(kind))
        assert metrics.kind_of(get_metrics(kind)) == kind
    with pytest.raises(ValueError):
        metrics.kind_of(["accuracy"])


def test_no_cpu_fallback(monkeypatch):
    from explainn_amd import metrics
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.roc_auc(np.array([0.0, 1.0]), np.array([0.1, 0.2]))


def test_evaluate_cli_arguments_and_table(tmp_path, monkeypatch):
    from explainn_amd import evaluate
    args = evaluate.parse_args(["m.pth.tar", "d.tsv", "-o", str(tmp_path), "-b", "7", "-r"])
    assert (args.model_file, args.tsv_file, args.output_dir, args.batch_size, args.rev_complement) == (
        "m.pth.tar", "d.tsv", str(tmp_path), 7, True)
    d = evaluate.parse_args(["m", "d"])
    assert d.output_dir == "./" and d.batch_size == 100 and d.rev_complement is False
    perf = {"aucROC": {"global": 0.75, "per_task": np.array([0.5, 1.0])},
            "aucPR": {"global": 0.625, "per_task": np.array([0.25, float("nan")])}}
    path = evaluate.write_table(perf, str(tmp_path))
    assert os.path.basename(path) == "performance-metrics.tsv"
    rows = [l.rstrip("\n").split("\t") for l in open(path)]
    assert rows[0] == ["metric", "global", "0", "1"]
    assert rows[1][0] == "aucROC" and [float(v) for v in rows[1][1:]] == [0.75, 0.5, 1.0]
    assert rows[2][0] == "aucPR" and float(rows[2][1]) == 0.625 and np.isnan(float(rows[2][3]))
    assert repr(0.1 + 0.2) in evaluate.format_table({"Pearson": {"global": 0.1 + 0.2, "per_task": np.array([1.0])}})


def test_trainer_default_keeps_host_metrics(tmp_path):
    """device_metrics defaults to off, and a Trainer built that way validates through the callables
    it was given (the reference's path)."""
    import inspect
    from explainn_amd import selene, train
    assert inspect.signature(selene.Trainer.__init__).parameters["device_metrics"].default is False
    assert inspect.signature(train._train).parameters["device_metrics"].default is False

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(4, 2)
            self._options = {}

        def forward(self, x):
            return self.lin(x)

    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(32, 4, generator=g), (torch.rand(32, 2, generator=g) > 0.5).float()
    y[0], y[1] = 0.0, 1.0
    loader = [(x[:16], y[:16]), (x[16:], y[16:])]
    calls = []

    def auc(yt, ys):
        from sklearn.metrics import roc_auc_score
        calls.append((type(yt), yt.shape))
        return float(roc_auc_score(yt, ys))

    model = Tiny()
    tr = selene.Trainer(model, {"train": loader, "validation": loader}, torch.nn.BCEWithLogitsLoss(),
                        {"aucROC": auc}, torch.optim.Adam(model.parameters()), max_steps=1,
                        output_dir=str(tmp_path), logging_verbosity=0)
    assert tr.device_metrics is False
    tr.step = 1
    tr.validate()
    for h in (tr.logger, tr._train_logger, tr._validation_logger):
        h.handlers.clear()
    assert calls == [(np.ndarray, (64,))]
    assert set(tr._validation_metrics) == {"aucROC"}
    with pytest.raises(ValueError, match="device metrics cover"):
        selene.Trainer(model, {"train": loader, "validation": loader}, torch.nn.BCEWithLogitsLoss(),
                       {"accuracy": auc}, torch.optim.Adam(model.parameters()), output_dir=str(tmp_path),
                       logging_verbosity=0, device_metrics=True)
