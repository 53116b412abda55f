"""Evaluation metrics computed on the device (csrc/metrics.hip).

The reference evaluates with scikit-learn's `roc_auc_score` / `average_precision_score` and scipy's
`pearsonr` / `spearmanr` on host copies (architectures.get_metrics, test.py::_get_performances);
three of the four are a sort.  Here predictions and targets stay where the model left them:

    roc_auc, average_precision, pearson, spearman     one metric
    binary_metrics, linear_metrics                    both members of a pair from ONE sort
    performances                                      every metric, global and per task
    get_device_metrics                                drop-in for get_metrics (callables -> float)

`y` (targets) and `s` (scores) are (N,) or (N, T); device tensors are used as they are, numpy arrays
and host tensors are moved to the current HIP device.  `per_task=False` is the Trainer's
`flatten()`: one value over all N*T entries; `per_task=True` gives one value per column.  Results
are fp64 device tensors (0-d, or (T,)) and nothing synchronises until a Python number is asked for:
`.item()`, `.tolist()`, `float()` -- or `read()`, which brings any number of results to the host in
one transfer.  That read also settles the input check, as scikit-learn and scipy would have:
NaN / infinity in either array, or binary targets other than 0 and 1, raise ValueError; a one-class
column (AUROC = NaN), a column without positives (AP = 0) and a constant column (correlations =
NaN) give an `UndefinedMetricWarning`.

There is no CPU fallback: without a HIP device every function raises.
"""
import warnings

import numpy as np
import torch

from . import _lib

BINARY, LINEAR = "binary", "linear"
NAMES = {BINARY: ("aucROC", "aucPR"), LINEAR: ("Pearson", "Spearman")}
MAX_COLUMN = 1 << 26


class UndefinedMetricWarning(UserWarning):
    """A metric is not defined for the data it was given (one class, no positive, constant input)."""


class _Call:
    """What one C call left on the device: both results of the pair, the status word, the class counts."""

    def __init__(self, kind, first, second, status, counts):
        self.kind, self.first, self.second, self.status, self.counts = kind, first, second, status, counts
        self.settled = False

    def settle(self, status, counts):
        """Raise / warn once per call, from host copies of the status word and the counts."""
        if self.settled:
            return
        self.settled = True
        status = int(status)
        if status & _lib.METRICS_NONFINITE:
            raise ValueError("Input contains NaN or infinity.")
        if status & _lib.METRICS_NOT_BINARY:
            raise ValueError("binary metrics need targets that are exactly 0 or 1")
        if self.kind == BINARY:
            c = np.asarray(counts).reshape(-1, 2)
            if (c[:, 0] == 0).any():
                warnings.warn("no positive class in the targets: aucPR is 0.0 and aucROC is not defined",
                              UndefinedMetricWarning, stacklevel=4)
            elif (c[:, 1] == 0).any():
                warnings.warn("only one class present in the targets: aucROC is not defined",
                              UndefinedMetricWarning, stacklevel=4)


class MetricValues(torch.Tensor):
    """fp64 device tensor of metric values; reading it as Python numbers settles the input check."""

    _call = None
    _which = 0

    def item(self):
        return read(self)[0]

    def tolist(self):
        return read(self)[0]

    def __float__(self):
        v = read(self)[0]
        if isinstance(v, list):
            raise TypeError("only a 0-d result converts to float")
        return v

    def numpy(self):
        return np.asarray(read(self)[0], dtype=np.float64)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        # anything computed from the values is a plain tensor: the check travels with the results only
        with torch._C.DisableTorchFunctionSubclass():
            out = func(*args, **(kwargs or {}))
        return out.as_subclass(torch.Tensor) if isinstance(out, MetricValues) else out


def _wrap(t, call, which):
    v = t.as_subclass(MetricValues)
    v._call, v._which = call, which
    return v


def _plain(v):
    return v.as_subclass(torch.Tensor)


def read(*values):
    """Python numbers (0-d -> float, (T,) -> list) of any number of results, ONE device-to-host
    transfer for all of them, their status words and class counts included."""
    calls = []
    for v in values:
        if not isinstance(v, MetricValues) or v._call is None:
            raise TypeError("read() takes results of explainn_amd.metrics")
        if all(v._call is not c for c in calls):
            calls.append(v._call)
    parts = [_plain(v).reshape(-1) for v in values]
    for c in calls:
        parts.append(c.status.to(torch.float64))
        if c.counts is not None:
            parts.append(c.counts.reshape(-1).to(torch.float64))
    flat = torch.cat(parts).cpu().numpy()
    o = sum(v.numel() for v in values)
    for c in calls:
        k = c.counts.numel() if c.counts is not None else 0
        c.settle(flat[o], flat[o + 1:o + 1 + k])
        o += 1 + k
    out, o = [], 0
    for v in values:
        n = v.numel()
        if v.dim() == 0:
            out.append(float(flat[o]))
            if np.isnan(flat[o]) and v._call.kind == LINEAR:
                warnings.warn("an input is constant: the correlation is not defined",
                              UndefinedMetricWarning, stacklevel=3)
        else:
            out.append([float(x) for x in flat[o:o + n]])
            if np.isnan(flat[o:o + n]).any() and v._call.kind == LINEAR:
                warnings.warn("an input column is constant: its correlation is not defined",
                              UndefinedMetricWarning, stacklevel=3)
        o += n
    return out


def _device_of(*arrays):
    for a in arrays:
        if torch.is_tensor(a) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise _lib.ExplainnError(
            "explainn_amd.metrics runs on a HIP device and none is available. There is no CPU "
            "fallback: use architectures.get_metrics (scikit-learn / scipy) on the host.")
    return torch.device("cuda", torch.cuda.current_device())


def _prepare(y, s):
    dev = _device_of(y, s)
    out = []
    for a in (y, s):
        t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
        t = _plain(t) if isinstance(t, MetricValues) else t
        t = t.detach().to(device=dev, dtype=torch.float32)
        if t.dim() == 1:
            t = t.reshape(-1, 1)
        if t.dim() != 2:
            raise ValueError("metrics take (N,) or (N, T) arrays, got shape %s" % (tuple(t.shape),))
        out.append(t.contiguous())
    if out[0].shape != out[1].shape:
        raise ValueError("targets %s and scores %s differ in shape" % (tuple(out[0].shape), tuple(out[1].shape)))
    if out[0].numel() == 0:
        raise ValueError("metrics of an empty array")
    return dev, out[0], out[1]


def workspace_bytes(N, T, per_task, kind):
    """Scratch the C call needs; raises for a column above 2**26 values (nothing is allocated)."""
    lib = _lib.load()
    n = int(lib.explainn_metrics_workspace_bytes(
        int(N), int(T), _lib.METRICS_PER_TASK if per_task else _lib.METRICS_GLOBAL,
        _lib.METRICS_BINARY if kind == BINARY else _lib.METRICS_LINEAR))
    if n < 0:
        msg = lib.explainn_last_error().decode("utf-8", "replace")
        raise ValueError(msg)
    return n


def _run(kind, y, s, per_task):
    dev, y, s = _prepare(y, s)
    N, T = y.shape
    mode = _lib.METRICS_PER_TASK if per_task else _lib.METRICS_GLOBAL
    ws, nbytes = _lib.workspace("explainn_metrics_workspace_bytes", dev, N, T, mode,
                                _lib.METRICS_BINARY if kind == BINARY else _lib.METRICS_LINEAR)
    shape = (T,) if per_task else ()
    first = torch.empty(shape, device=dev, dtype=torch.float64)
    second = torch.empty(shape, device=dev, dtype=torch.float64)
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    if kind == BINARY:
        counts = torch.empty(shape + (2,), device=dev, dtype=torch.int64)
        _lib.call("explainn_metrics_binary", dev, y, s, N, T, mode, first, second, counts, status, ws, nbytes)
    else:
        counts = None
        _lib.call("explainn_metrics_linear", dev, y, s, N, T, mode, first, second, status, ws, nbytes)
    call = _Call(kind, first, second, status, counts)
    return _wrap(first, call, 0), _wrap(second, call, 1)


def binary_metrics(y, s, per_task=False):
    """(aucROC, aucPR) from one sort of the scores."""
    return _run(BINARY, y, s, per_task)


def linear_metrics(y, s, per_task=False):
    """(Pearson, Spearman)."""
    return _run(LINEAR, y, s, per_task)


def class_counts(values):
    """(..., 2) int64 device tensor of (positives, negatives) behind a binary result."""
    if not isinstance(values, MetricValues) or values._call is None or values._call.counts is None:
        raise TypeError("class_counts() takes a result of the binary metrics")
    return values._call.counts


def roc_auc(y, s, per_task=False):
    return binary_metrics(y, s, per_task)[0]


def average_precision(y, s, per_task=False):
    return binary_metrics(y, s, per_task)[1]


def pearson(y, s, per_task=False):
    return linear_metrics(y, s, per_task)[0]


def spearman(y, s, per_task=False):
    return linear_metrics(y, s, per_task)[1]


class DeviceMetric:
    """`(y_true, y_score) -> float`, the calling convention of the get_metrics callables; `kind` and
    `index` tell selene.Trainer which pair and which member it stands for."""

    def __init__(self, name, kind, index):
        self.name, self.kind, self.index = name, kind, index
        self.__name__ = name

    def __call__(self, y_true, y_score):
        return read(_run(self.kind, y_true, y_score, False)[self.index])[0]


def get_device_metrics(input_data="binary"):
    """Counterpart of architectures.get_metrics with the same keys, computed on the device."""
    kind = BINARY if input_data == "binary" else LINEAR
    return {name: DeviceMetric(name, kind, i) for i, name in enumerate(NAMES[kind])}


def kind_of(metric_names):
    """The pair a Trainer's metric names belong to; ValueError when they are not one pair's."""
    names = list(metric_names)
    for kind, pair in NAMES.items():
        if names and all(n in pair for n in names):
            return kind
    raise ValueError("device metrics cover %s and %s; got %s" % (NAMES[BINARY], NAMES[LINEAR], names))


def performances(y, s, input_data="binary"):
    """Every metric of `input_data`, over all values and per task -- test.py::_get_performances:
    {name: {"global": float, "per_task": (T,) float64 array}}; two sorts (one per mode), one read."""
    kind = BINARY if input_data == "binary" else LINEAR
    g = _run(kind, y, s, False)
    p = _run(kind, y, s, True)
    vals = read(g[0], g[1], p[0], p[1])
    return {name: {"global": vals[i], "per_task": np.asarray(vals[2 + i], dtype=np.float64)}
            for i, name in enumerate(NAMES[kind])}
