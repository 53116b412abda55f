"""Evaluation of a trained ExplaiNN on a labelled TSV (reference: explainn/test.py,
`_get_performances`).

    python -m explainn_amd.evaluate MODEL.pth.tar DATA.tsv [-o DIR] [-b BATCH] [-r]

(The module is called `evaluate` so that nobody takes it for a part of the test suite.)  DATA.tsv is
the headerless training format `id <tab> sequence <tab> y0 [<tab> y1 ...]`.  The model's eval-mode
logits of every sequence -- with -r the float32 mean of the logits of both strands, as
interpret._get_well_predicted_sequences averages them -- and the labels stay on the device, where
explainn_amd.metrics computes aucROC and aucPR (binary labels: two distinct values in the first label
column, the rule of train.main) or Pearson and Spearman (anything else), over all values and per task.

Output, DIR/performance-metrics.tsv (also printed), tab separated:

    metric   global   0      1     ...          header; one column per task, named by its index
    aucROC   <float>  <float> ...               one row per metric, values as repr() of the fp64

`global` is the metric of the flattened (N*T) arrays, what selene.Trainer logs during training.  A
metric that is not defined for a column (one class, constant values) is written as nan.  Where the
reference's description does not pin test.py's file format, THIS format is the definition.
"""
import argparse
import os

import numpy as np
import torch

from . import metrics
from .architectures import BaseCodes
from .loader import read_tsv_codes
from .predict import _load_model
from .strands import eval_pass

_CHUNK = 4096        # sequences per device pass, as in predict()
TABLE = "performance-metrics.tsv"


def scores(model, codes, batch_size=100, rev_complement=False):
    """(N,T) fp32 device tensor of eval-mode logits of base codes (N,L); with rev_complement the
    mean of both strands' logits.  Eval-mode outputs do not depend on the batch they are in, so the
    device passes take max(batch_size, 4096) sequences."""
    dev = model.final.weight.device
    data = torch.as_tensor(np.ascontiguousarray(codes))
    chunk = max(int(batch_size), _CHUNK)
    out = torch.empty(len(data), model._options["n_features"], device=dev, dtype=torch.float32)
    with eval_pass(model):
        for i in range(0, len(data), chunk):
            xb = data[i:i + chunk].to(dev)
            fwd = model(BaseCodes(xb))
            if rev_complement:
                fwd = (fwd + model(BaseCodes(xb, reverse_complement=True))) / 2
            out[i:i + len(xb)] = fwd
    return out


def input_kind(labels):
    """train.main's rule: binary when the first label column holds exactly two distinct values."""
    return "binary" if np.unique(np.asarray(labels)[:, 0]).size == 2 else "linear"


def evaluate(model, codes, labels, batch_size=100, rev_complement=False, input_data=None):
    """{metric: {"global": float, "per_task": (T,) array}} of `model` on (codes, labels)."""
    labels = np.asarray(labels, dtype=np.float32)
    kind = input_data or input_kind(labels)
    s = scores(model, codes, batch_size, rev_complement)
    return metrics.performances(torch.from_numpy(labels).to(s.device), s, kind)


def format_table(perf):
    n_tasks = len(next(iter(perf.values()))["per_task"])
    lines = ["\t".join(["metric", "global"] + [str(t) for t in range(n_tasks)])]
    for name, v in perf.items():
        lines.append("\t".join([name, repr(float(v["global"]))] + [repr(float(x)) for x in v["per_task"]]))
    return "\n".join(lines) + "\n"


def write_table(perf, output_dir):
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, TABLE)
    with open(path, "wt") as fh:
        fh.write(format_table(perf))
    return path


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_file")
    ap.add_argument("tsv_file")
    ap.add_argument("-b", "--batch-size", type=int, default=100)
    ap.add_argument("-o", "--output-dir", default="./")
    ap.add_argument("-r", "--rev-complement", action="store_true")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    codes, labels, _ = read_tsv_codes(args.tsv_file)
    model = _load_model(args.model_file)
    L = model._options["sequence_length"]
    if codes.shape[1] != L:
        raise SystemExit("sequences are %d bp, the model takes %d" % (codes.shape[1], L))
    if labels.shape[1] != model._options["n_features"]:
        raise SystemExit("%d label columns, the model has %d tasks" % (labels.shape[1],
                                                                      model._options["n_features"]))
    perf = evaluate(model, codes, labels, args.batch_size, args.rev_complement)
    write_table(perf, args.output_dir)
    print(format_table(perf), end="")
    return perf


if __name__ == "__main__":
    main()
