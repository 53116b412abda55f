"""Scoring sequences longer than the model's `sequence_length` with overlapping windows.

The reference has no such entry point: its users cut a chromosome arm, a BAC or a set of peaks of
unequal length into windows on the host and hand the (W,4,L) matrix to predict.py -- L/stride times
the sequence in bytes and transfers, and the filter bank run again on every overlap.  Here the
sequence goes to the device once as base codes (1 byte per base) and the windows are cut there
(explainn_scan, include/explainn_hip.h); with a stride that is a multiple of 7 the filter bank can
run once over the sequence instead of once per window (mode "shared").

    starts, preds = scan(model, codes, stride=7)     # preds[i] = predict()'s row for window i

`python -m explainn_amd.scan MODEL FASTA` writes the windows of every FASTA record as TSV.
"""
import argparse

import numpy as np
import torch

from . import _lib
from .architectures import SequenceWindows
from .strands import TwoStrands, as_codes_1d, check_strands, stack_strands

MODES = {"auto": _lib.SCAN_AUTO, "windows": _lib.SCAN_WINDOWS, "shared": _lib.SCAN_SHARED}
_POOL = 7                    # MaxPool1d(7,7): the strides whose windows share one pooling grid
# Windows per device call, at most: bounds the logits of a call, and -- together with _CHUNK_TILES --
# the workspace of the shared track.
_CHUNK_PASSES = 32           # ... this many sub-batches of `batch_size` windows
_CHUNK_TILES = 4             # ... and a shared track of this many sub-batches of tiles


def window_starts(length, L, stride):
    """int64 starts of the windows of a sequence of `length` bases: W = (length - L)//stride + 1 of
    them, none when the sequence is shorter than L."""
    if stride < 1:
        raise ValueError("stride must be at least 1 (got %d)" % stride)
    W = (length - L) // stride + 1 if length >= L else 0
    return np.arange(W, dtype=np.int64) * stride


def chunk_limit(L, k, stride, batch_size):
    """Windows per device call.  A call's logits cover at most 32 sub-batches; with a stride that is
    a multiple of 7 the call may run on the shared track, whose workspace is one filter-bank output
    array (units x n x batch_size floats) per batch_size tiles: the limit keeps the track within
    _CHUNK_TILES such arrays (0.55 GB at 300 units, n = 26 and batch_size 4096), whatever the
    sequence length."""
    limit = _CHUNK_PASSES * batch_size
    if stride % _POOL == 0:
        n, m = (L - k + 1) // _POOL, stride // _POOL
        # J = ceil((m (W - 1) + n) / n) <= _CHUNK_TILES * batch_size
        limit = min(limit, (_CHUNK_TILES * batch_size * n - n) // m + 1)
    return max(1, limit)


def chunks(n_windows, limit):
    """[(first window, count), ...]: the windows 0..n_windows-1 in runs of at most `limit`.  Chunk
    (w0, c) reads the bases [w0*stride, (w0 + c - 1)*stride + L): boundaries on multiples of the
    stride, neighbours overlapping by L - stride, every window exactly once."""
    if limit < 1:
        raise ValueError("chunk limit must be at least 1")
    return [(w0, min(limit, n_windows - w0)) for w0 in range(0, n_windows, limit)]


def _check_args(stride, strands, mode):
    if stride < 1:
        raise ValueError("stride must be at least 1 (got %d)" % stride)
    check_strands(strands)
    if mode not in MODES:
        raise ValueError("mode must be one of %s (got %r)" % (", ".join(MODES), mode))
    if mode == "shared" and stride % _POOL:
        raise ValueError("mode 'shared' needs a stride that is a multiple of %d (got %d): windows share "
                         "pooled values only when they share MaxPool1d(7,7)'s grid" % (_POOL, stride))


def scan(model, codes, stride=7, strands="both", mode="auto", batch_size=4096, apply_sigmoid=False,
         chunk_windows=None):
    """Eval-mode predictions of every window codes[s : s + L], s = 0, stride, 2 stride, ...

    codes: 1-D uint8 base codes (0..3 = A,C,G,T, 4 = N), numpy array or tensor, host or device.
    Returns (starts, preds): starts (W,) int64, preds (W, T, 4) float64 in predict()'s order
    [Fwd, Rev, Mean, Max] -- (W, G, T, 4) for an ExplaiNNBank -- equal to predict() on the
    materialised windows.  strands="fwd" scores the forward strand only: columns 1..3 are NaN.
    mode: "windows" stages every window, "shared" (stride a multiple of 7) runs the filter bank once
    over the sequence, "auto" picks the one measured faster.  The two strands run on the model and
    its eval_replica() on two streams, as in predict().  A long sequence is scored in chunks of
    chunk_limit() windows (chunk_windows overrides it) whose windows are exactly those of the
    whole; a host sequence is transferred chunk by chunk."""
    stride = int(stride)
    _check_args(stride, strands, mode)
    o = model._options
    L, k = o["sequence_length"], o["kernel_size"]
    batch_size = max(1, int(batch_size))
    device = model.final.weight.device
    data = as_codes_1d(codes)
    starts = window_starts(data.shape[0], L, stride)
    W = len(starts)
    shape = tuple(model._logits_empty(0, torch.device("cpu")).shape[1:])
    out = np.full((W,) + shape + (4,), np.nan)
    if W == 0:
        return starts, out
    limit = int(chunk_windows) if chunk_windows is not None else chunk_limit(L, k, stride, batch_size)
    with TwoStrands(model, strands == "both") as ts:
        for w0, cnt in chunks(W, limit):
            piece = data[w0 * stride:(w0 + cnt - 1) * stride + L].to(device).contiguous()
            fwd, rev = ts.run(lambda m, rc: m._launch_scan(
                SequenceWindows(piece, 0, cnt, stride, rc, batch_size), MODES[mode]), held=(piece,))
            if rev is not None:
                out[w0:w0 + cnt] = stack_strands(fwd, rev).cpu().numpy()
            else:
                out[w0:w0 + cnt, ..., 0] = fwd.cpu().numpy()
    if apply_sigmoid:
        out = torch.sigmoid(torch.Tensor(out)).numpy()
    return starts, out


def scan_records(model, records, **kwargs):
    """scan() over (id, codes) pairs (loader.read_fasta_records): yields (id, starts, preds)."""
    for rid, codes in records:
        starts, preds = scan(model, codes, **kwargs)
        yield rid, starts, preds


def _load_model(model_file):
    from .predict import _load_model as load
    return load(model_file)


def main(argv=None):
    """FASTA records of any length -> long-format TSV (SeqId, Start, End, Class, Fwd, Rev, Mean, Max),
    one row per window and class; Start and End are 0-based, half-open."""
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.scan", description=main.__doc__)
    ap.add_argument("model_file")
    ap.add_argument("fasta_file")
    ap.add_argument("-s", "--stride", type=int, default=7)
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--mode", choices=tuple(MODES), default="auto")
    ap.add_argument("-o", "--output-file")
    ap.add_argument("--apply-sigmoid", action="store_true")
    args = ap.parse_args(argv)
    try:
        _check_args(args.stride, args.strands, args.mode)
    except ValueError as e:
        ap.error(str(e))
    from .loader import open_output, read_fasta_records
    records = read_fasta_records(args.fasta_file)
    model = _load_model(args.model_file)
    L = model._options["sequence_length"]
    with open_output(args.output_file) as fh:
        fh.write("SeqId\tStart\tEnd\tClass\tFwd\tRev\tMean\tMax\n")
        for rid, starts, preds in scan_records(model, records, stride=args.stride, strands=args.strands,
                                               mode=args.mode, apply_sigmoid=args.apply_sigmoid):
            for s, row in zip(starts, preds):
                for t in range(row.shape[0]):
                    fh.write("%s\t%d\t%d\t%d\t%s\n" % (rid, s, s + L, t, "\t".join(repr(float(v)) for v in row[t])))


if __name__ == "__main__":
    main()
