"""Where does each motif occur?  Every above-threshold filter hit of a sequence, listed on the device.

A trained ExplaiNN is a bank of motif detectors; the reference lists a filter's sites by walking the
dense float16 (N,U,Lo) activation array on the host (interpret.py:375-429) and vendors PWMScan to
annotate longer sequences.  In eval mode a filter's activation at a position depends only on the k
bases under it, so one pass over the base codes (explainn_call_sites, csrc/sites.hip) lists every
(unit, position) whose float16 activation exceeds the unit's threshold -- the positions np.where
finds in float16(model.linears[:3](windows)), bit for bit, without the windows or the array.

    calls = call_sites(model, codes, thresholds)        # both strands
    start, strand, score = calls.unit(3)                # '+' sites ascending, then '-' sites ascending

`python -m explainn_amd.sites MODEL FASTA -t thresholds.tsv` writes BED6; `thresholds.tsv` is what
`python -m explainn_amd.interpret ... --sites` writes (0.5 x each filter's largest activation).
"""
import argparse
import contextlib
import sys

import numpy as np
import torch

CHUNK_POSITIONS = 1 << 24    # start positions per device call
MAX_SITES = 50000000         # records a call_sites() result may hold (17 bytes each on the host)


class SiteCalls:
    """Sites of every unit: unit u's records are [offsets[u], offsets[u+1]) of `start` (int64, 0-based
    start of the k-mer on the forward strand), `strand` (int8, +1 / -1) and `score` (float32: the
    float16 activation).  Per unit: '+' sites in ascending start, then '-' sites in ascending start."""

    def __init__(self, offsets, start, strand, score, kernel_size):
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.start = np.asarray(start, dtype=np.int64)
        self.strand = np.asarray(strand, dtype=np.int8)
        self.score = np.asarray(score, dtype=np.float32)
        self.kernel_size = int(kernel_size)
        n = int(self.offsets[-1])
        if self.offsets.ndim != 1 or self.offsets[0] != 0 or np.any(np.diff(self.offsets) < 0) or \
                not (len(self.start) == len(self.strand) == len(self.score) == n):
            raise ValueError("offsets must be an ascending scan from 0 that ends at the record count")

    @property
    def units(self):
        return len(self.offsets) - 1

    def __len__(self):
        return int(self.offsets[-1])

    def unit(self, u):
        """(start, strand, score) of unit u (global unit index on a bank)."""
        if not 0 <= u < self.units:
            raise IndexError("unit %d outside [0, %d)" % (u, self.units))
        lo, hi = self.offsets[u], self.offsets[u + 1]
        return self.start[lo:hi], self.strand[lo:hi], self.score[lo:hi]

    def unit_ids(self):
        """int64 unit index of every record."""
        return np.repeat(np.arange(self.units, dtype=np.int64), np.diff(self.offsets))


def position_chunks(n_positions, chunk, period=0):
    """[(first start position, count), ...] covering 0..n_positions-1 in runs of at most `chunk`.  Chunk
    (p0, c) reads the bases [p0, p0 + c + k - 1): neighbours overlap by k - 1 bases and every start
    belongs to exactly one chunk.  With a record period the runs begin on record boundaries (the
    chunk is rounded down to whole records, one record at least)."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk_positions must be at least 1 (got %d)" % chunk)
    if period > 0:
        chunk = max(chunk // period, 1) * period
    return [(p0, min(chunk, n_positions - p0)) for p0 in range(0, n_positions, chunk)]


def _check_args(strands, chunk_positions, max_sites, period):
    if strands not in ("both", "fwd"):
        raise ValueError("strands must be 'both' or 'fwd' (got %r)" % (strands,))
    if chunk_positions is not None and int(chunk_positions) < 1:
        raise ValueError("chunk_positions must be at least 1 (got %r)" % (chunk_positions,))
    if int(max_sites) < 0:
        raise ValueError("max_sites must not be negative")
    if int(period) < 0:
        raise ValueError("period must not be negative")


def _too_many(counts, total, max_sites):
    top = np.argsort(-counts, kind="stable")[:5]
    return ValueError(
        "more than max_sites = %d sites (%d so far); the units with the most: %s.  A threshold of 0 makes "
        "every position a site: raise those thresholds, or max_sites" % (
            max_sites, total, ", ".join("filter%d (%d)" % (u, counts[u]) for u in top if counts[u] > 0)))


def assemble(blocks, units, kernel_size):
    """SiteCalls from per-call blocks [(strand, first position, offsets (units+1), pos, score), ...]
    given forward strand first and chunks in ascending order within a strand: a stable sort by unit
    keeps, inside every unit, '+' before '-' and ascending starts."""
    if not blocks:
        return SiteCalls(np.zeros(units + 1, np.int64), [], [], [], kernel_size)
    unit = np.concatenate([np.repeat(np.arange(units, dtype=np.int64), np.diff(o)) for _, _, o, _, _ in blocks])
    start = np.concatenate([np.asarray(p, dtype=np.int64) + p0 for _, p0, _, p, _ in blocks])
    strand = np.concatenate([np.full(len(p), s, dtype=np.int8) for s, _, _, p, _ in blocks])
    score = np.concatenate([np.asarray(sc, dtype=np.float32) for _, _, _, _, sc in blocks])
    order = np.argsort(unit, kind="stable")
    offsets = np.zeros(units + 1, dtype=np.int64)
    np.cumsum(np.bincount(unit, minlength=units), out=offsets[1:])
    return SiteCalls(offsets, start[order], strand[order], score[order], kernel_size)


def call_sites(model, codes, thresholds, strands="both", chunk_positions=None, max_sites=MAX_SITES, period=0):
    """Every site of every unit of `model` (an ExplaiNN, or an ExplaiNNBank: global unit indices) in
    `codes`: 1-D uint8 base codes (0..3 = A,C,G,T, 4 = N), numpy array or tensor, host or device.

    thresholds: (units,) floats; (u, p) is a site when the float16 eval-mode activation of unit u on
    codes[p : p + k] exceeds thresholds[u].  strands="both" also lists, as strand -1 at the same forward
    coordinate p, the sites of the filter on the reverse complement of codes[p : p + k].  period > 0:
    codes is a concatenation of records of `period` bases and no site crosses a record boundary.
    The sequence goes to the device in chunks of chunk_positions starts (default 2^24) that overlap by
    k - 1 bases; each chunk and strand takes a count call, one read of the total, and an emit call
    into a buffer of exactly that size.  The two strands run on the model and its eval_replica() on two
    streams.  More than max_sites records raise ValueError.  Returns a SiteCalls."""
    _check_args(strands, chunk_positions, max_sites, period)
    k, units = model._options["kernel_size"], model._units()
    data = codes if torch.is_tensor(codes) else torch.as_tensor(np.ascontiguousarray(codes))
    if data.dtype != torch.uint8 or data.dim() != 1:
        raise ValueError("codes must be a 1-D uint8 array of base codes")
    thr = torch.as_tensor(np.asarray(thresholds.detach().cpu() if torch.is_tensor(thresholds) else thresholds,
                                     dtype=np.float32))
    if tuple(thr.shape) != (units,):
        raise RuntimeError("thresholds must hold one value per unit: shape (%d,), got %s" % (units, tuple(thr.shape)))
    n_positions = max(int(data.shape[0]) - k + 1, 0)
    if model.training:
        raise NotImplementedError("calling sites is an eval-mode export path; call model.eval()")
    device = model._device()
    both = strands == "both"
    blocks = {1: [], -1: []}
    counts = np.zeros(units, dtype=np.int64)
    if n_positions > 0:
        thr = thr.to(device)
        cur = torch.cuda.current_stream(device)
        rep = side = None
        if both:
            rep = model.eval_replica()
            if model._rt.side_stream is None:
                model._rt.side_stream = torch.cuda.Stream(device)
            side = model._rt.side_stream
        chunk = int(chunk_positions) if chunk_positions is not None else CHUNK_POSITIONS
        legs = [(1, model, cur)] + ([(-1, rep, side)] if both else [])
        with torch.no_grad(), model.eval_cache(), (rep.eval_cache() if both else contextlib.nullcontext()):
            for p0, cnt in position_chunks(n_positions, chunk, period):
                piece = data[p0:p0 + cnt + k - 1].to(device).contiguous()
                if both:
                    side.wait_stream(cur)                       # the chunk and thresholds are on the device
                    piece.record_stream(side)
                    thr.record_stream(side)
                offs = {}
                for s, m, stream in legs:                       # count, both strands in flight
                    with torch.cuda.stream(stream):
                        offs[s] = m._launch_call_sites(piece, thr, 0, cnt, period, s < 0)[0].to(
                            "cpu", non_blocking=True)
                for s, m, stream in legs:
                    stream.synchronize()                        # the one read of the totals
                    counts += np.diff(offs[s].numpy())
                if int(counts.sum()) > max_sites:
                    raise _too_many(counts, int(counts.sum()), int(max_sites))
                out = {}
                for s, m, stream in legs:                       # emit, into buffers of exactly that size
                    total = int(offs[s][-1])
                    if total == 0:
                        continue
                    with torch.cuda.stream(stream):
                        _, pos, score = m._launch_call_sites(piece, thr, 0, cnt, period, s < 0, capacity=total)
                        out[s] = (pos.to("cpu", non_blocking=True), score.to("cpu", non_blocking=True))
                for s, m, stream in legs:
                    if s in out:
                        stream.synchronize()
                        blocks[s].append((s, p0, offs[s].numpy(), out[s][0].numpy(), out[s][1].numpy()))
                if both:
                    cur.wait_stream(side)
        if model.validate_input:
            if both:
                rep.check_input()
            model.check_input()
    return assemble(blocks[1] + blocks[-1], units, k)


def call_sites_records(model, records, thresholds, **kwargs):
    """call_sites() over (id, codes) pairs (loader.read_fasta_records): yields (id, SiteCalls)."""
    for rid, codes in records:
        yield rid, call_sites(model, codes, thresholds, **kwargs)


def bed_rows(seq_id, calls):
    """BED6 lines of one record: `SeqId start end filter<u> score strand`, 0-based half-open, sorted by
    (start, filter, strand) with '+' before '-'."""
    unit = calls.unit_ids()
    order = np.lexsort((-calls.strand, unit, calls.start))
    k = calls.kernel_size
    return ["%s\t%d\t%d\tfilter%d\t%.6g\t%s\n" % (seq_id, calls.start[i], calls.start[i] + k, unit[i],
                                                calls.score[i], "+" if calls.strand[i] > 0 else "-")
            for i in order]


def write_thresholds(path, thresholds):
    """thresholds.tsv: columns `filter`, `threshold`, one row per unit (filter<u>)."""
    with open(path, "wt") as fh:
        fh.write("filter\tthreshold\n")
        for u, t in enumerate(np.asarray(thresholds)):
            fh.write("filter%d\t%r\n" % (u, float(t)))


def read_thresholds(path, units):
    """The (units,) float32 thresholds of a thresholds.tsv; every filter0..filter<units-1> exactly once."""
    out = np.full(units, np.nan, dtype=np.float32)
    with open(path) as fh:
        header = fh.readline().rstrip("\n").split("\t")
        if header != ["filter", "threshold"]:
            raise ValueError("%s: expected the header 'filter<TAB>threshold'" % path)
        for line in fh:
            if not line.strip():
                continue
            name, _, value = line.rstrip("\n").partition("\t")
            if not name.startswith("filter") or not name[6:].isdigit() or int(name[6:]) >= units:
                raise ValueError("%s: %r is not one of filter0..filter%d" % (path, name, units - 1))
            if not np.isnan(out[int(name[6:])]):
                raise ValueError("%s: %s listed twice" % (path, name))
            out[int(name[6:])] = float(value)
    if np.isnan(out).any():
        raise ValueError("%s: no threshold for filter%d" % (path, int(np.flatnonzero(np.isnan(out))[0])))
    return out


def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.sites", description=main.__doc__)
    ap.add_argument("model_file")
    ap.add_argument("fasta_file")
    ap.add_argument("-t", "--thresholds", required=True, help="thresholds.tsv (filter, threshold)")
    ap.add_argument("-o", "--output-file")
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    return ap


def main(argv=None):
    """FASTA records of any length -> BED6 (SeqId, start, end, filter<u>, score, strand): one row per
    motif site, 0-based half-open, sorted by (start, filter, strand) within a record."""
    args = _parser().parse_args(argv)
    from .loader import read_fasta_records
    from .predict import _load_model
    records = read_fasta_records(args.fasta_file)
    model = _load_model(args.model_file)
    model.eval()
    thresholds = read_thresholds(args.thresholds, model._units())
    fh = open(args.output_file, "w") if args.output_file else sys.stdout
    try:
        for rid, calls in call_sites_records(model, records, thresholds, strands=args.strands):
            fh.writelines(bed_rows(rid, calls))
    finally:
        if fh is not sys.stdout:
            fh.close()


if __name__ == "__main__":
    main()
