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
`python -m explainn_amd.interpret ... --sites` writes (0.5 x each filter's largest activation) -- or,
with an error rate behind it, what `python -m explainn_amd.calibrate` writes from an empirical null:

    null = activation_null(model, background, shuffles=10)     # exact per-filter histogram of the activation
    calls = call_sites(model, codes, null.thresholds(1e-4), null=null)
    calls.pvalue                                        # (1 + null values >= score) / (1 + null size)

The float16 activation is never negative, so its 32768 bit patterns sort like the values: the null is a
32768-bin integer histogram per filter (explainn_activation_histogram, csrc/actnull.hip), and tails,
thresholds and p-values are exact functions of integers.  `--null NULL.npz` adds the p-value column.

    sq = site_qvalues(activation_null(model, codes), null)     # the scanned sequences' own histogram, no shuffles
    calls = call_sites(model, codes, sq.thresholds(0.05), null=null, qvalues=sq)
    calls.qvalue                                        # Benjamini-Hochberg over ALL positions and strands

A site's q-value is a function of (unit, bit pattern) too: explainn_site_qvalues (csrc/siteq.hip) forms the
table from the two histograms.  `--qvalues [--max-qvalue Q]` adds the column over the whole file.
"""
import argparse

import numpy as np
import torch

from .strands import TwoStrands, as_codes_1d, check_strands, eval_pass

CHUNK_POSITIONS = 1 << 24    # start positions per device call
MAX_SITES = 50000000         # records a call_sites() result may hold (17 bytes each on the host)


class SiteCalls:
    """Sites of every unit: unit u's records are [offsets[u], offsets[u+1]) of `start` (int64, 0-based
    start of the k-mer on the forward strand), `strand` (int8, +1 / -1) and `score` (float32: the
    float16 activation).  Per unit: '+' sites in ascending start, then '-' sites in ascending start."""

    def __init__(self, offsets, start, strand, score, kernel_size, pvalue=None, qvalue=None):
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.start = np.asarray(start, dtype=np.int64)
        self.strand = np.asarray(strand, dtype=np.int8)
        self.score = np.asarray(score, dtype=np.float32)
        self.kernel_size = int(kernel_size)
        n = int(self.offsets[-1])
        if self.offsets.ndim != 1 or self.offsets[0] != 0 or np.any(np.diff(self.offsets) < 0) or \
                not (len(self.start) == len(self.strand) == len(self.score) == n):
            raise ValueError("offsets must be an ascending scan from 0 that ends at the record count")
        # float64 empirical p-value of every record against an ActivationNull; None without a null
        self.pvalue = None if pvalue is None else np.asarray(pvalue, dtype=np.float64)
        if self.pvalue is not None and self.pvalue.shape != (n,):
            raise ValueError("pvalue must hold one value per record")
        # float64 Benjamini-Hochberg q-value of every record over all the tests of its unit (SiteQvalues); None
        # without one
        self.qvalue = None if qvalue is None else np.asarray(qvalue, dtype=np.float64)
        if self.qvalue is not None and self.qvalue.shape != (n,):
            raise ValueError("qvalue must hold one value per record")

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
    check_strands(strands)
    if chunk_positions is not None and int(chunk_positions) < 1:
        raise ValueError("chunk_positions must be at least 1 (got %r)" % (chunk_positions,))
    if int(max_sites) < 0:
        raise ValueError("max_sites must not be negative")
    if int(period) < 0:
        raise ValueError("period must not be negative")


def check_pvalue(pvalue):
    if not 0.0 <= float(pvalue) <= 1.0:
        raise ValueError("pvalue must be in [0, 1] (got %r)" % (pvalue,))


def _too_many(counts, total, max_sites, names=None,
              advice="A threshold of 0 makes every position a site: raise those thresholds, or max_sites"):
    top = np.argsort(-counts, kind="stable")[:5]
    name = (lambda u: "filter%d" % u) if names is None else (lambda u: names[u])
    return ValueError("more than max_sites = %d sites (%d so far); the units with the most: %s.  %s" % (
        max_sites, total, ", ".join("%s (%d)" % (name(u), counts[u]) for u in top if counts[u] > 0), advice))


# ---------------------------------------------------------------- one site list from chunks and legs
# A site list's rows are 2 * unit + (strand < 0).  A LEG is one device-side lister of some of those rows
# (call_sites: a strand of a model, rows = its units; scan_motifs: all rows at once):
#   leg.rows                     int64, the canonical row of each of the leg's own rows
#   leg.count(piece, cnt)        enqueues the count of a chunk's cnt starts; returns a callable that finishes
#                                it and gives the host offsets (len(rows) + 1)
#   leg.emit(piece, cnt, total)  likewise for the records: (pos relative to the chunk, *columns)
def site_blocks(pieces, legs, units, max_sites, too_many):
    """Blocks (first position, rows, offsets, pos, *columns) of every chunk and leg.  pieces: (first start,
    number of starts, the chunk's codes with the overlap behind them) in ascending order; what has to happen
    around a chunk happens in that iterator.  Per chunk every leg's count is started before any is finished,
    the counts are added (more than max_sites records: raise too_many(counts per unit, total) before
    anything of the chunk is emitted), and the same for emit, into buffers of exactly the counted size."""
    counts, blocks = np.zeros(2 * units, dtype=np.int64), []
    for p0, cnt, piece in pieces:
        offs = [finish() for finish in [leg.count(piece, cnt) for leg in legs]]     # the one read of the totals
        for leg, o in zip(legs, offs):
            counts[leg.rows] += np.diff(o)
        if int(counts.sum()) > max_sites:
            raise too_many(counts.reshape(units, 2).sum(axis=1), int(counts.sum()), int(max_sites))
        emits = [(leg, o, leg.emit(piece, cnt, int(o[-1]))) for leg, o in zip(legs, offs) if int(o[-1]) > 0]
        for leg, o, finish in emits:
            blocks.append((p0, leg.rows, o) + tuple(finish()))
    return blocks


def assemble(blocks, units, columns):
    """(offsets over units, start int64, strand int8, *columns) of site_blocks' blocks, chunks in ascending
    order; columns: the dtype of each record column.  One stable sort by canonical row keeps, inside every
    unit, '+' before '-' and ascending starts."""
    if not blocks:
        return (np.zeros(units + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int8)) + tuple(
            np.zeros(0, dt) for dt in columns)
    row = np.concatenate([np.repeat(np.asarray(rows, dtype=np.int64), np.diff(o)) for _, rows, o, *_ in blocks])
    start = np.concatenate([np.asarray(b[3], dtype=np.int64) + b[0] for b in blocks])
    order = np.argsort(row, kind="stable")
    per_row = np.bincount(row, minlength=2 * units)
    offsets = np.zeros(units + 1, dtype=np.int64)
    np.cumsum(per_row.reshape(units, 2).sum(axis=1), out=offsets[1:])
    return (offsets, start[order], np.repeat(np.tile(np.array([1, -1], np.int8), units), per_row)) + tuple(
        np.concatenate([np.asarray(b[4 + i], dtype=dt) for b in blocks])[order] for i, dt in enumerate(columns))


def concat_units(a, b):
    """A SiteCalls whose units are a's followed by b's (two calls over the same coordinates: a model's filters
    and known motifs, say); kernel_size is the larger of the two, and pvalue and qvalue are each kept only if both
    carry one.  spacing.spacing() of it counts filter-versus-filter, filter-versus-motif and motif-versus-motif
    pairs."""
    pvalue = None if a.pvalue is None or b.pvalue is None else np.concatenate([a.pvalue, b.pvalue])
    qvalue = None if a.qvalue is None or b.qvalue is None else np.concatenate([a.qvalue, b.qvalue])
    return SiteCalls(np.concatenate([a.offsets, b.offsets[1:] + a.offsets[-1]]), np.concatenate([a.start, b.start]),
                     np.concatenate([a.strand, b.strand]), np.concatenate([a.score, b.score]),
                     max(a.kernel_size, b.kernel_size), pvalue, qvalue)


class _StrandLeg:
    """One strand of a model (or of its eval_replica()) on one stream: rows = the units."""

    def __init__(self, model, stream, thr, period, strand):
        self.model, self.stream, self.thr, self.period, self.rc = model, stream, thr, period, strand < 0
        self.rows = 2 * np.arange(model._units(), dtype=np.int64) + int(self.rc)

    def _launch(self, piece, cnt, keep, **kwargs):
        with torch.cuda.stream(self.stream):
            out = self.model._launch_call_sites(piece, self.thr, 0, cnt, self.period, self.rc, **kwargs)
            host = [t.to("cpu", non_blocking=True) for t in out[keep]]

        def finish():
            self.stream.synchronize()
            return [t.numpy() for t in host]
        return finish

    def count(self, piece, cnt):
        finish = self._launch(piece, cnt, slice(0, 1))
        return lambda: finish()[0]

    def emit(self, piece, cnt, total):
        return self._launch(piece, cnt, slice(1, 3), capacity=total)


def call_sites(model, codes, thresholds, strands="both", chunk_positions=None, max_sites=MAX_SITES, period=0,
               null=None, qvalues=None):
    """Every site of every unit of `model` (an ExplaiNN, or an ExplaiNNBank: global unit indices) in
    `codes`: 1-D uint8 base codes (0..3 = A,C,G,T, 4 = N), numpy array or tensor, host or device.

    thresholds: (units,) floats; (u, p) is a site when the float16 eval-mode activation of unit u on
    codes[p : p + k] exceeds thresholds[u].  strands="both" also lists, as strand -1 at the same forward
    coordinate p, the sites of the filter on the reverse complement of codes[p : p + k].  period > 0:
    codes is a concatenation of records of `period` bases and no site crosses a record boundary.
    The sequence goes to the device in chunks of chunk_positions starts (default 2^24) that overlap by
    k - 1 bases; each chunk and strand takes a count call, one read of the total, and an emit call
    into a buffer of exactly that size.  The two strands run on the model and its eval_replica() on two
    streams.  More than max_sites records raise ValueError.  null: an ActivationNull of this model; the
    result then carries `pvalue`, the empirical p-value of every record.  qvalues: a SiteQvalues of this model
    (site_qvalues); the result then carries `qvalue`.  Returns a SiteCalls."""
    _check_args(strands, chunk_positions, max_sites, period)
    k, units = model._options["kernel_size"], model._units()
    if qvalues is not None and (qvalues.units, qvalues.kernel_size) != (units, k):
        raise ValueError("the q-values are of %d units of kernel size %d, the model of %d of %d" % (
            qvalues.units, qvalues.kernel_size, units, k))
    if null is not None and (null.units, null.kernel_size) != (units, k):
        raise ValueError("the null is of %d units of kernel size %d, the model of %d of %d" % (
            null.units, null.kernel_size, units, k))
    data = as_codes_1d(codes)
    thr = torch.as_tensor(np.asarray(thresholds.detach().cpu() if torch.is_tensor(thresholds) else thresholds,
                                     dtype=np.float32))
    if tuple(thr.shape) != (units,):
        raise RuntimeError("thresholds must hold one value per unit: shape (%d,), got %s" % (units, tuple(thr.shape)))
    n_positions = max(int(data.shape[0]) - k + 1, 0)
    if model.training:
        raise NotImplementedError("calling sites is an eval-mode export path; call model.eval()")
    device = model._device()
    both = strands == "both"
    blocks = []
    if n_positions > 0:
        thr = thr.to(device)
        chunk = int(chunk_positions) if chunk_positions is not None else CHUNK_POSITIONS
        # count and emit of the two strands interleave, so the legs are driven by site_blocks, not by ts.run
        with TwoStrands(model, both) as ts:
            cur, side = ts.cur, ts.side

            def pieces():
                for p0, cnt in position_chunks(n_positions, chunk, period):
                    piece = data[p0:p0 + cnt + k - 1].to(device).contiguous()
                    if both:
                        side.wait_stream(cur)                   # the chunk and thresholds are on the device
                        piece.record_stream(side)
                        thr.record_stream(side)
                    yield p0, cnt, piece
                    if both:
                        cur.wait_stream(side)

            legs = [_StrandLeg(model, cur, thr, period, 1)]
            if both:
                legs.append(_StrandLeg(ts.rep, side, thr, period, -1))
            blocks = site_blocks(pieces(), legs, units, max_sites, _too_many)
    calls = SiteCalls(*assemble(blocks, units, (np.float32,)), k)
    if null is not None:
        calls.pvalue = null.pvalue(calls.unit_ids(), calls.score)
    if qvalues is not None:
        calls.qvalue = qvalues.qvalue(calls.unit_ids(), calls.score)
    return calls


ACT_BINS = 32768             # non-negative float16 bit patterns (EXPLAINN_ACT_BINS)
ACT_INF = 0x7C00             # the pattern of +inf; the patterns above it are NaNs


def _null_stats(hist, alpha, want_tail=False, want_thresholds=False):
    """(tail, total, thresholds) of a device int64 (units, ACT_BINS) histogram (explainn_activation_null);
    tail / thresholds None unless asked for."""
    from . import _lib
    units, dev = hist.shape[0], hist.device
    total = torch.empty(units, device=dev, dtype=torch.int64)
    tail = torch.empty_like(hist) if want_tail else None
    thr = torch.empty(units, device=dev, dtype=torch.float32) if want_thresholds else None
    _lib.call("explainn_activation_null", dev, hist, units, float(alpha), tail, total, thr)
    return tail, total, thr


def _unit_bits(unit_ids, scores, units):
    """(int64 unit ids, int64 float16 bit patterns of the scores), checked: the index of a record in a
    (units, ACT_BINS) table."""
    unit = np.asarray(unit_ids, dtype=np.int64)
    with np.errstate(over="ignore"):                  # a score past 65504 is +inf in float16
        bits = (np.asarray(scores, dtype=np.float32).astype(np.float16).view(np.uint16).astype(np.int64)
                & (ACT_BINS - 1))
    if unit.shape != bits.shape or unit.ndim != 1:
        raise ValueError("unit_ids and scores must be 1-D and of one length")
    if len(unit) and (unit.min() < 0 or unit.max() >= units):
        raise IndexError("unit ids outside [0, %d)" % units)
    return unit, bits


class ActivationNull:
    """The empirical null of a model's filter activations: `hist` int64 (units, 32768) on the device,
    hist[u][b] = how many background k-mers gave unit u the float16 activation with bit pattern b;
    `tail[u][b]` = how many gave at least that value; `total[u]` = how many there were.  Integers
    throughout: thresholds and p-values are exact."""

    def __init__(self, hist, kernel_size, strands="both", shuffles=0, seed=0):
        if not torch.is_tensor(hist) or hist.dtype != torch.int64 or hist.dim() != 2 or \
                hist.shape[1] != ACT_BINS or hist.device.type != "cuda":
            raise ValueError("hist must be an int64 tensor of shape (units, %d) on a HIP device" % ACT_BINS)
        self.hist = hist.contiguous()
        self.kernel_size, self.strands, self.shuffles, self.seed = int(kernel_size), strands, int(shuffles), int(seed)
        if bool(self.hist[:, ACT_INF + 1:].any()):
            raise ValueError("the null holds NaN activations (bins above 0x7C00): the model's parameters are "
                             "not finite")
        self.tail, self.total, _ = _null_stats(self.hist, 0.0, want_tail=True)

    @property
    def units(self):
        return self.hist.shape[0]

    def thresholds(self, pvalue):
        """(units,) float32: per unit the smallest float16 value t such that at most
        floor(pvalue * total) of the null's activations are > t -- call_sites with it calls at most that
        many of the background's positions; +inf for a unit without a null."""
        check_pvalue(pvalue)
        return _null_stats(self.hist, pvalue, want_thresholds=True)[2].cpu().numpy()

    def pvalue(self, unit_ids, scores):
        """float64 (n,): (1 + null activations of the unit >= float16(score)) / (1 + total): the add-one
        empirical p-value, resolution 1 / (total + 1).  Gathered on the device; only the n values cross."""
        unit, bits = _unit_bits(unit_ids, scores, self.units)
        if len(unit) == 0:
            return np.zeros(0, dtype=np.float64)
        dev = self.hist.device
        u = torch.from_numpy(unit).to(dev)
        idx = u * ACT_BINS + torch.from_numpy(bits).to(dev)
        tail = self.tail.view(-1)[idx].cpu().numpy()
        total = self.total[u].cpu().numpy()
        return (1.0 + tail.astype(np.float64)) / (1.0 + total.astype(np.float64))

    def save(self, path):
        """.npz of the non-zero (unit, bin, count) triples, the totals and how the null was drawn."""
        nz = self.hist.nonzero()
        with open(path, "wb") as fh:
            np.savez(fh, unit=nz[:, 0].cpu().numpy().astype(np.int32), bin=nz[:, 1].cpu().numpy().astype(np.uint16),
                     count=self.hist[nz[:, 0], nz[:, 1]].cpu().numpy(), total=self.total.cpu().numpy(),
                     k=np.int64(self.kernel_size), units=np.int64(self.units), strands=np.str_(self.strands),
                     shuffles=np.int64(self.shuffles), seed=np.int64(self.seed))

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path) as z:
            hist = np.zeros((int(z["units"]), ACT_BINS), dtype=np.int64)
            hist[z["unit"].astype(np.int64), z["bin"].astype(np.int64)] = z["count"]
            if not np.array_equal(hist.sum(axis=1), z["total"]):
                raise ValueError("%s: the counts do not add up to the stored totals" % path)
            return cls(torch.from_numpy(hist).to(device), int(z["k"]), str(z["strands"]), int(z["shuffles"]),
                       int(z["seed"]))


def _count_activations(model, data, hist, period, shuffles, seed, both, chunk):
    """Adds the activations of `data` (1-D uint8, host or device) -- or, with shuffles = R > 0, of R
    dinucleotide shuffles of each of its records of `period` bases -- into hist, chunk by chunk."""
    k = model._options["kernel_size"]
    device = hist.device
    strands = (False, True) if both else (False,)
    if shuffles > 0:
        from .sequence import dinucleotide_shuffle_device
        rows = data.view(-1, period)
        per = max(chunk // period, 1)
        for r0 in range(0, rows.shape[0], per):
            shuf = dinucleotide_shuffle_device(rows[r0:r0 + per].to(device), shuffles, seed, row0=r0).view(-1)
            for rc in strands:
                model._launch_activation_histogram(shuf, hist, 0, None, period, rc)
        return
    n_positions = max(int(data.shape[0]) - k + 1, 0)
    for p0, cnt in position_chunks(n_positions, chunk, period):
        piece = data[p0:p0 + cnt + k - 1].to(device).contiguous()
        for rc in strands:
            model._launch_activation_histogram(piece, hist, 0, cnt, period, rc)


def _null_args(model, codes, period, shuffles, strands, chunk_positions):
    """The checks of activation_null: returns (1-D uint8 tensor, period)."""
    _check_args(strands, chunk_positions, 0, period)
    data = codes if torch.is_tensor(codes) else torch.as_tensor(np.ascontiguousarray(codes))
    if data.dtype != torch.uint8 or data.dim() not in (1, 2):
        raise ValueError("codes must be a 1-D, or (N, L), uint8 array of base codes")
    if data.dim() == 2:
        if period not in (0, data.shape[1]):
            raise ValueError("(N, L) codes mean period = L = %d (got period %d)" % (data.shape[1], period))
        period = int(data.shape[1])
        data = data.contiguous().view(-1)
    if int(shuffles) < 0:
        raise ValueError("shuffles must not be negative")
    if shuffles > 0 and (period < 1 or data.shape[0] % period != 0):
        raise ValueError("a shuffled background needs records: a period that divides the number of bases")
    if model.training:
        raise NotImplementedError("the activation null is an eval-mode export path; call model.eval()")
    return data.contiguous(), int(period)


def activation_null(model, codes, period=0, shuffles=0, seed=0, strands="both", chunk_positions=None):
    """The empirical null of every unit of `model` (an ExplaiNN or an ExplaiNNBank) over a background:
    the exact histogram of the float16 activation call_sites thresholds, at every live start of `codes`
    (1-D uint8 with `period` as in call_sites, or (N, L): period = L), both strands counted into one
    histogram unless strands="fwd".  shuffles = R > 0 (needs a period): the background is R
    dinucleotide-preserving shuffles of every record, drawn on the device chunk by chunk
    (sequence.dinucleotide_shuffle_device with `seed` and the chunk's first row as row0 -- a pure
    function of (seed, row, r), so the result does not depend on chunk_positions) instead of the
    records themselves.  The codes go to the device in chunks as position_chunks cuts them (whole
    records with a period).  Returns an ActivationNull."""
    data, period = _null_args(model, codes, period, shuffles, strands, chunk_positions)
    device = model._device()
    hist = torch.zeros(model._units(), ACT_BINS, device=device, dtype=torch.int64)
    chunk = int(chunk_positions) if chunk_positions is not None else CHUNK_POSITIONS
    with eval_pass(model):
        _count_activations(model, data, hist, period, int(shuffles), seed, strands == "both", chunk)
    return ActivationNull(hist, model._options["kernel_size"], strands, shuffles, seed)


def records_null(model, records, strands="both", seed=0):
    """One ActivationNull over the k-mers of every record's own codes (records of any lengths: an iterable of 1-D
    uint8 arrays), no k-mer across two records: the observed histogram site_qvalues needs, and the background of
    `calibrate --background sequence` when the records' lengths differ."""
    check_strands(strands)
    hist = torch.zeros(model._units(), ACT_BINS, device=model._device(), dtype=torch.int64)
    with eval_pass(model):
        for c in records:
            if len(c):
                data, _ = _null_args(model, np.asarray(c, dtype=np.uint8), 0, 0, strands, None)
                _count_activations(model, data, hist, 0, 0, seed, strands == "both", CHUNK_POSITIONS)
    return ActivationNull(hist, model._options["kernel_size"], strands, 0, seed)


# ---------------------------------------------------------------- q-values
def check_qvalue(alpha):
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("qvalue must be in [0, 1] (got %r)" % (alpha,))


def site_qtable(obs, p, alpha=0.0):
    """(q float64 (units, bins), total int64 (units,), first int32 (units,)) of explainn_site_qvalues, on the
    device: the Benjamini-Hochberg q-value of every score bin over ALL the tests of its unit.  obs: device int64
    (units, bins), the tests per bin; p: device float64 (units, bins), the p-value of the bin, non-increasing in
    the bin; first[u] = the smallest bin with q <= alpha (bins if none).  No host synchronisation."""
    from . import _lib
    if not torch.is_tensor(obs) or obs.dim() != 2 or not 1 <= obs.shape[1] <= _lib.SITEQ_MAX_BINS:
        raise ValueError("obs must be a (units, bins) tensor with 1 <= bins <= %d" % _lib.SITEQ_MAX_BINS)
    check_qvalue(alpha)
    units, bins = obs.shape
    _lib.require(obs, torch.int64, (units, bins), None, "obs")
    _lib.require(p, torch.float64, (units, bins), obs.device, "p")
    q = torch.empty((units, bins), dtype=torch.float64, device=obs.device)
    total = torch.empty((units,), dtype=torch.int64, device=obs.device)
    first = torch.empty((units,), dtype=torch.int32, device=obs.device)
    _lib.call("explainn_site_qvalues", obs.device, obs, p, units, bins, float(alpha), q, total, first)
    return q, total, first


class SiteQvalues:
    """The q-values of a model's filter sites: `q` float64 (units, 32768) on the device, q[u][b] = the
    Benjamini-Hochberg q-value of a site of unit u whose float16 activation has the bit pattern b, over all
    `total[u]` tests of the unit -- every live start and strand of the scanned sequences, not only the called
    sites, so it does not depend on a threshold.  Exact: a function of two integer histograms."""

    def __init__(self, observed, p, kernel_size, strands):
        self._obs, self._p, self.kernel_size, self.strands = observed, p, int(kernel_size), strands
        self.q, self.total, _ = site_qtable(observed, p)

    @property
    def units(self):
        return self.q.shape[0]

    def first(self, alpha):
        """int64 (units,): per unit the smallest bit pattern with q <= alpha; 32768 if none."""
        return site_qtable(self._obs, self._p, alpha)[2].cpu().numpy().astype(np.int64)

    def thresholds(self, alpha):
        """(units,) float32 thresholds at which call_sites (activation > threshold) lists exactly the sites with
        q <= alpha: the float16 value one bit pattern below the first that qualifies; +inf where none does (or
        only NaN patterns would), -1 where every pattern does."""
        first = self.first(alpha)
        below = np.clip(first - 1, 0, ACT_INF).astype(np.uint16).view(np.float16).astype(np.float32)
        return np.where(first == 0, np.float32(-1.0), below).astype(np.float32)

    def qvalue(self, unit_ids, scores):
        """float64 (n,): q[unit][bits(float16(score))], gathered on the device; only the n values cross."""
        unit, bits = _unit_bits(unit_ids, scores, self.units)
        if len(unit) == 0:
            return np.zeros(0, dtype=np.float64)
        dev = self.q.device
        return self.q.view(-1)[torch.from_numpy(unit).to(dev) * ACT_BINS + torch.from_numpy(bits).to(dev)].cpu().numpy()


def site_qvalues(observed, null):
    """The SiteQvalues of scanned sequences against a background.  observed: the ActivationNull of the scanned
    sequences themselves -- activation_null(model, codes, period=..., strands=...) without shuffles, with the
    strands and period call_sites will use (records_null for records of unequal lengths) -- so that its histogram
    holds every test call_sites makes.  null: the background's ActivationNull; a pattern's p-value is
    (1 + null.tail) / (1 + null.total) in fp64, the expression ActivationNull.pvalue evaluates."""
    if (observed.units, observed.kernel_size, observed.strands) != (null.units, null.kernel_size, null.strands):
        raise ValueError("observed is of %d units of kernel size %d on strands %r, the null of %d of %d on %r" % (
            observed.units, observed.kernel_size, observed.strands, null.units, null.kernel_size, null.strands))
    if observed.shuffles:
        raise ValueError("observed must count the scanned sequences themselves, not shuffles of them")
    if observed.hist.device != null.hist.device:
        raise ValueError("observed and null must be on one device")
    p = (1.0 + null.tail.to(torch.float64)) / (1.0 + null.total.to(torch.float64))[:, None]
    return SiteQvalues(observed.hist, p, null.kernel_size, null.strands)


def call_sites_records(model, records, thresholds, **kwargs):
    """call_sites() over (id, codes) pairs (loader.read_fasta_records): yields (id, SiteCalls)."""
    for rid, codes in records:
        yield rid, call_sites(model, codes, thresholds, **kwargs)


def bed_rows(seq_id, calls, names=None, widths=None):
    """BED6 lines of one record: `SeqId start end name score strand`, 0-based half-open, sorted by
    (start, unit, strand) with '+' before '-'.  name: names[unit], filter<u> without names; end: start +
    widths[unit], start + the kernel size without widths.  Calls that carry p-values get them as a seventh
    column."""
    unit = calls.unit_ids()
    order = np.lexsort((-calls.strand, unit, calls.start))
    rows = []
    for i in order:
        u = unit[i]
        row = "%s\t%d\t%d\t%s\t%.6g\t%s" % (
            seq_id, calls.start[i], calls.start[i] + (calls.kernel_size if widths is None else widths[u]),
            "filter%d" % u if names is None else names[u], calls.score[i], "+" if calls.strand[i] > 0 else "-")
        if calls.pvalue is not None:
            row += "\t%.6g" % calls.pvalue[i]
        if calls.qvalue is not None:
            row += "\t%.6g" % calls.qvalue[i]
        rows.append(row + "\n")
    return rows


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
    ap.add_argument("--null", help="NULL.npz of `python -m explainn_amd.calibrate --save-null`: adds a seventh "
                                   "column, the empirical p-value of the site's score")
    ap.add_argument("--qvalues", action="store_true",
                    help="needs --null: a first pass counts every activation of the file, and a further column holds "
                         "the site's Benjamini-Hochberg q-value over all positions and strands of the file")
    ap.add_argument("--max-qvalue", type=float, default=None,
                    help="with --qvalues: list only the sites at or below this q-value (and above the thresholds)")
    return ap


def main(argv=None):
    """FASTA records of any length -> BED6 (SeqId, start, end, filter<u>, score, strand): one row per
    motif site, 0-based half-open, sorted by (start, filter, strand) within a record.  With --null a
    seventh column holds the site's empirical p-value; with --qvalues an eighth its q-value over the whole file."""
    args = _parser().parse_args(argv)
    if args.qvalues and not args.null:
        raise SystemExit("--qvalues needs --null")
    if args.max_qvalue is not None and not (args.qvalues and 0.0 <= args.max_qvalue <= 1.0):
        raise SystemExit("--max-qvalue needs --qvalues and a value in [0, 1]")
    from .loader import open_output, read_fasta_records
    from .predict import _load_model
    records = read_fasta_records(args.fasta_file)
    model = _load_model(args.model_file)
    model.eval()
    thresholds = read_thresholds(args.thresholds, model._units())
    null = ActivationNull.load(args.null, model._device()) if args.null else None
    kwargs = {"null": null} if null is not None else {}
    if args.qvalues:
        # q-values are over the whole file: one pass counts every test, the second lists the sites
        if null.strands != args.strands:
            raise SystemExit("the null counts strands %r, --strands is %r" % (null.strands, args.strands))
        kwargs["qvalues"] = site_qvalues(records_null(model, (c for _, c in records), args.strands), null)
        if args.max_qvalue is not None:
            thresholds = np.maximum(thresholds, kwargs["qvalues"].thresholds(args.max_qvalue))
    with open_output(args.output_file) as fh:
        for rid, calls in call_sites_records(model, records, thresholds, strands=args.strands, **kwargs):
            fh.writelines(bed_rows(rid, calls))


if __name__ == "__main__":
    main()
