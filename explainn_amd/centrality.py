"""Are a filter's sites concentrated at the peak summit?  Motif centrality on summit-centred windows.

The question CentriMo of the MEME suite answers for PWMs: a motif that belongs to the assayed factor sits
where the ChIP-/ATAC-seq signal peaks, a co-factor's or a compositional one does not.  Two device passes
(csrc/central.hip) behind the best sites of explainn_amd.records; `pwmenrich` shares centred_records:

    pos = site_positions(model, peaks, thresholds)            # where every record's best site sits
    res = centrality(model, peaks, thresholds, control=None)  # or test_positions(pos)
    res.log_pvalue, res.region_start, res.region_end, res.center, res.count, res.sites, res.qvalue

site_positions: per record the best site of every filter (explainn_record_best: the largest float16 activation
over the record's live starts and strands, the lowest start among equal maxima) stays on the device and is
counted, where call_sites with the filter's threshold would call it, into a histogram over its start.  The
records are windows of one length L, so the bin is the start itself: start p and start M - 1 - p (M = L - k + 1)
are equally far from the centre, and the regions [j, M - 1 - j] are the centred ones.

centrality / test_positions: for every filter, every supplied threshold with enough sites and every region
(centred ones, or with local=True every range of starts) the one-sided binomial test of "more best sites in
the region than its share w / M of the starts explains", in fp64 on the device; the most significant
(threshold, region) is reported with its correction over everything tried.  With a control set the same
region is also tested against the control records' best sites (Fisher's exact test, one-sided).

Differences from CentriMo:
  * the score is the filter's own float16 activation and the thresholds are supplied (thresholds.tsv of
    `interpret --sites`, or of `calibrate` with an error rate behind them); several thresholds, each tried,
    play the part of --optimize-score;
  * among equal best activations of a record the lowest start is the site; CentriMo splits the count among
    them.  A filter whose activation saturates therefore piles its sites up at start 0: in local mode that
    can pass for a region at the left edge; the centred test is not affected, except through its widest
    regions, which reach the edges;
  * a region that holds no more sites than expected is given p = 1 without being evaluated (as `enrichment`
    does for thresholds), and the correction over the m (threshold, region) pairs tried is 1 - (1 - p)^m.

`python -m explainn_amd.centrality MODEL PEAKS.fa -t thresholds.tsv [-t more.tsv ...] [--control C.fa] [--local]
 [--min-width W] [--max-width W] [--min-sites N] -o OUT.tsv`
"""
import argparse

import numpy as np
import torch

from .enrichment import _strands, benjamini_hochberg
from .records import (FilterScorer, RecordBest, best_over_records, pack_site, record_codes, record_labels,
                      table_order)

COLUMNS = ("Filter", "Threshold", "Sites", "RegionStart", "RegionEnd", "Width", "Center", "Count", "Expected",
           "LogPvalue", "LogPadj", "Evalue", "Qvalue")
CONTROL_COLUMNS = ("CtrlSites", "CtrlCount", "LogFisher")
MAX_THRESHOLDS = 16          # EXPLAINN_CENTRALITY_MAX_THRESHOLDS
HIST_BYTES = 64 * 1024       # the [T][2][M] int32 histogram of one device call
_FIELDS = ("best_t", "best_lo", "best_width", "sites", "count", "n_tests", "log_pvalue", "log_padj", "ctrl_sites",
           "ctrl_count", "log_fisher")
_INT32, _FLOAT = ("best_t", "best_lo", "best_width"), ("log_pvalue", "log_padj", "log_fisher")
STAT_FORMAT = "%.6g\t%d\t%d\t%d\t%d\t%.1f\t%d\t%.4g\t%.6g\t%.6g\t%.4g\t%.4g"      # COLUMNS from Threshold on


def field_dtype(field, ns=np):
    """The dtype of one of _FIELDS in numpy (or, ns=torch, in torch)."""
    return ns.int32 if field in _INT32 else ns.float64 if field in _FLOAT else ns.int64


def check_thresholds(thresholds, units):
    """float32 (units, T) of `thresholds`, (units,) or (units, T) with 1 <= T <= 16."""
    thr = np.asarray(thresholds.detach().cpu() if torch.is_tensor(thresholds) else thresholds, dtype=np.float32)
    if thr.ndim == 1:
        thr = thr[:, None]
    if thr.ndim != 2 or thr.shape[0] != units or thr.shape[1] < 1:
        raise ValueError("thresholds must be (units,) or (units, T) with units = %d (got shape %s)" % (
            units, np.shape(thresholds)))
    if thr.shape[1] > MAX_THRESHOLDS:
        raise ValueError("at most %d thresholds per filter (got %d)" % (MAX_THRESHOLDS, thr.shape[1]))
    return np.ascontiguousarray(thr)


def check_widths(min_width, max_width, min_sites):
    """(min_width, max_width or None, min_sites) as ints; ValueError unless 1 <= min_width <= max_width and
    min_sites >= 0."""
    lo, hi, n = int(min_width), None if max_width is None else int(max_width), int(min_sites)
    if lo < 1 or (hi is not None and hi < lo):
        raise ValueError("need 1 <= min_width <= max_width (got %r, %r)" % (min_width, max_width))
    if n < 0:
        raise ValueError("min_sites must not be negative (got %r)" % (min_sites,))
    return lo, hi, n


def common_length(lengths, kernel_size):
    """The one length of the records that are at least kernel_size long (shorter ones are left out)."""
    live = sorted({int(n) for n in lengths if int(n) >= kernel_size})
    if not live:
        raise ValueError("no record is as long as the kernel (%d bases)" % kernel_size)
    if len(live) > 1:
        raise ValueError("centrality needs fixed-width summit windows: every record of at least %d bases must "
                         "have one length (got %s%s)" % (kernel_size, ", ".join(str(n) for n in live[:5]),
                                                         ", ..." if len(live) > 5 else ""))
    return live[0]


def region_coordinates(lo, width, kernel_size, length):
    """(region_start, region_end, center) of the regions [lo, lo + width - 1] of starts, in record
    coordinates: their k-mers span [lo, hi + k), and center = (lo + hi + k - L) / 2 is the offset of that span's
    middle from the record's.  width 0 (no region): 0, 0, NaN."""
    lo, width = np.asarray(lo, dtype=np.int64), np.asarray(width, dtype=np.int64)
    none = width <= 0
    hi = lo + width - 1
    return (np.where(none, 0, lo), np.where(none, 0, hi + kernel_size),
            np.where(none, np.nan, (lo + hi + kernel_size - length) / 2.0))


class SitePositions:
    """Where the best sites sit: `hist` int32 (units, T, 2, M), hist[u][t][set][p] = records of the primary
    (set 0) / control (set 1) set whose best site of unit u starts at p and passes thresholds[u][t]; `counts`
    int64 (2,) = (Np, Nc), the records in the test; `thresholds` float32 (units, T); `kernel_size` k and
    `length` L of the records, M = L - k + 1."""

    def __init__(self, hist, counts, thresholds, kernel_size, length, strands="both"):
        self.hist = np.ascontiguousarray(hist, dtype=np.int32)
        self.counts = np.asarray(counts, dtype=np.int64)
        self.kernel_size, self.length, self.strands = int(kernel_size), int(length), str(strands)
        if self.hist.ndim != 4 or self.hist.shape[2] != 2 or self.counts.shape != (2,):
            raise ValueError("hist must be (units, T, 2, M) and counts (2,)")
        self.thresholds = check_thresholds(thresholds, self.hist.shape[0])
        if self.thresholds.shape[1] != self.hist.shape[1] or self.hist.shape[3] != self.length - self.kernel_size + 1:
            raise ValueError("hist must hold T = %d thresholds and M = L - k + 1 = %d starts (got %s)" % (
                self.thresholds.shape[1], self.length - self.kernel_size + 1, self.hist.shape))

    @property
    def units(self):
        return self.hist.shape[0]

    @property
    def starts(self):
        return self.hist.shape[3]

    def save(self, path):
        with open(path, "wb") as fh:
            np.savez(fh, hist=self.hist, counts=self.counts, thresholds=self.thresholds, k=np.int64(self.kernel_size),
                     length=np.int64(self.length), strands=np.str_(self.strands))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["hist"], z["counts"], z["thresholds"], int(z["k"]), int(z["length"]), str(z["strands"]))


def positions_device(bits, site, labels, thresholds, starts, hist=None):
    """explainn_site_positions on device tensors: bits int16 and site int32 (units, N) as _launch_record_best
    gives them, labels uint8 (N,), thresholds float32 (units, T), `starts` = M.  hist: int32 (units, T, 2, M)
    on the device, added into (None: zeros).  Thresholds whose [T][2][M] histogram would pass 64 KiB go over
    in groups.  Returns (hist, counts int64 (2,) of this call)."""
    from . import _lib
    (units, n), dev = _lib.require(bits, torch.int16, (None, None), None, "bits").shape, bits.device
    M = int(starts)
    _lib.require(site, torch.int32, (units, n), dev, "site")
    _lib.require(labels, torch.uint8, (n,), dev, "labels")
    if not torch.is_tensor(thresholds) or thresholds.dtype != torch.float32 or thresholds.dim() != 2 or \
            thresholds.shape[0] != units or thresholds.device != dev:
        raise RuntimeError("thresholds must be a float32 (%d, T) tensor on %s" % (units, dev))
    T = thresholds.shape[1]
    if M < 1 or 2 * M * 4 > HIST_BYTES:
        raise ValueError("records of %d starts: the histogram of one threshold must fit %d bytes" % (M, HIST_BYTES))
    if hist is None:
        hist = torch.zeros((units, T, 2, M), device=dev, dtype=torch.int32)
    else:
        _lib.require(hist, torch.int32, (units, T, 2, M), dev, "hist")
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    group = min(HIST_BYTES // (2 * M * 4), MAX_THRESHOLDS)
    for t0 in range(0, T, group):
        whole = t0 == 0 and T <= group
        thr = thresholds.contiguous() if whole else thresholds[:, t0:t0 + group].contiguous()
        part = hist if whole else torch.zeros((units, thr.shape[1], 2, M), device=dev, dtype=torch.int32)
        _lib.call("explainn_site_positions", dev, bits, site, labels, thr, units, n, thr.shape[1], M, part, counts)
        if not whole:
            hist[:, t0:t0 + group] += part
    return hist, counts


def test_device(hist, counts, local=False, min_width=1, max_width=None, min_sites=1):
    """explainn_centrality_test on device tensors: hist int32 (units, T, 2, M), counts int64 (2,).  Returns a
    dict of device tensors, each (units,): best_t, best_lo, best_width (int32), sites, count, n_tests, ctrl_sites,
    ctrl_count (int64), log_pvalue, log_padj, log_fisher (float64)."""
    from . import _lib
    lo, hi, need = check_widths(min_width, max_width, min_sites)
    (units, T, _, M), dev = _lib.require(hist, torch.int32, (None, None, 2, None), None, "hist").shape, hist.device
    _lib.require(counts, torch.int64, (2,), dev, "counts")
    if T > MAX_THRESHOLDS or T * 2 * M * 4 > HIST_BYTES:
        raise ValueError("%d thresholds of %d starts: one test takes at most %d thresholds and %d bytes of "
                         "[T][2][M] counts; test fewer thresholds at once" % (T, M, MAX_THRESHOLDS, HIST_BYTES))
    hi = max(M, lo) if hi is None else hi
    out = {f: torch.empty(units, device=dev, dtype=field_dtype(f, torch)) for f in _FIELDS}
    _lib.call("explainn_centrality_test", dev, hist, counts, units, T, M, 1 if local else 0, lo, hi, need,
              *(out[f] for f in _FIELDS))
    return out


test_device.__test__ = False      # not a pytest test, whoever imports it


class Centrality:
    """Per unit (numpy, (units,)): `best_t` the index and `threshold` the value of the chosen threshold;
    `best_lo`, `best_width` the chosen region of starts (width 0: nothing was tried) and `region_start`,
    `region_end`, `center` the same in record coordinates (region_coordinates); `sites` the primary best sites
    that pass the threshold, `count` those inside the region, `expected` = sites x width / M; `n_tests` the
    (threshold, region) pairs tried; `log_pvalue` ln of the one-sided binomial p, `log_padj`
    ln(1 - (1 - p)^n_tests), `evalue` = exp(log_padj) x units, `qvalue` Benjamini-Hochberg of the p-values over
    the units; `ctrl_sites`, `ctrl_count` the control set's sites at that threshold and inside the region,
    `log_fisher` ln of the one-sided Fisher p of count / Np against ctrl_count / Nc, `fisher_evalue` =
    exp(log_fisher) x units and `fisher_qvalue`.  `counts` = (Np, Nc); `thresholds` (units, T)."""

    def __init__(self, best_t, best_lo, best_width, sites, count, n_tests, log_pvalue, log_padj, ctrl_sites, ctrl_count,
                 log_fisher, counts, thresholds, kernel_size, length, local=False, strands="both"):
        for f, x in zip(_FIELDS, (best_t, best_lo, best_width, sites, count, n_tests, log_pvalue, log_padj,
                                  ctrl_sites, ctrl_count, log_fisher)):
            setattr(self, f, np.asarray(x, dtype=field_dtype(f)))
        self.counts = np.asarray(counts, dtype=np.int64)
        self.kernel_size, self.length, self.local, self.strands = int(kernel_size), int(length), bool(local), str(strands)
        units = len(self.best_t)
        if self.counts.shape != (2,) or any(getattr(self, f).shape != (units,) for f in _FIELDS):
            raise ValueError("every per-unit field must be (units,) and counts (2,)")
        self.thresholds = check_thresholds(thresholds, units) if units else np.zeros((0, 1), np.float32)
        if units and (self.best_t.min() < 0 or self.best_t.max() >= self.thresholds.shape[1]):
            raise ValueError("best_t must index the %d thresholds" % self.thresholds.shape[1])
        M = self.length - self.kernel_size + 1
        self.threshold = self.thresholds[np.arange(units), self.best_t]
        self.region_start, self.region_end, self.center = region_coordinates(self.best_lo, self.best_width,
                                                                              self.kernel_size, self.length)
        self.expected = self.sites * self.best_width.astype(np.float64) / float(M)
        self.evalue = np.exp(self.log_padj) * units
        self.qvalue = benjamini_hochberg(np.exp(self.log_pvalue)) if units else np.zeros(0)
        self.fisher_evalue = np.exp(self.log_fisher) * units
        self.fisher_qvalue = benjamini_hochberg(np.exp(self.log_fisher)) if units else np.zeros(0)

    @property
    def units(self):
        return len(self.best_t)

    def save(self, path):
        """.npz of the device outputs, the thresholds, the record counts and the geometry."""
        with open(path, "wb") as fh:
            np.savez(fh, counts=self.counts, thresholds=self.thresholds, k=np.int64(self.kernel_size),
                     length=np.int64(self.length), local=np.bool_(self.local), strands=np.str_(self.strands),
                     **{f: getattr(self, f) for f in _FIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(*(z[f] for f in _FIELDS), z["counts"], z["thresholds"], int(z["k"]), int(z["length"]),
                       bool(z["local"]), str(z["strands"]))


def centred_records(records, control, need):
    """The front of both centrality paths: (code arrays of the primary records followed by the control's,
    their labels -- uint8, numpy, records shorter than `need` left out --, the one length L of the others)."""
    _, prim = record_codes(records)
    _, ctrl = record_codes(control) if control is not None else ([], [])
    if not prim:
        raise ValueError("no primary record")
    L = common_length([len(c) for c in prim + ctrl], need)
    return prim + ctrl, record_labels([len(c) for c in prim], [len(c) for c in ctrl], need), L


def _device_positions(model, records, thresholds, control, strands, chunk_bases, out):
    """The device half of site_positions: (hist, counts) on the device, thresholds (units, T), k, L."""
    scorer = FilterScorer(model, _strands(strands))
    k, units = scorer.need, scorer.units
    codes, labels, L = centred_records(records, control, k)
    thr = check_thresholds(thresholds, units)
    M = L - k + 1
    if 2 * M * 4 > HIST_BYTES:
        raise ValueError("records of %d starts: the histogram of one threshold must fit %d bytes" % (M, HIST_BYTES))
    if out is not None and (not isinstance(out, SitePositions) or (out.units, out.kernel_size, out.length) != (units, k, L)
                            or not np.array_equal(out.thresholds, thr) or out.strands != strands):
        raise ValueError("out must be a SitePositions of this model, these thresholds, strands and record length")
    bits, site = best_over_records(scorer, codes, chunk_bases, True)
    scorer.finish()
    dev = bits.device
    hist = None if out is None else torch.from_numpy(out.hist).to(dev)
    hist, counts = positions_device(bits, site, torch.from_numpy(labels).to(dev), torch.from_numpy(thr).to(dev), M, hist)
    if out is not None:
        counts = counts + torch.from_numpy(out.counts).to(dev)
    return hist, counts, thr, k, L


def site_positions(model, records, thresholds, control=None, strands="both", chunk_bases=None, out=None):
    """Position histograms of the best sites of every filter of `model` (an ExplaiNN, or an ExplaiNNBank:
    global unit indices) in `records` and, as set 1, in `control` (lists as best_sites takes them).
    thresholds: (units,) or (units, T <= 16) floats, as call_sites takes them (null.thresholds(p),
    thresholds.tsv); a record counts at a threshold where call_sites would call its best site.  All records
    of at least k bases must have one length (ValueError otherwise: the test is for fixed-width summit
    windows); shorter ones are left out.  The best sites stay on the device; chunk_bases as in best_sites (the
    result does not depend on it).  out: a SitePositions of the same model, thresholds and length to add
    into (and return).  Eval mode only.  Returns a SitePositions."""
    hist, counts, thr, k, L = _device_positions(model, records, thresholds, control, strands, chunk_bases, out)
    if out is None:
        return SitePositions(hist.cpu().numpy(), counts.cpu().numpy(), thr, k, L, strands)
    out.hist, out.counts = hist.cpu().numpy(), counts.cpu().numpy()
    return out


def positions_from_best(best, thresholds, control_best=None, device="cuda"):
    """site_positions from saved best sites (RecordBest: best_sites(), `enrichment --save-best`) of the primary
    and, optionally, the control records, uploaded once."""
    if not isinstance(best, RecordBest) or (control_best is not None and not isinstance(control_best, RecordBest)):
        raise ValueError("best and control_best must be RecordBest objects")
    k, units = best.kernel_size, best.score.shape[0]
    if control_best is not None and (control_best.kernel_size, control_best.score.shape[0]) != (k, units):
        raise ValueError("the control's best sites are of %d units of kernel size %d, the primary's of %d of %d" % (
            control_best.score.shape[0], control_best.kernel_size, units, k))
    thr = check_thresholds(thresholds, units)
    ctrl_lengths = control_best.lengths if control_best is not None else np.zeros(0, np.int64)
    L = common_length(list(best.lengths) + list(ctrl_lengths), k)
    labels = record_labels(best.lengths, ctrl_lengths, k)
    parts = [best] if control_best is None else [best, control_best]
    bits = torch.from_numpy(np.concatenate([b.bits.view(np.int16) for b in parts], axis=1)).to(device)
    site = torch.from_numpy(np.concatenate([pack_site(b.start, b.strand) for b in parts], axis=1)).to(device)
    hist, counts = positions_device(bits, site, torch.from_numpy(labels).to(bits.device),
                                    torch.from_numpy(thr).to(bits.device), L - k + 1)
    return SitePositions(hist.cpu().numpy(), counts.cpu().numpy(), thr, k, L)


def _result(out, counts, thr, k, L, local, strands):
    return Centrality(*(out[f].cpu().numpy() for f in _FIELDS), counts.cpu().numpy(), thr, k, L, local, strands)


def test_positions(positions, local=False, min_width=1, max_width=None, min_sites=1, device="cuda"):
    """The centrality test of a SitePositions: centred regions [j, M-1-j], or with local=True every range of
    starts, of min_width <= width <= max_width bins (None: up to M - 1; the whole record is never a region);
    thresholds with fewer than max(min_sites, 1) primary sites are not tried.  Returns a Centrality."""
    check_widths(min_width, max_width, min_sites)
    if not isinstance(positions, SitePositions):
        raise ValueError("positions must be a SitePositions")
    hist = torch.from_numpy(positions.hist).to(device)
    counts = torch.from_numpy(positions.counts).to(device)
    out = test_device(hist, counts, local, min_width, max_width, min_sites)
    return _result(out, counts, positions.thresholds, positions.kernel_size, positions.length, local, positions.strands)


test_positions.__test__ = False   # not a pytest test, whoever imports it


def centrality(model, records, thresholds, control=None, local=False, min_width=1, max_width=None, min_sites=1,
               strands="both", chunk_bases=None):
    """site_positions and test_positions in one go, the histograms never leaving the device.  Returns a
    Centrality."""
    check_widths(min_width, max_width, min_sites)
    hist, counts, thr, k, L = _device_positions(model, records, thresholds, control, strands, chunk_bases, None)
    return _result(test_device(hist, counts, local, min_width, max_width, min_sites), counts, thr, k, L, local, strands)


def table_rows(result, max_evalue=None, control=None, lead=None, keep=None):
    """The rows of the CLI's table: (filter, threshold, sites, region_start, region_end, width, center, count,
    expected, log_pvalue, log_padj, evalue, qvalue) and, with control (None: when the result has control
    records), (ctrl_sites, ctrl_count, log_fisher), of the units -- of `keep`, if given -- with evalue <=
    max_evalue (None: all), by ascending log_pvalue, ties by filter.  lead: a function of the unit whose tuple
    stands in place of (filter,)."""
    control = bool(result.counts[1] > 0) if control is None else bool(control)
    lead = lead or (lambda u: (int(u),))
    rows = []
    for u in table_order(result, max_evalue, keep):
        row = lead(u) + (float(result.threshold[u]), int(result.sites[u]), int(result.region_start[u]),
               int(result.region_end[u]), int(result.best_width[u]), float(result.center[u]), int(result.count[u]),
               float(result.expected[u]), float(result.log_pvalue[u]), float(result.log_padj[u]),
               float(result.evalue[u]), float(result.qvalue[u]))
        if control:
            row += (int(result.ctrl_sites[u]), int(result.ctrl_count[u]), float(result.log_fisher[u]))
        rows.append(row)
    return rows


def write_table(fh, rows, control=None, columns=COLUMNS, lead="filter%d"):
    """The rows as TSV: `lead` formats what table_rows' lead gave, STAT_FORMAT the rest."""
    control = (bool(rows) and len(rows[0]) > len(columns)) if control is None else bool(control)
    fh.write("\t".join(columns + (CONTROL_COLUMNS if control else ())) + "\n")
    for row in rows:
        line = (lead + "\t" + STAT_FORMAT) % row[:len(columns)]
        if control:
            line += "\t%d\t%d\t%.6g" % row[len(columns):]
        fh.write(line + "\n")


def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.centrality", description=main.__doc__)
    ap.add_argument("model_file")
    ap.add_argument("peaks_fasta")
    ap.add_argument("-t", "--thresholds", required=True, action="append",
                    help="thresholds.tsv (filter, threshold); repeat for several thresholds per filter")
    ap.add_argument("-o", "--output-file", required=True)
    ap.add_argument("--control", help="control FASTA: adds the Fisher test of the chosen region")
    ap.add_argument("--local", action="store_true", help="every range of starts, not only the centred ones")
    ap.add_argument("--min-width", type=int, default=1)
    ap.add_argument("--max-width", type=int, default=None)
    ap.add_argument("--min-sites", type=int, default=1)
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--max-evalue", type=float, default=10.0)
    ap.add_argument("--save-positions", help="write the position histograms as .npz (SitePositions.load)")
    return ap


def main(argv=None):
    """MODEL, a FASTA of summit-centred windows of one length and one or more thresholds.tsv -> a table of
    filters by central enrichment of their best sites: Filter, Threshold, Sites, RegionStart, RegionEnd (record
    coordinates, half open), Width (starts), Center (offset of the region from the record centre), Count,
    Expected, LogPvalue, LogPadj, Evalue, Qvalue and, with --control, CtrlSites, CtrlCount, LogFisher; one row
    per filter with Evalue <= --max-evalue, by ascending p-value."""
    args = _parser().parse_args(argv)
    from .loader import read_fasta_records
    from .predict import _load_model
    from .sites import read_thresholds
    check_widths(args.min_width, args.max_width, args.min_sites)
    peaks = read_fasta_records(args.peaks_fasta)
    control = read_fasta_records(args.control) if args.control else None
    model = _load_model(args.model_file)
    model.eval()
    thr = np.stack([read_thresholds(path, model._units()) for path in args.thresholds], axis=1)
    positions = site_positions(model, peaks, thr, control, args.strands)
    if args.save_positions:
        positions.save(args.save_positions)
    result = test_positions(positions, args.local, args.min_width, args.max_width, args.min_sites, model._device())
    with open(args.output_file, "w") as fh:
        write_table(fh, table_rows(result, args.max_evalue, control is not None), control is not None)


if __name__ == "__main__":
    main()
