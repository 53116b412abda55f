"""Which motifs occur together, and at what distance?  Spaced motif analysis of the site lists.

ExplaiNN's units are independent and its head is linear, so the model cannot represent cooperativity
between motifs; users look for it after the fact, in the sites (sites.call_sites).  This is the analysis
of SpaMo (Whitington et al. 2011): for every pair of filters the histogram of the distances between
their sites, by relative orientation, and a binomial test for a preferred spacing -- counted on the
device (explainn_site_spacing / explainn_spacing_test, csrc/spacing.hip) from the lists as they are.

    calls = call_sites(model, codes, null.thresholds(1e-4))
    counts = spacing(calls, max_distance=100)            # hist (U, U, 2, 201) int64 on the device
    res = counts.test(n_positions=len(codes))            # total, best_distance, best_count, pvalue, qvalue, ...

For an ordered pair of distinct site records i, j of units a, b: d = (start_j - start_i) * strand_i is
where the partner lies in the anchor's own orientation, o = 0 for the same strand and 1 for opposite
strands, and |d| <= D adds 1 to hist[a][b][o][d + D].  Only i == j is left out (by record, not by
position).  hist[a][b][0][D+d] == hist[b][a][0][D-d] and hist[a][b][1][D+d] == hist[b][a][1][D+d].

`python -m explainn_amd.spacing MODEL FASTA -t thresholds.tsv -o OUT.tsv` calls the sites of every
record and writes the significant spacings.
"""
import argparse

import numpy as np
import torch

MAX_DISTANCE = 1024          # EXPLAINN_SPACING_MAX_DISTANCE
MAX_BYTES = 2 << 30          # the largest histogram spacing() allocates unless told otherwise
COLUMNS = ("FilterA", "FilterB", "Orientation", "Distance", "Count", "Total", "Expected", "Ratio", "Pvalue",
           "Qvalue")


def _check_distance(max_distance):
    if int(max_distance) != max_distance or not 0 <= int(max_distance) <= MAX_DISTANCE:
        raise ValueError("max_distance must be an integer in [0, %d] (got %r)" % (MAX_DISTANCE, max_distance))
    return int(max_distance)


def _unit_set(units, total, what):
    """None (all units) or a 1-D int32 array of unit indices inside [0, total)."""
    if units is None:
        return None
    u = np.asarray(units.cpu() if torch.is_tensor(units) else units)
    if u.ndim != 1 or (u.size and not np.issubdtype(u.dtype, np.integer)):
        raise ValueError("%s must be a 1-D list of unit indices" % what)
    u = u.astype(np.int64)
    if u.size and (u.min() < 0 or u.max() >= total):
        raise IndexError("%s holds a unit outside [0, %d)" % (what, total))
    return u.astype(np.int32)


def site_lists(calls, max_distance, period=0):
    """The host half of spacing(): (start, offsets2, kernel_size) of a SiteCalls, or of a list of
    (SiteCalls, record_length) pairs, as explainn_site_spacing takes them.

    start: int64 coordinates in which no two sites of different records are within max_distance of each
    other.  period = L > 0: the calls are of a concatenation of records of L bases (call_sites(period=L))
    and a start p becomes p + (p // L) (max_distance + 1).  A list: record r's coordinates are shifted by
    the lengths of the records before it plus max_distance + 1 each, and unit u's '+' sites of all the
    records, then its '-' sites, are put together.  offsets2: int64 (2 units + 1): the list of (unit u,
    '+') is [offsets2[2u], offsets2[2u+1]), of (u, '-') [offsets2[2u+1], offsets2[2u+2]).  ValueError
    unless, per unit, the '+' sites come first and each strand's starts ascend."""
    D = _check_distance(max_distance)
    if int(period) < 0:
        raise ValueError("period must not be negative")
    if isinstance(calls, (list, tuple)):
        if not calls:
            raise ValueError("an empty list of records")
        if period:
            raise ValueError("period is for one SiteCalls of concatenated records; a list carries its lengths")
        first = calls[0][0]
        keys, starts, base = [], [], 0
        for c, length in calls:
            if (c.units, c.kernel_size) != (first.units, first.kernel_size):
                raise ValueError("the records' calls are of different models")
            if len(c) and (c.start.min() < 0 or c.start.max() >= int(length)):
                raise ValueError("a site starts outside its record of %d bases" % int(length))
            keys.append(_keys(c))
            starts.append(c.start + base)
            base += int(length) + D + 1
        key, start = np.concatenate(keys), np.concatenate(starts)
        for k in keys:                                   # each record must be in order before the merge hides it
            if np.any(np.diff(k) < 0):
                raise ValueError("per unit the '+' sites must come before the '-' sites")
        order = np.argsort(key, kind="stable")           # records stay in order inside a (unit, strand) list
        key, start = key[order], start[order]
        units, k = first.units, first.kernel_size
    else:
        key, start = _keys(calls), calls.start
        if period:
            start = start + (start // int(period)) * (D + 1)
        units, k = calls.units, calls.kernel_size
    step = np.diff(key)
    if np.any(step < 0):
        raise ValueError("per unit the '+' sites must come before the '-' sites")
    if np.any((step == 0) & (np.diff(start) < 0)):
        bad = int(np.flatnonzero((step == 0) & (np.diff(start) < 0))[0])
        raise ValueError("the sites of filter%d, strand %s, are not in ascending start (record %d)" % (
            key[bad] // 2, "-" if key[bad] & 1 else "+", bad + 1))
    offsets2 = np.zeros(2 * units + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=2 * units), out=offsets2[1:])
    return np.ascontiguousarray(start, dtype=np.int64), offsets2, k


def _keys(calls):
    """2 unit + (strand is '-') of every record."""
    if len(calls) and not np.all(np.abs(calls.strand) == 1):
        raise ValueError("strand must be +1 or -1")
    return 2 * calls.unit_ids() + (calls.strand < 0)


class SpacingTest:
    """What SpacingCounts.test() returns: device tensors (A, P, 2), orientation 0 = same strand, 1 = opposite.
    total (int64): pairs in the admissible bins; best_distance (int32), best_count (int64): the fullest
    bin; pvalue, qvalue (float64); tested (bool): the entries that are hypotheses; expected, ratio
    (float64) when n_positions was given, else None; bins (int64): the admissible bins m."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


class SpacingCounts:
    """Distance histograms of site pairs: `hist` int64 (A, P, 2, 2 D + 1) on the device, hist[a][b][o][d + D]
    = ordered pairs of distinct sites (i of unit anchors[a], j of unit partners[b]) with
    (start_j - start_i) * strand_i == d, o = 0 on the same strand and 1 on opposite strands.  `anchors`,
    `partners`: int32 arrays of unit indices; `site_counts` int64 (units, 2): sites per unit on '+' and '-'."""

    def __init__(self, hist, anchors, partners, max_distance, kernel_size, site_counts):
        self.max_distance = _check_distance(max_distance)
        self.kernel_size = int(kernel_size)
        self.site_counts = np.asarray(site_counts, dtype=np.int64)
        if self.site_counts.ndim != 2 or self.site_counts.shape[1] != 2:
            raise ValueError("site_counts must be (units, 2)")
        self.anchors = _unit_set(anchors, self.units, "anchors")
        self.partners = _unit_set(partners, self.units, "partners")
        if self.anchors is None:
            self.anchors = np.arange(self.units, dtype=np.int32)
        if self.partners is None:
            self.partners = np.arange(self.units, dtype=np.int32)
        shape = (len(self.anchors), len(self.partners), 2, 2 * self.max_distance + 1)
        if not torch.is_tensor(hist) or hist.dtype != torch.int64 or tuple(hist.shape) != shape:
            raise ValueError("hist must be an int64 tensor of shape %s" % (shape,))
        self.hist = hist.contiguous()

    @property
    def units(self):
        return self.site_counts.shape[0]

    def _device_sets(self):
        from . import _lib
        dev = _lib.device_for(self.hist.device, (), "the spacing test")
        return torch.from_numpy(self.anchors).to(dev), torch.from_numpy(self.partners).to(dev)

    def test(self, min_distance=None, min_count=10, n_positions=None):
        """SpaMo's test of a preferred spacing for every (anchor, partner, orientation): a SpacingTest.

        The admissible bins are min_distance <= |d| <= max_distance (min_distance defaults to the kernel
        size, so that overlapping k-mers are not tested).  Same filter, same strand: every unordered pair
        is counted once at +d and once at -d, and only the bins d > 0 are taken; same filter, opposite
        strands: every unordered pair is counted twice in one bin, and the counts are halved.  With m bins,
        n pairs in them and c in the fullest, pvalue = min(1, m P[Binomial(n, 1/m) >= c]); entries with
        n < max(min_count, 1) or m == 0 are not tested (pvalue 1, best_count 0).  qvalue: Benjamini-Hochberg
        over the tested entries, 1 elsewhere.  n_positions (start positions the sites were called on, per
        strand): also `expected`, the pairs that independent placement would put into the admissible bins,
        m sum_s n_{a,s} n_{b,+-s} / n_positions (halved for the same filter on opposite strands), and
        `ratio` = total / expected.  The test is one launch on the current stream; selecting the tested
        entries for the q-values reads their number back."""
        from . import _lib
        from .motifs import benjamini_hochberg
        D = self.max_distance
        md = self.kernel_size if min_distance is None else int(min_distance)
        if md < 0 or int(min_count) < 0:
            raise ValueError("min_distance and min_count must not be negative")
        A, P = len(self.anchors), len(self.partners)
        dev = self.hist.device
        anchors, partners = self._device_sets()
        total = torch.zeros((A, P, 2), dtype=torch.int64, device=dev)
        best_distance = torch.zeros((A, P, 2), dtype=torch.int32, device=dev)
        best_count = torch.zeros((A, P, 2), dtype=torch.int64, device=dev)
        pvalue = torch.ones((A, P, 2), dtype=torch.float64, device=dev)
        _lib.call("explainn_spacing_test", dev, self.hist, A, P, anchors, partners, D, md, int(min_count), total,
                  best_distance, best_count, pvalue)
        # the admissible bins of every entry: plain arithmetic on D and min_distance
        side = max(D - max(md, 1) + 1, 0)                          # bins with d > 0
        same = (anchors[:, None] == partners[None, :])
        bins = torch.full((A, P, 2), 2 * side + (1 if md == 0 else 0), dtype=torch.int64, device=dev)
        bins[..., 0] = torch.where(same, side, bins[..., 0])
        tested = (bins > 0) & (total >= max(int(min_count), 1))
        qvalue = torch.ones_like(pvalue)
        qvalue[tested] = benjamini_hochberg(pvalue[tested][None, :])[0]
        expected = ratio = None
        if n_positions is not None:
            if not float(n_positions) > 0:
                raise ValueError("n_positions must be positive")
            n = torch.from_numpy(self.site_counts).to(dev).to(torch.float64)
            na, nb = n[anchors.long()], n[partners.long()]                      # (A, 2), (P, 2)
            pairs = torch.stack((na[:, None, 0] * nb[None, :, 0] + na[:, None, 1] * nb[None, :, 1],
                                 na[:, None, 0] * nb[None, :, 1] + na[:, None, 1] * nb[None, :, 0]), dim=2)
            pairs[..., 1] = torch.where(same, pairs[..., 1] / 2, pairs[..., 1])
            expected = bins.to(torch.float64) * pairs / float(n_positions)
            ratio = total.to(torch.float64) / expected
        return SpacingTest(total=total, best_distance=best_distance, best_count=best_count, pvalue=pvalue,
                           qvalue=qvalue, tested=tested, bins=bins, expected=expected, ratio=ratio)

    def save(self, path):
        """.npz of the non-zero (anchor, partner, orientation, bin, count) entries, the unit sets and the site counts."""
        nz = self.hist.nonzero()
        with open(path, "wb") as fh:
            np.savez(fh, index=nz.cpu().numpy().astype(np.int32),
                     count=self.hist[nz[:, 0], nz[:, 1], nz[:, 2], nz[:, 3]].cpu().numpy(),
                     anchors=self.anchors, partners=self.partners, max_distance=np.int64(self.max_distance),
                     k=np.int64(self.kernel_size), site_counts=self.site_counts)

    @classmethod
    def load(cls, path, device="cuda"):
        if torch.device(device).type == "cuda" and not torch.cuda.is_available():
            raise RuntimeError("SpacingCounts.load(device=%r): no HIP device is available; pass device='cpu' to "
                               "read the counts (the test itself has no CPU fallback)" % (device,))
        with np.load(path) as z:
            D = int(z["max_distance"])
            hist = np.zeros((len(z["anchors"]), len(z["partners"]), 2, 2 * D + 1), dtype=np.int64)
            i = z["index"].astype(np.int64)
            hist[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = z["count"]
            return cls(torch.from_numpy(hist).to(device), z["anchors"], z["partners"], D, int(z["k"]),
                       z["site_counts"])


def spacing(calls, max_distance=100, period=0, anchors=None, partners=None, out=None, device=None,
            max_bytes=MAX_BYTES):
    """Distance histograms of every (anchor filter, partner filter) pair of `calls`: a SpacingCounts.

    calls: a SiteCalls (sites.call_sites; on a bank, global unit indices), with period = L when it is of a
    concatenation of records of L bases, or a list of (SiteCalls, record_length) pairs, one per record, of
    equal lengths or not: no pair is counted across two records.  max_distance: D, at most 1024.
    anchors, partners: unit indices (any order, overlapping or not; default all units) -- the histogram
    takes A P 2 (2D+1) 8 bytes, and more than max_bytes of it raise ValueError.  out: a SpacingCounts of the
    same D and unit sets to add into (several chromosomes; its site counts grow too) -- returned.
    The sites must be ascending per (unit, strand), '+' first (ValueError otherwise).  The starts and the
    list offsets go to the device once; the counting is one launch on the current stream and nothing is
    read back."""
    from . import _lib
    D = _check_distance(max_distance)
    start, offsets2, k = site_lists(calls, D, period)
    units = (len(offsets2) - 1) // 2
    an, pa = _unit_set(anchors, units, "anchors"), _unit_set(partners, units, "partners")
    A, P = (units if an is None else len(an)), (units if pa is None else len(pa))
    counts = np.diff(offsets2).reshape(units, 2)
    if out is not None:
        if out.max_distance != D or out.units != units or out.kernel_size != k or \
                not np.array_equal(out.anchors, np.arange(units) if an is None else an) or \
                not np.array_equal(out.partners, np.arange(units) if pa is None else pa):
            raise ValueError("out= was counted with another max_distance, model or unit sets")
        if device is not None and torch.device(device) != out.hist.device:
            raise ValueError("out= lives on %s, not on %s" % (out.hist.device, device))
    else:
        nbytes = A * P * 2 * (2 * D + 1) * 8
        if nbytes > int(max_bytes):
            raise ValueError(
                "the histogram of %d x %d filter pairs at max_distance %d takes %d bytes, more than max_bytes = %d: "
                "pass anchors= / partners= (subsets of the units) or a smaller max_distance" % (
                    A, P, D, nbytes, int(max_bytes)))
    dev = _lib.device_for(device if out is None else out.hist.device, (), "spacing")
    if out is None:
        out = SpacingCounts(torch.zeros((A, P, 2, 2 * D + 1), dtype=torch.int64, device=dev), an, pa, D, k,
                            np.zeros_like(counts))
    if len(start) and A and P:
        pos, off = torch.from_numpy(start).to(dev), torch.from_numpy(offsets2).to(dev)
        an_d = None if an is None else torch.from_numpy(an).to(dev)
        pa_d = None if pa is None else torch.from_numpy(pa).to(dev)
        _lib.call("explainn_site_spacing", dev, pos, off, units, an_d, A, pa_d, P, D, out.hist)
    out.site_counts = out.site_counts + counts
    return out


def table_rows(counts, result, max_qvalue=0.05):
    """The rows of the CLI's table: (a, b, o, distance, count, total, expected, ratio, pvalue, qvalue) of the
    tested entries with unit a <= unit b and qvalue <= max_qvalue, by ascending p-value (ties: a, b, o)."""
    keep = (result.tested & (result.qvalue <= max_qvalue)).cpu().numpy()
    a_unit, b_unit = counts.anchors.astype(np.int64), counts.partners.astype(np.int64)
    keep &= (a_unit[:, None] <= b_unit[None, :])[:, :, None]
    ai, bi, o = np.nonzero(keep)
    host = lambda t: t.cpu().numpy()[ai, bi, o]
    p = host(result.pvalue)
    nan = np.full(len(p), np.nan)
    cols = (a_unit[ai], b_unit[bi], o, host(result.best_distance), host(result.best_count), host(result.total),
            host(result.expected) if result.expected is not None else nan,
            host(result.ratio) if result.ratio is not None else nan, p, host(result.qvalue))
    order = np.lexsort((o, b_unit[bi], a_unit[ai], p))
    return [tuple(c[i].item() for c in cols) for i in order]


def write_table(fh, rows):
    fh.write("\t".join(COLUMNS) + "\n")
    for a, b, o, d, c, n, e, r, p, q in rows:
        fh.write("filter%d\tfilter%d\t%s\t%d\t%d\t%d\t%.6g\t%.6g\t%.6g\t%.6g\n" % (
            a, b, "opposite" if o else "same", d, c, n, e, r, p, q))


def spacing_records(model, records, thresholds, max_distance=100, strands="both", anchors=None, partners=None):
    """spacing() over the sites of (id, codes) records (loader.read_fasta_records), called record by record:
    (SpacingCounts, start positions per strand).  `model`: an ExplaiNN or an ExplaiNNBank (global units)."""
    from .sites import call_sites_records
    k = model._options["kernel_size"]
    per_record, n_positions = [], 0
    for (_, codes), (_, calls) in zip(records, call_sites_records(model, records, thresholds, strands=strands)):
        if len(codes) >= k:
            per_record.append((calls, len(codes)))
            n_positions += len(codes) - k + 1
    if not per_record:
        raise ValueError("no record is as long as the kernel (%d bases)" % k)
    return spacing(per_record, max_distance, anchors=anchors, partners=partners, device=model._device()), n_positions


def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.spacing", description=main.__doc__)
    ap.add_argument("model_file")
    ap.add_argument("fasta_file")
    ap.add_argument("-t", "--thresholds", required=True, help="thresholds.tsv (filter, threshold)")
    ap.add_argument("-o", "--output-file", required=True)
    ap.add_argument("-d", "--max-distance", type=int, default=100)
    ap.add_argument("--min-distance", type=int, default=None, help="default: the kernel size")
    ap.add_argument("--min-count", type=int, default=10)
    ap.add_argument("--max-qvalue", type=float, default=0.05)
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--save-counts", help="write the histograms as .npz (SpacingCounts.load)")
    return ap


def main(argv=None):
    """MODEL, a FASTA and thresholds.tsv -> a table of filter pairs with a preferred spacing: FilterA,
    FilterB, Orientation (same / opposite strand), Distance (of the fullest bin, in FilterA's orientation),
    Count, Total, Expected, Ratio, Pvalue, Qvalue; one row per pair a <= b and orientation with
    Qvalue <= --max-qvalue, by ascending p-value."""
    args = _parser().parse_args(argv)
    from .loader import read_fasta_records
    from .predict import _load_model
    from .sites import read_thresholds
    records = read_fasta_records(args.fasta_file)
    model = _load_model(args.model_file)
    model.eval()
    thresholds = read_thresholds(args.thresholds, model._units())
    counts, n_positions = spacing_records(model, records, thresholds, args.max_distance, args.strands)
    result = counts.test(args.min_distance, args.min_count, n_positions)
    if args.save_counts:
        counts.save(args.save_counts)
    with open(args.output_file, "w") as fh:
        write_table(fh, table_rows(counts, result, args.max_qvalue))


if __name__ == "__main__":
    main()
