"""Which known motifs are enriched in my peaks, and do their sites sit at the summit?  Enrichment and
centrality for PWMs -- what SEA / AME and CentriMo of the MEME suite answer -- on the device.

`enrichment` and `centrality` ask these questions of a model's own filters; this module asks them of motifs
that come from a database (JASPAR, a MEME file, `motifs.write_meme` output), so that a filter's enrichment can
be set beside that of the motif `motifs.annotate` matched it to.  One device pass is new
(explainn_pwm_record_best, csrc/pwmbest.hip), wrapped as a MotifScorer; the host path from records to the
best-site matrix is explainn_amd.records, shared with the filters, and the two tests are the existing ones.

    best = best_motif_sites(read_motifs("JASPAR.meme"), peaks)        # per record the best site of every motif
    res = motif_enrichment(motifs, peaks, control)                    # or control=None: dinucleotide shuffles
    res.log_pvalue, res.threshold, res.threshold_pvalue, res.tp, res.fp, res.qvalue, res.auroc
    cen = motif_centrality(motifs, peaks, pvalues=(1e-4, 1e-3))
    cen.log_pvalue, cen.region_start, cen.region_end, cen.center, cen.count, cen.sites, cen.qvalue

A motif's log-odds are quantised to integers 0..bins per cell (`pwmsites.quantise`), so a site's score is an
integer <= 8192: a 15-bit pattern that sorts like the score, which is what explainn_enrichment_test takes.
best_motif_sites: for every motif and record the largest integer score over the record's live starts (the w
bases inside the record, no N among them) and both strands, and where it sits: the lowest start among equal
maxima, '+' before '-' at one start.

The integer-to-float16 bridge.  explainn_site_positions compares the float16 VALUE of a pattern with a float
threshold, and integer patterns below 0x400 are float16 subnormals; realistic cutoffs lie there.  So
motif_centrality hands it `iscore + 0x400` as the pattern (all normal halves) and, for the integer threshold t,
the float32 value of the half with bits 0x400 + t - 1: `value > threshold` is then exactly `iscore >= t` for
every 0 <= t <= 8193.  explainn_enrichment_test takes the raw integers.

`python -m explainn_amd.pwmenrich enrichment MOTIFS PRIMARY.fa [--control C.fa | --shuffles R --seed S] -o OUT.tsv`
`python -m explainn_amd.pwmenrich centrality MOTIFS PEAKS.fa [--pvalue P ...] [--control C.fa] [--local] -o OUT.tsv`
There is no CPU path.
"""
import argparse
import contextlib

import numpy as np
import torch

from . import _lib
from . import centrality as _cen
from . import enrichment as _enr
from . import pwmsites as _pwm
from .enrichment import Enrichment, benjamini_hochberg
from .records import (LABEL_EXCLUDED, BestSites, RecordBest, best_over_records, enrichment_bits, record_codes,
                      record_labels, unpack_site)

BRIDGE = 0x400               # added to an integer score: the pattern of the smallest normal float16
ENRICHMENT_COLUMNS = ("Motif", "Name", "Threshold", "ThresholdPvalue") + _enr.COLUMNS[2:]
CENTRALITY_COLUMNS = ("Motif", "Name") + _cen.COLUMNS[1:]
_EFIELDS, _CFIELDS = _enr._FIELDS, _cen._FIELDS


# ---------------------------------------------------------------- the bridge (host)
def bridge_thresholds(iscore_thresholds):
    """float32 thresholds for explainn_site_positions from integer ones in [0, 8193]: the value of the float16
    with bits 0x400 + t - 1, so that value(iscore + 0x400) > it  <=>  iscore >= t."""
    t = np.asarray(iscore_thresholds, dtype=np.int64)
    if t.size and (t.min() < 0 or t.max() > 8193):
        raise ValueError("an integer score threshold lies outside [0, 8193]")
    return (t + (BRIDGE - 1)).astype(np.uint16).view(np.float16).astype(np.float32)


# ---------------------------------------------------------------- tables
class _Tables:
    """The quantised motifs: names, display names, S int16 (M,wmax,4), widths as given, live widths (0 for an
    empty motif), scale, lo, bins and the background."""

    def __init__(self, motifs, bg, pseudocount, bins):
        self.ids, mats = _pwm.motif_list(motifs)
        named = isinstance(motifs, (list, tuple)) and all(isinstance(m, tuple) and len(m) == 3 for m in motifs)
        self.names = [str(m[1]) for m in motifs] if named else list(self.ids)
        self.bg = _pwm._background(bg)
        self.S, self.widths, self.scale, self.lo = _pwm.quantise(mats, self.bg, pseudocount, bins)
        self.live = np.where(self.scale > 0, self.widths, 0).astype(np.int32)
        self.bins = int(bins)

    @property
    def M(self):
        return len(self.ids)

    @property
    def widest(self):
        """The width of the widest live motif (0: none is live)."""
        return int(self.live.max()) if self.M else 0

    def log_odds(self, iscore):
        """Real log-odds of per-motif integer scores (M,) or (M, ...): iscore / scale + w lo; NaN for an empty
        motif."""
        x = np.asarray(iscore, dtype=np.float64)
        shape = (-1,) + (1,) * (x.ndim - 1)
        ok = (self.scale > 0).reshape(shape)
        return np.where(ok, x / np.where(ok, self.scale.reshape(shape), 1.0) + (self.widths * self.lo).reshape(shape), np.nan)


def record_best_device(scores, widths, seq, offsets, both=True, want_site=True, flags=None):
    """explainn_pwm_record_best on device tensors: scores int16 (M,wmax,4), widths int32 (M,), seq uint8 (n,),
    offsets int64 (R+1,).  Returns (bits int16 (M,R), site int32 (M,R) or None) on the device; `flags`: an int32
    (1,) device tensor that bit 0 is ORed into for forged offsets.  Enqueued on the current stream."""
    dev = _lib.require(seq, torch.uint8, (None,), None, "seq").device
    _lib.require(scores, torch.int16, (None, None, None), dev, "scores")
    _lib.require(widths, torch.int32, (None,), dev, "widths")
    _lib.require(offsets, torch.int64, (None,), dev, "offsets")
    M, wmax = scores.shape[0], scores.shape[1]
    if scores.shape[2] != 4 or widths.shape[0] != M or offsets.shape[0] < 1:
        raise ValueError("scores must be (M,wmax,4), widths (M,) and offsets (R+1,)")
    R = offsets.shape[0] - 1
    bits = torch.empty((M, R), dtype=torch.int16, device=dev)
    site = torch.empty((M, R), dtype=torch.int32, device=dev) if want_site else None
    _lib.call("explainn_pwm_record_best", dev, seq, seq.shape[0], offsets, R, int(bool(both)), scores, widths, M,
              max(wmax, 1), bits, site, flags)
    return bits, site


class MotifScorer:
    """The motifs of a _Tables, uploaded to `device` once, on one or both strands: explainn_pwm_record_best."""

    def __init__(self, tab, both, device):
        self.both, self.device, self.units, self.need = both, device, tab.M, tab.widest
        self.scores = torch.from_numpy(tab.S).to(device).contiguous()
        self.widths = torch.from_numpy(tab.live).to(device)

    def best(self, seq, offsets, want_site):
        return record_best_device(self.scores, self.widths, seq, offsets, self.both, want_site)

    span = staticmethod(contextlib.nullcontext)

    def finish(self):
        pass


# ---------------------------------------------------------------- best sites
class MotifBest(BestSites):
    """The best site of every motif in every record: `iscore` int16 (M, N), the largest integer score over the
    record's live starts (0 without one); `start` int32 (M, N), the 0-based forward start of the w-mer that holds
    it (-1 without one) -- the lowest among equal maxima; `strand` int8 (M, N), +1 / -1 ('+' wins a tie at one
    start; 0 without a site); `lengths` int64 (N,); `widths` int32 (M,) as given, `names`; `scale`, `lo` float64
    (M,) of pwmsites.quantise (scale 0: an EMPTY motif, which has no site anywhere).  `score`: the real log-odds
    iscore / scale + w lo, float64 (M, N), NaN without a site."""

    def __init__(self, iscore, start, strand, lengths, widths, names, scale, lo, ids=None):
        self.iscore = np.asarray(iscore, dtype=np.int16)
        self.widths = np.asarray(widths, dtype=np.int32)
        self.names = [str(n) for n in names]
        self.scale, self.lo = np.asarray(scale, dtype=np.float64), np.asarray(lo, dtype=np.float64)
        M = len(self.names)
        self._set_sites(self.iscore, start, strand, lengths, ids, ("iscore", "M"), M)
        if self.widths.shape != (M,) or self.scale.shape != (M,) or self.lo.shape != (M,):
            raise ValueError("widths, scale and lo must hold one entry per motif")

    @property
    def units(self):
        return len(self.names)

    @property
    def bits(self):
        """uint16 (M, N): the integer scores as the patterns explainn_enrichment_test takes."""
        return self.iscore.view(np.uint16)

    @property
    def live_widths(self):
        return np.where(self.scale > 0, self.widths, 0).astype(np.int32)

    @property
    def score(self):
        ok = (self.scale > 0)[:, None] & (self.start >= 0)
        s = self.iscore / np.where(self.scale > 0, self.scale, 1.0)[:, None] + (self.widths * self.lo)[:, None]
        return np.where(ok, s, np.nan)

    @classmethod
    def from_device(cls, bits, site, lengths, widths, names, scale, lo, ids=None):
        return cls(bits, *unpack_site(site), lengths, widths, names, scale, lo, ids)

    def save(self, path):
        with open(path, "wb") as fh:
            np.savez(fh, iscore=self.iscore, start=self.start, strand=self.strand, lengths=self.lengths,
                     widths=self.widths, names=np.array(self.names, dtype=np.str_), scale=self.scale, lo=self.lo,
                     ids=self._ids_array())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["iscore"], z["start"], z["strand"], z["lengths"], z["widths"], [str(n) for n in z["names"]],
                       z["scale"], z["lo"], cls._ids_of(z))


def best_motif_sites(motifs, records, bg=None, pseudocount=0.1, bins=100, strands="both", chunk_bases=None,
                     device=None):
    """The best site of every motif in every record.  motifs: [(id, name, (w,4) matrix)] as read_motifs gives
    them, or anything pwmsites.scan_motifs accepts; records: a list of (id, codes) pairs
    (loader.read_fasta_records) or of 1-D uint8 code arrays (numpy or tensors, host or device), of any lengths.
    bg: None = uniform, or four frequencies.  The records go to the device concatenated, in chunks of at most
    chunk_bases bases (default 2^26) cut at record boundaries; the result does not depend on the chunking.
    Returns a MotifBest."""
    both = _enr._strands(strands) == 2
    tab = _Tables(motifs, bg, pseudocount, bins)
    ids, codes = record_codes(records)
    scorer = MotifScorer(tab, both, _lib.device_for(device, (), "pwmsites.best_motif_sites"))
    bits, site = best_over_records(scorer, codes, chunk_bases, True)
    return MotifBest.from_device(bits.cpu().numpy(), site.cpu().numpy(), [len(c) for c in codes], tab.widths, tab.ids,
                                 tab.scale, tab.lo, ids)


# ---------------------------------------------------------------- enrichment
class MotifEnrichment(Enrichment):
    """Enrichment's fields per motif, with `iscore_threshold` (= best_pattern) the integer score of the most
    significant threshold, `threshold` its real log-odds (NaN for an empty motif), `threshold_pvalue` the
    per-site p-value at that cutoff (tail[m][best_pattern] of explainn_pwm_null's table), `ids`, `names`,
    `widths`, and `excluded`: the records left out of the test for ALL motifs because they are shorter than
    the widest live motif (kernel_size holds that width).  evalue and qvalue are over all M motifs."""

    def __init__(self, fields, counts, threshold, threshold_pvalue, ids, names, widths, excluded=0, kernel_size=0,
                 strands="both", shuffles=0, seed=0):
        super().__init__(*fields, counts, kernel_size, strands, shuffles, seed)
        self.iscore_threshold = self.best_pattern
        self.threshold = np.asarray(threshold, dtype=np.float64)
        self.threshold_pvalue = np.asarray(threshold_pvalue, dtype=np.float64)
        self.ids, self.names = [str(i) for i in ids], [str(n) for n in names]
        self.widths, self.excluded = np.asarray(widths, dtype=np.int32), int(excluded)
        if self.threshold.shape != (self.units,) or self.threshold_pvalue.shape != (self.units,) or \
                len(self.ids) != self.units or len(self.names) != self.units or self.widths.shape != (self.units,):
            raise ValueError("threshold, threshold_pvalue, ids, names and widths must hold one entry per motif")

    def save(self, path):
        """.npz of the device outputs, the record counts, the motifs' names and how the control was drawn."""
        with open(path, "wb") as fh:
            np.savez(fh, counts=self.counts, k=np.int64(self.kernel_size), strands=np.str_(self.strands),
                     shuffles=np.int64(self.shuffles), seed=np.int64(self.seed), threshold=self.threshold,
                     threshold_pvalue=self.threshold_pvalue, ids=np.array(self.ids, dtype=np.str_),
                     names=np.array(self.names, dtype=np.str_), widths=self.widths, excluded=np.int64(self.excluded),
                     **{f: getattr(self, f) for f in _EFIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls([z[f] for f in _EFIELDS], z["counts"], z["threshold"], z["threshold_pvalue"],
                       [str(i) for i in z["ids"]], [str(n) for n in z["names"]], z["widths"], int(z["excluded"]),
                       int(z["k"]), str(z["strands"]), int(z["shuffles"]), int(z["seed"]))


def motif_enrichment(motifs, primary, control=None, shuffles=1, seed=0, bg=None, pseudocount=0.1, bins=100,
                     strands="both", chunk_bases=None, device=None):
    """Enrichment of every motif in the `primary` records against the `control` records (lists as
    best_motif_sites takes them).  control=None: the control set is `shuffles` dinucleotide-preserving shuffles
    of every primary record, drawn on the device (sequence.dinucleotide_shuffle_device with `seed`); this needs
    primary records of one length (ValueError otherwise).  A record's score for a motif is its best integer
    site score; one explainn_enrichment_test call takes the primary and control matrices side by side.
    Records shorter than the widest live motif are left out of the test for ALL motifs (one label vector serves
    the call; `excluded` counts them).  Returns a MotifEnrichment."""
    both = _enr._strands(strands) == 2
    tab = _Tables(motifs, bg, pseudocount, bins)
    scorer = MotifScorer(tab, both, _lib.device_for(device, (), "pwmsites.motif_enrichment"))
    bits, labels, shuffles = enrichment_bits(scorer, primary, control, shuffles, seed, chunk_bases)
    out = _enr.enrichment_test(bits, torch.from_numpy(labels).to(scorer.device))
    if tab.M:
        null = _pwm._null(tab.S, tab.live, tab.scale, tab.lo, tab.bins, tab.bg, 1.0, scorer.device)
        at = out["best_pattern"].to(torch.int64).clamp_(0, null.tail.shape[1] - 1)
        tpv = null.tail.gather(1, at[:, None])[:, 0].cpu().numpy()          # on the device: bit-equal to the table
    else:
        tpv = np.zeros(0)
    return enrichment_result([out[f].cpu().numpy() for f in _EFIELDS], out["counts"].cpu().numpy(), tab, tpv,
                             int(np.sum(labels == LABEL_EXCLUDED)), strands, shuffles, seed)


def enrichment_result(fields, counts, tab, threshold_pvalue, excluded, strands="both", shuffles=0, seed=0):
    """A MotifEnrichment from explainn_enrichment_test's outputs (in enrichment._FIELDS order), the tables
    (anything with ids, names, widths, widest and log_odds()) and the gathered per-site p-values."""
    fields = list(fields)
    best_pattern = np.asarray(fields[_EFIELDS.index("best_pattern")], dtype=np.int64)
    return MotifEnrichment(fields, counts, tab.log_odds(best_pattern), threshold_pvalue, tab.ids, tab.names,
                           tab.widths, excluded, tab.widest, strands, shuffles, seed)


def enrichment_rows(result, max_evalue=None):
    """The rows of the CLI's table: (id, name, threshold, threshold_pvalue, tp, tp %, fp, fp %, enrichment,
    log_pvalue, log_padj, evalue, qvalue, auroc) of the motifs with evalue <= max_evalue (None: all), by ascending
    log_pvalue, ties by motif order."""
    return _enr.table_rows(result, max_evalue, lambda u: (result.ids[u], result.names[u], float(result.threshold[u]),
                                                          float(result.threshold_pvalue[u])))


def write_enrichment_table(fh, rows):
    _enr.write_table(fh, rows, ENRICHMENT_COLUMNS, "%s\t%s\t%.6g\t%.4g")


# ---------------------------------------------------------------- filters and motifs in one table
def filters_and_motifs(filter_primary, motif_primary, filter_control, motif_control, device=None):
    """One enrichment table of a model's filters AND database motifs (the analogue of sites.concat_units): the
    RecordBest.bits of enrichment.best_sites and the MotifBest of best_motif_sites, of the same primary and the
    same control records, are stacked into one unit axis -- filters first -- and one explainn_enrichment_test
    call ranks them together.  A record shorter than the kernel or the widest live motif is left out.
    Returns an Enrichment with `names` ("filter<u>", then the motifs' ids) and `threshold` as float64: the
    float16 activation for a filter, the real log-odds for a motif."""
    sets = []
    for fb, mb in ((filter_primary, motif_primary), (filter_control, motif_control)):
        if not isinstance(fb, RecordBest) or not isinstance(mb, MotifBest):
            raise ValueError("filters_and_motifs takes RecordBest and MotifBest objects")
        if not np.array_equal(fb.lengths, mb.lengths):
            raise ValueError("the filters' and the motifs' best sites are not of the same records")
        sets.append(np.concatenate([fb.bits, mb.bits], axis=0))
    if sets[0].shape[0] != sets[1].shape[0] or filter_primary.score.shape[0] != filter_control.score.shape[0]:
        raise ValueError("the primary and the control sets hold different units")
    mp = motif_primary
    need = max([filter_primary.kernel_size] + [int(w) for w in mp.live_widths])
    labels = record_labels(filter_primary.lengths, filter_control.lengths, need)
    device = _lib.device_for(device, (), "pwmsites.filters_and_motifs")
    bits = torch.from_numpy(np.ascontiguousarray(np.concatenate(sets, axis=1)).view(np.int16)).to(device)
    out = _enr.enrichment_test(bits, torch.from_numpy(labels).to(device))
    res = Enrichment(*(out[f].cpu().numpy() for f in _EFIELDS), out["counts"].cpu().numpy(), need)
    U = filter_primary.score.shape[0]
    pat = res.best_pattern[U:].astype(np.float64)
    ok = mp.scale > 0
    res.threshold = np.concatenate([res.threshold[:U].astype(np.float64),
                                    np.where(ok, pat / np.where(ok, mp.scale, 1.0) + mp.widths * mp.lo, np.nan)])
    res.names = ["filter%d" % u for u in range(U)] + list(mp.names)
    return res


# ---------------------------------------------------------------- centrality
def width_groups(live_widths):
    """[(w, indices of the motifs of live width w)], ascending w, empty motifs (0) left out."""
    lw = np.asarray(live_widths)
    return [(int(w), np.flatnonzero(lw == w)) for w in sorted(set(lw[lw > 0].tolist()))]


class MotifCentrality:
    """centrality.Centrality's fields per motif (numpy, (M,)), the starts of a motif being M_starts = L - w + 1 of
    its own width w: best_t, best_lo, best_width, sites, count, n_tests, log_pvalue, log_padj, ctrl_sites,
    ctrl_count, log_fisher; `pvalues` (T,) the cutoffs and `iscore_thresholds` int32 (M, T) the integer
    thresholds explainn_pwm_null gives for them, `iscore_threshold` / `threshold` (real log-odds) / `pvalue` the
    chosen one; region_start, region_end, center in record coordinates (centrality.region_coordinates with the
    motif's width); expected = sites x best_width / M_starts; evalue = exp(log_padj) x live motifs and qvalue
    (Benjamini-Hochberg), fisher_evalue and fisher_qvalue over the LIVE motifs; an empty motif carries the "no
    threshold tried" outputs, evalue = live motifs and qvalue 1.  `counts` = (Np, Nc); `excluded` the records
    shorter than the widest live motif, left out for all motifs."""

    def __init__(self, fields, counts, pvalues, iscore_thresholds, tab, length, excluded=0, local=False, strands="both"):
        for f, x in zip(_CFIELDS, fields):
            setattr(self, f, np.asarray(x, dtype=_cen.field_dtype(f)))
        M = len(tab.ids)
        self.counts = np.asarray(counts, dtype=np.int64)
        self.pvalues = np.asarray(pvalues, dtype=np.float64).reshape(-1)
        self.iscore_thresholds = np.asarray(iscore_thresholds, dtype=np.int32).reshape(M, len(self.pvalues))
        self.ids, self.names, self.widths = list(tab.ids), list(tab.names), np.asarray(tab.widths, dtype=np.int32)
        self.live_widths = np.asarray(tab.live, dtype=np.int32)
        self.length, self.excluded, self.local, self.strands = int(length), int(excluded), bool(local), str(strands)
        if self.counts.shape != (2,) or any(getattr(self, f).shape != (M,) for f in _CFIELDS):
            raise ValueError("every per-motif field must be (M,) and counts (2,)")
        live = self.live_widths > 0
        n_live = int(live.sum())
        self.iscore_threshold = self.iscore_thresholds[np.arange(M), self.best_t] if M else np.zeros(0, np.int32)
        self.threshold = tab.log_odds(self.iscore_threshold)
        self.pvalue = self.pvalues[self.best_t] if M else np.zeros(0)
        self.starts = np.where(live, self.length - self.live_widths + 1, 0)
        self.region_start, self.region_end, self.center = _cen.region_coordinates(self.best_lo, self.best_width,
                                                                                   self.live_widths, self.length)
        self.expected = self.sites * self.best_width.astype(np.float64) / np.maximum(self.starts, 1)
        self.evalue = np.exp(self.log_padj) * n_live
        self.fisher_evalue = np.exp(self.log_fisher) * n_live
        self.qvalue, self.fisher_qvalue = np.ones(M), np.ones(M)
        if n_live:
            self.qvalue[live] = benjamini_hochberg(np.exp(self.log_pvalue[live]))
            self.fisher_qvalue[live] = benjamini_hochberg(np.exp(self.log_fisher[live]))

    @property
    def units(self):
        return len(self.ids)


def _check_pvalues(pvalues):
    p = np.atleast_1d(np.asarray(pvalues, dtype=np.float64))
    if p.ndim != 1 or not 1 <= len(p) <= _cen.MAX_THRESHOLDS or np.any(~(p >= 0.0)) or np.any(p > 1.0):
        raise ValueError("pvalues must be 1 to %d cutoffs in [0, 1] (got %r)" % (_cen.MAX_THRESHOLDS, pvalues))
    return p


def motif_centrality(motifs, records, pvalues=(1e-4,), control=None, local=False, min_width=1, max_width=None,
                     min_sites=1, bg=None, pseudocount=0.1, bins=100, strands="both", chunk_bases=None, device=None):
    """CentriMo's question for known motifs: are a motif's best sites concentrated at the centre of the
    `records` (summit-centred windows of one length L; ValueError otherwise -- records shorter than the widest
    live motif are left out for all motifs)?  pvalues: up to 16 per-site cutoffs; each becomes, per motif, the
    integer threshold explainn_pwm_null gives for it, and a record counts at a cutoff when its best site
    reaches that score.  The motifs are tested in groups of one width w, whose starts are L - w + 1
    (explainn_site_positions and explainn_centrality_test per group: centrality.positions_device /
    test_device), and the results are scattered back to motif order; log_padj is per motif.  control: records
    whose best sites are counted as set 1 (adds the Fisher test of the chosen region).  local, min_width,
    max_width, min_sites as centrality.centrality takes them.  Returns a MotifCentrality."""
    _cen.check_widths(min_width, max_width, min_sites)
    both = _enr._strands(strands) == 2
    pv = _check_pvalues(pvalues)
    tab = _Tables(motifs, bg, pseudocount, bins)
    if tab.widest == 0:
        raise ValueError("no motif is live (every motif is empty)")
    codes, labels_np, L = _cen.centred_records(records, control, tab.widest)
    device = _lib.device_for(device, (), "pwmsites.motif_centrality")
    labels = torch.from_numpy(labels_np).to(device)
    scorer = MotifScorer(tab, both, device)
    thr = np.stack([_pwm._null(tab.S, tab.live, tab.scale, tab.lo, tab.bins, tab.bg, p, device).thresholds.cpu().numpy()
                    for p in pv], axis=1).astype(np.int32)                               # (M, T)
    bits, site = best_over_records(scorer, codes, chunk_bases, True)
    pattern = bits + BRIDGE                                                              # normal halves, on the device
    fthr = torch.from_numpy(bridge_thresholds(thr)).to(device)
    full = {f: torch.zeros(tab.M, device=device, dtype=_cen.field_dtype(f, torch)) for f in _CFIELDS}
    counts = torch.from_numpy(np.array([np.sum(labels_np == 1), np.sum(labels_np == 0)], dtype=np.int64)).to(device)
    for w, idx in width_groups(tab.live):
        sel = torch.from_numpy(idx).to(device)
        hist, cnt = _cen.positions_device(pattern[sel].contiguous(), site[sel].contiguous(), labels,
                                          fthr[sel].contiguous(), L - w + 1)
        out = _cen.test_device(hist, cnt, local, min_width, max_width, min_sites)
        for f in _CFIELDS:
            full[f][sel] = out[f]
    return MotifCentrality([full[f].cpu().numpy() for f in _CFIELDS], counts.cpu().numpy(), pv, thr, tab, L,
                           int(np.sum(labels_np == LABEL_EXCLUDED)), local, strands)


def centrality_rows(result, max_evalue=None, control=None):
    """The rows of the CLI's table: (id, name) and centrality.table_rows' columns after the filter, of the LIVE
    motifs with evalue <= max_evalue (None: all), by ascending log_pvalue, ties by motif order."""
    return _cen.table_rows(result, max_evalue, control, lambda u: (result.ids[u], result.names[u]),
                           np.flatnonzero(result.live_widths > 0))


def write_centrality_table(fh, rows, control=None):
    _cen.write_table(fh, rows, control, CENTRALITY_COLUMNS, "%s\t%s")


# ---------------------------------------------------------------- command line
def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.pwmenrich", description=main.__doc__)
    sub = ap.add_subparsers(dest="command", required=True)
    for name in ("enrichment", "centrality"):
        p = sub.add_parser(name)
        p.add_argument("motifs", help="a MEME file, a JASPAR file or a directory of filter*.jaspar")
        p.add_argument("fasta_file", help="the primary records / the summit-centred peaks")
        p.add_argument("-o", "--output-file", required=True)
        p.add_argument("--control", help="control FASTA")
        p.add_argument("--bg", type=lambda text: _pwm._bg_arg(text, sequence=False), default=None,
                       help="uniform (default) or a,c,g,t")
        p.add_argument("--pseudocount", type=float, default=0.1)
        p.add_argument("--bins", type=int, default=100)
        p.add_argument("--strands", choices=("both", "fwd"), default="both")
        p.add_argument("--max-evalue", type=float, default=10.0)
    e, c = sub.choices["enrichment"], sub.choices["centrality"]
    e.add_argument("--shuffles", type=int, default=1, help="dinucleotide shuffles per primary record (no --control)")
    e.add_argument("--seed", type=int, default=0)
    e.add_argument("--save-best", help="write the primary records' best sites as .npz (MotifBest.load)")
    c.add_argument("--pvalue", type=float, action="append", help="per-site cutoff (default 1e-4); repeat for several")
    c.add_argument("--local", action="store_true", help="every range of starts, not only the centred ones")
    c.add_argument("--min-width", type=int, default=1)
    c.add_argument("--max-width", type=int, default=None)
    c.add_argument("--min-sites", type=int, default=1)
    return ap


def main(argv=None):
    """Known motifs (MEME / JASPAR) and a FASTA -> a table of motifs.  `enrichment`: by enrichment of their best
    site scores in the primary records against a control FASTA or dinucleotide shuffles; columns Motif, Name,
    Threshold (log-odds of the most significant score), ThresholdPvalue (per site, at that score), TP, TPpct, FP,
    FPpct, Enrichment, LogPvalue, LogPadj, Evalue, Qvalue, AUROC.  `centrality`: by central enrichment of their
    best sites in summit-centred windows of one length; centrality's columns after Motif, Name.  One row per
    motif with Evalue <= --max-evalue, by ascending p-value."""
    args = _parser().parse_args(argv)
    from .loader import read_fasta_records
    from .motifs import read_motifs
    motifs = read_motifs(args.motifs)
    records = read_fasta_records(args.fasta_file)
    control = read_fasta_records(args.control) if args.control else None
    common = dict(bg=args.bg, pseudocount=args.pseudocount, bins=args.bins, strands=args.strands)
    if args.command == "enrichment":
        result = motif_enrichment(motifs, records, control, args.shuffles, args.seed, **common)
        if args.save_best:
            best_motif_sites(motifs, records, **common).save(args.save_best)
        with open(args.output_file, "w") as fh:
            write_enrichment_table(fh, enrichment_rows(result, args.max_evalue))
    else:
        result = motif_centrality(motifs, records, tuple(args.pvalue or (1e-4,)), control, args.local, args.min_width,
                                  args.max_width, args.min_sites, **common)
        with open(args.output_file, "w") as fh:
            write_centrality_table(fh, centrality_rows(result, args.max_evalue, control is not None), control is not None)


if __name__ == "__main__":
    main()
