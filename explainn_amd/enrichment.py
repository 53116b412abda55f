"""Which filters are enriched in my peaks, and at what score?  Motif enrichment against a control set.

The first question asked of a trained ExplaiNN -- what SEA and AME of the MEME suite answer for PWMs.  Two
device passes (csrc/enrich.hip):

    best = best_sites(model, records)                     # per record the best site of every filter
    res = enrichment(model, peaks, control)               # or control=None: dinucleotide shuffles of the peaks
    res.log_pvalue, res.threshold, res.tp, res.fp, res.qvalue, res.auroc

best_sites: for every unit and record the largest float16 activation over the record's live starts and both
strands -- the value float16(model.linears[:3](window)).amax() gives, bit for bit, without windows or the
activation array -- and where it sits (the lowest start among equal maxima, '+' before '-').

enrichment: a record's score for a filter is that best activation.  The non-negative float16 bit patterns sort
like the values, so per filter the scores of the primary and the control records are two exact 32768-bin
integer histograms; at every score an included record holds, the one-sided Fisher (hypergeometric) test of
"primary records at or above it" is evaluated in fp64 on the device, and the most significant threshold is
reported with its multiple-testing correction over the thresholds tried.  Unlike SEA the score is the
filter's own activation, not a PWM log-odds, and a threshold at which the primary set is not enriched is
given p = 1 without being evaluated.

The host path from records to that matrix is explainn_amd.records, shared with `centrality` and `pwmenrich`.

`python -m explainn_amd.enrichment MODEL PRIMARY.fa [--control C.fa | --shuffles R --seed S] -o OUT.tsv`
"""
import argparse

import numpy as np
import torch

from .records import (CHUNK_BASES, LABEL_CONTROL, LABEL_EXCLUDED, LABEL_PRIMARY, FilterScorer,  # noqa: F401
                      RecordBest, best_over_records, enrichment_bits, record_chunks, record_codes, record_labels,
                      table_order)
from .strands import check_strands

COLUMNS = ("Filter", "Threshold", "TP", "TPpct", "FP", "FPpct", "Enrichment", "LogPvalue", "LogPadj", "Evalue",
           "Qvalue", "AUROC")
STAT_FORMAT = "%d\t%.2f\t%d\t%.2f\t%.4g\t%.6g\t%.6g\t%.4g\t%.4g\t%.4f"        # COLUMNS from TP on
_FIELDS = ("n_thresholds", "best_pattern", "tp", "fp", "log_pvalue", "log_padj", "u2", "auroc")


def _strands(strands):
    check_strands(strands)
    return 2 if strands == "both" else 1


def _device_best(model, codes, n_strands, chunk_bases, want_site):
    """records.best_over_records for a model's filters, under the name and signature callers know."""
    return best_over_records(FilterScorer(model, n_strands), codes, chunk_bases, want_site)


def best_sites(model, records, strands="both", chunk_bases=None):
    """The best site of every unit of `model` (an ExplaiNN, or an ExplaiNNBank: global unit indices) in every
    record.  records: a list of (id, codes) pairs (loader.read_fasta_records) or of 1-D uint8 code arrays, of
    any lengths.  strands="both" also takes the filter on the reverse complement of every k-mer.  The records
    go to the device concatenated, in chunks of at most chunk_bases bases (default 2^26) cut at record
    boundaries; the result does not depend on the chunking.  Eval mode only.  Returns a RecordBest."""
    scorer = FilterScorer(model, _strands(strands))
    ids, codes = record_codes(records)
    bits, site = best_over_records(scorer, codes, chunk_bases, True)
    scorer.finish()
    return RecordBest.from_device(bits.cpu().numpy(), site.cpu().numpy(), [len(c) for c in codes], scorer.need, ids)


def enrichment_test(bits, labels, want_tails=False):
    """explainn_enrichment_test on device tensors: bits int16 (units, N; patterns below 0x8000), labels uint8
    (N,).  Returns a dict of device tensors: n_thresholds, best_pattern (int32), tp, fp, u2 (int64), log_pvalue,
    log_padj, auroc (float64), each (units,), counts int64 (2,) = (Np, Nc) and, with want_tails, tails int32
    (units, 2, 32768): a_t and b_t (below 2^31)."""
    from . import _lib
    (units, n), dev = _lib.require(bits, torch.int16, (None, None), None, "bits").shape, bits.device
    _lib.require(labels, torch.uint8, (n,), dev, "labels")
    out = {"n_thresholds": torch.empty(units, device=dev, dtype=torch.int32),
           "best_pattern": torch.empty(units, device=dev, dtype=torch.int32),
           "tp": torch.empty(units, device=dev, dtype=torch.int64),
           "fp": torch.empty(units, device=dev, dtype=torch.int64),
           "log_pvalue": torch.empty(units, device=dev, dtype=torch.float64),
           "log_padj": torch.empty(units, device=dev, dtype=torch.float64),
           "u2": torch.empty(units, device=dev, dtype=torch.int64),
           "auroc": torch.empty(units, device=dev, dtype=torch.float64),
           "counts": torch.zeros(2, device=dev, dtype=torch.int64)}
    tails = torch.empty((units, 2, _lib.ACT_BINS), device=dev, dtype=torch.int32) if want_tails else None
    ws, nbytes = _lib.workspace("explainn_enrichment_workspace_bytes", dev, units, n)
    _lib.call("explainn_enrichment_test", dev, bits, labels, units, n, *(out[f] for f in _FIELDS), out["counts"], tails,
              ws, nbytes)
    if want_tails:
        out["tails"] = tails
    return out


def benjamini_hochberg(pvalue):
    """The 1-D numpy adapter of motifs.benjamini_hochberg ((Q,T) torch, per row): p-values (n,) -> q-values (n,)."""
    from .motifs import benjamini_hochberg as bh
    return bh(torch.as_tensor(np.asarray(pvalue, dtype=np.float64))[None, :])[0].numpy()


class Enrichment:
    """Per unit (numpy, (units,)): `n_thresholds` the scores tried; `best_pattern` the float16 bit pattern of
    the most significant one and `threshold` its value; `tp`, `fp` the primary / control records at or above
    it; `log_pvalue` ln of the one-sided Fisher p there; `log_padj` ln(1 - (1 - p)^n_thresholds); `evalue` =
    exp(log_padj) x units; `qvalue` Benjamini-Hochberg of the p-values over the units; `enrichment` =
    ((tp + 1) / (Np + 1)) / ((fp + 1) / (Nc + 1)), SEA's ratio; `u2` twice the Mann-Whitney U of primary over
    control and `auroc` = u2 / (2 Np Nc).  `counts` = (Np, Nc): the records in the test."""

    def __init__(self, n_thresholds, best_pattern, tp, fp, log_pvalue, log_padj, u2, auroc, counts, kernel_size=0,
                 strands="both", shuffles=0, seed=0):
        self.n_thresholds = np.asarray(n_thresholds, dtype=np.int32)
        self.best_pattern = np.asarray(best_pattern, dtype=np.int32)
        self.tp, self.fp, self.u2 = (np.asarray(x, dtype=np.int64) for x in (tp, fp, u2))
        self.log_pvalue, self.log_padj, self.auroc = (np.asarray(x, dtype=np.float64) for x in (log_pvalue, log_padj, auroc))
        self.counts = np.asarray(counts, dtype=np.int64)
        self.kernel_size, self.strands, self.shuffles, self.seed = int(kernel_size), str(strands), int(shuffles), int(seed)
        units = len(self.best_pattern)
        if self.counts.shape != (2,) or any(getattr(self, f).shape != (units,) for f in _FIELDS):
            raise ValueError("every per-unit field must be (units,) and counts (2,)")
        if units and (self.best_pattern.min() < 0 or self.best_pattern.max() > 0x7FFF):
            raise ValueError("best_pattern must be a non-negative float16 bit pattern")
        Np, Nc = (float(c) for c in self.counts)
        self.threshold = self.best_pattern.astype(np.uint16).view(np.float16)
        self.enrichment = ((self.tp + 1.0) / (Np + 1.0)) / ((self.fp + 1.0) / (Nc + 1.0))
        self.evalue = np.exp(self.log_padj) * units
        self.qvalue = benjamini_hochberg(np.exp(self.log_pvalue)) if units else np.zeros(0)

    @property
    def units(self):
        return len(self.best_pattern)

    def save(self, path):
        """.npz of the device outputs, the record counts and how the control was drawn."""
        with open(path, "wb") as fh:
            np.savez(fh, counts=self.counts, k=np.int64(self.kernel_size), strands=np.str_(self.strands),
                     shuffles=np.int64(self.shuffles), seed=np.int64(self.seed),
                     **{f: getattr(self, f) for f in _FIELDS})

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(*(z[f] for f in _FIELDS), z["counts"], int(z["k"]), str(z["strands"]), int(z["shuffles"]),
                       int(z["seed"]))


def enrichment(model, primary, control=None, shuffles=1, seed=0, strands="both", chunk_bases=None):
    """Enrichment of every filter of `model` (an ExplaiNN or an ExplaiNNBank) in the `primary` records against
    the `control` records (lists as best_sites takes them).  control=None: the control set is `shuffles`
    dinucleotide-preserving shuffles of every primary record, drawn on the device
    (sequence.dinucleotide_shuffle_device with `seed`: a pure function of (seed, record, shuffle)); this
    needs primary records of one length (ValueError otherwise).  Records shorter than the kernel are left out
    of the test.  Returns an Enrichment."""
    scorer = FilterScorer(model, _strands(strands))
    bits, labels, shuffles = enrichment_bits(scorer, primary, control, shuffles, seed, chunk_bases)
    out = enrichment_test(bits, torch.from_numpy(labels).to(bits.device))
    return Enrichment(*(out[f].cpu().numpy() for f in _FIELDS), out["counts"].cpu().numpy(), scorer.need, strands,
                      shuffles, seed)


def table_rows(result, max_evalue=None, lead=None):
    """The rows of the CLI's table: (filter, threshold, tp, tp %, fp, fp %, enrichment, log_pvalue, log_padj,
    evalue, qvalue, auroc) of the units with evalue <= max_evalue (None: all), by ascending log_pvalue, ties
    by filter.  lead: a function of the unit whose tuple stands in place of (filter, threshold)."""
    lead = lead or (lambda u: (int(u), float(result.threshold[u])))
    Np, Nc = (float(c) for c in result.counts)
    pct = lambda x, n: 100.0 * float(x) / n if n > 0 else float("nan")
    return [lead(u) + (int(result.tp[u]), pct(result.tp[u], Np), int(result.fp[u]), pct(result.fp[u], Nc),
                       float(result.enrichment[u]), float(result.log_pvalue[u]), float(result.log_padj[u]),
                       float(result.evalue[u]), float(result.qvalue[u]), float(result.auroc[u]))
            for u in table_order(result, max_evalue)]


def write_table(fh, rows, columns=COLUMNS, lead="filter%d\t%.6g"):
    """The rows as TSV: `lead` formats what table_rows' lead gave, STAT_FORMAT the rest."""
    fh.write("\t".join(columns) + "\n")
    for row in rows:
        fh.write((lead + "\t" + STAT_FORMAT + "\n") % tuple(row))


def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.enrichment", description=main.__doc__)
    ap.add_argument("model_file")
    ap.add_argument("primary_fasta")
    ap.add_argument("-o", "--output-file", required=True)
    ap.add_argument("--control", help="control FASTA; without it the control is shuffles of the primary records")
    ap.add_argument("--shuffles", type=int, default=1, help="dinucleotide shuffles per primary record")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--max-evalue", type=float, default=10.0)
    ap.add_argument("--save-best", help="write the primary records' best sites as .npz (RecordBest.load)")
    return ap


def main(argv=None):
    """MODEL and a FASTA of primary records (with a control FASTA, or shuffled on the device) -> a table of
    filters by enrichment: Filter, Threshold (the most significant score), TP, TPpct, FP, FPpct, Enrichment,
    LogPvalue, LogPadj, Evalue, Qvalue, AUROC; one row per filter with Evalue <= --max-evalue, by ascending
    p-value."""
    args = _parser().parse_args(argv)
    from .loader import read_fasta_records
    from .predict import _load_model
    primary = read_fasta_records(args.primary_fasta)
    control = read_fasta_records(args.control) if args.control else None
    model = _load_model(args.model_file)
    model.eval()
    result = enrichment(model, primary, control, args.shuffles, args.seed, args.strands)
    if args.save_best:
        best_sites(model, primary, args.strands).save(args.save_best)
    with open(args.output_file, "w") as fh:
        write_table(fh, table_rows(result, args.max_evalue))


if __name__ == "__main__":
    main()
