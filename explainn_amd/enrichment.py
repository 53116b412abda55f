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

`python -m explainn_amd.enrichment MODEL PRIMARY.fa [--control C.fa | --shuffles R --seed S] -o OUT.tsv`
"""
import argparse

import numpy as np
import torch

from .strands import check_strands

CHUNK_BASES = 1 << 26        # bases per device call of best_sites
COLUMNS = ("Filter", "Threshold", "TP", "TPpct", "FP", "FPpct", "Enrichment", "LogPvalue", "LogPadj", "Evalue",
           "Qvalue", "AUROC")
LABEL_PRIMARY, LABEL_CONTROL, LABEL_EXCLUDED = 1, 0, 2
_FIELDS = ("n_thresholds", "best_pattern", "tp", "fp", "log_pvalue", "log_padj", "u2", "auroc")


def _strands(strands):
    check_strands(strands)
    return 2 if strands == "both" else 1


def record_codes(records):
    """(ids, [1-D uint8 arrays]) of a list of (id, codes) pairs or of code arrays."""
    ids, codes = [], []
    for i, rec in enumerate(records):
        rid, c = rec if isinstance(rec, tuple) else (str(i), rec)
        c = c.cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        if c.dtype != np.uint8 or c.ndim != 1:
            raise ValueError("record %s: base codes must be a 1-D uint8 array" % (rid,))
        ids.append(rid)
        codes.append(c)
    return ids, codes


def record_chunks(lengths, chunk_bases):
    """[(first record, one past the last), ...]: runs of whole records of at most chunk_bases bases each (a
    record longer than that is a run of its own)."""
    chunk_bases = int(chunk_bases)
    if chunk_bases < 1:
        raise ValueError("chunk_bases must be at least 1 (got %d)" % chunk_bases)
    out, first, held = [], 0, 0
    for i, n in enumerate(lengths):
        if i > first and held + int(n) > chunk_bases:
            out.append((first, i))
            first, held = i, 0
        held += int(n)
    if len(lengths) > first:
        out.append((first, len(lengths)))
    return out


def record_labels(primary_lengths, control_lengths, kernel_size):
    """uint8 labels of the primary records followed by the control records: 1 / 0, and 2 (left out of the
    test) for a record shorter than the kernel, which has no site."""
    lab = np.concatenate([np.full(len(primary_lengths), LABEL_PRIMARY, np.uint8),
                          np.full(len(control_lengths), LABEL_CONTROL, np.uint8)])
    short = np.concatenate([np.asarray(primary_lengths, np.int64), np.asarray(control_lengths, np.int64)]) < kernel_size
    lab[short] = LABEL_EXCLUDED
    return lab


class RecordBest:
    """The best site of every unit in every record: `score` float16 (units, N), the largest activation over
    the record's live starts (0 where the record is shorter than the kernel); `start` int32 (units, N), the
    0-based forward start of the k-mer that holds it (-1 without one) -- the lowest among equal maxima;
    `strand` int8 (units, N), +1 / -1 ('+' wins a tie at one start; 0 without a site); `lengths` int64 (N,)."""

    def __init__(self, score, start, strand, lengths, kernel_size, ids=None):
        self.score = np.asarray(score, dtype=np.float16)
        self.start = np.asarray(start, dtype=np.int32)
        self.strand = np.asarray(strand, dtype=np.int8)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.kernel_size = int(kernel_size)
        self.ids = None if ids is None else [str(i) for i in ids]
        if self.score.ndim != 2 or self.score.shape != self.start.shape or self.score.shape != self.strand.shape or \
                self.lengths.shape != (self.score.shape[1],):
            raise ValueError("score, start and strand must be (units, N) and lengths (N,)")

    @property
    def bits(self):
        """uint16 (units, N): the scores' bit patterns, which sort like the scores."""
        return self.score.view(np.uint16)

    @classmethod
    def from_device(cls, bits, site, lengths, kernel_size, ids=None):
        site = np.asarray(site, dtype=np.int32)
        none = site < 0
        return cls(np.ascontiguousarray(bits).view(np.float16), np.where(none, -1, site >> 1),
                   np.where(none, 0, 1 - 2 * (site & 1)), lengths, kernel_size, ids)

    def save(self, path):
        with open(path, "wb") as fh:
            np.savez(fh, bits=self.bits, start=self.start, strand=self.strand, lengths=self.lengths,
                     k=np.int64(self.kernel_size), ids=np.array(self.ids if self.ids is not None else [], dtype=np.str_))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            ids = [str(i) for i in z["ids"]] if len(z["ids"]) == len(z["lengths"]) else None
            return cls(z["bits"].view(np.float16), z["start"], z["strand"], z["lengths"], int(z["k"]), ids)


def _device_best(model, codes, strands, chunk_bases, want_site):
    """(bits int16 -- the patterns are below 0x8000 --, site int32 or None), each (units, len(codes)) on the
    model's device: the records go over concatenated, in runs of whole records; every run is one
    explainn_record_best call."""
    if model.training:
        raise NotImplementedError("the best sites are an eval-mode export path; call model.eval()")
    device = model._device()
    lengths = np.array([len(c) for c in codes], dtype=np.int64)
    bits = torch.empty((model._units(), len(codes)), device=device, dtype=torch.int16)
    site = torch.empty((model._units(), len(codes)), device=device, dtype=torch.int32) if want_site else None
    chunk = CHUNK_BASES if chunk_bases is None else chunk_bases
    with torch.no_grad(), model.eval_cache():
        for r0, r1 in record_chunks(lengths, chunk):
            flat = np.concatenate(codes[r0:r1] + [np.full(1, 4, np.uint8)])      # never an empty tensor
            off = np.zeros(r1 - r0 + 1, dtype=np.int64)
            np.cumsum(lengths[r0:r1], out=off[1:])
            b, s = model._launch_record_best(torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device),
                                             strands, want_site)
            bits[:, r0:r1] = b
            if want_site:
                site[:, r0:r1] = s
    return bits, site


def best_sites(model, records, strands="both", chunk_bases=None):
    """The best site of every unit of `model` (an ExplaiNN, or an ExplaiNNBank: global unit indices) in every
    record.  records: a list of (id, codes) pairs (loader.read_fasta_records) or of 1-D uint8 code arrays, of
    any lengths.  strands="both" also takes the filter on the reverse complement of every k-mer.  The records
    go to the device concatenated, in chunks of at most chunk_bases bases (default 2^26) cut at record
    boundaries; the result does not depend on the chunking.  Eval mode only.  Returns a RecordBest."""
    n_strands = _strands(strands)
    ids, codes = record_codes(records)
    bits, site = _device_best(model, codes, n_strands, chunk_bases, True)
    if model.validate_input:
        model.check_input()
    return RecordBest.from_device(bits.cpu().numpy(), site.cpu().numpy(), [len(c) for c in codes],
                                  model._options["kernel_size"], ids)


def enrichment_test(bits, labels, want_tails=False):
    """explainn_enrichment_test on device tensors: bits int16 (units, N; patterns below 0x8000), labels uint8
    (N,).  Returns a dict of device tensors: n_thresholds, best_pattern (int32), tp, fp, u2 (int64), log_pvalue,
    log_padj, auroc (float64), each (units,), counts int64 (2,) = (Np, Nc) and, with want_tails, tails int32
    (units, 2, 32768): a_t and b_t (below 2^31)."""
    import ctypes as C

    from . import _lib
    if not torch.is_tensor(bits) or bits.dtype != torch.int16 or bits.dim() != 2 or bits.device.type != "cuda" or \
            not bits.is_contiguous():
        raise RuntimeError("bits must be a contiguous int16 tensor of shape (units, N) on a HIP device (there is "
                           "no CPU fallback)")
    units, n = bits.shape
    dev = bits.device
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or tuple(labels.shape) != (n,) or \
            labels.device != dev or not labels.is_contiguous():
        raise RuntimeError("labels must be a contiguous uint8 tensor of shape (%d,) on %s" % (n, dev))
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
    lib = _lib.load()
    nbytes = int(lib.explainn_enrichment_workspace_bytes(units, n))
    ws = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(lib.explainn_enrichment_test(
            bits.data_ptr(), labels.data_ptr(), units, n, *(out[f].data_ptr() for f in _FIELDS),
            out["counts"].data_ptr(), tails.data_ptr() if want_tails else None, ws.data_ptr(), nbytes,
            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    if want_tails:
        out["tails"] = tails
    return out


def benjamini_hochberg(pvalue):
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


def _shuffled_control(model, codes, shuffles, seed, n_strands, chunk_bases):
    """Device bits (units, N x shuffles) of `shuffles` dinucleotide-preserving shuffles of every record (all
    of one length L), drawn on the device chunk by chunk: column r * shuffles + s is shuffle s of record r."""
    from .sequence import dinucleotide_shuffle_device
    device = model._device()
    L = len(codes[0])
    rows = torch.from_numpy(np.stack(codes))
    per = max((CHUNK_BASES if chunk_bases is None else int(chunk_bases)) // max(L * shuffles, 1), 1)
    out = torch.empty((model._units(), len(codes) * shuffles), device=device, dtype=torch.int16)
    with torch.no_grad(), model.eval_cache():
        for r0 in range(0, len(codes), per):
            shuf = dinucleotide_shuffle_device(rows[r0:r0 + per].to(device), shuffles, seed, row0=r0).reshape(-1)
            n = shuf.numel() // L
            off = torch.arange(n + 1, device=device, dtype=torch.int64) * L
            out[:, r0 * shuffles:r0 * shuffles + n] = model._launch_record_best(shuf.contiguous(), off, n_strands, False)[0]
    return out


def enrichment(model, primary, control=None, shuffles=1, seed=0, strands="both", chunk_bases=None):
    """Enrichment of every filter of `model` (an ExplaiNN or an ExplaiNNBank) in the `primary` records against
    the `control` records (lists as best_sites takes them).  control=None: the control set is `shuffles`
    dinucleotide-preserving shuffles of every primary record, drawn on the device
    (sequence.dinucleotide_shuffle_device with `seed`: a pure function of (seed, record, shuffle)); this
    needs primary records of one length (ValueError otherwise).  Records shorter than the kernel are left out
    of the test.  Returns an Enrichment."""
    n_strands = _strands(strands)
    _, prim = record_codes(primary)
    if not prim:
        raise ValueError("no primary record")
    k = model._options["kernel_size"]
    if control is None:
        if int(shuffles) < 1:
            raise ValueError("shuffles must be at least 1 without a control set")
        if len({len(c) for c in prim}) != 1:
            raise ValueError("a shuffled control needs primary records of one length; pass control= for records "
                             "of unequal lengths")
        if len(prim[0]) == 0:
            raise ValueError("the primary records are empty")
        ctrl_lengths = np.repeat([len(c) for c in prim], int(shuffles))
    else:
        _, ctrl = record_codes(control)
        ctrl_lengths = [len(c) for c in ctrl]
        shuffles = 0
    labels = record_labels([len(c) for c in prim], ctrl_lengths, k)
    pbits, _ = _device_best(model, prim, n_strands, chunk_bases, False)
    if control is None:
        cbits = _shuffled_control(model, prim, int(shuffles), seed, n_strands, chunk_bases)
    else:
        cbits, _ = _device_best(model, ctrl, n_strands, chunk_bases, False)
    if model.validate_input:
        model.check_input()
    out = enrichment_test(torch.cat([pbits, cbits], dim=1).contiguous(), torch.from_numpy(labels).to(pbits.device))
    return Enrichment(*(out[f].cpu().numpy() for f in _FIELDS), out["counts"].cpu().numpy(), k, strands, shuffles, seed)


def table_rows(result, max_evalue=None):
    """The rows of the CLI's table: (filter, threshold, tp, tp %, fp, fp %, enrichment, log_pvalue, log_padj,
    evalue, qvalue, auroc) of the units with evalue <= max_evalue (None: all), by ascending log_pvalue, ties
    by filter."""
    Np, Nc = (float(c) for c in result.counts)
    keep = np.arange(result.units) if max_evalue is None else np.flatnonzero(result.evalue <= max_evalue)
    order = keep[np.lexsort((keep, result.log_pvalue[keep]))]
    pct = lambda x, n: 100.0 * float(x) / n if n > 0 else float("nan")
    return [(int(u), float(result.threshold[u]), int(result.tp[u]), pct(result.tp[u], Np), int(result.fp[u]),
             pct(result.fp[u], Nc), float(result.enrichment[u]), float(result.log_pvalue[u]),
             float(result.log_padj[u]), float(result.evalue[u]), float(result.qvalue[u]), float(result.auroc[u]))
            for u in order]


def write_table(fh, rows):
    fh.write("\t".join(COLUMNS) + "\n")
    for u, thr, tp, tpp, fp, fpp, enr, lp, la, ev, q, auc in rows:
        fh.write("filter%d\t%.6g\t%d\t%.2f\t%d\t%.2f\t%.4g\t%.6g\t%.6g\t%.4g\t%.4g\t%.4f\n" % (
            u, thr, tp, tpp, fp, fpp, enr, lp, la, ev, q, auc))


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
