"""Site thresholds with an error rate behind them.

    python -m explainn_amd.calibrate MODEL FASTA -o thresholds.tsv --pvalue 1e-4
        [--background shuffle|sequence] [--shuffles R] [--seed S] [--period L] [--save-null NULL.npz]
        [--qvalue Q --target FASTA]

Builds the empirical null of every filter's activation over a background (sites.activation_null: the
exact per-filter histogram of the float16 activation, on the device) and writes, per filter, the
smallest threshold at which `python -m explainn_amd.sites` calls at most floor(pvalue x null size)
of the background's positions -- the file sites.read_thresholds reads.

--background sequence counts the FASTA's own k-mers, both strands.  --background shuffle (the
default) counts --shuffles dinucleotide-preserving shuffles of every record instead, drawn on the
device: a background without the motifs but with the records' composition.  Shuffles need records of
one length: --period L cuts the records into rows of L bases (every record a multiple of L long); by
default L is the records' common length.  With a period no k-mer crosses a row boundary.
--save-null keeps the null for `python -m explainn_amd.sites --null`, which adds p-values.
--qvalue Q --target FASTA writes, in place of --pvalue's, the thresholds of a false discovery rate: those at
which `python -m explainn_amd.sites` lists exactly the sites of the target FASTA whose Benjamini-Hochberg
q-value, over every position and strand of that file, is at most Q (sites.site_qvalues).
"""
import argparse

import numpy as np


def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.calibrate", description=main.__doc__)
    ap.add_argument("model_file")
    ap.add_argument("fasta_file")
    ap.add_argument("-o", "--output-file", required=True, help="thresholds.tsv (filter, threshold)")
    ap.add_argument("--pvalue", type=float, default=1e-4, help="false-positive rate per background position")
    ap.add_argument("--background", choices=("shuffle", "sequence"), default="shuffle")
    ap.add_argument("--shuffles", type=int, default=10, help="shuffles per record (--background shuffle)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--period", type=int, default=None,
                    help="row length; default: the records' common length, 0 (none) if they differ")
    ap.add_argument("--save-null", help="write the null as .npz (sites --null)")
    ap.add_argument("--qvalue", type=float, default=None,
                    help="with --target: thresholds of this false discovery rate in place of --pvalue's")
    ap.add_argument("--target", help="FASTA to be scanned: --qvalue's thresholds list its sites with q-value <= Q")
    return ap


def background_null(model, records, background="shuffle", shuffles=10, seed=0, period=None):
    """The ActivationNull of (id, codes) records (loader.read_fasta_records) as the CLI builds it."""
    from . import sites
    codes = [np.asarray(c, dtype=np.uint8) for _, c in records if len(c)]
    if not codes:
        raise ValueError("the FASTA file holds no bases")
    if period is None:
        lengths = {len(c) for c in codes}
        period = lengths.pop() if len(lengths) == 1 else 0
    if period > 0:
        ragged = [len(c) for c in codes if len(c) % period]
        if ragged:
            raise ValueError("a record of %d bases is no whole number of rows of --period %d" % (ragged[0], period))
        rows = np.concatenate(codes).reshape(-1, period)
        return sites.activation_null(model, rows, shuffles=shuffles if background == "shuffle" else 0,
                                     seed=seed)
    if background == "shuffle":
        raise ValueError("--background shuffle needs records of one length, or --period L")
    # records of unequal lengths: one histogram over all of them, no k-mer across two records
    return sites.records_null(model, codes, "both", seed)


def main(argv=None):
    """MODEL and a background FASTA -> thresholds.tsv: per filter the threshold of a stated
    false-positive rate against the empirical null of its activation."""
    args = _parser().parse_args(argv)
    from .loader import read_fasta_records
    from .predict import _load_model
    from .sites import write_thresholds
    if not 0.0 <= args.pvalue <= 1.0:
        raise SystemExit("--pvalue must be in [0, 1]")
    if (args.qvalue is None) != (args.target is None) or not 0.0 <= (args.qvalue or 0.0) <= 1.0:
        raise SystemExit("--qvalue (in [0, 1]) and --target go together")
    records = read_fasta_records(args.fasta_file)
    model = _load_model(args.model_file)
    model.eval()
    null = background_null(model, records, args.background, args.shuffles, args.seed, args.period)
    if args.qvalue is None:
        thresholds = null.thresholds(args.pvalue)
    else:
        from .sites import records_null, site_qvalues
        observed = records_null(model, (c for _, c in read_fasta_records(args.target)), null.strands)
        thresholds = site_qvalues(observed, null).thresholds(args.qvalue)
    write_thresholds(args.output_file, thresholds)
    if args.save_null:
        null.save(args.save_null)


if __name__ == "__main__":
    main()
