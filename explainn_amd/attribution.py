"""Integrated Gradients of FASTA or TSV sequences with a trained ExplaiNN.

    python -m explainn_amd.attribution MODEL_FILE SEQS(.fa|.tsv) -o OUT.npz
        [--baseline zero|uniform|shuffle|device-shuffle] [--n-shuffles R] [--steps S] [--target T] [--rev-complement]

The reference has no attribution command line; this one and its output format are this package's own.
OUT.npz holds
    ids    (N,)      sequence identifiers (the FASTA header up to the first blank / the TSV's first column)
    ig     (N,4,L)   float32 Integrated Gradients, rows A,C,G,T by position (interpret.integrated_gradients)
    delta  (N,)      float32 convergence delta sum(ig) - (F(x) - F(baseline)); more --steps shrink it
--baseline shuffle averages over --n-shuffles dinucleotide-preserving shuffles of each sequence
(sequence.dinucleotide_shuffle, --seed), drawn on the host one Euler path at a time.  --baseline
device-shuffle is the fast one: the same kind of shuffles drawn on the device batch by batch
(sequence.dinucleotide_shuffle_device), from a different random stream -- same law, other shuffles for
the same --seed.  --target picks one logit (default: their sum).
--rev-complement runs the model on the reverse complement and maps the result back onto the given strand.
"""
import argparse

import numpy as np

from .interpret import integrated_gradients
from .loader import read_fasta_codes, read_tsv_codes
from .predict import _load_model
from .sequence import dinucleotide_shuffle


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_file")
    ap.add_argument("sequence_file", help="FASTA, or a headerless TSV `id <tab> sequence [...]` (*.tsv[.gz])")
    ap.add_argument("-o", "--output-file", required=True)
    ap.add_argument("--baseline", choices=("zero", "uniform", "shuffle", "device-shuffle"), default="zero",
                    help="shuffle: host shuffles; device-shuffle: drawn on the device, much faster, a different "
                         "random stream")
    ap.add_argument("--n-shuffles", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--target", type=int, default=None)
    ap.add_argument("-r", "--rev-complement", action="store_true")
    ap.add_argument("-b", "--batch-size", type=int, default=1024)
    args = ap.parse_args(argv)
    name = args.sequence_file[:-3] if args.sequence_file.endswith(".gz") else args.sequence_file
    if name.endswith(".tsv"):
        codes, _, ids = read_tsv_codes(args.sequence_file)
    else:
        codes, ids = read_fasta_codes(args.sequence_file)
    model = _load_model(args.model_file)
    L = model._options["sequence_length"]
    if codes.shape[1] != L:
        raise SystemExit("sequences are %d bp, the model takes %d" % (codes.shape[1], L))
    baselines = args.baseline
    if baselines == "shuffle":
        baselines = dinucleotide_shuffle(codes, n=args.n_shuffles, seed=args.seed)
    elif baselines == "device-shuffle":
        baselines = "shuffle"
    ig, delta = integrated_gradients(model, codes, baselines, target=args.target, steps=args.steps,
                                     batch_size=args.batch_size, rev_complement=args.rev_complement,
                                     return_delta=True, n_shuffles=args.n_shuffles, seed=args.seed)
    np.savez(args.output_file, ids=np.asarray(ids).astype(str), ig=ig, delta=delta)


if __name__ == "__main__":
    main()
