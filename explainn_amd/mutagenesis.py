"""In-silico mutagenesis of FASTA sequences with a trained ExplaiNN.

    python -m explainn_amd.mutagenesis MODEL_FILE FASTA -o OUT.npz [-r] [-b N] [--absolute]

The reference has no ISM command line; this one and its output format are this package's own.
OUT.npz holds
    ids     (N,)       sequence identifiers (the FASTA header up to the first blank)
    logits  (N,T)      float32 eval-mode logits of each sequence
    delta   (N,T,4,L)  float32 logit change of each single-base substitution, rows A,C,G,T by
                       position (interpret.in_silico_mutagenesis); the mutant logits themselves with
                       --absolute.  0 at the reference base.
-r runs the model on the reverse complement of every sequence and maps the result back onto the
given strand (logits are then those of the reverse strand).
"""
import argparse

import numpy as np

from .interpret import in_silico_mutagenesis
from .loader import read_fasta_codes
from .predict import _load_model


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model_file")
    ap.add_argument("fasta_file")
    ap.add_argument("-o", "--output-file", required=True)
    ap.add_argument("-r", "--rev-complement", action="store_true")
    ap.add_argument("-b", "--batch-size", type=int, default=1024)
    ap.add_argument("--absolute", action="store_true")
    args = ap.parse_args(argv)
    codes, ids = read_fasta_codes(args.fasta_file)
    model = _load_model(args.model_file)
    L = model._options["sequence_length"]
    if codes.shape[1] != L:
        raise SystemExit("sequences are %d bp, the model takes %d" % (codes.shape[1], L))
    delta, logits = in_silico_mutagenesis(model, codes, batch_size=args.batch_size, rev_complement=args.rev_complement,
                                          absolute=args.absolute, return_logits=True)
    np.savez(args.output_file, ids=np.asarray(ids), logits=logits, delta=delta)


if __name__ == "__main__":
    main()
