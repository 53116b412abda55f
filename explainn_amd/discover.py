"""Which words are over-represented in my peaks at all, independent of any model?  De novo motif discovery on the
device: a DREME-style greedy loop over exact words.

The rest of the analysis suite starts from a motif somebody has -- a filter (`enrichment`, `centrality`, `spacing`)
or a database entry (`pwmsites`, `pwmenrich`, `pwmvariants`).  This module finds the motifs: before a training run
it says whether the data carries signal, after it `motifs.annotate(filters, found.as_motifs())` says which filters
are a rediscovered enriched word, and the found motifs go straight into `pwmsites.scan_motifs`,
`pwmenrich.motif_enrichment`, `spacing` and `motifs.write_meme`.

    found = discover(primary, control)               # or control=None: dinucleotide shuffles of the primary records
    found.word, found.evalue, found.pfm              # one entry per motif, in the order they were found
    write_meme("found.meme", found.as_motifs(), nsites=found.nsites)

The loop ("Word discovery"; the definitions are include/explainn_hip.h's):
  1. for every width, count the records that contain each word in both sets (explainn_word_counts) and test every
     word with the one-sided Fisher test (explainn_word_test); n_tests is the sum of n_tested over the widths;
  2. stop if the best logp is 0, or logp + ln(n_tests) > ln(max_evalue), or max_motifs is reached; across widths
     the smallest logp wins, among equal values the larger width (equal counts give bit-equal values, and the longer
     word is the more specific finding), then the lowest code;
  3. otherwise build the accept mask from the round's tables -- bit 4i+b (b != the seed's base at i) is set iff the
     word v, the seed with base i replaced by b, indexed canonically, has pos[v] >= min_count and
     logp[v] <= ln(accept_pvalue) -- and run the sites pass (explainn_word_sites) on the primary set (pfm, nsites,
     tp) and on the control set (fp);
  4. put the Fisher logp of (tp, fp) beside the seed's, through the same test entry point on a one-word table;
  5. continue on the two erased sequences.
What differs from DREME: no IUPAC wildcards (a motif is a seed word and its enriched one-mismatch neighbours, which
were tested already), a Bonferroni factor over the words seen, erasure in both sets.

Both sets go to the device once and the rounds ping-pong two buffers per set; per round the host reads the best word
of each width, at most 3k neighbour entries and the two totals.

`python -m explainn_amd.discover PRIMARY.fa [--control C.fa | --shuffles R --seed S] -o OUT.meme [--table OUT.tsv]`.
There is no CPU path and no model argument.
"""
import argparse
import math

import numpy as np

from .records import control_plan, record_codes
from .strands import check_strands

MIN_WIDTH, MAX_WIDTH = 3, 10         # EXPLAINN_WORD_MIN_WIDTH, EXPLAINN_WORD_MAX_WIDTH
COLUMNS = ("Motif", "Word", "Width", "Pos", "Neg", "LogPvalue", "Evalue", "Nsites", "TP", "FP", "MotifLogPvalue")
_BASES = "ACGT"


def word_string(code, k):
    """The k-mer of a word code: first base most significant, A,C,G,T = 0..3."""
    return "".join(_BASES[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def reverse_complement_code(code, k):
    out = 0
    for i in range(k):
        out = out * 4 + (3 - ((int(code) >> (2 * i)) & 3))
    return out


def _check_width(k):
    if int(k) != k or not MIN_WIDTH <= int(k) <= MAX_WIDTH:
        raise ValueError("a word width must be an integer in [%d, %d] (got %r)" % (MIN_WIDTH, MAX_WIDTH, k))
    return int(k)


# ---------------------------------------------------------------- the device calls
def _records_on_device(seq, offsets, what):
    import torch

    from . import _lib
    dev = _lib.require(seq, torch.uint8, (None,), None, "seq").device
    _lib.require(offsets, torch.int64, (None,), dev, "offsets")
    if offsets.shape[0] < 1:
        raise ValueError("%s: offsets holds n_records + 1 entries, at least one" % what)
    return dev, offsets.shape[0] - 1


def word_counts(seq, offsets, k, both=True, out=None, flags=None):
    """explainn_word_counts on device tensors: seq uint8 (n,), offsets int64 (R + 1,).  Returns the int32 (4^k,)
    table of presence counts; `out=` is added into (files accumulate).  `flags`: an int32 (1,) device tensor the
    call ORs into.  Enqueued on the current stream."""
    import torch

    from . import _lib
    k = _check_width(k)
    dev, R = _records_on_device(seq, offsets, "word_counts")
    if out is None:
        out = torch.zeros(4 ** k, dtype=torch.int32, device=dev)
    _lib.require(out, torch.int32, (4 ** k,), dev, "out")
    _lib.call("explainn_word_counts", dev, seq if seq.shape[0] else None, seq.shape[0], offsets, R, k, int(bool(both)),
              out, flags)
    return out


def word_test(pos, neg, Np, Nc, min_count=5):
    """explainn_word_test on two int32 (n,) count tables: (logp float64 (n,), best_code int64 (), n_tested int64 (),
    best_logp float64 ()) as device tensors, with no host synchronisation."""
    import torch

    from . import _lib
    dev = _lib.require(pos, torch.int32, (None,), None, "pos").device
    n = pos.shape[0]
    _lib.require(neg, torch.int32, (n,), dev, "neg")
    logp = torch.empty(n, dtype=torch.float64, device=dev)
    best = torch.empty(2, dtype=torch.int64, device=dev)
    best_logp = torch.empty(1, dtype=torch.float64, device=dev)
    _lib.call("explainn_word_test", dev, pos if n else None, neg if n else None, n, int(Np), int(Nc), int(min_count),
              logp if n else None, best, best_logp)
    return logp, best[0], best[1], best_logp[0]


def word_sites(seq, offsets, k, seed, accept, both=True, erase=True, flags=None, want_pfm=True, out=None):
    """explainn_word_sites on device tensors: (pfm int64 (k,4) or None, totals int64 (2,) = nsites, nrecords,
    seq_out uint8 like seq or None).  erase=False leaves seq_out out; `out=`: the tensor to erase into."""
    import torch

    from . import _lib
    k = _check_width(k)
    dev, R = _records_on_device(seq, offsets, "word_sites")
    pfm = torch.zeros((k, 4), dtype=torch.int64, device=dev) if want_pfm else None
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    seq_out = None
    if erase:
        seq_out = torch.empty_like(seq) if out is None else _lib.require(out, torch.uint8, tuple(seq.shape), dev, "out")
    _lib.call("explainn_word_sites", dev, seq if seq.shape[0] else None, seq.shape[0], offsets, R, k, int(bool(both)),
              int(seed), int(accept), seq_out if seq.shape[0] else None, pfm, totals, flags)
    return pfm, totals, seq_out


# ---------------------------------------------------------------- the result
class Discovery:
    """The motifs of discover(), in the order they were found; one entry per motif:

      word, width, seed, accept     the seed as a string, its width, its code and the accept mask (uint64)
      pos, neg                      records of the primary / control set that held the seed when it was chosen
      log_pvalue, n_tests, evalue   the seed's Fisher ln p, the words tested in its round, exp(log_pvalue) n_tests
      pfm                           list of (width, 4) int64 count matrices over the motif's sites in the primary set
      nsites, tp, fp                sites and records with a site in the primary set, records with one in the control
      motif_log_pvalue              the Fisher ln p of (tp, fp)

    and per call Np, Nc (records), widths, strands, shuffles, seed0 (of the shuffles), flags (bit 0: a byte above
    4 was read as N) and n_tests_last (of the round that stopped the loop)."""

    def __init__(self, rounds, Np, Nc, widths, strands, shuffles, seed0, flags, n_tests_last):
        col = lambda f, dt: np.array([r[f] for r in rounds], dtype=dt)
        self.word = [r["word"] for r in rounds]
        self.width, self.seed, self.accept = col("width", np.int64), col("seed", np.int64), col("accept", np.uint64)
        self.pos, self.neg = col("pos", np.int64), col("neg", np.int64)
        self.log_pvalue, self.n_tests = col("log_pvalue", np.float64), col("n_tests", np.int64)
        self.evalue = np.exp(self.log_pvalue + np.log(np.maximum(self.n_tests, 1)))
        self.pfm = [np.asarray(r["pfm"], dtype=np.int64) for r in rounds]
        self.nsites, self.tp, self.fp = col("nsites", np.int64), col("tp", np.int64), col("fp", np.int64)
        self.motif_log_pvalue = col("motif_log_pvalue", np.float64)
        self.Np, self.Nc, self.widths, self.strands = int(Np), int(Nc), tuple(widths), strands
        self.shuffles, self.seed0, self.flags, self.n_tests_last = int(shuffles), int(seed0), int(flags), int(n_tests_last)

    def __len__(self):
        return len(self.word)

    def as_motifs(self):
        """[(id, name, (width, 4) float64 counts)] as write_meme, motifs.compare / annotate, pwmsites.scan_motifs
        and pwmenrich.motif_enrichment take it; ids are such as word3_GATAAGC."""
        return [("word%d_%s" % (i + 1, w), w, m.astype(np.float64)) for i, (w, m) in enumerate(zip(self.word, self.pfm))]

    def table(self):
        """The rows of the CLI's table, one tuple per motif in COLUMNS' order."""
        ids = [m[0] for m in self.as_motifs()]
        return [(ids[i], self.word[i], int(self.width[i]), int(self.pos[i]), int(self.neg[i]), float(self.log_pvalue[i]),
                 float(self.evalue[i]), int(self.nsites[i]), int(self.tp[i]), int(self.fp[i]),
                 float(self.motif_log_pvalue[i])) for i in range(len(self))]


def write_table(fh, rows):
    fh.write("\t".join(COLUMNS) + "\n")
    for row in rows:
        fh.write("%s\t%s\t%d\t%d\t%d\t%.6g\t%.6g\t%d\t%d\t%d\t%.6g\n" % tuple(row))


# ---------------------------------------------------------------- the loop
def _check_args(widths, min_count, max_evalue, accept_pvalue, max_motifs, strands):
    check_strands(strands)
    widths = tuple(_check_width(k) for k in widths)
    if not widths or len(set(widths)) != len(widths):
        raise ValueError("widths must name at least one width, each once (got %r)" % (widths,))
    if int(min_count) != min_count or int(min_count) < 1:
        raise ValueError("min_count must be an integer of at least 1 (got %r)" % (min_count,))
    if not max_evalue > 0.0:
        raise ValueError("max_evalue must be positive (got %r)" % (max_evalue,))
    if not 0.0 < accept_pvalue <= 1.0:
        raise ValueError("accept_pvalue must lie in (0, 1] (got %r)" % (accept_pvalue,))
    if int(max_motifs) != max_motifs or int(max_motifs) < 0:
        raise ValueError("max_motifs must be a non-negative integer (got %r)" % (max_motifs,))
    return widths


def _flat(codes):
    """(uint8 tensor with one N behind the last record -- never empty --, int64 offsets), on the host."""
    import torch
    off = np.zeros(len(codes) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in codes], out=off[1:])
    return torch.from_numpy(np.concatenate(list(codes) + [np.full(1, 4, np.uint8)])), torch.from_numpy(off)


def _neighbours(k, seed, both):
    """[(bit, table index)] of the 3k one-mismatch neighbours of the seed."""
    out = []
    for i in range(k):
        d = (seed >> (2 * (k - 1 - i))) & 3
        for b in range(4):
            if b != d:
                v = seed + (b - d) * 4 ** (k - 1 - i)
                out.append((4 * i + b, min(v, reverse_complement_code(v, k)) if both else v))
    return out


def discover(primary, control=None, shuffles=1, seed=0, widths=(6, 7, 8), min_count=5, max_evalue=0.05,
             accept_pvalue=0.01, max_motifs=25, strands="both", device=None, return_sequences=False):
    """The enriched words of the `primary` records against the `control` records (lists of (id, codes) or of code
    arrays, as enrichment.enrichment takes them), widened and erased greedily: a Discovery.

    control=None: the control is `shuffles` dinucleotide-preserving shuffles of every primary record, drawn once on
    the device before the first round (sequence.dinucleotide_shuffle_device with `seed`); this needs primary records
    of one length.  Np and Nc count every record of a set, short ones included.  return_sequences=True also returns
    the two erased sequences the loop ended on, (Discovery, primary uint8 tensor, control uint8 tensor), each with
    one N behind the last record.  See the module's text for the loop."""
    import torch

    from . import _lib
    widths = _check_args(widths, min_count, max_evalue, accept_pvalue, max_motifs, strands)
    both = strands == "both"
    _, prim = record_codes(primary)
    ctrl, ctrl_lengths, shuffles = control_plan(prim, control, shuffles)
    device = _lib.device_for(device, (), "discover.discover")
    Np, Nc = len(prim), len(ctrl_lengths)
    p_host, p_off = _flat(prim)
    p_seq, p_off = p_host.to(device), p_off.to(device)
    if ctrl is None:
        from .sequence import dinucleotide_shuffle_device
        L = len(prim[0])
        shuf = dinucleotide_shuffle_device(p_seq[:Np * L].view(Np, L), shuffles, seed).reshape(-1)
        c_seq = torch.cat([shuf, torch.full((1,), 4, dtype=torch.uint8, device=device)])
        c_off = torch.arange(Nc + 1, dtype=torch.int64, device=device) * L
    else:
        c_host, c_off = _flat(ctrl)
        c_seq, c_off = c_host.to(device), c_off.to(device)
    p_next, c_next = torch.empty_like(p_seq), torch.empty_like(c_seq)
    flags = torch.zeros(1, dtype=torch.int32, device=device)
    tables = {k: (torch.empty(4 ** k, dtype=torch.int32, device=device),
                  torch.empty(4 ** k, dtype=torch.int32, device=device)) for k in widths}
    cut, rounds = math.log(accept_pvalue), []
    while True:
        logps, heads = {}, []
        for k in widths:
            pos, neg = tables[k]
            pos.zero_(), neg.zero_()
            word_counts(p_seq, p_off, k, both, out=pos, flags=flags)
            word_counts(c_seq, c_off, k, both, out=neg, flags=flags)
            logps[k], code, n_tested, lp = word_test(pos, neg, Np, Nc, min_count)
            heads.append(torch.stack([code.to(torch.float64), n_tested.to(torch.float64), lp]))
        heads = torch.stack(heads).cpu().numpy()              # the round's one read of the tests: (widths, 3)
        n_tests = int(heads[:, 1].sum())
        found = [(float(heads[j, 2]), -k, int(heads[j, 0])) for j, k in enumerate(widths) if heads[j, 0] >= 0]
        if not found or len(rounds) >= max_motifs:
            break
        lp, k, code = min(found)
        k = -k
        if lp + math.log(n_tests) > math.log(max_evalue):
            break
        near = _neighbours(k, code, both)
        idx = torch.tensor([code] + [v for _, v in near], dtype=torch.int64, device=device)
        pos, neg = tables[k]
        got = torch.stack([pos[idx].to(torch.float64), neg[idx].to(torch.float64), logps[k][idx]]).cpu().numpy()
        accept = 0
        for j, (bit, _) in enumerate(near, start=1):
            if got[0, j] >= min_count and got[2, j] <= cut:
                accept |= 1 << bit
        pfm, tot_p, _ = word_sites(p_seq, p_off, k, code, accept, both, out=p_next)
        _, tot_c, _ = word_sites(c_seq, c_off, k, code, accept, both, want_pfm=False, out=c_next)
        both_tot = torch.stack([tot_p, tot_c])
        motif_lp = word_test(both_tot[0, 1:].to(torch.int32), both_tot[1, 1:].to(torch.int32), Np, Nc, min_count)[0]
        tot = both_tot.cpu().numpy()
        rounds.append(dict(word=word_string(code, k), width=k, seed=code, accept=accept, pos=int(got[0, 0]),
                           neg=int(got[1, 0]), log_pvalue=lp, n_tests=n_tests, pfm=pfm.cpu().numpy(),
                           nsites=int(tot[0, 0]), tp=int(tot[0, 1]), fp=int(tot[1, 1]),
                           motif_log_pvalue=float(motif_lp.cpu().numpy()[0])))
        p_seq, p_next, c_seq, c_next = p_next, p_seq, c_next, c_seq
    result = Discovery(rounds, Np, Nc, widths, strands, shuffles, seed, int(flags.item()), n_tests)
    return (result, p_seq, c_seq) if return_sequences else result


# ---------------------------------------------------------------- command line
def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.discover", description=main.__doc__)
    ap.add_argument("primary_fasta")
    ap.add_argument("-o", "--output-file", required=True, help="the discovered motifs, MEME minimal text")
    ap.add_argument("--control", help="control FASTA; without it the control is shuffles of the primary records")
    ap.add_argument("--shuffles", type=int, default=1, help="dinucleotide shuffles per primary record")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--widths", type=lambda t: tuple(int(v) for v in t.split(",")), default=(6, 7, 8))
    ap.add_argument("--min-count", type=int, default=5)
    ap.add_argument("--max-evalue", type=float, default=0.05)
    ap.add_argument("--accept-pvalue", type=float, default=0.01)
    ap.add_argument("--max-motifs", type=int, default=25)
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--table", help="a TSV with one row per motif")
    return ap


def main(argv=None):
    """A FASTA of primary records (with a control FASTA, or shuffled on the device) -> the enriched words as MEME
    motifs, in the order they were found; --table adds Motif, Word, Width, Pos, Neg, LogPvalue, Evalue, Nsites, TP,
    FP, MotifLogPvalue."""
    args = _parser().parse_args(argv)
    from .loader import read_fasta_records
    from .motifs import write_meme
    primary = read_fasta_records(args.primary_fasta)
    control = read_fasta_records(args.control) if args.control else None
    found = discover(primary, control, args.shuffles, args.seed, args.widths, args.min_count, args.max_evalue,
                     args.accept_pvalue, args.max_motifs, args.strands)
    write_meme(args.output_file, found.as_motifs(), nsites=[int(n) for n in found.nsites])
    if args.table:
        with open(args.table, "w") as fh:
            write_table(fh, found.table())


if __name__ == "__main__":
    main()
