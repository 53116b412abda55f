"""Where do the known motifs occur?  PWM hits of a sequence at an exact p-value cutoff, on the device.

`sites.call_sites` lists the sites of the model's own filters; this module lists those of motifs that come
from a database (JASPAR, a MEME file, `motifs.write_meme` output) -- what FIMO does, and what the reference
vendors PWMScan for -- so that filter sites can be annotated by the sites of known motifs and not only by
the shape of their matrices (`spacing.spacing(sites.concat_units(filter_calls, pwm_calls), ...)`).

    calls = scan_motifs(read_motifs("JASPAR.meme"), codes, pvalue=1e-4)      # both strands
    start, strand, score = calls.unit(3)                # '+' sites ascending, then '-' sites ascending
    calls.pvalue, calls.iscore, calls.widths, calls.names

A motif's log-odds against the background are rescaled to integers 0..bins per cell (`quantise`: FIMO's
per-motif rescaling; the pseudocount rule is this project's), so a site's score is an
integer and its null -- the score of a random w-mer drawn iid from the background -- is an exact
column-by-column convolution (explainn_pwm_null, fp64, on the device); the threshold of a motif is the
smallest integer score whose tail is <= pvalue.  The scan (explainn_pwm_sites, csrc/pwmsites.hip) lists every
(motif, strand, start) at or above it with the count / scan / emit scheme of call_sites.

`python -m explainn_amd.pwmsites MOTIFS FASTA -o OUT.bed` writes `SeqId start end name score strand pvalue`.
There is no CPU path.

    calls = scan_motifs(motifs, codes, qvalue=0.05)     # only sites at a false discovery rate of 5 %
    calls.qvalue                                        # Benjamini-Hochberg over ALL windows and strands

A site's score is an integer, so its q-value is a function of (motif, score): `score_histogram` counts the score
of every live window (explainn_pwm_score_histogram), and explainn_site_qvalues turns that histogram and the
null's tail into the table -- exact, and independent of the p-value cutoff.  `--qvalues [--max-qvalue Q]` adds
the column over the whole file (a first pass counts, the second lists).
"""
import argparse
import types

import numpy as np

from . import motifs as _motifs
from . import sites as _sites
from .sites import SiteCalls

WORKSPACE_BYTES = 256 << 20      # device scratch of one scan call; the chunk of start positions is sized to it


# ---------------------------------------------------------------- the score tables (host, fp64)
def _background(bg):
    """(4,) float64, all > 0, summing to 1; None: uniform."""
    if bg is None:
        return np.full(4, 0.25)
    b = np.zeros(0) if isinstance(bg, str) else np.asarray(bg, dtype=np.float64)
    if b.shape != (4,) or not np.all(np.isfinite(b)) or np.any(b <= 0) or abs(b.sum() - 1.0) > 1e-6:
        raise ValueError("bg must hold four positive frequencies (A, C, G, T) that sum to 1 (got %r)" % (bg,))
    return b / b.sum()


def _check_table_args(pseudocount, bins):
    if not (np.isfinite(pseudocount) and float(pseudocount) >= 0):
        raise ValueError("pseudocount must not be negative (got %r)" % (pseudocount,))
    if int(bins) != bins or not 1 <= int(bins) <= _motifs.MAX_BINS:
        raise ValueError("bins must be an integer in [1, %d] (got %r)" % (_motifs.MAX_BINS, bins))


def motif_list(motifs):
    """(names, [(w,4) float64]) of [(id, name, matrix)] or of anything motifs._as_set accepts; motifs without
    an identifier are called motif<i>."""
    if isinstance(motifs, (list, tuple)) and all(isinstance(m, tuple) and len(m) == 3 for m in motifs):
        return [str(m[0]) for m in motifs], [np.asarray(m[2], dtype=np.float64).reshape(-1, 4) for m in motifs]
    x, widths = _motifs._as_set(motifs, "cpu")
    x, widths = x.numpy().astype(np.float64), widths.numpy()
    if np.any(widths < 0) or np.any(widths > x.shape[1]):
        raise ValueError("a motif's width lies outside [0, %d]" % x.shape[1])
    return ["motif%d" % i for i in range(len(x))], [x[i, :widths[i]] for i in range(len(x))]


def quantise(motifs, bg=None, pseudocount=0.1, bins=100):
    """Integer score tables of [(w,4)] count or probability matrices (or [(id, name, matrix)]):

        p'[j][a] = (P[j][a] + pc bg[a]) / (1 + pc)          P = the column divided by its sum (0.25 where 0)
        l[j][a]  = log2(p'[j][a] / bg[a]);   lo, hi = min, max of l over the motif;   scale = bins / (hi - lo)
        S[j][a]  = rint((l[j][a] - lo) scale)                in [0, bins]; the real score of a site of
                                                            integer score s is s / scale + w lo

    Returns (S int16 (M,wmax,4) zero padded, widths int32 (M,), scale float64 (M,), lo float64 (M,)).  A motif of
    width 0, or one whose log-odds are all equal (hi == lo), is EMPTY: scale 0, lo 0, an all-zero table."""
    _check_table_args(pseudocount, bins)
    b = _background(bg)
    mats = [np.asarray(m[2] if isinstance(m, tuple) else m, dtype=np.float64).reshape(-1, 4) for m in motifs]
    M = len(mats)
    wmax = max([len(m) for m in mats] + [1])
    if wmax > _motifs.MAX_WIDTH:
        raise ValueError("motifs wider than %d columns are not supported (got %d)" % (_motifs.MAX_WIDTH, wmax))
    widths = np.array([len(m) for m in mats], dtype=np.int32).reshape(M)
    x = np.zeros((M, wmax, 4))                             # all motifs at once: a database holds thousands
    for i, m in enumerate(mats):
        x[i, :len(m)] = m
    bad = ~np.isfinite(x) | (x < 0)
    if bad.any():
        raise ValueError("motif %d holds a negative or non-finite entry" % int(np.nonzero(bad)[0][0]))
    inside = np.arange(wmax)[None, :, None] < widths[:, None, None]
    pc = float(pseudocount)
    tot = x.sum(axis=2, keepdims=True)
    p = np.where(tot > 0, x / np.where(tot > 0, tot, 1.0), 0.25)
    with np.errstate(divide="ignore"):
        l = np.log2((p + pc * b) / (1.0 + pc) / b)          # -inf where pc == 0 meets a zero probability
    bad = inside & ~np.isfinite(l)
    if bad.any():
        raise ValueError("motif %d has a zero probability and pseudocount is 0: its log-odds are not finite"
                         % int(np.nonzero(bad)[0][0]))
    a = np.where(inside, l, np.inf).min(axis=(1, 2))
    z = np.where(inside, l, -np.inf).max(axis=(1, 2))
    live = (widths > 0) & (z > a)
    scale = np.where(live, int(bins) / np.where(live, z - a, 1.0), 0.0)
    lo = np.where(live, a, 0.0)
    S = np.where(inside & live[:, None, None], np.rint((l - lo[:, None, None]) * scale[:, None, None]), 0.0).astype(np.int16)
    return S, widths, scale, lo


# ---------------------------------------------------------------- the device calls
class PwmNull:
    """The exact null of a set of quantised motifs, on the device: `tail` float64 (M, wmax bins + 2),
    tail[m][s] = P(score of a random w-mer >= s) (zero past w bins, all zero for an empty motif) and
    `thresholds` int32 (M,), the smallest s with tail[m][s] <= pvalue (w bins + 1: no score reaches it; an
    empty motif: 1).  `scores` (int16 (M,wmax,4)) and `widths` (int32, 0 for an empty motif) are the tables
    as the device calls take them; scale, lo (host float64) map integer scores back to log-odds."""

    def __init__(self, tail, thresholds, scores, widths, scale, lo, bins, bg, pvalue):
        self.tail, self.thresholds, self.scores, self.widths = tail, thresholds, scores, widths
        self.scale, self.lo, self.bins, self.bg, self.pvalue = scale, lo, int(bins), bg, float(pvalue)

    @property
    def wmax(self):
        return self.scores.shape[1]


def _null(S, live_widths, scale, lo, bins, bg, pvalue, device):
    import torch

    from . import _lib
    M, wmax = S.shape[0], S.shape[1]
    scores = torch.from_numpy(S).to(device).contiguous()
    widths = torch.from_numpy(live_widths).to(device)
    tail = torch.empty((M, wmax * int(bins) + 2), dtype=torch.float64, device=device)     # every entry is overwritten
    thr = torch.empty((M,), dtype=torch.int32, device=device)
    _lib.call("explainn_pwm_null", device, scores, widths, M, wmax, int(bins), float(bg[0]), float(bg[1]),
              float(bg[2]), float(bg[3]), float(pvalue), tail, thr)
    return PwmNull(tail, thr, scores, widths, scale, lo, bins, bg, pvalue)


def score_null(motifs, pvalue=1e-4, bg=None, pseudocount=0.1, bins=100, device=None):
    """quantise() and the exact null of every motif (explainn_pwm_null): a PwmNull.  Enqueued on the current
    stream; no host synchronisation."""
    _sites.check_pvalue(pvalue)
    _, mats = motif_list(motifs)
    b = _background(bg)
    S, widths, scale, lo = quantise(mats, b, pseudocount, bins)
    from . import _lib
    device = _lib.device_for(device, (), "pwmsites.score_null")
    return _null(S, np.where(scale > 0, widths, 0).astype(np.int32), scale, lo, bins, b, pvalue, device)


class PwmCalls(SiteCalls):
    """SiteCalls of known motifs: unit m = motif m, per motif '+' sites in ascending start, then '-' sites.
    `score` is the real log-odds (float32, bits), `iscore` the integer score (int32) the threshold and the
    p-value are functions of, `pvalue` float64; `widths` (int32, per motif) and `names` are carried, and
    kernel_size is the largest width.  `qvalue` (float64, None unless scan_motifs was asked for it) is the
    Benjamini-Hochberg q-value of the record over all the tests of its motif."""

    def __init__(self, offsets, start, strand, score, widths, names, iscore, pvalue, qvalue=None):
        self.widths = np.asarray(widths, dtype=np.int32)
        self.names = list(names)
        super().__init__(offsets, start, strand, score, int(self.widths.max()) if len(self.widths) else 0, pvalue,
                         qvalue)
        self.iscore = np.asarray(iscore, dtype=np.int32)
        if self.pvalue is None or self.iscore.shape != self.pvalue.shape:
            raise ValueError("iscore and pvalue must hold one value per record")
        if len(self.widths) != self.units or len(self.names) != self.units:
            raise ValueError("widths and names must hold one entry per motif")


def sequence_background(codes, strands="both"):
    """The ACGT frequencies of 1-D base codes (N left out), both strands pooled when strands == "both"
    (freq[A] == freq[T], freq[C] == freq[G])."""
    import torch
    if torch.is_tensor(codes):
        n = torch.bincount(codes.reshape(-1).to(torch.int64), minlength=256)[:4].cpu().numpy().astype(np.float64)
    else:
        n = np.bincount(np.asarray(codes).reshape(-1), minlength=256)[:4].astype(np.float64)
    if strands == "both":
        n = n + n[::-1]
    if np.any(n <= 0):
        raise ValueError("bg='sequence' needs every base A, C, G, T to occur in codes")
    return n / n.sum()


def _chunk_for(M, chunk_positions):
    """Start positions per call: what was asked for, else as many whole tiles as keep the workspace (one int
    per (motif, strand, tile)) under WORKSPACE_BYTES, 2^24 at the most."""
    from . import _lib
    if chunk_positions is not None:
        return int(chunk_positions)
    tiles = max(WORKSPACE_BYTES // (8 * max(M, 1)), 1)
    return int(min(_sites.CHUNK_POSITIONS, tiles * _lib.SITES_TILE))


def _count_scores(null, data, hist, both, period, chunk_positions):
    """Adds the scores of every live window of `data` (1-D uint8 tensor) under null's tables into hist, chunk by
    chunk (explainn_pwm_score_histogram)."""
    from . import _lib
    M, wmax, device = null.scores.shape[0], null.wmax, hist.device
    chunk = _sites.CHUNK_POSITIONS if chunk_positions is None else int(chunk_positions)
    for p0, cnt in _sites.position_chunks(int(data.shape[0]), chunk, period):
        piece = data[p0:p0 + cnt + wmax - 1].to(device).contiguous()
        _lib.call("explainn_pwm_score_histogram", device, piece, piece.shape[0], 0, cnt, int(period), int(both),
                  null.scores, null.widths, M, wmax, null.bins, hist)


def score_histogram(motifs, codes, bg=None, pseudocount=0.1, bins=100, strands="both", period=0, chunk_positions=None,
                    out=None, device=None):
    """The observed score histogram of `codes`: a device int64 (M, wmax bins + 2) tensor, [m][s] = the live windows
    of motif m, on either requested strand, whose integer score is s -- every test scan_motifs makes on these
    codes, the sites and all the others (each strand is a test).  motifs: as scan_motifs takes them (with bg,
    pseudocount and bins), or a PwmNull (score_null), whose tables are then used as they are.  The row stride is
    PwmNull.tail's.  out: a histogram to ADD into and return (one q-value over many records or files); None: a
    new one.  The sequence goes to the device in chunks of chunk_positions starts that overlap by wmax - 1 bases;
    the counts are integers, so the result does not depend on the chunking.  No host synchronisation."""
    import torch

    from . import _lib
    from .strands import as_codes_1d
    _sites._check_args(strands, chunk_positions, 0, period)
    data = as_codes_1d(codes)
    if isinstance(motifs, PwmNull):
        null = motifs
        device = null.scores.device
    else:
        b = sequence_background(data, strands) if isinstance(bg, str) and bg == "sequence" else _background(bg)
        null = score_null(motifs, 1.0, b, pseudocount, bins,
                          _lib.device_for(device, (data, out), "pwmsites.score_histogram"))
        device = null.scores.device
    M, stride = null.scores.shape[0], null.wmax * null.bins + 2
    if out is None:
        out = torch.zeros((M, stride), dtype=torch.int64, device=device)
    _lib.require(out, torch.int64, (M, stride), device, "out")
    if M and data.shape[0]:
        _count_scores(null, data, out, strands == "both", period, chunk_positions)
    return out


def scan_motifs(motifs, codes, pvalue=1e-4, bg=None, pseudocount=0.1, bins=100, strands="both", period=0,
                chunk_positions=None, max_sites=_sites.MAX_SITES, device=None, qvalue=None, observed=None):
    """Every site of every motif in `codes` at p-value <= pvalue: a PwmCalls.

    motifs: [(id, name, (w,4) matrix)] as read_meme / read_jaspar / read_motifs give them, or anything
    motifs.compare accepts (counts or probabilities).  codes: 1-D uint8 base codes (0..3 = A,C,G,T, 4 and above
    = N), numpy array or tensor, host or device.  bg: None = uniform, "sequence" = the ACGT frequencies of
    `codes` (both strands pooled when strands == "both"), or four frequencies.  (m, '+', p) is a site when
    the integer score of codes[p : p + w_m] under quantise()'s table reaches the motif's threshold (the
    smallest score with exact null tail <= pvalue); (m, '-', p) when that of its reverse complement does;
    a window that holds an N, or with period > 0 crosses a record boundary, is none.  The sequence goes to the
    device in chunks of start positions that overlap by wmax - 1 bases, sized so that the call's workspace
    stays under WORKSPACE_BYTES (or chunk_positions starts); each chunk takes a count call, one read of the
    total, and an emit call into buffers of exactly that size; the result does not depend on the chunking.
    More than max_sites records raise ValueError.

    qvalue = alpha: the result carries `qvalue`, the Benjamini-Hochberg q-value of every record over ALL the tests
    of its motif (explainn_site_qvalues on the observed score histogram and the null's tail: exact, and unlike a
    q-value estimated from the listed sites independent of pvalue), and only sites with q-value <= alpha are
    listed: each motif's integer threshold is raised to the smallest score that qualifies.  observed: a
    score_histogram accumulated beforehand over everything that forms one family of tests (many records, files)
    under the same motifs, bg, pseudocount, bins and strands; None counts `codes` alone.  observed without qvalue
    lists at pvalue and only adds the column."""
    import torch

    from . import _lib
    from .strands import as_codes_1d
    _sites._check_args(strands, chunk_positions, max_sites, period)
    _sites.check_pvalue(pvalue)
    want_q = qvalue is not None or observed is not None
    alpha = 1.0 if qvalue is None else float(qvalue)
    _sites.check_qvalue(alpha)
    names, mats = motif_list(motifs)
    data = as_codes_1d(codes)
    b = sequence_background(data, strands) if isinstance(bg, str) and bg == "sequence" else _background(bg)
    S, widths, scale, lo = quantise(mats, b, pseudocount, bins)
    device = _lib.device_for(device, (data,), "pwmsites.scan_motifs")
    M, wmax, n = len(mats), S.shape[1], int(data.shape[0])
    blocks, q = [], None
    if M and n:
        null = _null(S, np.where(scale > 0, widths, 0).astype(np.int32), scale, lo, bins, b, pvalue, device)
        thr = null.thresholds
        if want_q:
            if observed is None:
                observed = score_histogram(null, data, strands=strands, period=period, chunk_positions=chunk_positions)
            q, _, first = _sites.site_qtable(_lib.require(observed, torch.int64, tuple(null.tail.shape), device,
                                                          "observed"), null.tail, alpha)
            thr = torch.maximum(thr, first)
        chunks = _sites.position_chunks(n, _chunk_for(M, chunk_positions), period)
        ws, nbytes = _lib.workspace("explainn_pwm_sites_workspace_bytes", device, M, max(c for _, c in chunks))
        offsets = torch.empty((2 * M + 1,), dtype=torch.int64, device=device)
        both = int(strands == "both")
        with torch.cuda.device(device):
            def call(piece, cnt, pos, score, pv, capacity):
                _lib.call("explainn_pwm_sites", device, piece, piece.shape[0], 0, cnt, int(period), both, null.scores,
                          null.widths, M, wmax, thr, null.tail, int(bins), offsets, pos, score, pv,
                          capacity, ws, nbytes)

            def count(piece, cnt):
                call(piece, cnt, None, None, None, 0)
                return lambda: offsets.cpu().numpy()

            def emit(piece, cnt, total):
                out = [torch.empty((total,), dtype=dt, device=device)
                       for dt in (torch.int32, torch.int32, torch.float64)]      # pos, iscore, pvalue
                call(piece, cnt, *out, total)
                return lambda: [t.cpu().numpy() for t in out]

            # one leg on the current stream: its rows are the site list's, 2 m + (strand < 0)
            leg = types.SimpleNamespace(rows=np.arange(2 * M, dtype=np.int64), count=count, emit=emit)
            pieces = ((p0, cnt, data[p0:p0 + cnt + wmax - 1].to(device).contiguous()) for p0, cnt in chunks)
            blocks = _sites.site_blocks(pieces, [leg], M, max_sites, lambda *counted: _sites._too_many(
                *counted, names=names, advice="To list fewer, lower pvalue; or raise max_sites"))
    unit_offsets, start, strand, iscore, pv = _sites.assemble(blocks, M, (np.int32, np.float64))
    unit = np.repeat(np.arange(M), np.diff(unit_offsets))
    score = iscore / scale[unit] + widths[unit] * lo[unit]           # a record's motif is never empty: scale > 0
    qv = None
    if want_q:
        qv = np.zeros(0) if q is None or not len(unit) else q.view(-1)[
            torch.from_numpy(unit * q.shape[1] + iscore).to(device)].cpu().numpy()
    return PwmCalls(unit_offsets, start, strand, score, widths, names, iscore, pv, qv)


# ---------------------------------------------------------------- command line
def bed_rows(seq_id, calls):
    """Lines `SeqId start end name score strand pvalue` of one record's PwmCalls: sites.bed_rows with the
    motifs' names, end = start + the motif's width."""
    return _sites.bed_rows(seq_id, calls, calls.names, calls.widths)


def _bg_arg(text, sequence=True):
    """--bg: None for uniform, four frequencies, or -- where `sequence` says the tool takes it -- "sequence"."""
    if text == "uniform":
        return None
    if sequence and text == "sequence":
        return text
    try:
        vals = [float(v) for v in text.split(",")]
    except ValueError:
        vals = []
    if len(vals) != 4:
        raise argparse.ArgumentTypeError(
            "--bg takes uniform%s or four frequencies a,c,g,t" % (", sequence" if sequence else ""))
    return vals


def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.pwmsites", description=main.__doc__)
    ap.add_argument("motifs", help="a MEME file, a JASPAR file or a directory of filter*.jaspar")
    ap.add_argument("fasta_file")
    ap.add_argument("-o", "--output-file")
    ap.add_argument("--pvalue", type=float, default=1e-4)
    ap.add_argument("--bg", type=_bg_arg, default=None, help="uniform (default), sequence, or a,c,g,t")
    ap.add_argument("--pseudocount", type=float, default=0.1)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--qvalues", action="store_true",
                    help="a first pass counts the score of every window of the file, and an eighth column holds the "
                         "site's Benjamini-Hochberg q-value over all windows and strands of the file")
    ap.add_argument("--max-qvalue", type=float, default=None,
                    help="with --qvalues: list only the sites at or below this q-value (and at --pvalue)")
    return ap


def main(argv=None):
    """FASTA records of any length -> `SeqId start end name score strand pvalue`: one row per site of a known
    motif at p-value <= --pvalue, 0-based half-open, sorted by (start, motif, strand) within a record.  With
    --bg sequence every record is scored against its own base frequencies.  With --qvalues an eighth column holds
    the site's q-value over the whole file."""
    args = _parser().parse_args(argv)
    if args.qvalues and args.bg == "sequence":
        raise SystemExit("--qvalues does not go with --bg sequence: every record is then scored against its own "
                         "table, and the records do not form one family of tests")
    if args.max_qvalue is not None and not (args.qvalues and 0.0 <= args.max_qvalue <= 1.0):
        raise SystemExit("--max-qvalue needs --qvalues and a value in [0, 1]")
    from .loader import open_output, read_fasta_records
    motifs = _motifs.read_motifs(args.motifs)
    records = read_fasta_records(args.fasta_file)
    kwargs = {}
    if args.qvalues:
        # q-values are over the whole file: one pass counts every test, the second lists the sites
        null = score_null(motifs, args.pvalue, args.bg, args.pseudocount, args.bins)
        hist = None
        for _, codes in records:
            hist = score_histogram(null, codes, strands=args.strands, out=hist)
        kwargs = {"observed": hist, "qvalue": args.max_qvalue}
    with open_output(args.output_file) as fh:
        for rid, codes in records:
            fh.writelines(bed_rows(rid, scan_motifs(motifs, codes, pvalue=args.pvalue, bg=args.bg,
                                                    pseudocount=args.pseudocount, bins=args.bins,
                                                    strands=args.strands, **kwargs)))


if __name__ == "__main__":
    main()
