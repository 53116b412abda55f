"""Compare motifs on the device: what each filter learned and which filters are the same motif.

The reference sends the matrices interpret.py exports to external programs for this (Tomtom against JASPAR,
RSAT matrix-clustering).  Here the all-pairs comparison is one device call (csrc/motifs.hip,
explainn_motif_compare): for every (query, target) the best ungapped alignment over offsets and both strands
by width-normalised Pearson correlation -- RSAT's `cor` and `Ncor` ("Motif
comparison") -- and annotation, single-linkage clustering and reproducibility across the members of a model
bank are torch reductions over that matrix.  `significance` adds what an annotation is usually read by: the
p-value of every pair's best alignment under the null of Gupta et al. 2007 (Tomtom with incomplete scores and
Pearson columns; explainn_motif_significance), E-values and Benjamini-Hochberg
q-values over the targets of each query; `annotate(by="pvalue")` ranks and filters by them.  `write_meme`
writes the filters in the format an external Tomtom reads.

  python -m explainn_amd.motifs annotate MOTIFS DB -o OUT.tsv [--by pvalue [--max-qvalue Q] [--bins B]]
  python -m explainn_amd.motifs cluster MOTIFS [MOTIFS ...] -o OUT.tsv
  python -m explainn_amd.motifs merge MOTIFS [MOTIFS ...] -o OUT.meme [--linkage average|complete|single]
      [--min-ncor 0.4] [--min-support 0.5] [--min-ic 0] [--tree OUT.nwk] [--table OUT.tsv]
`tree` agglomerates a self-comparison into a dendrogram on the device (csrc/motiftree.hip; single, complete or
average linkage of Ncor quantised to 2^-20, so the tree is the same on every run), `MotifTree.cut` cuts it and
places every member in its cluster's frame from the alignments `compare` found, and `merge` sums the placed
count matrices per cluster: the non-redundant motifs of a model ("Motif tree").
MOTIFS / DB: a MEME file, a JASPAR file (the layout interpret.format_jaspar writes, any number of motifs),
or a directory of filter*.jaspar.
"""
import argparse
import collections
import glob
import os
import re

import numpy as np

MAX_WIDTH = 64

MAX_BINS = 128

MotifComparison = collections.namedtuple("MotifComparison", "ncor cor offset strand overlap")
MotifSignificance = collections.namedtuple("MotifSignificance", "pvalue evalue qvalue offset strand overlap score")


# ---------------------------------------------------------------- files
def read_meme(path):
    """MEME minimal text -> [(id, name, (w,4) float64 probabilities)]."""
    out = []
    with open(path) as fh:
        lines = [ln.strip() for ln in fh]
    i = 0
    while i < len(lines):
        if not lines[i].startswith("MOTIF"):
            i += 1
            continue
        parts = lines[i].split()
        if len(parts) < 2:
            raise ValueError("%s line %d: MOTIF without an identifier" % (path, i + 1))
        ident, name = parts[1], " ".join(parts[2:])
        i += 1
        while i < len(lines) and not lines[i].startswith("letter-probability matrix"):
            if lines[i].startswith("MOTIF"):
                raise ValueError("%s: motif %s has no letter-probability matrix" % (path, ident))
            i += 1
        if i == len(lines):
            raise ValueError("%s: motif %s has no letter-probability matrix" % (path, ident))
        m = re.search(r"alength=\s*(\d+)", lines[i])
        if m and int(m.group(1)) != 4:
            raise ValueError("%s: motif %s is not over a 4-letter alphabet" % (path, ident))
        m = re.search(r"\bw=\s*(\d+)", lines[i])
        want = int(m.group(1)) if m else None
        i += 1
        rows = []
        while i < len(lines) and (len(rows) < want if want is not None else not lines[i].startswith("MOTIF")):
            vals = lines[i].split()
            i += 1
            if not vals:
                continue
            try:
                row = [float(v) for v in vals]
            except ValueError:
                if want is None:
                    break                                  # the matrix ended (a URL line, the next section)
                raise ValueError("%s: motif %s: cannot read the row %r" % (path, ident, lines[i - 1]))
            if len(row) != 4:
                raise ValueError("%s: motif %s: a row of %d values" % (path, ident, len(row)))
            rows.append(row)
        if want is not None and len(rows) != want:
            raise ValueError("%s: motif %s: %d rows, w= %d" % (path, ident, len(rows), want))
        out.append((ident, name, np.array(rows, dtype=np.float64).reshape(-1, 4)))
    return out


def read_jaspar(path):
    """The layout interpret.format_jaspar writes ('>id name', then 'A [ ... ]' .. 'T [ ... ]'), any number of
    motifs in one file -> [(id, name, (w,4) float64 counts)].  An empty file gives an empty list."""
    out, head, rows = [], None, {}

    def close():
        if head is None:
            return
        if sorted(rows) != list("ACGT") or len({len(v) for v in rows.values()}) != 1:
            raise ValueError("%s: motif %s needs rows A, C, G, T of one length" % (path, head[0]))
        out.append((head[0], head[1], np.array([rows[a] for a in "ACGT"], dtype=np.float64).T.reshape(-1, 4)))

    with open(path) as fh:
        for ln in fh:
            ln = ln.strip()
            if not ln:
                continue
            if ln.startswith(">"):
                close()
                parts = ln[1:].split(None, 1)
                if not parts:
                    raise ValueError("%s: header without an identifier" % path)
                head, rows = (parts[0], parts[1].strip() if len(parts) > 1 else ""), {}
                continue
            m = re.match(r"^([ACGT])\s*\[(.*)\]\s*$", ln)
            if not m or head is None:
                raise ValueError("%s: cannot read %r" % (path, ln))
            rows[m.group(1)] = [float(v) for v in m.group(2).split()]
    close()
    return out


def _fmt(v):
    return np.format_float_positional(float(v), unique=True, trim="0")


def write_meme(path, motifs, nsites=None):
    """[(id, name, (w,4))] -> MEME minimal text.  Columns that already sum to 1 are written as they are (every
    digit, so read_meme returns them exactly); count columns are divided by their sum (an all-zero column
    becomes 0.25).  nsites: one number per motif; default: the largest column sum of a count matrix, 20 (MEME's
    own default) for probabilities."""
    with open(path, "wt") as fh:
        fh.write("MEME version 4\n\nALPHABET= ACGT\n\nstrands: + -\n\n"
                 "Background letter frequencies\nA 0.25 C 0.25 G 0.25 T 0.25\n\n")
        for i, (ident, name, m) in enumerate(motifs):
            m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
            tot = m.sum(axis=1)
            is_prob = bool(len(m)) and bool(np.all(np.abs(tot - 1.0) < 1e-6))
            if nsites is not None:
                ns = nsites[i]
            else:
                ns = 20 if is_prob or not len(m) else max(1, int(round(tot.max())))
            if not is_prob:
                m = np.where(tot[:, None] > 0, m / np.where(tot > 0, tot, 1.0)[:, None], 0.25)
            fh.write("MOTIF %s\n" % (("%s %s" % (ident, name)).strip()))
            fh.write("letter-probability matrix: alength= 4 w= %d nsites= %d E= 0\n" % (len(m), int(ns)))
            for row in m:
                fh.write(" ".join(_fmt(v) for v in row) + "\n")
            fh.write("\n")


def read_motifs(path):
    """A MEME file, a JASPAR file or a directory of filter*.jaspar (in filter order; empty files, which
    interpret writes for filters without a site, are skipped)."""
    if os.path.isdir(path):
        files = glob.glob(os.path.join(path, "filter*.jaspar"))
        if not files:
            raise ValueError("%s holds no filter*.jaspar" % path)
        num = lambda f: int(re.search(r"filter(\d+)\.jaspar$", f).group(1)) if re.search(r"filter(\d+)\.jaspar$", f) else -1
        out = []
        for f in sorted(files, key=lambda f: (num(f), f)):
            out.extend(read_jaspar(f))
        return out
    with open(path) as fh:
        text = fh.read(1 << 16)
    if re.search(r"^(MEME version|MOTIF\s)", text, re.M):
        return read_meme(path)
    return read_jaspar(path)


# ---------------------------------------------------------------- packing and the device call
def pack(motifs):
    """[(id, name, (w,4))] or [(w,4) arrays] -> ((M,wmax,4) float32 tensor, zero padded, int32 widths), on
    the host."""
    import torch
    mats = [np.asarray(m[2] if isinstance(m, tuple) else m, dtype=np.float64).reshape(-1, 4) for m in motifs]
    wmax = max([len(m) for m in mats] + [1])
    x = np.zeros((len(mats), wmax, 4), dtype=np.float32)
    for i, m in enumerate(mats):
        x[i, :len(m)] = m
    return torch.from_numpy(x), torch.tensor([len(m) for m in mats], dtype=torch.int32)


def _as_set(obj, device):
    """Anything compare accepts -> (float32 (M,w,4), int32 widths[M]) on `device`."""
    import torch
    widths = None
    if isinstance(obj, dict):                              # interpret.filter_pwms' result
        x = torch.as_tensor(np.asarray(obj["pfm"]))
        widths = (torch.as_tensor(np.asarray(obj["nsites"])) > 0).to(torch.int32) * x.shape[1]
    elif isinstance(obj, (tuple, list)) and len(obj) == 2 and torch.is_tensor(obj[0]) and obj[0].dim() == 3:
        x, widths = obj
    elif isinstance(obj, (list, tuple)):
        x, widths = pack(obj)
    else:
        x = torch.as_tensor(obj)
    if x.dim() != 3 or x.shape[2] != 4:
        raise ValueError("a motif set is (M, w, 4), rows A,C,G,T per column (got %s)" % (tuple(x.shape),))
    x = x.to(device=device, dtype=torch.float32).contiguous()
    if widths is None:                                     # a bare array: every motif w wide; a filter without
        widths = (x.reshape(len(x), -1).abs().sum(dim=1) > 0).to(torch.int32) * x.shape[1]   # a site is all zero
    widths = torch.as_tensor(widths).to(device=device, dtype=torch.int32).contiguous()
    if widths.shape != (len(x),):
        raise ValueError("widths must hold one entry per motif")
    return x, widths


def _pad(x, wmax):
    import torch
    if x.shape[1] == wmax:
        return x
    out = torch.zeros((x.shape[0], wmax, 4), dtype=x.dtype, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def _padded_sets(queries, targets, device):
    """Both sets on the device at one common wmax: (q, qw, t or None, tw or None, wmax)."""
    q, qw = _as_set(queries, device)
    t = tw = None
    if targets is not None:
        t, tw = _as_set(targets, device)
    wmax = max(q.shape[1], t.shape[1] if t is not None else 1, 1)
    if wmax > MAX_WIDTH:
        raise ValueError("motifs wider than %d columns are not supported (got %d)" % (MAX_WIDTH, wmax))
    return _pad(q, wmax), qw, (_pad(t, wmax) if t is not None else None), tw, wmax


def compare(queries, targets=None, min_overlap=5, pseudocount=0.0, both_strands=True, device=None):
    """The best alignment of every query with every target (targets=None: the queries with themselves).

    queries / targets: a list from read_meme / read_jaspar / read_motifs, a list of (w,4) arrays, pack()'s
    (tensor, widths), a (M,w,4) array or tensor (interpret.filter_pwms(...)["pfm"]: an all-zero matrix, a
    filter with nsites == 0, is given width 0) or filter_pwms' whole result.  Returns a MotifComparison of
    device tensors (Q,T): ncor and cor (float32), offset, strand, overlap (int16; views of one tensor).
    Enqueued on the current stream; no host synchronisation."""
    import torch

    from . import _lib
    if int(min_overlap) < 1:
        raise ValueError("min_overlap must be at least 1")
    if not float(pseudocount) >= 0:
        raise ValueError("pseudocount must not be negative")
    device = _lib.device_for(device, (queries, targets), "motifs.compare")
    q, qw, t, tw, wmax = _padded_sets(queries, targets, device)
    Q, T = len(q), len(t) if t is not None else len(q)
    ncor = torch.empty((Q, T), dtype=torch.float32, device=device)      # every entry is overwritten
    cor = torch.empty((Q, T), dtype=torch.float32, device=device)
    align = torch.empty((Q, T, 3), dtype=torch.int16, device=device)
    if Q and T:
        ws, nbytes = _lib.workspace("explainn_motif_compare_workspace_bytes", device, Q, T, wmax)
        _lib.call("explainn_motif_compare", device, q, qw, Q, t, tw, T, wmax, float(pseudocount), int(min_overlap),
                  int(bool(both_strands)), ncor, cor, align, ws, nbytes)
    return MotifComparison(ncor, cor, align[..., 0], align[..., 1], align[..., 2])


def benjamini_hochberg(pvalue):
    """(Q,T) p-values -> (Q,T) q-values, Benjamini-Hochberg over the T entries of each row:
    q_(k) = min_{j>=k} min(1, p_(j) T / j) with p sorted ascending (stable).  Plain torch, on the tensor's own
    device (host tensors too)."""
    import torch
    p = torch.as_tensor(pvalue)
    if p.dim() != 2:
        raise ValueError("benjamini_hochberg takes a (Q, T) matrix of p-values")
    T = p.shape[1]
    if T == 0 or p.shape[0] == 0:
        return p.clone()
    ps, order = torch.sort(p, dim=1, stable=True)
    rank = torch.arange(1, T + 1, dtype=p.dtype, device=p.device)
    adj = torch.clamp(ps * T / rank, max=1.0)
    adj = torch.flip(torch.cummin(torch.flip(adj, [1]), dim=1).values, [1])      # the minimum from the right
    return torch.empty_like(p).scatter_(1, order, adj)


def _significance_args(min_overlap, pseudocount, bins, workspace_bytes):
    if int(min_overlap) < 1:
        raise ValueError("min_overlap must be at least 1")
    if not float(pseudocount) >= 0:
        raise ValueError("pseudocount must not be negative")
    if int(bins) != bins or not 2 <= int(bins) <= MAX_BINS:
        raise ValueError("bins must be an integer in [2, %d] (got %r)" % (MAX_BINS, bins))
    if int(workspace_bytes) < 1:
        raise ValueError("workspace_bytes must be positive")


def _query_chunk(lib, Q, T, wmax, bins, both, budget):
    """The largest number of queries whose workspace fits `budget` bytes (at least 1)."""
    size = lambda n: int(lib.explainn_motif_significance_workspace_bytes(n, T, wmax, bins, both))
    if size(Q) <= budget:
        return Q
    lo, hi = 1, Q
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if size(mid) <= budget else (lo, mid - 1)
    return lo


def significance(queries, targets=None, min_overlap=5, pseudocount=0.0, both_strands=True, bins=100, device=None,
                 workspace_bytes=512 << 20):
    """The p-value of every query's best alignment with every target, and E- and q-values over the targets.

    The statistic of Gupta et al. 2007 -- Tomtom run with -incomplete-scores and Pearson columns: the score of
    an alignment is the sum over its overlap of the Pearson correlation of the aligned columns, quantised to
    `bins` steps; its null is what the same query columns score against columns drawn from the database (every
    column of every target, and of its reverse complement when both_strands; targets=None: the queries are the
    database, a query being part of its own null); the pair's p-value is that of its smallest alignment
    p-value after the Sidak step over the admissible alignments of the pair.  Two choices differ from the MEME
    program: the score range is fixed at [-1,1] and not rescaled to the observed range of each query (one pass,
    and the result is a function of the pair and the database alone), and both strands are counted in the
    Sidak exponent.  Tomtom's default complete-scores mode and its other column functions are not offered.

    Sets as for `compare`; strands, offsets, overlap and admissibility as there.  Every column inside a
    motif's width is a column of the database, also one without counts (a uniform column): a motif that is
    to stay out of the null has width 0.  Returns a MotifSignificance
    of device tensors (Q,T): pvalue, evalue (pvalue T), qvalue (Benjamini-Hochberg over the targets of each
    query), float64; offset, strand, overlap (int16, the alignment of the p-value) and score (int32, its
    quantised sum).  Everything after the quantisation is fp64; a p-value below the fp64 range is 0.
    workspace_bytes: the budget of device scratch; the queries are split into as many calls as it takes (one
    query per call when even that exceeds it) and the result does not depend on the split.  Enqueued on the
    current stream; no host synchronisation."""
    import torch

    from . import _lib
    _significance_args(min_overlap, pseudocount, bins, workspace_bytes)
    device = _lib.device_for(device, (queries, targets), "motifs.significance")
    q, qw, t, tw, wmax = _padded_sets(queries, targets, device)
    Q, T = len(q), len(t) if t is not None else len(q)
    both, bins = int(bool(both_strands)), int(bins)
    pvalue = torch.empty((Q, T), dtype=torch.float64, device=device)      # every entry is overwritten
    align = torch.empty((Q, T, 3), dtype=torch.int16, device=device)
    score = torch.empty((Q, T), dtype=torch.int32, device=device)
    if Q and T:
        step = _query_chunk(_lib.load(), Q, T, wmax, bins, both, int(workspace_bytes))
        if step < Q and t is None:                                       # the database is all of the queries
            t, tw = q, qw
        ws, nbytes = _lib.workspace("explainn_motif_significance_workspace_bytes", device, step, T, wmax, bins, both)
        for a in range(0, Q, step):
            n = min(step, Q - a)
            _lib.call("explainn_motif_significance", device, q[a:a + n], qw[a:a + n], n, t, tw, T, wmax,
                      float(pseudocount), int(min_overlap), both, bins, pvalue[a:a + n], align[a:a + n],
                      score[a:a + n], None, None, ws, nbytes)
    return MotifSignificance(pvalue, pvalue * T, benjamini_hochberg(pvalue), align[..., 0], align[..., 1],
                             align[..., 2], score)


# ---------------------------------------------------------------- reductions over the comparison
def _passing(result, min_ncor, min_cor):
    return (result.ncor >= min_ncor) & (result.cor >= min_cor)


def annotate(queries, database=None, top=3, min_ncor=0.4, min_cor=0.6, by="ncor", max_qvalue=0.05, **compare_args):
    """For each query up to `top` targets with Ncor >= min_ncor and cor >= min_cor, best Ncor first, ties to
    the lower target index: a list (one entry per query) of lists of dicts(target, ncor, cor, offset, strand,
    overlap).  `queries` may be a MotifComparison already computed (then `database` is not read).  The
    thresholds default to the lower bounds RSAT matrix-clustering is usually run with.

    by="pvalue": up to `top` targets with qvalue <= max_qvalue instead, smallest p-value first, ties to the
    lower target index; each hit also holds pvalue, evalue, qvalue and score, and its offset, strand and
    overlap are those of the p-value's alignment (ncor and cor stay the pair's best by Ncor, which may be
    another alignment; min_ncor and min_cor are not applied).  `queries` may be a MotifSignificance already
    computed; the hits then hold no ncor and cor.  Further arguments go to `compare` (and `significance`)."""
    import torch
    if by not in ("ncor", "pvalue"):
        raise ValueError("by must be 'ncor' or 'pvalue' (got %r)" % (by,))
    if by == "pvalue":
        if not 0 <= float(max_qvalue) <= 1:
            raise ValueError("max_qvalue must lie in [0, 1]")
        if isinstance(queries, MotifComparison):
            raise ValueError("by='pvalue' needs the motif sets or a MotifSignificance, not a MotifComparison")
        return _annotate_by_pvalue(queries, database, top, float(max_qvalue), compare_args)
    res = queries if isinstance(queries, MotifComparison) else compare(queries, database, **compare_args)
    Q, T = res.ncor.shape
    n = min(int(top), T)
    if n < 1 or Q == 0:
        return [[] for _ in range(Q)]
    score = torch.where(_passing(res, min_ncor, min_cor), res.ncor, torch.full_like(res.ncor, float("-inf")))
    val, idx = torch.sort(score, dim=1, descending=True, stable=True)
    val, idx = val[:, :n], idx[:, :n]
    pick = lambda a: torch.gather(a, 1, idx).cpu().numpy()
    val, idxh = val.cpu().numpy(), idx.cpu().numpy()
    cor, off, strand, ovl = pick(res.cor), pick(res.offset), pick(res.strand), pick(res.overlap)
    return [[dict(target=int(idxh[i, j]), ncor=float(val[i, j]), cor=float(cor[i, j]), offset=int(off[i, j]),
                  strand=int(strand[i, j]), overlap=int(ovl[i, j]))
             for j in range(n) if np.isfinite(val[i, j])] for i in range(Q)]


def _annotate_by_pvalue(queries, database, top, max_qvalue, args):
    import torch
    if isinstance(queries, MotifSignificance):
        sig, res = queries, None
    else:
        sig = significance(queries, database, **args)
        res = compare(queries, database, **{k: v for k, v in args.items() if k not in ("bins", "workspace_bytes")})
    Q, T = sig.pvalue.shape
    n = min(int(top), T)
    if n < 1 or Q == 0:
        return [[] for _ in range(Q)]
    key = torch.where(sig.qvalue <= max_qvalue, sig.pvalue, torch.full_like(sig.pvalue, float("inf")))
    val, idx = torch.sort(key, dim=1, stable=True)
    val, idx = val[:, :n], idx[:, :n]
    pick = lambda a: torch.gather(a, 1, idx).cpu().numpy()
    val, idxh = val.cpu().numpy(), idx.cpu().numpy()
    cols = {k: pick(getattr(sig, k)) for k in ("pvalue", "evalue", "qvalue", "offset", "strand", "overlap", "score")}
    if res is not None:
        cols.update(ncor=pick(res.ncor), cor=pick(res.cor))
    kind = dict(pvalue=float, evalue=float, qvalue=float, ncor=float, cor=float)
    return [[dict([("target", int(idxh[i, j]))] + [(k, kind.get(k, int)(v[i, j])) for k, v in cols.items()])
             for j in range(n) if np.isfinite(val[i, j])] for i in range(Q)]


def cluster(result, min_ncor=0.4, min_cor=0.6):
    """Single-linkage clusters of a self-comparison: the connected components of the pairs (either direction)
    with Ncor >= min_ncor and cor >= min_cor.  Returns (labels int64 [M], representatives int64 [C]): clusters
    are numbered 0.. in the order of their smallest member; a cluster's representative is the member with the
    largest summed Ncor to the members of its cluster, ties to the lower index."""
    import torch
    M = result.ncor.shape[0]
    if result.ncor.shape != (M, M):
        raise ValueError("cluster needs a self-comparison (M, M)")
    mask = _passing(result, min_ncor, min_cor)
    mask = mask | mask.T
    pairs = torch.nonzero(torch.triu(mask, diagonal=1)).cpu().numpy()
    parent = list(range(M))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b in pairs:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)          # the root is the smallest member
    roots = np.array([find(a) for a in range(M)], dtype=np.int64)
    order = {r: c for c, r in enumerate(sorted(set(roots.tolist())))}
    labels = np.array([order[r] for r in roots.tolist()], dtype=np.int64)
    lab = torch.from_numpy(labels).to(result.ncor.device)
    same = lab[:, None] == lab[None, :]
    total = torch.where(same, result.ncor, torch.zeros_like(result.ncor)).sum(dim=1).cpu().numpy()
    reps = np.zeros(len(order), dtype=np.int64)
    for c in range(len(order)):
        members = np.nonzero(labels == c)[0]
        reps[c] = members[np.argmax(total[members])]     # the first maximum: the lower index
    return labels, reps


def reproducibility(pfms, nsites=None, min_ncor=0.4, min_cor=0.6, result=None, **compare_args):
    """Which filters recur across the members of a model bank.  pfms: (G,U,k,4) count matrices, nsites: (G,U)
    (a filter with nsites == 0 matches nothing).  Returns (count int64 (G,U): the number of OTHER members that
    hold a filter passing both thresholds, partner int64 (G,U,G): the index of the best such filter in each
    member, by Ncor, ties to the lower index; -1 where there is none and for the member itself).  `result`: the
    comparison of the G*U filters (member-major) with themselves, when it has been computed already."""
    import torch
    pfms = np.asarray(pfms) if not torch.is_tensor(pfms) else pfms
    G, U = int(pfms.shape[0]), int(pfms.shape[1])
    if result is None:
        flat = torch.as_tensor(pfms).reshape(G * U, pfms.shape[2], 4)
        if nsites is not None:
            ns = torch.as_tensor(np.asarray(nsites)).reshape(G * U)
            result = compare((flat, (ns > 0).to(torch.int32) * flat.shape[1]), None, **compare_args)
        else:
            result = compare(flat, None, **compare_args)
    if result.ncor.shape != (G * U, G * U):
        raise ValueError("result must compare the %d filters with themselves" % (G * U))
    score = torch.where(_passing(result, min_ncor, min_cor), result.ncor,
                        torch.full_like(result.ncor, float("-inf"))).reshape(G, U, G, U)
    best = torch.argmax(score, dim=3)
    has = torch.isfinite(score.max(dim=3).values)
    has = has & ~torch.eye(G, dtype=torch.bool, device=has.device)[:, None, :]
    partner = torch.where(has, best, torch.full_like(best, -1))
    return has.sum(dim=2).cpu().numpy().astype(np.int64), partner.cpu().numpy().astype(np.int64)


# ---------------------------------------------------------------- motif tree and merged cluster motifs
LINKAGES = {"single": 0, "complete": 1, "average": 2}
TREE_SCALE = 1 << 20          # linkage values are Ncor quantised to 2^-20
MAX_LEAVES = 12288            # EXPLAINN_MOTIF_TREE_MAX_LEAVES: the per-slot cache of the tree kernel is in LDS


def _cut_threshold(min_ncor):
    """min_ncor on the tree's integer scale: a step is above the cut when sum >= threshold * pairs."""
    if not float(min_ncor) > 0:
        raise ValueError("min_ncor must be positive (got %r)" % (min_ncor,))
    return min(int(np.ceil(float(min_ncor) * TREE_SCALE)), (1 << 31) - 1)


class MotifTree:
    """The dendrogram of `tree`.  log int32 (M-1,8): lo, hi, leaves of the merged cluster, leaf_i, leaf_j, F, H,
    0 per step; link int64 (M-1,2): the linkage as (sum, pairs), height = sum / pairs / 2^20; gone int32 [M]: the
    step that merged slot c away (-1: never); flips, shifts int32 [M]: every leaf in the root's frame (meaningful
    as far as the steps had an overlap); widths int32 [M].  Tensors, on the device when `tree` made them."""

    def __init__(self, log, link, gone, flips, shifts, widths, linkage):
        self.log, self.link, self.gone, self.flips, self.shifts = log, link, gone, flips, shifts
        self.widths, self.linkage = widths, linkage

    @property
    def M(self):
        return int(self.widths.shape[0])

    @property
    def heights(self):
        """float64 [M-1] on the host: the linkage (an Ncor) at which each step merged; never increasing."""
        link = self.link.cpu().numpy()
        return link[:, 0].astype(np.float64) / link[:, 1].astype(np.float64) / TREE_SCALE

    def _nodes(self):
        """Per step the node ids (leaves 0..M-1, step t makes node M + t) of its two clusters."""
        log = self.log.cpu().numpy()
        node = list(range(self.M))
        out = np.zeros((len(log), 2), dtype=np.int64)
        for t, rec in enumerate(log):
            out[t] = node[rec[0]], node[rec[1]]
            node[rec[0]] = self.M + t
        return out, log

    def linkage_matrix(self):
        """The (M-1, 4) float64 matrix scipy.cluster.hierarchy.dendrogram draws: the two node ids, the distance
        1 - height, the leaves of the new node."""
        nodes, log = self._nodes()
        out = np.zeros((len(log), 4), dtype=np.float64)
        out[:, :2] = nodes
        out[:, 2] = 1.0 - self.heights
        out[:, 3] = log[:, 2]
        return out

    def newick(self, names=None):
        """The tree as Newick text, branch lengths in distance 1 - height; names default to the leaf numbers."""
        names = [str(i) for i in range(self.M)] if names is None else [re.sub(r"[\s():;,\[\]']", "_", str(n))
                                                                      for n in names]
        if len(names) != self.M:
            raise ValueError("newick needs one name per motif")
        if self.M == 0:
            return ";"
        log = self.log.cpu().numpy()
        dist = 1.0 - self.heights
        text, depth = list(names), [0.0] * self.M
        for t, rec in enumerate(log):
            lo, hi = int(rec[0]), int(rec[1])
            text[lo] = "(%s:%.6g,%s:%.6g)" % (text[lo], dist[t] - depth[lo], text[hi], dist[t] - depth[hi])
            depth[lo] = dist[t]
        return text[0] + ";"

    def _cut(self, min_ncor):
        import torch

        from . import _lib
        thr = _cut_threshold(min_ncor)
        dev = _lib.device_for(self.widths.device, (), "MotifTree.cut")
        M = self.M
        slots, flips, shifts, lo, hi = (torch.empty((M,), dtype=torch.int32, device=dev) for _ in range(5))
        if M:
            _lib.call("explainn_motif_tree_cut", dev, self.log, self.link, self.gone, self.widths, M, thr, slots,
                      flips, shifts, lo, hi)
        uniq, labels = torch.unique(slots, sorted=True, return_inverse=True)      # a slot is its smallest member
        spans = (hi - lo)[uniq.long()].cpu().numpy().astype(np.int32)             # the host synchronisation
        return labels.to(torch.int64), flips, shifts, spans, slots, uniq.to(torch.int32)

    def cut(self, min_ncor=0.4):
        """The clusters the steps with height >= min_ncor leave (min_ncor is taken on the tree's scale:
        ceil(min_ncor 2^20) / 2^20).  Returns (labels int64 [M], numbered 0.. in the order of the smallest member;
        flips, shifts int32 [M]: frame column shifts + c of a member's cluster holds column c of the member,
        reverse-complemented when flips is 1, the smallest shift of a cluster being 0 -- device tensors; spans
        int32 [C] on the host: the columns of each cluster's frame).  One host synchronisation."""
        return self._cut(min_ncor)[:4]


def tree(result, widths=None, linkage="average", max_bytes=2 << 30):
    """The agglomerative tree of a self-comparison (compare(motifs)): M - 1 merges of the two clusters with the
    largest linkage -- single (max), complete (min) or average Ncor over the leaf pairs, Ncor quantised to
    2^-20 so that every value is exact -- ties to the smaller slots (a cluster's slot is its smallest member).
    Only the upper triangle of `result` is read.  widths: int32 [M], the motif widths the placements need
    (default: the overlap of every motif with itself, which is its width unless it has no variance).  One
    workgroup runs the loop on the device (csrc/motiftree.hip); nothing is synchronised.  ValueError when the
    two M x M work matrices exceed max_bytes or M exceeds what the kernel holds."""
    import torch

    from . import _lib
    M = int(result.ncor.shape[0])
    if tuple(result.ncor.shape) != (M, M):
        raise ValueError("tree needs a self-comparison (M, M)")
    if linkage not in LINKAGES:
        raise ValueError("linkage must be one of %s (got %r)" % (", ".join(sorted(LINKAGES)), linkage))
    if M > 65535:
        raise ValueError("tree takes at most 65535 motifs: a leaf has 16 bits of the packed key (got %d)" % M)
    if 16 * M * M > int(max_bytes):
        raise ValueError("the two %d x %d work matrices take %d bytes, more than max_bytes = %d"
                         % (M, M, 16 * M * M, int(max_bytes)))
    if M > MAX_LEAVES:
        raise ValueError("tree takes at most %d motifs: the kernel caches one entry per slot in LDS (got %d)"
                         % (MAX_LEAVES, M))
    dev = _lib.device_for(result.ncor.device, (), "motifs.tree")
    ncor = result.ncor.to(torch.float32).contiguous()
    align = torch.stack([result.offset, result.strand, result.overlap], dim=-1).to(torch.int16).contiguous()
    if widths is None:
        widths = torch.diagonal(result.overlap)
    widths = torch.as_tensor(widths).to(device=dev, dtype=torch.int32).contiguous()
    if widths.shape != (M,):
        raise ValueError("widths must hold one entry per motif")
    log = torch.empty((max(M - 1, 0), 8), dtype=torch.int32, device=dev)
    link = torch.empty((max(M - 1, 0), 2), dtype=torch.int64, device=dev)
    gone, flips, shifts = (torch.empty((M,), dtype=torch.int32, device=dev) for _ in range(3))
    if M:
        kind = LINKAGES[linkage]
        ws, nbytes = _lib.workspace("explainn_motif_tree_workspace_bytes", dev, M, kind)
        _lib.call("explainn_motif_tree", dev, ncor, align, widths, M, kind, log, link, gone, flips, shifts, ws, nbytes)
    return MotifTree(log, link, gone, flips, shifts, widths, linkage)


_tree = tree                   # merge has a parameter of that name


def _column_ic(pfm):
    """Information content (bits) of count columns (.., 4); 0 for an empty column."""
    tot = pfm.sum(axis=-1, keepdims=True)
    p = np.where(tot > 0, pfm / np.where(tot > 0, tot, 1.0), 0.25)
    return 2.0 + np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0).sum(axis=-1)


class MergedMotifs:
    """The pooled motif of every cluster (`merge`), on the host.  pfm float64 (C, span_max, 4): per frame column
    the sum of the members' placed matrices; widths int32 [C]: the columns of each cluster; support int32
    (C, span_max): the members covering a column; labels int64 [M]; members: per cluster the member indices,
    ascending; flips, shifts int32 [M]: a member's placement in its cluster's frame; names: cluster<c>_n<size>;
    tree: the MotifTree that was cut."""

    def __init__(self, pfm, widths, support, labels, members, flips, shifts, names, tree=None):
        self.pfm, self.widths, self.support, self.labels, self.members = pfm, widths, support, labels, members
        self.flips, self.shifts, self.names, self.tree = flips, shifts, names, tree

    def __len__(self):
        return len(self.widths)

    def as_motifs(self):
        """[(name, "", (w, 4) float64 counts)]: what write_meme, compare, annotate, pwmsites.scan_motifs and
        pwmenrich.motif_enrichment take."""
        return [(self.names[c], "", self.pfm[c, :int(self.widths[c])].copy()) for c in range(len(self))]

    def trimmed(self, min_support=0.5, min_ic=0.0):
        """Cut the flanking columns that fewer than min_support of the cluster's members cover, or whose
        information content is below min_ic bits; inner columns stay.  A cluster without a column left has
        width 0.  Shifts are moved with the frame (a trimmed member's shift may become negative)."""
        if not 0 <= float(min_support) <= 1:
            raise ValueError("min_support must lie in [0, 1]")
        C = len(self)
        ic = _column_ic(self.pfm)
        left, widths = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=np.int32)
        for c in range(C):
            w = int(self.widths[c])
            ok = (self.support[c, :w] >= float(min_support) * len(self.members[c])) & (ic[c, :w] >= float(min_ic))
            keep = np.nonzero(ok)[0]
            if len(keep):
                left[c], widths[c] = keep[0], keep[-1] + 1 - keep[0]
        smax = int(widths.max()) if C else 0
        pfm = np.zeros((C, smax, 4), dtype=np.float64)
        support = np.zeros((C, smax), dtype=np.int32)
        for c in range(C):
            pfm[c, :widths[c]] = self.pfm[c, left[c]:left[c] + widths[c]]
            support[c, :widths[c]] = self.support[c, left[c]:left[c] + widths[c]]
        shifts = (np.asarray(self.shifts, dtype=np.int64) - left[np.asarray(self.labels, dtype=np.int64)]) \
            .astype(np.int32) if len(self.labels) else np.zeros(0, dtype=np.int32)
        return MergedMotifs(pfm, widths, support, self.labels, self.members, self.flips, shifts, self.names,
                            self.tree)


def merge(motifs, tree=None, min_ncor=0.4, linkage="average", device=None, **compare_args):
    """The non-redundant motifs of a set: cut the set's tree at min_ncor, place every member in its cluster's
    frame by the alignments `compare` found, and sum the placed count matrices per cluster (fp64, members in
    ascending order, on the device: the same bits on every run).  motifs: anything `compare` accepts; matrices
    are summed as given, so pre-scale them to weight them.  tree: a MotifTree of the same set (default:
    compare(motifs, **compare_args), then tree(..., linkage)).  Returns a MergedMotifs."""
    import torch

    from . import _lib
    _cut_threshold(min_ncor)
    device = _lib.device_for(device, (motifs,), "motifs.merge")
    x, w = _as_set(motifs, device)
    if x.shape[1] > MAX_WIDTH:
        raise ValueError("motifs wider than %d columns are not supported (got %d)" % (MAX_WIDTH, x.shape[1]))
    x = _pad(x, max(x.shape[1], 1))
    M, wmax = int(x.shape[0]), int(x.shape[1])
    if tree is None:
        tree = _tree(compare((x, w), None, device=device, **compare_args), w, linkage)
    if tree.M != M:
        raise ValueError("the tree holds %d motifs, the set %d" % (tree.M, M))
    w = torch.where((w < 0) | (w > wmax), torch.zeros_like(w), w)
    labels, flips, shifts, spans, slots, cluster_slots = tree._cut(min_ncor)
    n, smax = len(spans), (int(spans.max()) if len(spans) else 0)
    pfm = torch.empty((n, smax, 4), dtype=torch.float64, device=device)
    support = torch.empty((n, smax), dtype=torch.int32, device=device)
    if n and smax:
        _lib.call("explainn_motif_tree_pool", device, x, w, slots, flips, shifts, cluster_slots, M, wmax, n, smax, pfm,
                  support)
    labels = labels.cpu().numpy()
    members = [np.nonzero(labels == c)[0] for c in range(n)]
    names = ["cluster%d_n%d" % (c, len(m)) for c, m in enumerate(members)]
    return MergedMotifs(pfm.cpu().numpy(), spans, support.cpu().numpy(), labels, members, flips.cpu().numpy(),
                        shifts.cpu().numpy(), names, tree)


# ---------------------------------------------------------------- command line
def _cli_merge(a):
    motifs = []
    for path in a.motifs:
        motifs.extend(read_motifs(path))
    merged = merge(motifs, min_ncor=a.min_ncor, linkage=a.linkage, min_overlap=a.min_overlap,
                   pseudocount=a.pseudocount)
    out = merged.trimmed(a.min_support, a.min_ic)
    write_meme(a.output, out.as_motifs())
    if a.tree:
        with open(a.tree, "wt") as fh:
            fh.write(merged.tree.newick([m[0] for m in motifs]) + "\n")
    if a.table:
        with open(a.table, "wt") as fh:
            fh.write("Motif\tCluster\tStrand\tShift\tWidth\n")
            for i, (ident, _, m) in enumerate(motifs):
                fh.write("%s\t%s\t%s\t%d\t%d\n" % (ident, out.names[out.labels[i]], "-" if out.flips[i] else "+",
                                                   out.shifts[i], len(np.asarray(m).reshape(-1, 4))))


def _cli_annotate(a):
    queries, db = read_motifs(a.motifs), read_motifs(a.db)
    by_p = a.by == "pvalue"
    more = dict(by="pvalue", max_qvalue=a.max_qvalue, bins=a.bins) if by_p else {}
    hits = annotate(queries, db, top=a.top, min_ncor=a.min_ncor, min_cor=a.min_cor, min_overlap=a.min_overlap,
                    pseudocount=a.pseudocount, **more)
    with open(a.output, "wt") as fh:
        fh.write("Query\tTarget\tTargetName\tNcor\tCor\tOffset\tStrand\tOverlap%s\n"
                 % ("\tPvalue\tEvalue\tQvalue" if by_p else ""))
        for (qid, _, _), rows in zip(queries, hits):
            for h in rows:
                tid, tname, _ = db[h["target"]]
                fh.write("%s\t%s\t%s\t%.4f\t%.4f\t%d\t%s\t%d" % (qid, tid, tname, h["ncor"], h["cor"], h["offset"],
                                                               "-" if h["strand"] else "+", h["overlap"]))
                if by_p:
                    fh.write("\t%.3e\t%.3e\t%.3e" % (h["pvalue"], h["evalue"], h["qvalue"]))
                fh.write("\n")


def _cli_cluster(a):
    motifs = []
    for path in a.motifs:
        motifs.extend(read_motifs(path))
    res = compare(motifs, None, min_overlap=a.min_overlap, pseudocount=a.pseudocount)
    labels, reps = cluster(res, a.min_ncor, a.min_cor)
    with open(a.output, "wt") as fh:
        fh.write("Motif\tCluster\tRepresentative\n")
        for (ident, _, _), c in zip(motifs, labels):
            fh.write("%s\t%d\t%s\n" % (ident, c, motifs[reps[c]][0]))


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.motifs",
                                 description="Annotate and cluster motifs by Ncor or p-value on the device")
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("-o", "--output", required=True)
        p.add_argument("--min-ncor", type=float, default=0.4)
        p.add_argument("--min-cor", type=float, default=0.6)
        p.add_argument("--min-overlap", type=int, default=5)
        p.add_argument("--pseudocount", type=float, default=0.0)

    p = sub.add_parser("annotate", help="the best database motifs of every query motif")
    p.add_argument("motifs")
    p.add_argument("db")
    p.add_argument("--top", type=int, default=3)
    p.add_argument("--by", choices=("ncor", "pvalue"), default="ncor",
                   help="rank by Ncor (thresholds --min-ncor, --min-cor) or by p-value (threshold --max-qvalue)")
    p.add_argument("--max-qvalue", type=float, default=0.05)
    p.add_argument("--bins", type=int, default=100)
    common(p)
    p.set_defaults(run=_cli_annotate)
    p = sub.add_parser("cluster", help="single-linkage clusters of one or more motif sets")
    p.add_argument("motifs", nargs="+")
    common(p)
    p.set_defaults(run=_cli_cluster)
    p = sub.add_parser("merge", help="the merged motif of every cluster of a hierarchical tree")
    p.add_argument("motifs", nargs="+")
    p.add_argument("-o", "--output", required=True, help="the merged motifs, MEME text")
    p.add_argument("--linkage", choices=("average", "complete", "single"), default="average")
    p.add_argument("--min-ncor", type=float, default=0.4)
    p.add_argument("--min-overlap", type=int, default=5)
    p.add_argument("--pseudocount", type=float, default=0.0)
    p.add_argument("--min-support", type=float, default=0.5)
    p.add_argument("--min-ic", type=float, default=0.0)
    p.add_argument("--tree", help="write the tree as Newick text")
    p.add_argument("--table", help="write the placement of every motif: Motif Cluster Strand Shift Width")
    p.set_defaults(run=_cli_merge)
    a = ap.parse_args(argv)
    a.run(a)


if __name__ == "__main__":
    main()
