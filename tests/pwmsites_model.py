"""Numpy model of known-motif sites (csrc/pwmsites.hip, explainn_amd/pwmsites.py).

Written from the contract in include/explainn_hip.h, not from the package: quantised tables, the exact null
by column-by-column convolution (and, independently, by enumerating every w-mer), tails, thresholds, and a
brute-force scan of both strands with N and a record period.  Everything is fp64 / integer numpy."""
import itertools

import numpy as np

MAX_WIDTH, MAX_BINS = 64, 128


def uniform():
    return np.full(4, 0.25)


def quantise(mats, bg=None, pc=0.1, bins=100):
    """(S int16 (M,wmax,4), widths, scale, lo): cell by cell as the issue states it.  Empty (width 0 or
    hi == lo): scale 0."""
    bg = uniform() if bg is None else np.asarray(bg, dtype=np.float64)
    wmax = max([len(m) for m in mats] + [1])
    S = np.zeros((len(mats), wmax, 4), dtype=np.int16)
    widths = np.array([len(m) for m in mats], dtype=np.int32).reshape(len(mats))
    scale, lo = np.zeros(len(mats)), np.zeros(len(mats))
    for i, m in enumerate(mats):
        m = np.asarray(m, dtype=np.float64).reshape(-1, 4)
        if not len(m):
            continue
        l = np.zeros((len(m), 4))
        for j in range(len(m)):
            tot = m[j].sum()
            col = m[j] / tot if tot > 0 else np.full(4, 0.25)
            for a in range(4):
                l[j, a] = np.log2((col[a] + pc * bg[a]) / (1 + pc) / bg[a])
        if l.max() == l.min():
            continue
        lo[i], scale[i] = l.min(), bins / (l.max() - l.min())
        S[i, :len(m)] = np.rint((l - lo[i]) * scale[i])
    return S, widths, scale, lo


def live_widths(widths, scale):
    """The widths as the device takes them: 0 for an empty motif."""
    return np.where(np.asarray(scale) > 0, widths, 0).astype(np.int32)


def null_pdf(Sm, bg, bins):
    """pdf (w bins + 1,) of the score of a random w-mer: pdf_new[s] = sum_a bg[a] pdf_old[s - S[j][a]], a in
    order."""
    w = len(Sm)
    pdf = np.zeros(w * bins + 1)
    pdf[0] = 1.0
    for j in range(w):
        new = np.zeros_like(pdf)
        top = j * bins + 1                      # the live range of pdf_old
        for a in range(4):
            s = int(Sm[j][a])
            new[s:s + top] += bg[a] * pdf[:top]
        pdf = new
    return pdf


def enumerated_pdf(Sm, bg, bins):
    """The same by definition: every one of the 4^w w-mers, its probability added at its score (math.fsum per
    score would be the gold standard; w <= 6 keeps plain accumulation within 1e-16)."""
    w = len(Sm)
    pdf = np.zeros(w * bins + 1)
    for kmer in itertools.product(range(4), repeat=w):
        s, p = 0, 1.0
        for j, a in enumerate(kmer):
            s += int(Sm[j][a])
            p *= bg[a]
        pdf[s] += p
    return pdf


def tail_of(pdf):
    return np.cumsum(pdf[::-1])[::-1]


def threshold_of(tail, pcut):
    """The smallest s with tail[s] <= pcut; len(tail) = w bins + 1 if there is none."""
    ok = np.flatnonzero(tail <= pcut)
    return int(ok[0]) if len(ok) else len(tail)


def null_table(S, lwidths, bins, bg, pcut):
    """(tail float64 (M, wmax bins + 2), thresholds int32 (M,)) as explainn_pwm_null writes them."""
    M, wmax = S.shape[0], S.shape[1]
    tail = np.zeros((M, wmax * bins + 2))
    thr = np.ones(M, dtype=np.int32)
    for m in range(M):
        w = int(lwidths[m])
        if not 1 <= w <= wmax:
            continue
        t = tail_of(null_pdf(S[m, :w], bg, bins))
        tail[m, :len(t)] = t
        thr[m] = threshold_of(t, pcut)
    return tail, thr


def min_relative_gap(tail, lwidths, bins, pcut):
    """The smallest |tail / pcut - 1| over the motifs' own score ranges: how far every tail value stays from
    the cutoff (a threshold is safe against rounding when this is far above the rounding error)."""
    gap = np.inf
    for m in range(len(tail)):
        w = int(lwidths[m])
        if w >= 1:
            gap = min(gap, float(np.abs(tail[m, :w * bins + 1] / pcut - 1.0).min()))
    return gap


def rc_codes(codes):
    c = np.asarray(codes)[::-1]
    return np.where(c < 4, 3 - c, c).astype(np.uint8)


def scan(S, lwidths, thr, codes, start=0, n_positions=None, period=0, both=True):
    """(offsets int64 (2M+1), pos int32 start-relative, iscore int32) as explainn_pwm_sites lists them: row
    2m = '+', 2m+1 = '-', each in ascending position."""
    codes = np.minimum(np.asarray(codes, dtype=np.int64), 4)
    M, wmax = S.shape[0], S.shape[1]
    n_positions = len(codes) - start if n_positions is None else n_positions
    end = min(start + n_positions + wmax - 1, len(codes))
    pos, isc, counts = [], [], []
    for m in range(M):
        w = int(lwidths[m])
        for strand in (1, -1):
            hits, vals = np.zeros(0, np.int64), np.zeros(0, np.int64)
            if 1 <= w <= wmax and (strand > 0 or both) and end - start >= w:
                p = np.arange(start, min(start + n_positions, end - w + 1))        # the windows that fit
                win = np.lib.stride_tricks.sliding_window_view(codes[:end], w)[p]   # (n, w): one window per row
                live = ~np.any(win >= 4, axis=1)
                if period > 0:
                    live &= p % period <= period - w
                p, win = p[live], win[live]
                if strand < 0:
                    win = 3 - win[:, ::-1]                                          # its reverse complement
                s = S[m, np.arange(w)[None, :], win].astype(np.int64).sum(axis=1)
                hits, vals = p[s >= thr[m]] - start, s[s >= thr[m]]
            pos += hits.tolist()
            isc += vals.tolist()
            counts.append(len(hits))
    offsets = np.zeros(2 * M + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return offsets, np.array(pos, dtype=np.int32), np.array(isc, dtype=np.int32)


def calls(mats, codes, pcut, bg=None, pc=0.1, bins=100, both=True, period=0):
    """What scan_motifs returns, as a dict: offsets (M+1), start, strand, iscore, score (float32), pvalue,
    widths."""
    bg = uniform() if bg is None else np.asarray(bg, dtype=np.float64)
    S, widths, scale, lo = quantise(mats, bg, pc, bins)
    lw = live_widths(widths, scale)
    tail, thr = null_table(S, lw, bins, bg, pcut)
    off2, pos, isc = scan(S, lw, thr, codes, period=period, both=both)
    M = len(mats)
    row = np.repeat(np.arange(2 * M), np.diff(off2))
    unit = row // 2
    score = (isc / scale[unit] + widths[unit] * lo[unit]).astype(np.float32) if len(unit) else np.zeros(0, np.float32)
    return dict(offsets=off2[::2].copy(), start=pos.astype(np.int64), strand=(1 - 2 * (row % 2)).astype(np.int8),
                iscore=isc, score=score, pvalue=tail[unit, isc] if len(unit) else np.zeros(0), widths=widths,
                unit=unit, thresholds=thr, tail=tail)


def sequence_background(codes, both=True):
    n = np.array([np.sum(np.asarray(codes) == a) for a in range(4)], dtype=np.float64)
    if both:
        n = n + n[::-1]
    return n / n.sum()


def bed_rows(seq_id, c, names):
    """`SeqId start end name score strand pvalue`, sorted by (start, motif, strand), '+' first."""
    keys = sorted(range(len(c["start"])), key=lambda i: (c["start"][i], c["unit"][i], -c["strand"][i]))
    return ["%s\t%d\t%d\t%s\t%.6g\t%s\t%.6g\n" % (
        seq_id, c["start"][i], c["start"][i] + c["widths"][c["unit"][i]], names[c["unit"][i]], c["score"][i],
        "+" if c["strand"][i] > 0 else "-", c["pvalue"][i]) for i in keys]


# ---------------------------------------------------------------- inputs the tests share
def dirichlet_motifs(widths, seed, alpha=0.3):
    g = np.random.default_rng(seed)
    return [g.dirichlet(np.full(4, alpha), size=w).reshape(w, 4) for w in widths]


def random_codes(n, seed, n_frac=0.01):
    g = np.random.default_rng(seed)
    c = g.integers(0, 4, size=n).astype(np.uint8)
    c[g.random(n) < n_frac] = 4
    return c


def consensus(m):
    return np.argmax(np.asarray(m), axis=1).astype(np.uint8)


def plant(codes, m, at, reverse=False):
    """The motif's consensus (or its reverse complement) written into codes at `at`."""
    word = consensus(m)
    codes[at:at + len(word)] = rc_codes(word) if reverse else word
    return codes
