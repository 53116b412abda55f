"""Numpy model of the haplotype windows explainn_stage_haplotype_windows stages (DESIGN.md section 8,
"Haplotypes"): the haplotype is BUILT piece by piece (np.concatenate) and sliced with N padding --
deliberately not the kernel's prefix-sum index arithmetic.  tests/test_haplotypes_cpu.py checks the table
builder of explainn_amd/variants.py against it, tests/test_gpu_haplotypes.py the device."""
import numpy as np

NONE = np.zeros(0, dtype=np.uint8)


def haplotype_window(seq, start, edits, L):
    """L bases from `start` (haplotype coordinates, signed) of seq with every (pos, ref_len, alt) of
    `edits` -- ordered, non-overlapping -- spliced in; outside the haplotype N, bytes above 4 N."""
    seq = np.asarray(seq, dtype=np.uint8)
    pieces, at = [], 0
    for pos, ref_len, alt in edits:
        assert pos >= at, "the model takes an ordered, non-overlapping run"
        pieces += [seq[at:pos], np.asarray(alt, dtype=np.uint8)]
        at = pos + ref_len
    pieces.append(seq[at:])
    hap = np.concatenate(pieces)
    out = np.full(L, 4, dtype=np.uint8)
    lo, hi = max(start, 0), min(start + L, len(hap))
    if hi > lo:
        out[lo - start:hi - start] = hap[lo:hi]
    out[out > 4] = 4
    return out


def row_run(tab, b):
    """The (pos, ref_len, alt) list of row b of explainn_haplotypes' fields, in list order; None for a
    run the entry points must refuse (the whole row N, flag bit 0)."""
    first, count = int(tab["row_first"][b]), int(tab["row_count"][b])
    if count < 0 or first < 0 or first + count > len(tab["edit_index"]):
        return None
    run, end = [], None
    for e in tab["edit_index"][first:first + count]:
        e = int(e)
        if e < 0 or e >= len(tab["pos"]):
            return None
        pos, rl, al, ao = (int(tab[f][e]) for f in ("pos", "ref_len", "alt_len", "alt_off"))
        if rl < 0 or al < 0 or ao < 0 or ao + al > len(tab["alt"]) or (end is not None and pos < end):
            return None
        run.append((pos, rl, tab["alt"][ao:ao + al]))
        end = pos + rl
    return run


def tables_matrix(seq, tab, L, rows=None):
    """The (rows, L) code matrix the tables describe: an interpreter of the table fields on top of
    haplotype_window."""
    out = []
    for b in (range(len(tab["row_start"])) if rows is None else rows):
        run = row_run(tab, b)
        out.append(np.full(L, 4, np.uint8) if run is None else
                   haplotype_window(seq, int(tab["row_start"][b]), run, L))
    return np.stack(out) if out else np.zeros((0, L), dtype=np.uint8)


def dense_run(rng, p0, n):
    """n edits from p0 on, one or two bases apart (so some abut): SNVs and 1-base insertions and
    deletions in turn."""
    run, p = [], p0
    for i in range(n):
        kind = i % 3
        if kind == 0:
            run.append((p, 1, rng.integers(0, 4, size=1).astype(np.uint8)))
        elif kind == 1:
            run.append((p, 0, rng.integers(0, 4, size=1).astype(np.uint8)))
        else:
            run.append((p, 1, NONE))
        p += 1 + int(rng.integers(0, 2))
    return run


def run_cases(seq, L, seed=0):
    """The runs the staging kernel must get right, as (start, [(pos, ref_len, alt), ...]) rows; start in
    the coordinates of the row's own haplotype.  seq must be at least 5 L long and L >= 30."""
    rng = np.random.default_rng(seed)
    N = len(seq)
    assert N >= 5 * L and L >= 30 and N >= 700

    def bases(n):
        return rng.integers(0, 4, size=n).astype(np.uint8)

    c = N // 2
    long_alt = [(c - 30, 1, bases(1)), (c, 2, bases(L + 17)), (c + 10, 1, bases(1))]
    cases = [
        (c - 40, []),                                                   # run length 0: the reference window
        (c - L // 2, [(c, 1, bases(1))]),                               # 1: SNV
        (c - L // 2, [(c, 0, bases(4))]),                               # 1: insertion
        (c - L // 2, [(c, 6, NONE)]),                                   # 1: deletion
        (c - 20, [(c, 1, bases(1)), (c + 9, 1, bases(1))]),             # 2
        (c - 20, [(c, 2, bases(2)), (c + 2, 1, bases(1))]),             # abutting edits
        (c - 20, [(c, 3, NONE), (c + 3, 0, bases(2))]),                 # a deletion abutting an insertion
        (c - 20, [(c, 0, bases(3)), (c, 0, bases(2))]),                 # two insertions at one position
        (c - 30, [(c - 20, 0, bases(5)), (c, 4, NONE), (c + 15, 1, bases(1))]),   # 3: insertion + deletion + SNV
        (c + 28, [(c, 3, bases(8)), (c + 40, 1, bases(1))]),            # wholly left (+5) and one inside
        (c + 20, [(c, 9, NONE), (c + 12, 0, bases(2)), (c + 50, 2, bases(2))]),   # two wholly left (-9, +2)
        (c - 40, long_alt),                                             # alt_len > L mid-run: from before it
        (c + 5, long_alt),                                              # ... the window inside the alt run
        (c + L + 17 - 10, long_alt),                                    # ... its end and the edit behind it
        (c - 62, [(c, 2, bases(5)), (c + 61, 3, bases(4))]),            # across q = 63/64 and q = 127/128
        (c - 63, [(c, 0, bases(1)), (c + 64, 1, bases(1))]),            # an insertion that ends at q = 64; q = 128
        (c, [(c, 1, bases(1)), (c + L - 1, 1, bases(1))]),              # edits at q = 0 and q = L-1
        (c, [(c, 0, bases(2)), (c + L - 3, 5, NONE)]),                  # insertion at q = 0, deletion at q = L-1
        (c - 10, [(c, 1, bases(1)), (c + L + 50, 1, bases(1)), (c + L + 90, 0, bases(3))]),   # extends right
        (c - L - 5, [(c, 2, bases(7)), (c + 5, 1, bases(1))]),          # wholly right: the reference row
        (-15, [(3, 0, bases(9)), (20, 1, bases(1))]),                   # N padding at the sequence start
        (-L - 3, [(5, 1, bases(1)), (9, 1, bases(1))]),                 # a window wholly before the sequence
        (N - L + 12, [(N - 30, 1, bases(1)), (N - 12, 2, bases(1))]),   # N padding at the sequence end
        (N - L // 2, [(N - 40, 1, bases(1)), (N - 20, 15, NONE)]),      # a deletion past the window, to seq_len - 5
        (N - 20 - L // 2, [(N - 40, 0, bases(2)), (N - 20, 25, NONE)]),  # a deletion that runs past seq_len
        (c - 10, [(c, 1, np.array([4], np.uint8)), (c + 5, 2, np.array([0, 4, 2], np.uint8))]),   # N inside alt
    ]
    # both sides of the 64-edit chunk and a third chunk; the runs begin left of the window
    for n, back in ((63, 30), (64, 30), (65, 30), (130, 60), (130, 150)):
        cases.append((c, dense_run(rng, c - back, n)))
    ns = np.flatnonzero(np.asarray(seq) == 4)
    assert ns.size, "the sequence needs an N run"
    at = int(ns[len(ns) // 2])
    cases.append((at - L // 2, [(max(at - 9, 0), 2, bases(6)), (at, 1, bases(1))]))
    return cases


def tables_from_runs(cases, B, first=0):
    """explainn_haplotypes' fields (numpy) of B rows that cycle through `cases` from case `first`: every
    edit of every row gets a record of its own, in a shuffled edit table -- so edit_index never runs in
    table order -- and the rows' runs lie in edit_index in reverse row order."""
    rows = [cases[(first + i) % len(cases)] for i in range(B)]
    edits = [e for _, run in rows for e in run]
    order = np.random.default_rng(B).permutation(len(edits))
    slot = np.empty(len(edits), dtype=np.int64)
    slot[order] = np.arange(len(edits))
    table = [edits[i] for i in order]
    alt_len = np.array([len(a) for _, _, a in table], dtype=np.int64)
    runs, j = [], 0
    for _, run in rows:
        runs.append(slot[j:j + len(run)])
        j += len(run)
    row_first, at = np.zeros(B, dtype=np.int64), 0
    for b in reversed(range(B)):
        row_first[b] = at
        at += len(runs[b])
    return {"row_start": np.array([s for s, _ in rows], dtype=np.int64),
            "row_first": row_first,
            "row_count": np.array([len(r) for r in runs], dtype=np.int32),
            "edit_index": np.concatenate(runs[::-1] + [np.zeros(0, np.int64)]).astype(np.int32),
            "pos": np.array([p for p, _, _ in table], dtype=np.int64),
            "ref_len": np.array([r for _, r, _ in table], dtype=np.int32),
            "alt_len": alt_len.astype(np.int32),
            "alt_off": (np.cumsum(alt_len) - alt_len).astype(np.int32),
            "alt": np.concatenate([a for _, _, a in table] + [NONE]).astype(np.uint8)}


def cases_matrix(seq, cases, B, L, first=0):
    """The same rows built case by case, without any table."""
    return np.stack([haplotype_window(seq, *cases[(first + i) % len(cases)], L) for i in range(B)])


def carried_window(seq, start, pos, ref_len, alts, carried, L):
    """The window at `start` (reference coordinates) of the haplotype that carries the variants
    `carried`: those with pos >= start, spliced in by position (stable).  A variant left of the window
    start does not move it, and one that straddles it is left out."""
    idx = sorted((int(i) for i in carried if pos[int(i)] >= start), key=lambda i: int(pos[i]))
    return haplotype_window(seq, int(start), [(int(pos[i]), int(ref_len[i]), alts[i]) for i in idx], L)


def spaced_variants(seq, n, seed=0, gap=12):
    """n variants of one sequence that never overlap (at least `gap` bases between their starts, REF
    alleles of at most 6): SNVs, 1-10-base insertions and 1-6-base deletions.  (pos, ref_len, alts)."""
    rng = np.random.default_rng(seed)
    N = len(seq)
    pos = np.sort(rng.choice(np.arange(2, (N - 8) // gap), size=n, replace=False)) * gap + rng.integers(0, gap - 6, n)
    ref_len, alts = [], []
    for i in range(n):
        rl, al = [(1, 1), (0, int(rng.integers(1, 11))), (int(rng.integers(1, 7)), 0)][i % 3]
        ref_len.append(rl)
        alts.append(rng.integers(0, 4, size=al).astype(np.uint8))
    return pos.astype(np.int64), np.array(ref_len, dtype=np.int64), alts
