"""Numpy model of the edited windows explainn_stage_edited_windows stages (DESIGN.md section 8,
"Variant effects"): the haplotype is BUILT (np.concatenate) and sliced with N padding -- deliberately
not the kernel's per-position index arithmetic.  tests/test_variants_cpu.py checks the row-table
builder of explainn_amd/variants.py against it, tests/test_gpu_variants.py the device."""
import numpy as np

import scan_model as sm


def edited_window(seq, start, pos, ref_len, alt, L):
    """L bases from `start` (haplotype coordinates, signed) of seq with seq[pos : pos+ref_len] replaced
    by alt; outside the haplotype N, bytes above 4 N."""
    seq = np.asarray(seq, dtype=np.uint8)
    hap = np.concatenate((seq[:pos], np.asarray(alt, dtype=np.uint8), seq[pos + ref_len:]))
    out = np.full(L, 4, dtype=np.uint8)
    lo, hi = max(start, 0), min(start + L, len(hap))
    if hi > lo:
        out[lo - start:hi - start] = hap[lo:hi]
    out[out > 4] = 4
    return out


def edited_matrix(seq, row_start, row_edit, pos, ref_len, alt_len, alt_off, alt, L):
    """The (rows, L) code matrix of a row table and an edit table (explainn_edits' fields)."""
    rows = []
    none = np.zeros(0, dtype=np.uint8)
    for s, e in zip(row_start, row_edit):
        if e < 0:
            rows.append(edited_window(seq, int(s), 0, 0, none, L))
        else:
            a = np.asarray(alt)[int(alt_off[e]):int(alt_off[e]) + int(alt_len[e])]
            rows.append(edited_window(seq, int(s), int(pos[e]), int(ref_len[e]), a, L))
    return np.stack(rows) if rows else np.zeros((0, L), dtype=np.uint8)


def centred(pos, ref_len, alt_len, L, shift=0):
    """The window start the issue defines (restated, not imported)."""
    return pos - (L - max(ref_len, alt_len)) // 2 + shift


def edit_cases(seq, L, seed=0):
    """The edit classes the staging kernel must get right, as (start, edit) rows: edit None or
    (pos, ref_len, alt).  seq must be at least 5 L long and hold an N run (sm.random_codes(n_runs=...))."""
    rng = np.random.default_rng(seed)
    N = len(seq)
    assert N >= 5 * L and L >= 30

    def bases(n):
        return rng.integers(0, 4, size=n).astype(np.uint8)

    def mid(pos, ref_len, alt):
        return centred(pos, ref_len, len(alt), L), (pos, ref_len, alt)

    c = N // 2
    cases = [
        mid(c + 1, 1, bases(70)),                       # alt_len 70 -> ref_len 1
        (c - 40, None),                                 # no edit
        mid(c, 1, bases(1)),                            # SNV
        mid(c + 3, 3, bases(3)),                        # MNV
        mid(c + 5, 0, bases(5)),                        # insertion, ref_len 0
        mid(c + 7, 4, bases(0)),                        # deletion, alt_len 0
        mid(c + 9, 30, bases(2)),                       # ref_len 30 -> alt_len 2
        mid(c + 11, 2, bases(L + 17)),                  # alt_len > L, the window inside the alt run
        (c + 11 - 5, (c + 11, 2, bases(L + 17))),       # ... starting before it
        (c + 11 + 3, (c + 11, 2, bases(L + 30))),       # ... and straddling the window start with alt beyond the end
        (c, (c, 1, bases(1))),                          # edit at q = 0
        (c - L + 1, (c, 1, bases(1))),                  # edit at q = L-1
        (c, (c, 0, bases(3))),                          # insertion at q = 0
        (c - L + 1, (c, 5, bases(0))),                  # deletion that starts at q = L-1
        (c + 4, (c, 6, bases(10))),                     # straddles the window start: pos < start < pos + alt_len
        (c - L + 4, (c, 6, bases(10))),                 # straddles the window end
        (c + 8 + 20, (c, 3, bases(8))),                 # wholly left of the window: coordinates shift by +5
        (c + 20, (c, 9, bases(0))),                     # wholly left, a deletion: shift by -9
        (c - L - 5, (c, 2, bases(7))),                  # wholly right of the window: the reference row
        (c - 62, (c, 2, bases(5))),                     # crosses q = 63/64
        (c - 126, (c, 5, bases(4))),                    # crosses q = 127/128
        (c - 63, (c, 0, bases(2))),                     # insertion that ends at q = 64
        mid(10, 1, bases(1)),                           # within L/2 of the sequence start: N padding on the left
        mid(N - 12, 2, bases(1)),                       # ... of the end: N padding on the right
        mid(3, 0, bases(9)), mid(N - 2, 2, bases(6)),
        mid(N - 20, 15, bases(0)),                      # a deletion whose right flank runs past seq_len
        mid(N - 6, 6, bases(0)),                        # a deletion of the sequence's last bases
        (-L - 3, (5, 1, bases(1))),                     # a window wholly before the sequence
        mid(c + 20, 2, np.array([0, 4, 2], np.uint8)),  # an N inside alt
    ]
    ns = np.flatnonzero(np.asarray(seq) == 4)
    assert ns.size, "the sequence needs an N run"
    at = int(ns[len(ns) // 2])
    cases += [mid(at, 1, bases(1)), mid(max(at - 3, 0), 2, bases(6)), (at - L // 2, None)]
    return cases


def tables_from_cases(cases, B, first=0):
    """Row and edit tables (explainn_edits' fields, numpy) of B rows that cycle through `cases` from
    case `first`: every row with an edit gets an edit record of its own, in a shuffled edit table."""
    rows = [cases[(first + i) % len(cases)] for i in range(B)]
    edits = [e for _, e in rows if e is not None]
    order = np.random.default_rng(B).permutation(len(edits))            # edit table order != row order
    slot = np.empty(len(edits), dtype=np.int64)
    slot[order] = np.arange(len(edits))
    table = [edits[i] for i in order]
    alt_len = np.array([len(a) for _, _, a in table], dtype=np.int64)
    row_edit, j = [], 0
    for _, e in rows:
        if e is None:
            row_edit.append(-1)
        else:
            row_edit.append(int(slot[j]))
            j += 1
    return {"row_start": np.array([s for s, _ in rows], dtype=np.int64),
            "row_edit": np.array(row_edit, dtype=np.int32),
            "pos": np.array([p for p, _, _ in table], dtype=np.int64),
            "ref_len": np.array([r for _, r, _ in table], dtype=np.int32),
            "alt_len": alt_len.astype(np.int32),
            "alt_off": (np.cumsum(alt_len) - alt_len).astype(np.int32),
            "alt": np.concatenate([a for _, _, a in table] + [np.zeros(0, np.uint8)]).astype(np.uint8)}


def cases_matrix(seq, cases, B, L, first=0):
    """The same rows built case by case, without any table."""
    none = np.zeros(0, dtype=np.uint8)
    out = []
    for i in range(B):
        s, e = cases[(first + i) % len(cases)]
        out.append(edited_window(seq, s, *(e if e is not None else (0, 0, none)), L))
    return np.stack(out)


def mixed_variants(seq, n, L, seed=0):
    """n variants of one sequence: SNVs, MNVs, insertions, deletions, replacements; some close to the
    ends; two multi-allelic sites (same pos and ref, different alts).  Returns (pos, ref_len, alts)."""
    rng = np.random.default_rng(seed)
    N = len(seq)
    pos, ref_len, alts = [], [], []
    for i in range(n):
        kind = i % 5
        rl, al = [(1, 1), (3, 3), (0, int(rng.integers(1, 11))), (int(rng.integers(1, 11)), 0),
                  (int(rng.integers(1, 31)), int(rng.integers(1, 80)))][kind]
        if i % 7 == 0:
            p = int(rng.integers(0, L // 2))
        elif i % 7 == 1:
            p = N - rl - int(rng.integers(0, L // 2))
        else:
            p = int(rng.integers(0, N - rl + 1))
        pos.append(p); ref_len.append(rl)
        alts.append(rng.integers(0, 4, size=al).astype(np.uint8))
    for i in (2, 3):                                                     # multi-allelic: a second alt
        pos[-i], ref_len[-i] = pos[i], ref_len[i]
        alts[-i] = rng.integers(0, 4, size=len(alts[i]) + 1).astype(np.uint8)
    return np.array(pos, dtype=np.int64), np.array(ref_len, dtype=np.int64), alts


def allele_matrices(seq, pos, ref_len, alts, L, shifts):
    """(ref, alt) code matrices (V*S, L) of the windows score_variants scores, variant-major."""
    none = np.zeros(0, dtype=np.uint8)
    ref, alt = [], []
    for p, r, a in zip(pos, ref_len, alts):
        for s in shifts:
            st = centred(int(p), int(r), len(a), L, s)
            ref.append(edited_window(seq, st, 0, 0, none, L))
            alt.append(edited_window(seq, st, int(p), int(r), a, L))
    return np.stack(ref), np.stack(alt)


def oracle_effects(orc, sd, ref_mat, alt_mat, V, S, dtype=np.float64):
    """The fp64 oracle's (units (V,U,T), delta (V,T), logits dict) on the materialised windows: units =
    (outs_alt - outs_ref) * final.weight averaged over the two strands and the S shifts, delta = the
    same average of the logit difference."""
    W = np.asarray(sd["final.weight"], dtype=dtype)                      # (T,U)
    o, lg = {}, {}
    for name, mat in (("ref", ref_mat), ("alt", alt_mat)):
        for strand, m in (("fwd", mat), ("rev", sm.rc_rows(mat))):
            x = sm.onehot(m)
            o[name, strand] = np.asarray(orc.unit_outputs(sd, x, dtype=dtype))
            lg[name, strand] = np.asarray(orc.forward(sd, x, dtype=dtype))
    d = ((o["alt", "fwd"] - o["ref", "fwd"]) + (o["alt", "rev"] - o["ref", "rev"])) / 2
    d = d.reshape(V, S, -1).mean(axis=1)
    units = d[:, :, None] * W.T[None]
    dl = ((lg["alt", "fwd"] + lg["alt", "rev"]) / 2 - (lg["ref", "fwd"] + lg["ref", "rev"]) / 2)
    return units, dl.reshape(V, S, -1).mean(axis=1), lg
