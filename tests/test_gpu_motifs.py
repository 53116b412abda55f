"""Motif comparison on the device (csrc/motifs.hip, explainn_amd.motifs) against tests/motifs_model.py.

Tolerance of ncor and cor against the fp64 model: the larger of 3x the error the model makes when it is run in
fp32 on the same case (the rule of tests/parity_util.py) and 1e-6 (a few fp32 ulps of 1: cor is bounded by 1
and is a sum of at most 256 products).  The alignment is checked through the model: the model's Ncor at the
device's (strand, offset) is within that tolerance of the model's maximum at every pair -- palindromes tie
exactly across strands and may land on either -- and where the model's best beats its runner-up by more than
1e-4 the device's (strand, offset) are the model's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import motifs_model as mm

pytestmark = pytest.mark.gpu

WIDTHS = (0, 1, 2, 4, 5, 19, 20, 33, 64)
SHAPES = ((1, 1), (1, 65), (63, 3), (65, 64), (130, 5))
Q_MAX, T_MAX = 130, 65
GUARD, FILL = 48, -7
DEPTH = 20                 # counts per column: the smallest non-zero column variance is 0.0045 (pc 1), above 1e-3


def _columns(rng, w):
    return np.stack([rng.multinomial(DEPTH, p) for p in rng.dirichlet([0.3] * 4, size=w)]).astype(np.float64) \
        if w else np.zeros((0, 4))


@functools.lru_cache(maxsize=None)
def _sets(wmax):
    """(queries, targets) as lists of (w,4) count matrices: random motifs of every width up to wmax, and the
    planted rows -- targets copy, reverse-complement and cut queries, so every tile holds some of each."""
    rng = np.random.default_rng(wmax)
    widths = [w for w in WIDTHS if w <= wmax]
    q = [_columns(rng, widths[i % len(widths)]) for i in range(Q_MAX)]
    t = [_columns(rng, widths[(i * 5 + 3) % len(widths)]) for i in range(T_MAX)]
    half = _columns(rng, wmax // 2)
    pal = np.concatenate([half, mm.revcomp(half)])
    full = _columns(rng, wmax)
    cut = max(1, wmax // 3)
    uniform = np.full((min(wmax, 5), 4), DEPTH / 4.0)
    mixed = full.copy()
    mixed[1::2] = DEPTH / 4.0                       # every other column uniform: windows without variance
    q[0], t[0] = full, full                          # an identical copy (also the (1,1) case)
    q[1], t[1] = full, mm.revcomp(full)              # a reverse-complement copy
    q[2], t[2] = pal, pal                            # a palindrome as a query and as a target
    q[3] = full[cut:]                                # a sub-motif cut from either end: best offsets > 0 and < 0
    q[4] = full[:wmax - cut]
    t[3], t[4] = full[cut:], full[:wmax - cut]
    q[5], t[5] = uniform, uniform                    # all-uniform columns
    q[6], t[6] = mixed, np.full((wmax, 4), 3.0)      # and a motif of equal counts
    q[62], t[63], t[64] = pal, full, mm.revcomp(full[cut:])      # planted rows at the tile edges too
    q[64], q[129] = mm.revcomp(full), full[cut:]
    return q, t


@functools.lru_cache(maxsize=None)
def _case(wmax, min_overlap, both, pc, probs=False):
    """Packed inputs, the fp64 model (every alignment and the best) and the tolerances, once per case; every
    (Q, T) of SHAPES is a slice, because a pair depends on its two motifs alone."""
    q, t = _sets(wmax)
    x, xw = mm.pack(q, wmax)
    y, yw = mm.pack(t, wmax)
    if probs:                                        # the same motifs as fp32 probabilities
        x, y = x / DEPTH, y / DEPTH
    al = mm.all_alignments(x, xw, y, yw, min_overlap, pc, both)
    # the variance floor decides nothing here: every window's SX, SY is exactly 0 or well above it
    for s in (al["sx"], al["sy"]):
        assert ((s == 0) | (s >= 1e-3)).all()
    best = mm.best_of(al)
    b32 = mm.best_of(mm.all_alignments(x, xw, y, yw, min_overlap, pc, both, dtype=np.float32))
    tol = {k: max(3.0 * float(np.abs(b32[k].astype(np.float64) - best[k]).max()), 1e-6) for k in ("ncor", "cor")}
    for a in (x, xw, y, yw):
        a.setflags(write=False)
    return x, xw, y, yw, al, best, tol


def _launch(x, xw, y, yw, wmax, min_overlap=5, both=True, pc=0.0, want=(True, True), shift=1, expect=0):
    """explainn_motif_compare through ctypes with every input at an odd element offset of its buffer and a
    guard band around every output; checks the bands and that the inputs are unchanged.  y None: self."""
    from explainn_amd import _lib
    lib = _lib.load()
    Q, T = len(xw), (len(yw) if y is not None else len(xw))

    def dev_in(a, dtype):
        buf = torch.full((shift + a.size,), 77, dtype=dtype, device="cuda")
        buf[shift:] = torch.tensor(np.asarray(a)).reshape(-1).cuda()
        return buf

    def dev_out(n, dtype):
        return torch.full((shift + n + GUARD,), FILL, dtype=dtype, device="cuda")

    ins = [dev_in(x, torch.float32), dev_in(xw, torch.int32)]
    if y is not None:
        ins += [dev_in(y, torch.float32), dev_in(yw, torch.int32)]
    before = [b.clone() for b in ins]
    ncor, cor, align = dev_out(Q * T, torch.float32), dev_out(Q * T, torch.float32), dev_out(Q * T * 3, torch.int16)
    nbytes = int(lib.explainn_motif_compare_workspace_bytes(Q, T, max(wmax, 1)))
    ws = torch.empty((nbytes + 16,), dtype=torch.uint8, device="cuda")
    ptr = lambda b, size: b.data_ptr() + shift * size
    rc = lib.explainn_motif_compare(
        ptr(ins[0], 4), ptr(ins[1], 4), Q, ptr(ins[2], 4) if y is not None else None,
        ptr(ins[3], 4) if y is not None else None, T, wmax, pc, min_overlap, int(both), ptr(ncor, 4),
        ptr(cor, 4) if want[0] else None, ptr(align, 2) if want[1] else None, ws.data_ptr(), nbytes,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == expect, lib.explainn_last_error()
    torch.cuda.synchronize()
    for b, b0 in zip(ins, before):
        assert torch.equal(b, b0), "an input changed"
    written = (True,) + tuple(want) if rc == 0 else (False, False, False)
    for buf, n, w in ((ncor, Q * T, written[0]), (cor, Q * T, written[1]), (align, Q * T * 3, written[2])):
        inside = buf[shift:shift + n]
        assert (buf[:shift] == FILL).all() and (buf[shift + n:] == FILL).all(), "write outside an output"
        assert w or (inside == FILL).all(), "an output that was not asked for was written"
    return (ncor[shift:shift + Q * T].reshape(Q, T).cpu().numpy(),
            cor[shift:shift + Q * T].reshape(Q, T).cpu().numpy() if want[0] else None,
            align[shift:shift + Q * T * 3].reshape(Q, T, 3).cpu().numpy().astype(np.int64) if want[1] else None)


def _check(got, al, best, tol, Q, T, what):
    ncor, cor, align = got
    want_n, want_c = best["ncor"][:Q, :T], best["cor"][:Q, :T]
    err_n, err_c = np.abs(ncor - want_n).max(), np.abs(cor - want_c).max()
    print("%s: |ncor - model| %.2e (tol %.2e), |cor - model| %.2e (tol %.2e)" % (what, err_n, tol["ncor"], err_c,
                                                                              tol["cor"]))
    assert np.isfinite(ncor).all() and np.isfinite(cor).all()
    assert err_n <= tol["ncor"], what
    assert err_c <= tol["cor"], what
    o, s, w = align[..., 0], align[..., 1], align[..., 2]
    found = best["found"][:Q, :T]
    assert not ncor[~found].any() and not cor[~found].any() and not align[~found].any(), what
    assert ((s == 0) | (s == 1)).all()
    wmax = (len(al["offsets"]) + 1) // 2
    assert (np.abs(o) < wmax).all()
    qi, ti = np.nonzero(found)
    j = o[qi, ti] + wmax - 1
    assert al["adm"][qi, ti, s[qi, ti], j].all(), what + ": an alignment that is not admissible"
    at_dev = al["ncor"][qi, ti, s[qi, ti], j]
    assert (np.abs(at_dev - want_n[qi, ti]) <= tol["ncor"]).all(), what + ": not a best alignment"
    assert np.array_equal(w[qi, ti], al["w"][qi, ti, s[qi, ti], j]), what
    clear = found & (want_n - best["runner_up"][:Q, :T] > 1e-4)
    assert np.array_equal(o[clear], best["offset"][:Q, :T][clear]), what
    assert np.array_equal(s[clear], best["strand"][:Q, :T][clear]), what
    return clear.mean()


@pytest.mark.parametrize("pc", [0.0, 1.0])
@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("min_overlap", [1, 5, 70])
@pytest.mark.parametrize("wmax", [19, 33, 64])
def test_device_equals_model(wmax, min_overlap, both, pc):
    x, xw, y, yw, al, best, tol = _case(wmax, min_overlap, both, pc)
    for Q, T in SHAPES:
        got = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax, min_overlap, both, pc)
        clear = _check(got, al, best, tol, Q, T, "wmax %d mo %d both %d pc %g (%d,%d)" % (wmax, min_overlap, both, pc,
                                                                                         Q, T))
    assert clear > 0.25                             # the exact comparison of (strand, offset) covered many pairs


def test_planted_rows():
    wmax = 19
    x, xw, y, yw, al, best, tol = _case(wmax, 5, True, 0.0)
    ncor, cor, align = _launch(x, xw, y, yw, wmax)
    cut = wmax // 3
    assert abs(ncor[0, 0] - 1) <= 1e-6 and align[0, 0].tolist() == [0, 0, wmax]          # identical
    assert abs(ncor[1, 1] - 1) <= 1e-6 and align[1, 1].tolist() == [0, 1, wmax]          # reverse complement
    assert abs(ncor[2, 2] - 1) <= 1e-6 and align[2, 2, 0] == 0 and align[2, 2, 2] == 2 * (wmax // 2)   # palindrome
    assert abs(cor[3, 0] - 1) <= 1e-6 and align[3, 0].tolist() == [cut, 0, wmax - cut]    # cut from the front
    assert abs(cor[0, 3] - 1) <= 1e-6 and align[0, 3].tolist() == [-cut, 0, wmax - cut]
    assert abs(cor[4, 0] - 1) <= 1e-6 and align[4, 0].tolist() == [0, 0, wmax - cut]      # cut from the back
    assert abs(cor[129, 64] - 1) <= 1e-6 and align[129, 64, 1] == 1
    assert not ncor[5].any() and not ncor[:, 5].any() and not ncor[:, 6].any()            # no variance: cor 0
    assert align[5, 5].tolist() == [0, 0, 5]           # the first admissible alignment of a pair without variance
    zero = np.nonzero(xw == 0)[0]
    assert len(zero) and not ncor[zero].any() and not align[zero].any()


def test_probabilities_and_counts_agree():
    """The same motifs as fp32 probabilities: the model is rebuilt from those very numbers."""
    wmax = 33
    x, xw, y, yw, al, best, tol = _case(wmax, 5, True, 0.0, probs=True)
    got = _launch(x[:65], xw[:65], y[:64], yw[:64], wmax)
    _check(got, al, best, tol, 65, 64, "probabilities")


def test_optional_outputs_determinism_and_alignment_of_buffers():
    wmax = 33
    x, xw, y, yw, al, best, tol = _case(wmax, 5, True, 0.0)
    Q, T = 65, 64
    full = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax)
    again = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    for want in ((False, False), (True, False), (False, True)):
        part = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax, want=want)
        assert np.array_equal(part[0].view(np.uint32), full[0].view(np.uint32))
        assert part[1] is None or np.array_equal(part[1], full[1])
        assert part[2] is None or np.array_equal(part[2], full[2])
    aligned = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax, shift=0)
    assert all(np.array_equal(a, b) for a, b in zip(full, aligned))


def test_self_comparison():
    wmax = 19
    q, _ = _sets(wmax)
    x, xw = mm.pack(q, wmax)
    me = _launch(x, xw, None, None, wmax)
    two = _launch(x, xw, x, xw, wmax)
    assert all(np.array_equal(a, b) for a, b in zip(me, two))
    al = mm.all_alignments(x, xw, x, xw, 5, 0.0, True)
    best = mm.best_of(al)
    b32 = mm.best_of(mm.all_alignments(x, xw, x, xw, 5, 0.0, True, dtype=np.float32))
    tol = {k: max(3.0 * float(np.abs(b32[k].astype(np.float64) - best[k]).max()), 1e-6) for k in ("ncor", "cor")}
    _check(me, al, best, tol, len(x), len(x), "self")
    assert np.abs(me[0] - me[0].T).max() <= tol["ncor"]
    wide = np.nonzero(xw > 0)[0]
    assert (np.abs(me[0][wide, wide] - 1) <= 1e-6).all() or (me[0][wide, wide] == 0).any()


def test_bad_widths_are_width_zero():
    wmax = 19
    x, xw, y, yw, al, best, tol = _case(wmax, 5, True, 0.0)
    bad, zero = xw[:63].copy(), xw[:63].copy()
    bad[0], bad[7], zero[0], zero[7] = -1, wmax + 1, 0, 0
    a = _launch(x[:63], bad, y[:3], yw[:3], wmax)
    b = _launch(x[:63], zero, y[:3], yw[:3], wmax)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert not a[0][0].any() and not a[0][7].any() and a[0][1].any()


def test_argument_errors():
    from explainn_amd import _lib
    wmax = 19
    x, xw, y, yw, al, best, tol = _case(wmax, 5, True, 0.0)
    a = (x[:3], xw[:3], y[:5], yw[:5])
    _launch(*a, wmax, min_overlap=0, expect=_lib.E_ARG)
    _launch(*a, wmax, pc=-1.0, expect=_lib.E_ARG)
    _launch(*a, 0, expect=_lib.E_ARG)
    _launch(*a, 65, expect=_lib.E_UNSUPPORTED)
    _launch(x[:3], xw[:3], None, None, wmax, expect=_lib.OK)
    lib = _lib.load()
    z = torch.zeros(64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = z.data_ptr()
    assert lib.explainn_motif_compare(p, p, -1, p, p, 2, 4, 0.0, 5, 1, p, None, None, p, 256, s) == _lib.E_ARG
    assert lib.explainn_motif_compare(p, p, 2, p, p, -1, 4, 0.0, 5, 1, p, None, None, p, 256, s) == _lib.E_ARG
    assert lib.explainn_motif_compare(p, p, 2, None, None, 3, 4, 0.0, 5, 1, p, None, None, p, 256, s) == _lib.E_ARG
    assert lib.explainn_motif_compare(p, p, 2, p, p, 2, 4, 0.0, 5, 1, p, None, None, p, 16, s) == _lib.E_ARG   # workspace
    assert lib.explainn_motif_compare(p, p, 0, p, p, 2, 4, 0.0, 5, 1, p, None, None, None, 0, s) == _lib.OK     # nothing to do
    assert lib.explainn_motif_compare(p, p, 2, p, p, 0, 4, 0.0, 5, 1, p, None, None, None, 0, s) == _lib.OK
    torch.cuda.synchronize()
    assert not z.any()
    got = _launch(*a, wmax)                          # the next good call still works
    _check(got, al, best, tol, 3, 5, "after errors")


# ---- the Python layer on a planted bank-like set ----
G, U, K = 3, 5, 19


@functools.lru_cache(maxsize=None)
def _bank():
    rng = np.random.default_rng(77)
    pfm = np.stack([[np.stack([rng.multinomial(100, p) for p in rng.dirichlet([0.3] * 4, size=K)])
                     for _ in range(U)] for _ in range(G)]).astype(np.int64)
    a = pfm[0, 1].copy()                             # planted in all three members
    pfm[1, 4] = mm.revcomp(a)
    pfm[2, 0, :3], pfm[2, 0, 3:] = 25, a[:-3]        # shifted by three columns
    b = pfm[0, 3].copy()                             # planted in two
    pfm[2, 2] = mm.revcomp(b)
    nsites = np.full((G, U), 100, dtype=np.int64)
    pfm[1, 0], nsites[1, 0] = 0, 0                   # a filter without a site
    return pfm, nsites


def test_python_layer():
    from explainn_amd import motifs
    pfm, nsites = _bank()
    flat = pfm.reshape(G * U, K, 4)
    res = motifs.compare(flat)
    assert res.ncor.is_cuda and tuple(res.ncor.shape) == (G * U, G * U) and res.offset.dtype == torch.int16
    x, xw = mm.pack([m if n else m[:0] for m, n in zip(flat, nsites.reshape(-1))], K)
    best = mm.compare(x, xw)
    assert np.abs(res.ncor.cpu().numpy() - best["ncor"]).max() <= 1e-5
    # the same through every accepted form of a set
    lst = [("filter%d" % i, "bank", m) for i, m in enumerate(flat)]
    for other in (motifs.compare(lst), motifs.compare(motifs.pack(lst)), motifs.compare(torch.from_numpy(flat).cuda()),
                  motifs.compare(dict(pfm=flat, nsites=nsites.reshape(-1))), motifs.compare(lst, lst)):
        assert torch.equal(other.ncor, res.ncor) and torch.equal(other.strand, res.strand)
    assert not res.ncor[U].any() and not res.ncor[:, U].any()          # nsites == 0: width 0
    a = [1, U + 4, 2 * U]
    assert res.strand[1, U + 4] == 1 and res.offset[1, 2 * U] == 3 and res.overlap[1, 2 * U] == K - 3
    assert res.offset[2 * U, 1] == -3 and abs(float(res.cor[1, 2 * U]) - 1) <= 1e-6

    count, partner = motifs.reproducibility(pfm, nsites)
    want = np.zeros((G, U), dtype=np.int64)
    want[0, 1] = want[1, 4] = want[2, 0] = 2
    want[0, 3] = want[2, 2] = 1
    assert np.array_equal(count, want)
    assert partner[0, 1].tolist() == [-1, 4, 0] and partner[1, 4].tolist() == [1, -1, 0]
    assert partner[2, 0].tolist() == [1, 4, -1] and partner[0, 3].tolist() == [-1, -1, 2]
    assert partner[2, 2].tolist() == [3, -1, -1] and (partner[1, 0] == -1).all()
    c2, p2 = motifs.reproducibility(pfm, nsites, result=res)
    assert np.array_equal(c2, count) and np.array_equal(p2, partner)

    labels, reps = motifs.cluster(res)
    assert labels[a[0]] == labels[a[1]] == labels[a[2]] and labels[3] == labels[2 * U + 2] != labels[1]
    assert len(set(labels.tolist())) == G * U - 3 and len(reps) == G * U - 3
    assert reps[labels[1]] in (1, U + 4)              # the two unshifted copies tie up to rounding
    assert all(labels[r] == c for c, r in enumerate(reps))

    hits = motifs.annotate(lst[:U], lst[U:], top=2)
    assert [h["target"] for h in hits[1]] == [4, U] and hits[1][0]["strand"] == 1 and hits[1][1]["offset"] == 3
    assert [h["target"] for h in hits[3]] == [U + 2] and hits[0] == [] and hits[2] == []
    assert hits[1][0]["ncor"] >= hits[1][1]["ncor"]
    empty = motifs.compare(lst[:0], lst)
    assert tuple(empty.ncor.shape) == (0, G * U)
    with pytest.raises(ValueError):
        motifs.compare([np.ones((65, 4))])


def test_command_line(tmp_path):
    import os
    from explainn_amd import motifs
    from explainn_amd.interpret import format_jaspar
    pfm, nsites = _bank()
    os.makedirs(os.path.join(tmp_path, "motifs"))
    for u in range(U):
        with open(os.path.join(tmp_path, "motifs", "filter%d.jaspar" % u), "w") as fh:
            fh.write(format_jaspar(pfm[0, u], "filter%d" % u, "m0"))
    db = os.path.join(tmp_path, "db.meme")
    motifs.write_meme(db, [("T%d" % i, "name%d" % i, m) for i, m in enumerate(pfm[1:].reshape(-1, K, 4)) if m.any()])
    out = os.path.join(tmp_path, "ann.tsv")
    motifs.main(["annotate", os.path.join(tmp_path, "motifs"), db, "-o", out])
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert rows[0] == ["Query", "Target", "TargetName", "Ncor", "Cor", "Offset", "Strand", "Overlap"]
    assert [r[:3] for r in rows[1:]] == [["filter1", "T4", "name4"], ["filter1", "T5", "name5"],
                                         ["filter3", "T7", "name7"]]
    assert rows[1][6] == "-" and rows[2][5:] == ["3", "+", str(K - 3)]
    out = os.path.join(tmp_path, "clu.tsv")
    motifs.main(["cluster", os.path.join(tmp_path, "motifs"), db, "-o", out])
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert rows[0] == ["Motif", "Cluster", "Representative"] and len(rows) == 1 + U + 2 * U - 1
    by = {r[0]: r[1:] for r in rows[1:]}
    assert by["filter1"] == by["T4"] == by["T5"] and by["filter3"] == by["T7"] and by["filter1"][1] in ("filter1", "T4")
