"""Motif significance on the device (csrc/motifs.hip explainn_motif_significance, explainn_amd.motifs) against
tests/motifsig_model.py, stage by stage.

  column scores   equal to the fp64 model's, except where the model's unrounded value lies within 1e-3 bin
                  units of a rounding boundary (+-1 there); such pairs are at most 1 % of all
  histograms      the bincount of the device's own column scores, exactly
  p-values        the model is run on the device's own column scores, so everything after the rounding is
                  integer work or fp64 sums of positive terms: the score at the device's alignment equals the
                  model's, the p-value is within 1e-10 relative of the model's there ((number of additions)
                  2^-53 is at most (64 130 + 8193) 2^-53 = 2e-12) and no larger than the model's minimum times
                  (1 + 1e-10); where the model's runner-up p_align exceeds its best by more than 1e-6 relative
                  the alignment is the model's, which must cover more than half of the pairs.
The motif sets are those of tests/test_gpu_motifs.py (20 counts per column, planted copies, reverse complements,
cuts, palindromes and uniform columns at the tile edges)."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import motifs_model as mm
import motifsig_model as sm
from test_gpu_motifs import FILL, GUARD, SHAPES, G, K, U, _bank, _sets

pytestmark = pytest.mark.gpu

OUTPUTS = ("align", "score", "colscore", "hist")


@functools.lru_cache(maxsize=None)
def _packed(wmax):
    q, t = _sets(wmax)
    x, xw = mm.pack(q, wmax)
    y, yw = mm.pack(t, wmax)
    for a in (x, xw, y, yw):
        a.setflags(write=False)
    return x, xw, y, yw


def _launch(x, xw, y, yw, wmax, min_overlap=5, both=True, pc=0.0, bins=100, want=OUTPUTS, shift=1, expect=0,
            short=0):
    """explainn_motif_significance through ctypes with every input at an odd element offset of its buffer and a
    guard band around every output; checks the bands and that the inputs are unchanged.  y None: self."""
    from explainn_amd import _lib
    lib = _lib.load()
    Q, T = len(xw), (len(yw) if y is not None else len(xw))
    S = 2 if both else 1
    w1, nb = max(wmax, 1), max(bins, 0) + 1

    def dev_in(a, dtype):
        buf = torch.full((shift + a.size,), 77, dtype=dtype, device="cuda")
        buf[shift:] = torch.tensor(np.asarray(a)).reshape(-1).cuda()
        return buf

    def dev_out(n, dtype):
        return torch.full((shift + n + GUARD,), FILL % 256 if dtype == torch.uint8 else FILL, dtype=dtype, device="cuda")

    ins = [dev_in(x, torch.float32), dev_in(xw, torch.int32)]
    if y is not None:
        ins += [dev_in(y, torch.float32), dev_in(yw, torch.int32)]
    before = [b.clone() for b in ins]
    sizes = dict(pvalue=(Q * T, torch.float64, 8), align=(Q * T * 3, torch.int16, 2), score=(Q * T, torch.int32, 4),
                 colscore=(Q * w1 * S * w1 * T, torch.uint8, 1), hist=(Q * w1 * nb, torch.int32, 4))
    out = {k: dev_out(n, dt) for k, (n, dt, _) in sizes.items()}
    nbytes = int(lib.explainn_motif_significance_workspace_bytes(Q, T, wmax, bins, int(both)))
    ws = torch.empty((max(nbytes, 16) + 16,), dtype=torch.uint8, device="cuda")
    ptr = lambda b, size: b.data_ptr() + shift * size
    arg = lambda k: ptr(out[k], sizes[k][2]) if k == "pvalue" or k in want else None
    rc = lib.explainn_motif_significance(
        ptr(ins[0], 4), ptr(ins[1], 4), Q, ptr(ins[2], 4) if y is not None else None,
        ptr(ins[3], 4) if y is not None else None, T, wmax, pc, min_overlap, int(both), bins, arg("pvalue"),
        arg("align"), arg("score"), arg("colscore"), arg("hist"), ws.data_ptr(), nbytes - short,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == expect, lib.explainn_last_error()
    torch.cuda.synchronize()
    for b, b0 in zip(ins, before):
        assert torch.equal(b, b0), "an input changed"
    res = {}
    for k, (n, dt, _) in sizes.items():
        buf, fill = out[k], (FILL % 256 if dt == torch.uint8 else FILL)
        assert (buf[:shift] == fill).all() and (buf[shift + n:] == fill).all(), "write outside " + k
        if rc == 0 and (k == "pvalue" or k in want):
            res[k] = buf[shift:shift + n].cpu().numpy()
        else:
            assert (buf[shift:shift + n] == fill).all(), k + " was not asked for and was written"
            res[k] = None
    if rc != 0:
        return None
    res["pvalue"] = res["pvalue"].reshape(Q, T)
    if res["align"] is not None:
        res["align"] = res["align"].reshape(Q, T, 3).astype(np.int64)
    if res["score"] is not None:
        res["score"] = res["score"].reshape(Q, T).astype(np.int64)
    if res["colscore"] is not None:
        res["colscore"] = res["colscore"].reshape(Q, w1, S, w1, T)
    if res["hist"] is not None:
        res["hist"] = res["hist"].reshape(Q, w1, nb).astype(np.int64)
    return res


def _check_colscore(got, x, xw, y, yw, pc, both, bins, what):
    """Stage 1 against the fp64 model.  Returns the share of pairs near a rounding boundary."""
    want, raw = sm.column_scores(x, xw, y, yw, pc, both, bins)
    valid = want != sm.NONE
    assert np.array_equal(got == sm.NONE, ~valid), what + ": the columns that exist"
    if not valid.any():
        return 0.0
    edge = raw[valid] + 0.5
    near = np.abs(edge - np.rint(edge)) <= 1e-3
    diff = got[valid].astype(np.int64) - want[valid].astype(np.int64)
    print("%s: %d column pairs, %.3f %% within 1e-3 of a boundary, %d differ from the model" % (
        what, valid.sum(), 100 * near.mean(), (diff != 0).sum()))
    assert not diff[~near].any(), what + ": a column score differs away from a rounding boundary"
    assert (np.abs(diff) <= 1).all(), what
    assert near.mean() <= 0.01, what
    assert got[valid].max() <= bins
    return float(near.mean())


def _check(got, x, xw, y, yw, wmax, min_overlap, pc, both, bins, what):
    """Stages 1 to 3 of one launch.  Returns (share of pairs compared exactly, the model)."""
    if y is None:
        y, yw = x, xw
    Q, T = len(xw), len(yw)
    _check_colscore(got["colscore"], x, xw, y, yw, pc, both, bins, what)
    assert np.array_equal(got["hist"], sm.histograms(got["colscore"], bins)), what + ": histograms"
    m = sm.significance(x, xw, y, yw, min_overlap, pc, both, bins, colscore=got["colscore"])
    p, o, s, w = got["pvalue"], got["align"][..., 0], got["align"][..., 1], got["align"][..., 2]
    found = m["found"]
    assert np.isfinite(p).all() and (p >= 0).all() and (p <= 1).all(), what
    assert (p[~found] == 1).all() and not got["align"][~found].any() and not got["score"][~found].any(), what
    assert ((s == 0) | (s == 1)).all() and (np.abs(o) < wmax).all()
    qi, ti = np.nonzero(found)
    if len(qi) == 0:
        return 1.0, m
    j = o[qi, ti] + wmax - 1
    at = (qi, ti, s[qi, ti], j)
    assert m["adm"][at].all(), what + ": an alignment that is not admissible"
    assert np.array_equal(got["score"][qi, ti], m["score_all"][at]), what + ": score"
    assert np.array_equal(w[qi, ti], m["w_all"][at]), what + ": overlap"
    there = sm.sidak(m["p_all"][at], m["n_align"][qi, ti])
    rel = np.abs(p[qi, ti] - there) / np.maximum(there, 1e-300)
    over = p[qi, ti] / np.maximum(m["pvalue"][qi, ti], 1e-300) - 1
    print("%s: p-value against the model at the device's alignment: %.2e relative; above the model's minimum "
          "by at most %.2e relative; smallest p %.2e" % (what, rel.max(), over.max(), p[qi, ti].min()))
    assert (rel <= 1e-10).all(), what + ": p-value"
    assert (p[qi, ti] <= m["pvalue"][qi, ti] * (1 + 1e-10)).all(), what + ": not a best alignment"
    clear = found & (m["runner_up"] > m["p_align"] * (1 + 1e-6))
    for k, mine in (("offset", o), ("strand", s), ("overlap", w)):
        assert np.array_equal(mine[clear], m[k][clear]), what + ": " + k
    return float(clear[found].mean()), m


CASES = [(19, 100, 5, True), (19, 16, 1, False), (19, 128, 1, True), (19, 100, 1, False),
         (33, 100, 5, True), (33, 16, 1, True), (33, 128, 5, False)]


@pytest.mark.parametrize("wmax,bins,min_overlap,both", CASES)
def test_device_equals_model(wmax, bins, min_overlap, both):
    x, xw, y, yw = _packed(wmax)
    exact = pairs = 0
    for Q, T in SHAPES:
        what = "wmax %d bins %d mo %d both %d (%d,%d)" % (wmax, bins, min_overlap, both, Q, T)
        got = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax, min_overlap, both, 0.0, bins)
        clear, m = _check(got, x[:Q], xw[:Q], y[:T], yw[:T], wmax, min_overlap, 0.0, both, bins, what)
        exact += clear * m["found"].sum()
        pairs += m["found"].sum()
    print("the alignment was compared exactly on %.1f %% of the pairs" % (100.0 * exact / pairs))
    assert exact > 0.5 * pairs                          # the exact comparison of the alignment covered most pairs


@pytest.mark.parametrize("Q,T", [(1, 1), (4, 65)])
def test_widest_motifs_and_most_bins(Q, T):
    """wmax 64 x bins 128: the largest pmf (8193 entries), the largest LDS footprint of every kernel."""
    wmax, bins = 64, 128
    x, xw, y, yw = _packed(wmax)
    got = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax, 5, True, 1.0, bins)
    _check(got, x[:Q], xw[:Q], y[:T], yw[:T], wmax, 5, 1.0, True, bins, "wmax 64 bins 128 pc 1 (%d,%d)" % (Q, T))
    assert got["align"][0, 0].tolist() == [0, 0, wmax] and got["score"][0, 0] == wmax * bins
    assert 0 <= got["pvalue"][0, 0] < 1e-15


@pytest.mark.parametrize("bins", [16, 100, 128])
def test_fp32_restatement_of_the_column_score(bins):
    """What the device's arithmetic (fp32 unit columns, three fused multiply-adds) can move: the unrounded value
    by at most 2e-5 bin units, and no score away from a rounding boundary."""
    wmax = 33
    x, xw, y, yw = _packed(wmax)
    want, raw = sm.column_scores(x, xw, y, yw, 0.0, True, bins)
    uq, _, _ = sm._units(x, xw, 0.0)
    ut, rt, _ = sm._units(y, yw, 0.0)
    views = np.stack([ut, rt]).astype(np.float32)
    c32 = np.einsum("qia,stja->qisjt", uq.astype(np.float32), views).astype(np.float32)
    raw32 = (c32 + np.float32(1)) * np.float32(bins / 2.0)
    valid = want != sm.NONE
    moved = np.abs(raw32.astype(np.float64) - raw)[valid].max()
    print("bins %d: the fp32 restatement moves the unrounded value by at most %.2e" % (bins, moved))
    assert moved <= 2e-5
    edge = raw[valid] + 0.5
    far = np.abs(edge - np.rint(edge)) > 1e-3
    b32 = np.clip(np.floor(raw32 + np.float32(0.5)), 0, bins).astype(np.int64)
    assert np.array_equal(b32[valid][far], want[valid][far].astype(np.int64))


def test_planted_rows():
    wmax, bins = 19, 100
    x, xw, y, yw = _packed(wmax)
    r = _launch(x, xw, y, yw, wmax, bins=bins)
    p, align, score = r["pvalue"], r["align"], r["score"]
    cut = wmax // 3
    assert align[0, 0].tolist() == [0, 0, wmax] and p[0, 0] < 1e-15 and score[0, 0] == wmax * bins     # identical
    assert align[1, 1].tolist() == [0, 1, wmax] and p[1, 1] < 1e-15                                   # reverse complement
    assert align[2, 2, 0] == 0 and align[2, 2, 2] == 2 * (wmax // 2) and p[2, 2] < 1e-15              # palindrome
    assert align[3, 0].tolist() == [cut, 0, wmax - cut] and p[3, 0] < 1e-10                           # cut from the front
    assert align[0, 3].tolist() == [-cut, 0, wmax - cut] and p[0, 3] < 1e-10
    assert align[4, 0].tolist() == [0, 0, wmax - cut] and p[4, 0] < 1e-10                             # cut from the back
    assert align[129, 64, 1] == 1 and p[129, 64] < 1e-10
    zero = np.nonzero(xw == 0)[0]
    assert len(zero) and (p[zero] == 1).all() and not align[zero].any() and not score[zero].any()
    tz = np.nonzero(yw == 0)[0]
    assert len(tz) and (p[:, tz] == 1).all() and not align[:, tz].any()
    # all-uniform motifs: every column score sits at bins / 2, and the result is finite
    cs = r["colscore"]
    assert (cs[5, :5][cs[5, :5] != sm.NONE] == bins // 2).all() and (cs[0, 0, :, :5, 5] == bins // 2).all()
    assert (cs[:, :, :, :, 6][cs[:, :, :, :, 6] != sm.NONE] == bins // 2).all()
    assert np.isfinite(p[5]).all() and np.isfinite(p[:, 5]).all() and np.isfinite(p[:, 6]).all()
    assert (score[5, yw > 0] == align[5, yw > 0, 2] * (bins // 2)).all()


def test_bad_widths_are_width_zero():
    wmax = 19
    x, xw, y, yw = _packed(wmax)
    bad, zero = xw[:63].copy(), xw[:63].copy()
    bad[0], bad[7], zero[0], zero[7] = -1, wmax + 1, 0, 0
    tbad, tzero = yw[:3].copy(), yw[:3].copy()
    tbad[1], tzero[1] = 99, 0
    a = _launch(x[:63], bad, y[:3], tbad, wmax)
    b = _launch(x[:63], zero, y[:3], tzero, wmax)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert (a["pvalue"][0] == 1).all() and (a["pvalue"][7] == 1).all() and (a["pvalue"][:, 1] == 1).all()
    assert not a["align"][0].any() and not a["align"][:, 1].any() and (a["pvalue"][1, 0] < 1)
    assert not a["hist"][0].any() and a["hist"][1, 0].sum() == 2 * (tzero.sum())
    # nothing but width 0 in the database: N = 0, every p-value is 1
    c = _launch(x[:5], xw[:5], y[:2], np.zeros(2, dtype=np.int32), wmax)
    assert (c["pvalue"] == 1).all() and not c["align"].any() and not c["hist"].any()


def test_determinism_and_optional_outputs():
    wmax = 19
    x, xw, y, yw = _packed(wmax)
    Q, T = 63, 3
    a = (x[:Q], xw[:Q], y[:T], yw[:T])
    full = _launch(*a, wmax)
    again = _launch(*a, wmax)
    assert all(np.array_equal(full[k], again[k]) for k in full)
    assert np.array_equal(full["pvalue"].view(np.uint64), again["pvalue"].view(np.uint64))
    for n in range(len(OUTPUTS)):
        for want in itertools.combinations(OUTPUTS, n):
            part = _launch(*a, wmax, want=want)           # checks that the others stay untouched
            assert np.array_equal(part["pvalue"].view(np.uint64), full["pvalue"].view(np.uint64)), want
            assert all(np.array_equal(part[k], full[k]) for k in want)
    aligned = _launch(*a, wmax, shift=0)
    assert all(np.array_equal(full[k], aligned[k]) for k in full)


def test_self_form():
    wmax = 19
    x, xw, _, _ = _packed(wmax)
    me = _launch(x[:65], xw[:65], None, None, wmax)
    two = _launch(x[:65], xw[:65], x[:65], xw[:65], wmax)
    assert all(np.array_equal(me[k], two[k]) for k in me)
    wide = np.nonzero(xw[:65] > 4)[0]
    assert (me["hist"][wide, 0].sum(axis=1) == 2 * xw[:65].sum()).all()      # a query is part of its own null


def test_argument_errors():
    from explainn_amd import _lib
    wmax = 19
    x, xw, y, yw = _packed(wmax)
    a = (x[:3], xw[:3], y[:5], yw[:5])
    _launch(*a, wmax, min_overlap=0, expect=_lib.E_ARG)
    _launch(*a, wmax, pc=-1.0, expect=_lib.E_ARG)
    _launch(*a, wmax, bins=1, expect=_lib.E_ARG)
    _launch(*a, wmax, bins=129, expect=_lib.E_ARG)
    _launch(*a, 0, expect=_lib.E_ARG)
    _launch(*a, 65, expect=_lib.E_UNSUPPORTED)
    _launch(*a, wmax, short=1, expect=_lib.E_ARG)           # a workspace one byte short
    _launch(x[:3], xw[:3], None, None, wmax, expect=_lib.OK)
    lib = _lib.load()
    z = torch.zeros(64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = z.data_ptr()
    call = lambda Q, t, T, ws, n: lib.explainn_motif_significance(p, p, Q, t, t, T, 4, 0.0, 5, 1, 100, p, None, None,
                                                                  None, None, ws, n, s)
    assert call(-1, p, 2, p, 256) == _lib.E_ARG
    assert call(2, p, -1, p, 256) == _lib.E_ARG
    assert call(2, None, 3, p, 256) == _lib.E_ARG           # the self form needs T == Q
    assert call(2, p, 2, p, 16) == _lib.E_ARG               # workspace
    assert call(2, p, 2, None, 1 << 30) == _lib.E_ARG
    assert call(0, p, 2, None, 0) == _lib.OK                # nothing to do
    assert call(2, p, 0, None, 0) == _lib.OK
    for bad in ((-1, 2, 4, 100, 1), (2, 2, 0, 100, 1), (2, 2, 65, 100, 1), (2, 2, 4, 1, 1), (2, 2, 4, 129, 0)):
        assert lib.explainn_motif_significance_workspace_bytes(*bad) == 0
    torch.cuda.synchronize()
    assert not z.any()
    got = _launch(*a, wmax)                                 # the next good call still works
    _check(got, *a, wmax, 5, 0.0, True, 100, "after errors")


# ---- the Python layer ----
def test_query_chunks_do_not_change_the_result():
    from explainn_amd import _lib, motifs
    wmax = 19
    x, xw, y, yw = _packed(wmax)
    Q, T = 65, 64
    q, t = (torch.tensor(x[:Q]), torch.tensor(xw[:Q])), (torch.tensor(y[:T]), torch.tensor(yw[:T]))
    size = lambda n, T: int(_lib.load().explainn_motif_significance_workspace_bytes(n, T, wmax, 100, 1))
    whole = motifs.significance(q, t)
    raw = _launch(x[:Q], xw[:Q], y[:T], yw[:T], wmax)
    assert np.array_equal(whole.pvalue.cpu().numpy().view(np.uint64), raw["pvalue"].view(np.uint64))
    assert np.array_equal(whole.offset.cpu().numpy(), raw["align"][..., 0])
    assert np.array_equal(whole.score.cpu().numpy(), raw["score"])
    for n in (1, 7):
        part = motifs.significance(q, t, workspace_bytes=size(n, T))
        assert all(torch.equal(a, b) for a, b in zip(part, whole)), n
    me = motifs.significance(q)                             # self, in one call and in chunks
    for n in (1, 7):
        part = motifs.significance(q, workspace_bytes=size(n, Q))
        assert all(torch.equal(a, b) for a, b in zip(part, me)), n
    assert all(torch.equal(a, b) for a, b in zip(motifs.significance(q, q), me))
    tiny = motifs.significance(q, t, workspace_bytes=1)      # below one query's need: one query per call
    assert torch.equal(tiny.pvalue, whole.pvalue)


def test_python_layer():
    from explainn_amd import motifs
    pfm, nsites = _bank()
    flat = pfm.reshape(G * U, K, 4)
    res = motifs.significance(flat)
    assert res.pvalue.is_cuda and res.pvalue.dtype == torch.float64 and tuple(res.pvalue.shape) == (G * U, G * U)
    assert res.qvalue.dtype == torch.float64 and res.offset.dtype == torch.int16 and res.score.dtype == torch.int32
    x, xw = mm.pack([m if n else m[:0] for m, n in zip(flat, nsites.reshape(-1))], K)
    p = res.pvalue.cpu().numpy()
    raw = _launch(x, xw, None, None, K)                     # the same call by hand, held to the model
    assert np.array_equal(p.view(np.uint64), raw["pvalue"].view(np.uint64))
    assert np.array_equal(res.score.cpu().numpy(), raw["score"])
    clear, _ = _check(raw, x, xw, None, None, K, 5, 0.0, True, 100, "bank")
    assert clear > 0.5
    assert np.array_equal(res.evalue.cpu().numpy(), p * (G * U))
    assert np.array_equal(res.qvalue.cpu().numpy(), sm.bh_qvalues(p))
    # the same through every accepted form of a set
    # (in a list a motif carries its own width: the filter without a site is given as zero columns -- as 19
    # all-zero rows it would be 19 uniform columns of the database)
    lst = [("filter%d" % i, "bank", mat if n else mat[:0]) for i, (mat, n) in enumerate(zip(flat, nsites.reshape(-1)))]
    for other in (motifs.significance(lst), motifs.significance(motifs.pack(lst)),
                  motifs.significance(torch.from_numpy(flat).cuda()),
                  motifs.significance(dict(pfm=flat, nsites=nsites.reshape(-1))), motifs.significance(lst, lst)):
        assert torch.equal(other.pvalue, res.pvalue) and torch.equal(other.strand, res.strand)
    assert (res.pvalue[U] == 1).all() and (res.pvalue[:, U] == 1).all()          # nsites == 0: width 0
    assert res.strand[1, U + 4] == 1 and res.offset[1, 2 * U] == 3 and res.overlap[1, 2 * U] == K - 3
    assert res.offset[2 * U, 1] == -3 and float(res.pvalue[1, 2 * U]) < 1e-10 and float(res.pvalue[1, 1]) < 1e-15

    hits = motifs.annotate(lst[:U], lst[U:], top=2, by="pvalue")
    assert [h["target"] for h in hits[1]] == [4, U] and hits[1][0]["strand"] == 1 and hits[1][1]["offset"] == 3
    assert [h["target"] for h in hits[3]] == [U + 2] and hits[0] == [] and hits[2] == [] and hits[4] == []
    assert hits[1][0]["pvalue"] <= hits[1][1]["pvalue"] and hits[1][1]["qvalue"] <= 0.05
    assert set(hits[1][0]) == {"target", "ncor", "cor", "offset", "strand", "overlap", "score", "pvalue", "evalue",
                               "qvalue"}
    sig = motifs.significance(lst[:U], lst[U:])
    assert [[h["target"] for h in r] for r in motifs.annotate(sig, by="pvalue", top=2)] == \
        [[h["target"] for h in r] for r in hits]
    plain = motifs.annotate(lst[:U], lst[U:], top=2)        # the default is unchanged
    assert [h["target"] for h in plain[1]] == [4, U] and set(plain[1][0]) == {"target", "ncor", "cor", "offset",
                                                                              "strand", "overlap"}
    empty = motifs.significance(lst[:0], lst)
    assert tuple(empty.pvalue.shape) == (0, G * U) and tuple(empty.qvalue.shape) == (0, G * U)
    with pytest.raises(ValueError):
        motifs.significance([np.ones((65, 4))])


def test_command_line(tmp_path):
    from explainn_amd import motifs
    from explainn_amd.interpret import format_jaspar
    pfm, nsites = _bank()
    os.makedirs(os.path.join(tmp_path, "motifs"))
    for u in range(U):
        with open(os.path.join(tmp_path, "motifs", "filter%d.jaspar" % u), "w") as fh:
            fh.write(format_jaspar(pfm[0, u], "filter%d" % u, "m0"))
    db = os.path.join(tmp_path, "db.meme")
    motifs.write_meme(db, [("T%d" % i, "name%d" % i, m) for i, m in enumerate(pfm[1:].reshape(-1, K, 4)) if m.any()])
    head = ["Query", "Target", "TargetName", "Ncor", "Cor", "Offset", "Strand", "Overlap"]
    planted = [["filter1", "T4", "name4"], ["filter1", "T5", "name5"], ["filter3", "T7", "name7"]]
    out = os.path.join(tmp_path, "ann.tsv")
    motifs.main(["annotate", os.path.join(tmp_path, "motifs"), db, "-o", out])
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert rows[0] == head and [r[:3] for r in rows[1:]] == planted
    assert rows[1][6] == "-" and rows[2][5:] == ["3", "+", str(K - 3)]
    # the default file is what the Ncor code path writes: the same bytes as formatting annotate()'s hits
    queries, dbm = motifs.read_motifs(os.path.join(tmp_path, "motifs")), motifs.read_motifs(db)
    text = "\t".join(head) + "\n"
    for (qid, _, _), hs in zip(queries, motifs.annotate(queries, dbm)):
        for h in hs:
            text += "%s\t%s\t%s\t%.4f\t%.4f\t%d\t%s\t%d\n" % (qid, dbm[h["target"]][0], dbm[h["target"]][1], h["ncor"],
                                                            h["cor"], h["offset"], "-" if h["strand"] else "+",
                                                            h["overlap"])
    assert open(out).read() == text
    out = os.path.join(tmp_path, "sig.tsv")
    motifs.main(["annotate", os.path.join(tmp_path, "motifs"), db, "-o", out, "--by", "pvalue", "--max-qvalue", "0.01",
                 "--bins", "64"])
    rows = [ln.rstrip("\n").split("\t") for ln in open(out)]
    assert rows[0] == head + ["Pvalue", "Evalue", "Qvalue"] and all(len(r) == 11 for r in rows)
    assert [r[:3] for r in rows[1:]] == planted
    assert rows[1][6] == "-" and rows[2][5:8] == ["3", "+", str(K - 3)]
    assert all(float(r[8]) < 1e-10 and float(r[10]) <= 0.01 and float(r[9]) == pytest.approx(float(r[8]) * 9, rel=2e-3)
               for r in rows[1:])
