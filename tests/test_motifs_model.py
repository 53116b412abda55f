"""CPU checks of motif comparison: the numpy model of tests/motifs_model.py against np.corrcoef and against
its own plain loops, and the host code of explainn_amd.motifs (readers, writer, annotate, cluster,
reproducibility) on hand-made inputs.  The device call itself is tests/test_gpu_motifs.py."""
import os

import numpy as np
import pytest
import torch

import motifs_model as mm
from explainn_amd import motifs

MEME_TEXT = """MEME version 4

ALPHABET= ACGT

strands: + -

Background letter frequencies
A 0.25 C 0.25 G 0.25 T 0.25

MOTIF MA0001.1 AGL3
letter-probability matrix: alength= 4 w= 3 nsites= 97 E= 0
 0.000000  0.969072  0.010309  0.020619
 0.5 0.25 0.125 0.125

0.1 0.2 0.3 0.4
URL http://example.invalid/MA0001.1

MOTIF second
letter-probability matrix: alength= 4 w= 2
0.25 0.25 0.25 0.25
1 0 0 0
"""


def _freq(rng, w, alpha=0.4):
    return rng.dirichlet([alpha] * 4, size=w)


def _result(q, t=None, **kw):
    """A MotifComparison of host tensors from the model."""
    x, w = mm.pack(q)
    if t is None:
        b = mm.compare(x, w, **kw)
    else:
        wmax = max(x.shape[1], max(len(m) for m in t))
        x, w = mm.pack(q, wmax)
        y, v = mm.pack(t, wmax)
        b = mm.compare(x, w, y, v, **kw)
    return motifs.MotifComparison(torch.from_numpy(b["ncor"].astype(np.float32)),
                                  torch.from_numpy(b["cor"].astype(np.float32)),
                                  torch.from_numpy(b["offset"].astype(np.int16)),
                                  torch.from_numpy(b["strand"].astype(np.int16)),
                                  torch.from_numpy(b["overlap"].astype(np.int16)))


def test_cor_is_pearson_of_the_aligned_cells():
    rng = np.random.default_rng(0)
    seen = 0
    for wq, wt in ((6, 9), (9, 6), (1, 4), (12, 12), (19, 24)):
        q, t = _freq(rng, wq), _freq(rng, wt)
        for s, o, w, cor, ncor in mm.alignments_loops(q, t, min_overlap=1):
            tt = mm.revcomp(t) if s else t
            lo = max(0, -o)
            a, b = q[lo:lo + w].ravel(), tt[lo + o:lo + o + w].ravel()
            assert abs(cor - np.corrcoef(a, b)[0, 1]) < 1e-12, (wq, wt, s, o)
            assert abs(ncor - cor * w / (wq + wt - w)) < 1e-15
            seen += 1
    assert seen > 100


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("min_overlap,pc", [(1, 0.0), (5, 1.0), (70, 0.0)])
def test_vectorised_equals_loops(min_overlap, pc, both):
    rng = np.random.default_rng(1)
    mats = [rng.multinomial(20, p).astype(np.float64) for p in
            (_freq(rng, w) for w in (0, 1, 2, 5, 7, 12, 12))]
    mats.append(np.full((6, 4), 5.0))                       # equal counts: no variance anywhere
    mats.append(np.concatenate([mats[5], mm.revcomp(mats[5])]))   # a palindrome
    x, w = mm.pack(mats)
    got = mm.compare(x, w, min_overlap=min_overlap, pc=pc, both_strands=both)
    for i, q in enumerate(mats):
        for j, t in enumerate(mats):
            ncor, cor, o, s, ov = mm.best_loops(q, t, min_overlap, pc, both)
            assert abs(got["ncor"][i, j] - ncor) < 1e-12 and abs(got["cor"][i, j] - cor) < 1e-12, (i, j)
            if ncor - got["runner_up"][i, j] > 1e-9:
                assert (got["offset"][i, j], got["strand"][i, j], got["overlap"][i, j]) == (o, s, ov), (i, j)
    # a bad width is a width of 0
    bad = w.copy()
    bad[3] = x.shape[1] + 1
    zero = w.copy()
    zero[3] = 0
    a, b = mm.compare(x, bad, min_overlap=min_overlap, pc=pc), mm.compare(x, zero, min_overlap=min_overlap, pc=pc)
    assert np.array_equal(a["ncor"], b["ncor"]) and not a["ncor"][3].any() and not a["ncor"][:, 3].any()


def test_planted_alignments_and_tie_rule():
    rng = np.random.default_rng(2)
    m = _freq(rng, 12)
    assert mm.best_loops(m, m)[:1] == (pytest.approx(1.0),) and mm.best_loops(m, m)[2:] == (0, 0, 12)
    ncor, cor, o, s, w = mm.best_loops(m, mm.revcomp(m))
    assert (round(ncor, 12), o, s, w) == (1.0, 0, 1, 12)
    ncor, cor, o, s, w = mm.best_loops(m[3:10], m)          # a sub-motif: found where it was cut
    assert (round(cor, 12), o, s, w) == (1.0, 3, 0, 7) and abs(ncor - 7 / 12) < 1e-12
    ncor, cor, o, s, w = mm.best_loops(m, m[3:10])
    assert (round(cor, 12), o, s, w) == (1.0, -3, 0, 7)
    pal = np.concatenate([m[:5], mm.revcomp(m[:5])])        # both strands tie exactly: strand 0 wins
    assert mm.best_loops(pal, pal)[2:] == (0, 0, 10)
    x, w = mm.pack([pal, m])
    got = mm.compare(x, w)
    assert got["strand"][0, 0] == 0 and got["offset"][0, 0] == 0
    # nothing admissible at a width of 0; min_overlap above both widths means the narrower motif whole
    assert mm.best_loops(m[:0], m) == (0.0, 0.0, 0, 0, 0)
    assert all(a[2] == 7 for a in mm.alignments_loops(m[3:10], m, min_overlap=70))


def test_meme_reader_and_round_trips(tmp_path):
    path = os.path.join(tmp_path, "in.meme")
    with open(path, "w") as fh:
        fh.write(MEME_TEXT)
    got = motifs.read_meme(path)
    assert [(i, n) for i, n, _ in got] == [("MA0001.1", "AGL3"), ("second", "")]
    assert got[0][2].shape == (3, 4) and got[0][2][0, 1] == 0.969072 and got[0][2][2, 3] == 0.4
    assert np.array_equal(got[1][2], [[0.25] * 4, [1, 0, 0, 0]])
    rng = np.random.default_rng(3)
    probs = [("m%d" % i, "name %d" % i if i else "", rng.dirichlet([0.5] * 4, size=w)) for i, w in enumerate((1, 7, 30))]
    out = os.path.join(tmp_path, "out.meme")
    motifs.write_meme(out, probs)
    back = motifs.read_motifs(out)                          # the format is recognised
    assert len(back) == 3
    for (i0, n0, m0), (i1, n1, m1) in zip(probs, back):
        assert (i0, n0) == (i1, n1) and np.array_equal(m0, m1)
    # counts are written as frequencies, an empty column as 0.25
    counts = np.array([[3, 1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1]], dtype=np.int64)
    motifs.write_meme(out, [("c", "x", counts)])
    assert "nsites= 4" in open(out).read()
    assert np.array_equal(motifs.read_meme(out)[0][2], [[0.75, 0.25, 0, 0], [0.25] * 4, [0.25] * 4])


def test_jaspar_round_trip(tmp_path):
    from explainn_amd.interpret import format_jaspar
    rng = np.random.default_rng(4)
    pfms = [rng.integers(0, 500, size=(19, 4)), rng.integers(0, 9, size=(5, 4))]
    one = os.path.join(tmp_path, "all.jaspar")
    os.makedirs(os.path.join(tmp_path, "motifs"))
    with open(one, "w") as fh:
        for u, pfm in enumerate(pfms):
            text = format_jaspar(pfm, "filter%d" % u, "run one")
            fh.write(text)
            with open(os.path.join(tmp_path, "motifs", "filter%d.jaspar" % (u + 9)), "w") as g:
                g.write(text)
    open(os.path.join(tmp_path, "motifs", "filter2.jaspar"), "w").close()      # a filter without a site
    for got in (motifs.read_jaspar(one), motifs.read_motifs(one)):
        assert [(i, n) for i, n, _ in got] == [("filter0", "run one"), ("filter1", "run one")]
        assert all(np.array_equal(m, p) for (_, _, m), p in zip(got, pfms))
    got = motifs.read_motifs(os.path.join(tmp_path, "motifs"))                 # numeric order, empty file skipped
    assert [i for i, _, _ in got] == ["filter0", "filter1"] and np.array_equal(got[1][2], pfms[1])
    assert motifs.read_jaspar(os.path.join(tmp_path, "motifs", "filter2.jaspar")) == []
    x, w = motifs.pack(got)
    assert tuple(x.shape) == (2, 19, 4) and w.tolist() == [19, 5] and not x[1, 5:].any()
    assert x.dtype == torch.float32 and w.dtype == torch.int32


def _comparison(ncor, cor=None):
    ncor = torch.tensor(ncor, dtype=torch.float32)
    cor = ncor.clone() if cor is None else torch.tensor(cor, dtype=torch.float32)
    z = torch.zeros(ncor.shape, dtype=torch.int16)
    return motifs.MotifComparison(ncor, cor, z, z, z)


def test_cluster_on_a_hand_made_matrix():
    S = np.eye(7)
    for a, b, v in ((5, 2, 0.9), (2, 6, 0.5), (1, 4, 0.7), (5, 6, 0.45), (0, 3, 0.39)):
        S[a, b] = S[b, a] = v
    S[3, 3] = 0.0                                           # a motif of width 0 does not even match itself
    S[4, 0] = 0.8                                           # one direction passes: still an edge
    cor = (S > 0).astype(np.float64)
    cor[1, 4] = cor[4, 1] = 0.5                             # Ncor passes, cor does not: no edge
    labels, reps = motifs.cluster(_comparison(S, cor))
    # {0,4} {1} {2,5,6} {3}: chained through 2, numbered by smallest member
    assert labels.tolist() == [0, 1, 2, 3, 0, 2, 2] and labels.dtype == np.int64
    # sums inside {2,5,6}: 2 -> 1+.9+.5, 5 -> 1+.9+.45, 6 -> 1+.5+.45; inside {0,4}: 0 -> 1, 4 -> 1.8
    assert reps.tolist() == [4, 1, 2, 3]
    labels, reps = motifs.cluster(_comparison(S, cor), min_ncor=0.95)
    assert labels.tolist() == list(range(7)) and reps.tolist() == list(range(7))
    S2 = np.ones((3, 3))                                    # a tie between representatives: the lower index
    assert motifs.cluster(_comparison(S2))[1].tolist() == [0]


def test_annotate_order_and_ties():
    ncor = [[0.5, 0.9, 0.5, 0.3, 0.9], [0.1, 0.2, 0.3, 0.39, 0.0], [0.7, 0.7, 0.7, 0.7, 0.7]]
    cor = [[0.7, 0.9, 0.7, 0.9, 0.59], [0.9] * 5, [0.9] * 5]
    res = _comparison(ncor, cor)
    hits = motifs.annotate(res, top=3)
    assert [h["target"] for h in hits[0]] == [1, 0, 2]      # 4 fails cor, 3 fails Ncor; the tie 0, 2 in index order
    assert hits[0][0]["ncor"] == pytest.approx(0.9) and hits[0][1]["cor"] == pytest.approx(0.7)
    assert hits[1] == []
    assert [h["target"] for h in hits[2]] == [0, 1, 2]
    assert [h["target"] for h in motifs.annotate(res, top=9)[2]] == [0, 1, 2, 3, 4]
    assert [h["target"] for h in motifs.annotate(res, top=2, min_ncor=0.2, min_cor=0.0)[0]] == [1, 4]
    assert motifs.annotate(res, top=0) == [[], [], []]


def test_reproducibility_on_a_planted_bank():
    rng = np.random.default_rng(5)
    G, U, k = 3, 4, 12
    pfm = np.zeros((G, U, k, 4))
    for g in range(G):
        for u in range(U):
            pfm[g, u] = np.stack([rng.multinomial(50, p) for p in _freq(rng, k, 0.3)])
    a = pfm[0, 1].copy()
    pfm[1, 3] = mm.revcomp(a)                               # in all three members
    pfm[2, 0] = np.concatenate([np.full((2, 4), 12.5), a[:-2]])    # shifted by two columns
    b = pfm[0, 2].copy()
    pfm[2, 3] = b                                           # in two
    nsites = np.full((G, U), 50)
    pfm[1, 0] = 0
    nsites[1, 0] = 0
    flat = [m if n else m[:0] for m, n in zip(pfm.reshape(G * U, k, 4), nsites.reshape(-1))]
    res = _result(flat)
    count, partner = motifs.reproducibility(pfm, nsites, result=res)
    want = np.zeros((G, U), dtype=np.int64)
    want[0, 1] = want[1, 3] = want[2, 0] = 2
    want[0, 2] = want[2, 3] = 1
    assert np.array_equal(count, want) and count.dtype == np.int64
    assert partner.shape == (G, U, G)
    assert partner[0, 1].tolist() == [-1, 3, 0] and partner[1, 3].tolist() == [1, -1, 0]
    assert partner[2, 0].tolist() == [1, 3, -1] and partner[0, 2].tolist() == [-1, -1, 3]
    assert partner[2, 3].tolist() == [2, -1, -1] and (partner[1, 0] == -1).all() and (partner[0, 0] == -1).all()
    labels, reps = motifs.cluster(res)
    assert labels[1] == labels[4 + 3] == labels[8 + 0] and labels[2] == labels[8 + 3] != labels[1]
    assert len(set(labels.tolist())) == G * U - 3


def test_compare_refuses_bad_arguments_and_the_host():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        motifs.compare([np.ones((5, 4))], device="cpu")
    with pytest.raises(ValueError):
        motifs.compare([np.ones((5, 4))], min_overlap=0)
    with pytest.raises(ValueError):
        motifs.compare([np.ones((5, 4))], pseudocount=-1.0)
