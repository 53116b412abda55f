"""The motif tree's numpy model (tests/motiftree_model.py) against its own definitions, against scipy and against
tests/motifs_model.compare, and the host side of explainn_amd.motifs' tree / merge (no device needed)."""
import functools

import numpy as np
import pytest

import motifs_model as mm
import motiftree_model as mt

LINKAGES = ("single", "complete", "average")


@functools.lru_cache(maxsize=None)
def _compared(kind):
    """(motifs, packed x, widths, the fp64 comparison of motifs_model) of a named set."""
    if kind == "family":
        mats, _ = mt.family_set(5)
    elif kind == "twice":                              # every motif present twice: exact ties in q
        mats, _ = mt.family_set(6, bases=3, copies=6)
        mats = mats + [m.copy() for m in mats]
    elif kind == "zeros":                              # width-0 motifs mixed in
        mats, _ = mt.family_set(7, bases=3, copies=5)
        for at in (0, 4, 9, 17):
            mats.insert(at, np.zeros((0, 4)))
    else:                                              # unrelated random motifs, widths 6 to 24
        rng = np.random.default_rng(8)
        mats = [mt.random_motif(rng, int(w)) for w in rng.integers(6, 25, size=30)]
    x, w = mm.pack(mats)
    best = mm.compare(x, w)
    return mats, x, w, best


def _tree(kind, linkage, brute=False):
    _, _, w, best = _compared(kind)
    return (mt.tree_brute if brute else mt.tree)(best["ncor"], best["offset"], best["strand"], w, linkage)


def _placed_cor(x, w, i, fi, hi, j, fj, hj):
    """cor of the frame columns two placed leaves share, by the definitions of motifs_model."""
    di, ni = mm.prepare(mt.placed(x[i, :w[i]], fi))
    dj, nj = mm.prepare(mt.placed(x[j, :w[j]], fj))
    a, b = max(hi, hj), min(hi + w[i], hj + w[j])
    xy = sum(float(di[c - hi] @ dj[c - hj]) for c in range(a, b))
    sx, sy = sum(ni[c - hi] for c in range(a, b)), sum(nj[c - hj] for c in range(a, b))
    return 0.0 if sx < mm.VAR_FLOOR or sy < mm.VAR_FLOOR else xy / np.sqrt(sx * sy)


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("kind", ["family", "twice", "zeros", "random"])
def test_every_step_places_its_best_pair_as_compared(kind, linkage):
    _, x, w, best = _compared(kind)
    tr = _tree(kind, linkage)
    M = len(w)
    slot, f, h = np.arange(M), np.zeros(M, np.int64), np.zeros(M, np.int64)
    checked = 0
    for rec in tr["log"]:
        lo, hi, leaves, i, j, F, H = (int(v) for v in rec[:7])
        assert lo < hi and i < j and {slot[i], slot[j]} == {lo, hi}
        moved = slot == hi
        f[moved], h[moved] = mt.apply(F, H, f[moved], h[moved], w[moved].astype(np.int64))
        slot[moved] = lo
        assert leaves == (slot == lo).sum()
        assert f[lo] == 0                              # a cluster's smallest leaf is never flipped
        if best["overlap"][i, j] > 0:
            checked += 1
            assert mt.overlap_of(h[i], w[i], h[j], w[j]) == best["overlap"][i, j]
            assert f[i] ^ f[j] == best["strand"][i, j]
            assert abs(_placed_cor(x, w, i, f[i], h[i], j, f[j], h[j]) - best["cor"][i, j]) <= 1e-5
    assert checked >= (M - 1) // 2
    assert np.array_equal(f, tr["flips"]) and np.array_equal(h, tr["shifts"])
    assert (np.diff(mt.heights(tr)) <= 0).all()
    assert M == 0 or tr["flips"][0] == 0
    assert sorted(tr["gone"].tolist()) == [-1] + list(range(M - 1))


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("kind", ["family", "twice", "zeros", "random"])
def test_row_updates_equal_the_brute_force_definition(kind, linkage):
    a, b = _tree(kind, linkage), _tree(kind, linkage, brute=True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_ties_go_to_the_smaller_slots():
    w = np.full(4, 8, np.int32)
    ncor = np.full((4, 4), 0.5, np.float32)
    z = np.zeros((4, 4), np.int64)
    for linkage in LINKAGES:
        tr = mt.tree(ncor, z, z, w, linkage)
        assert tr["log"][:, :2].tolist() == [[0, 1], [0, 2], [0, 3]]
        assert tr["log"][:, 3:5].tolist() == [[0, 1], [0, 2], [0, 3]]
    ncor[1, 3] = 0.75
    tr = mt.tree(ncor, z, z, w, "single")
    assert tr["log"][:, :2].tolist() == [[1, 3], [0, 1], [0, 2]] and tr["log"][1, 3:5].tolist() == [0, 1]
    for M in (0, 1):
        tr = mt.tree(np.zeros((M, M)), np.zeros((M, M)), np.zeros((M, M)), np.zeros(M), "average")
        assert tr["log"].shape == (0, 8) and len(tr["gone"]) == M


def _partition(labels):
    return {frozenset(np.nonzero(labels == c)[0].tolist()) for c in set(labels.tolist())}


@pytest.mark.parametrize("linkage", LINKAGES)
def test_heights_and_cuts_equal_scipy(linkage):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    rng = np.random.default_rng(11)
    M = 30
    ncor = rng.uniform(0.05, 0.95, size=(M, M)).astype(np.float32)
    q = mt.quantise(ncor)
    iu = np.triu_indices(M, 1)
    assert len(set(q[iu].tolist())) == len(iu[0])      # tie-free
    z = np.zeros((M, M), np.int64)
    w = np.full(M, 10, np.int32)
    tr = mt.tree(ncor, z, z, w, linkage)
    Z = hier.linkage(1.0 - q[iu].astype(np.float64) / mt.SCALE, method=linkage)
    assert np.abs((1.0 - mt.heights(tr)) - Z[:, 2]).max() <= 1e-12
    assert np.array_equal(tr["log"][:, 2], Z[:, 3].astype(np.int64))
    for k in (0.3, 0.5, 0.7):
        thr = int(k * mt.SCALE)
        assert np.abs(mt.heights(tr) * mt.SCALE - thr).min() > 1      # the cut is clear of every height
        labels = mt.cut(tr, w, thr / mt.SCALE)[0]
        want = hier.fcluster(Z, t=1.0 - thr / mt.SCALE, criterion="distance")
        assert _partition(labels) == _partition(want)


@pytest.mark.parametrize("kind", ["family", "twice", "zeros", "random"])
def test_single_linkage_cut_is_the_union_find(kind):
    _, _, w, best = _compared(kind)
    tr = _tree(kind, "single")
    q = mt.quantise(best["ncor"])
    M = len(w)
    for min_ncor in (0.2, 0.45, 0.8):
        parent = list(range(M))

        def find(a):
            while parent[a] != a:
                a = parent[a]
            return a
        for i in range(M):
            for j in range(i + 1, M):
                if q[i, j] >= mt.threshold(min_ncor):
                    a, b = find(i), find(j)
                    parent[max(a, b)] = min(a, b)
        roots = np.array([find(a) for a in range(M)])
        labels, _, _, _, slots = mt.cut(tr, w, min_ncor)
        assert np.array_equal(slots[labels], roots)
        assert np.array_equal(labels, np.searchsorted(np.unique(roots), roots))


def test_cut_and_pool_rebuild_the_families():
    """Every copy is a piece of its base, so in a cluster's frame all members agree column by column.  Two copies
    of a base share at least 8 of the 12 columns they span together (Ncor >= 0.66), so a cut at 0.6 keeps the
    families whole under every linkage."""
    mats, fam = mt.family_set(5)
    _, x, w, _ = _compared("family")
    for linkage in LINKAGES:
        tr = _tree("family", linkage)
        labels, flips, shifts, spans, slots = mt.cut(tr, w, 0.6)
        assert np.array_equal(labels, fam)
        merged, support = mt.pool(x, w, labels, flips, shifts, spans)
        assert merged.shape == (4, spans.max(), 4) and merged.dtype == np.float64
        for c in range(4):
            mem = np.nonzero(labels == c)[0]
            assert flips[mem[0]] == 0 and shifts[mem].min() == 0 and spans[c] == (shifts[mem] + w[mem]).max()
            assert spans[c] <= 14 and support[c, :spans[c]].min() >= 1 and not support[c, spans[c]:].any()
            for y in mem:
                cols = slice(shifts[y], shifts[y] + w[y])
                assert np.array_equal(mt.placed(x[y, :w[y]], flips[y]) * support[c, cols, None], merged[c, cols])
    with pytest.raises(ValueError):
        mt.cut(tr, w, 0.0)
    lo, hi = mt.cut(tr, w, 0.05)[0], mt.cut(tr, w, 0.999)[0]
    assert lo.max() < 4 <= hi.max()


# ---- the host side of explainn_amd.motifs ----
def _host_tree(kind="family", linkage="average"):
    import torch
    from explainn_amd import motifs
    tr = _tree(kind, linkage)
    w = _compared(kind)[2]
    t = {k: torch.from_numpy(v) for k, v in tr.items()}
    return motifs.MotifTree(t["log"], t["link"], t["gone"], t["flips"], t["shifts"], torch.from_numpy(w), linkage), tr


def test_newick_and_linkage_matrix_are_well_formed():
    tree, tr = _host_tree()
    M = tree.M
    assert np.array_equal(tree.heights, mt.heights(tr))
    names = ["m%d" % i for i in range(M)]
    text = tree.newick(names)
    assert text.endswith(";") and text.count("(") == text.count(")") == M - 1 and text.count(",") == M - 1
    depth = 0
    for ch in text:
        depth += (ch == "(") - (ch == ")")
        assert depth >= 0
    import re
    assert sorted(re.findall(r"m\d+", text)) == sorted(names)
    assert all(float(v) >= -1e-12 for v in re.findall(r":([-0-9.e+]+)", text))
    assert tree.newick(["a b", "c(d)"] + names[2:]).count("a_b:") == 1
    Z = tree.linkage_matrix()
    assert Z.shape == (M - 1, 4) and (np.diff(Z[:, 2]) >= 0).all()
    assert sorted(Z[:, :2].astype(int).ravel().tolist()) == list(range(2 * M - 2))      # every node is merged once
    size = np.concatenate([np.ones(M), Z[:, 3]])
    assert np.array_equal(size[Z[:, 0].astype(int)] + size[Z[:, 1].astype(int)], Z[:, 3])
    assert (Z[:, :2].max(axis=1) < M + np.arange(M - 1)).all()
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    assert hier.is_valid_linkage(Z)
    with pytest.raises(ValueError):
        tree.newick(names[:-1])


def test_trimmed():
    from explainn_amd import motifs
    pfm = np.zeros((2, 6, 4))
    pfm[0, :, 0] = [1, 4, 4, 3, 4, 1]                  # cluster 0: four members, the ends covered by one
    pfm[0, 3] = [1, 1, 1, 0]                           # an inner column of low information stays
    pfm[1, :3] = 1.0                                   # cluster 1: uniform columns
    support = np.array([[1, 4, 4, 3, 4, 1], [2, 2, 2, 0, 0, 0]], np.int32)
    labels = np.array([0, 0, 0, 0, 1, 1])
    members = [np.arange(4), np.arange(4, 6)]
    m = motifs.MergedMotifs(pfm, np.array([6, 3], np.int32), support, labels, members, np.zeros(6, np.int32),
                            np.array([0, 1, 1, 1, 0, 0], np.int32), ["cluster0_n4", "cluster1_n2"])
    t = m.trimmed()
    assert t.widths.tolist() == [4, 3] and np.array_equal(t.pfm[0, :4], pfm[0, 1:5])
    assert t.support[0].tolist()[:4] == [4, 4, 3, 4] and t.shifts.tolist() == [-1, 0, 0, 0, 0, 0]
    assert m.trimmed(min_support=0.0).widths.tolist() == [6, 3]
    t = m.trimmed(min_support=0.0, min_ic=1.0)
    assert t.widths.tolist() == [6, 0] and t.pfm.shape == (2, 6, 4)
    got = t.as_motifs()
    assert [g[0] for g in got] == ["cluster0_n4", "cluster1_n2"] and got[0][2].shape == (6, 4) and got[1][2].shape == (0, 4)
    with pytest.raises(ValueError):
        m.trimmed(min_support=1.5)


def test_refusals_and_command_line_arguments(tmp_path):
    import torch
    from explainn_amd import motifs
    tree, _ = _host_tree()
    for bad in (0, -0.5, float("nan")):
        with pytest.raises(ValueError):
            tree.cut(bad)
        with pytest.raises(ValueError):
            motifs.merge([np.ones((8, 4))], min_ncor=bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        tree.cut(0.4)

    def res(M, device="cpu"):
        e = lambda dt: torch.empty((M, M), dtype=dt, device=device)
        return motifs.MotifComparison(e(torch.float32), e(torch.float32), e(torch.int16), e(torch.int16),
                                      e(torch.int16))
    with pytest.raises(ValueError, match="max_bytes"):
        motifs.tree(res(40), max_bytes=16 * 40 * 40 - 1)
    with pytest.raises(ValueError, match="65535"):
        motifs.tree(res(65536, "meta"), max_bytes=1 << 60)
    with pytest.raises(ValueError, match="at most"):
        motifs.tree(res(motifs.MAX_LEAVES + 1, "meta"), max_bytes=1 << 60)
    with pytest.raises(ValueError, match="linkage"):
        motifs.tree(res(4), linkage="ward")
    with pytest.raises(ValueError, match="self-comparison"):
        motifs.tree(motifs.MotifComparison(*(torch.empty((3, 4)) for _ in range(5))))
    with pytest.raises(RuntimeError, match="HIP device"):
        motifs.tree(res(4))
    assert motifs._cut_threshold(0.4) == int(np.ceil(0.4 * (1 << 20))) == mt.threshold(0.4)

    path = str(tmp_path / "in.meme")
    motifs.write_meme(path, [("a", "", np.ones((8, 4)))])
    for argv in (["merge", path], ["merge", "-o", "x.meme"], ["merge", path, "-o", "x.meme", "--linkage", "ward"],
                 ["merge", path, "-o", "x.meme", "--min-ncor", "much"]):
        with pytest.raises(SystemExit):
            motifs.main(argv)
    with pytest.raises(ValueError):
        motifs.main(["merge", path, "-o", str(tmp_path / "x.meme"), "--min-ncor", "0"])
