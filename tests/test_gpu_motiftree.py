"""Motif tree, cut, placement and pooled cluster motifs on the device (csrc/motiftree.hip, explainn_amd.motifs.tree /
MotifTree.cut / merge) against tests/motiftree_model.py.  The model is run on the device's own comparison (the
tree reads Ncor quantised to 2^-20), and everything after that is integer-exact or a fixed order of fp64 adds, so
every array is compared with array_equal: the log, the labels, flips, shifts and spans, the support, and the pooled
matrices bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import motifs_model as mm
import motiftree_model as mt

pytestmark = pytest.mark.gpu

LINKAGES = ("single", "complete", "average")


@functools.lru_cache(maxsize=None)
def _mats(kind):
    if kind == "family":                               # 4 bases x 10 copies, widths 8 to 14
        return tuple(mt.family_set(5)[0])
    if kind == "twice":                                # every motif present twice: exact ties in q
        mats = mt.family_set(5)[0]
        return tuple(mats + [m.copy() for m in mats])
    if kind == "zeros":                                # width-0 motifs mixed in
        mats = mt.family_set(7, bases=3, copies=5)[0]
        for at in (0, 4, 9, 17):
            mats.insert(at, np.zeros((0, 4)))
        return tuple(mats)
    if kind == "big":                                  # M = 1030, widths 6 to 24
        return tuple(mt.family_set(9, bases=103, copies=10, widths=(10, 24))[0])
    M = int(kind)                                      # M motifs, half of them in families
    rng = np.random.default_rng(M)
    mats = mt.family_set(M, bases=max(M // 10, 1), copies=5)[0][:M // 2]
    return tuple(mats + [mt.random_motif(rng, int(w)) for w in rng.integers(6, 25, size=M - len(mats))])


@functools.lru_cache(maxsize=None)
def _compared(kind):
    """The device comparison of a set, its host copy, and the packed matrices."""
    from explainn_amd import motifs
    mats = list(_mats(kind))
    res = motifs.compare(mats)
    x, w = mm.pack(mats)
    host = {k: getattr(res, k).cpu().numpy() for k in ("ncor", "offset", "strand", "overlap")}
    for a in (x, w) + tuple(host.values()):
        a.setflags(write=False)
    return mats, res, x, w, host


@functools.lru_cache(maxsize=None)
def _model(kind, linkage):
    _, _, _, w, host = _compared(kind)
    tr = mt.tree(host["ncor"], host["offset"], host["strand"], w, linkage)
    for a in tr.values():
        a.setflags(write=False)
    return tr


def _device_tree(kind, linkage):
    from explainn_amd import motifs
    _, res, _, w, _ = _compared(kind)
    return motifs.tree(res, torch.from_numpy(np.array(w)), linkage)


def _tree_arrays(tree):
    return {k: getattr(tree, k).cpu().numpy() for k in ("log", "link", "gone", "flips", "shifts")}


def _check_tree(tree, model, what):
    got = _tree_arrays(tree)
    for k, v in model.items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k], v), "%s: %s" % (what, k)
    assert np.array_equal(tree.heights, mt.heights(model))


def _check_cut_and_pool(kind, tree, model, min_ncor, what):
    from explainn_amd import motifs
    mats, _, x, w, _ = _compared(kind)
    labels, flips, shifts, spans = tree.cut(min_ncor)
    ml, mf, ms, msp, _ = mt.cut(model, w, min_ncor)
    assert labels.dtype == torch.int64 and flips.dtype == torch.int32 and spans.dtype == np.int32
    assert np.array_equal(labels.cpu().numpy(), ml), what
    assert np.array_equal(flips.cpu().numpy(), mf), what
    assert np.array_equal(shifts.cpu().numpy(), ms), what
    assert np.array_equal(spans, msp), what
    merged = motifs.merge(mats, tree=tree, min_ncor=min_ncor)
    want, support = mt.pool(x, w, ml, mf, ms, msp)
    assert merged.pfm.dtype == np.float64 and merged.pfm.shape == want.shape, what
    assert np.array_equal(merged.pfm.view(np.uint64), want.view(np.uint64)), what + ": pooled bits"
    assert merged.support.dtype == np.int32 and np.array_equal(merged.support, support), what
    assert np.array_equal(merged.widths, msp) and np.array_equal(merged.labels, ml)
    assert np.array_equal(merged.flips, mf) and np.array_equal(merged.shifts, ms)
    assert [m.tolist() for m in merged.members] == [np.nonzero(ml == c)[0].tolist() for c in range(len(msp))]
    assert merged.names == ["cluster%d_n%d" % (c, (ml == c).sum()) for c in range(len(msp))]
    return merged


@pytest.mark.parametrize("M", [1, 2, 3])
def test_smallest_sets(M):
    for linkage in LINKAGES:
        tree = _device_tree(str(M), linkage)
        model = _model(str(M), linkage)
        assert tuple(tree.log.shape) == (M - 1, 8) and tuple(tree.link.shape) == (M - 1, 2)
        _check_tree(tree, model, "M %d %s" % (M, linkage))
        merged = _check_cut_and_pool(str(M), tree, model, 0.4, "M %d %s" % (M, linkage))
        assert len(merged) >= 1


@pytest.mark.parametrize("linkage", LINKAGES)
@pytest.mark.parametrize("kind", ["family", "130"])
def test_every_linkage(kind, linkage):
    tree, model = _device_tree(kind, linkage), _model(kind, linkage)
    _check_tree(tree, model, kind + " " + linkage)
    _check_cut_and_pool(kind, tree, model, 0.6, kind + " " + linkage)


def test_families_are_rebuilt():
    tree, model = _device_tree("family", "average"), _model("family", "average")
    merged = _check_cut_and_pool("family", tree, model, 0.6, "family")
    assert merged.labels.tolist() == mt.family_set(5)[1].tolist() and len(merged) == 4
    assert merged.widths.max() <= 14 and (merged.flips[[0, 10, 20, 30]] == 0).all()


@pytest.mark.parametrize("kind", ["twice", "zeros", "65"])
def test_ties_empty_motifs_and_wavefront_edges(kind):
    _, _, _, w, host = _compared(kind)
    if kind == "twice":
        q = mt.quantise(host["ncor"])[np.triu_indices(len(w), 1)]
        assert len(np.unique(q)) < len(q) // 2         # ties decide this tree
    if kind == "zeros":
        assert (np.asarray(w) == 0).sum() == 4
    for linkage in ("average", "complete"):
        tree, model = _device_tree(kind, linkage), _model(kind, linkage)
        _check_tree(tree, model, kind + " " + linkage)
        _check_cut_and_pool(kind, tree, model, 0.6, kind + " " + linkage)
    if kind == "zeros":                                # Ncor 0 with everything: they merge last, each alone at a cut
        zero = np.nonzero(np.asarray(w) == 0)[0]
        labels = tree.cut(0.05)[0].cpu().numpy()
        assert all((labels == labels[z]).sum() == 1 for z in zero)
        assert not model["link"][-len(zero):, 0].any()


def test_more_than_one_slot_per_lane():
    """M = 1030: slots past the first 1024, rows of more than 64 x 16 entries."""
    _, _, _, w, _ = _compared("big")
    assert len(w) == 1030 and min(w) >= 6 and max(w) <= 24
    tree, model = _device_tree("big", "average"), _model("big", "average")
    _check_tree(tree, model, "M 1030")
    merged = _check_cut_and_pool("big", tree, model, 0.6, "M 1030")
    assert len(merged) >= 103 and (model["log"][:, 1] >= 1024).any()


def test_two_cuts_of_one_tree():
    tree, model = _device_tree("130", "average"), _model("130", "average")
    a = _check_cut_and_pool("130", tree, model, 0.35, "cut 0.35")
    b = _check_cut_and_pool("130", tree, model, 0.8, "cut 0.8")
    assert len(a) < len(b)
    again = _check_cut_and_pool("130", tree, model, 0.35, "cut 0.35 again")
    assert np.array_equal(again.pfm.view(np.uint64), a.pfm.view(np.uint64))


def test_single_linkage_cut_is_motifs_cluster():
    from explainn_amd import motifs
    _, res, _, w, host = _compared("130")
    M = len(w)
    up = torch.triu(res.ncor, diagonal=1)
    sym = up + up.T + torch.diag(torch.diagonal(res.ncor))
    both = motifs.MotifComparison(sym, sym.clone(), res.offset, res.strand, res.overlap)
    vals = host["ncor"][np.triu_indices(M, 1)]
    clear = [t for t in np.arange(0.40, 0.70, 0.005) if np.abs(vals - t).min() >= 1e-3]
    assert clear, "no threshold is 1e-3 away from every Ncor of the set"
    thr = float(clear[0])
    assert np.abs(vals - thr).min() >= 1e-3
    want, _ = motifs.cluster(both, min_ncor=thr, min_cor=-1.0)
    labels = motifs.tree(both, torch.from_numpy(np.array(w)), "single").cut(thr)[0]
    assert np.array_equal(labels.cpu().numpy(), want) and 1 < want.max() + 1 < M


def test_merged_motifs_are_a_motif_set():
    from explainn_amd import motifs
    mats, _, _, _, _ = _compared("family")
    merged = motifs.merge(mats, min_ncor=0.6, linkage="complete")
    assert len(merged) == 4 and merged.tree.linkage == "complete"
    back = motifs.compare(merged.as_motifs(), mats)
    ncor, cor = back.ncor.cpu().numpy(), back.cor.cpu().numpy()
    fam = mt.family_set(5)[1]
    assert np.array_equal(fam[ncor.argmax(axis=1)], np.arange(4))
    for c in range(4):                                 # the pooled motif is its family's base: every copy is a piece of it
        assert cor[c, fam == c].min() >= 1 - 1e-5
    own = motifs.compare(merged.trimmed().as_motifs())
    assert np.abs(torch.diagonal(own.ncor).cpu().numpy() - 1).max() <= 1e-6
    same = motifs.merge(motifs.pack(mats), min_ncor=0.6, linkage="complete")
    assert np.array_equal(same.pfm.view(np.uint64), merged.pfm.view(np.uint64))


def test_refusals():
    from explainn_amd import motifs
    _, res, _, w, _ = _compared("family")
    with pytest.raises(ValueError, match="max_bytes"):
        motifs.tree(res, max_bytes=16 * 40 * 40 - 1)
    tree = motifs.tree(res, max_bytes=16 * 40 * 40)
    assert np.array_equal(tree.widths.cpu().numpy(), w)        # the default widths: every motif's overlap with itself
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            tree.cut(bad)
        with pytest.raises(ValueError):
            motifs.merge(list(_mats("family")), min_ncor=bad)
    with pytest.raises(ValueError):
        motifs.tree(res, linkage="ward")


def test_argument_errors_launch_nothing():
    from explainn_amd import _lib
    lib = _lib.load()
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, s = z.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = int(lib.explainn_motif_tree_workspace_bytes(4, _lib.LINKAGE_AVERAGE))
    assert need >= 2 * 4 * 4 * 8 and lib.explainn_motif_tree_workspace_bytes(4, 3) == 0
    assert lib.explainn_motif_tree_workspace_bytes(-1, 0) == 0
    assert lib.explainn_motif_tree_workspace_bytes(_lib.MOTIF_TREE_MAX_LEAVES + 1, 0) == 0
    tree = lambda M, kind, nbytes: lib.explainn_motif_tree(p, p, p, M, kind, p, p, p, p, p, p, nbytes, s)
    assert tree(-1, 0, need) == _lib.E_ARG
    assert tree(4, 3, need) == _lib.E_ARG and tree(4, -1, need) == _lib.E_ARG
    assert tree(4, 2, need - 1) == _lib.E_ARG
    assert tree(_lib.MOTIF_TREE_MAX_LEAVES + 1, 2, 1 << 40) == _lib.E_UNSUPPORTED
    assert tree(0, 2, 0) == _lib.OK
    assert lib.explainn_motif_tree_cut(p, p, p, p, -1, 5, p, p, p, p, p, s) == _lib.E_ARG
    assert lib.explainn_motif_tree_cut(p, p, p, p, 4, 0, p, p, p, p, p, s) == _lib.E_ARG
    pool = lambda M, wmax, n, span: lib.explainn_motif_tree_pool(p, p, p, p, p, p, M, wmax, n, span, p, p, s)
    assert pool(-1, 8, 0, 4) == _lib.E_ARG and pool(4, 0, 2, 4) == _lib.E_ARG and pool(4, 65, 2, 4) == _lib.E_ARG
    assert pool(4, 8, 5, 4) == _lib.E_ARG and pool(4, 8, 2, -1) == _lib.E_ARG
    assert pool(4, 8, 0, 4) == _lib.OK and pool(4, 8, 2, 0) == _lib.OK
    torch.cuda.synchronize()
    assert not z.any()


def test_two_runs_give_the_same_bytes():
    from explainn_amd import motifs
    mats = list(_mats("130"))
    runs = []
    for _ in range(2):
        merged = motifs.merge(mats, min_ncor=0.5)
        runs.append([a.tobytes() for a in _tree_arrays(merged.tree).values()] +
                    [merged.pfm.tobytes(), merged.support.tobytes(), merged.shifts.tobytes(), merged.flips.tobytes()])
    assert runs[0] == runs[1]


def test_command_line(tmp_path):
    from explainn_amd import motifs
    mats = list(_mats("family"))
    named = [("m%d" % i, "", m) for i, m in enumerate(mats)]
    path, out = os.path.join(tmp_path, "in.meme"), os.path.join(tmp_path, "out.meme")
    nwk, tsv = os.path.join(tmp_path, "out.nwk"), os.path.join(tmp_path, "out.tsv")
    motifs.write_meme(path, named)
    motifs.main(["merge", path, "-o", out, "--min-ncor", "0.6", "--linkage", "complete", "--tree", nwk, "--table", tsv])
    want = motifs.merge(motifs.read_motifs(path), min_ncor=0.6, linkage="complete").trimmed()
    got = motifs.read_meme(out)
    assert [g[0] for g in got] == ["cluster%d_n10" % c for c in range(4)]
    for (_, _, m), (_, _, pfm) in zip(got, want.as_motifs()):
        assert m.shape == pfm.shape and np.abs(m - pfm / pfm.sum(axis=1, keepdims=True)).max() <= 1e-12
    rows = [ln.rstrip("\n").split("\t") for ln in open(tsv)]
    assert rows[0] == ["Motif", "Cluster", "Strand", "Shift", "Width"] and len(rows) == 41
    assert [r[0] for r in rows[1:]] == [n[0] for n in named]
    assert [r[1] for r in rows[1:]] == ["cluster%d_n10" % (i // 10) for i in range(40)]
    assert [r[2] for r in rows[1:]] == ["-" if f else "+" for f in want.flips]
    assert [int(r[3]) for r in rows[1:]] == want.shifts.tolist()
    assert [int(r[4]) for r in rows[1:]] == [len(m) for m in mats]
    text = open(nwk).read().strip()
    assert text == want.tree.newick([n[0] for n in named]) and text.count(",") == 39
