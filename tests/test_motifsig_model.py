"""CPU checks of motif significance: the numpy model of tests/motifsig_model.py against its own plain loops
and against the properties the statistic must have, and the host code of explainn_amd.motifs (the q-value
step on host tensors, the argument checks that run before any device call).  The device call itself is
tests/test_gpu_motifsig.py."""
import numpy as np
import pytest
import torch

import motifs_model as mm
import motifsig_model as sm
from explainn_amd import motifs

DEPTH = 20


def _columns(rng, w):
    return np.stack([rng.multinomial(DEPTH, p) for p in rng.dirichlet([0.3] * 4, size=w)]).astype(np.float64) \
        if w else np.zeros((0, 4))


def _packed(q, t):
    wmax = max([len(m) for m in q + t] + [1])
    x, xw = mm.pack(q, wmax)
    y, yw = mm.pack(t, wmax)
    return x, xw, y, yw


@pytest.mark.parametrize("both", [True, False])
@pytest.mark.parametrize("bins,min_overlap,pc", [(4, 1, 0.0), (9, 3, 1.0)])
def test_loops_and_vectorised_agree(bins, min_overlap, pc, both):
    rng = np.random.default_rng(bins)
    q = [_columns(rng, w) for w in (5, 0, 1, 7)]
    t = [_columns(rng, w) for w in (6, 3, 0, 1)] + [q[0], mm.revcomp(q[3])[1:]]
    x, xw, y, yw = _packed(q, t)
    res = sm.significance(x, xw, y, yw, min_overlap, pc, both, bins)
    for a in range(len(q)):
        for b in range(len(t)):
            one = sm.pair_loops(q[a], t, b, min_overlap, pc, both, bins)
            for k in ("offset", "strand", "overlap", "score", "n_align"):
                assert one[k] == res[k][a, b], (k, a, b)
            for k in ("p_align", "pvalue"):
                assert abs(one[k] - res[k][a, b]) <= 1e-12 * one[k], (k, a, b)
    # the self form: the queries are the database
    me = sm.significance(x, xw, None, None, min_overlap, pc, both, bins)
    two = sm.significance(x, xw, x, xw, min_overlap, pc, both, bins)
    assert np.array_equal(me["pvalue"], two["pvalue"]) and me["N"] == int(xw.sum()) * (2 if both else 1)
    one = sm.pair_loops(q[0], q, 3, min_overlap, pc, both, bins)
    assert abs(one["pvalue"] - me["pvalue"][0, 3]) <= 1e-12 * one["pvalue"]


def test_precomputed_column_scores_drive_the_later_stages():
    rng = np.random.default_rng(3)
    q = [_columns(rng, w) for w in (8, 5)]
    t = [_columns(rng, w) for w in (9, 4, 12)]
    x, xw, y, yw = _packed(q, t)
    cs, raw = sm.column_scores(x, xw, y, yw, 0.0, True, 16)
    assert cs.shape == (2, 12, 2, 12, 3) and (cs[0, 8:] == sm.NONE).all() and (cs[:, :, :, 4:, 1] == sm.NONE).all()
    assert np.isnan(raw[cs == sm.NONE]).all() and (np.abs(raw[cs != sm.NONE] - 8.0) <= 8.0 + 1e-9).all()
    a = sm.significance(x, xw, y, yw, 5, 0.0, True, 16)
    b = sm.significance(x, xw, y, yw, 5, 0.0, True, 16, colscore=cs.reshape(-1))
    assert np.array_equal(a["pvalue"], b["pvalue"]) and np.array_equal(a["score"], b["score"])
    moved = cs.copy()
    moved[0, 0, 0, 0, 0] = (int(moved[0, 0, 0, 0, 0]) + 1) % 17       # one entry of the null and of one diagonal
    c = sm.significance(x, xw, y, yw, 5, 0.0, True, 16, colscore=moved)
    assert not np.array_equal(a["hist"], c["hist"])


def test_planted_motifs():
    wmax, bins = 19, 100
    rng = np.random.default_rng(19)
    full = _columns(rng, wmax)
    cut = wmax // 3
    q = [full, full[cut:], full[:wmax - cut], _columns(rng, 0)]
    t = [_columns(rng, int(w)) for w in rng.integers(6, wmax + 1, size=40)]
    t[3], t[11], t[20] = full, mm.revcomp(full), full[cut:]
    x, xw, y, yw = _packed(q, t)
    r = sm.significance(x, xw, y, yw, 5, 0.0, True, bins)
    got = lambda a, b: (r["offset"][a, b], r["strand"][a, b], r["overlap"][a, b])
    assert got(0, 3) == (0, 0, wmax) and r["pvalue"][0, 3] < 1e-10            # an identical copy
    assert got(0, 11) == (0, 1, wmax) and r["pvalue"][0, 11] < 1e-10          # its reverse complement
    assert got(1, 3) == (cut, 0, wmax - cut) and r["pvalue"][1, 3] < 1e-10    # a cut sub-motif inside the full one
    assert got(0, 20) == (-cut, 0, wmax - cut) and r["pvalue"][0, 20] < 1e-10
    assert got(2, 3) == (0, 0, wmax - cut) and r["pvalue"][2, 3] < 1e-10
    assert r["score"][0, 3] == wmax * bins                                   # every column correlates at 1
    # a query without width: p = 1, zeros
    assert (r["pvalue"][3] == 1).all() and not r["offset"][3].any() and not r["overlap"][3].any()
    assert (r["qvalue"][3] == 1).all() and (r["evalue"][3] == len(t)).all()
    # each h[q][i] sums to 1 and SF(0) = 1
    wq = [len(m) for m in q]
    for a in range(3):
        h = r["hist"][a, :wq[a]] / r["N"]
        assert (r["hist"][a, :wq[a]].sum(axis=1) == r["N"]).all() and not r["hist"][a, wq[a]:].any()
        for sf in sm.range_sf(h):
            assert abs(sf[0] - 1) <= 1e-12 and (np.diff(sf) <= 0).all() and sf[-1] >= 0
    assert r["N"] == 2 * sum(len(m) for m in t)
    assert ((r["pvalue"] >= r["p_align"]) | (r["pvalue"] >= 1 - 1e-12)).all()          # the Sidak step only raises


def test_qvalues():
    rng = np.random.default_rng(5)
    p = rng.random((7, 33)) ** 4
    p[0, :5] = p[0, 5]                                  # ties
    p[1] = 1.0
    p[2, 3] = 0.0
    qv = sm.bh_qvalues(p)
    assert (qv >= p).all() and (qv <= 1).all()
    for a in range(len(p)):                             # monotone in p
        order = np.argsort(p[a], kind="stable")
        assert (np.diff(qv[a][order]) >= 0).all()
    # the textbook statement, row by row
    for a in range(len(p)):
        order = np.argsort(p[a], kind="stable")
        T = p.shape[1]
        want = np.empty(T)
        for k in range(T):
            want[order[k]] = min(min(1.0, p[a][order[j]] * T / (j + 1)) for j in range(k, T))
        assert np.array_equal(qv[a], want)
    # the function the package runs on the device, here on host tensors
    got = motifs.benjamini_hochberg(torch.from_numpy(p))
    assert got.dtype == torch.float64 and np.array_equal(got.numpy(), qv)
    assert motifs.benjamini_hochberg(torch.zeros((0, 4), dtype=torch.float64)).shape == (0, 4)
    assert motifs.benjamini_hochberg(torch.zeros((3, 0), dtype=torch.float64)).shape == (3, 0)
    assert np.array_equal(motifs.benjamini_hochberg(p[:1]).numpy(), qv[:1])
    with pytest.raises(ValueError):
        motifs.benjamini_hochberg(torch.zeros(4))


@pytest.mark.parametrize("bins,both", [(100, True), (16, True), (128, False)])
def test_calibration_on_unrelated_motifs(bins, both):
    """Unrelated random motifs: p < 0.05 in no more than 8 % of the pairs (the Sidak step and the independence
    of columns make the test conservative; a numpy prototype of the statistic gave 0.02 - 0.05)."""
    rng = np.random.default_rng(bins)
    q = [_columns(rng, int(w)) for w in rng.integers(6, 21, size=40)]
    t = [_columns(rng, int(w)) for w in rng.integers(6, 21, size=60)]
    x, xw, y, yw = _packed(q, t)
    r = sm.significance(x, xw, y, yw, 5, 0.0, both, bins)
    share = float((r["pvalue"] < 0.05).mean())
    print("bins %d both %d: share of pairs with p < 0.05: %.4f" % (bins, both, share))
    assert share <= 0.08
    assert (r["pvalue"] > 0).all() and (r["pvalue"] <= 1).all()


def test_argument_checks_before_any_device_call():
    m = [np.ones((5, 4))]
    for bad in (dict(bins=1), dict(bins=129), dict(bins=10.5), dict(min_overlap=0), dict(pseudocount=-1.0),
                dict(workspace_bytes=0)):
        with pytest.raises(ValueError):
            motifs.significance(m, m, **bad)
    with pytest.raises(ValueError):
        motifs.annotate(m, m, by="evalue")
    with pytest.raises(ValueError):
        motifs.annotate(m, m, by="pvalue", max_qvalue=1.5)
    with pytest.raises(ValueError):
        motifs.annotate(m, m, by="pvalue", bins=0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            motifs.significance(m, m)
    # annotate over a result computed elsewhere needs no device
    p = torch.tensor([[0.5, 1e-9, 1e-3, 1e-9], [1.0, 0.9, 0.8, 0.7]], dtype=torch.float64)
    z = torch.zeros((2, 4), dtype=torch.int16)
    sig = motifs.MotifSignificance(p, p * 4, motifs.benjamini_hochberg(p), z, z + 1, z + 5, z.to(torch.int32))
    hits = motifs.annotate(sig, by="pvalue", top=3)
    assert [h["target"] for h in hits[0]] == [1, 3, 2] and hits[1] == []       # ties to the lower target index
    assert hits[0][0]["strand"] == 1 and hits[0][0]["overlap"] == 5 and "ncor" not in hits[0][0]
    assert hits[0][2]["qvalue"] == pytest.approx(1e-3 * 4 / 3) and hits[0][0]["evalue"] == pytest.approx(4e-9)
    assert [h["target"] for h in motifs.annotate(sig, by="pvalue", top=1)[0]] == [1]
    assert [len(h) for h in motifs.annotate(sig, by="pvalue", max_qvalue=1.0, top=9)] == [4, 4]
