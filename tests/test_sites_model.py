"""CPU: the numpy restatement of motif-site calling (tests/sites_model.py) against the reference-fed
fixtures and its own algebra: reverse-strand mapping, chunking, record period."""
import numpy as np
import pytest

import sites_model as sm
from oracle import explainn_oracle as eo
from oracle import interpret_oracle as io
from test_interpret_oracle import PFM_CASES, load

U, K, L = 5, 7, 40


@pytest.fixture(scope="module")
def toy():
    sd = eo.random_state_dict(U, K, L, 1, seed=3)
    g = np.random.default_rng(4)
    codes = g.integers(0, 4, size=173).astype(np.uint8)
    codes[g.random(173) < 0.03] = 4
    acts = sm.kmer_acts(sd, codes)
    thr = (0.5 * acts.max(axis=1)).astype(np.float16)
    return sd, codes, acts, thr


def _same(a, b):
    assert len(a) == len(b)
    for (pa, sa), (pb, sb) in zip(a, b):
        assert np.array_equal(pa, pb) and np.array_equal(sa, sb)


@pytest.mark.parametrize("name", PFM_CASES)
def test_lists_recount_to_the_oracle_pfm(name):
    z, m = load(name)
    lists = sm.fixed_length_lists(z["acts"], z["idxs"], z["thresholds"], m["rc"], m["cap"])
    pfm, nsites = sm.pfm_from_lists(z["codes"], lists, m["k"], m["rc"])
    ref_pfm, ref_n = io.site_pfms(z["codes"], z["acts"], z["idxs"], z["thresholds"], m["k"], m["rc"], cap=m["cap"])
    assert np.array_equal(pfm, ref_pfm) and np.array_equal(nsites, ref_n)
    assert np.array_equal(pfm, z["pfm"]) and np.array_equal(nsites, z["nsites"])


def test_kmer_activation_is_the_reference_activation():
    """The per-k-mer chain gives the reference's float16 activations of a whole window, to one ulp."""
    z, m = load("pfm_u8_k9")
    sd = {k[3:]: z[k] for k in z.files if k.startswith("sd/")}
    mine = np.stack([sm.kmer_acts(sd, row) for row in z["codes"][:12]])
    ref = z["acts"][:12]
    ulp = np.maximum(np.abs(ref.astype(np.float64)), 2.0 ** -14) * 2.0 ** -10
    assert (np.abs(mine.astype(np.float64) - ref.astype(np.float64)) <= ulp).all()
    assert (mine == ref).mean() > 0.995


def test_reverse_strand_is_the_forward_pass_on_the_reverse_complement(toy):
    sd, codes, acts, thr = toy
    rev = sm.kmer_acts(sd, codes, reverse=True)
    acts_rc = sm.kmer_acts(sd, sm.rc_codes(codes))
    assert np.array_equal(rev, acts_rc[:, ::-1])
    _same(sm.site_lists(rev, thr), sm.reverse_lists_from_rc(acts_rc, thr, K))
    P = len(codes) - K + 1
    for (pos, _), (pos_rc, _) in zip(sm.site_lists(rev, thr), sm.site_lists(acts_rc, thr)):
        assert np.array_equal(np.sort(P - 1 - pos_rc), pos)            # p = len - k - p'
    assert any(len(p) for p, _ in sm.site_lists(rev, thr))


@pytest.mark.parametrize("chunk", [1, K, 37])
def test_chunks_unite_to_the_whole(toy, chunk):
    sd, codes, acts, thr = toy
    whole = sm.site_lists(acts, thr)
    _same(sm.chunked_lists(acts, thr, chunk), whole)
    assert sum(len(p) for p, _ in whole) > 0


def test_period_drops_exactly_the_record_crossing_starts():
    sd = eo.random_state_dict(U, K, L, 1, seed=3)
    g = np.random.default_rng(8)
    M = 6
    recs = g.integers(0, 4, size=(M, L)).astype(np.uint8)
    flat = recs.reshape(-1)
    acts = sm.kmer_acts(sd, flat)
    thr = (0.25 * acts.max(axis=1)).astype(np.float16)
    P = M * L - K + 1
    mask = sm.period_mask(P, L, K)
    assert (~mask).sum() == (M - 1) * (K - 1)
    assert all((p % L) + K > L for p in np.flatnonzero(~mask))
    per_record = [sm.site_lists(sm.kmer_acts(sd, r), thr) for r in recs]
    want = [(np.concatenate([per_record[i][u][0] + i * L for i in range(M)]),
             np.concatenate([per_record[i][u][1] for i in range(M)])) for u in range(U)]
    _same(sm.site_lists(acts, thr, mask), want)
    # without the mask some record-crossing start is a site: the mask is what removes it
    assert sum(len(p) for p, _ in sm.site_lists(acts, thr)) > sum(len(p) for p, _ in want)
    # a chunk that starts on a record boundary sees the same phase
    _same(sm.chunked_lists(acts, thr, 2 * L, mask), want)
    assert np.array_equal(sm.period_mask(2 * L, L, K, first=2 * L), mask[2 * L:4 * L])
