"""GPU: de novo word discovery (csrc/words.hip through explainn_word_counts / explainn_word_test /
explainn_word_sites, explainn_amd/discover.py and `python -m explainn_amd.discover`) against the numpy model
tests/words_model.py.  Counts, sites, count matrices, erased sequences and flags are compared with array_equal;
log p-values within enrichment_model.log_tolerance(Np + Nc)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import enrichment_model as em  # noqa: E402
import words_model as wm  # noqa: E402

pytestmark = pytest.mark.gpu
MARK = 0xA5                      # behind every sequence: a read of it would raise flag bit 0
GUARD = 64


def _dv():
    from explainn_amd import discover
    return discover


def _dev(codes, offsets, seq_len=None):
    """(seq view of seq_len bytes of a tensor with GUARD marker bytes behind it, offsets) on the device."""
    codes = np.asarray(codes, dtype=np.uint8)
    seq_len = len(codes) if seq_len is None else seq_len
    full = torch.from_numpy(np.concatenate([codes, np.full(GUARD, MARK, np.uint8)])).cuda()
    return full[:seq_len], torch.from_numpy(np.asarray(offsets, dtype=np.int64)).cuda()


def _flags():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def _edge(k):
    return wm.flatten(wm.edge_records(k))


# ---------------------------------------------------------------- counts
@pytest.mark.parametrize("both", [True, False], ids=["both", "fwd"])
@pytest.mark.parametrize("k", range(3, 11))
def test_counts_every_width(k, both):
    codes, off = _edge(k)
    want, want_flags = wm.word_counts(codes, off, k, both)
    seq, offs = _dev(codes, off)
    f = _flags()
    got = _dv().word_counts(seq, offs, k, both, flags=f)
    assert got.dtype == torch.int32 and got.shape == (4 ** k,)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(f.item()) == want_flags == 1                      # the byte of 7
    # the long record alone: its word, repeated across the passes, is counted once
    long = wm.edge_records(k)[9]
    one = _dv().word_counts(*_dev(*wm.flatten([long])), k, both).cpu().numpy()
    assert one.max() == 1 and np.array_equal(one, wm.word_counts(*wm.flatten([long]), k, both)[0])


@pytest.mark.parametrize("k", [7, 8])                            # the LDS count table and the direct adds
def test_counts_accumulate_and_do_not_depend_on_the_split(k):
    recs = wm.edge_records(k)
    want = wm.word_counts(*wm.flatten(recs), k)[0]
    for cuts in ([0, len(recs) // 2, len(recs)], [0, 1, 9, 10, 200, len(recs)], [0, len(recs)]):
        out = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
        for a, b in zip(cuts[:-1], cuts[1:]):
            same = _dv().word_counts(*_dev(*wm.flatten(recs[a:b])), k, True, out=out)
            assert same is out
        assert np.array_equal(out.cpu().numpy(), want), cuts
    twice = _dv().word_counts(*_dev(*wm.flatten(recs)), k, True, out=out)
    assert np.array_equal(twice.cpu().numpy(), 2 * want)
    # no record at all, and records only of no live start
    assert int(_dv().word_counts(*_dev(np.full(1, 4, np.uint8), [0]), k).sum()) == 0
    assert int(_dv().word_counts(*_dev(np.full(30, 4, np.uint8), [0, 10, 30]), k).sum()) == 0


@pytest.mark.parametrize("k", [6, 8])
def test_forged_offsets_are_skipped(k):
    g = np.random.default_rng(k)
    codes = g.integers(0, 4, size=400).astype(np.uint8)
    seq_len = 300                                                # the tensor is longer: no read leaves the allocation
    off = np.array([0, 40, 25, 70, 110, seq_len + 5, 150, 200, seq_len], dtype=np.int64)
    good = [(0, 40), (25, 70), (70, 110), (150, 200), (200, seq_len)]
    want, want_flags = wm.word_counts(codes, off, k, True, seq_len=seq_len)
    plain = wm.word_counts(*wm.flatten([codes[a:b] for a, b in good]), k)[0]
    assert want_flags == 2 and np.array_equal(want, plain)       # the other records' counts are unchanged
    seq, offs = _dev(codes, off, seq_len)
    f = _flags()
    got = _dv().word_counts(seq, offs, k, True, flags=f)
    assert np.array_equal(got.cpu().numpy(), want) and int(f.item()) == 2
    # the sites pass skips them too
    seed = int(np.argmax(want))
    wpfm, wtot, wout, wflags = wm.word_sites(codes[:seq_len], off, k, seed, 0, True, seq_len=seq_len)
    f = _flags()
    pfm, tot, out = _dv().word_sites(seq, offs, k, seed, 0, True, flags=f)
    assert np.array_equal(pfm.cpu().numpy(), wpfm) and np.array_equal(tot.cpu().numpy(), wtot)
    assert np.array_equal(out.cpu().numpy(), wout) and int(f.item()) == wflags == 2


# ---------------------------------------------------------------- the test
@functools.lru_cache(maxsize=None)
def _planted_tables(plant, k):
    prim, ctrl = wm.planted_case(plant)
    return wm.word_counts(*wm.flatten(prim), k)[0], wm.word_counts(*wm.flatten(ctrl), k)[0]


def _check_test(pos, neg, Np, Nc, min_count):
    logp, best, n_tested, best_lp = wm.word_test(pos, neg, Np, Nc, min_count)
    got = _dv().word_test(torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), Np, Nc, min_count)
    glogp, gbest, gtested, gbest_lp = (t.cpu().numpy() for t in got)
    tol = em.log_tolerance(Np + Nc)
    assert int(gtested) == n_tested
    assert np.array_equal(glogp != 0.0, logp != 0.0) and np.all(glogp <= 0.0)
    assert np.max(np.abs(glogp - logp), initial=0.0) <= tol
    if best < 0:
        assert int(gbest) == -1 and float(gbest_lp) == 0.0
        return
    assert float(gbest_lp) == glogp[int(gbest)] == glogp.min()
    assert abs(logp[int(gbest)] - best_lp) <= tol
    assert int(gbest) == int(np.flatnonzero(glogp == glogp.min())[0])        # the tie rule on the device's own values
    if wm.best_gap(logp, pos, neg) > em.MIN_GAP:
        assert int(gbest) == best


@pytest.mark.parametrize("k", [6, 7, 8])
@pytest.mark.parametrize("plant", wm.PLANTS)
def test_word_test_on_the_planted_tables(plant, k):
    pos, neg = _planted_tables(plant, k)
    _check_test(pos, neg, 40, 60, 3)


def test_word_test_edges():
    pos, neg = _planted_tables(wm.PLANTS[0], 6)
    _check_test(pos, neg, 40, 60, 41)                             # min_count excludes everything: best -1
    _check_test(np.array([9], np.int32), np.array([1], np.int32), 40, 60, 3)       # n_words = 1
    _check_test(np.array([0], np.int32), np.array([0], np.int32), 40, 60, 0)
    # equal counts at several codes: the lowest code, and bit-equal values
    pos = np.array([0, 5, 9, 9, 2, 9], np.int32)
    neg = np.array([3, 0, 1, 1, 0, 1], np.int32)
    _check_test(pos, neg, 40, 60, 3)
    got = _dv().word_test(torch.from_numpy(pos).cuda(), torch.from_numpy(neg).cuda(), 40, 60, 3)
    assert int(got[1]) == 2 and float(got[0][2]) == float(got[0][3]) == float(got[0][5])
    g = np.random.default_rng(3)                                  # more words than one pass of the grid takes
    n = 4 ** 9 + 1000
    pos = np.where(g.random(n) < 0.03, g.integers(5, 30, size=n), g.integers(0, 5, size=n)).astype(np.int32)
    _check_test(pos, g.integers(0, 12, size=n).astype(np.int32), 5000, 7000, 5)


# ---------------------------------------------------------------- sites
def _site_records(k, seed):
    """Records around one seed: at both ends of a record, '-'-only, overlapping (poly-A, two letters), next to an N,
    across the tile boundaries of a long record, a byte of 7, and 30 random ones."""
    g = np.random.default_rng([k, seed])
    rnd = lambda n, hi=4: g.integers(0, hi, size=n).astype(np.uint8)
    s = np.array(wm.digits(seed, k), np.uint8)
    r = (3 - s)[::-1]
    near = s.copy()
    near[k // 2] = (near[k // 2] + 1) % 4                        # one mismatch: a site under some masks
    recs = [np.concatenate([s, rnd(11), s]), r.copy(), np.concatenate([rnd(3), r, rnd(3)]), np.zeros(2 * k + 3, np.uint8),
            rnd(120, 2), np.concatenate([s, np.full(1, 4, np.uint8), s[:-1], np.full(2, 4, np.uint8), s]),
            np.concatenate([near, rnd(5), near[::-1]]), rnd(0), rnd(k - 1), s.copy()]
    long = rnd(3 * wm.SPAN + 7)
    for at in (wm.SPAN - k, wm.SPAN - 1, wm.SPAN + k, 2 * wm.SPAN - k // 2, 3 * wm.SPAN + 7 - k):
        long[at:at + k] = s if at % 2 else r
    odd = rnd(40)
    odd[20] = 7
    return recs + [long, odd] + [rnd(int(g.integers(20, 300))) for _ in range(30)]


@functools.lru_cache(maxsize=None)
def _site_seeds(k):
    g = np.random.default_rng(k)
    seeds = [0, int(g.integers(4 ** k))]                         # poly-A and a random word
    if k % 2 == 0:
        half = wm.digits(int(g.integers(4 ** (k // 2))), k // 2)
        seeds.append(wm.code_of("".join("ACGT"[b] for b in half + [3 - b for b in half[::-1]])))    # a palindrome
    return seeds


@pytest.mark.parametrize("both", [True, False], ids=["both", "fwd"])
@pytest.mark.parametrize("k", [3, 6, 8, 10])
def test_sites(k, both):
    g = np.random.default_rng(100 + k)
    for seed in _site_seeds(k):
        codes, off = wm.flatten(_site_records(k, seed))
        seq, offs = _dev(codes, off)
        for accept in (0, (1 << (4 * k)) - 1, int(g.integers(0, 1 << (4 * k), dtype=np.uint64))):
            wpfm, wtot, wout, wflags = wm.word_sites(codes, off, k, seed, accept, both)
            f = _flags()
            pfm, tot, out = _dv().word_sites(seq, offs, k, seed, accept, both, flags=f)
            what = (k, both, seed, hex(accept))
            assert np.array_equal(tot.cpu().numpy(), wtot), what
            assert np.array_equal(pfm.cpu().numpy(), wpfm), what
            assert np.array_equal(out.cpu().numpy(), wout), what
            assert int(f.item()) == wflags == 1, what
            assert wtot[0] > 0 and np.all(wpfm.sum(axis=1) == wtot[0])
        # seq_out = NULL and pfm = NULL leave the other outputs as they were
        pfm2, tot2, none = _dv().word_sites(seq, offs, k, seed, accept, both, erase=False)
        assert none is None and torch.equal(pfm2, pfm) and torch.equal(tot2, tot)
        none, tot3, out3 = _dv().word_sites(seq, offs, k, seed, accept, both, want_pfm=False)
        assert none is None and torch.equal(tot3, tot) and torch.equal(out3, out)


@pytest.mark.parametrize("k", [3, 6, 8, 10])
def test_sites_named_inputs(k):
    dv = _dv()
    # poly-A under AAA...: every start is one '+' site and every base is erased
    n = wm.SPAN + 2 * k
    pfm, tot, out = dv.word_sites(*_dev(np.zeros(n, np.uint8), [0, n]), k, 0, 0, True)
    assert tot.tolist() == [n - k + 1, 1] and bool((out == 4).all())
    assert pfm[:, 0].tolist() == [n - k + 1] * k and int(pfm[:, 1:].sum()) == 0
    # a '-'-only site: the count matrix is the seed's own bases
    seed = _site_seeds(k)[1]
    rec = np.array(wm.digits(wm.rc(seed, k), k), np.uint8)
    assert wm.rc(seed, k) != seed
    pfm, tot, out = dv.word_sites(*_dev(rec, [0, k]), k, seed, 0, True)
    assert tot.tolist() == [1, 1] and pfm.argmax(dim=1).tolist() == wm.digits(seed, k) and bool((out == 4).all())
    pfm, tot, out = dv.word_sites(*_dev(rec, [0, k]), k, seed, 0, False)
    assert tot.tolist() == [0, 0] and int(pfm.sum()) == 0 and np.array_equal(out.cpu().numpy(), rec)
    if k % 2 == 0:                                               # a palindromic seed: one '+' site per start
        pal = _site_seeds(k)[2]
        rec = np.array(wm.digits(pal, k) * 2, np.uint8)
        pfm, tot, out = dv.word_sites(*_dev(rec, [0, 2 * k]), k, pal, 0, True)
        assert tot.tolist() == [2, 1] and pfm.argmax(dim=1).tolist() == wm.digits(pal, k)


# ---------------------------------------------------------------- discover
FIELDS = ("width", "seed", "accept", "pos", "neg", "n_tests", "nsites", "tp", "fp")


def _check_discovery(found, rounds, Np, Nc):
    tol = em.log_tolerance(Np + Nc)
    assert len(found) == len(rounds) and (found.Np, found.Nc) == (Np, Nc)
    for i, r in enumerate(rounds):
        assert found.word[i] == r["word"]
        for f in FIELDS:
            assert int(getattr(found, f)[i]) == r[f], (i, f)
        assert np.array_equal(found.pfm[i], r["pfm"]) and found.pfm[i].dtype == np.int64
        assert abs(found.log_pvalue[i] - r["log_pvalue"]) <= tol
        assert abs(found.motif_log_pvalue[i] - r["motif_log_pvalue"]) <= tol
        assert abs(np.log(found.evalue[i]) - (r["log_pvalue"] + np.log(r["n_tests"]))) <= tol + 1e-12


@pytest.mark.parametrize("plant", wm.PLANTS)
def test_discover_equals_the_model_loop(plant):
    prim, ctrl = wm.planted_case(plant)
    rounds, n_last = wm.discover(prim, ctrl, widths=(6, 7, 8), min_count=3)
    assert len(rounds) == 1
    found, p_out, c_out = _dv().discover(prim, ctrl, widths=(6, 7, 8), min_count=3, return_sequences=True)
    _check_discovery(found, rounds, 40, 60)
    assert found.n_tests_last == n_last and found.flags == 0
    assert np.array_equal(p_out.cpu().numpy(), rounds[-1]["primary_out"])
    assert np.array_equal(c_out.cpu().numpy(), rounds[-1]["control_out"])
    # a second run gives the same bits
    again = _dv().discover(prim, ctrl, widths=(6, 7, 8), min_count=3)
    assert again.word == found.word and np.array_equal(again.log_pvalue, found.log_pvalue)
    assert np.array_equal(again.motif_log_pvalue, found.motif_log_pvalue) and np.array_equal(again.evalue, found.evalue)
    assert all(np.array_equal(a, b) for a, b in zip(again.pfm, found.pfm))
    # forward strand only
    rounds, _ = wm.discover(prim, ctrl, widths=(6, 7, 8), min_count=3, both=False)
    _check_discovery(_dv().discover(prim, ctrl, widths=(6, 7, 8), min_count=3, strands="fwd"), rounds, 40, 60)


def test_discover_round_by_round():
    """Two plants, more than one round: the erased sequences of every round, by stopping the loop after it; and a
    case whose accept mask is not empty."""
    prim, ctrl = wm.two_plant_case()
    rounds, _ = wm.discover(prim, ctrl, widths=(6, 7, 8), min_count=3)
    assert len(rounds) >= 2
    for n in range(1, len(rounds) + 1):
        found, p_out, c_out = _dv().discover(prim, ctrl, widths=(6, 7, 8), min_count=3, max_motifs=n,
                                             return_sequences=True)
        _check_discovery(found, rounds[:n], 40, 60)
        assert np.array_equal(p_out.cpu().numpy(), rounds[n - 1]["primary_out"])
        assert np.array_equal(c_out.cpu().numpy(), rounds[n - 1]["control_out"])
    none, p_out, _ = _dv().discover(prim, ctrl, widths=(6, 7, 8), min_count=3, max_motifs=0, return_sequences=True)
    assert len(none) == 0 and np.array_equal(p_out.cpu().numpy(), wm.flatten(prim)[0])
    prim, ctrl = wm.variant_case()
    rounds, _ = wm.discover(prim, ctrl, widths=(6, 7), min_count=3)
    assert rounds[0]["accept"] != 0
    _check_discovery(_dv().discover(prim, ctrl, widths=(6, 7), min_count=3), rounds, 50, 70)


def test_discover_finds_nothing_in_random_sets():
    prim, ctrl = wm.random_case(0)
    found = _dv().discover(prim, ctrl, widths=(6, 7, 8), min_count=3)
    assert len(found) == 0 and found.as_motifs() == [] and found.table() == []
    assert found.n_tests_last == wm.discover(prim, ctrl, widths=(6, 7, 8), min_count=3)[1]


def test_discover_with_shuffled_control():
    from explainn_amd.sequence import dinucleotide_shuffle_device
    prim, _ = wm.planted_case(wm.PLANTS[0])
    shuf = dinucleotide_shuffle_device(torch.from_numpy(np.stack(prim)).cuda(), 2, 11).reshape(-1, 60).cpu().numpy()
    assert shuf.shape == (80, 60)
    rounds, n_last = wm.discover(prim, list(shuf), widths=(6, 7, 8), min_count=3)
    found = _dv().discover(prim, None, shuffles=2, seed=11, widths=(6, 7, 8), min_count=3)
    assert len(rounds) >= 1 and (found.shuffles, found.seed0) == (2, 11)
    _check_discovery(found, rounds, 40, 80)
    assert found.n_tests_last == n_last


def test_discovered_motifs_feed_the_other_tools(tmp_path):
    from explainn_amd import motifs, pwmsites
    prim, ctrl = wm.planted_case(wm.PLANTS[0])
    found = _dv().discover(prim, ctrl, widths=(6, 7, 8), min_count=3)
    ms = found.as_motifs()
    assert ms[0][0] == "word1_" + found.word[0] and ms[0][2].shape == (found.width[0], 4)
    cmp = motifs.compare(ms)
    assert float(cmp.ncor[0, 0]) > 0.999
    calls = pwmsites.scan_motifs(ms, wm.flatten(prim)[0], pvalue=1e-3)
    assert calls.units == len(ms) and len(calls) >= found.tp[0] // 2
    # the command line: FASTA in, MEME and table out
    def fasta(path, recs):
        with open(path, "w") as fh:
            for i, r in enumerate(recs):
                fh.write(">r%d\n%s\n" % (i, "".join("ACGTN"[b] for b in r)))
    fasta(tmp_path / "p.fa", prim)
    fasta(tmp_path / "c.fa", ctrl)
    _dv().main([str(tmp_path / "p.fa"), "--control", str(tmp_path / "c.fa"), "--min-count", "3", "--widths", "6,7,8",
                "-o", str(tmp_path / "out.meme"), "--table", str(tmp_path / "out.tsv")])
    back = motifs.read_meme(str(tmp_path / "out.meme"))
    assert [m[0] for m in back] == [m[0] for m in ms]
    for (_, _, got), (_, _, want) in zip(back, ms):
        assert np.array_equal(got, want / want.sum(axis=1, keepdims=True))
    lines = open(tmp_path / "out.tsv").read().splitlines()
    assert lines[0].split("\t") == list(_dv().COLUMNS) and len(lines) == 1 + len(found)
    assert lines[1].split("\t")[:5] == [ms[0][0], found.word[0], str(found.width[0]), str(found.pos[0]), str(found.neg[0])]
