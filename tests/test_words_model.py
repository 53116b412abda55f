"""CPU: the model of de novo word discovery (tests/words_model.py) against independent restatements -- a sliding
string window, enumeration of all 4^k windows, a per-base brute force of the erasure --, its loop on the planted
cases, the C boundary of the three word entry points and their argument refusals, which need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import words_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "ACGTN"


# ---------------------------------------------------------------- strings, the second statement
def reverse_complement(word):
    return "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[ch] for ch in reversed(word))


def string_counts(records, k, both):
    """{word: records that contain it}: a sliding window over strings, the canonical word the smaller string (the
    letters sort like the codes)."""
    out = {}
    for rec in records:
        text = "".join(LETTERS[min(int(b), 4)] for b in rec)
        seen = set()
        for s in range(len(text) - k + 1):
            w = text[s:s + k]
            if "N" not in w:
                seen.add(min(w, reverse_complement(w)) if both else w)
        for w in seen:
            out[w] = out.get(w, 0) + 1
    return out


@pytest.mark.parametrize("both", [True, False], ids=["both", "fwd"])
@pytest.mark.parametrize("k", [3, 4, 7, 10])
def test_counts_equal_a_sliding_string_window(k, both):
    recs = wm.edge_records(k)[:40]
    codes, off = wm.flatten(recs)
    counts, flags = wm.word_counts(codes, off, k, both)
    want = string_counts(recs, k, both)
    assert flags == 1                                             # the byte of 7
    assert int(np.count_nonzero(counts)) == len(want)
    for w, n in want.items():
        assert counts[wm.code_of(w)] == n, w
    if both:
        for w in np.flatnonzero(counts):
            assert int(w) == wm.canonical(int(w), k)              # non-canonical entries stay 0
    # one count for the word the long record repeats across its passes, in a set of its own
    long = recs[9]
    assert len(long) == 2 * wm.SPAN + k + 3
    c1, _ = wm.word_counts(*wm.flatten([long]), k, both)
    assert c1.max() == 1


def test_rc_canonical_and_palindromes():
    g = np.random.default_rng(0)
    for k in range(3, 11):
        for c in g.integers(0, 4 ** k, size=50):
            c = int(c)
            w = wm.word_string(c, k)
            assert wm.code_of(w) == c and wm.rc(wm.rc(c, k), k) == c
            assert wm.word_string(wm.rc(c, k), k) == reverse_complement(w)
            assert wm.canonical(c, k) == wm.canonical(wm.rc(c, k), k) <= c
    for k in (3, 4, 5, 6):
        pal = [c for c in range(4 ** k) if wm.rc(c, k) == c]
        assert len(pal) == (0 if k % 2 else 4 ** (k // 2))        # a free half at even widths, none at odd ones
    assert wm.rc(wm.code_of("TGACGTCA"), 8) == wm.code_of("TGACGTCA")


@pytest.mark.parametrize("k", [3, 4])
def test_pattern_matcher_against_all_windows(k):
    g = np.random.default_rng(k)
    for _ in range(12):
        seed = int(g.integers(4 ** k))
        accept = int(g.integers(0, 1 << (4 * k)))
        sd = wm.word_string(seed, k)
        for c in range(4 ** k):
            w = wm.word_string(c, k)
            diff = [i for i in range(k) if w[i] != sd[i]]
            want = not diff or (len(diff) == 1 and bool(accept >> (4 * diff[0] + "ACGT".index(w[diff[0]])) & 1))
            assert wm.matches(c, k, seed, accept) == want, (sd, w, hex(accept))


def _covered_brute(rec, k, seed, accept, both):
    """Per base: is it covered by a live window that matches on either requested strand?"""
    cov = np.zeros(len(rec), dtype=bool)
    for p in range(len(rec)):
        for s in range(max(0, p - k + 1), min(p, len(rec) - k) + 1):
            w = rec[s:s + k]
            if np.any(w >= 4):
                continue
            fwd = sum(int(b) * 4 ** (k - 1 - i) for i, b in enumerate(w))
            rev = sum((3 - int(b)) * 4 ** i for i, b in enumerate(w))
            if wm.matches(fwd, k, seed, accept) or (both and wm.matches(rev, k, seed, accept)):
                cov[p] = True
    return cov


@pytest.mark.parametrize("both", [True, False], ids=["both", "fwd"])
def test_sites_pass_against_a_per_base_brute_force(both):
    g = np.random.default_rng(5)
    for k in (3, 5):
        recs = [g.integers(0, 3, size=int(n)).astype(np.uint8) for n in (0, k - 1, k, 30, 41)] + [np.zeros(12, np.uint8)]
        recs[3][7:9] = 4
        codes, off = wm.flatten(recs)
        for accept in (0, (1 << (4 * k)) - 1, int(g.integers(0, 1 << (4 * k)))):
            seed = int(g.integers(3 ** 2))                        # few letters, short seed: many sites and overlaps
            pfm, totals, out, flags = wm.word_sites(codes, off, k, seed, accept, both)
            assert flags == 0 and out[-1] == 4
            nrec = 0
            for r, rec in enumerate(recs):
                cov = _covered_brute(rec, k, seed, accept, both)
                got = out[off[r]:off[r + 1]]
                assert np.array_equal(got, np.where(cov, 4, rec)), (k, r, hex(accept))
                nrec += bool(cov.any())
            assert totals[1] == nrec and np.all(pfm.sum(axis=1) == totals[0])
    # poly-A under AAA: every start is a '+' site, every base is erased
    pfm, totals, out, _ = wm.word_sites(np.zeros(9, np.uint8), [0, 9], 3, 0, 0, True)
    assert totals.tolist() == [7, 1] and np.all(out == 4) and pfm[:, 0].tolist() == [7, 7, 7]
    # a '-'-only site: the window is the reverse complement of the seed, the pfm counts the seed's own bases
    seed = wm.code_of("GATAAG")
    rec = np.array(wm.digits(wm.rc(seed, 6), 6), np.uint8)
    pfm, totals, out, _ = wm.word_sites(rec, [0, 6], 6, seed, 0, True)
    assert totals.tolist() == [1, 1] and [int(np.argmax(row)) for row in pfm] == wm.digits(seed, 6)
    assert wm.word_sites(rec, [0, 6], 6, seed, 0, False)[1].tolist() == [0, 0]


@pytest.mark.parametrize("plant", wm.PLANTS)
def test_loop_finds_the_planted_word(plant):
    prim, ctrl = wm.planted_case(plant)
    rounds, n_tests = wm.discover(prim, ctrl, widths=(6, 7, 8), min_count=3)
    assert len(rounds) == 1                                       # one motif, then the stop
    first = rounds[0]
    assert first["word"] in plant or first["word"] in reverse_complement(plant)
    assert first["tp"] >= first["pos"] >= 3 and first["fp"] >= first["neg"]
    assert first["log_pvalue"] + np.log(first["n_tests"]) <= np.log(0.05)
    assert np.all(first["pfm"].sum(axis=1) == first["nsites"])
    # the erased sets hold the seed no more
    k = first["width"]
    p_off = np.arange(len(prim) + 1) * 60
    assert wm.word_counts(first["primary_out"], p_off, k)[0][first["seed"]] == 0
    # a looser accept cut-off keeps the seed and cannot lose sites
    loose, _ = wm.discover(prim, ctrl, widths=(6, 7, 8), min_count=3, accept_pvalue=0.5, max_motifs=1)
    assert loose[0]["seed"] == first["seed"] and loose[0]["nsites"] >= first["nsites"]


def test_accept_mask_takes_an_enriched_neighbour():
    """GATAAG in 24 primary records and its neighbour GATTAG (position 3, base T: bit 15) in 12 more."""
    prim, ctrl = wm.variant_case()
    rounds, _ = wm.discover(prim, ctrl, widths=(6,), min_count=3, max_motifs=1)
    first = rounds[0]
    assert first["word"] in ("GATAAG", "CTTATC") and first["accept"] != 0
    i, b = (3, 3) if first["word"] == "GATAAG" else (2, 0)        # on the other strand: CTAATC, position 2, base A
    assert (first["accept"] >> (4 * i + b)) & 1
    assert first["tp"] >= 36 and first["nsites"] >= 36


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_loop_finds_nothing_in_random_sets(seed):
    prim, ctrl = wm.random_case(seed)
    rounds, n_tests = wm.discover(prim, ctrl, widths=(6, 7, 8), min_count=3, max_evalue=0.05)
    assert rounds == [] and n_tests > 0


def test_test_rule_and_ties():
    pos = np.array([0, 5, 5, 2, 9, 9, 1], np.int32)
    neg = np.array([0, 0, 9, 0, 1, 1, 0], np.int32)
    logp, best, n_tested, lp = wm.word_test(pos, neg, 40, 60, 3)
    assert n_tested == 6 and best == 4 and lp == logp[4] == logp[5] < logp[1] < 0.0    # the lowest code of a tie
    assert logp[0] == logp[2] == logp[3] == logp[6] == 0.0        # empty, depleted, below min_count
    assert wm.word_test(pos, neg, 40, 60, 10)[1:] == (-1, 6, 0.0)
    assert wm.best_gap(logp, pos, neg) == logp[1] - logp[4]


# ---------------------------------------------------------------- the C boundary
def test_header_exports_and_constants():
    from explainn_amd import _lib
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in (("explainn_word_counts", 9), ("explainn_word_test", 10), ("explainn_word_sites", 13)):
        m = re.search(r"int %s\(([^)]*)\)\s*;" % name, code)
        assert m and m.group(1).count(",") + 1 == arity
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == arity
    const = lambda n: int(re.search(r"#define EXPLAINN_%s (\d+)" % n, text).group(1))
    assert const("WORD_SPAN") == _lib.WORD_SPAN == wm.SPAN
    assert (const("WORD_MIN_WIDTH"), const("WORD_MAX_WIDTH")) == (_lib.WORD_MIN_WIDTH, _lib.WORD_MAX_WIDTH) == (3, 10)
    mk = open(os.path.join(ROOT, "explainn_amd", "csrc", "Makefile")).read()
    assert "words.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from explainn_amd import _lib
    return _lib.load()


def test_entry_points_refuse_bad_arguments_without_a_launch(lib):
    """Every refusal below returns before the first HIP call, so it needs no device; the pointers are never read."""
    from explainn_amd import _lib
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    err = lambda: lib.explainn_last_error().decode()
    for k in (2, 11, -1):
        assert lib.explainn_word_counts(p, 10, p, 1, k, 1, p, None, None) == _lib.E_ARG and "k" in err()
        assert lib.explainn_word_sites(p, 10, p, 1, k, 1, 0, 0, None, None, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_counts(p, -1, p, 1, 6, 1, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_counts(p, 10, p, -1, 6, 1, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_counts(p, 10, None, 1, 6, 1, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_counts(p, 10, p, 1, 6, 1, None, None, None) == _lib.E_ARG
    assert lib.explainn_word_counts(None, 10, p, 1, 6, 1, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, -1, 4, 6, 1, p, p, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, 4 ** 10 + 1, 4, 6, 1, p, p, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, 4, -1, 6, 1, p, p, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, 4, 1 << 30, 1 << 30, 1, p, p, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, 4, 4, 6, -1, p, p, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(None, p, 4, 4, 6, 1, p, p, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, 4, 4, 6, 1, None, p, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, 4, 4, 6, 1, p, None, p, None) == _lib.E_ARG
    assert lib.explainn_word_test(p, p, 4, 4, 6, 1, p, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_sites(p, 10, p, 1, 6, 1, 4 ** 6, 0, None, None, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_sites(p, 10, p, 1, 6, 1, -1, 0, None, None, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_sites(p, 10, p, 1, 6, 1, 0, 1 << 24, None, None, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_sites(p, 10, p, 1, 6, 1, 0, 0, None, None, None, None, None) == _lib.E_ARG
    assert lib.explainn_word_sites(p, 10, None, 1, 6, 1, 0, 0, None, None, p, None, None) == _lib.E_ARG
    assert lib.explainn_word_sites(p, 10, p, 1, 6, 1, 0, 0, p, None, p, None, None) == _lib.E_ARG       # seq_out is seq
    assert "another array" in err()


def test_python_refusals_that_need_no_device():
    from explainn_amd import discover as dv
    recs = [np.zeros(20, np.uint8)] * 3
    for kw, what in ((dict(widths=(2,)), "width"), (dict(widths=(11,)), "width"), (dict(widths=()), "widths"),
                     (dict(widths=(6, 6)), "widths"), (dict(min_count=0), "min_count"), (dict(max_evalue=0), "max_evalue"),
                     (dict(accept_pvalue=0.0), "accept_pvalue"), (dict(max_motifs=-1), "max_motifs"),
                     (dict(strands="rev"), "strands"), (dict(shuffles=0), "shuffles")):
        with pytest.raises(ValueError, match=what):
            dv.discover(recs, **kw)
    with pytest.raises(ValueError, match="one length"):
        dv.discover([np.zeros(20, np.uint8), np.zeros(21, np.uint8)])
    with pytest.raises(ValueError, match="no primary record"):
        dv.discover([], recs)
    assert dv.COLUMNS == tuple("Motif Word Width Pos Neg LogPvalue Evalue Nsites TP FP MotifLogPvalue".split())
    assert dv.word_string(wm.code_of("GATAAGC"), 7) == "GATAAGC"
    assert dv.reverse_complement_code(wm.code_of("GATAAGC"), 7) == wm.code_of("GCTTATC")
    d = dv.Discovery([dict(word="GATAAGC", width=7, seed=wm.code_of("GATAAGC"), accept=0, pos=9, neg=1, log_pvalue=-9.0,
                           n_tests=100, pfm=np.ones((7, 4), np.int64), nsites=4, tp=9, fp=1, motif_log_pvalue=-9.0)],
                     40, 60, (6, 7, 8), "both", 0, 0, 0, 100)
    assert d.as_motifs()[0][0] == "word1_GATAAGC" and d.table()[0][:5] == ("word1_GATAAGC", "GATAAGC", 7, 9, 1)
    assert abs(d.evalue[0] - 100 * np.exp(-9.0)) < 1e-12
