"""CPU: the numpy model of variant effects on known motifs (tests/pwmvariants_model.py) against a start-by-start
brute force over the full haplotype, allele trimming on VCF-style anchored indels, the C boundary of
explainn_pwm_variant_best, and the argument refusals of explainn_amd/pwmvariants.py that need no device."""
import os
import re

import numpy as np
import pytest

import pwmbest_model as bm
import pwmsites_model as pm
import pwmvariants_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T, N = 0, 1, 2, 3, 4


def _palindrome(w=8, seed=3):
    half = np.random.default_rng(seed).dirichlet(np.full(4, 0.3), size=w // 2)
    return np.concatenate([half, half[::-1, ::-1]])


def _cases(n):
    """Variants of every kind on a sequence of n bases, the edges included: (pos, ref_len, alts)."""
    g = np.random.default_rng(11)
    rnd = lambda k: g.integers(0, 4, size=k).astype(np.uint8)
    pos, ref_len, alts = vm.random_variants(n, 40, seed=5, max_len=6)
    extra = [(0, 1, rnd(1)), (n - 1, 1, rnd(1)), (n, 0, rnd(3)), (0, 0, rnd(2)), (0, 3, rnd(0)), (n - 4, 4, rnd(0)),
             (50, 0, rnd(0)), (60, 2, np.array([N, A], np.uint8)), (70, 9, rnd(1)), (80, 1, rnd(12)), (1, 1, rnd(1)),
             (n - 2, 1, rnd(2))]
    for p, r, a in extra:
        pos.append(p), ref_len.append(r), alts.append(a)
    return pos, ref_len, alts


@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
def test_model_equals_brute_force_over_the_full_haplotype(both):
    mats = pm.dirichlet_motifs([1, 2, 4, 6, 9, 13], seed=1) + [_palindrome(), np.full((5, 4), 0.25), np.zeros((0, 4))]
    tab = bm.tables(mats)
    S, lw = tab["S"], tab["live"]
    n = 160
    codes = pm.random_codes(n, seed=2, n_frac=0.03)
    codes[100:120] = A                                            # a flat stretch: ties
    pos, ref_len, alts = _cases(n)
    pos, ref_len, alts = pos + [105, 108], ref_len + [1, 0], alts + [np.array([A], np.uint8), np.array([A, A], np.uint8)]
    p, rl, al, ao, pool = vm.edit_table(pos, ref_len, alts)
    bits, site, flags = vm.variant_best(S, lw, codes, p, rl, al, ao, pool, both)
    assert flags == 0
    for v in range(len(p)):
        for k, allele in enumerate((codes[p[v]:p[v] + rl[v]], pool[ao[v]:ao[v] + al[v]])):
            hap = vm.haplotype(codes, int(p[v]), int(rl[v]), allele)
            assert len(hap) == n - rl[v] + len(allele)
            for m in range(len(mats)):
                want = vm.allele_brute(S[m], int(lw[m]), hap, int(p[v]), len(allele), both)
                assert (int(bits[m, v, k]), int(site[m, v, k])) == want, (v, k, m)
    assert np.all(site[-1] == -1) and np.all(site[-2] == -1)      # the empty and the flat motif
    live = site[:-2]
    assert np.any(live >= 0) and np.any(live == -1)
    if both:
        assert np.any(live[live >= 0] & 1 == 1)
        pal = site[6]
        assert np.all(pal[pal >= 0] & 1 == 0)                     # a palindrome ties everywhere: '+'
    # the w = 1 motif has no window at a pure deletion and l windows otherwise
    w1 = site[0]
    for v in range(len(p)):
        assert (w1[v, 0] >= 0) == (rl[v] > 0 and np.any(codes[p[v]:p[v] + rl[v]] < 4)), v
    # an SNV that rewrites A to A inside the flat stretch: every touched window ties, index 0 wins
    assert np.all(site[2:4, len(p) - 2, :] >> 1 == 0)


def test_model_flags_and_bad_records():
    tab = bm.tables(pm.dirichlet_motifs([4, 7], seed=4))
    S, lw = tab["S"], tab["live"]
    codes = pm.random_codes(60, seed=5, n_frac=0.0)
    good = vm.edit_table([10, 30], [1, 2], [[C], [G, G, T]])
    assert vm.variant_best(S, lw, codes, *good)[2] == 0
    odd = codes.copy()
    odd[10 + 7] = 9                                               # past wmax - 1 = 6 bases of the allele: not read
    assert vm.variant_best(S, lw, odd, *good)[2] == 0
    odd[10 + 6] = 9
    b, s, f = vm.variant_best(S, lw, odd, *good)
    assert f == 1 and np.all(s[1, 0] >= 0)                        # the windows left of it are still live
    p, rl, al, ao, pool = vm.edit_table([10], [1], [[200]])
    assert vm.variant_best(S, lw, codes, p, rl, al, ao, pool)[2] == 1
    for bad in ((-1, 1, 1, 0), (10, -1, 1, 0), (10, 1, -1, 0), (59, 2, 1, 0), (10, 1, 1, -1), (10, 1, 2, 0),
                (10, 129, 1, 0)):
        b, s, f = vm.variant_best(S, lw, codes, [bad[0]], [bad[1]], [bad[2]], [bad[3]], np.zeros(1, np.uint8))
        assert f == 2 and np.all(s == -1) and np.all(b == 0), bad


def test_trimming_of_anchored_indels():
    seq = lambda *x: np.array(x, dtype=np.uint8)
    same = lambda got, want: got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert same(vm.trim(10, seq(C, A), seq(C)), (11, seq(A), seq()))                  # CA -> C: deletion of A at 11
    assert same(vm.trim(10, seq(C), seq(C, A, G)), (11, seq(), seq(A, G)))             # C -> CAG: insertion at 11
    assert same(vm.trim(10, seq(A), seq(G)), (10, seq(A), seq(G)))                     # an SNV stays
    assert same(vm.trim(10, seq(A, C, G), seq(A, T, G)), (11, seq(C), seq(T)))         # prefix and suffix
    assert same(vm.trim(10, seq(A, A), seq(A)), (11, seq(A), seq()))                   # the prefix goes first
    assert same(vm.trim(10, seq(A, C), seq(A, C)), (12, seq(), seq()))                 # REF == ALT: nothing is left
    from explainn_amd import pwmvariants as pv
    g = np.random.default_rng(3)
    refs = [g.integers(0, 2, size=int(g.integers(0, 6))).astype(np.uint8) for _ in range(200)]
    alts = [g.integers(0, 2, size=int(g.integers(0, 6))).astype(np.uint8) for _ in range(200)]
    pos, r2, a2 = pv.trim_alleles(np.arange(200), refs, alts)
    for v in range(200):
        assert same((pos[v], r2[v], a2[v]), vm.trim(v, refs[v], alts[v])), v
        # the trimmed edit makes the same haplotype: what was cut is what the alleles shared
        lead = pos[v] - v
        assert np.array_equal(refs[v][:lead], alts[v][:lead])
        assert np.array_equal(np.concatenate([refs[v][:lead], a2[v], refs[v][lead + len(r2[v]):]]), alts[v])


def test_effects_of_the_model_on_a_planted_site():
    mats = pm.dirichlet_motifs([8, 10, 12], seed=8, alpha=0.1)
    codes = pm.random_codes(400, seed=9, n_frac=0.0)
    pm.plant(codes, mats[2], 200)
    col = int(np.argmax(np.max(mats[2], axis=1) - np.sort(mats[2], axis=1)[:, -2]))
    worst = int(np.argmin(mats[2][col]))
    res = vm.motif_variants(mats, codes, [200 + col], [1], [[worst]], pvalue=1e-6)
    k = np.flatnonzero(res["motif"] == 2)
    assert len(k) == 1 and res["effect"][k[0]] == "loss" and res["delta"][k[0]] < 0
    assert res["ref_offset"][k[0]] == -col and res["ref_strand"][k[0]] == 1
    mutated = codes.copy()
    mutated[200 + col] = worst
    back = vm.motif_variants(mats, mutated, [200 + col], [1], [[codes[200 + col]]], pvalue=1e-6)
    k2 = np.flatnonzero(back["motif"] == 2)
    assert len(k2) == 1 and back["effect"][k2[0]] == "gain"
    assert back["alt_iscore"][k2[0]] == res["ref_iscore"][k[0]] and back["ref_iscore"][k2[0]] == res["alt_iscore"][k[0]]
    every = vm.motif_variants(mats, codes, [200 + col], [1], [[worst]], pvalue=1e-6, keep="all")
    assert len(every["motif"]) == 3 and set(every["effect"]) <= {"loss", "gain", "both", "none"}
    hit = (every["ref_iscore"] >= every["thresholds"][every["motif"]]) | (
        every["alt_iscore"] >= every["thresholds"][every["motif"]])
    for f in ("motif", "ref_iscore", "alt_iscore", "effect", "ref_pvalue"):
        assert np.array_equal(every[f][hit], res[f])


# ---------------------------------------------------------------- the C boundary and the host half
def test_header_and_signature():
    from explainn_amd import _lib
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert re.search(r"int explainn_pwm_variant_best\(", text)
    assert "explainn_pwm_variant_best" in _lib.EXPORTS and len(_lib.SIGNATURES["explainn_pwm_variant_best"][1]) == 18
    assert int(re.search(r"#define EXPLAINN_PWM_VARIANT_MAX_ALLELE (\d+)", text).group(1)) == \
        _lib.PWM_VARIANT_MAX_ALLELE == vm.MAX_ALLELE == 128
    mk = open(os.path.join(ROOT, "explainn_amd", "csrc", "Makefile")).read()
    assert "pwmvariants.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()


def test_refusals_that_need_no_device():
    from explainn_amd import pwmvariants as pv
    mats = pm.dirichlet_motifs([6, 8], seed=1)
    codes = pm.random_codes(300, seed=2, n_frac=0.0)
    snv = ([10], [1], [np.array([(codes[10] + 1) % 4], np.uint8)])
    with pytest.raises(ValueError, match="strands"):
        pv.motif_variants(mats, codes, *snv, strands="rev")
    with pytest.raises(ValueError, match="keep"):
        pv.motif_variants(mats, codes, *snv, keep="some")
    with pytest.raises(ValueError, match="pvalue"):
        pv.motif_variants(mats, codes, *snv, pvalue=1.5)
    with pytest.raises(ValueError, match="per-record backgrounds"):
        pv.motif_variants(mats, codes, *snv, bg="sequence")
    with pytest.raises(ValueError, match="chunk_variants"):
        pv.motif_variants(mats, codes, *snv, chunk_variants=0)
    with pytest.raises(ValueError, match="bins"):
        pv.motif_variants(mats, codes, *snv, bins=0)
    with pytest.raises(ValueError, match="outside the sequence"):
        pv.motif_variants(mats, codes, [299], [2], [np.zeros(1, np.uint8)])
    with pytest.raises(ValueError, match="REF allele"):
        pv.motif_variants(mats, codes, *snv, check_ref=[np.array([(codes[10] + 1) % 4], np.uint8)])
    with pytest.raises(ValueError, match="longer than 128"):
        pv.motif_variants(mats, codes, [20], [0], [np.zeros(129, np.uint8)])
    # 130 bases that share their first two with the sequence: 128 after trimming, so it is not the cap that refuses
    long_alt = np.concatenate([codes[20:22], np.full(128, (codes[22] + 1) % 4)]).astype(np.uint8)
    data, tab = pv._prepare(codes, [20], [3], [long_alt], True, None)
    assert tab["pos"][0] == 22 and tab["ref_len"][0] == 1 and tab["alt_len"][0] == 128
    with pytest.raises(ValueError, match="longer than 128"):
        pv._prepare(codes, [20], [3], [long_alt], False, None)
    with pytest.raises(SystemExit):
        pv._parser().parse_args(["m.meme", "x.fa", "x.vcf", "--bg", "sequence"])
    assert pv.HEADER.split() == ("Chrom Pos Id Ref Alt Motif Name Effect RefScore AltScore Delta RefPvalue AltPvalue "
                                 "RefOffset RefStrand AltOffset AltStrand").split()
