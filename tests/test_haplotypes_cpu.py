"""CPU checks of the haplotype stack (explainn_amd/variants.py, include/explainn_hip.h): the tables of
build_haplotype_tables against the numpy haplotype model (tests/haplotype_model.py) through an
interpreter of the table fields, run selection at both window ends, the straddler count, the overlap
error, the genotype reader, the command line with the device call stubbed, and the C ABI's struct against
its ctypes twin.  No device call is made."""
import os
import re

import numpy as np
import pytest

import haplotype_model as hm
import scan_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _variants():
    from explainn_amd import variants
    return variants


def _b(*codes):
    return np.array(codes, dtype=np.uint8)


def test_model_cases_and_their_tables_agree():
    """The case table itself: tables_from_runs describes the rows cases_matrix builds, and the runs have
    the lengths the device tests rely on."""
    for L in (200, 40):
        seq = sm.random_codes(1000, seed=L, n_runs=5)
        cases = hm.run_cases(seq, L)
        assert {0, 1, 2, 3, 63, 64, 65, 130} <= {len(run) for _, run in cases}
        assert len(cases) <= 64
        for B, first in ((1, 0), (64, 0), (65, 5)):
            tab = hm.tables_from_runs(cases, B, first)
            assert np.array_equal(hm.tables_matrix(seq, tab, L), hm.cases_matrix(seq, cases, B, L, first))
    # a run of one edit is the single-edit window of tests/variants_model.py
    import variants_model as vm
    for start, e in vm.edit_cases(seq, 40):
        if e is not None:
            assert np.array_equal(hm.haplotype_window(seq, start, [e], 40), vm.edited_window(seq, start, *e, 40))


@pytest.mark.parametrize("L", [200, 40])
def test_tables_stage_the_model_windows(L):
    V = _variants()
    seq = sm.random_codes(2000, seed=L, n_runs=4)
    pos, ref_len, alts = hm.spaced_variants(seq, 120, seed=L)
    rng = np.random.default_rng(L)
    haps = [rng.permutation(120)[:n] for n in (60, 120, 1, 0)]           # carried in any order
    starts = np.concatenate((rng.integers(-L, len(seq), 40), pos[::7], pos[::11] - L + 1, pos[::13] + 1))
    tab = V.build_haplotype_tables(pos, ref_len, alts, haps, starts, L)
    H, R = len(haps), len(starts)
    assert tab["row_start"].dtype == tab["row_first"].dtype == tab["pos"].dtype == np.int64
    assert all(tab[f].dtype == np.int32 for f in ("row_count", "edit_index", "ref_len", "alt_len", "alt_off"))
    assert tab["alt"].dtype == np.uint8 and tab["straddling"].shape == (H, R)
    assert len(tab["row_start"]) == len(tab["row_first"]) == len(tab["row_count"]) == H * R
    assert len(tab["edit_index"]) == sum(len(h) for h in haps)           # 4 bytes per carried variant
    assert np.array_equal(tab["row_start"].reshape(H, R), np.broadcast_to(starts, (H, R)))
    got = hm.tables_matrix(seq, tab, L).reshape(H, R, L)
    for h in range(H):
        for r in range(R):
            want = hm.carried_window(seq, starts[r], pos, ref_len, alts, haps[h], L)
            assert np.array_equal(got[h, r], want), (h, r)
    assert (tab["row_count"].reshape(H, R)[3] == 0).all()
    assert tab["row_count"].max() > 3
    # a run is no longer than the window needs: every edit of it begins inside the window
    for b in np.flatnonzero(tab["row_count"] > 0):
        run = hm.row_run(tab, b)
        shift = np.cumsum([0] + [len(a) - r for _, r, a in run])[:-1]
        assert run[0][0] >= tab["row_start"][b] and run[-1][0] + shift[-1] < tab["row_start"][b] + L


def test_run_selection_at_both_ends():
    V = _variants()
    L = 40
    pos, ref_len = [100, 110, 145, 150], [1, 8, 1, 1]
    alts = [_b(2), _b(), _b(1), _b(3)]
    starts = [100, 101, 99]
    tab = V.build_haplotype_tables(pos, ref_len, alts, [[3, 2, 1, 0]], starts, L)
    first, count = tab["row_first"], tab["row_count"]
    # an edit exactly at start is in the run; one base further right it is not
    assert tab["edit_index"][first[0]] == 0 and tab["edit_index"][first[1]] == 1
    # start 100: the deletion of 8 pulls pos 145 to offset 137 < 140 and leaves 150 at 142
    assert count[0] == 3 and tab["edit_index"][first[0]:first[0] + 3].tolist() == [0, 1, 2]
    # start 101: the same run less its first edit, hstart counted from the run's own first edit
    assert count[1] == 2
    # start 99: 145 -> 137 < 139, 150 -> 142
    assert count[2] == 3
    # pushed out by an insertion: 135 is inside [100, 140) on the reference, 135 + 6 is not
    tab = V.build_haplotype_tables([105, 135], [0, 1], [_b(0, 1, 2, 3, 0, 1), _b(2)], [[0, 1], [1]], [100], L)
    assert tab["row_count"].tolist() == [1, 1]
    assert tab["edit_index"][tab["row_first"][0]] == 0 and tab["edit_index"][tab["row_first"][1]] == 1
    # the last base of the window: hstart == start + L - 1 is in, start + L is out
    tab = V.build_haplotype_tables([139, 140], [1, 1], [_b(1), _b(1)], [[0], [1]], [100], L)
    assert tab["row_count"].tolist() == [1, 0]
    assert tab["straddling"].sum() == 0


def test_straddling_variants_are_left_out_and_counted():
    V = _variants()
    L = 40
    seq = sm.random_codes(400, seed=9)
    pos, ref_len = np.array([100, 120]), np.array([6, 1])
    alts = [_b(1, 1), _b(2)]
    starts = [100, 101, 105, 106, 95]
    tab = V.build_haplotype_tables(pos, ref_len, alts, [[0, 1], [1]], starts, L)
    assert tab["straddling"].tolist() == [[0, 1, 1, 0, 0], [0, 0, 0, 0, 0]]
    assert tab["row_count"].reshape(2, 5).tolist() == [[2, 1, 1, 1, 2], [1, 1, 1, 1, 1]]
    got = hm.tables_matrix(seq, tab, L).reshape(2, 5, L)
    for r, s in enumerate(starts):
        assert np.array_equal(got[0, r], hm.carried_window(seq, s, pos, ref_len, alts, [0, 1], L))
    # a straddled row is the row of the haplotype without that variant
    assert np.array_equal(got[0, 1], got[1, 1]) and not np.array_equal(got[0, 0], got[1, 0])
    # an insertion has no REF base to straddle
    tab = V.build_haplotype_tables([100], [0], [_b(1, 2)], [[0]], [99, 100, 101], L)
    assert tab["straddling"].sum() == 0 and tab["row_count"].tolist() == [1, 1, 0]


def test_overlapping_variants_raise():
    V = _variants()
    pos, ref_len, alts = [50, 52, 60, 60], [3, 1, 1, 0], [_b(1), _b(2), _b(3), _b(0, 0)]
    with pytest.raises(ValueError, match=r"#0 at 50 \(ref_len 3\) and #1 at 52"):
        V.build_haplotype_tables(pos, ref_len, alts, [[2], [1, 0]], [40], 40)
    # an SNV listed before an insertion at its position overlaps it; after it, it does not
    with pytest.raises(ValueError, match="#2 at 60"):
        V.build_haplotype_tables(pos, ref_len, alts, [[2, 3]], [40], 40)
    V.build_haplotype_tables(pos, ref_len, alts, [[3, 2], [0], [1, 2]], [40], 40)
    V.build_haplotype_tables([50, 53], [3, 1], alts[:2], [[1, 0]], [40], 40)          # abutting is legal
    with pytest.raises(ValueError, match="outside 0..3"):
        V.build_haplotype_tables(pos, ref_len, alts, [[4]], [40], 40)
    empty = V.build_haplotype_tables([], [], [], [], [], 40)
    assert all(np.asarray(v).size == 0 for v in empty.values())


VCF = """##fileformat=VCFv4.2
##contig=<ID=chr1>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\ts3
chr1\t10\tphased\tA\tG\t.\tPASS\t.\tGT:DP\t0|1:9\t1|0:3\t1|1:2
chr1\t20\tunph\tC\tT\t.\tPASS\t.\tGT\t1/1\t0/1\t0/0
chr1\t30\tmulti\tac\tA,ACGT\t.\tPASS\t.\tDP:GT\t7:1|2\t1:2/2\t5:1/2
chr1\t40\tmiss\tG\tC\t.\tPASS\t.\tGT\t.|1\t./.\t.
chr1\t50\thaploid\tT\tA\t.\tPASS\t.\tGT\t1\t0\t1
chr1\t60\tsym\tN\t<DEL>,C\t.\tPASS\t.\tGT\t1|2\t2/2\t0|1
"""


def test_read_vcf_genotypes(tmp_path):
    V = _variants()
    path = tmp_path / "g.vcf"
    path.write_text(VCF)
    variants, names, carried, unphased = V.read_vcf_genotypes(str(path))
    assert names == ["s1", "s2", "s3"]
    assert [tuple(v) for v in variants] == [tuple(v) for v in V.read_vcf(str(path))[0]]
    assert [(v.id, v.alt) for v in variants] == [("phased", "G"), ("unph", "T"), ("multi", "A"), ("multi", "ACGT"),
                                                 ("miss", "C"), ("haploid", "A"), ("sym", "C")]
    assert carried.shape == (7, 3, 2) and carried.dtype == np.uint8
    assert carried.tolist() == [
        [[0, 1], [1, 0], [1, 1]],          # phased calls are placed
        [[1, 1], [0, 0], [0, 0]],          # unphased: homozygous ALT on both, heterozygous on neither
        [[1, 0], [0, 0], [0, 0]],          # multi-allelic: 1|2 puts allele 1 on haplotype 0 ...
        [[0, 1], [1, 1], [0, 0]],          # ... and allele 2 on haplotype 1; 2/2 is homozygous for allele 2
        [[0, 1], [0, 0], [0, 0]],          # '.' is the reference allele
        [[1, 0], [0, 0], [1, 0]],          # haploid calls fill haplotype 0
        [[0, 1], [1, 1], [0, 0]],          # the symbolic allele 1 has no row; allele 2 keeps its number
    ]
    assert unphased.tolist() == [0, 1, 1]  # s2: 0/1; s3: 1/2
    sub = V.read_vcf_genotypes(str(path), samples=["s3", "s1"])
    assert sub[1] == ["s3", "s1"] and np.array_equal(sub[2], carried[:, [2, 0]]) and sub[3].tolist() == [1, 0]
    with pytest.raises(ValueError, match="nobody"):
        V.read_vcf_genotypes(str(path), samples=["nobody"])


def test_haplotypes_cli(tmp_path, monkeypatch):
    V = _variants()
    L = 40
    recs = {"chrA": sm.random_codes(300, seed=1), "chrB": sm.random_codes(200, seed=2)}
    letters = np.array(list("ACGTN"))
    fa = tmp_path / "g.fa"
    fa.write_text("".join(">%s\n%s\n" % (rid, "".join(letters[c])) for rid, c in recs.items()))
    refA = "".join(letters[recs["chrA"][99:101]])
    vcf = tmp_path / "v.vcf"
    vcf.write_text("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tp1\tp2\n"
                   "chrA\t100\ta\t%s\t%s\t.\t.\t.\tGT\t0|1\t1|1\n" % (refA, refA[0]) +
                   "chrA\t120\tb\t%s\t%sAC\t.\t.\t.\tGT\t1|0\t0/1\n" % ((letters[recs["chrA"][119]],) * 2) +
                   "chrB\t50\tc\t%s\tN\t.\t.\t.\tGT\t1|1\t0|0\n" % letters[recs["chrB"][49]])
    bed = tmp_path / "r.bed"
    bed.write_text("# regions\nchrB\t40\t60\tname\nchrA\t90\t131\nchrC\t1\t2\n")

    class Stub:
        _options = {"sequence_length": L, "n_features": 2}

    calls = []

    def fake(model, codes, pos, ref_len, alts, haplotypes, starts, strands="both", apply_sigmoid=False,
             check_ref=None, **kw):
        calls.append((len(codes), list(pos), list(ref_len), [a.tolist() for a in alts],
                      [h.tolist() for h in haplotypes], list(starts), strands, check_ref is not None))
        H, R = len(haplotypes), len(starts)
        hap = np.zeros((H, R, 2, 4))
        hap[..., 0] = np.arange(H)[:, None, None] + 0.5
        hap[..., 1] = 0.25
        hap[..., 2] = np.arange(R)[None, :, None] + np.array([0.125, 0.75])
        ref = np.full((R, 2, 4), 2.0)
        return {"hap": hap, "ref": ref, "delta": hap[..., 2] - ref[None, ..., 2], "straddling": np.zeros((H, R))}

    monkeypatch.setattr("explainn_amd.predict._load_model", lambda path: Stub())
    monkeypatch.setattr(V, "score_haplotypes", fake)
    out = tmp_path / "o.tsv"
    V.main(["m.pt", str(fa), str(vcf), "--haplotypes", "--regions", str(bed), "-o", str(out)])
    assert calls == [
        (300, [99, 119], [2, 1], [[int(recs["chrA"][99])], [int(recs["chrA"][119]), 0, 1]],
         [[1], [0], [0], [0]], [(90 + 131) // 2 - L // 2], "both", True),
        (200, [49], [1], [[4]], [[0], [0], [], []], [(40 + 60) // 2 - L // 2], "both", True)]
    rows = [line.split("\t") for line in out.read_text().splitlines()]
    assert rows[0] == ["Chrom", "Start", "End", "Sample", "Hap", "Class", "RefMean", "HapFwd", "HapRev", "HapMean",
                       "Delta"]
    body = rows[1:]
    # regions in file order; the region on a sequence the FASTA lacks is dropped
    assert [tuple(r[:6]) for r in body] == [
        (ch, s, e, p, h, t) for ch, s, e in (("chrB", "40", "60"), ("chrA", "90", "131"))
        for p in ("p1", "p2") for h in ("1", "2") for t in ("0", "1")]
    assert [float(x) for x in body[0][6:]] == [2.0, 0.5, 0.25, 0.125, 0.125 - 2.0]
    assert [float(x) for x in body[7][6:]] == [2.0, 3.5, 0.25, 0.75, 0.75 - 2.0]
    # one sample, no REF check, forward strand
    calls.clear()
    V.main(["m.pt", str(fa), str(vcf), "--haplotypes", "--regions", str(bed), "--samples", "p2", "--no-check-ref",
            "--strands", "fwd", "-o", str(out)])
    assert [c[4] for c in calls] == [[[0], [0]], [[], []]] and [c[6:] for c in calls] == [("fwd", False)] * 2
    assert len(out.read_text().splitlines()) == 1 + 2 * 2 * 2
    with pytest.raises(SystemExit):
        V.main(["m.pt", str(fa), str(vcf), "--haplotypes"])


def _header():
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_haplotypes_abi_matches_header():
    import ctypes as C
    from explainn_amd import _lib
    text = _header()
    body = re.search(r"typedef struct explainn_haplotypes \{(.*?)\} explainn_haplotypes;", text, re.S).group(1)
    fields, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", decl)
            kinds.append("ptr" if "*" in decl else decl.split()[0])
    assert tuple(fields) == _lib.HAPLOTYPE_FIELDS
    assert tuple(f for f, _ in _lib.Haplotypes._fields_) == _lib.HAPLOTYPE_FIELDS
    for (name, ct), kind in zip(_lib.Haplotypes._fields_, kinds):
        assert (ct is C.c_void_p) == (kind == "ptr"), name
        assert kind == "ptr" or (kind == "int64_t" and ct is C.c_int64), name
    for name, nargs in (("explainn_stage_haplotype_windows", 8), ("explainn_score_haplotypes", 10)):
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == nargs
        proto = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(proto.split(",")) == nargs, name
    # the edit table's fields are explainn_edits', in its order
    assert _lib.HAPLOTYPE_FIELDS[4:9] == _lib.EDIT_FIELDS[2:7]


def test_haplotypes_exports_in_library():
    import __graft_entry__ as g
    g.build()
    from explainn_amd import _lib
    lib = _lib.load()
    for name in ("explainn_stage_haplotype_windows", "explainn_score_haplotypes"):
        assert hasattr(lib, name), "missing export " + name


def test_haplotype_windows_are_edited_windows():
    """HaplotypeWindows is accepted wherever EditedWindows is."""
    from explainn_amd.architectures import EditedWindows, HaplotypeWindows
    assert issubclass(HaplotypeWindows, EditedWindows)
    assert [n for n, _ in HaplotypeWindows._TABLES] == list(__import__("explainn_amd")._lib.HAPLOTYPE_FIELDS[:9])
