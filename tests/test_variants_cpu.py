"""CPU checks of the variant-effect stack (explainn_amd/variants.py, include/explainn_hip.h): the row
and edit tables against the numpy haplotype model (tests/variants_model.py), window placement,
chunking, the VCF reader, the fp64 identity units.sum(1) == delta on the oracle, and the C ABI's
struct against its ctypes twin.  No device call is made."""
import gzip
import os
import re

import numpy as np
import pytest

from oracle import explainn_oracle as orc
import scan_model as sm
import variants_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _variants():
    from explainn_amd import variants
    return variants


def test_window_start():
    V = _variants()
    # SNV in a window of 200: 99 bases to its left, 100 to its right
    assert V.window_start(1000, 1, 1, 200) == 1000 - 99
    assert V.window_start(1000, 1, 1, 200, shift=3) == 1000 - 96
    # the longer allele is centred, and both alleles share the start
    assert V.window_start(1000, 30, 2, 200) == V.window_start(1000, 2, 30, 200) == 1000 - 85
    assert V.window_start(50, 0, 0, 201) == 50 - 100
    # an allele longer than the window: the window starts inside it
    assert V.window_start(10, 1, 260, 200) == 40
    got = V.window_start(np.array([5, 1000]), np.array([1, 0]), np.array([1, 7]), 40, shift=-2)
    assert got.tolist() == [5 - 19 - 2, 1000 - 16 - 2]
    for pos, r, a, L, s in ((7, 3, 11, 83, 4), (0, 0, 1, 40, 0), (123, 70, 1, 200, -6)):
        assert V.window_start(pos, r, a, L, s) == vm.centred(pos, r, a, L, s)


@pytest.mark.parametrize("L", [200, 40])
@pytest.mark.parametrize("shifts", [(0,), (0, 3, -2, 6)])
def test_tables_stage_the_model_windows(L, shifts):
    """Every edit class of the device case table as a variant (the cases' own starts are replaced by
    window_start + shift), plus two multi-allelic sites: the rows the tables describe are the ref and
    alt windows built by concatenation."""
    V = _variants()
    seq = sm.random_codes(1000, seed=L, n_runs=6)
    edits = [e for _, e in vm.edit_cases(seq, L, seed=1) if e is not None]
    edits += [(edits[2][0], edits[2][1], np.array([3, 3], np.uint8)), (edits[6][0], edits[6][1], np.zeros(0, np.uint8))]
    pos = [e[0] for e in edits]
    ref_len = [e[1] for e in edits]
    alts = [e[2] for e in edits]
    tab = V.build_tables(pos, ref_len, alts, L, shifts)
    n, S = len(edits), len(shifts)
    assert tab["row_start"].dtype == np.int64 and tab["row_edit"].dtype == np.int32
    assert tab["pos"].dtype == np.int64 and all(tab[f].dtype == np.int32 for f in ("ref_len", "alt_len", "alt_off"))
    assert tab["alt"].dtype == np.uint8 and len(tab["row_start"]) == len(tab["row_edit"]) == 2 * n * S
    assert tab["row_edit"].reshape(n, S, 2)[:, :, 0].tolist() == [[-1] * S] * n
    assert tab["row_edit"].reshape(n, S, 2)[:, :, 1].tolist() == [[v] * S for v in range(n)]
    got = vm.edited_matrix(seq, L=L, **tab).reshape(n, S, 2, L)
    ref, alt = vm.allele_matrices(seq, pos, ref_len, alts, L, shifts)
    assert np.array_equal(got[:, :, 0], ref.reshape(n, S, L))
    assert np.array_equal(got[:, :, 1], alt.reshape(n, S, L))
    # the reference rows are plain windows of the sequence
    starts = np.array([[vm.centred(p, r, len(a), L, s) for s in shifts] for p, r, a in edits]).reshape(-1)
    plain = np.stack([sm.window_matrix(seq, int(s), 1, 1, L)[0] for s in starts])
    assert np.array_equal(ref, plain)
    # an SNV changes exactly one base of its window, at the same offset for every shift
    snv = got[1]
    assert [(snv[s, 0] != snv[s, 1]).sum() <= 1 for s in range(S)] == [True] * S


def test_model_cases_cover_the_classes():
    """The case table itself: a wholly-right edit leaves the reference row, a wholly-left one shifts
    it, and tables_from_cases describes the rows cases_matrix builds."""
    L = 200
    seq = sm.random_codes(1000, seed=3, n_runs=5)
    cases = vm.edit_cases(seq, L)
    for B, first in ((1, 0), (64, 0), (65, 7)):
        tab = vm.tables_from_cases(cases, B, first)
        assert np.array_equal(vm.edited_matrix(seq, L=L, **tab), vm.cases_matrix(seq, cases, B, L, first))
    c = len(seq) // 2
    right = vm.edited_window(seq, c - L - 5, c, 2, np.array([1, 1, 1], np.uint8), L)
    assert np.array_equal(right, sm.window_matrix(seq, c - L - 5, 1, 1, L)[0])
    left = vm.edited_window(seq, c + 28, c, 3, np.zeros(8, np.uint8), L)
    assert np.array_equal(left, sm.window_matrix(seq, c + 23, 1, 1, L)[0])


def test_chunks_hold_exactly_the_rows_of_the_whole():
    V = _variants()
    for n, S, limit in ((40, 3, 50), (40, 3, 6), (40, 3, 5), (7, 1, 4), (1, 7, 1), (100, 2, 10 ** 6)):
        runs = V.chunks(n, S, limit)
        rows = np.concatenate([np.arange(2 * S * v0, 2 * S * (v0 + c)) for v0, c in runs])
        assert np.array_equal(rows, np.arange(2 * S * n)), (n, S, limit)
        assert all(c >= 1 for _, c in runs)
        assert all(2 * S * c <= max(limit, 2 * S) for _, c in runs)
    assert V.chunks(0, 3, 10) == []


def test_build_tables_rejects_bad_input():
    V = _variants()
    with pytest.raises(ValueError):
        V.build_tables([1, 2], [1], [np.zeros(1, np.uint8)] * 2, 40)
    with pytest.raises(ValueError):
        V.build_tables([1], [-1], [np.zeros(1, np.uint8)], 40)
    with pytest.raises(ValueError):
        V.build_tables([1], [1], [np.zeros(1, np.uint8)], 40, shifts=())
    empty = V.build_tables([], [], [], 40, (0, 1))
    assert all(len(v) == 0 for v in empty.values())


VCF = """##fileformat=VCFv4.2
##contig=<ID=chr1>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
chr1\t10\trs1\tA\tG\t.\tPASS\t.
chr1\t20\t.\tac\tA,ACGT\t.\tPASS\t.
chr2\t5\tsv1\tN\t<DEL>\t.\tPASS\t.
chr2\t7\tmix\tT\tTR,*,<INS>\t.\tPASS\t.
chr2\t9\tbnd\tG\tG]chr1:5]\t.\tPASS\t.
chr2\t11\tnone\tG\t.\t.\tPASS\t.
"""


def test_read_vcf(tmp_path):
    V = _variants()
    plain = tmp_path / "a.vcf"
    plain.write_text(VCF)
    zipped = tmp_path / "a.vcf.gz"
    with gzip.open(zipped, "wt") as fh:
        fh.write(VCF)
    for path in (plain, zipped):
        recs, skipped = V.read_vcf(str(path))
        assert skipped == 5                          # <DEL>, *, <INS>, the breakend, the missing allele
        assert [tuple(r) for r in recs] == [
            ("chr1", 9, "rs1", "A", "G"), ("chr1", 19, ".", "ac", "A"), ("chr1", 19, ".", "ac", "ACGT"),
            ("chr2", 6, "mix", "T", "TR")]
    assert V.allele_codes("ac").tolist() == [0, 1] and V.allele_codes("TR").tolist() == [3, 4]
    assert V.allele_codes("nNgt").tolist() == [4, 4, 2, 3] and V.allele_codes("").tolist() == []


def test_unit_effects_sum_to_delta_fp64():
    """units.sum(1) == delta: the bias and everything else shared by the two alleles cancels."""
    U, k, L, T = 4, 5, 40, 2
    sd = orc.random_state_dict(U, k, L, T, seed=2)
    seq = sm.random_codes(400, seed=5, n_runs=2)
    pos, ref_len, alts = vm.mixed_variants(seq, 10, L, seed=6)
    shifts = (0, 3, 6)
    ref, alt = vm.allele_matrices(seq, pos, ref_len, alts, L, shifts)
    units, delta, _ = vm.oracle_effects(orc, sd, ref, alt, len(pos), len(shifts))
    assert units.shape == (10, U, T) and delta.shape == (10, T)
    assert np.abs(delta).max() > 1e-3, "the variants must move the logits"
    assert np.abs(units.sum(1) - delta).max() < 1e-10


def _header():
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_edits_abi_matches_header():
    import ctypes as C
    from explainn_amd import _lib
    text = _header()
    body = re.search(r"typedef struct explainn_edits \{(.*?)\} explainn_edits;", text, re.S).group(1)
    fields, kinds = [], []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", decl)
            kinds.append("ptr" if "*" in decl else decl.split()[0])
    assert tuple(fields) == _lib.EDIT_FIELDS
    assert tuple(f for f, _ in _lib.Edits._fields_) == _lib.EDIT_FIELDS
    for (name, ct), kind in zip(_lib.Edits._fields_, kinds):
        assert (ct is C.c_void_p) == (kind == "ptr"), name
        assert kind == "ptr" or (kind == "int64_t" and ct is C.c_int64), name
    for name, nargs in (("explainn_stage_edited_windows", 8), ("explainn_score_edits", 10)):
        assert name in _lib.EXPORTS and len(_lib.SIGNATURES[name][1]) == nargs
        proto = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(proto.split(",")) == nargs, name


def test_edits_exports_in_library():
    import __graft_entry__ as g
    g.build()
    from explainn_amd import _lib
    lib = _lib.load()
    for name in ("explainn_stage_edited_windows", "explainn_score_edits"):
        assert hasattr(lib, name), "missing export " + name
