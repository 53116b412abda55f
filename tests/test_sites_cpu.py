"""CPU: the host side of motif-site calling (explainn_amd/sites.py and the --sites writers of
explainn_amd/interpret.py): chunk arithmetic, the SiteCalls container, BED rows, argument errors,
command-line parsing.  Nothing here touches a device."""
import os
import re

import numpy as np
import pytest

from explainn_amd import _lib, sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_constant_matches_header():
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    assert int(re.search(r"#define EXPLAINN_SITES_TILE (\d+)", text).group(1)) == _lib.SITES_TILE
    assert _lib.SITES_TILE % 256 == 0


@pytest.mark.parametrize("n,chunk", [(1, 1), (10, 3), (10, 10), (10, 11), (1000, 37), (0, 5)])
def test_chunks_cover_every_start_once(n, chunk):
    ch = sites.position_chunks(n, chunk)
    assert [p for p0, c in ch for p in range(p0, p0 + c)] == list(range(n))
    assert all(1 <= c <= chunk for _, c in ch)
    assert len(ch) == -(-n // chunk)


def test_chunks_with_a_period_begin_on_record_boundaries():
    ch = sites.position_chunks(95, 25, period=10)          # 25 -> 20: whole records
    assert ch == [(0, 20), (20, 20), (40, 20), (60, 20), (80, 15)]
    assert sites.position_chunks(30, 4, period=10) == [(0, 10), (10, 10), (20, 10)]    # one record at least
    with pytest.raises(ValueError):
        sites.position_chunks(10, 0)


def _calls():
    # unit 0: '+' 5, 9 then '-' 5; unit 1: none; unit 2: '-' 0, '+' would precede
    fwd, rev = 2 * np.arange(3), 2 * np.arange(3) + 1             # a strand's rows: 2 * unit + (strand < 0)
    blocks = [(0, fwd, np.array([0, 1, 1, 1]), np.array([5], np.int32), np.array([1.5], np.float32)),
              (0, rev, np.array([0, 1, 1, 2]), np.array([5, 0], np.int32), np.array([3.5, 0.5], np.float32)),
              (8, fwd, np.array([0, 1, 1, 2]), np.array([1, 4], np.int32), np.array([2.5, 0.25], np.float32))]
    return _site_calls(blocks)


def _site_calls(blocks):
    return sites.SiteCalls(*sites.assemble(blocks, 3, (np.float32,)), 4)


def test_assemble_and_unit():
    c = _calls()
    assert c.units == 3 and len(c) == 5 and c.kernel_size == 4
    assert np.array_equal(c.offsets, [0, 3, 3, 5])
    start, strand, score = c.unit(0)
    assert start.tolist() == [5, 9, 5] and strand.tolist() == [1, 1, -1] and score.tolist() == [1.5, 2.5, 3.5]
    assert c.unit(1)[0].size == 0
    start, strand, score = c.unit(2)
    assert start.tolist() == [12, 0] and strand.tolist() == [1, -1] and score.tolist() == [0.25, 0.5]
    assert c.start.dtype == np.int64 and c.strand.dtype == np.int8 and c.score.dtype == np.float32
    assert c.unit_ids().tolist() == [0, 0, 0, 2, 2]
    with pytest.raises(IndexError):
        c.unit(3)
    empty = _site_calls([])
    assert len(empty) == 0 and empty.offsets.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        sites.SiteCalls([0, 2], [1], [1], [1.0], 4)


def test_bed_rows_sorted_by_start_filter_strand():
    rows = sites.bed_rows("chrT", _calls())
    assert rows == ["chrT\t0\t4\tfilter2\t0.5\t-\n",
                    "chrT\t5\t9\tfilter0\t1.5\t+\n",
                    "chrT\t5\t9\tfilter0\t3.5\t-\n",
                    "chrT\t9\t13\tfilter0\t2.5\t+\n",
                    "chrT\t12\t16\tfilter2\t0.25\t+\n"]
    assert sites.bed_rows("x", _site_calls([])) == []


def test_argument_errors():
    from explainn_amd import ExplaiNN
    m = ExplaiNN(3, 5, 30, 1).eval()
    codes = np.zeros(40, dtype=np.uint8)
    with pytest.raises(ValueError, match="strands"):
        sites.call_sites(m, codes, np.zeros(3), strands="rev")
    with pytest.raises(ValueError, match="chunk_positions"):
        sites.call_sites(m, codes, np.zeros(3), chunk_positions=0)
    with pytest.raises(ValueError, match="period"):
        sites.call_sites(m, codes, np.zeros(3), period=-1)
    with pytest.raises(ValueError, match="1-D uint8"):
        sites.call_sites(m, codes.astype(np.int64), np.zeros(3))
    with pytest.raises(ValueError, match="1-D uint8"):
        sites.call_sites(m, codes.reshape(2, 20), np.zeros(3))
    with pytest.raises(RuntimeError, match="one value per unit"):
        sites.call_sites(m, codes, np.zeros(4))
    with pytest.raises(NotImplementedError):
        sites.call_sites(m.train(), codes, np.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        sites.call_sites(m.eval(), codes, np.zeros(3))
    with pytest.raises(NotImplementedError):
        m.train()._launch_call_sites(None, None)
    msg = str(sites._too_many(np.array([3, 900, 0, 40]), 943, 100))
    assert "max_sites = 100" in msg and msg.index("filter1 (900)") < msg.index("filter3 (40)") and "filter2" not in msg


def test_thresholds_round_trip(tmp_path):
    thr = np.array([0.5, 1.25, 3.0517578125e-05], dtype=np.float16)
    path = tmp_path / "thresholds.tsv"
    sites.write_thresholds(path, thr)
    assert open(path).readline() == "filter\tthreshold\n"
    assert np.array_equal(sites.read_thresholds(path, 3), thr.astype(np.float32))
    with pytest.raises(ValueError, match="filter3|no threshold"):
        sites.read_thresholds(path, 4)
    with pytest.raises(ValueError):
        sites.read_thresholds(path, 2)
    with open(path, "at") as fh:
        fh.write("filter1\t2.0\n")
    with pytest.raises(ValueError, match="twice"):
        sites.read_thresholds(path, 3)


def test_cli_parsing():
    ap = sites._parser()
    a = ap.parse_args(["m.pth.tar", "x.fa", "-t", "thr.tsv"])
    assert (a.model_file, a.fasta_file, a.thresholds, a.output_file, a.strands) == \
        ("m.pth.tar", "x.fa", "thr.tsv", None, "both")
    a = ap.parse_args(["m", "x", "-t", "t", "-o", "out.bed", "--strands", "fwd"])
    assert a.output_file == "out.bed" and a.strands == "fwd"
    for bad in (["m", "x"], ["m", "x", "-t", "t", "--strands", "rev"]):
        with pytest.raises(SystemExit):
            ap.parse_args(bad)


def test_sites_writers_on_a_stubbed_result(tmp_path):
    from explainn_amd import interpret as it
    codes = np.array([[0, 1, 2, 3, 4, 0, 1], [3, 3, 2, 2, 1, 1, 0],
                      [2, 0, 2, 0, 2, 0, 2], [1, 1, 1, 1, 1, 1, 1]], dtype=np.uint8)
    x = (codes[:, None, :] == np.arange(4)[None, :, None]).astype(np.float32)
    assert np.array_equal(it._onehot_to_codes(x), codes)
    lists = [np.array([[0, 1, 1], [1, 4, 1], [0, 2, -1]], dtype=np.int64), np.zeros((0, 3), dtype=np.int64)]
    kmers = [it.site_kmers(x, lst, 3, rev_complement=True) for lst in lists]
    assert kmers == [["CGT", "CCA", "GAG"], []]          # strand -1 of sequence 0 reads row 0 + N/2 = 2
    it.write_sites(str(tmp_path), lists, kmers, np.array([0.5, 2.0], dtype=np.float16))
    assert open(tmp_path / "sites" / "filter0.fa").read() == ">0_+_1\nCGT\n>1_+_4\nCCA\n>0_-_2\nGAG\n"
    assert open(tmp_path / "sites" / "filter1.fa").read() == ""
    assert np.array_equal(sites.read_thresholds(tmp_path / "thresholds.tsv", 2), [0.5, 2.0])
    assert it.site_kmers(x, np.array([[0, 3, 1]]), 3) == ["TNA"]


def test_interpret_cli_has_the_sites_flag():
    import inspect
    from explainn_amd import interpret as it
    assert inspect.signature(it.interpret).parameters["sites"].default is False
    assert "--sites" in inspect.getsource(it.main)
