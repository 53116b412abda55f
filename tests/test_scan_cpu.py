"""Host side of the tiled scan: FASTA records of unequal length, window arithmetic, chunking, the
CLI's argument checks and its TSV.  No GPU."""
import gzip

import numpy as np
import pytest

from explainn_amd import scan as S
from explainn_amd.loader import read_fasta_records


def test_read_fasta_records(tmp_path):
    text = ">a first\nACGT\nacgtn\n>empty\n>b\nNNXA\r\n>c\nT\n"
    p = tmp_path / "x.fa"
    p.write_text(text)
    g = tmp_path / "x.fa.gz"
    with gzip.open(g, "wt") as fh:
        fh.write(text)
    for path in (p, g):
        recs = read_fasta_records(str(path))
        assert [r[0] for r in recs] == ["a", "empty", "b", "c"]
        assert recs[0][1].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 4]
        assert recs[1][1].shape == (0,) and recs[1][1].dtype == np.uint8
        assert recs[2][1].tolist() == [4, 4, 4, 0]
        assert recs[3][1].tolist() == [3]
        assert all(r[1].dtype == np.uint8 and r[1].ndim == 1 for r in recs)


def test_window_starts():
    assert S.window_starts(199, 200, 7).tolist() == []
    assert S.window_starts(0, 200, 7).tolist() == []
    assert S.window_starts(200, 200, 7).tolist() == [0]
    assert S.window_starts(206, 200, 7).tolist() == [0]
    assert S.window_starts(207, 200, 7).tolist() == [0, 7]
    assert S.window_starts(1000, 200, 50).tolist() == list(range(0, 801, 50))
    assert S.window_starts(1000, 200, 7).dtype == np.int64
    with pytest.raises(ValueError):
        S.window_starts(1000, 200, 0)


@pytest.mark.parametrize("W,limit,n_chunks", [(100, 100, 1), (100, 1000, 1), (100, 50, 2), (100, 51, 2),
                                              (1000, 7, 143), (1, 1, 1)])
def test_chunks_cover_every_window_once(W, limit, n_chunks):
    L, stride = 200, 14
    cs = S.chunks(W, limit)
    assert len(cs) == n_chunks
    starts = S.window_starts(stride * (W - 1) + L, L, stride)
    seen = []
    for (w0, cnt), nxt in zip(cs, cs[1:] + [None]):
        assert 1 <= cnt <= limit
        lo, hi = w0 * stride, (w0 + cnt - 1) * stride + L        # the bases the chunk reads
        assert lo % stride == 0
        seen += (lo + S.window_starts(hi - lo, L, stride)).tolist()
        if nxt is not None:
            assert hi - nxt[0] * stride == L - stride                # neighbours overlap by L - stride
    assert seen == starts.tolist()


def test_chunk_limit_bounds_the_shared_track():
    L, k, bs = 200, 19, 4096
    n = (L - k + 1) // 7
    for stride in (7, 14, 49, 7 * n, 7 * (n + 2)):
        m = stride // 7
        W = S.chunk_limit(L, k, stride, bs)
        assert -(-(m * (W - 1) + n) // n) <= 4 * bs < -(-(m * W + n) // n) or W == 32 * bs
    assert S.chunk_limit(L, k, 10, bs) == 32 * bs


def test_argument_errors():
    for argv in (["m.pt", "x.fa", "-s", "0"], ["m.pt", "x.fa", "--mode", "shared", "-s", "10"],
                 ["m.pt", "x.fa", "--mode", "bogus"], ["m.pt", "x.fa", "--strands", "rev"]):
        with pytest.raises(SystemExit) as e:
            S.main(argv)
        assert e.value.code == 2
    with pytest.raises(ValueError):
        S._check_args(0, "both", "auto")
    with pytest.raises(ValueError):
        S._check_args(10, "both", "shared")
    S._check_args(10, "both", "auto")
    S._check_args(14, "fwd", "shared")


def test_cli_writes_tsv(tmp_path, monkeypatch):
    fa = tmp_path / "x.fa"
    fa.write_text(">chrA\n" + "ACGT" * 60 + "\n>short\nACGT\n>chrB\n" + "ttga" * 52 + "\n")

    class Stub:
        _options = {"sequence_length": 200, "n_features": 2}

    calls = []

    def fake_scan(model, codes, stride=7, strands="both", mode="auto", apply_sigmoid=False, **kw):
        calls.append((len(codes), stride, strands, mode, apply_sigmoid))
        starts = S.window_starts(len(codes), 200, stride)
        preds = np.zeros((len(starts), 2, 4))
        preds[:, 1, :] = np.array([0.25, -1.5, -0.625, 0.25])
        preds[:, 0, 0] = starts
        return starts, preds

    monkeypatch.setattr(S, "_load_model", lambda path: Stub())
    monkeypatch.setattr(S, "scan", fake_scan)
    out = tmp_path / "out.tsv"
    S.main(["m.pt", str(fa), "-s", "20", "--strands", "fwd", "--mode", "windows", "-o", str(out)])
    assert calls == [(240, 20, "fwd", "windows", False), (4, 20, "fwd", "windows", False),
                     (208, 20, "fwd", "windows", False)]
    rows = [line.split("\t") for line in out.read_text().splitlines()]
    assert rows[0] == ["SeqId", "Start", "End", "Class", "Fwd", "Rev", "Mean", "Max"]
    body = rows[1:]
    assert [(r[0], int(r[1]), int(r[2]), int(r[3])) for r in body] == [
        ("chrA", 0, 200, 0), ("chrA", 0, 200, 1), ("chrA", 20, 220, 0), ("chrA", 20, 220, 1),
        ("chrA", 40, 240, 0), ("chrA", 40, 240, 1), ("chrB", 0, 200, 0), ("chrB", 0, 200, 1)]
    assert [float(v) for v in body[3][4:]] == [0.25, -1.5, -0.625, 0.25]
    assert float(body[2][4]) == 20.0
