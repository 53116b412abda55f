"""explainn_amd/records.py without a device: the chunk-and-place driver under a fake scorer on CPU tensors, the
control's checks and the site word."""
import contextlib

import numpy as np
import pytest
import torch

from explainn_amd import records as rec

LENGTHS = [0, 3, 0, 10, 35, 5, 1]


class FakeScorer:
    """Two units whose "best site" can be told from the record alone: row 0 is the record's length & 0x7FFF, row 1
    its first base (7 for an empty record); the site word is the length.  Keeps a log of its calls."""
    units, need, device = 2, 4, torch.device("cpu")

    def __init__(self):
        self.calls, self.entered, self.finished = [], 0, 0

    def best(self, seq, offsets, want_site):
        assert seq.dtype == torch.uint8 and offsets.dtype == torch.int64 and int(offsets[0]) == 0
        n = offsets.numel() - 1
        self.calls.append((seq.numel(), n))
        length = offsets[1:] - offsets[:-1]
        first = torch.tensor([int(seq[offsets[r]]) if length[r] > 0 else 7 for r in range(n)], dtype=torch.int16)
        bits = torch.stack([(length & 0x7FFF).to(torch.int16), first])
        return bits, (length.to(torch.int32)[None, :].expand(2, n) if want_site else None)

    @contextlib.contextmanager
    def span(self):
        self.entered += 1
        yield

    def finish(self):
        self.finished += 1


def _records():
    g = np.random.default_rng(5)
    return [g.integers(0, 4, size=n).astype(np.uint8) for n in LENGTHS]


@pytest.mark.parametrize("chunk_bases", [1, 2, 20, 1000, None])
def test_every_column_is_its_own_record_for_every_chunking(chunk_bases):
    codes, scorer = _records(), FakeScorer()
    bits, site = rec.best_over_records(scorer, codes, chunk_bases, True)
    assert bits.dtype == torch.int16 and site.dtype == torch.int32 and bits.shape == site.shape == (2, len(codes))
    assert bits[0].tolist() == LENGTHS
    assert bits[1].tolist() == [int(c[0]) if len(c) else 7 for c in codes]
    assert site[0].tolist() == LENGTHS and site[1].tolist() == LENGTHS
    # one call per run of record_chunks, each with the run's bases and the trailing N
    runs = rec.record_chunks(LENGTHS, rec.CHUNK_BASES if chunk_bases is None else chunk_bases)
    assert scorer.calls == [(sum(LENGTHS[r0:r1]) + 1, r1 - r0) for r0, r1 in runs]
    assert scorer.entered == 1 and scorer.finished == 0


def test_the_runs_include_an_overlong_record_and_a_run_of_empty_records():
    assert rec.record_chunks(LENGTHS, 20) == [(0, 4), (4, 5), (5, 7)]             # 35 > 20: a run of its own
    scorer = FakeScorer()
    rec.best_over_records(scorer, _records(), 20, False)
    assert scorer.calls == [(14, 4), (36, 1), (7, 2)]
    scorer = FakeScorer()
    bits, _ = rec.best_over_records(scorer, [np.zeros(0, np.uint8)] * 3, 1, False)
    assert scorer.calls == [(1, 3)] and bits.tolist() == [[0, 0, 0], [7, 7, 7]]   # only the trailing N goes over


def test_no_record_no_call_and_no_site_unless_asked():
    scorer = FakeScorer()
    bits, site = rec.best_over_records(scorer, [], 5, True)
    assert bits.shape == (2, 0) and site.shape == (2, 0) and scorer.calls == [] and scorer.entered == 1
    bits, site = rec.best_over_records(scorer, _records(), 20, False)
    assert site is None and bits.shape == (2, len(LENGTHS)) and scorer.finished == 0


def test_control_plan():
    prim = [np.zeros(6, np.uint8), np.ones(6, np.uint8)]
    with pytest.raises(ValueError, match="no primary record"):
        rec.control_plan([], None, 1)
    with pytest.raises(ValueError, match="shuffles must be at least 1"):
        rec.control_plan(prim, None, 0)
    with pytest.raises(ValueError, match="one length"):
        rec.control_plan(prim + [np.zeros(7, np.uint8)], None, 1)
    with pytest.raises(ValueError, match="primary records are empty"):
        rec.control_plan([np.zeros(0, np.uint8)] * 2, None, 1)
    ctrl, lengths, shuffles = rec.control_plan(prim, [("c", np.zeros(3, np.uint8)), np.zeros(9, np.uint8)], 5)
    assert [len(c) for c in ctrl] == [3, 9] and list(lengths) == [3, 9] and shuffles == 0
    ctrl, lengths, shuffles = rec.control_plan(prim, None, 3)
    assert ctrl is None and shuffles == 3 and np.array_equal(lengths, np.repeat([6, 6], 3))


def test_bg_argument_error_texts():
    import argparse

    from explainn_amd.pwmsites import _bg_arg
    assert _bg_arg("uniform") is None and _bg_arg("sequence") == "sequence" and _bg_arg("1,2,3,4") == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(argparse.ArgumentTypeError) as err:
        _bg_arg("1,2,3")
    assert str(err.value) == "--bg takes uniform, sequence or four frequencies a,c,g,t"
    with pytest.raises(argparse.ArgumentTypeError) as err:
        _bg_arg("sequence", sequence=False)
    assert str(err.value) == "--bg takes uniform or four frequencies a,c,g,t"


def test_site_word_round_trip():
    words = np.array([[-1, 0, 1, 2, ((2 ** 30 - 1) << 1) | 1]], dtype=np.int32)
    start, strand = rec.unpack_site(words)
    assert start.tolist() == [[-1, 0, 0, 1, 2 ** 30 - 1]] and strand.tolist() == [[0, 1, -1, 1, -1]]
    back = rec.pack_site(start, strand)
    assert back.dtype == np.int32 and np.array_equal(back, words)
