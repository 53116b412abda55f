"""CPU: the chunk driver and the assembler every site caller shares (explainn_amd/sites.py: site_blocks,
assemble), driven by stub legs built on the numpy model of known-motif sites.  A stub's finish is the identity
and its arrays are numpy's: the chunk loop, the max_sites check and the ordering, with no device."""
import numpy as np
import pytest

import pwmsites_model as pm
from explainn_amd import sites
from test_pwmsites_model import _assembled, _model_case

PCUT = 1e-2


class StubLeg:
    """The rows `rows` (canonical: 2 * motif + (strand < 0)) of the model's scan of a chunk."""

    def __init__(self, case, rows, period):
        self.S, self.lw, self.thr, self.tail = case
        self.rows, self.period, self.emits = np.asarray(rows), period, 0

    def _scan(self, piece, cnt):
        off, pos, isc = pm.scan(self.S, self.lw, self.thr, piece, 0, cnt, self.period)
        keep = np.concatenate([np.arange(off[r], off[r + 1]) for r in self.rows])
        mine = np.concatenate([[0], np.cumsum(np.diff(off)[self.rows])])
        return mine, pos[keep], isc[keep], self.tail[np.repeat(self.rows, np.diff(mine)) // 2, isc[keep]]

    def count(self, piece, cnt):
        return lambda: self._scan(piece, cnt)[0]

    def emit(self, piece, cnt, total):
        self.emits += 1
        out = self._scan(piece, cnt)[1:]
        assert len(out[0]) == total
        return lambda: out


def _case():
    mats, codes = _model_case()
    S, widths, scale, lo = pm.quantise(mats)
    lw = pm.live_widths(widths, scale)
    tail, thr = pm.null_table(S, lw, 100, pm.uniform(), PCUT)
    return mats, codes, (S, lw, thr, tail), (widths, scale, lo)


def _drive(codes, legs, chunk, period, wmax, max_sites=10 ** 9):
    pieces = ((p0, cnt, codes[p0:p0 + cnt + wmax - 1]) for p0, cnt in sites.position_chunks(len(codes), chunk, period))
    return sites.site_blocks(pieces, legs, 3, max_sites, sites._too_many)


@pytest.mark.parametrize("period", [0, 50])
@pytest.mark.parametrize("chunk", [1, 97, 700])
def test_driver_and_assembler_equal_the_model(chunk, period):
    mats, codes, case, table = _case()
    assert chunk <= len(codes) == 700
    want = pm.calls(mats, codes, PCUT, period=period)
    assert len(want["start"]) > 20
    one = _drive(codes, [StubLeg(case, np.arange(6), period)], chunk, period, case[0].shape[1])
    # call_sites' shape: a leg per strand, its rows the units
    two = _drive(codes, [StubLeg(case, [0, 2, 4], period), StubLeg(case, [1, 3, 5], period)], chunk, period,
                 case[0].shape[1])
    for blocks in (one, two):
        got = _assembled(blocks, *table)
        for key in ("offsets", "start", "strand", "iscore", "score", "pvalue"):
            assert np.array_equal(getattr(got, key), want[key]), key


def test_max_sites_raises_before_the_chunk_is_emitted():
    mats, codes, case, _ = _case()
    per_chunk = [int(pm.scan(*case[:3], codes[p0:p0 + cnt + 10], 0, cnt)[0][-1])
                 for p0, cnt in sites.position_chunks(len(codes), 97)]
    assert all(per_chunk[:3])                                     # the third chunk is the one that overflows
    legs = [StubLeg(case, [0, 2, 4], 0), StubLeg(case, [1, 3, 5], 0)]
    with pytest.raises(ValueError, match=r"max_sites = %d sites \(%d so far\)" % (sum(per_chunk[:3]) - 1,
                                                                                  sum(per_chunk[:3]))):
        _drive(codes, legs, 97, 0, 11, max_sites=sum(per_chunk[:3]) - 1)
    # chunks 0 and 1 (a leg without a site in a chunk is skipped), nothing of chunk 2
    first_two = [codes[p0:p0 + cnt + 10] for p0, cnt in sites.position_chunks(len(codes), 97)[:2]]
    assert [leg.emits for leg in legs] == [sum(leg.count(piece, 97)()[-1] > 0 for piece in first_two) for leg in legs]
    assert 2 <= sum(leg.emits for leg in legs) <= 4
    legs = [StubLeg(case, np.arange(6), 0)]
    assert len(_drive(codes, legs, 97, 0, 11, max_sites=sum(per_chunk))) == legs[0].emits == len(per_chunk)
