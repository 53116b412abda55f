"""GPU: the two site callers on the same codes -- call_sites (a model's filters) and scan_motifs (known
motifs) share the chunk driver and the assembler of explainn_amd/sites.py and the COUNT / scan / EMIT scheme
of csrc/sitescan.h: cut into chunks just under and just over a tile, every array of either result equals the
single-chunk call's exactly."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pwmsites_model as pm  # noqa: E402
from test_gpu_sites import _dense, _net, _thresholds, _tile  # noqa: E402

pytestmark = pytest.mark.gpu

U, K, L = 5, 19, 200
KEYS = {"filters": ("offsets", "start", "strand", "score"),
        "motifs": ("offsets", "start", "strand", "iscore", "score", "pvalue")}


@functools.lru_cache(maxsize=None)
def _inputs():
    from explainn_amd import _lib
    tile = _tile()
    codes = np.random.default_rng(41).integers(0, 4, size=3 * tile + 7).astype(np.uint8)
    codes[tile - 5:tile + 6] = 4                                  # an N run across a tile boundary
    codes.setflags(write=False)
    net = _net(U, K, L, seed=2)
    thr = _thresholds(_dense(net, codes), special=False)          # 0.5 x each unit's maximum
    mats = pm.dirichlet_motifs([6 + i % 14 for i in range(_lib.PWM_GROUP + 1)], seed=42)      # widths 6 .. 19
    return codes, net, thr, mats


def _call(period, chunk):
    from explainn_amd import pwmsites, sites
    codes, net, thr, mats = _inputs()
    return {"filters": sites.call_sites(net, codes, thr, period=period, chunk_positions=chunk),
            "motifs": pwmsites.scan_motifs(mats, codes, pvalue=1e-2, period=period, chunk_positions=chunk)}


@functools.lru_cache(maxsize=None)
def _whole(period):
    return _call(period, None)


@pytest.mark.parametrize("period", [0, 200])
@pytest.mark.parametrize("chunk", ["TILE-1", "TILE+1"])
def test_chunked_calls_equal_the_single_chunk_call(chunk, period):
    tile = _tile()
    whole, part = _whole(period), _call(period, eval(chunk, {"TILE": tile}))
    for who, keys in KEYS.items():
        a, b = whole[who], part[who]
        assert len(a) > 50 and {1, -1} <= set(a.strand.tolist())
        assert a.start.min() < tile - 20 and a.start.max() > 2 * tile      # sites in the first and the last tile
        for key in keys:
            assert np.array_equal(getattr(b, key), getattr(a, key)), (who, key)
