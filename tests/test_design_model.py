"""tests/design_model.py against an enumeration of every candidate on tiny cases, the loop around a toy
ISM function, and the C ABI / Python surface of the design feature that needs no GPU."""
import numpy as np
import pytest

from tests import design_model as dm


def _enumerate(delta_f, delta_r, codes, mask, weights, min_gain):
    """The winner of every sequence by walking all 4L candidates in plain Python (fp64 scalars)."""
    B, T, _, L = delta_f.shape
    w = np.broadcast_to(np.asarray(weights, dtype=np.float32), (B, T))
    out = []
    for b in range(B):
        cands = []
        for p in range(L):
            for a in range(4):
                of = 0.0
                for t in range(T):
                    of += float(w[b, t]) * float(delta_f[b, t, a, p])
                g = of
                if delta_r is not None:
                    orv = 0.0
                    for t in range(T):
                        orv += float(w[b, t]) * float(delta_r[b, t, 3 - a, L - 1 - p])
                    g = 0.5 * (of + orv)
                if a == codes[b, p] or (mask is not None and mask[b, p] == 0):
                    continue
                if not g > float(np.float32(min_gain)):
                    continue
                cands.append((-g, p, a))
        out.append(min(cands) if cands else None)
    return out


def _grid_maps(rng, B, T, L):
    return (rng.integers(-4, 5, size=(B, T, 4, L)) / 8.0).astype(np.float32)


@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("B,T,L", [(6, 1, 5), (9, 3, 8), (7, 2, 1)])
def test_pick_vs_enumeration(B, T, L, both, per_row):
    rng = np.random.default_rng(100 * B + 10 * T + L + both)
    df = _grid_maps(rng, B, T, L)
    dr = _grid_maps(rng, B, T, L) if both else None
    codes = rng.integers(0, 5, size=(B, L)).astype(np.uint8)
    mask = (rng.random((B, L)) < 0.7).astype(np.uint8)
    mask[0] = 0                                           # an all-closed row
    w = (rng.integers(-2, 3, size=(B, T) if per_row else (T,)) / 2.0).astype(np.float32)
    # planted exact ties: row 1 gets the same map value everywhere, every position open
    df[1] = 0.25
    if both:
        dr[1] = 0.25
    mask[1] = 1
    if per_row:
        w[1] = 1.0
    for min_gain in (0.0, 0.3, 100.0):
        ref = _enumerate(df, dr, codes, mask, w, min_gain)
        pos, rb, alt, gain, codes2, mask2 = dm.pick(df, dr, codes, mask, w, lock=True, min_gain=min_gain)
        for b in range(B):
            if ref[b] is None:
                assert (pos[b], rb[b], alt[b], gain[b]) == (-1, 255, 255, 0.0)
                assert np.array_equal(codes2[b], codes[b]) and np.array_equal(mask2[b], mask[b])
            else:
                g, p, a = ref[b]
                assert (pos[b], alt[b], gain[b], rb[b]) == (p, a, -g, codes[b, p])
                want = codes[b].copy()
                want[p] = a
                assert np.array_equal(codes2[b], want)
                assert mask2[b, p] == 0 and np.array_equal(np.delete(mask2[b], p), np.delete(mask[b], p))
        assert pos[0] == -1
        if min_gain == 100.0:
            assert np.all(pos == -1)
    # unlocked, unmasked: the mask stays None, an N takes base 0 on a full tie
    codes[1, 0] = 4
    pos, rb, alt, gain, _, m = dm.pick(df, dr, codes, None, np.ones(T, np.float32))
    assert m is None and (pos[1], rb[1], alt[1], gain[1]) == (0, 4, 0, 0.25 * T)


def test_tie_rule_and_reverse_coordinates():
    """The lowest p, then the lowest a, wins an exact tie; the reverse map is read at (3-a, L-1-p)."""
    L = 6
    df = np.zeros((1, 1, 4, L), np.float32)
    df[0, 0, 2, 4] = df[0, 0, 1, 4] = df[0, 0, 3, 2] = 1.0
    codes = np.zeros((1, L), np.uint8)
    pos, _, alt, gain, _, _ = dm.pick(df, None, codes, None, np.ones(1, np.float32))
    assert (pos[0], alt[0], gain[0]) == (2, 3, 1.0)
    dr = np.zeros_like(df)
    dr[0, 0, 3 - 1, L - 1 - 4] = 3.0                      # adds to base 1 at position 4 only
    pos, _, alt, gain, _, _ = dm.pick(df, dr, codes, None, np.ones(1, np.float32))
    assert (pos[0], alt[0], gain[0]) == (4, 1, 2.0)


def test_loop_locks_and_logs():
    """A toy ISM: delta = a fixed preference table minus the current base's entry, so the loop has a
    known optimum; with lock every position is used once, without it a position can move twice."""
    rng = np.random.default_rng(3)
    B, L, T = 4, 5, 2
    pref = rng.integers(1, 8, size=(T, 4, L)).astype(np.float32)

    def ism(codes, rc):
        c = np.where(codes < 4, 3 - codes, codes)[:, ::-1] if rc else codes
        tab = pref[:, ::-1, ::-1] if rc else pref
        cur = np.stack([np.where(c < 4, tab[t][np.minimum(c, 3), np.arange(L)], 0) for t in range(T)], axis=1)
        delta = tab[None] - cur[:, :, None, :]
        return cur.sum(axis=2), delta.astype(np.float32)
    codes = rng.integers(0, 5, size=(B, L)).astype(np.uint8)
    w = np.array([1.0, 0.5], np.float32)
    for both in (False, True):
        res = dm.evolve(ism, codes, w, rounds=L + 2, both_strands=both, lock=True)
        assert res["pos"].shape == (B, L + 2) and res["logits"].shape == (B, L + 3, 2 if both else 1, T)
        best = (pref * w[:, None, None]).sum(axis=0)
        for b in range(B):
            used = res["pos"][b][res["pos"][b] >= 0]
            assert len(set(used)) == len(used)
            assert np.all(np.diff(res["gain"][b][res["pos"][b] >= 0]) <= 0)       # greedy: gains never grow
            assert np.all(best[res["codes"][b], np.arange(L)] == best.max(axis=0))
        score = (res["logits"].astype(np.float64).mean(axis=2) * w).sum(axis=2)
        assert np.array_equal(score[:, 1:] - score[:, :-1], res["gain"])
        assert np.array_equal(res["rounds_codes"][0], codes) and np.array_equal(res["rounds_codes"][-1], res["codes"])
    res = dm.evolve(ism, codes, w, rounds=3, mask=np.array([0, 1, 1, 0, 1]), lock=False)
    assert np.array_equal(res["codes"][:, [0, 3]], codes[:, [0, 3]])


def test_abi_and_surface():
    from explainn_amd import ExplaiNN, ExplaiNNBank, _lib, design
    assert "explainn_evolve_pick" in _lib.EXPORTS and len(_lib.SIGNATURES["explainn_evolve_pick"][1]) == 16
    assert callable(ExplaiNN.evolve) and callable(design.evolve) and callable(design.main)
    bank = ExplaiNNBank(2, 3, 5, 40, 1)
    with pytest.raises(ValueError, match="member"):
        bank.evolve(None, None)
    ev = design.Evolution(np.array([[0, 4]], np.uint8), np.array([[1, -1]], np.int32), np.array([[2, 255]], np.uint8),
                          np.array([[3, 255]], np.uint8), np.array([[0.5, 0.0]]),
                          np.array([[[[1.0]], [[1.5]], [[1.5]]]], np.float32), np.ones(1, np.float32))
    assert ev.sequences() == ["AN"] and ev.mutations() == [(0, 0, 1, "G", "T", 0.5, 1.5)]
    assert np.array_equal(ev.score, [[1.0, 1.5, 1.5]])
