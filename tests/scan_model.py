"""Numpy restatement of the tiled scan's index algebra ("Tiled scan"): what
explainn_stage_windows stages, which tiles the shared mode runs the filter bank on, and how the
unfold cuts every window's pooled vector out of the tile track.  tests/test_scan_model.py checks it
against the oracle's pooled values; tests/test_gpu_scan.py uses the materialised windows."""
import numpy as np

POOL = 7


def random_codes(length, seed=0, n_runs=0, tile=None):
    """Random base codes with n_runs runs of N; with `tile`, half of the runs straddle a multiple of it
    (the shared mode's tile boundaries when the scan starts at 0)."""
    rng = np.random.default_rng(seed)
    seq = rng.integers(0, 4, size=length).astype(np.uint8)
    for r in range(n_runs):
        ln = int(rng.integers(1, 40))
        at = int(rng.integers(0, max(1, length - ln)))
        if tile and r % 2 == 0 and length > tile:
            at = max(0, int(rng.integers(1, max(2, length // tile))) * tile - ln // 2)
        seq[at:at + ln] = 4
    return seq


def onehot(codes):
    """(B,L) codes -> (B,4,L) float32 one-hot, N = all-zero column."""
    codes = np.asarray(codes)
    return (codes[:, None, :] == np.arange(4)[None, :, None]).astype(np.float32)


def rc_rows(codes):
    """Reverse complement of every row: 3 - code, reversed, N stays N."""
    r = np.asarray(codes)[..., ::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


def window_matrix(seq, start0, B, step, L, rc=False):
    """What explainn_stage_windows stages: row b = seq[start0 + b*step : ... + L], positions outside
    the sequence read as N, bytes above 4 as N; rc reverse-complements every row."""
    seq = np.asarray(seq)
    idx = start0 + np.arange(B, dtype=np.int64)[:, None] * step + np.arange(L, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < len(seq))
    mat = np.where(inside, seq[np.clip(idx, 0, max(len(seq) - 1, 0))] if len(seq) else 4, 4).astype(np.uint8)
    mat[mat > 4] = 4
    return rc_rows(mat) if rc else mat


def pooled_len(L, k):
    return (L - k + 1) // POOL


def n_tiles(n, m, n_windows):
    """Tiles that cover every pooled value a window reads: the track needs P < m (n_windows-1) + n."""
    return -(-(m * (n_windows - 1) + n) // n)


def tile_plan(start, n_windows, stride, L, k, rc=False):
    """(start0, step, J) of the tiles of the shared mode: tile j is the window at start0 + j*step.
    Forward: tiles 7n apart from `start`.  Reverse strand: rc(window i) is forward window
    n_windows-1-i of rc(region), region = seq[start : start + Leff]; tile j of THAT sequence starts
    L + 7n*j bases before the region's end and is staged reverse-complemented."""
    assert stride % POOL == 0
    n, m = pooled_len(L, k), stride // POOL
    J = n_tiles(n, m, n_windows)
    if not rc:
        return start, POOL * n, J
    Leff = stride * (n_windows - 1) + L
    return start + Leff - L, -POOL * n, J


def unfold(track_tiles, m, n_windows, rc=False):
    """track_tiles (J,U,n): pooled values of the tiles.  Returns (n_windows,U,n) in the caller's
    window order: ext[u][w][i] = tiles[(m i' + w) div n][u][(m i' + w) mod n], i' = i on the forward
    strand and n_windows-1-i on the reverse strand."""
    J, U, n = track_tiles.shape
    i = np.arange(n_windows)
    it = n_windows - 1 - i if rc else i
    P = m * it[:, None] + np.arange(n)[None, :]              # (W,n)
    assert P.max() < J * n
    return track_tiles[P // n, :, P % n].transpose(0, 2, 1)  # (W,n,U) -> (W,U,n)


def padded_reads(start, n_windows, stride, L, k):
    """Bases a window's pooled values depend on, relative to the region [start, start + Leff): the
    largest offset read (must stay below Leff: tiles are padded past it, and no valid window may see
    the padding)."""
    n, m = pooled_len(L, k), stride // POOL
    P = m * (n_windows - 1) + n - 1                          # the last pooled value any window reads
    return POOL * P + POOL - 1 + k - 1                       # last base under its last conv position
