"""Input encoding for the hot path (reference: explainn/sequence/__init__.py).

Same semantics -- rows A,C,G,T, any other letter an all-zero column, reverse complement =
flip of both axes -- but table-driven/vectorised instead of a per-character Python loop.
"""
import numpy as np

_LUT = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _LUT[ord(_c)] = _i
    _LUT[ord(_c.lower())] = _i
_COMP = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")


def encode_codes(seq):
    """Base codes 0..3 (4 = anything else) of one sequence, uint8 (L,)."""
    return _LUT[np.frombuffer(seq.encode("ascii", "replace"), dtype=np.uint8)]


def encode_codes_many(seqs):
    """(N, L) uint8 base codes of equal-length sequences: the input format of
    architectures.BaseCodes (L bytes per sequence instead of the 32*L of a float64 one-hot)."""
    out = np.empty((len(seqs), len(seqs[0]) if len(seqs) else 0), dtype=np.uint8)
    for i, s in enumerate(seqs):
        c = encode_codes(s)
        if len(c) != out.shape[1]:
            raise ValueError("sequence %d has length %d, expected %d" % (i, len(c), out.shape[1]))
        out[i] = c
    return out


def rc_codes(codes):
    """Reverse complement on base codes (what rc_one_hot_encoding does to the one-hot): reverse,
    A<->T, C<->G, N stays N."""
    codes = np.asarray(codes)
    r = codes[..., ::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


def codes_to_one_hot(codes, dtype=np.float32):
    """(N, L) codes -> (N, 4, L) one-hot (N columns all zero)."""
    codes = np.asarray(codes)
    return (codes[:, None, :] == np.arange(4, dtype=np.uint8)[None, :, None]).astype(dtype)


def one_hot_encode(seq):
    """sequence/__init__.py:8-28 -> float64 (4, L)."""
    codes = encode_codes(seq)
    out = np.zeros((4, len(codes)), dtype=float)
    ok = codes < 4
    out[codes[ok], np.nonzero(ok)[0]] = 1.0
    return out


def one_hot_encode_many(seqs):
    """sequence/__init__.py:4-6 -> (N, 4, L)."""
    return np.array([one_hot_encode(s) for s in seqs])


def one_hot_decode(encoded_seq):
    """sequence/__init__.py:34-47: columns with exactly one 1 -> letter, anything else -> N."""
    enc = np.asarray(encoded_seq)
    idx = enc.argmax(axis=0)
    ok = (enc == 1).sum(axis=0) == 1
    letters = np.array(list("ACGT"))[idx]
    return "".join(np.where(ok, letters, "N"))


def one_hot_decode_many(seqs):
    return np.array([one_hot_decode(s) for s in seqs])


def rc_one_hot_encoding(encoded_seq):
    """sequence/__init__.py:59-61."""
    return encoded_seq[::-1, ::-1]


def rc_one_hot_encoding_many(arr):
    """sequence/__init__.py:49-57."""
    return np.array([rc_one_hot_encoding(e) for e in arr])


def rc(seq):
    """sequence/__init__.py:67-69 (Bio.Seq.reverse_complement for the DNA alphabet)."""
    return seq.translate(_COMP)[::-1]


def rc_many(arr):
    return np.array([rc(s) for s in arr])


def _euler_shuffle(row, rng):
    """One dinucleotide-preserving shuffle of a 1-D code row (Altschul & Erickson 1985): a random
    arborescence towards the last symbol fixes every other vertex's last edge, the remaining edges
    of each vertex are shuffled, and the Euler path from the first symbol is read off."""
    n = len(row)
    if n < 3:
        return row.copy()
    last = int(row[-1])
    succ = [[] for _ in range(5)]
    for a, b in zip(row[:-1], row[1:]):
        succ[int(a)].append(int(b))
    verts = [v for v in range(5) if succ[v] or v == last]
    while True:
        # a last edge per vertex (other than the final one), drawn from its edges; accept when every
        # vertex reaches the final one through them
        pick = {v: int(rng.integers(len(succ[v]))) for v in verts if v != last and succ[v]}
        ok = True
        for v in pick:
            seen, cur = set(), v
            while cur != last and cur not in seen:
                seen.add(cur)
                cur = succ[cur][pick[cur]] if cur in pick else last
            if cur != last:
                ok = False
                break
        if ok:
            break
    order = {}
    for v in verts:
        edges = list(succ[v])
        if v in pick:
            tail = edges.pop(pick[v])
            edges = [edges[j] for j in rng.permutation(len(edges))] + [tail]
        else:
            edges = [edges[j] for j in rng.permutation(len(edges))]
        order[v] = edges
    out = np.empty(n, dtype=row.dtype)
    cur = int(row[0])
    used = {v: 0 for v in verts}
    out[0] = cur
    for i in range(1, n):
        nxt = order[cur][used[cur]]
        used[cur] += 1
        out[i] = nxt
        cur = nxt
    return out


def dinucleotide_shuffle(codes, n=1, seed=0):
    """Seeded shuffles of base-code rows that keep every dinucleotide count and the first and last
    base (Altschul-Erickson Euler path), the usual DNA baseline of Integrated Gradients.  N (code 4)
    is a fifth symbol.  codes: uint8 (L,) or (N,L); returns (n,L) or (N,n,L) uint8.  Host-side numpy."""
    codes = np.asarray(codes, dtype=np.uint8)
    if codes.ndim not in (1, 2):
        raise ValueError("codes must be (L,) or (N, L) base codes")
    if codes.size and codes.max() > 4:
        raise ValueError("base codes must be 0..4")
    if n < 1:
        raise ValueError("n must be at least 1")
    rows = codes[None] if codes.ndim == 1 else codes
    out = np.empty((rows.shape[0], n, rows.shape[1]), dtype=np.uint8)
    for i, row in enumerate(rows):
        rng = np.random.default_rng([int(seed), i])
        for r in range(n):
            out[i, r] = _euler_shuffle(row, rng)
    return out[0] if codes.ndim == 1 else out


def dinucleotide_shuffle_device(codes, n=1, seed=0, row0=0, max_rounds=0, return_capped=False):
    """dinucleotide_shuffle on the device (csrc/shuffle.hip): codes is a uint8 CUDA tensor (L,) or (N,L),
    the result a uint8 tensor (n,L) or (N,n,L) on the same device, enqueued on the current stream with no
    host synchronisation.  Same law as the host function -- every arrangement with the row's dinucleotide
    counts, first and last base equally likely, N a fifth symbol -- but a different random stream: a
    counter-based generator keyed by (seed, row0 + row index, shuffle index), so the shuffles of a seed
    differ from the host's sequence by sequence, and a row's shuffles do not depend on how the rows are
    split into calls (pass the offset of the first row as row0) or on n.  Bytes above 4 are read as N and
    come back as 4.  max_rounds caps the cycle-popping rounds of the last-exit sampler (0: 64*L, not
    reachable in practice); return_capped=True also returns a uint8 (n,) or (N,n) tensor, 1 where the cap
    was hit and the row's own last exits were used instead."""
    import torch

    from . import _lib
    if not torch.is_tensor(codes):
        raise ValueError("codes must be a uint8 tensor of (L,) or (N, L) base codes")
    if codes.dim() not in (1, 2):
        raise ValueError("codes must be (L,) or (N, L) base codes")
    if codes.dtype != torch.uint8:
        raise ValueError("base codes must be uint8")
    if n < 1:
        raise ValueError("n must be at least 1")
    if codes.device.type != "cuda":
        raise RuntimeError("dinucleotide_shuffle_device runs only on a HIP device; call .cuda() "
                           "(sequence.dinucleotide_shuffle is the host version)")
    rows = (codes[None] if codes.dim() == 1 else codes).contiguous()
    N, L = rows.shape
    if N and L < 1:
        raise ValueError("codes holds no positions")
    out = torch.empty((N, n, L), dtype=torch.uint8, device=rows.device)
    capped = torch.empty((N, n), dtype=torch.uint8, device=rows.device) if return_capped else None
    if N:
        _lib.call("explainn_dinucleotide_shuffle", rows.device, rows, N, L, int(n), int(seed) & (2 ** 64 - 1), int(row0),
                  int(max_rounds), out, capped)
    if codes.dim() == 1:
        out = out[0]
        capped = capped[0] if return_capped else None
    return (out, capped) if return_capped else out
