"""Numpy restatement of the device's dinucleotide-preserving shuffle ("Shuffles"),
in plain loops: the generator, the order of draws, cycle popping, the cap and the walk.  Written from the
DESIGN text, not from csrc/shuffle.hip; tests/test_gpu_shuffle.py requires the kernel to give these bytes.
"""
import numpy as np

MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix(z):
    """The splitmix64 finaliser on a 64-bit integer."""
    z &= MASK
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & MASK
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


class Stream:
    """The draws of one (seed, row, r): draw t = mix(key + GOLD*(t+1)) >> 32, t = 0, 1, ...; reduced to
    [0, m) by the high half of the 32 x 32-bit product."""

    def __init__(self, seed, row, r):
        self.key = mix(mix(mix(seed + GOLD) ^ (row & MASK)) ^ r)
        self.t = 0

    def below(self, m):
        self.t += 1
        u = mix(self.key + GOLD * self.t) >> 32
        return (u * m) >> 32


def _pick(counts, j):
    """The first symbol whose cumulative count over b = 0..4 exceeds j."""
    acc = 0
    for b in range(5):
        acc += counts[b]
        if j < acc:
            return b
    raise AssertionError("draw outside the counts")


def _draw_exit(c, v, rng):
    row = [0 if b == v else int(c[v][b]) for b in range(5)]
    return _pick(row, rng.below(sum(row)))


def pair_counts(sym):
    c = np.zeros((5, 5), dtype=np.int64)
    for a, b in zip(sym[:-1], sym[1:]):
        c[a, b] += 1
    return c


def own_last_exits(sym):
    """e(v) = the successor at the last occurrence of v among positions 0..L-2."""
    own = {}
    for a, b in zip(sym[:-1], sym[1:]):
        own[int(a)] = int(b)
    return own


def walk(sym, exits, rng):
    """The walk with the last exits `exits` ({v: e(v)} for every v that needs one) reserved."""
    c = pair_counts(sym)
    for v, b in exits.items():
        c[v, b] -= 1
    out = np.empty(len(sym), dtype=np.uint8)
    cur = int(sym[0])
    out[0] = cur
    for i in range(1, len(sym)):
        m = int(c[cur].sum())
        if m > 0:
            b = _pick(c[cur], rng.below(m))
            c[cur, b] -= 1
        else:
            b = exits[cur]
        out[i] = b
        cur = b
    return out


def shuffle_one(row, seed, row_index, r, max_rounds=0):
    """(shuffled row, capped) of one (row, r)."""
    return shuffle_one_popped(row, seed, row_index, r, max_rounds)[:2]


def shuffle_one_popped(row, seed, row_index, r, max_rounds=0):
    """(shuffled row, capped, cycles popped) of one (row, r)."""
    sym = np.minimum(np.asarray(row, dtype=np.uint8), 4).astype(np.int64)
    L = len(sym)
    if L < 3:
        return sym.astype(np.uint8), 0, 0
    if max_rounds <= 0:
        max_rounds = 64 * L
    rng = Stream(seed, row_index, r)
    c = pair_counts(sym)
    last = int(sym[-1])
    need = [v for v in range(5) if v != last and v in set(int(s) for s in sym[:-1])]
    e = {v: _draw_exit(c, v, rng) for v in need}
    capped, popped = 0, 0
    while True:
        on_cycle = None
        for v in need:
            cur = v
            for _ in range(5):
                if cur != last:
                    cur = e[cur]
            if cur != last:
                on_cycle = cur
                break
        if on_cycle is None:
            break
        if popped >= max_rounds:
            e, capped = {v: own_last_exits(sym)[v] for v in need}, 1
            break
        cyc, w = set(), on_cycle
        while w not in cyc:
            cyc.add(w)
            w = e[w]
        for v in sorted(cyc):
            e[v] = _draw_exit(c, v, rng)
        popped += 1
    return walk(sym, e, rng), capped, popped


def shuffle(codes, n=1, seed=0, row0=0, max_rounds=0):
    """(out (N,n,L) uint8, capped (N,n) uint8) of codes (N,L): what explainn_dinucleotide_shuffle writes."""
    codes = np.asarray(codes, dtype=np.uint8)
    N, L = codes.shape
    out = np.empty((N, n, L), dtype=np.uint8)
    capped = np.zeros((N, n), dtype=np.uint8)
    for i in range(N):
        for r in range(n):
            out[i, r], capped[i, r] = shuffle_one(codes[i], seed, row0 + i, r, max_rounds)
    return out, capped


def _mix_lanes(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def shuffle_lanes(codes, n=1, seed=0, row0=0, max_rounds=0):
    """shuffle() with every (row, r) as one lane of numpy arrays: the same draws in the same order, loops
    over positions and rounds only.  test_shuffle_model.py holds it to shuffle(); the GPU tests use it for
    the large shapes."""
    codes = np.asarray(codes, dtype=np.uint8)
    N, L = codes.shape
    sym = np.minimum(codes, 4).astype(np.int64)
    M = N * n
    if L < 3 or M == 0:
        return np.repeat(sym.astype(np.uint8)[:, None], n, axis=1), np.zeros((N, n), dtype=np.uint8)
    if max_rounds <= 0:
        max_rounds = 64 * L
    rows = np.arange(N)
    c_row = np.zeros((N, 5, 5), dtype=np.int64)
    own_row = np.zeros((N, 5), dtype=np.int64)
    occ_row = np.zeros((N, 5), dtype=bool)
    for i in range(L - 1):
        np.add.at(c_row, (rows, sym[:, i], sym[:, i + 1]), 1)
        own_row[rows, sym[:, i]] = sym[:, i + 1]
        occ_row[rows, sym[:, i]] = True
    c = np.repeat(c_row, n, axis=0)
    own = np.repeat(own_row, n, axis=0)
    last = np.repeat(sym[:, -1], n)
    need = np.repeat(occ_row, n, axis=0)
    lanes = np.arange(M)
    need[lanes, last] = False
    with np.errstate(over="ignore"):
        row_id = (np.repeat(rows, n) + row0).astype(np.int64).view(np.uint64)
        key = _mix_lanes(_mix_lanes(np.uint64(mix(seed + GOLD)) ^ row_id) ^ np.tile(np.arange(n), N).astype(np.uint64))
    t = np.zeros(M, dtype=np.uint64)

    def below(m, idx):
        t[idx] += np.uint64(1)
        with np.errstate(over="ignore"):
            u = _mix_lanes(key[idx] + np.uint64(GOLD) * t[idx]) >> np.uint64(32)
        return ((u * m.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)

    def draw_exit(idx, v):
        rc = c[idx, v, :].copy()
        rc[:, v] = 0
        j = below(rc.sum(axis=1), idx)
        return (np.cumsum(rc, axis=1) <= j[:, None]).sum(axis=1)

    e = np.zeros((M, 5), dtype=np.int64)
    for v in range(5):
        idx = np.nonzero(need[:, v])[0]
        e[idx, v] = draw_exit(idx, v)
    capped = np.zeros(M, dtype=np.uint8)
    popped = np.zeros(M, dtype=np.int64)
    active = lanes
    while active.size:
        u = np.full(active.size, 8, dtype=np.int64)
        for v in range(5):
            cur = np.full(active.size, v, dtype=np.int64)
            for _ in range(5):
                cur = np.where(cur != last[active], e[active, cur], cur)
            hit = (u == 8) & need[active, v] & (cur != last[active])
            u[hit] = cur[hit]
        active, u = active[u != 8], u[u != 8]
        cap = popped[active] >= max_rounds
        e[active[cap]] = own[active[cap]]
        capped[active[cap]] = 1
        active, u = active[~cap], u[~cap]
        cyc = np.zeros((active.size, 5), dtype=bool)
        for _ in range(4):
            cyc[np.arange(active.size), u] = True
            u = e[active, u]
        for v in range(5):
            idx = active[cyc[:, v]]
            e[idx, v] = draw_exit(idx, v)
        popped[active] += 1
    for v in range(5):
        idx = np.nonzero(need[:, v])[0]
        c[idx, v, e[idx, v]] -= 1
    out = np.empty((M, L), dtype=np.uint8)
    cur = np.repeat(sym[:, 0], n)
    out[:, 0] = cur
    for i in range(1, L):
        rc = c[lanes, cur, :]
        m = rc.sum(axis=1)
        act = np.nonzero(m > 0)[0]
        nxt = e[lanes, cur]
        b = (np.cumsum(rc[act], axis=1) <= below(m[act], act)[:, None]).sum(axis=1)
        nxt[act] = b
        c[act, cur[act], b] -= 1
        out[:, i] = nxt
        cur = nxt
    return out.reshape(N, n, L), capped.reshape(N, n)


def arrangements(row):
    """Every distinct arrangement with the row's pair counts, first and last symbol (DFS), as tuples."""
    sym = [min(int(s), 4) for s in row]
    c = pair_counts(np.asarray(sym))
    found, path = [], [sym[0]]

    def rec():
        if len(path) == len(sym):
            if path[-1] == sym[-1]:
                found.append(tuple(path))
            return
        a = path[-1]
        for b in range(5):
            if c[a, b]:
                c[a, b] -= 1
                path.append(b)
                rec()
                path.pop()
                c[a, b] += 1

    rec()
    return found
