"""Numpy restatement of motif-site calling ("Motif sites"): from a float16
activation array to site lists -- what explainn_call_sites (csrc/sites.hip), explainn_amd.sites and
interpret.filter_site_list produce.  tests/test_sites_model.py checks it against the reference-fed
fixtures; tests/test_gpu_sites.py compares the device with it."""
import numpy as np


def rc_codes(codes):
    """Reverse complement of base codes: 3 - code, reversed, N (4) stays N."""
    r = np.asarray(codes)[..., ::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


def onehot(codes):
    """(B,L) codes -> (B,4,L) float32 one-hot, N = all-zero column."""
    codes = np.asarray(codes)
    return (codes[:, None, :] == np.arange(4)[None, :, None]).astype(np.float32)


def folded(sd):
    """(Wt (U,k,5) fp32 with the N entry 0, alpha, shift) of the eval-mode filter bank: BatchNorm1 folded
    into exp(alpha * sum + shift)."""
    w = np.asarray(sd["linears.0.weight"], dtype=np.float32)                  # (U,4,k)
    U, _, k = w.shape
    Wt = np.zeros((U, k, 5), dtype=np.float32)
    Wt[:, :, :4] = w.transpose(0, 2, 1)
    a = np.asarray(sd["linears.1.weight"], np.float64) / np.sqrt(np.asarray(sd["linears.1.running_var"], np.float64) + 1e-5)
    shift = np.asarray(sd["linears.1.bias"], np.float64) + a * (
        np.asarray(sd["linears.0.bias"], np.float64) - np.asarray(sd["linears.1.running_mean"], np.float64))
    return Wt, a.astype(np.float32), shift.astype(np.float32)


def kmer_acts(sd, codes, reverse=False):
    """float16 (U, P) activations of every start p of a 1-D code sequence, P = len - k + 1: the sum
    starts from 0 and adds the taps in j order in fp32.  reverse: the filter on rc(codes[p : p + k]),
    i.e. tap j meets comp(codes[p + k - 1 - j]), reported at the forward coordinate p."""
    Wt, alpha, shift = folded(sd)
    U, k, _ = Wt.shape
    c = np.minimum(np.asarray(codes, dtype=np.int64), 4)
    P = len(c) - k + 1
    acc = np.zeros((U, max(P, 0)), dtype=np.float32)
    if P <= 0:
        return acc.astype(np.float16)
    comp = np.array([3, 2, 1, 0, 4])
    for j in range(k):
        col = comp[c[k - 1 - j:k - 1 - j + P]] if reverse else c[j:j + P]
        acc = acc + Wt[:, j, :][:, col]
    return np.exp(alpha[:, None] * acc + shift[:, None], dtype=np.float32).astype(np.float16)


def period_mask(n_positions, period, k, first=0):
    """bool (n_positions,): False where a start's k-mer would cross a record boundary
    (p mod period > period - k); all True without a period."""
    p = first + np.arange(n_positions, dtype=np.int64)
    return np.ones(n_positions, dtype=bool) if period <= 0 else (p % period) <= period - k


def site_lists(acts16, thresholds, mask=None):
    """Per unit (positions int64 ascending, scores float32) where acts16 (U,P) float16 > threshold."""
    out = []
    for u in range(acts16.shape[0]):
        hit = acts16[u] > np.float32(thresholds[u])
        if mask is not None:
            hit = hit & mask
        pos = np.flatnonzero(hit).astype(np.int64)
        out.append((pos, acts16[u, pos].astype(np.float32)))
    return out


def reverse_lists_from_rc(acts16_rc, thresholds, k):
    """Reverse-strand lists in forward coordinates from the FORWARD activations of rc(seq): a site of
    rc(seq) at p' is the reverse-strand site at len - k - p' = P - 1 - p'."""
    return site_lists(acts16_rc[:, ::-1], thresholds)


def chunked_lists(acts16, thresholds, chunk, mask=None):
    """The union of calls over runs of `chunk` start positions, each reported start-relative and moved
    back by the chunk's first position."""
    U, P = acts16.shape
    parts = [[] for _ in range(U)]
    for p0 in range(0, P, chunk):
        sub = site_lists(acts16[:, p0:p0 + chunk], thresholds, None if mask is None else mask[p0:p0 + chunk])
        for u, (pos, sc) in enumerate(sub):
            parts[u].append((pos + p0, sc))
    return [(np.concatenate([p for p, _ in ps]) if ps else np.zeros(0, np.int64),
             np.concatenate([s for _, s in ps]) if ps else np.zeros(0, np.float32)) for ps in parts]


def fixed_length_lists(acts16, idxs, thresholds, rev_complement=False, cap=None):
    """interpret.py:375-429 on the dense (N,U,Lo) float16 array: per unit the (sequence index,
    position, strand) entries in (strand, idxs order, position) order, the first `cap` of them.  With
    rev_complement the reverse half's rows follow the forward half's."""
    N, U, Lo = acts16.shape
    idxs = np.asarray(idxs, dtype=np.int64)
    half = N // 2 if rev_complement else N
    out = []
    for u in range(U):
        ent = []
        for strand, base in ((1, 0), (-1, half)) if rev_complement else ((1, 0),):
            for i in idxs:
                for j in np.flatnonzero(acts16[i + base, u] > np.float32(thresholds[u])):
                    ent.append((i, j, strand))
        out.append(np.array(ent[:cap], dtype=np.int64).reshape(-1, 3))
    return out


def pfm_from_lists(codes, lists, k, rev_complement=False):
    """(pfm (U,k,4), nsites (U,)) recounted from (sequence index, position, strand) lists: the k-mer is
    read from the row the site was found on; an N counts for no letter."""
    codes = np.asarray(codes)
    half = len(codes) // 2 if rev_complement else len(codes)
    pfm = np.zeros((len(lists), k, 4), dtype=np.int64)
    nsites = np.zeros(len(lists), dtype=np.int64)
    for u, lst in enumerate(lists):
        nsites[u] = len(lst)
        for i, j, strand in lst:
            site = codes[i + (half if strand < 0 else 0), j:j + k]
            for t in range(k):
                if site[t] < 4:
                    pfm[u, t, site[t]] += 1
    return pfm, nsites
