"""Integer / fp64 numpy model of variant effects on known motifs (csrc/pwmvariants.hip,
explainn_amd/pwmvariants.py; DESIGN.md section 3 item 25, section 8 "Variant effects on known motifs"), written
from the contract in include/explainn_hip.h on top of pwmbest_model (the best site of a record) and
pwmsites_model (tables, null).

Each haplotype IS materialised here: seq[:pos] + allele + seq[pos + ref_len:].  The range the allele's windows
touch is cut from it, clipped to the haplotype, and handed to pwmbest_model.best_of_record; the start it
returns is shifted back by what was clipped on the left to give the window's index i.  Trimming, hit selection
and `effect` are modelled as motif_variants states them."""
import numpy as np

import pwmbest_model as bm
import pwmsites_model as pm

MAX_ALLELE = 128


def haplotype(codes, pos, ref_len, allele):
    codes = np.asarray(codes, dtype=np.uint8)
    return np.concatenate([codes[:pos], np.asarray(allele, dtype=np.uint8), codes[pos + ref_len:]])


def record_ok(pos, ref_len, alt_len, alt_off, seq_len, alt_bytes):
    return (pos >= 0 and ref_len >= 0 and alt_len >= 0 and pos + ref_len <= seq_len and alt_off >= 0 and
            alt_off + alt_len <= alt_bytes and ref_len <= MAX_ALLELE and alt_len <= MAX_ALLELE)


def allele_best(Sm, w, hap, pos, l, both=True, best=bm.best_of_record):
    """(bits, site) of one motif at one allele of l bases at pos of the materialised haplotype `hap`: the starts
    s = pos - w + 1 + i, i = 0 .. w + l - 2; site = (i << 1) | is_minus."""
    if w < 1 or w + l - 1 < 1:
        return 0, -1
    first = pos - w + 1                                    # the start of index 0
    lo, hi = max(first, 0), min(pos + l + w - 1, len(hap))
    bits, site = best(Sm, w, hap[lo:hi], both)
    if site < 0:
        return 0, -1
    return bits, site + ((lo - first) << 1)


def variant_best(S, lwidths, codes, pos, ref_len, alt_len, alt_off, alt, both=True, seq_len=None, alt_bytes=None,
                 best=bm.best_of_record):
    """(bits uint16 (M,V,2), site int32 (M,V,2), flags) as explainn_pwm_variant_best writes them.  flags bit 0:
    a byte above 4 in seq within wmax - 1 bases of an allele of a good record, or in its alt allele; bit 1: a bad
    record, which has no site."""
    M, wmax = S.shape[0], S.shape[1]
    seq_len = len(codes) if seq_len is None else seq_len
    alt_bytes = len(alt) if alt_bytes is None else alt_bytes
    seq = np.asarray(codes, dtype=np.uint8)[:seq_len]
    V = len(pos)
    bits, site, flags = np.zeros((M, V, 2), np.uint16), np.full((M, V, 2), -1, np.int32), 0
    for v in range(V):
        p, rl, al, ao = int(pos[v]), int(ref_len[v]), int(alt_len[v]), int(alt_off[v])
        if not record_ok(p, rl, al, ao, seq_len, alt_bytes):
            flags |= 2
            continue
        for A, allele in enumerate((seq[p:p + rl], np.asarray(alt, dtype=np.uint8)[ao:ao + al])):
            hap = haplotype(seq, p, rl, allele)
            l = len(allele)
            if np.any(hap[max(p - wmax + 1, 0):min(p + l + wmax - 1, len(hap))] > 4):
                flags |= 1
            for m in range(M):
                w = int(lwidths[m])
                bits[m, v, A], site[m, v, A] = allele_best(S[m], w if 1 <= w <= wmax else 0, hap, p, l, both, best)
    return bits, site, flags


def allele_brute(Sm, w, hap, pos, l, both=True):
    """The contract read off start by start over the FULL haplotype, with best_brute's scoring: every start s of
    the haplotype in turn, kept when it is one of s = pos - w + 1 + i, 0 <= i <= w + l - 2."""
    hap = np.minimum(np.asarray(hap, dtype=np.int64), 4)
    best, site = -1, -1
    if w >= 1:
        for s in range(len(hap) - w + 1):
            i = s - (pos - w + 1)
            if not 0 <= i <= w + l - 2:
                continue
            win = hap[s:s + w]
            if win.max() >= 4:
                continue
            fwd = sum(int(Sm[j][win[j]]) for j in range(w))
            rev = sum(int(Sm[j][3 - win[w - 1 - j]]) for j in range(w))
            for minus, sc in ((0, fwd), (1, rev)) if both else ((0, fwd),):
                if sc > best:
                    best, site = sc, (i << 1) | minus
    return max(best, 0), site


# ------------------------------------------------------------------------------------------- trimming
def trim(pos, ref, alt):
    """(pos, ref, alt) without the shared prefix, then without the shared suffix, of the two alleles."""
    ref, alt = np.asarray(ref, dtype=np.uint8), np.asarray(alt, dtype=np.uint8)
    a = 0
    while a < min(len(ref), len(alt)) and ref[a] == alt[a]:
        a += 1
    ref, alt = ref[a:], alt[a:]
    z = 0
    while z < min(len(ref), len(alt)) and ref[len(ref) - 1 - z] == alt[len(alt) - 1 - z]:
        z += 1
    return pos + a, ref[:len(ref) - z], alt[:len(alt) - z]


# ------------------------------------------------------------------------------------------- motif_variants
def effect_of(ref_iscore, alt_iscore, thr):
    r, a = ref_iscore >= thr, alt_iscore >= thr
    return "loss" if r and not a else "gain" if a and not r else "both" if r else "none"


def motif_variants(mats, codes, pos, ref_len, alts, pvalue=1e-4, bg=None, pc=0.1, bins=100, both=True, do_trim=True,
                   keep="hits"):
    """What motif_variants returns, as a dict of arrays ordered by variant, then motif (plus thresholds, tail)."""
    tab = bm.tables(mats, bg, pc, bins)
    tail, thr = pm.null_table(tab["S"], tab["live"], bins, tab["bg"], pvalue)
    codes = np.asarray(codes, dtype=np.uint8)
    tp, tr, ta = [], [], []
    for p, rl, a in zip(pos, ref_len, alts):
        p, r, a = (trim if do_trim else lambda *x: x)(int(p), codes[int(p):int(p) + int(rl)], np.asarray(a, np.uint8))
        tp.append(p), tr.append(len(r)), ta.append(np.asarray(a, dtype=np.uint8))
    alt_len = np.array([len(a) for a in ta], dtype=np.int64)
    alt_off = np.cumsum(alt_len) - alt_len
    pool = np.concatenate(ta + [np.zeros(0, np.uint8)])
    bits, site, flags = variant_best(tab["S"], tab["live"], codes, tp, tr, alt_len, alt_off, pool, both)
    isc = np.where(site >= 0, bits.astype(np.int64), -1)
    rows = {k: [] for k in ("variant", "motif", "ref_iscore", "alt_iscore", "ref_score", "alt_score", "delta",
                            "ref_pvalue", "alt_pvalue", "ref_offset", "alt_offset", "ref_strand", "alt_strand", "effect")}
    M = len(mats)
    for v in range(len(tp)):
        for m in range(M):
            r, a = int(isc[m, v, 0]), int(isc[m, v, 1])
            if keep == "hits" and not (r >= thr[m] or a >= thr[m]):
                continue
            w = int(tab["widths"][m])
            sc = [s / tab["scale"][m] + w * tab["lo"][m] if s >= 0 else np.nan for s in (r, a)]
            rows["variant"].append(v), rows["motif"].append(m)
            rows["ref_iscore"].append(r), rows["alt_iscore"].append(a)
            rows["ref_score"].append(sc[0]), rows["alt_score"].append(sc[1]), rows["delta"].append(sc[1] - sc[0])
            rows["ref_pvalue"].append(tail[m, r] if r >= 0 else 1.0)
            rows["alt_pvalue"].append(tail[m, a] if a >= 0 else 1.0)
            for A, name in enumerate(("ref", "alt")):
                s = int(site[m, v, A])
                rows[name + "_offset"].append((s >> 1) - w + 1 if s >= 0 else 0)
                rows[name + "_strand"].append(0 if s < 0 else 1 - 2 * (s & 1))
            rows["effect"].append(effect_of(r, a, int(thr[m])))
    out = {k: np.array(x) for k, x in rows.items()}
    out.update(pos=np.array(tp, dtype=np.int64), ref_len=np.array(tr, dtype=np.int32), alt_len=alt_len.astype(np.int32),
               thresholds=thr, tail=tail, flags=flags, tab=tab)
    return out


# ------------------------------------------------------------------------------------------- inputs
def edit_table(pos, ref_len, alts):
    """(pos int64, ref_len int32, alt_len int32, alt_off int32, alt uint8) of lists."""
    alts = [np.asarray(a, dtype=np.uint8).reshape(-1) for a in alts]
    alt_len = np.array([len(a) for a in alts], dtype=np.int64).reshape(len(alts))
    return (np.asarray(pos, dtype=np.int64).reshape(-1), np.asarray(ref_len, dtype=np.int32).reshape(-1),
            alt_len.astype(np.int32), (np.cumsum(alt_len) - alt_len).astype(np.int32),
            np.concatenate(alts + [np.zeros(0, np.uint8)]))


def random_variants(n, V, seed, max_len=10, snv_frac=0.6):
    """V variants of a sequence of n bases: SNVs, and MNVs / insertions / deletions / replacements of at most
    max_len bases (alleles without N).  Returns (pos, ref_len, alts)."""
    g = np.random.default_rng(seed)
    pos, ref_len, alts = [], [], []
    for _ in range(V):
        if g.random() < snv_frac:
            rl, al = 1, 1
        else:
            rl, al = int(g.integers(0, max_len + 1)), int(g.integers(0, max_len + 1))
        p = int(g.integers(0, n - rl + 1))
        pos.append(p), ref_len.append(rl), alts.append(g.integers(0, 4, size=al).astype(np.uint8))
    return pos, ref_len, alts
