"""GPU: variant effects on known motifs (csrc/pwmvariants.hip through explainn_pwm_variant_best,
explainn_amd/pwmvariants.py and `python -m explainn_amd.pwmvariants`) against the numpy model
tests/pwmvariants_model.py, and against explainn_pwm_record_best on spliced records.  Every comparison is exact
(array_equal)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pwmbest_model as bm  # noqa: E402
import pwmsites_model as pm  # noqa: E402
import pwmvariants_model as vm  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7
GUARD = 96                       # elements past every table and output, filled with a marker
MARK = 0xA5
N_SEQ = 2000
A, N = 0, 4


def _lib():
    from explainn_amd import _lib
    return _lib


def _guarded(a, fill):
    """A device tensor of a's values followed by GUARD elements of `fill` (never an empty buffer)."""
    a = np.ascontiguousarray(a)
    full = np.concatenate([a.reshape(-1), np.full(GUARD, fill, dtype=a.dtype)])
    return torch.from_numpy(full).cuda()


def _call(S, lw, codes, table, both=True, want_site=True, seq_len=None, alt_bytes=None, want_flags=True):
    """One explainn_pwm_variant_best call on host arrays: (bits uint16 (M,V,2), site int32 (M,V,2) or None, flags).
    Every input and output has a guard region behind it: the inputs' holds bytes above 4 (a read of it would raise
    flag bit 0), the outputs' must come back untouched."""
    lib = _lib()
    pos, ref_len, alt_len, alt_off, pool = table
    M, wmax, V = S.shape[0], S.shape[1], len(pos)
    seq_len = len(codes) if seq_len is None else seq_len
    alt_bytes = len(pool) if alt_bytes is None else alt_bytes
    Sd, wd = _guarded(S, 0), _guarded(np.asarray(lw, dtype=np.int32), 0)
    cd, ad = _guarded(np.asarray(codes, dtype=np.uint8), MARK), _guarded(np.asarray(pool, dtype=np.uint8), MARK)
    pd = _guarded(np.asarray(pos, dtype=np.int64), -1)
    rd, ld, od = (_guarded(np.asarray(x, dtype=np.int32), -1) for x in (ref_len, alt_len, alt_off))
    n = M * V * 2
    bits = torch.full((n + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    site = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") if want_site else None
    flags = torch.zeros(1 + GUARD, dtype=torch.int32, device="cuda") if want_flags else None
    lib.check(lib.load().explainn_pwm_variant_best(
        cd.data_ptr(), seq_len, pd.data_ptr(), rd.data_ptr(), ld.data_ptr(), od.data_ptr(), ad.data_ptr(), alt_bytes,
        V, int(both), Sd.data_ptr(), wd.data_ptr(), M, wmax, bits.data_ptr(), site.data_ptr() if want_site else None,
        flags.data_ptr() if want_flags else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert bool((bits[n:] == SENTINEL).all()) and (site is None or bool((site[n:] == SENTINEL).all()))
    assert flags is None or bool((flags[1:] == 0).all())
    return (bits[:n].cpu().numpy().view(np.uint16).reshape(M, V, 2),
            site[:n].cpu().numpy().reshape(M, V, 2) if want_site else None, int(flags[0].item()) if want_flags else None)


def _check(S, lw, codes, variants, both=True, flag=0):
    """bits, site and flags equal the model's on (pos, ref_len, alts); returns (bits, site)."""
    table = vm.edit_table(*variants)
    want_bits, want_site, want_flag = vm.variant_best(S, lw, codes, *table, both=both)
    bits, site, got_flag = _call(S, lw, codes, table, both)
    assert np.array_equal(bits, want_bits) and np.array_equal(site, want_site)
    assert got_flag == want_flag == flag
    return bits, site


def _tables(widths, seed, extra=()):
    tab = bm.tables(pm.dirichlet_motifs(widths, seed) + list(extra))
    return tab["S"], tab["live"]


def _palindrome(w=8, seed=3):
    half = np.random.default_rng(seed).dirichlet(np.full(4, 0.3), size=w // 2)
    return np.concatenate([half, half[::-1, ::-1]])


def _rnd(k, seed):
    return np.random.default_rng(seed).integers(0, 4, size=k).astype(np.uint8)


def _kinds(n, seed):
    """SNVs, MNVs, pure insertions, pure deletions, replacements and alleles of 128 bases, the sequence's two ends
    and the insertion behind its last base: (pos, ref_len, alts)."""
    pos, ref_len, alts = vm.random_variants(n, 60, seed=seed, max_len=10)
    extra = [(0, 1, 1), (n - 1, 1, 1), (n, 0, 3), (0, 0, 2), (0, 4, 0), (n - 5, 5, 0), (500, 0, 0), (600, 3, 3),
             (700, 128, 1), (800, 1, 128), (900, 128, 128), (1000, 0, 128), (1100, 128, 0), (n - 128, 128, 2),
             (0, 128, 0), (n, 0, 128), (1, 1, 1), (n - 2, 2, 5), (300, 0, 1), (301, 1, 0)]
    for k, (p, r, a) in enumerate(extra):
        pos.append(p), ref_len.append(r), alts.append(_rnd(a, seed * 100 + k))
    return pos, ref_len, alts


@pytest.fixture(scope="module")
def codes():
    return pm.random_codes(N_SEQ, seed=21, n_frac=0.01)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("M", [1, 15, 16, 17, 33])
def test_motif_counts_around_the_group(M, codes):
    widths = list(np.random.default_rng(M).integers(6, 25, size=M))
    S, lw = _tables(widths, seed=7)
    bits, site = _check(S, lw, codes, _kinds(N_SEQ, seed=M))
    assert np.any(bits > 0) and np.any((site >= 0) & (site & 1 == 1)) and np.any((site >= 0) & (site & 1 == 0))


@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
def test_every_width_and_an_empty_motif(both, codes):
    """Widths 1, 2, 6..24 and 64 (wmax 64), one empty motif and one width past wmax, against every kind of variant."""
    S, lw = _tables([1, 2] + list(range(6, 25)) + [64, 9, 9], seed=2)
    lw = lw.copy()
    lw[-2], lw[-1] = 0, 65
    variants = _kinds(N_SEQ, seed=3)
    bits, site = _check(S, lw, codes, variants, both)
    assert np.all(site[-2:] == -1) and np.all(bits[-2:] == 0)
    rl, al = np.array(variants[1]), np.array([len(a) for a in variants[2]])
    assert np.all(site[0, rl == 0, 0] == -1) and np.all(site[0, al == 0, 1] == -1)    # w = 1 at l = 0: no window
    assert np.any(site[1, rl == 0, 0] >= 0)                                           # w = 2 at l = 0: one window
    if not both:
        assert np.all(site[site >= 0] & 1 == 0)
    # the index of a site stays inside 0 .. w + l - 2
    for m, w in enumerate(lw[:-2]):
        for k, l in enumerate((rl, al)):
            s = site[m, :, k]
            assert np.all((s >> 1)[s >= 0] <= (w + l - 2)[s >= 0])


def test_wmax_of_one(codes):
    S, lw = _tables([1, 1, 1], seed=4)
    assert S.shape[1] == 1
    bits, site = _check(S, lw, codes, _kinds(N_SEQ, seed=5))
    assert np.any(site >= 0) and np.any(site == -1)


def test_n_and_bytes_above_four(codes):
    S, lw = _tables([6, 12, 19, 24], seed=6)
    clean = pm.random_codes(N_SEQ, seed=8, n_frac=0.0)
    variants = ([400, 800, 1200, 1600], [1, 0, 2, 1],
                [_rnd(1, 1), np.array([1, N, 2], np.uint8), _rnd(0, 2), np.array([N], np.uint8)])
    flank = clean.copy()
    flank[395], flank[1203], flank[1250] = N, N, N                # N in a flank, left and right
    bits, site = _check(S, lw, flank, variants)
    assert np.all(site[:, 3, 1] == -1) and np.all(site[:, 3, 0] >= 0)    # an SNV to N: no live window on alt
    assert np.all(site[:, 1, 1] >= 0)                                     # N inside an insertion: its ends still count
    odd = flank.copy()
    odd[395], odd[1203] = 7, 255                                  # the same places, bytes above 4: read as N
    b2, s2 = _check(S, lw, odd, variants, flag=1)
    assert np.array_equal(b2, bits) and np.array_equal(s2, site)
    far = clean.copy()
    far[400 + 24], far[400 - 24] = 9, 9                            # one base past the segment (wmax = 24): not read
    far[1250] = 9
    _check(S, lw, far, (variants[0][:1], variants[1][:1], variants[2][:1]), flag=0)
    inside = (variants[0], variants[1], [variants[2][0], np.array([1, 200, 2], np.uint8), variants[2][2], variants[2][3]])
    b3, s3 = _check(S, lw, clean, inside, flag=1)                 # a byte above 4 in an alt allele
    want = _check(S, lw, clean, variants)
    assert np.array_equal(b3, want[0]) and np.array_equal(s3, want[1])


def test_bad_records_have_no_site_and_nothing_is_read_or_written_outside(codes):
    """Each kind of bad record: flag bit 1, no site on both alleles for every motif; the good records around them are
    scored as alone.  The tables are followed by guard regions (bytes above 4 behind seq and alt: reading one would
    raise flag bit 0) and the outputs by sentinels that _call checks."""
    S, lw = _tables([6, 13, 24, 64], seed=9)
    clean = pm.random_codes(N_SEQ, seed=10, n_frac=0.0)
    pool = _rnd(40, 11)
    good = [(100, 1, 1, 0), (N_SEQ - 1, 1, 2, 1), (N_SEQ, 0, 3, 3), (0, 2, 0, 6)]
    bad = [(-1, 1, 1, 0), (-(1 << 40), 1, 1, 0), (100, -1, 1, 0), (100, 1, -1, 0), (N_SEQ, 1, 1, 0),
           (N_SEQ - 1, 2, 1, 0), (1 << 40, 0, 1, 0), (100, 1, 1, -1), (100, 1, 2, 39), (100, 1, 1, 40),
           (100, 1, 1, 2147483647), (100, 129, 1, 0), (100, 1, 129, 0), (100, 2147483647, 1, 0),
           ((1 << 63) - 1, 1, 1, 0), (100, 1, 2147483647, 1)]
    for rec in bad:
        rows = good[:2] + [rec] + good[2:]
        table = tuple(np.array([r[i] for r in rows], dtype=np.int64 if i == 0 else np.int32) for i in range(4)) + (pool,)
        want = vm.variant_best(S, lw, clean, *table)
        bits, site, flag = _call(S, lw, clean, table)
        assert flag == want[2] == 2, rec
        assert np.array_equal(bits, want[0]) and np.array_equal(site, want[1]), rec
        assert np.all(site[:, 2] == -1) and np.all(bits[:, 2] == 0) and np.all(site[:3, [0, 1]] >= 0), rec
    # a table that is good only for a shorter alt pool / sequence than the buffers hold
    table = tuple(np.array([r[i] for r in good], dtype=np.int64 if i == 0 else np.int32) for i in range(4)) + (pool,)
    bits, site, flag = _call(S, lw, clean, table, alt_bytes=5)
    want = vm.variant_best(S, lw, clean, *table, alt_bytes=5)
    assert flag == want[2] == 2 and np.array_equal(site, want[1]) and np.all(site[:, 2] == -1)
    bits, site, flag = _call(S, lw, clean, table, seq_len=N_SEQ - 1)
    want = vm.variant_best(S, lw, clean, *table, seq_len=N_SEQ - 1)
    assert flag == want[2] == 2 and np.array_equal(site, want[1]) and np.array_equal(bits, want[0])


@pytest.mark.parametrize("both", [False, True], ids=["fwd", "both"])
def test_ties_go_to_the_lowest_index_then_plus(both):
    pal = _palindrome(8)
    S, lw = _tables([6, 11], seed=12, extra=[pal, _palindrome(12, seed=5)])
    flat = pm.random_codes(N_SEQ, seed=13, n_frac=0.0)
    flat[500:700] = A                                             # poly-A: every window of it scores alike
    variants = ([600, 610, 620, 630, 1000, 1500], [1, 0, 3, 1, 1, 2],
                [np.array([A], np.uint8), np.array([A, A], np.uint8), np.array([A], np.uint8), _rnd(1, 1), _rnd(1, 2),
                 _rnd(5, 3)])
    bits, site = _check(S, lw, flat, variants, both)
    assert np.all(site[:, :3, :] >> 1 == 0)                       # all ties: index 0
    assert np.all(site[2:][site[2:] >= 0] & 1 == 0)               # a palindrome's strands tie everywhere: '+'
    if both:
        assert np.any((site[:2] >= 0) & (site[:2] & 1 == 1))


@pytest.mark.parametrize("V", [0, 1, 3, 4, 5, 257])
def test_variant_counts(V, codes):
    S, lw = _tables([7, 10, 15, 21, 8], seed=14)
    variants = vm.random_variants(N_SEQ, V, seed=V + 1, max_len=10)
    bits, site = _check(S, lw, codes, variants)
    assert bits.shape == (5, V, 2)


def test_without_the_site_output_and_without_flags(codes):
    S, lw = _tables([7, 10, 15, 21, 8], seed=14)
    table = vm.edit_table(*_kinds(N_SEQ, seed=15))
    want = vm.variant_best(S, lw, codes, *table)
    bits, site, flags = _call(S, lw, codes, table, want_site=False, want_flags=False)
    assert site is None and flags is None and np.array_equal(bits, want[0])


def test_round_robin_equals_slices(codes):
    """More variants than the grid has wavefronts: a wave takes several variants in turn over the same staged bytes.
    The same bits as the calls on slices of 300 variants, each wave's first; the first slice is held to the model."""
    S, lw = _tables(list(np.random.default_rng(16).integers(6, 25, size=33)), seed=16)
    V = 6000
    table = vm.edit_table(*vm.random_variants(N_SEQ, V, seed=17, max_len=10))
    bits, site, flag = _call(S, lw, codes, table)
    assert flag == 0
    for v0 in range(0, V, 300):
        part = tuple(t[v0:v0 + 300] for t in table[:4]) + (table[4],)
        b, s, _ = _call(S, lw, codes, part)
        assert np.array_equal(bits[:, v0:v0 + 300], b) and np.array_equal(site[:, v0:v0 + 300], s), v0
    part = tuple(t[:300] for t in table[:4]) + (table[4],)
    want = vm.variant_best(S, lw, codes, *part)
    assert np.array_equal(bits[:, :300], want[0]) and np.array_equal(site[:, :300], want[1])


def test_equals_record_best_on_spliced_records(codes):
    """Per width group, the touched range of every haplotype as a record of its own through the existing
    explainn_pwm_record_best: the same bits, and the same sites once shifted back by what the haplotype's ends cut."""
    from explainn_amd import pwmenrich
    widths = [6, 9, 9, 12, 12, 12, 19, 24, 1, 2]
    S, lw = _tables(widths, seed=18)
    variants = _kinds(N_SEQ, seed=19)
    pos, ref_len, alt_len, alt_off, pool = table = vm.edit_table(*variants)
    bits, site, _ = _call(S, lw, codes, table)
    V = len(pos)
    for w, idx in bm.width_groups(lw):
        recs, shift = [], []
        for v in range(V):
            for allele in (codes[pos[v]:pos[v] + ref_len[v]], pool[alt_off[v]:alt_off[v] + alt_len[v]]):
                hap = vm.haplotype(codes, int(pos[v]), int(ref_len[v]), allele)
                first = int(pos[v]) - w + 1
                lo, hi = max(first, 0), min(int(pos[v]) + len(allele) + w - 1, len(hap))
                recs.append(hap[lo:max(hi, lo)])
                shift.append(lo - first)
        off = np.zeros(len(recs) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in recs], out=off[1:])
        flat = torch.from_numpy(np.concatenate(recs + [np.full(1, 4, np.uint8)])).cuda()
        b, s = pwmenrich.record_best_device(torch.from_numpy(S[idx]).cuda(), torch.from_numpy(lw[idx]).cuda(), flat,
                                            torch.from_numpy(off).cuda())
        b, s = b.cpu().numpy().view(np.uint16), s.cpu().numpy()
        s = np.where(s >= 0, s + (np.array(shift, dtype=np.int32) << 1)[None, :], -1)
        assert np.array_equal(bits[idx].reshape(len(idx), -1), b), w
        assert np.array_equal(site[idx].reshape(len(idx), -1), s), w


def test_argument_errors(codes):
    lib = _lib()
    L = lib.load()
    S, lw = _tables([6, 8], seed=20)
    t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in
         (codes, np.array([5], np.int64), np.array([1], np.int32), np.array([1], np.int32), np.array([0], np.int32),
          np.array([2], np.uint8), S, lw)]
    out = torch.zeros(4, dtype=torch.int16, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(seq=t[0].data_ptr(), seq_len=N_SEQ, pos=t[1].data_ptr(), alt=t[5].data_ptr(), alt_bytes=1, V=1, M=2, wmax=8,
             bits=out.data_ptr()):
        return L.explainn_pwm_variant_best(seq, seq_len, pos, t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(), alt,
                                           alt_bytes, V, 1, t[6].data_ptr(), t[7].data_ptr(), M, wmax, bits, None, None,
                                           stream)

    assert call() == lib.OK
    for kw in (dict(seq_len=-1), dict(alt_bytes=-1), dict(V=-1), dict(V=1 << 30), dict(M=-1), dict(wmax=0),
               dict(wmax=65), dict(pos=None), dict(bits=None), dict(seq=None), dict(alt=None)):
        assert call(**kw) == lib.E_ARG, kw
        assert b"pwm_variant_best" in L.explainn_last_error()
    assert call(M=0, bits=None) == lib.OK and call(V=0, pos=None) == lib.OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------- motif_variants
@pytest.fixture(scope="module")
def planted():
    """Eight motifs; the consensus of motif 5 planted at 300 ('+') and at 900 ('-') of 2000 bases, and mutated at its
    most informative column at 1400: an SNV there restores it.  Returns (mats, codes, variants, model result)."""
    mats = pm.dirichlet_motifs([6, 8, 10, 12, 12, 12, 15, 19], seed=22, alpha=0.1)
    seq = pm.random_codes(N_SEQ, seed=23, n_frac=0.005)
    seq[280:340], seq[880:940], seq[1380:1440] = (pm.random_codes(60, seed=s, n_frac=0.0) for s in (1, 2, 3))
    m = mats[5]
    col = int(np.argmax(np.max(m, axis=1) - np.sort(m, axis=1)[:, -2]))
    worst, top = int(np.argmin(m[col])), int(np.argmax(m[col]))
    pm.plant(seq, m, 300)
    pm.plant(seq, m, 900, reverse=True)
    pm.plant(seq, m, 1400)
    seq[1400 + col] = worst
    pos, ref_len, alts = vm.random_variants(N_SEQ, 60, seed=24, max_len=10)
    keep = [i for i, p in enumerate(pos) if not any(a - 30 <= p <= a + 30 for a in (300, 900, 1400))]
    pos, ref_len, alts = [pos[i] for i in keep], [ref_len[i] for i in keep], [alts[i] for i in keep]
    # the loss on '+', the loss on '-' (the column mirrored, the base complemented), the gain, and a VCF-style
    # anchored deletion and insertion inside the planted sites
    pos += [300 + col, 900 + 11 - col, 1400 + col, 302, 903]
    ref_len += [1, 1, 1, 3, 1]
    alts += [np.array([worst], np.uint8), np.array([3 - worst], np.uint8), np.array([top], np.uint8), seq[302:303].copy(),
             np.concatenate([seq[903:904], _rnd(4, 9)])]
    return mats, seq, (pos, ref_len, alts), col


def _same(eff, want, mats):
    """The integer fields equal the model's; the float fields follow, exactly, from the package's own tables: the
    log-odds by PwmCalls.score's formula on quantise()'s scale and lo, the p-values gathered from the device's tail."""
    from explainn_amd import pwmvariants as pv
    for f in ("variant", "motif", "ref_iscore", "alt_iscore", "ref_offset", "alt_offset", "ref_strand", "alt_strand"):
        assert np.array_equal(getattr(eff, f), want[f]), f
    assert np.array_equal(eff.effect_names, want["effect"])
    _, widths, scale, lo = pv._pwm.quantise(mats)
    tail = pv._pwm.score_null(bm.named(mats), 1.0).tail.cpu().numpy()
    m = eff.motif
    for name in ("ref", "alt"):
        isc, none = getattr(eff, name + "_iscore"), getattr(eff, name + "_iscore") < 0
        assert np.array_equal(getattr(eff, name + "_score")[~none], (isc / scale[m] + widths[m] * lo[m])[~none])
        assert np.all(np.isnan(getattr(eff, name + "_score")[none]))
        assert np.array_equal(getattr(eff, name + "_pvalue")[~none], tail[m, isc][~none])
        assert np.all(getattr(eff, name + "_pvalue")[none] == 1.0)
    assert np.array_equal(eff.delta, eff.alt_score - eff.ref_score, equal_nan=True)
    assert np.array_equal(eff.pos, want["pos"]) and np.array_equal(eff.ref_len, want["ref_len"])
    assert np.array_equal(eff.alt_len, want["alt_len"]) and np.array_equal(eff.thresholds, want["thresholds"])


@pytest.mark.parametrize("strands", ["both", "fwd"])
def test_motif_variants_equals_the_model_for_every_chunking(planted, strands):
    from explainn_amd import pwmvariants as pv
    mats, seq, variants, col = planted
    want = vm.motif_variants(mats, seq, *variants, pvalue=1e-4, both=strands == "both")
    assert len(want["motif"]) > 3
    whole = pv.motif_variants(bm.named(mats), seq, *variants, pvalue=1e-4, strands=strands)
    _same(whole, want, mats)
    assert whole.flags == 0
    for chunk in (1, 7):
        _same(pv.motif_variants(bm.named(mats), torch.from_numpy(seq).cuda(), *variants, pvalue=1e-4, strands=strands,
                                chunk_variants=chunk), want, mats)
    # the model's own fp64 tail stays far from the cutoff: the thresholds do not hang on a rounding
    assert pm.min_relative_gap(want["tail"], want["tab"]["live"], 100, 1e-4) > 1e-9


def test_hits_are_the_filtered_all_and_trim_moves_the_anchor(planted):
    from explainn_amd import pwmvariants as pv
    mats, seq, variants, col = planted
    every = pv.motif_variants(bm.named(mats), seq, *variants, pvalue=1e-4, keep="all")
    hits = pv.motif_variants(bm.named(mats), seq, *variants, pvalue=1e-4)
    V = len(variants[0])
    assert len(every) == V * len(mats) and 0 < len(hits) < len(every)
    _same(every, vm.motif_variants(mats, seq, *variants, pvalue=1e-4, keep="all"), mats)
    thr = every.thresholds[every.motif]
    mask = (every.ref_iscore >= thr) | (every.alt_iscore >= thr)
    for f in pv.MotifVariantEffects.FIELDS:
        assert np.array_equal(getattr(every, f)[mask], getattr(hits, f), equal_nan=True), f
    assert set(every.effect_names[~mask]) == {"none"} and "none" not in set(hits.effect_names)
    # the anchored deletion seq[302:305] -> seq[302] and the anchored insertion behind 903 lose their anchor
    assert hits.pos[V - 2] == 303 and hits.ref_len[V - 2] == 2 and hits.alt_len[V - 2] == 0
    assert hits.pos[V - 1] == 904 and hits.ref_len[V - 1] == 0
    raw = pv.motif_variants(bm.named(mats), seq, *variants, pvalue=1e-4, trim=False)
    assert raw.pos[V - 2] == 302 and raw.ref_len[V - 2] == 3 and raw.alt_len[V - 2] == 1
    _same(raw, vm.motif_variants(mats, seq, *variants, pvalue=1e-4, do_trim=False), mats)


def test_planted_site_is_lost_and_regained(planted):
    from explainn_amd import pwmvariants as pv
    mats, seq, variants, col = planted
    eff = pv.motif_variants(bm.named(mats), seq, *variants, pvalue=1e-6)
    V = len(variants[0])
    at = {(int(v), int(m)): k for k, (v, m) in enumerate(zip(eff.variant, eff.motif))}
    loss, loss_minus, gain = at[(V - 5, 5)], at[(V - 4, 5)], at[(V - 3, 5)]
    names = eff.effect_names
    assert names[loss] == "loss" and names[loss_minus] == "loss" and names[gain] == "gain"
    assert "loss" in set(names) and "gain" in set(names)
    assert eff.delta[loss] < 0 and eff.delta[gain] > 0 and eff.ref_pvalue[loss] <= 1e-6 < eff.alt_pvalue[loss]
    assert eff.ref_offset[loss] == -col and eff.ref_strand[loss] == 1
    assert eff.ref_offset[loss_minus] == -(11 - col) and eff.ref_strand[loss_minus] == -1
    assert eff.alt_offset[gain] == -col and eff.alt_iscore[gain] == eff.ref_iscore[loss]
    # the deletion and the insertion inside the planted sites destroy them too
    assert names[at[(V - 2, 5)]] == "loss" and names[at[(V - 1, 5)]] == "loss"


def test_refusals_on_the_device(planted):
    from explainn_amd import pwmvariants as pv
    mats, seq, variants, col = planted
    dev = torch.from_numpy(seq).cuda()
    with pytest.raises(ValueError, match="longer than 128"):
        pv.motif_variants(bm.named(mats), dev, [50], [1], [np.full(130, (seq[50] + 1) % 4, np.uint8)])
    with pytest.raises(ValueError, match="REF allele"):
        pv.motif_variants(bm.named(mats), dev, [50], [1], [np.zeros(1, np.uint8)], check_ref=[np.array([(seq[50] + 1) % 4], np.uint8)])
    old = pv.ALL_BYTES
    pv.ALL_BYTES = 1000
    try:
        with pytest.raises(ValueError, match="keep='all'"):
            pv.motif_variants(bm.named(mats), dev, *variants, keep="all")
    finally:
        pv.ALL_BYTES = old
    empty = pv.motif_variants(bm.named(mats), dev, [], [], [])
    assert len(empty) == 0 and empty.delta.dtype == np.float64 and empty.flags == 0
    assert len(pv.motif_variants([], dev, *variants)) == 0


def test_cli_round_trip(planted, tmp_path):
    from explainn_amd import motifs as mo
    from explainn_amd import pwmvariants as pv
    from explainn_amd.variants import Variant
    mats, seq, variants, col = planted
    letters = np.array(list("ACGTN"))
    recs = {"chrA": seq[:700], "chrB": seq[700:1300], "chrC": seq[1300:]}
    with open(tmp_path / "x.fa", "w") as fh:
        for rid, c in recs.items():
            fh.write(">%s\n%s\n" % (rid, "".join(letters[c])))
    text = lambda c: "".join(letters[np.asarray(c, dtype=np.int64)])
    m = mats[5]
    worst, top = int(np.argmin(m[col])), int(np.argmax(m[col]))
    lines = [("chrA", 300 + col, "loss", text(seq[300 + col:301 + col]), "ACGT"[worst]),
             ("chrB", 200 + 11 - col, "lossrc", text(seq[911 - col:912 - col]), "ACGT"[3 - worst]),
             ("chrC", 100 + col, "gain", text(seq[1400 + col:1401 + col]), "ACGT"[top]),
             ("chrA", 302, "del", text(seq[302:305]), text(seq[302:303])),
             ("chrZ", 5, "nowhere", "A", "C"),
             ("chrB", 203, "sym", text(seq[903:904]), "<DEL>")]
    with open(tmp_path / "x.vcf", "w") as fh:
        fh.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for chrom, p, vid, ref, alt in lines:
            fh.write("%s\t%d\t%s\t%s\t%s\n" % (chrom, p + 1, vid, ref, alt))
    mo.write_meme(str(tmp_path / "m.meme"), bm.named(mats))
    pv.main([str(tmp_path / "m.meme"), str(tmp_path / "x.fa"), str(tmp_path / "x.vcf"), "--pvalue", "1e-6", "-o",
             str(tmp_path / "out.tsv")])
    rows = [l.rstrip("\n").split("\t") for l in open(tmp_path / "out.tsv")]
    assert rows[0] == pv.HEADER.split()
    got = {(r[2], r[5]): r for r in rows[1:]}
    motif = mo.read_motifs(str(tmp_path / "m.meme"))[5][0]
    assert got[("loss", motif)][7] == "loss" and got[("lossrc", motif)][7] == "loss" and got[("gain", motif)][7] == "gain"
    assert got[("del", motif)][7] == "loss"
    assert got[("loss", motif)][:5] == ["chrA", str(300 + col + 1), "loss", lines[0][3], lines[0][4]]
    assert got[("loss", motif)][13:15] == [str(-col), "+"] and got[("lossrc", motif)][14] == "-"
    assert not any(r[2] in ("nowhere", "sym") for r in rows[1:])
    # the same rows as the library call on the same motifs and records
    vs = [Variant(c, p, i, r, a) for c, p, i, r, a in lines[:5]]
    index, results = pv.motif_variant_records(mo.read_motifs(str(tmp_path / "m.meme")), list(recs.items()), vs, pvalue=1e-6)
    want = [l for idx, eff in zip(index, results) for l in pv.tsv_rows(vs, idx, eff)]
    assert want == [l for l in open(tmp_path / "out.tsv")][1:] and len(want) >= 4
