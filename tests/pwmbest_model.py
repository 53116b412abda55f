"""Integer / fp64 numpy model of known-motif enrichment and centrality (csrc/pwmbest.hip,
explainn_amd/pwmenrich.py; DESIGN.md section 3 item 21, section 8 "Known-motif enrichment"), written from the
contract in include/explainn_hip.h on top of pwmsites_model (tables, null), enrichment_model and
centrality_model (the two tests).

Best sites: per (motif, record) the largest integer score over live starts and strands -- `best_brute` reads
the key rule off start by start and strand by strand, `best_of_record` is the vectorised form the GPU test
uses.  The bridge: integer scores as float16 patterns that explainn_site_positions can compare.  Width
groups, the enrichment and centrality assemblies and the per-site p-value at the chosen threshold."""
import numpy as np

import centrality_model as cm
import enrichment_model as em
import pwmsites_model as pm

BRIDGE = 0x400
MAX_LEN = 1 << 30


# ------------------------------------------------------------------------------------------- best sites
def _clip(rec):
    return np.minimum(np.asarray(rec, dtype=np.int64), 4)


def best_brute(Sm, w, rec, both=True):
    """(bits, site) of one motif (table Sm (wmax,4), live width w) in one record, every (start, strand) in
    turn: a strictly larger score replaces the held one, so the first met -- the lowest start, '+' before '-'
    -- wins a tie."""
    rec = _clip(rec)
    best, site = -1, -1
    if w >= 1:
        for p in range(len(rec) - w + 1):
            win = rec[p:p + w]
            if win.max() >= 4:
                continue
            fwd = sum(int(Sm[j][win[j]]) for j in range(w))
            rev = sum(int(Sm[j][3 - win[w - 1 - j]]) for j in range(w))
            for minus, s in ((0, fwd), (1, rev)) if both else ((0, fwd),):
                if s > best:
                    best, site = s, (p << 1) | minus
    return max(best, 0), site


def best_of_record(Sm, w, rec, both=True):
    """The same, vectorised."""
    rec = _clip(rec)
    if w < 1 or len(rec) < w:
        return 0, -1
    win = np.lib.stride_tricks.sliding_window_view(rec, w)
    live = np.flatnonzero(~np.any(win >= 4, axis=1))
    if not len(live):
        return 0, -1
    win = win[live]
    cols = np.arange(w)[None, :]
    f = Sm[cols, win].astype(np.int64).sum(axis=1)
    r = Sm[cols, 3 - win[:, ::-1]].astype(np.int64).sum(axis=1) if both else f
    top = np.maximum(f, r)
    i = int(np.argmax(top == top.max()))
    return int(top[i]), (int(live[i]) << 1) | int(f[i] != top[i])


def record_ok(a, b, seq_len):
    return 0 <= a <= b <= seq_len and b - a < MAX_LEN


def record_best(S, lwidths, codes, offsets, both=True, seq_len=None, best=best_of_record):
    """(bits uint16 (M,R), site int32 (M,R), flag) as explainn_pwm_record_best writes them.  A record whose
    offsets descend or leave [0, seq_len], or of 2^30 bases or more, has no live start and sets the flag; a
    width outside [1, wmax] makes the motif empty."""
    M, wmax = S.shape[0], S.shape[1]
    seq_len = len(codes) if seq_len is None else seq_len
    R = len(offsets) - 1
    bits, site, flag = np.zeros((M, R), np.uint16), np.full((M, R), -1, np.int32), 0
    for r in range(R):
        a, b = int(offsets[r]), int(offsets[r + 1])
        if not record_ok(a, b, seq_len):
            flag = 1
            continue
        for m in range(M):
            w = int(lwidths[m])
            bits[m, r], site[m, r] = best(S[m], w if 1 <= w <= wmax else 0, codes[a:b], both)
    return bits, site, flag


def record_best_equal(S, lwidths, rows, both=True):
    """(bits, site) of R records of one length, rows (R, L): record_best vectorised over the records (for
    the cases with tens of thousands of records; test_pwmbest_model.py holds it to record_best)."""
    rows = _clip(rows)
    R, L = rows.shape
    M, wmax = S.shape[0], S.shape[1]
    bits, site = np.zeros((M, R), np.uint16), np.full((M, R), -1, np.int32)
    for m in range(M):
        w = int(lwidths[m])
        if not 1 <= w <= wmax or L < w:
            continue
        win = np.lib.stride_tricks.sliding_window_view(rows, w, axis=1)            # (R, P, w)
        live = ~np.any(win >= 4, axis=2)
        idx = np.minimum(win, 3)
        cols = np.arange(w)[None, None, :]
        f = S[m][cols, idx].astype(np.int64).sum(axis=2)
        r = S[m][cols, 3 - idx[:, :, ::-1]].astype(np.int64).sum(axis=2) if both else f
        top = np.where(live, np.maximum(f, r), -1)
        best = top.max(axis=1)
        p = np.argmax(top == best[:, None], axis=1)
        minus = f[np.arange(R), p] != best
        bits[m] = np.maximum(best, 0)
        site[m] = np.where(best < 0, -1, (p << 1) | minus)
    return bits, site


def of_records(S, lwidths, records, both=True):
    """record_best of a list of code arrays: (iscore int16, start int32, strand int8), each (M,N), as MotifBest
    holds them."""
    off = np.zeros(len(records) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in records], out=off[1:])
    flat = np.concatenate(list(records) + [np.zeros(0, np.uint8)]).astype(np.uint8)
    bits, site, _ = record_best(S, lwidths, flat, off, both)
    none = site < 0
    return (bits.astype(np.int16), np.where(none, -1, site >> 1).astype(np.int32),
            np.where(none, 0, 1 - 2 * (site & 1)).astype(np.int8), site)


# ------------------------------------------------------------------------------------------- the bridge
def bridge_pattern(iscore):
    """The pattern handed to explainn_site_positions for an integer score."""
    return (np.asarray(iscore, dtype=np.int64) + BRIDGE).astype(np.uint16)


def bridge_threshold(t):
    """The float32 threshold for the integer threshold t: the value of the half with bits 0x400 + t - 1."""
    return (np.asarray(t, dtype=np.int64) + (BRIDGE - 1)).astype(np.uint16).view(np.float16).astype(np.float32)


# ------------------------------------------------------------------------------------------- assemblies
def tables(mats, bg=None, pc=0.1, bins=100):
    bg = pm.uniform() if bg is None else np.asarray(bg, dtype=np.float64)
    S, widths, scale, lo = pm.quantise(mats, bg, pc, bins)
    return dict(S=S, widths=widths, scale=scale, lo=lo, live=pm.live_widths(widths, scale), bg=bg, bins=bins)


def labels_of(primary, control, widest):
    lab = np.concatenate([np.ones(len(primary), np.uint8), np.zeros(len(control), np.uint8)])
    lab[np.array([len(c) for c in list(primary) + list(control)], dtype=np.int64) < widest] = 2
    return lab


def log_odds(tab, iscore):
    ok = tab["scale"] > 0
    return np.where(ok, np.asarray(iscore, dtype=np.float64) / np.where(ok, tab["scale"], 1.0) + tab["widths"] * tab["lo"],
                    np.nan)


def enrichment(mats, primary, control, bg=None, pc=0.1, bins=100, both=True):
    """What motif_enrichment returns with a control set: enrichment_model.test_stats of the stacked integer
    scores (with `gap`), plus labels, excluded, threshold (log-odds), threshold_pvalue (the model's own tail at
    best_pattern) and the tail table."""
    tab = tables(mats, bg, pc, bins)
    bits = of_records(tab["S"], tab["live"], list(primary) + list(control), both)[0]
    labels = labels_of(primary, control, int(tab["live"].max()))
    out = em.test_stats(bits.view(np.uint16), labels)
    tail, _ = pm.null_table(tab["S"], tab["live"], bins, tab["bg"], 1.0)
    out.update(labels=labels, excluded=int(np.sum(labels == 2)), threshold=log_odds(tab, out["best_pattern"]),
               threshold_pvalue=tail[np.arange(len(mats)), out["best_pattern"]], tail=tail, bits=bits, tab=tab)
    return out


def width_groups(lwidths):
    lw = np.asarray(lwidths)
    return [(int(w), np.flatnonzero(lw == w)) for w in sorted(set(lw[lw > 0].tolist()))]


def centrality(mats, primary, control, pvalues, bg=None, pc=0.1, bins=100, both=True, **kwargs):
    """What motif_centrality returns: per width group centrality_model.positions on the bridged patterns and
    thresholds and centrality_model.test_stats, scattered to motif order (empty motifs keep the "no threshold
    tried" zeros; gap inf).  Also iscore_thresholds (M,T), labels, length."""
    tab = tables(mats, bg, pc, bins)
    recs = list(primary) + list(control)
    widest = int(tab["live"].max())
    L = sorted({len(c) for c in recs if len(c) >= widest})
    assert len(L) == 1
    L = L[0]
    bits, _, _, site = of_records(tab["S"], tab["live"], recs, both)
    labels = labels_of(primary, control, widest)
    thr = np.stack([pm.null_table(tab["S"], tab["live"], bins, tab["bg"], p)[1] for p in pvalues], axis=1)
    M = len(mats)
    out = {f: np.zeros(M, dtype=np.float64 if f in cm.LOG_FIELDS else np.int64) for f in cm.FIELDS}
    out["gap"] = np.full(M, np.inf)
    for w, idx in width_groups(tab["live"]):
        hist, counts = cm.positions(bridge_pattern(bits[idx]), site[idx], labels, bridge_threshold(thr[idx]), L - w + 1)
        st = cm.test_stats(hist, counts, **kwargs)
        for f in cm.FIELDS + ("gap",):
            out[f][idx] = st[f]
    out.update(iscore_thresholds=thr.astype(np.int32), labels=labels, length=L, tab=tab,
               counts=np.array([np.sum(labels == 1), np.sum(labels == 0)], dtype=np.int64))
    return out


# ------------------------------------------------------------------------------------------- inputs
PLANTED_WIDTHS = (6, 8, 10, 12, 12, 15, 19, 12)


def planted_case(seed=5, n_primary=120, n_control=240, length=100, motif=3):
    """8 Dirichlet(0.3) motifs; 120 primary records of 100 bases with motif 3's consensus planted within +-4 of
    the centre (start 44 of 0..88) in 7 of every 10 records, alternating strands; 240 random control records.
    Returns (mats, primary, control)."""
    mats = pm.dirichlet_motifs(PLANTED_WIDTHS, seed=seed)
    g = np.random.default_rng(seed + 1)
    primary = [g.integers(0, 4, size=length).astype(np.uint8) for _ in range(n_primary)]
    control = [g.integers(0, 4, size=length).astype(np.uint8) for _ in range(n_control)]
    centre = (length - len(mats[motif])) // 2
    for i, rec in enumerate(primary):
        if i % 10 < 7:
            pm.plant(rec, mats[motif], centre + int(g.integers(-4, 5)), reverse=bool(i % 2))
    return mats, primary, control


def named(mats):
    return [("MA%04d.1" % i, "name%d" % i, m) for i, m in enumerate(mats)]
