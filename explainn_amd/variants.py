"""What does this variant do?  Reference and alternative allele of SNVs and short indels, scored on
the device.

The reference has no such entry point: its users build both haplotype windows of every variant on the
host, transfer a (2V, L) matrix for 1-byte edits and call predict.py; in-silico mutagenesis computes
all 3L substitutions of a window where one is asked for, and cannot express an indel.  Here the
sequence goes to the device once as base codes (1 byte per base); a row table (window start, edit
index) and an edit table (pos, ref_len, alt_len, alt bases) follow, 12 bytes per row and 20 per
variant, and the windows are cut and edited there (explainn_score_edits, include/explainn_hip.h).

    res = score_variants(model, codes, pos, ref_len, alts, shifts=range(7), unit_effects=True)
    res["delta"]     # (V, T): alt - ref, strands and window placements averaged
    res["units"]     # (V, units, T): the units (motifs) that carry it; sums to delta over units

MaxPool1d(7,7) puts its grid at the window start, so a variant's effect depends on its phase mod 7
inside the window: `shifts` slides the window (both alleles alike) and the scores are averaged.

A window that carries several variants at once -- two variants 50 bases apart, a person's phased
genotype over a region -- goes through score_haplotypes(): the same per-variant edit table, and per
haplotype a list of the variants it carries (explainn_score_haplotypes).

    res = score_haplotypes(model, codes, pos, ref_len, alts, haplotypes=[[0, 3, 4], [3]], starts=[1000, 1200])
    res["hap"]       # (H, R, T, 4): haplotype h in the window at starts[r]
    res["delta"]     # (H, R, T): haplotype - reference

`python -m explainn_amd.variants MODEL FASTA VCF` writes one TSV row per variant and class; with
`--haplotypes --regions BED` one row per region, sample, haplotype and class from the VCF's genotypes.
"""
import argparse
import sys
from collections import namedtuple

import numpy as np
import torch

from .architectures import EditedWindows, HaplotypeWindows
from .strands import TwoStrands, as_codes_1d, check_strands, stack_strands

_CHUNK_PASSES = 32           # rows per device call, at most: this many sub-batches of `batch_size` rows
_MAX_POOL = (1 << 31) - 1    # bytes the alt pool may hold (explainn_edits.alt_bytes < 2^31)

Variant = namedtuple("Variant", "chrom pos id ref alt")      # pos 0-based; ref / alt as written in the file


def window_start(pos, ref_len, alt_len, L, shift=0):
    """Start of the window both alleles of a variant are scored in: the longer allele is centred
    (then slid by `shift`).  The start is left of `pos` or at it, so it means the same base on both
    haplotypes: the left flank is identical, and after an indel the right flank slides."""
    return pos - (L - np.maximum(ref_len, alt_len)) // 2 + shift


def build_tables(pos, ref_len, alts, L, shifts=(0,)):
    """The tables of explainn_score_edits for V variants and S shifts, as numpy arrays:
    row_start int64 / row_edit int32 of 2*V*S rows -- row (v*S + s)*2 is the reference window of variant
    v at shift s (row_edit -1), the next row its alternative allele (row_edit v) -- and one edit per
    variant: pos int64, ref_len / alt_len / alt_off int32, alt uint8 (the alt alleles end to end)."""
    pos = np.asarray(pos, dtype=np.int64).reshape(-1)
    ref_len = np.asarray(ref_len, dtype=np.int64).reshape(-1)
    V = len(pos)
    if len(ref_len) != V or len(alts) != V:
        raise ValueError("pos, ref_len and alts must have one entry per variant")
    shifts = np.asarray(list(shifts), dtype=np.int64)
    if shifts.size == 0:
        raise ValueError("shifts must hold at least one window placement")
    alts = [np.asarray(a, dtype=np.uint8).reshape(-1) for a in alts]
    alt_len = np.fromiter((len(a) for a in alts), dtype=np.int64, count=V)
    if (ref_len < 0).any():
        raise ValueError("ref_len must not be negative")
    alt = np.concatenate(alts) if V else np.zeros(0, dtype=np.uint8)
    if alt.size > _MAX_POOL or (V and max(int(ref_len.max()), int(alt_len.max())) > _MAX_POOL):
        raise ValueError("alleles of %d bytes exceed the alt pool's limit of 2^31 - 1" % alt.size)
    alt_off = np.cumsum(alt_len) - alt_len
    start = window_start(pos, ref_len, alt_len, L)[:, None] + shifts[None, :]          # (V,S)
    row_start = np.repeat(start.reshape(-1), 2)
    row_edit = np.stack((np.full((V, len(shifts)), -1, dtype=np.int64),
                         np.broadcast_to(np.arange(V, dtype=np.int64)[:, None], (V, len(shifts)))), axis=-1)
    return {"row_start": row_start, "row_edit": row_edit.reshape(-1).astype(np.int32), "pos": pos,
            "ref_len": ref_len.astype(np.int32), "alt_len": alt_len.astype(np.int32),
            "alt_off": alt_off.astype(np.int32), "alt": alt.astype(np.uint8)}


def chunks(n_variants, n_shifts, limit_rows):
    """[(first variant, count), ...]: the variants in runs whose 2*n_shifts*count rows stay within
    limit_rows (one variant where even that does not fit).  A variant's rows never straddle a run, so a
    run's shifts are averaged on the device; the rows of the runs are exactly the rows of the whole."""
    per = max(1, int(limit_rows) // (2 * n_shifts))
    return [(v0, min(per, n_variants - v0)) for v0 in range(0, n_variants, per)]


def _check_ref_alleles(codes_d, pos, ref_len, check_ref):
    """VCF REF alleles against codes[pos : pos + ref_len], compared on the device."""
    V = len(pos)
    if len(check_ref) != V:
        raise ValueError("check_ref must have one allele per variant")
    refs = [np.asarray(r, dtype=np.uint8).reshape(-1) for r in check_ref]
    lens = np.fromiter((len(r) for r in refs), dtype=np.int64, count=V)
    wrong = np.flatnonzero(lens != ref_len)
    if wrong.size == 0 and lens.sum() > 0:
        owner = np.repeat(np.arange(V, dtype=np.int64), lens)
        within = np.arange(lens.sum(), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
        dev = codes_d.device
        at = torch.from_numpy(pos[owner] + within).to(dev)
        differ = codes_d[at] != torch.from_numpy(np.concatenate(refs)).to(dev)
        wrong = np.unique(owner[differ.cpu().numpy()])
    if wrong.size:
        raise ValueError("%d variant(s) whose REF allele is not what the sequence holds at pos; the first: %s"
                         % (wrong.size, ", ".join("#%d at %d" % (v, pos[v]) for v in wrong[:5])))


def _final_rows(model):
    """final.weight as (T, units) with global unit indices: a bank's (G,T,U) member by member."""
    w = model.final.weight.detach()
    return w if w.dim() == 2 else w.permute(1, 0, 2).reshape(w.shape[1], -1)


def _begin(model, codes, strands, batch_size):
    """What both scorers open with: (codes as a 1-D tensor, L, batch_size, the shape of a row of logits,
    units)."""
    check_strands(strands)
    batch_size = max(1, int(batch_size))
    data = as_codes_1d(codes)
    shape = tuple(model._logits_empty(0, torch.device("cpu")).shape[1:])
    return data, model._options["sequence_length"], batch_size, shape, model._units()


def _check_inside(tab, length):
    """Every variant of the edit table lies inside the sequence of `length` bases."""
    if len(tab["pos"]) and (tab["pos"].min() < 0 or (tab["pos"] + tab["ref_len"]).max() > length):
        bad = np.flatnonzero((tab["pos"] < 0) | (tab["pos"] + tab["ref_len"] > length))
        raise ValueError("%d variant(s) outside the sequence of %d bases (0 <= pos, pos + ref_len <= length); "
                         "the first: #%d at %d" % (bad.size, length, bad[0], tab["pos"][bad[0]]))


def _score_spans(model, data, tab, names, spans, rows_of, launch, both, check_ref, unit_effects):
    """The sequence and the tables `names` of tab go to the device once (check_ref is settled there); then
    the rows [r0, r1) of every span are scored, on both strands at once (strands.TwoStrands):
    rows_of(seq_d, tables, r0, r1, reverse_complement) makes the span's rows, the model's method `launch`
    scores them.  Yields (r0, r1, fwd, rev, ofwd, orev) per span: logits and, with unit_effects, unit
    outputs of the two strands, on the device; rev and the outputs are None where not asked for.  Input
    validation is settled behind the last span."""
    if not spans:
        return
    device = model.final.weight.device
    ts = TwoStrands(model, both)
    seq_d = data.to(device).contiguous()
    if check_ref is not None:
        _check_ref_alleles(seq_d, tab["pos"], tab["ref_len"].astype(np.int64), check_ref)
    dt = {k: torch.from_numpy(tab[k]).to(device) for k in names}
    with ts:
        for r0, r1 in spans:
            fwd, rev = ts.run(lambda m, rc: getattr(m, launch)(rows_of(seq_d, dt, r0, r1, rc), unit_effects))
            ofwd = orev = None
            if unit_effects:
                (fwd, ofwd), (rev, orev) = fwd, (rev if both else (None, None))
            yield r0, r1, fwd, rev, ofwd, orev


def _strand_mean(fwd, rev):
    return fwd if rev is None else (fwd + rev) / 2


def _unit_effects(d, wrows):
    """(rows, units) differences of unit outputs -> (rows, units, T) on the host: each times its unit's
    final.weight row."""
    return (d[:, :, None] * wrows.t()[None, :, :]).cpu().numpy()


def _columns(fwd, rev):
    """Logits of the two strands -> predict()'s columns (rows, ..., 4) on the host; NaN in columns 1..3
    for the forward strand alone."""
    if rev is not None:
        return stack_strands(fwd, rev).cpu().numpy()
    out = np.full(tuple(fwd.shape) + (4,), np.nan)
    out[..., 0] = fwd.cpu().numpy()
    return out


def _sigmoid(scores):
    return torch.sigmoid(torch.from_numpy(scores)).numpy()


def score_variants(model, codes, pos, ref_len, alts, shifts=(0,), strands="both", batch_size=4096,
                   check_ref=None, unit_effects=False, apply_sigmoid=False, chunk_rows=None):
    """Eval-mode predictions of the reference and the alternative allele of V variants of one sequence.

    codes: 1-D uint8 base codes (0..3 = A,C,G,T, 4 = N), numpy array or tensor, host or device; it goes
    to the device once, whole.  Variant v replaces codes[pos[v] : pos[v] + ref_len[v]] (0-based) by
    alts[v], a uint8 code array: SNV, MNV, insertion (ref_len 0), deletion (empty alt) or any ref -> alt
    replacement.  Both alleles are scored in the window window_start() places, once per shift of
    `shifts`; positions outside the sequence read as N.  Returns a dict:
      ref, alt  (V, S, T, 4) float64 in predict()'s order [Fwd, Rev, Mean, Max] -- (V, S, G, T, 4) for an
                ExplaiNNBank -- each row what predict() gives on the materialised window;
      delta     (V, T) / (V, G, T): the mean over shifts of alt[..., 2] - ref[..., 2] (column 0 with
                strands="fwd", which leaves columns 1..3 NaN);
      units     with unit_effects: (V, units, T) float32, (outs_alt - outs_ref)[v,u] * final.weight[t,u]
                averaged over strands and shifts (before any sigmoid).  The bias cancels, so
                units.sum(1) is delta to fp32 rounding; on a bank units are global indices (member g
                owns [g*U, (g+1)*U)) weighted by their own member's rows, and member g's delta is the
                sum over its units.
    check_ref: the VCF REF alleles as code arrays; a mismatch with the sequence raises ValueError.
    The two strands run on the model and its eval_replica() on two streams, as in scan(); the rows go
    to the device in chunks of at most 32 * batch_size rows (chunk_rows overrides it)."""
    data, L, batch_size, shape, units = _begin(model, codes, strands, batch_size)
    shifts = tuple(int(s) for s in shifts)
    tab = build_tables(pos, ref_len, alts, L, shifts)
    V, S = len(tab["pos"]), len(shifts)
    _check_inside(tab, data.shape[0])
    res = {"ref": np.full((V, S) + shape + (4,), np.nan), "alt": np.full((V, S) + shape + (4,), np.nan),
           "delta": np.zeros((V,) + shape)}
    if unit_effects:
        res["units"] = np.zeros((V, units, shape[-1]), dtype=np.float32)
    if V == 0:
        return res
    both = strands == "both"
    wrows = _final_rows(model) if unit_effects else None
    limit = int(chunk_rows) if chunk_rows is not None else _CHUNK_PASSES * batch_size
    spans = [(2 * S * v0, 2 * S * (v0 + cnt)) for v0, cnt in chunks(V, S, limit)]

    def rows_of(seq_d, dt, r0, r1, rc):
        return EditedWindows(seq_d, dt["row_start"][r0:r1], dt["row_edit"][r0:r1], dt["pos"], dt["ref_len"],
                             dt["alt_len"], dt["alt_off"], dt["alt"], rc, batch_size)

    for r0, r1, fwd, rev, ofwd, orev in _score_spans(model, data, tab, tuple(tab), spans, rows_of,
                                                     "_launch_score_edits", both, check_ref, unit_effects):
        v0, v1 = r0 // (2 * S), r1 // (2 * S)
        if unit_effects:
            # (rows / 2, units): alt - ref
            d = _strand_mean(ofwd[1::2] - ofwd[0::2], orev[1::2] - orev[0::2] if both else None)
            res["units"][v0:v1] = _unit_effects(d.reshape(v1 - v0, S, units).mean(dim=1), wrows)
        full = _columns(fwd, rev).reshape((v1 - v0, S, 2) + shape + (4,))
        res["ref"][v0:v1], res["alt"][v0:v1] = full[:, :, 0], full[:, :, 1]
    if apply_sigmoid:
        res["ref"], res["alt"] = _sigmoid(res["ref"]), _sigmoid(res["alt"])
    col = 2 if both else 0
    res["delta"] = (res["alt"][..., col] - res["ref"][..., col]).mean(axis=1)
    return res


def build_haplotype_tables(pos, ref_len, alts, haplotypes, starts, L):
    """The tables of explainn_score_haplotypes for H haplotypes in R windows, as numpy arrays.

    pos / ref_len / alts: the V variants, as build_tables takes them; they become the edit table (pos
    int64, ref_len / alt_len / alt_off int32, alt uint8), one record per variant.  haplotypes: H integer
    arrays, the variants each haplotype carries, in any order; each is sorted by position (stable, so
    two insertions at one position keep their order) and two carried variants that overlap raise
    ValueError.  starts: the R window left edges, in reference coordinates.

    Row h*R + r is haplotype h in the window at starts[r]: row_start = starts[r], and its run (row_first
    int64, row_count int32, into edit_index int32, the sorted lists end to end) holds the haplotype's
    variants from the first with pos >= starts[r] while they begin inside the window,
    hstart < starts[r] + L -- later ones cannot reach it, earlier ones lie left of it.  A carried variant
    with pos < starts[r] < pos + ref_len straddles the left edge: the window would begin inside its alt
    allele, at no reference coordinate; it is left out and counted in straddling (H, R)."""
    tab = build_tables(pos, ref_len, alts, L)
    epos, eref, ealt = tab["pos"], tab["ref_len"].astype(np.int64), tab["alt_len"].astype(np.int64)
    V = len(epos)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    H, R = len(haplotypes), len(starts)
    lists, first, count = [], np.zeros((H, R), dtype=np.int64), np.zeros((H, R), dtype=np.int64)
    straddling = np.zeros((H, R), dtype=np.int64)
    offset = 0
    for h, carried in enumerate(haplotypes):
        idx = np.asarray(carried, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= V):
            raise ValueError("haplotype %d carries a variant outside 0..%d" % (h, V - 1))
        idx = idx[np.argsort(epos[idx], kind="stable")]
        p, end = epos[idx], epos[idx] + eref[idx]
        clash = np.flatnonzero(end[:-1] > p[1:])
        if clash.size:
            a, b = idx[clash[0]], idx[clash[0] + 1]
            raise ValueError("haplotype %d carries overlapping variants #%d at %d (ref_len %d) and #%d at %d"
                             % (h, a, epos[a], eref[a], b, epos[b]))
        # where each variant begins on the haplotype that carries all of them: pos + the shift of those before
        shift = np.concatenate((np.zeros(1, np.int64), np.cumsum(ealt[idx] - eref[idx])))
        hstart = p + shift[:-1]
        f = np.searchsorted(p, starts, side="left")
        # the run's own coordinates start at its first edit: the shift before it does not count
        stop = np.searchsorted(hstart, starts + L + shift[f], side="left")
        first[h], count[h] = offset + f, np.maximum(stop - f, 0)
        if idx.size:
            straddling[h] = (f > 0) & (end[np.maximum(f - 1, 0)] > starts)
        lists.append(idx)
        offset += idx.size
    edit_index = np.concatenate(lists + [np.zeros(0, np.int64)])
    if edit_index.size > _MAX_POOL:
        raise ValueError("haplotype lists of %d entries exceed 2^31 - 1" % edit_index.size)
    out = {"row_start": np.tile(starts, H), "row_first": first.reshape(-1),
           "row_count": count.reshape(-1).astype(np.int32), "edit_index": edit_index.astype(np.int32)}
    out.update({k: tab[k] for k in ("pos", "ref_len", "alt_len", "alt_off", "alt")})
    out["straddling"] = straddling
    return out


_HAP_TABLES = ("row_start", "row_first", "row_count", "edit_index", "pos", "ref_len", "alt_len", "alt_off", "alt")


def score_haplotypes(model, codes, pos, ref_len, alts, haplotypes, starts, strands="both", batch_size=4096,
                     check_ref=None, unit_effects=False, apply_sigmoid=False, chunk_rows=None):
    """Eval-mode predictions of H haplotypes of one sequence in R windows, each haplotype carrying any
    number of the V variants (codes, pos, ref_len, alts, check_ref as score_variants takes them;
    haplotypes and starts as build_haplotype_tables).  Returns a dict:
      hap         (H, R, T, 4) float64 in predict()'s order [Fwd, Rev, Mean, Max] -- (H, R, G, T, 4) for
                  an ExplaiNNBank -- each row what predict() gives on the materialised window;
      ref         (R, T, 4): the reference windows, each scored once;
      delta       (H, R, T): hap[..., 2] - ref[..., 2] (column 0 with strands="fwd", which leaves
                  columns 1..3 NaN);
      straddling  (H, R): the carried variants left out of a row because the window's left edge lies
                  inside their REF allele (build_haplotype_tables);
      units       with unit_effects: (H, R, units, T) float32, (outs_hap - outs_ref)[u] * final.weight[t,u]
                  averaged over strands; sums over units to delta to fp32 rounding (score_variants has
                  the bank layout).
    Strands, streams and chunking are score_variants': the rows go to the device in chunks of at most
    32 * batch_size rows (chunk_rows overrides it), the reference windows first."""
    data, L, batch_size, shape, units = _begin(model, codes, strands, batch_size)
    tab = build_haplotype_tables(pos, ref_len, alts, haplotypes, starts, L)
    H = len(haplotypes)
    R = len(tab["row_start"]) // H if H else len(np.asarray(starts).reshape(-1))
    _check_inside(tab, data.shape[0])
    # the reference windows are rows of their own, without a run, ahead of the haplotypes' rows
    ref_start = np.asarray(starts, dtype=np.int64).reshape(-1)
    tab["row_start"] = np.concatenate((ref_start, tab["row_start"]))
    tab["row_first"] = np.concatenate((np.zeros(R, np.int64), tab["row_first"]))
    tab["row_count"] = np.concatenate((np.zeros(R, np.int32), tab["row_count"]))
    rows = R + H * R
    scores = np.full((rows,) + shape + (4,), np.nan)
    res = {"straddling": tab["straddling"]}
    if unit_effects:
        res["units"] = np.zeros((H * R, units, shape[-1]), dtype=np.float32)
    both = strands == "both"
    wrows = _final_rows(model) if unit_effects else None
    limit = max(1, int(chunk_rows) if chunk_rows is not None else _CHUNK_PASSES * batch_size)
    # the reference rows in chunks of their own, so that a chunk of haplotype rows finds them all
    spans = [(r0, min(r0 + limit, R)) for r0 in range(0, R, limit)]
    spans += [(r0, min(r0 + limit, rows)) for r0 in range(R, rows, limit)]

    def rows_of(seq_d, dt, r0, r1, rc):
        return HaplotypeWindows(seq_d, dt["row_start"][r0:r1], dt["row_first"][r0:r1], dt["row_count"][r0:r1],
                                dt["edit_index"], dt["pos"], dt["ref_len"], dt["alt_len"], dt["alt_off"],
                                dt["alt"], rc, batch_size)

    ref_parts, ref_outs = ([], []), None
    for r0, r1, fwd, rev, ofwd, orev in _score_spans(model, data, tab, _HAP_TABLES, spans, rows_of,
                                                     "_launch_score_haplotypes", both, check_ref, unit_effects):
        if unit_effects and r0 < R:
            ref_parts[0].append(ofwd)
            ref_parts[1].append(orev)
        elif unit_effects:
            if ref_outs is None:
                ref_outs = (torch.cat(ref_parts[0]), torch.cat(ref_parts[1]) if both else None)
            window = torch.arange(r0 - R, r1 - R, device=ofwd.device) % R
            # (rows, units): hap - ref
            d = _strand_mean(ofwd - ref_outs[0][window], orev - ref_outs[1][window] if both else None)
            res["units"][r0 - R:r1 - R] = _unit_effects(d, wrows)
        scores[r0:r1] = _columns(fwd, rev)
    if apply_sigmoid:
        scores = _sigmoid(scores)
    res["ref"] = scores[:R]
    res["hap"] = scores[R:].reshape((H, R) + shape + (4,))
    col = 2 if both else 0
    res["delta"] = res["hap"][..., col] - res["ref"][None, ..., col]
    if unit_effects:
        res["units"] = res["units"].reshape(H, R, units, shape[-1])
    return res


def _is_symbolic(allele):
    return allele in ("", ".", "*") or allele.startswith("<") or "[" in allele or "]" in allele


def read_vcf(path):
    """VCF (plain or gzipped text) -> (variants, skipped): the columns CHROM POS ID REF ALT of every
    record as Variant(chrom, pos, id, ref, alt) with pos 0-based, one per ALT allele of a multi-allelic
    line; `skipped` counts the alleles left out: symbolic alleles (<DEL>, ...), the overlapping-deletion
    star, breakends (any allele with a bracket) and the missing allele '.'."""
    from .loader import _open
    out, skipped = [], 0
    with _open(path, "rt") as fh:
        for line in fh:
            if not line.strip() or line.startswith("#"):
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 5:
                raise ValueError("VCF line with fewer than 5 columns: %r" % line[:80])
            chrom, pos, vid, ref = f[0], int(f[1]) - 1, f[2], f[3]
            for alt in f[4].split(","):
                if _is_symbolic(alt) or _is_symbolic(ref):
                    skipped += 1
                else:
                    out.append(Variant(chrom, pos, vid, ref, alt))
    return out, skipped


def read_vcf_genotypes(path, samples=None):
    """VCF with genotypes -> (variants, sample_names, carried, unphased).  variants: as read_vcf makes
    them, one Variant per usable ALT allele (symbolic alleles have no row).  sample_names: the samples
    read, in file order, or the names given in `samples` (a name the file lacks raises ValueError).
    carried: uint8 (alleles, samples, 2), 1 where haplotype h of sample s carries ALT-allele row a.  A
    phased call a|b is placed as written; an unphased call that is homozygous for one ALT allele goes on
    both haplotypes; an unphased heterozygous call goes on neither and is counted, per sample, in
    unphased (samples,); '.' is the reference allele; a haploid call fills haplotype 0."""
    from .loader import _open
    import re
    out, rows, names, cols = [], [], None, None
    with _open(path, "rt") as fh:
        for line in fh:
            if not line.strip() or line.startswith("##"):
                continue
            f = line.rstrip("\r\n").split("\t")
            if line.startswith("#"):
                have = f[9:]
                names = list(have) if samples is None else list(samples)
                missing = [n for n in names if n not in have]
                if missing:
                    raise ValueError("sample(s) not in the VCF: %s" % ", ".join(missing))
                cols = [9 + have.index(n) for n in names]
                unphased = np.zeros(len(names), dtype=np.int64)
                continue
            if names is None:
                raise ValueError("VCF record before the #CHROM header line")
            if len(f) < 5:
                raise ValueError("VCF line with fewer than 5 columns: %r" % line[:80])
            chrom, pos, vid, ref = f[0], int(f[1]) - 1, f[2], f[3]
            fmt = f[8].split(":") if len(f) > 8 else []
            if names and "GT" not in fmt:
                raise ValueError("VCF record without a GT field: %r" % line[:80])
            calls = []
            for s, c in enumerate(cols):
                if c >= len(f):
                    raise ValueError("VCF line with fewer sample columns than the header: %r" % line[:80])
                text = f[c].split(":")[fmt.index("GT")]
                al = [None if a in (".", "") else int(a) for a in re.split(r"[|/]", text)]
                if len(al) > 2:
                    raise ValueError("genotype %r: more than two haplotypes are not supported" % text)
                phased = len(al) == 1 or "|" in text
                if not phased and al[0] != al[1] and any(a for a in al):
                    unphased[s] += 1
                calls.append((al, phased))
            for k, alt in enumerate(f[4].split(","), start=1):
                if _is_symbolic(alt) or _is_symbolic(ref):
                    continue
                out.append(Variant(chrom, pos, vid, ref, alt))
                row = np.zeros((len(names), 2), dtype=np.uint8)
                for s, (al, phased) in enumerate(calls):
                    if phased:
                        for h, a in enumerate(al):
                            row[s, h] = a == k
                    elif al[0] == al[1] == k:
                        row[s] = 1
                rows.append(row)
    if names is None:
        raise ValueError("VCF without a #CHROM header line")
    carried = np.stack(rows) if rows else np.zeros((0, len(names), 2), dtype=np.uint8)
    return out, names, carried, unphased


def read_bed(path):
    """BED (plain or gzipped text) -> [(chrom, start, end), ...], 0-based half-open as written."""
    from .loader import _open
    out = []
    with _open(path, "rt") as fh:
        for line in fh:
            f = line.split()
            if not f or f[0].startswith("#") or f[0] in ("track", "browser"):
                continue
            if len(f) < 3:
                raise ValueError("BED line with fewer than 3 columns: %r" % line[:80])
            out.append((f[0], int(f[1]), int(f[2])))
    return out


def _haplotypes_main(args, ap):
    """--haplotypes: every sample's two haplotypes in the window centred on each BED region -> TSV
    (Chrom, Start, End, Sample, Hap, Class, RefMean, HapFwd, HapRev, HapMean, Delta), one row per
    region, sample, haplotype (1, 2) and class; regions in file order."""
    if not args.regions:
        ap.error("--haplotypes needs --regions BED")
    from .loader import open_output, read_fasta_records
    from .predict import _load_model
    variants, names, carried, unphased = read_vcf_genotypes(
        args.vcf_file, args.samples.split(",") if args.samples else None)
    regions = read_bed(args.regions)
    records = read_fasta_records(args.fasta_file)
    model = _load_model(args.model_file)
    L = model._options["sequence_length"]
    if unphased.sum():
        sys.stderr.write("%d unphased heterozygous call(s) left on the reference allele\n" % unphased.sum())
    lines = {}
    for rid, codes in records:
        idx = [i for i, v in enumerate(variants) if v.chrom == rid]
        reg = [j for j, r in enumerate(regions) if r[0] == rid]
        if not reg:
            continue
        refs = [allele_codes(variants[i].ref) for i in idx]
        haps = [np.flatnonzero(carried[idx, s, h]) for s in range(len(names)) for h in (0, 1)]
        starts = [(regions[j][1] + regions[j][2]) // 2 - L // 2 for j in reg]
        res = score_haplotypes(model, codes, [variants[i].pos for i in idx], [len(r) for r in refs],
                               [allele_codes(variants[i].alt) for i in idx], haps, starts, strands=args.strands,
                               apply_sigmoid=args.apply_sigmoid, check_ref=None if args.no_check_ref else refs)
        for r, j in enumerate(reg):
            rows = []
            for s, name in enumerate(names):
                for h in (0, 1):
                    hap, ref = res["hap"][2 * s + h, r], res["ref"][r]
                    for t in range(ref.shape[0]):
                        row = [rid, str(regions[j][1]), str(regions[j][2]), name, str(h + 1), str(t)]
                        row += [repr(float(x)) for x in (ref[t, 2], *hap[t, :3], res["delta"][2 * s + h, r, t])]
                        rows.append("\t".join(row) + "\n")
            lines[j] = rows
    if len(lines) < len(regions):
        sys.stderr.write("%d region(s) on sequences the FASTA does not hold\n" % (len(regions) - len(lines)))
    with open_output(args.output_file) as fh:
        fh.write("Chrom\tStart\tEnd\tSample\tHap\tClass\tRefMean\tHapFwd\tHapRev\tHapMean\tDelta\n")
        for j in sorted(lines):
            fh.writelines(lines[j])


def allele_codes(allele):
    """An allele string -> uint8 base codes: ACGT in either case, every other letter (N and the other
    IUPAC codes) -> 4."""
    from .sequence import _LUT
    return _LUT[np.frombuffer(allele.encode("ascii", "replace"), dtype=np.uint8)]


def score_records(model, records, variants, **kwargs):
    """score_variants() per FASTA record: records [(id, codes), ...] (loader.read_fasta_records),
    variants a list of Variant.  Returns (index, results): results[j] is the dict of the variants
    index[j] (positions in `variants`, file order kept) of one record; variants whose chromosome is
    not among the records appear in no index."""
    by = {}
    for i, v in enumerate(variants):
        by.setdefault(v.chrom, []).append(i)
    index, results = [], []
    for rid, codes in records:
        idx = by.get(rid)
        if not idx:
            continue
        refs = [allele_codes(variants[i].ref) for i in idx]
        kw = dict(kwargs)
        if kw.pop("check_ref", True):
            kw["check_ref"] = refs
        results.append(score_variants(model, codes, [variants[i].pos for i in idx], [len(r) for r in refs],
                                      [allele_codes(variants[i].alt) for i in idx], **kw))
        index.append(idx)
    return index, results


def main(argv=None):
    """Variants of a VCF on the sequences of a FASTA -> TSV (Chrom, Pos, Id, Ref, Alt, Class, RefFwd,
    RefRev, RefMean, AltFwd, AltRev, AltMean, Delta), one row per variant and class, window placements
    averaged; Pos is the VCF's (1-based)."""
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.variants", description=main.__doc__)
    ap.add_argument("model_file")
    ap.add_argument("fasta_file")
    ap.add_argument("vcf_file")
    ap.add_argument("-o", "--output-file")
    ap.add_argument("--shifts", type=int, default=7, help="window placements 0..S-1 (default 7: one pooling period)")
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--top-units", type=int, default=0, metavar="K",
                    help="add a column Units: unit:effect of the K largest |effect|")
    ap.add_argument("--apply-sigmoid", action="store_true")
    ap.add_argument("--no-check-ref", action="store_true")
    ap.add_argument("--haplotypes", action="store_true",
                    help="score the samples' phased haplotypes (GT) in the windows centred on --regions")
    ap.add_argument("--regions", metavar="BED")
    ap.add_argument("--samples", metavar="A,B", help="with --haplotypes: these samples only")
    args = ap.parse_args(argv)
    if args.haplotypes:
        return _haplotypes_main(args, ap)
    if args.shifts < 1:
        ap.error("--shifts must be at least 1")
    from .loader import open_output, read_fasta_records
    from .predict import _load_model
    variants, skipped = read_vcf(args.vcf_file)
    records = read_fasta_records(args.fasta_file)
    model = _load_model(args.model_file)
    index, results = score_records(model, records, variants, shifts=tuple(range(args.shifts)),
                                   strands=args.strands, unit_effects=args.top_units > 0,
                                   apply_sigmoid=args.apply_sigmoid, check_ref=not args.no_check_ref)
    where = {i: (res, j) for idx, res in zip(index, results) for j, i in enumerate(idx)}
    if skipped or len(where) < len(variants):
        sys.stderr.write("%d symbolic allele(s) skipped, %d variant(s) on sequences the FASTA does not hold\n"
                         % (skipped, len(variants) - len(where)))
    with open_output(args.output_file) as fh:
        fh.write("Chrom\tPos\tId\tRef\tAlt\tClass\tRefFwd\tRefRev\tRefMean\tAltFwd\tAltRev\tAltMean\tDelta"
                 + ("\tUnits" if args.top_units > 0 else "") + "\n")
        for i, v in enumerate(variants):
            if i not in where:
                continue
            res, j = where[i]
            ref, alt = res["ref"][j].mean(axis=0), res["alt"][j].mean(axis=0)        # (T,4): shifts averaged
            for t in range(ref.shape[0]):
                row = [v.chrom, str(v.pos + 1), v.id, v.ref, v.alt, str(t)]
                row += [repr(float(x)) for x in (*ref[t, :3], *alt[t, :3], res["delta"][j, t])]
                if args.top_units > 0:
                    eff = res["units"][j, :, t]
                    top = np.argsort(-np.abs(eff), kind="stable")[:args.top_units]
                    row.append(",".join("%d:%s" % (u, repr(float(eff[u]))) for u in top))
                fh.write("\t".join(row) + "\n")


if __name__ == "__main__":
    main()
