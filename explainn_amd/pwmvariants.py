"""Which known motif does this variant create or destroy?  The best PWM site of the reference and of the
alternative allele of SNVs and short indels, on the device.

`variants.score_variants` says what a variant does to the model's logits and which of the model's own filters
carry it; `pwmsites.scan_motifs` says where database motifs occur.  This module joins the two without a model:
for every (variant, motif) the best site among the windows the allele touches, on both haplotypes -- what
motifbreakR, atSNP or a FIMO run on both alleles report, and the independent evidence that belongs beside a
filter's share in `score_variants(..., unit_effects=True)["units"]`.

    eff = motif_variants(read_motifs("JASPAR.meme"), codes, pos, ref_len, alts, pvalue=1e-4)
    eff.variant, eff.motif          # the (variant, motif) pairs where either allele reaches the motif's threshold
    eff.effect                      # "loss", "gain" or "both"
    eff.delta                       # alt_score - ref_score, log-odds

The sequence goes to the device once as base codes; the edit table is `variants.build_tables`' (20 bytes per
variant), the score tables and their exact null are `pwmsites.score_null`'s.  Neither haplotype is built: the
kernel (explainn_pwm_variant_best, csrc/pwmvariants.hip) splices the few bases around each allele.  A motif of
width w has w + l - 1 windows at an allele of l bases (the w - 1 windows across the junction of a deletion), so
a p-value here is the exact per-window tail of the best score and is NOT corrected for that number of windows.

`python -m explainn_amd.pwmvariants MOTIFS FASTA VCF -o OUT.tsv` writes one row per (variant, motif) pair.
There is no CPU path.
"""
import argparse
import sys

import numpy as np

from . import motifs as _motifs
from . import pwmsites as _pwm
from . import sites as _sites
from .strands import as_codes_1d, check_strands
from .variants import _check_inside, _check_ref_alleles, allele_codes, build_tables, read_vcf

MAX_ALLELE = 128                 # EXPLAINN_PWM_VARIANT_MAX_ALLELE: bases per allele, after trimming
OUTPUT_BYTES = 256 << 20         # the dense (M, chunk, 2) outputs of one device call; the chunk of variants is sized to it
ALL_BYTES = 1 << 30              # keep="all": the host arrays of V * M pairs may take this much
_PAIR_BYTES = 12                 # per (motif, variant): two alleles of uint16 bits and int32 site
_ROW_BYTES = 96                  # per kept pair on the host, all fields together
EFFECTS = ("loss", "gain", "both", "none")


def trim_alleles(pos, refs, alts):
    """The shared prefix, then the shared suffix, of REF and ALT removed: (pos int64, refs, alts) with pos moved
    right by the prefix.  A VCF's anchor base touches no window of its own: CA -> C at p becomes the deletion of A
    at p + 1."""
    pos = np.array(pos, dtype=np.int64).reshape(-1)
    out_r, out_a = [], []
    for v, (r, a) in enumerate(zip(refs, alts)):
        n = min(len(r), len(a))
        same = np.flatnonzero(r[:n] != a[:n])
        lead = int(same[0]) if same.size else n
        r, a = r[lead:], a[lead:]
        n = min(len(r), len(a))
        same = np.flatnonzero(r[::-1][:n] != a[::-1][:n])
        tail = int(same[0]) if same.size else n
        pos[v] += lead
        out_r.append(r[:len(r) - tail])
        out_a.append(a[:len(a) - tail])
    return pos, out_r, out_a


class MotifVariantEffects:
    """The (variant, motif) pairs of motif_variants, ordered by variant, then motif; one entry per pair:

      variant, motif          int64: indices into the call's variants and motifs
      ref_iscore, alt_iscore  int32: the best integer score among the windows the allele touches, -1 without a
                              live window
      ref_score, alt_score    float64: the log-odds iscore / scale + w lo (PwmCalls.score's formula), NaN without
      delta                   alt_score - ref_score
      ref_pvalue, alt_pvalue  float64: the exact null tail of the best score of ONE window (PwmNull.tail[m][iscore]),
                              1.0 without a site; NOT corrected for the w + l - 1 windows the maximum is taken over
      ref_offset, alt_offset  int32: start - pos of the best window on its own haplotype (pos: the trimmed one), 0
                              without a site
      ref_strand, alt_strand  int8: +1 / -1, 0 without a site
      effect                  int8 index into EFFECTS: loss (ref >= thr > alt), gain (alt >= thr > ref), both, and --
                              only with keep="all" -- none; `effect_names` gives the strings

    and per call: names, titles, widths (M,), thresholds int32 (M,), the trimmed pos int64 / ref_len / alt_len
    int32 (V,), and flags (bit 0: a byte above 4 near an allele was read as N)."""

    FIELDS = ("variant", "motif", "ref_iscore", "alt_iscore", "ref_score", "alt_score", "delta", "ref_pvalue",
              "alt_pvalue", "ref_offset", "alt_offset", "ref_strand", "alt_strand", "effect")

    def __init__(self, fields, names, titles, widths, thresholds, pos, ref_len, alt_len, flags):
        for k in self.FIELDS:
            setattr(self, k, fields[k])
        self.names, self.titles = list(names), list(titles)
        self.widths, self.thresholds = np.asarray(widths, dtype=np.int32), np.asarray(thresholds, dtype=np.int32)
        self.pos, self.ref_len, self.alt_len, self.flags = pos, ref_len, alt_len, int(flags)

    def __len__(self):
        return len(self.variant)

    @property
    def effect_names(self):
        return np.array(EFFECTS)[self.effect]


def variant_best_device(scores, widths, seq, tab, both=True, want_site=True, flags=None):
    """explainn_pwm_variant_best on device tensors: scores int16 (M,wmax,4), widths int32 (M,), seq uint8 (n,) and
    tab, a dict of the edit table (pos int64, ref_len / alt_len / alt_off int32 (V,), alt uint8).  Returns (bits
    int16 (M,V,2), site int32 (M,V,2) or None) on the device; `flags`: an int32 (1,) device tensor the call ORs
    into.  Enqueued on the current stream."""
    import torch

    from . import _lib
    dev = _lib.require(seq, torch.uint8, (None,), None, "seq").device
    _lib.require(scores, torch.int16, (None, None, 4), dev, "scores")
    M, wmax = scores.shape[0], scores.shape[1]
    _lib.require(widths, torch.int32, (M,), dev, "widths")
    V = _lib.require(tab["pos"], torch.int64, (None,), dev, "pos").shape[0]
    for k in ("ref_len", "alt_len", "alt_off"):
        _lib.require(tab[k], torch.int32, (V,), dev, k)
    alt = _lib.require(tab["alt"], torch.uint8, (None,), dev, "alt")
    bits = torch.empty((M, V, 2), dtype=torch.int16, device=dev)
    site = torch.empty((M, V, 2), dtype=torch.int32, device=dev) if want_site else None
    _lib.call("explainn_pwm_variant_best", dev, seq if seq.shape[0] else None, seq.shape[0], tab["pos"], tab["ref_len"],
              tab["alt_len"], tab["alt_off"], alt if alt.shape[0] else None, alt.shape[0], V, int(bool(both)), scores,
              widths, M, max(wmax, 1), bits, site, flags)
    return bits, site


def _ref_alleles(data, pos, ref_len):
    """codes[pos : pos + ref_len] of every variant as host arrays (one gather where the codes are on a device)."""
    lens = ref_len.astype(np.int64)
    if data.device.type == "cpu":
        host = data.numpy()
        return [host[p:p + n] for p, n in zip(pos, lens)]
    import torch
    within = np.arange(lens.sum(), dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    flat = data[torch.from_numpy(np.repeat(pos, lens) + within).to(data.device)].cpu().numpy()
    return np.split(flat, np.cumsum(lens)[:-1]) if len(lens) else []


def _prepare(codes, pos, ref_len, alts, trim, check_ref):
    """The checked, trimmed edit table of a call (host numpy, build_tables' fields) and the codes as a tensor."""
    data = as_codes_1d(codes)
    tab = build_tables(pos, ref_len, alts, 0)
    _check_inside(tab, data.shape[0])
    if check_ref is not None:
        _check_ref_alleles(data, tab["pos"], tab["ref_len"].astype(np.int64), check_ref)
    if trim and len(tab["pos"]):
        alt_list = np.split(tab["alt"], np.cumsum(tab["alt_len"].astype(np.int64))[:-1])
        tpos, refs, alt_list = trim_alleles(tab["pos"], _ref_alleles(data, tab["pos"], tab["ref_len"]), alt_list)
        tab = build_tables(tpos, [len(r) for r in refs], alt_list, 0)
    longest = max(int(tab["ref_len"].max()), int(tab["alt_len"].max())) if len(tab["pos"]) else 0
    if longest > MAX_ALLELE:
        bad = np.flatnonzero(np.maximum(tab["ref_len"], tab["alt_len"]) > MAX_ALLELE)
        raise ValueError("%d variant(s) with an allele longer than %d bases%s; the first: #%d at %d" % (
            bad.size, MAX_ALLELE, " after trimming" if trim else "", bad[0], tab["pos"][bad[0]]))
    return data, tab


def _check_args(pvalue, bg, strands, keep, chunk_variants):
    check_strands(strands)
    _sites.check_pvalue(pvalue)
    if isinstance(bg, str):
        raise ValueError("bg=%r: motif_variants scores every variant against one table; give four frequencies "
                         "(per-record backgrounds are not supported)" % (bg,))
    if keep not in ("hits", "all"):
        raise ValueError("keep must be 'hits' or 'all' (got %r)" % (keep,))
    if chunk_variants is not None and int(chunk_variants) < 1:
        raise ValueError("chunk_variants must be at least 1 (got %r)" % (chunk_variants,))


_EMPTY = {"variant": np.int64, "motif": np.int64, "ref_iscore": np.int32, "alt_iscore": np.int32,
          "ref_score": np.float64, "alt_score": np.float64, "delta": np.float64, "ref_pvalue": np.float64,
          "alt_pvalue": np.float64, "ref_offset": np.int32, "alt_offset": np.int32, "ref_strand": np.int8,
          "alt_strand": np.int8, "effect": np.int8}


def _select(null, bits, site, v0, keep_all):
    """The kept pairs of one chunk, chosen and gathered on the device: a dict of host arrays, variant-major."""
    import torch
    M, stride = null.tail.shape
    isc = torch.where(site >= 0, bits.to(torch.int32), torch.full_like(site, -1)).permute(1, 0, 2)      # (c, M, 2)
    thr = null.thresholds[None, :]
    hit_r, hit_a = isc[:, :, 0] >= thr, isc[:, :, 1] >= thr
    v, m = torch.nonzero(torch.ones_like(hit_r) if keep_all else hit_r | hit_a, as_tuple=True)
    s = site.permute(1, 0, 2)[v, m]                                                                # (n, 2)
    i = isc[v, m]
    none = i < 0
    pv = null.tail.view(-1)[m[:, None] * stride + i.clamp(min=0).to(torch.int64)]
    pv = torch.where(none, torch.ones_like(pv), pv)
    w = null.widths[m][:, None]
    r, a = hit_r[v, m], hit_a[v, m]
    effect = torch.where(r & ~a, 0, torch.where(a & ~r, 1, torch.where(r, 2, 3))).to(torch.int8)
    offset = torch.where(none, torch.zeros_like(s), (s >> 1) - w + 1)
    strand = torch.where(none, torch.zeros_like(s), 1 - 2 * (s & 1)).to(torch.int8)
    out = {"variant": v + v0, "motif": m, "ref_iscore": i[:, 0], "alt_iscore": i[:, 1], "ref_pvalue": pv[:, 0],
           "alt_pvalue": pv[:, 1], "ref_offset": offset[:, 0], "alt_offset": offset[:, 1], "ref_strand": strand[:, 0],
           "alt_strand": strand[:, 1], "effect": effect}
    return {k: t.cpu().numpy() for k, t in out.items()}


def motif_variants(motifs, codes, pos, ref_len, alts, pvalue=1e-4, bg=None, pseudocount=0.1, bins=100,
                   strands="both", trim=True, keep="hits", check_ref=None, chunk_variants=None):
    """The effect of V variants of one sequence on the sites of known motifs: a MotifVariantEffects.

    motifs, bg (None = uniform, or four frequencies; "sequence" is refused), pseudocount and bins: as scan_motifs
    takes them; a motif's integer threshold thr is the smallest score whose exact null tail is <= pvalue
    (pwmsites.score_null).  codes, pos, ref_len, alts and check_ref: as score_variants takes them.  trim removes
    the shared prefix, then the shared suffix, of REF and ALT on the host (trim_alleles) -- the anchor base of a
    VCF indel touches no window of its own -- and the trimmed pos / ref_len / alt_len are returned; an allele
    longer than MAX_ALLELE bases after trimming raises ValueError.

    For allele A of l bases (ref: l = ref_len, alt: l = alt_len) and a motif of width w, the windows the allele
    touches are the starts pos - w + 1 + i, i = 0 .. w + l - 2, of the haplotype codes[:pos] + allele +
    codes[pos + ref_len:] -- with l = 0 the w - 1 windows across the junction.  The best score over the live ones
    (inside the haplotype, no N) and the requested strands is the allele's; ties go to the leftmost window, then
    '+'.  keep="hits" keeps the (variant, motif) pairs where either allele reaches thr; keep="all" keeps every
    pair (refused above ALL_BYTES of host arrays).  The p-values are per window: exact for the best score of one
    window and NOT corrected for the number of windows the maximum was taken over.

    The variants go to the device in chunks sized so that the dense (M, chunk, 2) outputs stay under OUTPUT_BYTES
    (or chunk_variants variants); per chunk the kept pairs are selected on the device.  The result does not depend
    on the chunking."""
    import torch

    from . import _lib
    _check_args(pvalue, bg, strands, keep, chunk_variants)
    ids, mats = _pwm.motif_list(motifs)
    named = isinstance(motifs, (list, tuple)) and all(isinstance(m, tuple) and len(m) == 3 for m in motifs)
    titles = [str(m[1]) for m in motifs] if named else list(ids)
    _pwm._check_table_args(pseudocount, bins)
    data, tab = _prepare(codes, pos, ref_len, alts, trim, check_ref)
    M, V = len(mats), len(tab["pos"])
    if keep == "all" and M * V * _ROW_BYTES > ALL_BYTES:
        raise ValueError("keep='all' would hold %d (variant, motif) pairs, over %d bytes on the host; use keep='hits' "
                         "or fewer variants per call" % (M * V, ALL_BYTES))
    device = _lib.device_for(None, (data,), "pwmvariants.motif_variants")
    widths = np.array([len(m) for m in mats], dtype=np.int32).reshape(M)
    if M == 0:
        fields = {k: np.zeros(0, dt) for k, dt in _EMPTY.items()}
        return MotifVariantEffects(fields, ids, titles, widths, np.zeros(0, np.int32), tab["pos"], tab["ref_len"],
                                   tab["alt_len"], 0)
    null = _pwm.score_null([(i, i, m) for i, m in zip(ids, mats)], pvalue, bg, pseudocount, bins, device)
    parts, flags = [], 0
    if V:
        chunk = int(chunk_variants) if chunk_variants is not None else max(1, OUTPUT_BYTES // (_PAIR_BYTES * M))
        seq_d = data.to(device).contiguous()
        alt_d = torch.from_numpy(tab["alt"]).to(device)
        flag_d = torch.zeros(1, dtype=torch.int32, device=device)
        edits = {k: torch.from_numpy(tab[k]).to(device) for k in ("pos", "ref_len", "alt_len", "alt_off")}
        for v0 in range(0, V, chunk):
            piece = {k: t[v0:v0 + chunk] for k, t in edits.items()}
            piece["alt"] = alt_d
            bits, site = variant_best_device(null.scores, null.widths, seq_d, piece, strands == "both", True, flag_d)
            parts.append(_select(null, bits, site, v0, keep == "all"))
        flags = int(flag_d.item())
    fields = {k: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
              for k, dt in _EMPTY.items() if k not in ("ref_score", "alt_score", "delta")}
    m = fields["motif"]
    for name in ("ref", "alt"):
        isc = fields[name + "_iscore"].astype(np.float64)
        ok = (isc >= 0) & (null.scale[m] > 0)
        # a pair's motif is never empty where it has a site: scale > 0
        fields[name + "_score"] = np.where(ok, isc / np.where(ok, null.scale[m], 1.0) + widths[m] * null.lo[m], np.nan)
    fields["delta"] = fields["alt_score"] - fields["ref_score"]
    thr = null.thresholds.cpu().numpy()
    return MotifVariantEffects(fields, ids, titles, widths, thr, tab["pos"], tab["ref_len"], tab["alt_len"], flags)


def motif_variant_records(motifs, records, variants, **kwargs):
    """motif_variants() per FASTA record: records [(id, codes), ...] (loader.read_fasta_records), variants a list
    of variants.Variant.  Returns (index, results): results[j] is the MotifVariantEffects of the variants index[j]
    (positions in `variants`, file order kept) of one record; variants whose chromosome is not among the records
    appear in no index.  check_ref (default True) compares the VCF's REF alleles with the record."""
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
        results.append(motif_variants(motifs, codes, [variants[i].pos for i in idx], [len(r) for r in refs],
                                      [allele_codes(variants[i].alt) for i in idx], **kw))
        index.append(idx)
    return index, results


# ---------------------------------------------------------------- command line
HEADER = ("Chrom\tPos\tId\tRef\tAlt\tMotif\tName\tEffect\tRefScore\tAltScore\tDelta\tRefPvalue\tAltPvalue\tRefOffset\t"
          "RefStrand\tAltOffset\tAltStrand\n")


def tsv_rows(variants, idx, eff):
    """The lines of one record's MotifVariantEffects: idx[j] is the position in `variants` of its variant j.  Pos is
    the VCF's (1-based, untrimmed); the offsets are relative to the trimmed position; a score without a site is
    written nan, its strand '.'."""
    sign = {1: "+", -1: "-", 0: "."}
    rows = []
    for k in range(len(eff)):
        v, m = variants[idx[eff.variant[k]]], eff.motif[k]
        rows.append("%s\t%d\t%s\t%s\t%s\t%s\t%s\t%s\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\t%d\t%s\t%d\t%s\n" % (
            v.chrom, v.pos + 1, v.id, v.ref, v.alt, eff.names[m], eff.titles[m], EFFECTS[eff.effect[k]],
            eff.ref_score[k], eff.alt_score[k], eff.delta[k], eff.ref_pvalue[k], eff.alt_pvalue[k], eff.ref_offset[k],
            sign[int(eff.ref_strand[k])], eff.alt_offset[k], sign[int(eff.alt_strand[k])]))
    return rows


def _parser():
    ap = argparse.ArgumentParser(prog="python -m explainn_amd.pwmvariants", description=main.__doc__)
    ap.add_argument("motifs", help="a MEME file, a JASPAR file or a directory of filter*.jaspar")
    ap.add_argument("fasta_file")
    ap.add_argument("vcf_file")
    ap.add_argument("-o", "--output-file")
    ap.add_argument("--pvalue", type=float, default=1e-4)
    ap.add_argument("--bg", type=lambda t: _pwm._bg_arg(t, sequence=False), default=None,
                    help="uniform (default) or a,c,g,t")
    ap.add_argument("--pseudocount", type=float, default=0.1)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--strands", choices=("both", "fwd"), default="both")
    ap.add_argument("--all", action="store_true", help="every (variant, motif) pair, not only those at --pvalue")
    ap.add_argument("--no-trim", action="store_true", help="keep the bases REF and ALT share (a VCF's anchor base)")
    ap.add_argument("--no-check-ref", action="store_true")
    return ap


def main(argv=None):
    """Variants of a VCF on the sequences of a FASTA against known motifs -> TSV (Chrom, Pos, Id, Ref, Alt, Motif,
    Name, Effect, RefScore, AltScore, Delta, RefPvalue, AltPvalue, RefOffset, RefStrand, AltOffset, AltStrand): one
    row per (variant, motif) pair where either allele has a site at --pvalue; Pos is the VCF's (1-based).  The
    p-values are per window, not corrected for the windows an allele touches."""
    args = _parser().parse_args(argv)
    from .loader import open_output, read_fasta_records
    motifs = _motifs.read_motifs(args.motifs)
    variants, skipped = read_vcf(args.vcf_file)
    records = read_fasta_records(args.fasta_file)
    index, results = motif_variant_records(
        motifs, records, variants, pvalue=args.pvalue, bg=args.bg, pseudocount=args.pseudocount, bins=args.bins,
        strands=args.strands, trim=not args.no_trim, keep="all" if args.all else "hits",
        check_ref=not args.no_check_ref)
    placed = sum(len(idx) for idx in index)
    if skipped or placed < len(variants):
        sys.stderr.write("%d symbolic allele(s) skipped, %d variant(s) on sequences the FASTA does not hold\n"
                         % (skipped, len(variants) - placed))
    with open_output(args.output_file) as fh:
        fh.write(HEADER)
        for idx, eff in zip(index, results):
            fh.writelines(tsv_rows(variants, idx, eff))


if __name__ == "__main__":
    main()
