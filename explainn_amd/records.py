"""From records to the best site of every unit: the one host path under `enrichment`, `centrality` and
`pwmenrich`.

A *scorer* is what differs between a model's filters (FilterScorer) and database motifs
(pwmenrich.MotifScorer): `units`, `need` (the shortest record that has a site), `device`, `best(seq, offsets,
want_site)` -> (bits int16 (units, R), site int32 (units, R) or None) for the R records
seq[offsets[r]:offsets[r + 1]], `span()` (a context manager around a run of `best` calls) and `finish()` (once,
after the last scoring call and before the test).  The rest is written once, for any scorer: the chunked
driver, the shuffled control, the control's checks and labels, the site word, the best-site containers'
common half and the order of a table's rows.  Nothing here needs a device but the scorer's own `best`.
"""
import contextlib

import numpy as np
import torch

from .strands import eval_pass

CHUNK_BASES = 1 << 26        # bases per device call of best_over_records
LABEL_PRIMARY, LABEL_CONTROL, LABEL_EXCLUDED = 1, 0, 2


def record_codes(records):
    """(ids, [1-D uint8 arrays]) of a list of (id, codes) pairs or of code arrays."""
    ids, codes = [], []
    for i, rec in enumerate(records):
        rid, c = rec if isinstance(rec, tuple) else (str(i), rec)
        c = c.cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        if c.dtype != np.uint8 or c.ndim != 1:
            raise ValueError("record %s: base codes must be a 1-D uint8 array" % (rid,))
        ids.append(rid)
        codes.append(c)
    return ids, codes


def record_chunks(lengths, chunk_bases):
    """[(first record, one past the last), ...]: runs of whole records of at most chunk_bases bases each (a
    record longer than that is a run of its own)."""
    chunk_bases = int(chunk_bases)
    if chunk_bases < 1:
        raise ValueError("chunk_bases must be at least 1 (got %d)" % chunk_bases)
    out, first, held = [], 0, 0
    for i, n in enumerate(lengths):
        if i > first and held + int(n) > chunk_bases:
            out.append((first, i))
            first, held = i, 0
        held += int(n)
    if len(lengths) > first:
        out.append((first, len(lengths)))
    return out


def record_labels(primary_lengths, control_lengths, kernel_size):
    """uint8 labels of the primary records followed by the control records: 1 / 0, and 2 (left out of the
    test) for a record shorter than the kernel, which has no site."""
    lab = np.concatenate([np.full(len(primary_lengths), LABEL_PRIMARY, np.uint8),
                          np.full(len(control_lengths), LABEL_CONTROL, np.uint8)])
    short = np.concatenate([np.asarray(primary_lengths, np.int64), np.asarray(control_lengths, np.int64)]) < kernel_size
    lab[short] = LABEL_EXCLUDED
    return lab


# ---------------------------------------------------------------- the site word
def unpack_site(site):
    """(start, strand) of the device's int32 site words (start << 1) | is_minus, -1 without a site: start -1
    and strand 0 there, strand +1 / -1 elsewhere."""
    site = np.asarray(site, dtype=np.int32)
    none = site < 0
    return np.where(none, -1, site >> 1), np.where(none, 0, 1 - 2 * (site & 1))


def pack_site(start, strand):
    """The int32 site words of (start, strand): unpack_site's inverse."""
    start = np.asarray(start)
    return np.where(start < 0, -1, (start.astype(np.int64) << 1) | (np.asarray(strand) < 0)).astype(np.int32)


class BestSites:
    """What the best-site containers share: `start` int32 and `strand` int8, shaped like the score matrix,
    `lengths` int64 (N,) and `ids` (None, or one per record; in an .npz an empty array stands for None)."""

    def _set_sites(self, scores, start, strand, lengths, ids, what, rows=None):      # what: for the error
        self.start = np.asarray(start, dtype=np.int32)
        self.strand = np.asarray(strand, dtype=np.int8)
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.ids = None if ids is None else [str(i) for i in ids]
        if scores.ndim != 2 or scores.shape != self.start.shape or scores.shape != self.strand.shape or \
                (rows is not None and scores.shape[0] != rows) or self.lengths.shape != (scores.shape[1],):
            raise ValueError("%s, start and strand must be (%s, N) and lengths (N,)" % what)

    def _ids_array(self):
        return np.array(self.ids if self.ids is not None else [], dtype=np.str_)

    @staticmethod
    def _ids_of(z):
        return [str(i) for i in z["ids"]] if len(z["ids"]) == len(z["lengths"]) else None


class RecordBest(BestSites):
    """The best site of every unit in every record: `score` float16 (units, N), the largest activation over
    the record's live starts (0 where the record is shorter than the kernel); `start` int32 (units, N), the
    0-based forward start of the k-mer that holds it (-1 without one) -- the lowest among equal maxima;
    `strand` int8 (units, N), +1 / -1 ('+' wins a tie at one start; 0 without a site); `lengths` int64 (N,)."""

    def __init__(self, score, start, strand, lengths, kernel_size, ids=None):
        self.score = np.asarray(score, dtype=np.float16)
        self.kernel_size = int(kernel_size)
        self._set_sites(self.score, start, strand, lengths, ids, ("score", "units"))

    @property
    def bits(self):
        """uint16 (units, N): the scores' bit patterns, which sort like the scores."""
        return self.score.view(np.uint16)

    @classmethod
    def from_device(cls, bits, site, lengths, kernel_size, ids=None):
        return cls(np.ascontiguousarray(bits).view(np.float16), *unpack_site(site), lengths, kernel_size, ids)

    def save(self, path):
        with open(path, "wb") as fh:
            np.savez(fh, bits=self.bits, start=self.start, strand=self.strand, lengths=self.lengths,
                     k=np.int64(self.kernel_size), ids=self._ids_array())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["bits"].view(np.float16), z["start"], z["strand"], z["lengths"], int(z["k"]), cls._ids_of(z))


# ---------------------------------------------------------------- scorers and the driver
class FilterScorer:
    """The filters of `model` (an ExplaiNN, or an ExplaiNNBank: global unit indices) on n_strands (1 or 2)
    strands: explainn_record_best.  Eval mode only."""

    def __init__(self, model, n_strands):
        self.model, self.n_strands = model, n_strands
        self.units, self.need = model._units(), model._options["kernel_size"]

    @property
    def device(self):
        return self.model._device()

    def best(self, seq, offsets, want_site):
        return self.model._launch_record_best(seq, offsets, self.n_strands, want_site)

    @contextlib.contextmanager
    def span(self):
        if self.model.training:
            raise NotImplementedError("the best sites are an eval-mode export path; call model.eval()")
        with eval_pass(self.model, settle=False):       # best_over_records opens several spans before one finish()
            yield

    def finish(self):
        if self.model.validate_input:
            self.model.check_input()


def best_over_records(scorer, codes, chunk_bases=None, want_site=True):
    """(bits int16 -- the patterns are below 0x8000 --, site int32 or None), each (units, len(codes)) on the
    scorer's device: the 1-D uint8 arrays `codes` go over concatenated, in runs of whole records of at most
    chunk_bases bases (None: CHUNK_BASES); every run is one scorer.best call and column r is record r."""
    lengths = np.array([len(c) for c in codes], dtype=np.int64)
    with scorer.span():
        device = scorer.device
        bits = torch.empty((scorer.units, len(codes)), device=device, dtype=torch.int16)
        site = torch.empty((scorer.units, len(codes)), device=device, dtype=torch.int32) if want_site else None
        for r0, r1 in record_chunks(lengths, CHUNK_BASES if chunk_bases is None else chunk_bases):
            flat = np.concatenate(codes[r0:r1] + [np.full(1, 4, np.uint8)])      # never an empty tensor
            off = np.zeros(r1 - r0 + 1, dtype=np.int64)
            np.cumsum(lengths[r0:r1], out=off[1:])
            b, s = scorer.best(torch.from_numpy(flat).to(device), torch.from_numpy(off).to(device), want_site)
            bits[:, r0:r1] = b
            if want_site:
                site[:, r0:r1] = s
    return bits, site


def shuffled_control(scorer, codes, shuffles, seed, chunk_bases=None):
    """Device bits (units, N x shuffles) of `shuffles` dinucleotide-preserving shuffles of every record (all
    of one length L), drawn on the device chunk by chunk: column r * shuffles + s is shuffle s of record r."""
    from .sequence import dinucleotide_shuffle_device
    L = len(codes[0])
    rows = torch.from_numpy(np.stack(codes))
    per = max(int(CHUNK_BASES if chunk_bases is None else chunk_bases) // max(L * shuffles, 1), 1)
    with scorer.span():
        device = scorer.device
        out = torch.empty((scorer.units, len(codes) * shuffles), device=device, dtype=torch.int16)
        for r0 in range(0, len(codes), per):
            shuf = dinucleotide_shuffle_device(rows[r0:r0 + per].to(device), shuffles, seed, row0=r0).reshape(-1)
            n = shuf.numel() // L
            off = torch.arange(n + 1, device=device, dtype=torch.int64) * L
            out[:, r0 * shuffles:r0 * shuffles + n] = scorer.best(shuf.contiguous(), off, False)[0]
    return out


def control_plan(prim, control, shuffles):
    """(ctrl, ctrl_lengths, shuffles) for the primary code arrays `prim`.  With a control set: its code arrays,
    their lengths and 0.  Without: None, the lengths of `shuffles` >= 1 shuffles of every primary record -- which
    must be of one length and not empty -- and shuffles."""
    if not prim:
        raise ValueError("no primary record")
    if control is not None:
        _, ctrl = record_codes(control)
        return ctrl, [len(c) for c in ctrl], 0
    if int(shuffles) < 1:
        raise ValueError("shuffles must be at least 1 without a control set")
    if len({len(c) for c in prim}) != 1:
        raise ValueError("a shuffled control needs primary records of one length; pass control= for records "
                         "of unequal lengths")
    if len(prim[0]) == 0:
        raise ValueError("the primary records are empty")
    return None, np.repeat([len(c) for c in prim], int(shuffles)), int(shuffles)


def enrichment_bits(scorer, primary, control=None, shuffles=1, seed=0, chunk_bases=None):
    """What explainn_enrichment_test takes: (bits int16 (units, Np + Nc) on the device, the primary records'
    best scores, then the control's; labels uint8, numpy, records shorter than scorer.need left out; shuffles)."""
    _, prim = record_codes(primary)
    ctrl, ctrl_lengths, shuffles = control_plan(prim, control, shuffles)
    labels = record_labels([len(c) for c in prim], ctrl_lengths, scorer.need)
    pbits, _ = best_over_records(scorer, prim, chunk_bases, False)
    if ctrl is None:
        cbits = shuffled_control(scorer, prim, shuffles, seed, chunk_bases)
    else:
        cbits, _ = best_over_records(scorer, ctrl, chunk_bases, False)
    scorer.finish()
    return torch.cat([pbits, cbits], dim=1).contiguous(), labels, shuffles


# ---------------------------------------------------------------- tables
def table_order(result, max_evalue=None, keep=None):
    """The units of a result table, in its order: those of `keep` (None: all) with evalue <= max_evalue (None:
    all), by ascending log_pvalue, ties by index."""
    keep = np.arange(result.units) if keep is None else np.asarray(keep)
    if max_evalue is not None:
        keep = keep[result.evalue[keep] <= max_evalue]
    return keep[np.lexsort((keep, result.log_pvalue[keep]))]
