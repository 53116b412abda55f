"""Case lists for the filter -> PWM export (csrc/interpret.hip) away from the 200 bp shape, and their
fp64 reference.  tests/test_export_model.py (CPU) asserts that every case reaches what it claims and
holds no float16 knife edge; tests/test_gpu_export_edges.py runs the cases on the device and compares
exactly.

The kernel walks the start positions of a sequence in chunks of SITE_T = 256 threads; a site's rank
among the sites of its unit is  offset of its sequence + sites in earlier chunks + sites of earlier
waves of the chunk + sites of earlier lanes of the wave,  and only ranks below the cap are counted.
A case therefore needs Lo = L - k + 1 > 256 to enter the chunk loop twice, and a cap that falls
inside a later chunk for the carried count to decide anything.

Reference: the oracle's eval forward in fp64, its activations rounded to float16 (the array the
reference's test.py stores), then oracle/interpret_oracle.py's thresholds / sites / counts.

Knife edges: the device forms the activation in fp32 (v_exp_f32), so where the fp64 value sits
within the device's error of a float16 rounding boundary the two float16 values may differ.  That
matters in two places only: at the unit's maximum (it sets the threshold) and across the threshold
(it makes or unmakes a site).  delta() bounds the device's relative error by 4x the fp32 oracle's on
the same case (floor 2^-20); knife_edges() counts the selected activations for which float16 of
a(1 - delta) and a(1 + delta) differ and either the larger reaches the unit's maximum or the two lie
on different sides of the threshold.  Every case is seeded so that the count is zero, which is what
lets the device comparison be array_equal.
"""
import functools
import math

import numpy as np

from oracle import explainn_oracle as eo
from oracle import interpret_oracle as io

SITE_T = 256                 # csrc/interpret.hip
SCAN_LANES = 64              # site_scan_kernel: sequences per trip
DELTA_FLOOR = 2.0 ** -20
THR_MARGIN = 2.0 ** -17      # chosen thresholds keep every activation this far (relative) from the
#                              float16 midpoint above them; the CPU test checks the case's own delta

# what the list as a whole has to reach: tag -> what is lost when no case claims it
REQUIRED = {
    "lo256": "Lo = 256: one full chunk, the loop must not run a second time",
    "lo257": "Lo = 257: one live thread in chunk 2",
    "chunks3_ragged": "3 position chunks with a ragged last one (Lo = 582, the C5 length)",
    "chunks4": "4 position chunks (Lo = 982, the C4 length)",
    "k2": "k = 2 with Lo > 256 (smallest histogram and weight tile)",
    "k32": "k = 32 with Lo > 256 (largest histogram and weight tile)",
    "U1": "U = 1: three padding lanes in the only quad",
    "U2": "U = 2: two padding lanes",
    "U3": "U = 3: one padding lane",
    "cap_in_later_chunk": "the cap reached in chunk >= 2 of a sequence that is not the first selected one",
    "cap_in_batch1": "the cap reached in batch 1; batches 2 and 3 must add nothing (off clamped to cap)",
    "cap_on_reverse": "reverse-complement halves with the cap reached on the reverse strand",
    "selection_runs": "unselected sequences first, last and in runs; 2 % N bases; one sequence all N",
    "inf_unit": "a unit whose float16 activations overflow to +inf (threshold inf, no site)",
    "zero_unit": "a unit whose float16 activations underflow to 0 (threshold 0, no site)",
    "batch1": "batches of one sequence",
    "batch65": "a batch of 65 sequences: second trip of site_scan_kernel with one live lane",
}


def _case(name, U, k, L, N, seed, tags, batch_sizes=(1024,), sel="all", n_frac=0.0, rc=False,
          shrink=False, mode="pwms", extremes=None, cap=None):
    return dict(name=name, U=U, k=k, L=L, N=N, seed=seed, tags=tuple(tags), batch_sizes=tuple(batch_sizes),
                sel=sel, n_frac=n_frac, rc=rc, shrink=shrink, mode=mode, extremes=extremes, cap=cap)


# mode "pwms": through interpret.filter_pwms (maxima -> thresholds -> sites); mode "sites": through
# model.filter_sites with thresholds chosen here near each unit's median activation.
# cap: None (the product's 1e6), or a rule evaluated on the reference's own counts (reference()).
CASES = [
    _case("lo256", 5, 5, 260, 12, 0, ["lo256", "batch1"], batch_sizes=(1024, 1)),
    _case("lo257", 5, 5, 261, 12, 0, ["lo257"], batch_sizes=(5,)),
    _case("c5_len", 6, 19, 600, 10, 0, ["chunks3_ragged", "selection_runs"], batch_sizes=(1024, 4),
          sel="runs", n_frac=0.02),
    _case("c4_len", 4, 19, 1000, 6, 0, ["chunks4"], batch_sizes=(4,)),
    _case("k2", 7, 2, 300, 8, 0, ["k2"], sel="runs", n_frac=0.02),
    _case("k32", 7, 32, 300, 8, 0, ["k32"], sel="runs", n_frac=0.02),
    _case("u1", 1, 9, 300, 8, 0, ["U1"]),
    _case("u2", 2, 9, 300, 8, 0, ["U2"], batch_sizes=(3,)),
    _case("u3", 3, 9, 300, 8, 0, ["U3"]),
    _case("dense_cap", 5, 19, 600, 8, 0, ["cap_in_later_chunk"], batch_sizes=(1024, 3), sel="runs",
          shrink=True, mode="sites", cap="later_chunk"),
    _case("batch_cap", 5, 19, 600, 9, 0, ["cap_in_batch1"], batch_sizes=(3,), shrink=True, cap="batch1"),
    _case("rc_cap", 4, 9, 300, 16, 0, ["cap_on_reverse"], batch_sizes=(1024, 3), rc=True, shrink=True,
          cap="reverse"),
    _case("extremes", 6, 9, 300, 8, 0, ["inf_unit", "zero_unit"], extremes=(1, 2)),
    _case("b65", 3, 5, 60, 66, 0, ["batch65"], batch_sizes=(65,)),
]


def case(name):
    return next(c for c in CASES if c["name"] == name)


def onehot(codes):
    codes = np.asarray(codes)
    return (codes[:, None, :] == np.arange(4)[None, :, None]).astype(np.float32)


def chunks(c):
    return -(-(c["L"] - c["k"] + 1) // SITE_T)


def _rc_codes(codes):
    r = codes[:, ::-1]
    return np.where(r < 4, 3 - r, r).astype(np.uint8)


def _selection(c, half):
    """Selected indices into the forward half.  "runs": unselected first, last and as a pair."""
    if c["sel"] == "all":
        return np.arange(half, dtype=np.int64)
    keep = np.ones(half, dtype=bool)
    keep[[0, 3, 4, half - 1]] = False
    return np.flatnonzero(keep).astype(np.int64)


def _acts64(sd, x):
    return eo.forward(sd, x, training=False, dtype=np.float64, return_cache=True)[1]["acts"]


def _f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a).astype(np.float16)


def inputs(c):
    """(state dict float32, codes uint8 (N,L), idxs): everything the device is given."""
    return _inputs(c["name"])


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = case(name)
    U, k, L, N = c["U"], c["k"], c["L"], c["N"]
    sd = eo.random_state_dict(U, k, L, 1, seed=100 + c["seed"])
    g = np.random.default_rng(1000 + c["seed"])
    half = N // 2 if c["rc"] else N
    codes = g.integers(0, 4, size=(half, L)).astype(np.uint8)
    if c["n_frac"] > 0:
        codes[g.random((half, L)) < c["n_frac"]] = 4
    idxs = _selection(c, half)
    if c["sel"] == "runs":
        codes[idxs[2]] = 4                                   # one selected sequence of only N
    if c["rc"]:
        codes = np.concatenate([codes, _rc_codes(codes)])
    if c["shrink"] or c["extremes"]:
        y = np.log(_acts64(sd, onehot(codes)))               # (N,U,Lo) exponents
        s = np.sqrt(sd["linears.1.running_var"].astype(np.float64) + eo.BN_EPS)
        g1 = sd["linears.1.weight"].astype(np.float64)
        if c["shrink"]:
            # exponent span 0.6 ln 2: the smallest activation stays above half the largest, so with
            # thresholds of half the maximum nearly every position is a site
            span = y.max(axis=(0, 2)) - y.min(axis=(0, 2))
            sd["linears.1.weight"] = (g1 * 0.6 * math.log(2.0) / span).astype(np.float32)
        if c["extremes"]:
            # conv bias such that the exponent is gamma*conv/sigma + target: +16 puts every position
            # above float16's largest finite value (exp(11.09)), -22 below half its smallest
            # subnormal (exp(-17.33)); |gamma*conv/sigma| stays below 4
            b0 = sd["linears.0.bias"].astype(np.float64)
            for u, target in zip(c["extremes"], (16.0, -22.0)):
                b0[u] = sd["linears.1.running_mean"][u] + s[u] / g1[u] * (target - sd["linears.1.bias"][u])
            sd["linears.0.bias"] = b0.astype(np.float32)
    return sd, codes, idxs


def selected_rows(c, idxs, N):
    return np.concatenate([idxs, idxs + N // 2]) if c["rc"] else idxs


def delta(c):
    """4x the worst relative deviation of the fp32 oracle's activations (the arithmetic behind
    interpret_oracle.acts_outs_preds, before its float16 rounding) from the fp64 ones, floor 2^-20."""
    sd, codes, _ = inputs(c)
    x = onehot(codes)
    a64 = _acts64(sd, x)
    a32 = eo.unit_activations(sd, x, dtype=np.float32).astype(np.float64)
    return max(DELTA_FLOOR, 4.0 * float((np.abs(a32 - a64) / a64).max()))


def knife_edges(a64_sel, thr16, d, at_max):
    """Number of activations of a64_sel (S,U,Lo: the selected rows) that a relative error of d could
    move across a float16 rounding boundary that matters (module docstring)."""
    lo, hi = _f16(a64_sel * (1.0 - d)), _f16(a64_sel * (1.0 + d))
    split = lo != hi
    t = np.asarray(thr16, dtype=np.float16)[None, :, None]
    edge = split & ((lo > t) != (hi > t))
    if at_max:
        edge |= split & (hi >= _f16(a64_sel).max(axis=(0, 2))[None, :, None])
    return int(edge.sum())


def _median_thresholds(a64_sel):
    """Per unit the float16 value nearest the median activation whose midpoint to the next float16 --
    the real value above which an activation rounds past it -- has no activation within THR_MARGIN."""
    out = np.zeros(a64_sel.shape[1], dtype=np.float16)
    for u in range(a64_sel.shape[1]):
        a = a64_sel[:, u, :].reshape(-1)
        t = np.float16(np.median(a))
        for _ in range(64):
            up = np.nextafter(t, np.float16(np.inf))
            mid = 0.5 * (float(t) + float(up))
            if np.abs(a / mid - 1.0).min() > THR_MARGIN:
                break
            t = np.nextafter(t, np.float16(0))
        else:
            raise AssertionError("no clean float16 threshold near the median of unit %d" % u)
        out[u] = t
    return out


def per_sequence_counts(acts16, rows, thr16):
    """(U, len(rows), chunks) site counts of the selected rows in selection order, per position chunk."""
    hit = acts16[rows] > np.asarray(thr16, dtype=np.float16)[None, :, None]        # (S,U,Lo)
    Lo = hit.shape[2]
    return np.stack([hit[:, :, p0:p0 + SITE_T].sum(axis=2) for p0 in range(0, Lo, SITE_T)], axis=2).transpose(1, 0, 2)


def _cap(c, cnt, n_fwd):
    """The cap of a case from the reference's own counts cnt (U,S,chunks)."""
    rule = c["cap"]
    if rule is None:
        return io.SITE_CAP
    per_seq = cnt.sum(axis=2)                                                     # (U,S)
    if rule == "later_chunk":
        # unit 0, last selected sequence: everything before it, its first chunk, half its second
        s = cnt.shape[1] - 1
        return int(per_seq[0, :s].sum() + cnt[0, s, 0] + (cnt[0, s, 1] + 1) // 2)
    if rule == "batch1":
        # inside the first batch of every unit, past its first sequence
        b = c["batch_sizes"][0]
        return int(min(per_seq[:, :b].sum(axis=1).min() - 7, per_seq[:, 0].max() + per_seq[:, 1].min() // 2))
    if rule == "reverse":
        # unit 0: the whole forward strand, one reverse sequence, and most of the next
        return int(per_seq[0, :n_fwd + 1].sum() + per_seq[0, n_fwd + 1] * 9 // 10)
    raise ValueError(rule)


def reference(c):
    """dict(acts64, acts16 (N,U,Lo), rows, thresholds float16 (U,), cap, pfm, nsites, hit (N,U), counts
    (U,S,chunks)): what the device has to return for the case, from the fp64 oracle alone."""
    return _reference(c["name"])


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = case(name)
    sd, codes, idxs = inputs(c)
    a64 = _acts64(sd, onehot(codes))
    a16 = _f16(a64)
    rows = selected_rows(c, idxs, len(codes))
    if c["mode"] == "pwms":
        thr = io.act_thresholds(a16, idxs, c["rc"]).astype(np.float16)
    else:
        thr = _median_thresholds(a64[rows])
    cnt = per_sequence_counts(a16, rows, thr)
    cap = _cap(c, cnt, len(idxs))
    pfm, nsites = io.site_pfms(codes, a16, idxs, thr, c["k"], c["rc"], cap=cap)
    hit = np.zeros((len(codes), c["U"]), dtype=bool)
    hit[rows] = (a16[rows] > thr[None, :, None]).any(axis=2)
    return dict(acts64=a64, acts16=a16, rows=rows, thresholds=thr, cap=cap, pfm=pfm, nsites=nsites, hit=hit,
                counts=cnt)
