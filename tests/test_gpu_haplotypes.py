"""Haplotypes on the device: explainn_stage_haplotype_windows, explainn_score_haplotypes and
explainn_amd.variants.score_haplotypes.  -m gpu.  Every case runs once.

What is compared with what:
  * explainn_stage_haplotype_windows against explainn_stage_codes on the (B,L) matrix the numpy
    haplotype model builds by concatenation (tests/haplotype_model.py): the eval logits and the unit
    outputs of the staged batch, and the loss and all 14 gradients of one train step, torch.equal -- both
    routes feed identical packed buffers into a deterministic pipeline;
  * runs of one edit and empty runs against explainn_stage_edited_windows on the equivalent
    explainn_edits, torch.equal;
  * bad tables: the bad row equals an all-N row, flag bit 0, every other row as the model;
  * score_haplotypes against predict() on the host-materialised windows, np.array_equal on all four
    columns, and against the fp64 oracle at TOL (1e-4 absolute, the project's logit tolerance).
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import TOL, close, model, to_np  # noqa: E402
import haplotype_model as hm  # noqa: E402
import scan_model as sm  # noqa: E402
import variants_model as vm  # noqa: E402

pytestmark = pytest.mark.gpu

L0, K0 = 200, 19
SEQ_LEN = 1000


def _lib():
    from explainn_amd import _lib
    return _lib


def _sd(U, k, L, T, seed=0):
    sd = orc.random_state_dict(U, k, L, T, seed=seed)
    rng = np.random.default_rng(seed + 5)
    # half of the units pool the minimum (gamma1 < 0)
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, U) * np.where(np.arange(U) % 2, 1, -1)).astype(np.float32)
    return sd


def _oracle_logits(sd, mat):
    return orc.forward(sd, sm.onehot(mat), dtype=np.float64)


def _eval_model(sd, U, k, L, T):
    m = model(sd, U, k, L, T).eval()
    m.validate_input = False
    return m


def _ctx(m, B):
    dev = m._device()
    with torch.cuda.device(dev):
        ctx = m._context(B, dev)
        ps, keep = m._params_struct(dev)
    return ctx, ps, keep, m._stream(dev)


def _staged(m, ctx, ps, stream, B, stage):
    """(eval logits, unit outputs) of the batch `stage` stages."""
    lib, h = ctx.lib, ctx.handle
    logits = m._logits_empty(B, torch.device("cuda"))
    outs = torch.empty(B, m._units(), device="cuda")
    _lib().check(stage())
    _lib().check(lib.explainn_forward_eval(h, None, B, C.byref(ps), logits.data_ptr(), stream))
    _lib().check(stage())
    _lib().check(lib.explainn_unit_outputs(h, None, B, C.byref(ps), outs.data_ptr(), stream))
    torch.cuda.synchronize()
    return logits, outs


def _flags(ctx, stream):
    flags = C.c_int(0)
    _lib().check(ctx.lib.explainn_input_flags(ctx.handle, C.byref(flags), stream))
    return flags.value


def _haps(tab):
    """explainn_haplotypes of numpy tables, each allocated at its stated size: (struct, the device
    tensors that keep it alive)."""
    names = _lib().HAPLOTYPE_FIELDS[:9]
    dev = {k: torch.from_numpy(np.ascontiguousarray(tab[k])).cuda() for k in names}
    hp = _lib().Haplotypes()
    for k, t in dev.items():
        setattr(hp, k, t.data_ptr() if t.numel() else None)
    hp.n_index, hp.n_edits, hp.alt_bytes = len(tab["edit_index"]), len(tab["pos"]), len(tab["alt"])
    return hp, dev


def _edits(tab):
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in tab.items()}
    ed = _lib().Edits()
    for k, t in dev.items():
        setattr(ed, k, t.data_ptr() if t.numel() else None)
    ed.n_edits, ed.alt_bytes = len(tab["pos"]), len(tab["alt"])
    return ed, dev


# ---- explainn_stage_haplotype_windows -------------------------------------------------------------

@pytest.mark.parametrize("rc", [0, 1])
@pytest.mark.parametrize("L,k,B,first", [(L0, K0, 1, 27), (L0, K0, 64, 0), (L0, K0, 65, 5), (40, 5, 65, 0)])
def test_stage_haplotype_windows_equals_stage_codes(L, k, B, first, rc):
    """Every run of haplotype_model.run_cases (lengths 0..130, see there), whole and ragged 64-row tiles,
    both strands; at L = 40 the row is shorter than a position tile.  B = 1 stages a 64-edit run."""
    U, T = 8, 2
    seq = sm.random_codes(SEQ_LEN, seed=L + B, n_runs=6)
    cases = hm.run_cases(seq, L, seed=B)
    assert B > 1 or len(cases[first][1]) == 64
    tab = hm.tables_from_runs(cases, B, first)
    mat = hm.cases_matrix(seq, cases, B, L, first)
    sd = _sd(U, k, L, T, seed=3)
    m = _eval_model(sd, U, k, L, T)
    ctx, ps, keep, stream = _ctx(m, B)
    h, lib = ctx.handle, ctx.lib
    seq_d, mat_d = torch.from_numpy(seq).cuda(), torch.from_numpy(mat).cuda()
    hp, alive = _haps(tab)
    la, oa = _staged(m, ctx, ps, stream, B, lambda: lib.explainn_stage_haplotype_windows(
        h, seq_d.data_ptr(), len(seq), C.byref(hp), 0, B, rc, stream))
    assert _flags(ctx, stream) == 0, "N padding, N in alt and N in seq must not raise the flag"
    lb, ob = _staged(m, ctx, ps, stream, B, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), B, rc, stream))
    assert torch.equal(la, lb), float((la - lb).abs().max())
    assert torch.equal(oa, ob), float((oa - ob).abs().max())
    close(to_np(la), _oracle_logits(sd, sm.rc_rows(mat) if rc else mat), TOL, "stage_haplotype_windows logits")
    if B == 65:
        # row0: the last 20 rows of the same tables are rows 45.. of the matrix
        lc, oc = _staged(m, ctx, ps, stream, 20, lambda: lib.explainn_stage_haplotype_windows(
            h, seq_d.data_ptr(), len(seq), C.byref(hp), 45, 20, rc, stream))
        assert torch.equal(lc, la[45:]) and torch.equal(oc, oa[45:])


def test_stage_haplotype_windows_on_a_bank():
    from explainn_amd import ExplaiNNBank
    G, U, T, B = 2, 8, 2, 65
    bank = ExplaiNNBank.from_models([model(_sd(U, K0, L0, T, seed=20 + g), U, K0, L0, T) for g in range(G)])
    bank = bank.cuda().eval()
    bank.validate_input = False
    seq = sm.random_codes(SEQ_LEN, seed=21, n_runs=4)
    cases = hm.run_cases(seq, L0, seed=22)
    tab = hm.tables_from_runs(cases, B, 9)
    mat_d = torch.from_numpy(hm.cases_matrix(seq, cases, B, L0, 9)).cuda()
    seq_d = torch.from_numpy(seq).cuda()
    ctx, ps, keep, stream = _ctx(bank, B)
    h, lib = ctx.handle, ctx.lib
    hp, alive = _haps(tab)
    la, oa = _staged(bank, ctx, ps, stream, B, lambda: lib.explainn_stage_haplotype_windows(
        h, seq_d.data_ptr(), len(seq), C.byref(hp), 0, B, 1, stream))
    lb, ob = _staged(bank, ctx, ps, stream, B, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), B, 1, stream))
    assert la.shape == (B, G, T) and oa.shape == (B, G * U)
    assert torch.equal(la, lb) and torch.equal(oa, ob) and _flags(ctx, stream) == 0
    # explainn_score_haplotypes on the bank context: the same rows in sub-batches of its own
    lg, ou = torch.zeros_like(la), torch.zeros_like(oa)
    _lib().check(lib.explainn_score_haplotypes(h, seq_d.data_ptr(), len(seq), C.byref(hp), B, 1, C.byref(ps),
                                              lg.data_ptr(), ou.data_ptr(), stream))
    torch.cuda.synchronize()
    assert torch.equal(lg, la) and torch.equal(ou, oa)


def _grads_struct(m):
    L_ = _lib()
    g = L_.Grads()
    sd = dict(m.state_dict())
    keep = {}
    for f in L_.GRAD_FIELDS:
        keep[f] = torch.zeros_like(sd[L_.PARAM_KEYS[f]]).contiguous()
        setattr(g, f, keep[f].data_ptr())
    return g, keep


def test_stage_haplotype_windows_train_step_is_bit_equal():
    """A staged haplotype batch feeds a train step like a staged code matrix: the same loss and the same
    14 gradients, bit for bit (this pins bm, the bitmask layout only training reads)."""
    U, T, B = 8, 2, 65
    sd = _sd(U, K0, L0, T, seed=6)
    seq = sm.random_codes(SEQ_LEN, seed=8, n_runs=4)
    cases = hm.run_cases(seq, L0, seed=2)
    tab = hm.tables_from_runs(cases, B, 3)
    mat = hm.cases_matrix(seq, cases, B, L0, 3)
    rng = np.random.default_rng(9)
    keep_mask = torch.from_numpy((rng.random((B, 100 * U)) > 0.3).astype(np.uint8)).cuda()
    y = torch.from_numpy((rng.random((B, T)) > 0.5).astype(np.float32)).cuda()
    seq_d, mat_d = torch.from_numpy(seq).cuda(), torch.from_numpy(mat).cuda()
    hp, alive = _haps(tab)
    results = []
    for which in ("haplotypes", "codes"):
        m = model(sd, U, K0, L0, T).train()
        ctx, ps, keepalive, stream = _ctx(m, B)
        h, lib = ctx.handle, ctx.lib
        g, gk = _grads_struct(m)
        logits = torch.empty(B, T, device="cuda")
        dl = torch.empty(B, T, device="cuda")
        loss = torch.empty(1, device="cuda")
        if which == "haplotypes":
            _lib().check(lib.explainn_stage_haplotype_windows(h, seq_d.data_ptr(), len(seq), C.byref(hp), 0, B, 1,
                                                             stream))
        else:
            _lib().check(lib.explainn_stage_codes(h, mat_d.data_ptr(), B, 1, stream))
        _lib().check(lib.explainn_forward_train(h, None, B, C.byref(ps), keep_mask.data_ptr(), 0.3, 0,
                                               logits.data_ptr(), stream))
        _lib().check(lib.explainn_loss_grad(h, 0, logits.data_ptr(), y.data_ptr(), B, loss.data_ptr(),
                                           dl.data_ptr(), stream))
        _lib().check(lib.explainn_backward(h, dl.data_ptr(), B, C.byref(ps), C.byref(g), 0, stream))
        torch.cuda.synchronize()
        results.append((logits, loss, gk))
    (la, sa, ga), (lb, sb, gb) = results
    assert torch.equal(la, lb) and torch.equal(sa, sb) and torch.isfinite(sa).all()
    assert len(ga) == 14
    for f in ga:
        assert torch.equal(ga[f], gb[f]), "grad %s: %g" % (f, float((ga[f] - gb[f]).abs().max()))
    # (the comparison is of a real step: the filter gradient, which reads bm, is not zero; the filter
    # bias's is, exactly, under BatchNorm)
    assert ga["conv_w"].abs().max() > 0 and ga["final_w"].abs().max() > 0


# ---- agreement with the single-edit route ---------------------------------------------------------

@pytest.mark.parametrize("rc", [0, 1])
def test_single_edit_runs_equal_stage_edited_windows(rc):
    """Every edit class of variants_model.edit_cases as a run of one edit (and the rows without an edit
    as empty runs): the batch explainn_stage_edited_windows stages."""
    U, T, B = 8, 2, 65
    seq = sm.random_codes(SEQ_LEN, seed=31, n_runs=6)
    cases = vm.edit_cases(seq, L0, seed=32)
    etab = vm.tables_from_cases(cases, B)
    has = etab["row_edit"] >= 0
    htab = {k: etab[k] for k in ("row_start", "pos", "ref_len", "alt_len", "alt_off", "alt")}
    htab["row_count"] = has.astype(np.int32)
    htab["row_first"] = (np.cumsum(has) - has).astype(np.int64)
    htab["edit_index"] = etab["row_edit"][has].astype(np.int32)
    sd = _sd(U, K0, L0, T, seed=33)
    m = _eval_model(sd, U, K0, L0, T)
    ctx, ps, keep, stream = _ctx(m, B)
    h, lib = ctx.handle, ctx.lib
    seq_d = torch.from_numpy(seq).cuda()
    hp, alive = _haps(htab)
    ed, alive2 = _edits(etab)
    la, oa = _staged(m, ctx, ps, stream, B, lambda: lib.explainn_stage_haplotype_windows(
        h, seq_d.data_ptr(), len(seq), C.byref(hp), 0, B, rc, stream))
    lb, ob = _staged(m, ctx, ps, stream, B, lambda: lib.explainn_stage_edited_windows(
        h, seq_d.data_ptr(), len(seq), C.byref(ed), 0, B, rc, stream))
    assert torch.equal(la, lb) and torch.equal(oa, ob) and _flags(ctx, stream) == 0
    assert not torch.equal(la[0], la[1])


# ---- bad tables -----------------------------------------------------------------------------------

def test_bad_tables_make_the_row_n_and_raise_the_flag():
    U, T, B, ROW = 8, 1, 64, 8
    seq = sm.random_codes(SEQ_LEN, seed=1, n_runs=3)
    sd = _sd(U, K0, L0, T, seed=4)
    m = _eval_model(sd, U, K0, L0, T)
    ctx, ps, keep, stream = _ctx(m, B)
    h, lib = ctx.handle, ctx.lib
    cases = hm.run_cases(seq, L0)
    tab = hm.tables_from_runs(cases, B)
    seq_d = torch.from_numpy(seq).cuda()
    assert tab["row_count"][ROW] == 3 and tab["row_first"][0] + tab["row_count"][0] == len(tab["edit_index"])

    def staged(t):
        hp, alive = _haps(t)
        out, _ = _staged(m, ctx, ps, stream, B, lambda: lib.explainn_stage_haplotype_windows(
            h, seq_d.data_ptr(), len(seq), C.byref(hp), 0, B, 0, stream))
        return out, _flags(ctx, stream)

    def codes(mat):
        mat_d = torch.from_numpy(mat).cuda()
        return _staged(m, ctx, ps, stream, B, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), B, 0, stream))[0]

    good = hm.cases_matrix(seq, cases, B, L0)
    clean, f0 = staged(tab)
    assert f0 == 0, "a clean batch raises no flag"
    assert torch.equal(clean, codes(good))
    f, n = int(tab["row_first"][ROW]), len(tab["edit_index"])
    e0, e1 = (int(e) for e in tab["edit_index"][f:f + 2])
    last = int(tab["edit_index"][f + 2])
    assert tab["alt_len"][last] == 1

    def changed(field, at, value):
        t = dict(tab)
        t[field] = tab[field].copy()
        t[field][at] = value
        return t

    swapped = dict(tab)
    swapped["edit_index"] = tab["edit_index"].copy()
    swapped["edit_index"][[f, f + 1]] = tab["edit_index"][[f + 1, f]]
    bad = {
        "unsorted run": (ROW, swapped),
        "overlapping run": (ROW, changed("ref_len", e0, int(tab["pos"][e1] - tab["pos"][e0]) + 1)),
        "edit_index = n_edits": (ROW, changed("edit_index", f + 1, len(tab["pos"]))),
        "edit_index = -1": (ROW, changed("edit_index", f + 2, -1)),
        "row_first + row_count = n_index + 1": (0, changed("row_first", 0, tab["row_first"][0] + 1)),
        "row_first < 0": (ROW, changed("row_first", ROW, -1)),
        "negative count": (ROW, changed("row_count", ROW, -1)),
        "alt run past the pool": (ROW, changed("alt_off", last, len(tab["alt"]))),
        "negative ref_len": (ROW, changed("ref_len", e1, -1)),
        "negative alt_len": (ROW, changed("alt_len", e1, -2)),
    }
    for name, (row, t) in bad.items():
        assert hm.row_run(t, row) is None, name + ": the model accepts the run"
        want = good.copy()
        want[row] = 4
        assert np.array_equal(hm.tables_matrix(seq, t, L0), want), name
        got, flag = staged(t)
        assert flag & 1, name
        assert torch.isfinite(got).all() and torch.equal(got, codes(want)), name
    # a violation in the third chunk of a run, far right of the window: the whole row all the same
    row = next(b for b in range(B) if tab["row_count"][b] == 130)
    f = int(tab["row_first"][row])
    t = dict(tab)
    t["edit_index"] = tab["edit_index"].copy()
    t["edit_index"][[f + 128, f + 129]] = tab["edit_index"][[f + 129, f + 128]]
    want = good.copy()
    want[row] = 4
    got, flag = staged(t)
    assert flag & 1 and torch.equal(got, codes(want))
    # and the context is usable afterwards
    again, f5 = staged(tab)
    assert f5 == 0 and torch.equal(again, clean)
    # argument checks leave the context usable too
    hp, alive = _haps(tab)
    L_ = _lib()
    args = (seq_d.data_ptr(), len(seq), C.byref(hp))
    assert lib.explainn_stage_haplotype_windows(h, *args, 0, B + 1, 0, stream) == L_.E_ARG
    assert lib.explainn_stage_haplotype_windows(h, None, len(seq), C.byref(hp), 0, B, 0, stream) == L_.E_ARG
    assert lib.explainn_stage_haplotype_windows(h, *args, -1, B, 0, stream) == L_.E_ARG
    hp.alt_bytes = 2 ** 31
    assert lib.explainn_stage_haplotype_windows(h, *args, 0, B, 0, stream) == L_.E_ARG
    hp.alt_bytes, hp.n_index = len(tab["alt"]), -1
    assert lib.explainn_stage_haplotype_windows(h, *args, 0, B, 0, stream) == L_.E_ARG
    again, f6 = staged(tab)
    assert f6 == 0 and torch.equal(again, clean)


# ---- explainn_score_haplotypes --------------------------------------------------------------------

def test_score_haplotypes_entry_point():
    """130 rows at max_batch 64: three passes, the last ragged; argument errors leave the context usable."""
    L_ = _lib()
    U, T, R, SB = 8, 2, 130, 64
    sd = _sd(U, K0, L0, T, seed=11)
    seq = sm.random_codes(SEQ_LEN, seed=12, n_runs=5)
    cases = hm.run_cases(seq, L0, seed=3)
    tab = hm.tables_from_runs(cases, R)
    mat = hm.cases_matrix(seq, cases, R, L0)
    m = _eval_model(sd, U, K0, L0, T)
    ctx, ps, keep, stream = _ctx(m, SB)
    h, lib = ctx.handle, ctx.lib
    assert ctx.max_batch == SB
    seq_d = torch.from_numpy(seq).cuda()
    hp, alive = _haps(tab)
    want_l, want_o = torch.empty(R, T, device="cuda"), torch.empty(R, U, device="cuda")
    for r0 in range(0, R, 50):                       # (other sub-batches than the entry point's own)
        n = min(50, R - r0)
        mat_d = torch.from_numpy(mat[r0:r0 + n]).cuda()
        lg, ou = _staged(m, ctx, ps, stream, n, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), n, 0, stream))
        want_l[r0:r0 + n], want_o[r0:r0 + n] = lg, ou

    def run(logits, outs, rc=0):
        return lib.explainn_score_haplotypes(h, seq_d.data_ptr(), len(seq), C.byref(hp), R, rc, C.byref(ps),
                                             logits.data_ptr() if logits is not None else None,
                                             outs.data_ptr() if outs is not None else None, stream)

    lg, ou = torch.zeros(R, T, device="cuda"), torch.zeros(R, U, device="cuda")
    L_.check(run(lg, ou))
    torch.cuda.synchronize()
    assert torch.equal(lg, want_l) and torch.equal(ou, want_o)
    # it leaves no staged batch behind
    assert lib.explainn_forward_eval(h, None, R % SB, C.byref(ps), lg.data_ptr(), stream) == L_.E_STATE
    lg2, ou2 = torch.zeros(R, T, device="cuda"), torch.zeros(R, U, device="cuda")
    L_.check(run(lg2, None))
    L_.check(run(None, ou2))
    torch.cuda.synchronize()
    assert torch.equal(lg2, want_l) and torch.equal(ou2, want_o)
    assert run(None, None) == L_.E_ARG
    L_.check(run(lg2, ou2, rc=1))                    # ... and the next call works
    torch.cuda.synchronize()
    close(to_np(lg2), _oracle_logits(sd, sm.rc_rows(mat)), TOL, "rc logits")
    L_.check(lib.explainn_dense_input(h, 1))
    assert run(lg, ou) == L_.E_UNSUPPORTED
    L_.check(lib.explainn_dense_input(h, 0))
    L_.check(run(lg, ou))
    torch.cuda.synchronize()
    assert torch.equal(lg, want_l) and torch.equal(ou, want_o)
    assert _flags(ctx, stream) == 0


# ---- score_haplotypes against predict() and the oracle --------------------------------------------

def _haplotype_problem(seed, n=90):
    seq = sm.random_codes(2000, seed=seed, n_runs=5)
    pos, ref_len, alts = hm.spaced_variants(seq, n, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    haps = [rng.permutation(n)[:c] for c in (n // 2, n, 3, 0)]
    starts = np.array([int(pos[n // 4]) - 60, int(pos[n // 2]) + 1, -30, len(seq) - 150, int(pos[2 * n // 3])])
    return seq, pos, ref_len, alts, haps, starts


def _windows(seq, pos, ref_len, alts, haps, starts, L):
    return np.stack([hm.carried_window(seq, s, pos, ref_len, alts, h, L) for h in haps for s in starts])


def test_score_haplotypes_equals_predict():
    from explainn_amd.predict import predict
    from explainn_amd.variants import score_haplotypes
    U, T = 12, 2
    sd = _sd(U, K0, L0, T, seed=70)
    seq, pos, ref_len, alts, haps, starts = _haplotype_problem(71)
    H, R = len(haps), len(starts)
    m = _eval_model(sd, U, K0, L0, T)
    # several chunks, several sub-batches per chunk; the reference rows in two chunks
    res = score_haplotypes(m, seq, pos, ref_len, alts, haps, starts, batch_size=3, chunk_rows=4, unit_effects=True)
    mat = _windows(seq, pos, ref_len, alts, haps, starts, L0)
    ref_mat = _windows(seq, pos, ref_len, alts, [[]], starts, L0)
    assert res["hap"].shape == (H, R, T, 4) and res["ref"].shape == (R, T, 4) and res["delta"].shape == (H, R, T)
    assert res["straddling"].shape == (H, R)
    for name, rows in (("hap", mat), ("ref", ref_mat)):
        want = predict(m, rows).reshape(res[name].shape)
        print("%s: max|score_haplotypes - predict| = %.3e" % (name, np.abs(res[name] - want).max()))
        assert np.array_equal(res[name], want), name
        flat = res[name].reshape(len(rows), T, 4)
        close(flat[..., 0], _oracle_logits(sd, rows), TOL, name + " fwd vs oracle")
        close(flat[..., 1], _oracle_logits(sd, sm.rc_rows(rows)), TOL, name + " rev vs oracle")
    assert np.array_equal(res["delta"], res["hap"][..., 2] - res["ref"][None, ..., 2])
    assert np.abs(res["delta"][:2]).max() > 1e-3 and np.array_equal(res["hap"][3], res["ref"])
    assert res["units"].shape == (H, R, U, T) and res["units"].dtype == np.float32
    close(res["units"].astype(np.float64).sum(2), res["delta"], TOL, "units.sum(2) vs delta")
    # one chunk, one sub-batch, a device-resident sequence: the same bits
    whole = score_haplotypes(m, torch.from_numpy(seq).cuda(), pos, ref_len, alts, haps, starts)
    assert "units" not in whole
    assert np.array_equal(whole["hap"], res["hap"]) and np.array_equal(whole["ref"], res["ref"])
    fwd = score_haplotypes(m, seq, pos, ref_len, alts, haps, starts, strands="fwd", chunk_rows=7)
    assert np.array_equal(fwd["hap"][..., 0], res["hap"][..., 0]) and np.isnan(fwd["hap"][..., 1:]).all()
    assert np.array_equal(fwd["delta"], fwd["hap"][..., 0] - fwd["ref"][None, ..., 0])
    refs = [seq[p:p + r].copy() for p, r in zip(pos, ref_len)]
    ok = score_haplotypes(m, seq, pos, ref_len, alts, haps, starts, check_ref=refs)
    assert np.array_equal(ok["hap"], res["hap"])
    v = next(i for i, r in enumerate(ref_len) if r >= 3)
    refs[v][1] = (refs[v][1] + 1) % 4
    with pytest.raises(ValueError, match="#%d at %d" % (v, pos[v])):
        score_haplotypes(m, seq, pos, ref_len, alts, haps, starts, check_ref=refs)
    with pytest.raises(ValueError, match="outside the sequence"):
        score_haplotypes(m, seq, [len(seq) - 1], [2], [np.zeros(1, np.uint8)], [[0]], starts)
    empty = score_haplotypes(m, seq, pos, ref_len, alts, [], starts, unit_effects=True)
    assert empty["hap"].shape == (0, R, T, 4) and empty["ref"].shape == (R, T, 4)
    assert empty["units"].shape == (0, R, U, T) and np.array_equal(empty["ref"], res["ref"])


def test_score_haplotypes_on_a_bank():
    from explainn_amd import ExplaiNNBank
    from explainn_amd.variants import score_haplotypes
    G, U, T = 2, 8, 2
    sds = [_sd(U, K0, L0, T, seed=80 + g) for g in range(G)]
    bank = ExplaiNNBank.from_models([model(sd, U, K0, L0, T) for sd in sds]).cuda().eval()
    bank.validate_input = False
    seq, pos, ref_len, alts, haps, starts = _haplotype_problem(81, n=60)
    H, R = len(haps), len(starts)
    res = score_haplotypes(bank, seq, pos, ref_len, alts, haps, starts, unit_effects=True, batch_size=8, chunk_rows=9)
    assert res["hap"].shape == (H, R, G, T, 4) and res["ref"].shape == (R, G, T, 4)
    assert res["delta"].shape == (H, R, G, T) and res["units"].shape == (H, R, G * U, T)
    for g in range(G):
        mem = bank.member(g).eval()
        mem.validate_input = False
        one = score_haplotypes(mem, seq, pos, ref_len, alts, haps, starts, unit_effects=True)
        close(res["hap"][:, :, g], one["hap"], TOL, "bank member %d hap" % g)
        close(res["ref"][:, g], one["ref"], TOL, "bank member %d ref" % g)
        close(res["delta"][:, :, g], one["delta"], TOL, "bank member %d delta" % g)
        close(res["units"][:, :, g * U:(g + 1) * U], one["units"], TOL, "bank member %d units" % g)
