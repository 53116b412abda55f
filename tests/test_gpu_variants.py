"""Variant effects on the device: explainn_stage_edited_windows, explainn_score_edits and
explainn_amd.variants.  -m gpu.  Every case runs once.

What is compared with what:
  * explainn_stage_edited_windows against explainn_stage_codes on the (B,L) matrix the numpy haplotype
    model builds by concatenation (tests/variants_model.py): the eval logits of the staged batch,
    torch.equal; one train step's gradients at GRAD_TOL_GOLDEN (that pins bm);
  * explainn_score_edits against row-by-row staging plus explainn_forward_eval / explainn_unit_outputs,
    torch.equal;
  * score_variants against predict() on the host-materialised ref and alt windows: np.array_equal on
    all four columns -- exact because the staged batch is the same bytes and fc_fwd and the head treat
    sequences independently;
  * independently, the same outputs and the unit effects against the fp64 oracle at TOL (1e-4 absolute,
    the project's logit tolerance).
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import GRAD_TOL_GOLDEN, TOL, close, close_rel, model, to_np  # noqa: E402
import scan_model as sm  # noqa: E402
import variants_model as vm  # noqa: E402

pytestmark = pytest.mark.gpu


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
    out = []
    for i in range(0, len(mat), 256):
        out.append(orc.forward(sd, sm.onehot(mat[i:i + 256]), dtype=np.float64))
    return np.concatenate(out)


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


def _staged_logits(m, ctx, ps, stream, B, stage):
    lib = ctx.lib
    logits = torch.empty(B, m._options["n_features"], device="cuda")
    _lib().check(stage())
    _lib().check(lib.explainn_forward_eval(ctx.handle, None, B, C.byref(ps), logits.data_ptr(), stream))
    torch.cuda.synchronize()
    return logits


def _flags(ctx, stream):
    flags = C.c_int(0)
    _lib().check(ctx.lib.explainn_input_flags(ctx.handle, C.byref(flags), stream))
    return flags.value


def _edits(tab):
    """explainn_edits of numpy tables: (struct, the device tensors that keep it alive)."""
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in tab.items()}
    ed = _lib().Edits()
    for k, t in dev.items():
        setattr(ed, k, t.data_ptr() if t.numel() else None)
    ed.n_edits, ed.alt_bytes = len(tab["pos"]), len(tab["alt"])
    return ed, dev


L0, K0 = 200, 19
SEQ_LEN = 1000


# ---- explainn_stage_edited_windows ----------------------------------------------------------------

@pytest.mark.parametrize("rc", [0, 1])
@pytest.mark.parametrize("L,k,B,first", [(L0, K0, 1, 0), (L0, K0, 64, 0), (L0, K0, 65, 5), (40, 5, 65, 0)])
def test_stage_edited_windows_equals_stage_codes(L, k, B, first, rc):
    """Every edit class of variants_model.edit_cases, whole and ragged 64-row tiles, both strands; at
    L = 40 the row is shorter than a position tile."""
    U, T = 8, 2
    seq = sm.random_codes(SEQ_LEN, seed=L + B, n_runs=6)
    cases = vm.edit_cases(seq, L, seed=B)
    tab = vm.tables_from_cases(cases, B, first)
    mat = vm.cases_matrix(seq, cases, B, L, first)
    sd = _sd(U, k, L, T, seed=3)
    m = _eval_model(sd, U, k, L, T)
    ctx, ps, keep, stream = _ctx(m, B)
    h, lib = ctx.handle, ctx.lib
    seq_d, mat_d = torch.from_numpy(seq).cuda(), torch.from_numpy(mat).cuda()
    ed, alive = _edits(tab)
    a = _staged_logits(m, ctx, ps, stream, B, lambda: lib.explainn_stage_edited_windows(
        h, seq_d.data_ptr(), len(seq), C.byref(ed), 0, B, rc, stream))
    assert _flags(ctx, stream) == 0, "N padding, N in alt and N in seq must not raise the flag"
    b = _staged_logits(m, ctx, ps, stream, B, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), B, rc, stream))
    assert torch.equal(a, b), float((a - b).abs().max())
    close(to_np(a), _oracle_logits(sd, sm.rc_rows(mat) if rc else mat), TOL, "stage_edited_windows logits")
    if B == 65:
        # row0: the last 20 rows of the same tables are rows 45.. of the matrix
        c = _staged_logits(m, ctx, ps, stream, 20, lambda: lib.explainn_stage_edited_windows(
            h, seq_d.data_ptr(), len(seq), C.byref(ed), 45, 20, rc, stream))
        assert torch.equal(c, a[45:])


def test_stage_edited_windows_flags():
    U, T, B = 8, 1, 64
    seq = sm.random_codes(SEQ_LEN, seed=1, n_runs=3)
    sd = _sd(U, K0, L0, T, seed=4)
    m = _eval_model(sd, U, K0, L0, T)
    ctx, ps, keep, stream = _ctx(m, B)
    h, lib = ctx.handle, ctx.lib
    cases = [c for c in vm.edit_cases(seq, L0) if c[1] is not None]
    tab = vm.tables_from_cases(cases, B)
    seq_d = torch.from_numpy(seq).cuda()

    def staged(t, s_d=seq_d):
        ed, alive = _edits(t)
        out = _staged_logits(m, ctx, ps, stream, B, lambda: lib.explainn_stage_edited_windows(
            h, s_d.data_ptr(), len(seq), C.byref(ed), 0, B, 0, stream))
        return out, _flags(ctx, stream)

    clean, f0 = staged(tab)
    assert f0 == 0
    # a byte 9 in alt, at a position a row reads: the flag, and the logits of an N there
    e0 = int(tab["row_edit"][0])                     # row 0: alt_len 70, the window is centred on it
    at = int(tab["alt_off"][e0]) + 35
    bad, asn = dict(tab), dict(tab)
    bad["alt"], asn["alt"] = tab["alt"].copy(), tab["alt"].copy()
    bad["alt"][at], asn["alt"][at] = 9, 4
    got, f1 = staged(bad)
    want, f2 = staged(asn)
    assert f1 & 1 and f2 == 0
    assert torch.equal(got, want) and not torch.equal(got[0], clean[0])
    # a byte 9 in seq inside a row
    seq9 = seq.copy()
    seq9[SEQ_LEN // 2 - 30] = 9
    _, f3 = staged(tab, torch.from_numpy(seq9).cuda())
    assert f3 & 1
    # a row whose edit index is past the table: flagged, the run completes, the row reads as N
    wild = dict(tab)
    wild["row_edit"] = tab["row_edit"].copy()
    wild["row_edit"][5] = len(tab["pos"])
    wild["row_edit"][6] = 2 ** 31 - 1
    got, f4 = staged(wild)
    assert f4 & 1 and torch.isfinite(got).all()
    mat = vm.cases_matrix(seq, cases, B, L0)
    mat[5:7] = 4
    mat_d = torch.from_numpy(mat).cuda()
    want = _staged_logits(m, ctx, ps, stream, B, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), B, 0, stream))
    assert torch.equal(got, want)
    # a negative length and an alt run that leaves the pool: the same
    for field, value in (("ref_len", -1), ("alt_len", -3), ("alt_off", len(tab["alt"]) - 1), ("alt_off", -1)):
        t = dict(tab)
        t[field] = tab[field].copy()
        e = int(tab["row_edit"][5])
        if field == "alt_off" and value > 0:
            assert tab["alt_len"][e] > 1
        t[field][e] = value
        got, f = staged(t)
        assert f & 1, field
        assert torch.equal(got[5], want[5]) and torch.equal(got[7:], clean[7:]), field
    # and the context is usable afterwards
    again, f5 = staged(tab)
    assert f5 == 0 and torch.equal(again, clean)
    # argument checks leave the context usable too
    ed, alive = _edits(tab)
    L_ = _lib()
    assert lib.explainn_stage_edited_windows(h, seq_d.data_ptr(), len(seq), C.byref(ed), 0, B + 1, 0, stream) == L_.E_ARG
    assert lib.explainn_stage_edited_windows(h, None, len(seq), C.byref(ed), 0, B, 0, stream) == L_.E_ARG
    assert lib.explainn_stage_edited_windows(h, seq_d.data_ptr(), len(seq), C.byref(ed), -1, B, 0, stream) == L_.E_ARG
    ed.alt_bytes = 2 ** 31
    assert lib.explainn_stage_edited_windows(h, seq_d.data_ptr(), len(seq), C.byref(ed), 0, B, 0, stream) == L_.E_ARG


def _grads_struct(m):
    L_ = _lib()
    g = L_.Grads()
    sd = dict(m.state_dict())
    keep = {}
    for f in L_.GRAD_FIELDS:
        keep[f] = torch.zeros_like(sd[L_.PARAM_KEYS[f]]).contiguous()
        setattr(g, f, keep[f].data_ptr())
    return g, keep


def test_stage_edited_windows_train_step_gradients():
    """A staged edited batch feeds a train step like a staged code matrix: same keep mask, same
    gradients (bit equality expected; the claim is GRAD_TOL_GOLDEN)."""
    U, T, B = 8, 2, 65
    sd = _sd(U, K0, L0, T, seed=6)
    seq = sm.random_codes(SEQ_LEN, seed=8, n_runs=4)
    cases = vm.edit_cases(seq, L0, seed=2)
    tab = vm.tables_from_cases(cases, B, 3)
    mat = vm.cases_matrix(seq, cases, B, L0, 3)
    rng = np.random.default_rng(9)
    keep_mask = torch.from_numpy((rng.random((B, 100 * U)) > 0.3).astype(np.uint8)).cuda()
    y = torch.from_numpy((rng.random((B, T)) > 0.5).astype(np.float32)).cuda()
    seq_d, mat_d = torch.from_numpy(seq).cuda(), torch.from_numpy(mat).cuda()
    ed, alive = _edits(tab)
    results = []
    for which in ("edits", "codes"):
        m = model(sd, U, K0, L0, T).train()
        ctx, ps, keepalive, stream = _ctx(m, B)
        h, lib = ctx.handle, ctx.lib
        g, gk = _grads_struct(m)
        logits = torch.empty(B, T, device="cuda")
        dl = torch.empty(B, T, device="cuda")
        loss = torch.empty(1, device="cuda")
        if which == "edits":
            _lib().check(lib.explainn_stage_edited_windows(h, seq_d.data_ptr(), len(seq), C.byref(ed), 0, B, 1, stream))
        else:
            _lib().check(lib.explainn_stage_codes(h, mat_d.data_ptr(), B, 1, stream))
        _lib().check(lib.explainn_forward_train(h, None, B, C.byref(ps), keep_mask.data_ptr(), 0.3, 0,
                                               logits.data_ptr(), stream))
        _lib().check(lib.explainn_loss_grad(h, 0, logits.data_ptr(), y.data_ptr(), B, loss.data_ptr(),
                                           dl.data_ptr(), stream))
        _lib().check(lib.explainn_backward(h, dl.data_ptr(), B, C.byref(ps), C.byref(g), 0, stream))
        torch.cuda.synchronize()
        results.append((logits, gk))
    (la, ga), (lb, gb) = results
    close(to_np(la), to_np(lb), TOL, "train logits, staged edits vs staged codes")
    for f in ga:
        close_rel(to_np(ga[f]), to_np(gb[f]), tol=GRAD_TOL_GOLDEN, what="staged edits grad " + f)
        print("grad %-8s bit-equal: %s" % (f, torch.equal(ga[f], gb[f])))


# ---- explainn_score_edits -------------------------------------------------------------------------

def test_score_edits_equals_row_by_row_staging():
    """150 rows at max_batch 64: three passes, the last ragged."""
    L_ = _lib()
    U, T, R, SB = 8, 2, 150, 64
    sd = _sd(U, K0, L0, T, seed=11)
    seq = sm.random_codes(SEQ_LEN, seed=12, n_runs=5)
    cases = vm.edit_cases(seq, L0, seed=3)
    tab = vm.tables_from_cases(cases, R)
    m = _eval_model(sd, U, K0, L0, T)
    ctx, ps, keep, stream = _ctx(m, SB)
    h, lib = ctx.handle, ctx.lib
    assert ctx.max_batch == SB
    seq_d = torch.from_numpy(seq).cuda()
    ed, alive = _edits(tab)
    want_l = torch.empty(R, T, device="cuda")
    want_o = torch.empty(R, U, device="cuda")
    for r0 in range(0, R, 50):                       # (other sub-batches than the entry point's own)
        for fn, out, w in ((lib.explainn_forward_eval, want_l, T), (lib.explainn_unit_outputs, want_o, U)):
            L_.check(lib.explainn_stage_edited_windows(h, seq_d.data_ptr(), len(seq), C.byref(ed), r0, 50, 0, stream))
            L_.check(fn(h, None, 50, C.byref(ps), out.data_ptr() + 4 * w * r0, stream))
    torch.cuda.synchronize()
    close(to_np(want_l), _oracle_logits(sd, vm.cases_matrix(seq, cases, R, L0)), TOL, "row-by-row logits")

    def run(logits, outs, rc=0):
        return lib.explainn_score_edits(h, seq_d.data_ptr(), len(seq), C.byref(ed), R, rc, C.byref(ps),
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
    close(to_np(lg2), _oracle_logits(sd, sm.rc_rows(vm.cases_matrix(seq, cases, R, L0))), TOL, "rc logits")
    L_.check(lib.explainn_dense_input(h, 1))
    assert run(lg, ou) == L_.E_UNSUPPORTED
    L_.check(lib.explainn_dense_input(h, 0))
    L_.check(run(lg, ou))
    torch.cuda.synchronize()
    assert torch.equal(lg, want_l) and torch.equal(ou, want_o)
    assert _flags(ctx, stream) == 0


# ---- score_variants against predict() and the oracle ----------------------------------------------

SHIFTS = (0, 3, 6)


@pytest.mark.parametrize("U,T", [(3, 1), (100, 3)])
def test_score_variants_equals_predict(U, T):
    from explainn_amd.predict import predict
    from explainn_amd.variants import score_variants
    sd = _sd(U, K0, L0, T, seed=U + T)
    seq = sm.random_codes(3000, seed=U, n_runs=8)
    pos, ref_len, alts = vm.mixed_variants(seq, 40, L0, seed=T)
    m = _eval_model(sd, U, K0, L0, T)
    # several chunks (7 variants each), several sub-batches per chunk
    res = score_variants(m, seq, pos, ref_len, alts, shifts=SHIFTS, batch_size=16, chunk_rows=45)
    ref_mat, alt_mat = vm.allele_matrices(seq, pos, ref_len, alts, L0, SHIFTS)
    V, S = len(pos), len(SHIFTS)
    assert res["ref"].shape == res["alt"].shape == (V, S, T, 4) and res["delta"].shape == (V, T)
    for name, mat in (("ref", ref_mat), ("alt", alt_mat)):
        want = predict(m, mat).reshape(V, S, T, 4)
        print("%s: max|score_variants - predict| = %.3e" % (name, np.abs(res[name] - want).max()))
        assert np.array_equal(res[name], want), name
        close(res[name][..., 0].reshape(V * S, T), _oracle_logits(sd, mat), TOL, name + " fwd vs oracle")
        close(res[name][..., 1].reshape(V * S, T), _oracle_logits(sd, sm.rc_rows(mat)), TOL, name + " rev vs oracle")
    assert np.array_equal(res["delta"], (res["alt"][..., 2] - res["ref"][..., 2]).mean(axis=1))
    assert np.abs(res["delta"]).max() > 1e-3
    # one chunk, one sub-batch, a device-resident sequence: the same bits
    whole = score_variants(m, torch.from_numpy(seq).cuda(), pos, ref_len, alts, shifts=SHIFTS)
    assert np.array_equal(whole["ref"], res["ref"]) and np.array_equal(whole["alt"], res["alt"])
    if U == 3:
        fwd = score_variants(m, seq, pos, ref_len, alts, shifts=SHIFTS, strands="fwd", chunk_rows=100)
        assert np.array_equal(fwd["ref"][..., 0], res["ref"][..., 0]) and np.isnan(fwd["alt"][..., 1:]).all()
        assert np.array_equal(fwd["delta"], (fwd["alt"][..., 0] - fwd["ref"][..., 0]).mean(axis=1))
        sig = score_variants(m, seq, pos, ref_len, alts, shifts=SHIFTS, apply_sigmoid=True)
        close(sig["alt"], 1 / (1 + np.exp(-res["alt"])), 1e-6, "apply_sigmoid")
        # REF alleles: the sequence's own pass, one wrong base raises
        refs = [seq[p:p + r].copy() for p, r in zip(pos, ref_len)]
        ok = score_variants(m, seq, pos, ref_len, alts, shifts=SHIFTS, check_ref=refs)
        assert np.array_equal(ok["alt"], res["alt"])
        v = next(i for i, r in enumerate(ref_len) if r >= 3)
        refs[v][1] = (refs[v][1] + 1) % 4
        with pytest.raises(ValueError, match="#%d at %d" % (v, pos[v])):
            score_variants(m, seq, pos, ref_len, alts, shifts=SHIFTS, check_ref=refs)
        empty = score_variants(m, seq, [], [], [], shifts=SHIFTS, unit_effects=True)
        assert empty["ref"].shape == (0, S, T, 4) and empty["delta"].shape == (0, T)
        assert empty["units"].shape == (0, U, T)
        for bad_pos, bad_len in ((-1, 1), (len(seq) - 1, 2)):
            with pytest.raises(ValueError, match="outside the sequence"):
                score_variants(m, seq, [bad_pos], [bad_len], [np.zeros(1, np.uint8)])


@pytest.mark.parametrize("U,T", [(3, 3), (100, 1)])
def test_unit_effects_against_oracle(U, T):
    from explainn_amd.variants import score_variants
    sd = _sd(U, K0, L0, T, seed=50 + U)
    seq = sm.random_codes(2000, seed=51, n_runs=5)
    pos, ref_len, alts = vm.mixed_variants(seq, 12, L0, seed=52)
    m = _eval_model(sd, U, K0, L0, T)
    res = score_variants(m, seq, pos, ref_len, alts, shifts=SHIFTS, unit_effects=True, batch_size=32, chunk_rows=30)
    ref_mat, alt_mat = vm.allele_matrices(seq, pos, ref_len, alts, L0, SHIFTS)
    units, delta, _ = vm.oracle_effects(orc, sd, ref_mat, alt_mat, len(pos), len(SHIFTS))
    assert res["units"].shape == units.shape and res["units"].dtype == np.float32
    close(res["units"], units, TOL, "unit effects vs oracle")
    close(res["units"].astype(np.float64).sum(1), delta, TOL, "units.sum(1) vs the oracle's delta")
    close(res["delta"], delta, TOL, "delta vs oracle")
    plain = score_variants(m, seq, pos, ref_len, alts, shifts=SHIFTS)
    assert "units" not in plain and np.array_equal(plain["alt"], res["alt"])


def test_score_variants_bank_equals_members():
    from explainn_amd import ExplaiNNBank
    from explainn_amd.variants import score_variants
    G, U, T = 3, 8, 2
    sds = [_sd(U, K0, L0, T, seed=40 + g) for g in range(G)]
    bank = ExplaiNNBank.from_models([model(sd, U, K0, L0, T) for sd in sds]).cuda().eval()
    bank.validate_input = False
    seq = sm.random_codes(2000, seed=41, n_runs=4)
    pos, ref_len, alts = vm.mixed_variants(seq, 15, L0, seed=42)
    res = score_variants(bank, seq, pos, ref_len, alts, shifts=SHIFTS, unit_effects=True, batch_size=40, chunk_rows=60)
    V, S = len(pos), len(SHIFTS)
    assert res["ref"].shape == (V, S, G, T, 4) and res["delta"].shape == (V, G, T)
    assert res["units"].shape == (V, G * U, T)
    for g in range(G):
        mem = bank.member(g).eval()
        mem.validate_input = False
        one = score_variants(mem, seq, pos, ref_len, alts, shifts=SHIFTS, unit_effects=True)
        for key in ("ref", "alt", "delta"):
            close(res[key][:, :, g] if key != "delta" else res[key][:, g], one[key], TOL,
                  "bank member %d %s" % (g, key))
        close(res["units"][:, g * U:(g + 1) * U], one["units"], TOL, "bank member %d units" % g)


# ---- the command line -----------------------------------------------------------------------------

def test_variants_cli(tmp_path):
    from explainn_amd import variants
    U, T = 6, 2
    sd = _sd(U, K0, L0, T, seed=60)
    m = _eval_model(sd, U, K0, L0, T)
    ckpt = str(tmp_path / "m.pt")
    torch.save({"options": dict(m._options), "state_dict": {key: v.cpu() for key, v in m.state_dict().items()}}, ckpt)
    recs = {"chrA": sm.random_codes(700, seed=61), "chrB": sm.random_codes(450, seed=62)}
    letters = np.array(list("ACGTN"))
    fa = tmp_path / "g.fa"
    with open(fa, "w") as fh:
        for rid, codes in recs.items():
            s = "".join(letters[codes])
            fh.write(">%s some description\n" % rid)
            fh.writelines(s[i:i + 60] + "\n" for i in range(0, len(s), 60))

    def ref(rid, pos1, n):
        return "".join(letters[recs[rid][pos1 - 1:pos1 - 1 + n]])

    def other(base):
        return "ACGT"[("ACGT".find(base) + 1) % 4]

    a, b, c = ref("chrA", 300, 1), ref("chrB", 200, 3), ref("chrA", 650, 2)
    vcf = tmp_path / "v.vcf"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n"
                   "chrA\t300\tsnv\t%s\t%s\n" % (a, other(a)) +
                   "chrB\t200\tmulti\t%s\t%s,%sacgtt\n" % (b, b[0], b.lower()) +
                   "chrA\t650\tsym\t%s\t<DEL>\n" % c[0] +
                   "chrA\t650\tdel\t%s\t%s\n" % (c, c[0]))
    out = tmp_path / "o.tsv"
    variants.main([ckpt, str(fa), str(vcf), "-o", str(out), "--shifts", "2", "--top-units", "3"])
    rows = [line.rstrip("\n").split("\t") for line in open(out)]
    assert rows[0] == ["Chrom", "Pos", "Id", "Ref", "Alt", "Class", "RefFwd", "RefRev", "RefMean", "AltFwd",
                       "AltRev", "AltMean", "Delta", "Units"]
    body = rows[1:]
    assert [tuple(r[:6]) for r in body] == [
        (ch, str(p), i, r, al, str(t)) for ch, p, i, r, al in (
            ("chrA", 300, "snv", a, other(a)), ("chrB", 200, "multi", b, b[0]),
            ("chrB", 200, "multi", b, b.lower() + "acgtt"), ("chrA", 650, "del", c, c[0])) for t in range(T)]
    code = {ch: i for i, ch in enumerate("ACGT")}
    enc = lambda s: np.array([code[x] for x in s.upper()], dtype=np.uint8)
    resA = variants.score_variants(m, recs["chrA"], [299, 649], [1, 2], [enc(other(a)), enc(c[0])],
                                   shifts=(0, 1), unit_effects=True)
    resB = variants.score_variants(m, recs["chrB"], [199, 199], [3, 3], [enc(b[0]), enc(b + "acgtt")],
                                   shifts=(0, 1), unit_effects=True)
    want = [(resA, 0), (resB, 0), (resB, 1), (resA, 1)]
    for i, (res, j) in enumerate(want):
        for t in range(T):
            r = body[i * T + t]
            assert float(r[12]) == res["delta"][j, t]
            got = [float(x) for x in r[6:12]]
            exp = list(res["ref"][j].mean(axis=0)[t, :3]) + list(res["alt"][j].mean(axis=0)[t, :3])
            assert got == [float(x) for x in exp]
            top = [(int(u), float(e)) for u, e in (item.split(":") for item in r[13].split(","))]
            eff = res["units"][j, :, t]
            assert len(top) == 3 and [u for u, _ in top] == list(np.argsort(-np.abs(eff), kind="stable")[:3])
            assert [e for _, e in top] == [float(eff[u]) for u, _ in top]
    # a REF allele that is not the sequence's: refused unless --no-check-ref
    vcf.write_text("#CHROM\tPOS\tID\tREF\tALT\nchrA\t300\tsnv\t%s\t%s\n" % (other(a), a))
    with pytest.raises(ValueError, match="REF allele"):
        variants.main([ckpt, str(fa), str(vcf), "-o", str(out)])
    variants.main([ckpt, str(fa), str(vcf), "-o", str(out), "--no-check-ref", "--shifts", "1", "--strands", "fwd"])
    rows = [line.rstrip("\n").split("\t") for line in open(out)]
    assert len(rows) == 1 + T and rows[1][7] == "nan"
