"""The model bank (ExplaiNNBank / explainn_create_bank) on the device.  The reference is never the
code under test: the fp64 oracle member by member, or the existing single-model path on
bank.member(g).  Bounds are the suite's own (parity_util).

Head routes of a bank (csrc/head.hip, DESIGN.md section 8 "Model bank"): the one head, with the
member index taken at run time (a stand-alone model is the bank of one)
  forward   train, T <= 8 and a member's statistics fit LDS: logits_bn_kernel (one launch);
            otherwise head_fwd_train + logits_kernel (also T > 8: no GEMM form); eval: logits_kernel
  backward  StepEngine, T <= 4: head_bwd_kernel<true, false> (loss recomputed inside: no "loss" stage);
            StepEngine, T > 4: bank_loss_kernel ("loss" stage) + head_bwd_kernel<false, false>;
            autograd (dlogits given): head_bwd_kernel<false, false>.  A bank never rides in passA.
-m gpu."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import record_margin  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import (GRAD_TOL_GOLDEN, TOL, check_grads, close, close_rel, model, oracle_step,  # noqa: E402
                         to_np)

pytestmark = pytest.mark.gpu

Case = namedtuple("Case", "name G U k L T B kind freeze n_frac codes masked")
CASES = [
    # T = 1, B = 100 (a single model rides in passA here; the bank: logits_bn + fused-loss head_bwd)
    Case("t1_b100", 2, 8, 19, 200, 1, 100, "binary", 0, 0.0, False, True),
    # T = 1, B = 1024, members straddle the 32-unit tiles, N bases, frozen filters: logits_bn + fused loss
    Case("t1_b1024_u33", 3, 33, 19, 200, 1, 1024, "binary", 3, 0.01, False, True),
    # T = 3, B = 600, short filters, MSE: logits_bn + fused loss
    Case("t3_b600_k4", 3, 8, 4, 60, 3, 600, "linear", 0, 0.0, False, True),
    # T = 6, B = 600: logits_bn, bank_loss_kernel + head_bwd<false, false>
    Case("t6_b600", 2, 33, 19, 200, 6, 600, "binary", 0, 0.0, False, True),
    # T = 50, B = 256 (a single model takes the GEMMs): head_fwd_train + logits_kernel, bank_loss + head_bwd<false, false>
    Case("t50_b256", 10, 8, 19, 200, 50, 256, "binary", 0, 0.0, False, True),
    # base codes read as their reverse complement
    Case("codes_rc", 2, 8, 19, 200, 1, 100, "binary", 3, 0.01, True, True),
]


def _member_sd(c, g):
    rng = np.random.default_rng(1000 * c.G + 17 * g + c.T)
    sd = orc.random_state_dict(c.U, c.k, c.L, c.T, seed=100 + 7 * g + c.B)
    # |gamma1| bounded away from zero, half of them negative (tests/test_gpu_dispatch_sweep.py: a unit
    # with gamma1 ~ 0 has ill-conditioned gradients in fp32 whatever the summation order)
    sd["linears.1.weight"] = (rng.uniform(0.6, 1.4, c.U) * np.where(np.arange(c.U) % 2, 1, -1)).astype(np.float32)
    return sd


def _bank(c, sds):
    from explainn_amd import ExplaiNNBank
    bank = ExplaiNNBank.from_models([model(sd, c.U, c.k, c.L, c.T) for sd in sds]).cuda().train()
    bank.freeze_top_n_filters = c.freeze
    return bank


def _batch(c):
    rng = np.random.default_rng(c.B + c.T)
    x = orc.random_onehot(c.B, c.L, seed=c.B + 3, n_frac=c.n_frac)
    if c.kind == "binary":
        y = (rng.random((c.B, c.T)) > 0.5).astype(np.float32)
    else:
        y = rng.normal(size=(c.B, c.T)).astype(np.float32)
    return x, y


def _device_x(c, x):
    """(what the bank gets, the one-hot the model then runs on)"""
    from explainn_amd.architectures import BaseCodes
    if not c.codes:
        return torch.from_numpy(x).cuda(), x
    codes = x.argmax(axis=1).astype(np.uint8)
    codes[x.sum(axis=1) == 0] = 4
    return BaseCodes(torch.from_numpy(codes).cuda(), True), np.ascontiguousarray(x[:, ::-1, ::-1])


def _member_grads(bank, grads, g):
    return [(name, bank._member_view(name, gr, g)) for (name, _), gr in zip(bank.named_parameters(), grads)]


def _check_member_vs_oracle(c, label, bank, g, sd, x_run, y, keep_g, logits, loss, grads):
    ref_logits, ref_loss, ref_grads, nb = oracle_step(sd, x_run, y, freeze=c.freeze, keep=keep_g, kind=c.kind)
    close(to_np(logits[:, g]), ref_logits, what=label + " logits")
    if loss is not None:
        close(float(loss[g]), float(ref_loss), what=label + " loss")
    check_grads(_member_grads(bank, grads, g), ref_grads, label + " ")
    bufs = dict(bank.named_buffers())
    for key, v in nb.items():
        if "tracked" in key:
            assert int(bufs[key].item()) == int(v), key
        else:
            close_rel(to_np(bank._member_view(key, bufs[key], g)), v, tol=GRAD_TOL_GOLDEN, what=label + " " + key)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_bank_step_against_oracle(c):
    """Test 5: the fused step of a bank through StepEngine (dropout off), member by member against the
    fp64 oracle on that member's state_dict and the shared batch."""
    from explainn_amd.engine import StepEngine
    sds = [_member_sd(c, g) for g in range(c.G)]
    x, y = _batch(c)
    xt, x_run = _device_x(c, x)
    bank = _bank(c, sds)
    bank.dropout_p = 0.0
    eng = StepEngine(bank, c.B, c.kind)
    eng.ctx.stage_timing(True)
    logits, loss = eng.step(xt, torch.from_numpy(y).cuda(), freeze_top_n_filters=c.freeze)
    torch.cuda.synchronize()
    stages = eng.ctx.stage_times()
    eng.ctx.stage_timing(False)
    assert "head_bwd" in stages and "head_fwd" in stages, stages        # never inside passA
    assert ("loss" in stages) == (c.T > 4), stages
    assert logits.shape == (c.B, c.G, c.T) and loss.shape == (c.G,)
    for g in range(c.G):
        _check_member_vs_oracle(c, "bank %s engine m%d" % (c.name, g), bank, g, sds[g], x_run, y, None,
                                logits, loss, eng.views)


@pytest.mark.parametrize("c", [c for c in CASES if c.masked], ids=[c.name for c in CASES if c.masked])
def test_bank_autograd_with_keep_mask_against_oracle(c):
    """Test 5, autograd path: bank(x) under an explicit keep mask (B, 100*G*U), the sum of the members'
    losses, loss.backward(); member g against the oracle with ITS slice of the mask."""
    sds = [_member_sd(c, g) for g in range(c.G)]
    x, y = _batch(c)
    xt, x_run = _device_x(c, x)
    bank = _bank(c, sds)
    keep = (np.random.default_rng(5).random((c.B, 100 * c.G * c.U)) > 0.3).astype(np.uint8)
    bank.set_dropout_mask(torch.from_numpy(keep))
    logits = bank(xt)
    assert logits.shape == (c.B, c.G, c.T)
    yt = torch.from_numpy(y).cuda()
    fn = torch.nn.functional.binary_cross_entropy_with_logits if c.kind == "binary" else torch.nn.functional.mse_loss
    losses = torch.stack([fn(logits[:, g], yt) for g in range(c.G)])
    losses.sum().backward()
    grads = [p.grad for p in bank.parameters()]
    for g in range(c.G):
        keep_g = np.ascontiguousarray(keep[:, 100 * c.U * g:100 * c.U * (g + 1)])
        _check_member_vs_oracle(c, "bank %s autograd m%d" % (c.name, g), bank, g, sds[g], x_run, y, keep_g,
                                logits.detach(), losses.detach(), grads)


def _against_member(c, label, bank, g, xt, yt, logits, loss, views):
    """Member g of a finished bank step vs StepEngine on the stand-alone model with the parameters
    and buffers the bank had BEFORE the step (`bank` here is that earlier state's copy)."""
    from explainn_amd.engine import StepEngine
    m = bank.member(g)
    m.dropout_p = 0.0
    e1 = StepEngine(m, c.B, c.kind)
    lg1, ls1 = e1.step(xt, yt, freeze_top_n_filters=c.freeze)
    torch.cuda.synchronize()
    close(to_np(logits[:, g]), to_np(lg1), what=label + " logits")
    close(float(loss[g]), float(ls1), what=label + " loss")
    worst = float((logits[:, g] - lg1).abs().max())
    for (name, _), gb, g1 in zip(bank.named_parameters(), views, e1.views):
        mine = bank._member_view(name, gb, g)
        close_rel(to_np(mine), to_np(g1), tol=GRAD_TOL_GOLDEN, what=label + " grad " + name)
        worst = max(worst, float((mine - g1).abs().max()))
    return worst, m


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_bank_step_against_single_model_path(c):
    """Test 6: the bank step vs the existing path on bank.member(g), same batch, dropout off; then the
    eval forward from the updated buffers, bank(x)[:, g] vs member(g)(x)."""
    import copy
    from explainn_amd.engine import StepEngine
    sds = [_member_sd(c, g) for g in range(c.G)]
    x, y = _batch(c)
    xt, _ = _device_x(c, x)
    yt = torch.from_numpy(y).cuda()
    bank = _bank(c, sds)
    bank.dropout_p = 0.0
    before = copy.deepcopy(bank)
    eng = StepEngine(bank, c.B, c.kind)
    logits, loss = eng.step(xt, yt, freeze_top_n_filters=c.freeze)
    torch.cuda.synchronize()
    worst = 0.0
    for g in range(c.G):
        label = "bank %s vs member %d" % (c.name, g)
        w, m = _against_member(c, label, before, g, xt, yt, logits, loss, eng.views)
        worst = max(worst, w)
        mb = dict(m.named_buffers())
        for key, v in bank.named_buffers():
            if "tracked" in key:
                assert int(v.item()) == int(mb[key].item())
            else:
                close_rel(to_np(bank._member_view(key, v, g)), to_np(mb[key]), tol=GRAD_TOL_GOLDEN,
                          what=label + " " + key)
    record_margin("bank %s vs single-model path, max |difference| over logits and gradients" % c.name, worst, TOL)
    print("bank %s vs single-model path: max |difference| %.3e" % (c.name, worst))
    bank.eval()
    with torch.no_grad():
        got = bank(xt)
        assert got.shape == (c.B, c.G, c.T)
        for g in range(c.G):
            close(to_np(got[:, g]), to_np(bank.member(g)(xt)), what="bank %s eval member %d" % (c.name, g))


def _perturbed(bank, c, seed):
    import copy
    other = copy.deepcopy(bank)
    sd = orc.random_state_dict(c.U, c.k, c.L, c.T, seed=seed)
    other.load_member(1, {key: torch.from_numpy(np.array(v)) for key, v in sd.items()})
    return other


@pytest.mark.parametrize("G,U,B,masked", [(20, 100, 100, True), (4, 300, 1024, False)])
def test_bank_members_are_independent_bitwise(G, U, B, masked):
    """Test 7: perturbing every parameter of member 1 (and its dropout-mask slice) leaves the other
    members' logits, losses and gradient slices bit-identical; two identical steps are bit-identical."""
    from explainn_amd import ExplaiNNBank
    from explainn_amd.engine import StepEngine
    c = Case("indep", G, U, 19, 200, 1, B, "binary", 0, 0.0, False, masked)
    torch.manual_seed(11)
    bank = ExplaiNNBank(G, U, 19, 200, 1).cuda().train()
    x, y = _batch(c)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    keep = None
    if masked:
        keep = (np.random.default_rng(9).random((B, 100 * G * U)) > 0.3).astype(np.uint8)

    def run(b, kp):
        if kp is None:
            e = StepEngine(b, B, "binary")
            lg, ls = e.step(xt, yt, seed=1234)       # built-in generator: keyed by the unit, so member-local
            torch.cuda.synchronize()
            return lg.clone(), ls.clone(), [v.clone() for v in e.views]
        b.zero_grad()
        b.set_dropout_mask(torch.from_numpy(kp))
        lg = b(xt)
        ls = torch.stack([torch.nn.functional.binary_cross_entropy_with_logits(lg[:, g], yt) for g in range(G)])
        ls.sum().backward()
        return lg.detach().clone(), ls.detach().clone(), [p.grad.clone() for p in b.parameters()]

    import copy
    a = run(copy.deepcopy(bank), keep)
    again = run(copy.deepcopy(bank), keep)
    assert torch.equal(a[0], again[0]) and torch.equal(a[1], again[1])
    assert all(torch.equal(p, q) for p, q in zip(a[2], again[2])), "two identical bank steps differ"
    keep2 = None
    if masked:
        keep2 = keep.copy()
        keep2[:, 100 * U:200 * U] ^= 1
    other = _perturbed(bank, c, seed=77)
    b2 = run(other, keep2)
    assert not torch.equal(a[0][:, 1], b2[0][:, 1]), "the perturbation did not reach member 1"
    for g in (0, 2):
        assert torch.equal(a[0][:, g], b2[0][:, g]) and torch.equal(a[1][g], b2[1][g]), g
        for (name, _), p, q in zip(bank.named_parameters(), a[2], b2[2]):
            assert torch.equal(bank._member_view(name, p, g), bank._member_view(name, q, g)), (g, name)


def test_bank_builtin_dropout_differs_between_members():
    """Test 8: with BatchNorm2's weight 0 and bias 1 the kept-bits words are the keep mask
    (tests/test_gpu_parity.py::test_builtin_dropout_generator_statistics); two members with IDENTICAL
    parameters draw different masks, each at the generator's keep rate (same sigma bounds as there)."""
    from explainn_amd import ExplaiNNBank, _lib
    G, U, k, L, T, B = 2, 32, 19, 200, 1, 1024
    sd = orc.random_state_dict(U, k, L, T, seed=5, perturb=False)
    sd["linears.7.weight"] = np.zeros_like(sd["linears.7.weight"])
    sd["linears.7.bias"] = np.ones_like(sd["linears.7.bias"])
    bank = ExplaiNNBank.from_models([model(sd, U, k, L, T) for _ in range(G)]).cuda().train()
    x = torch.from_numpy(orc.random_onehot(B, L, seed=6)).cuda()
    torch.manual_seed(1234)
    with torch.no_grad():
        bank(x)
    ctx = bank._rt.ctx
    assert ctx.lib.explainn_groups(ctx.handle) == G
    words = torch.empty(G * U, B, 4, dtype=torch.int32, device="cuda")
    _lib.check(ctx.lib.explainn_debug_keep_bits(ctx.handle, B, words.data_ptr(),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    w = words.cpu().numpy().view(np.uint32)
    bits = np.unpackbits(w.view(np.uint8).reshape(G * U, B, 16), axis=2, bitorder="little")[:, :, :100].astype(bool)
    m0, m1 = bits[:U], bits[U:]
    assert not np.array_equal(m0, m1), "two members of a bank share their dropout mask"
    p_keep = 1.0 - 19661.0 / 65536.0
    var = p_keep * (1 - p_keep)
    for g, M in enumerate((m0, m1)):
        for what, values, n_per, k_sigma in (("overall", np.array([M.mean()]), M.size, 4.0),
                                             ("per channel", M.mean(axis=(0, 1)), U * B, 4.6),
                                             ("per sequence", M.mean(axis=(0, 2)), U * 100, 5.0),
                                             ("per unit", M.mean(axis=(1, 2)), B * 100, 4.4)):
            z = np.abs(values - p_keep).max() / np.sqrt(var / n_per)
            record_margin("bank dropout keep rate, member %d %s" % (g, what), z, k_sigma)
            assert z < k_sigma, "member %d %s: keep rate off by %.2f sigma (bound %.1f)" % (g, what, z, k_sigma)


def test_bank_refuses_single_model_calls_and_stays_usable():
    """Test 9: what folds units through `final` in kernels of its own raises the documented error on a
    bank, in Python and at the C ABI, and the context goes on working."""
    import copy
    from explainn_amd import _lib
    from explainn_amd.engine import StepEngine
    c = CASES[0]
    sds = [_member_sd(c, g) for g in range(c.G)]
    x, y = _batch(c)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    bank = _bank(c, sds)
    bank.dropout_p = 0.0
    before = copy.deepcopy(bank)
    with pytest.raises(ValueError, match=r"member\(g\)"):
        bank(xt.clone().requires_grad_(True))
    bank.eval()
    with pytest.raises(ValueError, match=r"member\(g\)"):
        bank(xt.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"member\(g\)"):
        bank.input_gradient(xt, torch.ones(c.B, c.G, c.T, device="cuda"))
    with pytest.raises(ValueError, match=r"member\(g\)"):
        bank.in_silico_mutagenesis(xt)
    with pytest.raises(ValueError, match=r"member\(g\)"):
        bank.sync_bn = object()
    bank.train()
    eng = StepEngine(bank, c.B, c.kind)
    ctx, ps = eng.ctx, eng.ps
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(c.B, c.G, c.T, device="cuda")
    dx = torch.empty(c.B, 4, c.L, device="cuda")
    lib, h = ctx.lib, ctx.handle
    calls = [
        lambda: lib.explainn_forward_eval_keep(h, xt.data_ptr(), c.B, C.byref(ps), out.data_ptr(), stream),
        lambda: lib.explainn_input_grad(h, out.data_ptr(), c.B, C.byref(ps), dx.data_ptr(), stream),
        lambda: lib.explainn_backward_input(h, out.data_ptr(), c.B, C.byref(ps), C.byref(eng.gs), 0,
                                            dx.data_ptr(), stream),
        lambda: lib.explainn_ism(h, xt.data_ptr(), c.B, C.byref(ps), out.data_ptr(), dx.data_ptr(),
                                 dx.data_ptr(), 1 << 20, stream),
    ]
    sync_args = _lib.SyncArgs(x=xt.data_ptr(), B_local=c.B, B_global=c.B, params=C.pointer(ps),
                              grads=C.pointer(eng.gs), logits=out.data_ptr())
    calls.append(lambda: lib.explainn_sync_phase(h, 1, C.byref(sync_args), None, None, stream))
    for call in calls:
        assert call() == _lib.E_UNSUPPORTED
        assert b"member(g)" in lib.explainn_last_error()
    logits, loss = eng.step(xt, yt, freeze_top_n_filters=c.freeze)
    torch.cuda.synchronize()
    for g in range(c.G):
        _against_member(c, "after refused calls, member %d" % g, before, g, xt, yt, logits, loss, eng.views)


def test_bank_export_paths_and_split_step_against_members():
    """Entry points the header lists as supported on a bank: per-unit outputs (B, G*U) and
    activations equal the members', and explainn_train_step_fc + _conv equal explainn_train_step
    bit for bit."""
    from explainn_amd.engine import StepEngine
    from explainn_amd.parallel import GradAllReduce
    c = CASES[0]
    sds = [_member_sd(c, g) for g in range(c.G)]
    x, y = _batch(c)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    bank = _bank(c, sds).eval()
    with torch.no_grad():
        outs = bank.linears(xt)
        acts = bank.linears[:3](xt[:8])
        assert outs.shape == (c.B, c.G * c.U) and acts.shape == (8, c.G * c.U, c.L - c.k + 1)
        for g in range(c.G):
            m = bank.member(g)
            sl = slice(g * c.U, (g + 1) * c.U)
            close(to_np(outs[:, sl]), to_np(m.linears(xt)), what="bank unit outputs member %d" % g)
            close(to_np(acts[:, sl]), to_np(m.linears[:3](xt[:8])), what="bank unit activations member %d" % g)
    bank.train()
    eng = StepEngine(bank, c.B, c.kind)
    lg, ls = eng.step(xt, yt, seed=5)
    whole = (lg.clone(), ls.clone(), eng.flat_grad.clone())
    lg, ls = eng.step(xt, yt, seed=5, grad_sync=GradAllReduce(eng.flat_grad, split=eng.conv_grad_elements))
    torch.cuda.synchronize()
    assert torch.equal(whole[0], lg) and torch.equal(whole[1], ls) and torch.equal(whole[2], eng.flat_grad)


def test_bank_cli_run_end_to_end(tmp_path):
    """Test 10 (first half): `train -i 3 --bank` on a generated TSV.  Every init.<g>/best_model.pth.tar
    loads with the existing predict._load_model; the smallest `loss` of init.<g>/validation.txt is the
    loss recomputed from that checkpoint; a bank rebuilt from the checkpoints gives each member's
    logits; the final long run resumes from the selected checkpoint with its optimiser state."""
    from explainn_amd import ExplaiNNBank
    from explainn_amd.loader import read_tsv_codes
    from explainn_amd.predict import _load_model
    from explainn_amd.selene import _load_checkpoint_file
    from explainn_amd.train import main
    rng = np.random.default_rng(3)
    L = 200

    def write(path, n):
        with open(path, "wt") as fh:
            for i in range(n):
                seq = rng.integers(0, 4, L)
                label = int(rng.random() > 0.5)
                if label:
                    pos = int(rng.integers(0, L - 8))
                    seq[pos:pos + 8] = [0, 1, 2, 3, 3, 2, 1, 0]
                fh.write("s%d\t%s\t%d\n" % (i, "".join("ACGT"[b] for b in seq), label))
    tr_file, va_file = str(tmp_path / "train.tsv"), str(tmp_path / "validation.tsv")
    write(tr_file, 300)
    write(va_file, 100)
    out = tmp_path / "out"
    torch.manual_seed(4)
    main([tr_file, va_file, "-o", str(out), "-i", "3", "--bank", "--cnn-units", "8", "-b", "50",
          "--max-epochs", "2", "--patience", "2"])
    codes, labels, _ = read_tsv_codes(va_file)
    ct, yt = torch.from_numpy(codes).cuda(), torch.from_numpy(labels).cuda()
    models, best = [], None
    for g in range(3):
        d = out / ("init.%d" % g)
        for name in ("train.txt", "validation.txt", "best_model.pth.tar"):
            assert (d / name).exists(), (g, name)
        rows = (d / "validation.txt").read_text().splitlines()
        assert rows[0].split("\t") == ["loss", "aucROC", "aucPR"] and len(rows) >= 2
        losses = [float(r.split("\t")[0]) for r in rows[1:]]
        m = _load_model(str(d / "best_model.pth.tar"))
        with torch.no_grad():
            lg = m(ct)
        # (100 validation sequences in batches of 50: the average of the batch losses is the mean over all)
        close(min(losses), float(torch.nn.functional.binary_cross_entropy_with_logits(lg, yt)),
              what="init.%d validation loss vs its checkpoint" % g)
        ck = _load_checkpoint_file(str(d / "best_model.pth.tar"))
        assert abs(float(ck["min_loss"]) - min(losses)) < 1e-6 and ck["arch"] == "ExplaiNN"
        models.append((m, lg))
        if best is None or min(losses) < best[0]:
            best = (min(losses), ck["step"])
    bank = ExplaiNNBank.from_models([m for m, _ in models]).cuda().eval()
    with torch.no_grad():
        got = bank(ct)
    for g, (_, lg) in enumerate(models):
        close(to_np(got[:, g]), to_np(lg), what="bank member %d eval logits vs its checkpoint" % g)
    assert (out / "best_model.pth.tar").exists()
    log = (out / "selene.log").read_text()
    assert "Resuming from checkpoint: step %d," % best[1] in log, log[-400:]


def test_bank_adam_trajectory_against_members():
    """Test 10 (second half): five fused-Adam steps of a bank, dropout off, vs the same five on each
    member alone with the same batches: per-step losses within 1e-2 (the bound
    test_adam_trajectory_golden uses once trajectories may part)."""
    from explainn_amd import ExplaiNNBank, get_optimizer
    from explainn_amd.engine import StepEngine
    G, U, k, L, T, B = 3, 8, 19, 200, 1, 100
    c = Case("adam", G, U, k, L, T, B, "binary", 0, 0.0, False, False)
    torch.manual_seed(21)
    bank = ExplaiNNBank(G, U, k, L, T).cuda().train()
    bank.dropout_p = 0.0
    members = [bank.member(g) for g in range(G)]
    batches = []
    for i in range(5):
        x = orc.random_onehot(B, L, seed=40 + i)
        y = (np.random.default_rng(50 + i).random((B, T)) > 0.5).astype(np.float32)
        batches.append((torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()))

    def trajectory(m):
        eng = StepEngine(m, B, "binary")
        eng.attach_grads()
        opt = get_optimizer(m.parameters(), lr=1e-3)
        out = []
        for xt, yt in batches:
            _, loss = eng.step(xt, yt)
            out.append(loss.clone())
            opt.step()
        torch.cuda.synchronize()
        return torch.stack(out).cpu().numpy()        # (5, G) or (5, 1)

    got = trajectory(bank)
    worst = 0.0
    for g, m in enumerate(members):
        ref = trajectory(m)[:, 0]
        worst = max(worst, float(np.abs(got[:, g] - ref).max()))
    record_margin("bank Adam trajectory vs members, max |loss difference|", worst, 1e-2)
    print("bank Adam trajectory: max |loss difference| %.3e" % worst)
    assert worst <= 1e-2
