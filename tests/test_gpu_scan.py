"""The tiled scan on the device: explainn_stage_windows, explainn_scan (both modes) and
explainn_amd.scan.scan.  -m gpu.  Every case runs once.

What is compared with what:
  * explainn_stage_windows against explainn_stage_codes on the host-materialised (B,L) matrix: the
    eval logits of the staged batch, torch.equal; one train step's gradients at GRAD_TOL_GOLDEN;
  * scan(mode="windows") and scan(mode="shared") against predict() on the materialised windows:
    np.array_equal on all four columns.  Exact because a position's conv sum is one fixed-order MFMA
    chain of exact products wherever the position sits in a tile, the pooled extreme is a selection,
    and fc_fwd and the head treat sequences independently;
  * independently of predict(), the same outputs against the fp64 oracle on the materialised windows
    at TOL (1e-4 absolute, the project's logit tolerance).
Shapes: the four (L, k) of tests/test_scan_model.py, with every U of {3, 100, 300} and every T of
{1, 3, 50} appearing (not their full product: the oracle runs every window of every case in fp64).
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import explainn_oracle as orc  # noqa: E402
from parity_util import GRAD_TOL_GOLDEN, TOL, close, close_rel, model, to_np  # noqa: E402
import scan_model as sm  # noqa: E402

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
    """fp64 eval logits of a (W,L) code matrix, in batches."""
    out = []
    for i in range(0, len(mat), 256):
        out.append(orc.forward(sd, sm.onehot(mat[i:i + 256]), dtype=np.float64))
    return np.concatenate(out)


def _eval_model(sd, U, k, L, T):
    m = model(sd, U, k, L, T).eval()
    m.validate_input = False
    return m


# ---- explainn_stage_windows ---------------------------------------------------------------------

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


L0, K0 = 200, 19
N0 = (L0 - K0 + 1) // 7


@pytest.mark.parametrize("rc", [0, 1])
@pytest.mark.parametrize("step,start0,B", [
    (1, -30, 64), (1, 2950, 65), (7, -5, 1000), (7, 1000, 1), (50, -100, 65), (50, 100, 64),
    (L0, -L0 - 3, 65), (-7 * N0, 2900, 64), (-7 * N0, 11900, 65), (63, 17, 65), (-64, 6000, 64), (-1, 40, 65)])
def test_stage_windows_equals_stage_codes(step, start0, B, rc):
    """N padding at both ends (start0 < 0, start0 + B*step + L > seq_len), both directions of step,
    both strands, whole and ragged 64-row tiles."""
    seq = sm.random_codes(3000 if abs(step) < 100 else 12000, seed=abs(step) + B, n_runs=12)
    m = _eval_model(_sd(8, K0, L0, 2, seed=3), 8, K0, L0, 2)
    ctx, ps, keep, stream = _ctx(m, B)
    h, lib = ctx.handle, ctx.lib
    seq_d = torch.from_numpy(seq).cuda()
    mat = sm.window_matrix(seq, start0, B, step, L0)
    mat_d = torch.from_numpy(mat).cuda()
    a = _staged_logits(m, ctx, ps, stream, B, lambda: lib.explainn_stage_windows(
        h, seq_d.data_ptr(), len(seq), start0, step, B, rc, stream))
    flags = C.c_int(0)
    _lib().check(lib.explainn_input_flags(h, C.byref(flags), stream))
    assert flags.value == 0, "positions outside the sequence must not raise the flag"
    b = _staged_logits(m, ctx, ps, stream, B, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), B, rc, stream))
    assert torch.equal(a, b)
    ref = _oracle_logits(_sd(8, K0, L0, 2, seed=3), sm.rc_rows(mat) if rc else mat)
    close(to_np(a), ref, TOL, "stage_windows logits")


def test_stage_windows_flags_a_bad_byte_in_range():
    seq = sm.random_codes(2000, seed=1)
    seq[700] = 9
    m = _eval_model(_sd(8, K0, L0, 1, seed=4), 8, K0, L0, 1)
    ctx, ps, keep, stream = _ctx(m, 64)
    h, lib = ctx.handle, ctx.lib
    seq_d = torch.from_numpy(seq).cuda()
    flags = C.c_int(0)
    # windows that do not touch the byte: no flag
    _lib().check(lib.explainn_stage_windows(h, seq_d.data_ptr(), len(seq), 900, 7, 64, 0, stream))
    _lib().check(lib.explainn_input_flags(h, C.byref(flags), stream))
    assert flags.value == 0
    mat = sm.window_matrix(seq, 600, 64, 7, L0)
    a = _staged_logits(m, ctx, ps, stream, 64, lambda: lib.explainn_stage_windows(
        h, seq_d.data_ptr(), len(seq), 600, 7, 64, 0, stream))
    _lib().check(lib.explainn_input_flags(h, C.byref(flags), stream))
    assert flags.value & 1
    raw = mat.copy()                                 # the materialised matrix with the byte as it is
    rows = np.arange(64)
    cols = 700 - (600 + 7 * rows)
    hit = (cols >= 0) & (cols < L0)
    assert hit.any() and (mat[rows[hit], cols[hit]] == 4).all()
    raw[rows[hit], cols[hit]] = 9
    mat_d = torch.from_numpy(raw).cuda()
    b = _staged_logits(m, ctx, ps, stream, 64, lambda: lib.explainn_stage_codes(h, mat_d.data_ptr(), 64, 0, stream))
    _lib().check(lib.explainn_input_flags(h, C.byref(flags), stream))
    assert flags.value & 1
    assert torch.equal(a, b)                         # the byte reads as N on both paths


def _grads_struct(m):
    L_ = _lib()
    g = L_.Grads()
    sd = dict(m.state_dict())
    keep = {}
    for f in L_.GRAD_FIELDS:
        keep[f] = torch.zeros_like(sd[L_.PARAM_KEYS[f]]).contiguous()
        setattr(g, f, keep[f].data_ptr())
    return g, keep


def test_stage_windows_train_step_gradients():
    """A staged window batch feeds a train step like a staged code matrix: same keep mask, same
    gradients (bit equality expected; the claim is GRAD_TOL_GOLDEN)."""
    U, T, B = 8, 2, 96
    sd = _sd(U, K0, L0, T, seed=6)
    seq = sm.random_codes(1500, seed=8, n_runs=4)
    mat = sm.window_matrix(seq, -20, B, 13, L0)
    rng = np.random.default_rng(9)
    keep_mask = torch.from_numpy((rng.random((B, 100 * U)) > 0.3).astype(np.uint8)).cuda()
    y = torch.from_numpy((rng.random((B, T)) > 0.5).astype(np.float32)).cuda()
    seq_d, mat_d = torch.from_numpy(seq).cuda(), torch.from_numpy(mat).cuda()
    results = []
    for which in ("windows", "codes"):
        m = model(sd, U, K0, L0, T).train()
        ctx, ps, keepalive, stream = _ctx(m, B)
        h, lib = ctx.handle, ctx.lib
        g, gk = _grads_struct(m)
        logits = torch.empty(B, T, device="cuda")
        dl = torch.empty(B, T, device="cuda")
        loss = torch.empty(1, device="cuda")
        if which == "windows":
            _lib().check(lib.explainn_stage_windows(h, seq_d.data_ptr(), len(seq), -20, 13, B, 1, stream))
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
    close(to_np(la), to_np(lb), TOL, "train logits, staged windows vs staged codes")
    for f in ga:
        close_rel(to_np(ga[f]), to_np(gb[f]), tol=GRAD_TOL_GOLDEN, what="staged windows grad " + f)
        print("grad %-8s bit-equal: %s" % (f, torch.equal(ga[f], gb[f])))


# ---- scan against predict() and the oracle ------------------------------------------------------

def _check_scan(sd, U, k, L, T, seq, stride, mode, batch_size, label):
    from explainn_amd.predict import predict
    from explainn_amd.scan import scan
    m = _eval_model(sd, U, k, L, T)
    # scan first, on a fresh model: its contexts then hold batch_size windows, and a scan of more
    # windows than that runs in sub-batches (predict() afterwards grows the contexts)
    starts, preds = scan(m, seq, stride=stride, mode=mode, batch_size=batch_size)
    W = (len(seq) - L) // stride + 1
    assert np.array_equal(starts, np.arange(W) * stride) and preds.shape == (W, T, 4)
    mat = sm.window_matrix(seq, 0, W, stride, L)
    ref = predict(m, mat)
    same = np.array_equal(preds, ref)
    print("%s: W=%d max|scan - predict| = %.3e" % (label, W, np.abs(preds - ref).max()))
    assert same, "%s: scan differs from predict() on the materialised windows" % label
    close(preds[:, :, 0], _oracle_logits(sd, mat), TOL, label + " fwd vs oracle")
    close(preds[:, :, 1], _oracle_logits(sd, sm.rc_rows(mat)), TOL, label + " rev vs oracle")
    return m, preds


SHAPES = [
    # L, k, U, T, sequence length, batch_size
    (200, 19, 300, 1, 6000, 256),
    (50, 5, 3, 3, 50000, 1024),
    (83, 7, 100, 50, 3000, 128),
    (600, 32, 100, 3, 9000, 64),
    (200, 19, 3, 50, 200, 64),          # one window: the sequence is exactly L long
]


@pytest.mark.parametrize("L,k,U,T,length,bs", SHAPES)
@pytest.mark.parametrize("mult", ["7", "14", "7n", "7(n+2)"])
def test_scan_shared_equals_predict(L, k, U, T, length, bs, mult):
    n = (L - k + 1) // 7
    stride = {"7": 7, "14": 14, "7n": 7 * n, "7(n+2)": 7 * (n + 2)}[mult]
    sd = _sd(U, k, L, T, seed=U + T)
    seq = sm.random_codes(length, seed=L + stride, n_runs=max(2, length // 400), tile=7 * n)
    _check_scan(sd, U, k, L, T, seq, stride, "shared", bs, "shared L%d k%d U%d T%d s%d" % (L, k, U, T, stride))


@pytest.mark.parametrize("L,k,U,T,length,bs", SHAPES)
@pytest.mark.parametrize("stride", [1, 10, "L"])
def test_scan_windows_equals_predict(L, k, U, T, length, bs, stride):
    stride = L if stride == "L" else stride
    if stride == 1:
        length = min(length, L + 2500)       # (every base starts a window: keep the oracle's work bounded)
    sd = _sd(U, k, L, T, seed=U + T)
    seq = sm.random_codes(length, seed=L + stride, n_runs=max(2, length // 400), tile=7 * ((L - k + 1) // 7))
    _check_scan(sd, U, k, L, T, seq, stride, "windows", bs, "windows L%d k%d U%d T%d s%d" % (L, k, U, T, stride))


@pytest.mark.parametrize("mode,stride", [("shared", 7), ("shared", 21), ("windows", 7), ("windows", 3)])
@pytest.mark.parametrize("rc", [False, True])
def test_scan_start_not_a_multiple_of_7(mode, stride, rc):
    """The C entry point with start = 5 (and a start before the sequence: N padding), more windows
    than max_batch, against the eval forward of the materialised windows."""
    from explainn_amd.architectures import BaseCodes, SequenceWindows
    from explainn_amd.scan import MODES
    U, T = 33, 3
    sd = _sd(U, K0, L0, T, seed=12)
    seq = sm.random_codes(4000, seed=stride, n_runs=8, tile=7 * N0)
    seq_d = torch.from_numpy(seq).cuda()
    for start in (5, -9):
        W = (len(seq) - start - L0) // stride + 1
        m = _eval_model(sd, U, K0, L0, T)
        got = m._launch_scan(SequenceWindows(seq_d, start, W, stride, rc, 100), MODES[mode])
        assert m._rt.ctx.max_batch == 100 < W
        mat = sm.window_matrix(seq, start, W, stride, L0)
        ref = m(BaseCodes(torch.from_numpy(mat).cuda(), rc))
        assert torch.equal(got, ref), (mode, stride, rc, start, float((got - ref).abs().max()))
        close(to_np(got), _oracle_logits(sd, sm.rc_rows(mat) if rc else mat), TOL, "scan start %d" % start)


def test_scan_chunked_equals_unchunked_and_is_deterministic():
    from explainn_amd.scan import scan
    U, T = 20, 2
    sd = _sd(U, K0, L0, T, seed=21)
    seq = sm.random_codes(9000, seed=22, n_runs=10, tile=7 * N0)
    m = _eval_model(sd, U, K0, L0, T)
    for mode in ("shared", "windows"):
        s0, whole = scan(m, seq, stride=14, mode=mode, batch_size=128)
        s1, again = scan(m, seq, stride=14, mode=mode, batch_size=128)
        assert np.array_equal(whole, again), "two identical scans differ"
        for limit in (len(s0), len(s0) // 2 + 1, 37):
            s2, parts = scan(m, seq, stride=14, mode=mode, batch_size=128, chunk_windows=limit)
            assert np.array_equal(s0, s2) and np.array_equal(whole, parts), (mode, limit)
    # a device-resident sequence, one strand, and the two modes against each other
    seq_d = torch.from_numpy(seq).cuda()
    _, a = scan(m, seq_d, stride=14, mode="shared", strands="fwd", batch_size=128)
    _, b = scan(m, seq_d, stride=14, mode="windows", strands="fwd", batch_size=128)
    assert np.array_equal(a[..., 0], b[..., 0]) and np.isnan(a[..., 1:]).all()
    assert np.array_equal(a[..., 0], whole[..., 0])
    # mode="auto" on a call large enough for the shared track (the AUTO rule of api.hip): same bits
    long_seq = sm.random_codes(7 * 21000 + L0, seed=23, n_runs=20, tile=7 * N0)
    _, auto = scan(m, long_seq, stride=7, strands="fwd", batch_size=2048)
    _, wins = scan(m, long_seq, stride=7, strands="fwd", mode="windows", batch_size=2048)
    assert len(auto) == 21001 and np.array_equal(auto[..., 0], wins[..., 0])
    starts, empty = scan(m, seq[:L0 - 1], stride=7)
    assert len(starts) == 0 and empty.shape == (0, T, 4)
    _, sig = scan(m, seq[:1000], stride=7, apply_sigmoid=True)
    _, raw = scan(m, seq[:1000], stride=7)
    close(sig, 1 / (1 + np.exp(-raw)), 1e-6, "apply_sigmoid")


@pytest.mark.parametrize("T", [3, 50])
def test_scan_bank_equals_members(T):
    from explainn_amd import ExplaiNNBank
    from explainn_amd.scan import scan
    G, U, k, L = 3, 8, 19, 200
    sds = [_sd(U, k, L, T, seed=40 + g) for g in range(G)]
    bank = ExplaiNNBank.from_models([model(sd, U, k, L, T) for sd in sds]).cuda().eval()
    bank.validate_input = False
    seq = sm.random_codes(5000, seed=41, n_runs=6, tile=7 * N0)
    for mode, stride in (("shared", 7), ("windows", 10), ("shared", 14)):
        starts, preds = scan(bank, seq, stride=stride, mode=mode, batch_size=200)
        assert preds.shape == (len(starts), G, T, 4)
        for g in range(G):
            mem = bank.member(g).eval()
            mem.validate_input = False
            _, one = scan(mem, seq, stride=stride, mode=mode, batch_size=200)
            close(preds[:, g], one, TOL, "bank member %d %s T%d" % (g, mode, T))
            if T <= 8:
                assert np.array_equal(preds[:, g], one), (g, mode)


# ---- state and errors ---------------------------------------------------------------------------

def test_scan_state_and_errors():
    L_ = _lib()
    U, T, B = 8, 1, 64
    sd = _sd(U, K0, L0, T, seed=30)
    m = model(sd, U, K0, L0, T).train()
    ctx, ps, keep, stream = _ctx(m, B)
    h, lib = ctx.handle, ctx.lib
    seq = sm.random_codes(3000, seed=31)
    seq_d = torch.from_numpy(seq).cuda()
    x = torch.from_numpy(orc.random_onehot(B, L0, seed=32)).cuda()
    logits = torch.empty(B, T, device="cuda")
    g, gk = _grads_struct(m)
    W = 300
    out = torch.empty(W, T, device="cuda")
    ws_bytes = int(lib.explainn_scan_workspace_bytes(h, W, 7, L_.SCAN_SHARED))
    assert ws_bytes > 0 and lib.explainn_scan_workspace_bytes(h, W, 7, L_.SCAN_WINDOWS) == 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

    def run_scan(mode, stride):
        return lib.explainn_scan(h, seq_d.data_ptr(), len(seq), 0, W, stride, 0, C.byref(ps), out.data_ptr(),
                                 mode, ws.data_ptr(), ws_bytes, stream)

    for mode in (L_.SCAN_WINDOWS, L_.SCAN_SHARED):
        # a scan between a train forward and its backward: the backward must fail
        L_.check(lib.explainn_forward_train(h, x.data_ptr(), B, C.byref(ps), None, 0.0, 0, logits.data_ptr(), stream))
        L_.check(run_scan(mode, 7))
        assert lib.explainn_backward(h, logits.data_ptr(), B, C.byref(ps), C.byref(g), 0, stream) == L_.E_STATE
        # and no staged batch is left behind
        assert lib.explainn_forward_eval(h, None, B, C.byref(ps), logits.data_ptr(), stream) == L_.E_STATE
    # SHARED needs a multiple of 7; the context stays usable
    assert run_scan(L_.SCAN_SHARED, 10) == L_.E_ARG
    assert lib.explainn_scan_workspace_bytes(h, W, 10, L_.SCAN_SHARED) == L_.E_ARG
    assert run_scan(L_.SCAN_AUTO, 10) == L_.OK
    auto = out.clone()
    L_.check(run_scan(L_.SCAN_WINDOWS, 10))
    torch.cuda.synchronize()
    assert torch.equal(auto, out)
    # a short workspace
    assert lib.explainn_scan(h, seq_d.data_ptr(), len(seq), 0, W, 7, 0, C.byref(ps), out.data_ptr(),
                             L_.SCAN_SHARED, ws.data_ptr(), ws_bytes - 1, stream) == L_.E_ARG
    # dense input mode
    L_.check(lib.explainn_dense_input(h, 1))
    assert run_scan(L_.SCAN_WINDOWS, 7) == L_.E_UNSUPPORTED
    assert run_scan(L_.SCAN_SHARED, 7) == L_.E_UNSUPPORTED
    L_.check(lib.explainn_dense_input(h, 0))
    L_.check(lib.explainn_forward_eval(h, x.data_ptr(), B, C.byref(ps), logits.data_ptr(), stream))
    torch.cuda.synchronize()
    assert torch.isfinite(logits).all()


def test_scan_bad_byte_raises_once_and_leaves_no_flag_behind():
    """A byte that is no base code is seen by both strands, so both contexts raise their sticky flag.
    scan() settles them behind its loop: it must raise the one ValueError, and it must read (and so
    clear) BOTH flags before it does -- the next scan(), on clean codes, must not raise for the last
    one's byte.  The first two launches of a handle validate inside the launch itself; three clean
    scans put the model and its replica past that, on the deferred schedule this test is about."""
    from explainn_amd.scan import scan
    sd = _sd(8, K0, L0, 1, seed=4)
    m = model(sd, 8, K0, L0, 1).eval()
    assert m.validate_input is True
    clean = sm.random_codes(400, seed=2)
    bad = clean.copy()
    bad[250] = 7
    first = scan(m, clean, stride=7, strands="both", mode="windows")[1]
    for _ in range(2):
        scan(m, clean, stride=7, strands="both", mode="windows")
    with pytest.raises(ValueError, match="input is not one-hot: base codes must be 0..4"):
        scan(m, bad, stride=7, strands="both", mode="windows")
    again = scan(m, clean, stride=7, strands="both", mode="windows")[1]
    assert np.array_equal(first, again)
