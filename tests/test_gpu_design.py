"""Greedy in-silico evolution on the device (csrc/evolve.hip): the stand-alone selection against the
numpy model bit for bit, the loop against the host loop it replaces (model.in_silico_mutagenesis per
strand and round, the model's selection, the edit) bit for bit, its consistency with the logits, edges,
errors and the CLI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import explainn_oracle as orc
from parity_util import model as make_model
from tests import design_model as dm

pytestmark = pytest.mark.gpu
TOL = 1e-4                     # the project's logit tolerance (tests/test_gpu_ism.py)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1. explainn_evolve_pick against the model ---------------------------------------------------
def _pick_device(df, dr, codes, mask, w, lock, min_gain):
    from explainn_amd import _lib
    lib = _lib.load()
    B, T, _, L = df.shape
    tf, tr = _dev(df), (_dev(dr) if dr is not None else None)
    tc, tm, tw = _dev(codes), (_dev(mask) if mask is not None else None), _dev(w)
    pos = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    ref = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
    alt = torch.full((B,), 77, dtype=torch.uint8, device="cuda")
    gain = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(lib.explainn_evolve_pick(
        tf.data_ptr(), tr.data_ptr() if tr is not None else None, tc.data_ptr(),
        tm.data_ptr() if tm is not None else None, tw.data_ptr(), int(w.ndim == 2), B, T, L, int(lock),
        min_gain, pos.data_ptr(), ref.data_ptr(), alt.data_ptr(), gain.data_ptr(),
        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return (pos.cpu().numpy(), ref.cpu().numpy(), alt.cpu().numpy(), gain.cpu().numpy(), tc.cpu().numpy(),
            tm.cpu().numpy() if tm is not None else None)


def _pick_inputs(rng, B, T, L, both, per_row):
    """Maps on a grid of eighths, codes with N, weights with w[., 0] = 1.  Row 0 is quiet: its only
    non-zero entries are 1/8 in task 0, so 0.15 exceeds all of its gains."""
    grid = lambda: (rng.integers(-4, 5, size=(B, T, 4, L)) / 8.0).astype(np.float32)
    df, dr = grid(), (grid() if both else None)
    for d in (df, dr):
        if d is not None:
            d[0] = 0
            d[0, 0] = (rng.random((4, L)) < 0.5) / 8.0
    codes = rng.integers(0, 4, size=(B, L)).astype(np.uint8)
    codes[rng.random((B, L)) < 0.08] = 4
    w = (rng.integers(-2, 3, size=(B, T) if per_row else (T,)) / 2.0).astype(np.float32)
    w[..., 0] = 1.0
    return df, dr, codes, w


@pytest.mark.parametrize("L", [7, 61, 257])
@pytest.mark.parametrize("T", [1, 3, 5, 9])
@pytest.mark.parametrize("B", [1, 64, 65, 130])
@pytest.mark.parametrize("per_row", [False, True])
@pytest.mark.parametrize("both", [False, True])
def test_pick_matches_model(both, per_row, B, T, L):
    """Three calls per parametrisation (a batch of one cannot hold a row that moves and one that does not in
    one call); over them a tie for the maximum, a row without a move and a row with one are asserted."""
    rng = np.random.default_rng(((B * 16 + T) * 512 + L) * 4 + 2 * both + per_row)
    df, dr, codes, w = _pick_inputs(rng, B, T, L, both, per_row)
    masked = (rng.random((B, L)) < 0.7).astype(np.uint8)
    masked[0] = 0                                             # an all-zero row
    if B > 1:
        masked[1] = 0
        masked[1, rng.integers(L)] = 1                        # a single open position
    tied = np.ones((B, L), np.uint8)
    dft, drt = df.copy(), (dr.copy() if both else None)
    for d in (dft, drt):                                      # row 0: every candidate ties
        if d is not None:
            d[0] = 0
            d[0, 0] = 0.25
    calls = [(df, dr, masked, 1, 0.0),                        # masks; the all-zero row does not move
             (df, dr, None, 0, 0.15),                         # no mask; min_gain above every gain of row 0
             (dft, drt, tied, 1, 0.0)]                        # row 0 moves on a tie of all its candidates
    seen = dict(tie=0, none=0, moved=0)
    for f, r, mask, lock, min_gain in calls:
        want = dm.pick(f, r, codes, mask, w, lock, min_gain)
        got = _pick_device(f, r, codes, mask, w, lock, min_gain)
        for name, g, x in zip(("pos", "ref", "alt"), got[:3], want[:3]):
            assert np.array_equal(g, x), (name, min_gain)
        assert np.array_equal(_bits(got[3]), _bits(want[3])), ("gain", min_gain)
        assert np.array_equal(got[4], want[4])
        assert (got[5] is None and want[5] is None) or np.array_equal(got[5], want[5])
        # what the call exercised, from the model's side
        gains = dm.objective(f, r, w)
        ok = dm.admissible(gains, codes, mask, min_gain)
        top = np.where(ok, gains, -np.inf).max(axis=(1, 2))
        seen["tie"] += int(((ok & (gains == top[:, None, None])).sum(axis=(1, 2)) >= 2).sum())
        seen["none"] += int((want[0] < 0).sum())
        seen["moved"] += int((want[0] >= 0).sum())
    assert seen["tie"] > 0 and seen["none"] > 0 and seen["moved"] > 0, seen


# ---- 2. / 3. the loop against the host loop -------------------------------------------------------
def _model_case(U, k, L, T, B, seed):
    sd = orc.random_state_dict(U, k, L, T, seed=seed)
    sd["linears.1.weight"][::3] = -np.abs(sd["linears.1.weight"][::3]) - 0.3          # min-pooling units
    rng = np.random.default_rng(seed + 1)
    codes = rng.integers(0, 4, size=(B, L)).astype(np.uint8)
    codes[rng.random((B, L)) < 0.02] = 4
    for b, s, n in ((1, 0, 6), (B // 2, L // 3, 9), (B - 1, L - 4, 4)):              # N runs
        codes[b, s:s + n] = 4
    return make_model(sd, U, k, L, T).eval(), codes, rng


def _host_ism(m):
    from explainn_amd.architectures import BaseCodes

    def ism(codes, rc):
        lg, d = m.in_silico_mutagenesis(BaseCodes(torch.tensor(codes, device="cuda"), rc))
        return lg.cpu().numpy(), d.cpu().numpy()
    return ism


SHAPES = {"small": (5, 5, 61, 3, 65, 5), "wide": (33, 19, 200, 1, 130, 4)}      # U, k, L, T, B, rounds
FORMS = [(False, True, False), (True, True, True), (False, False, True), (True, False, False)]   # both, lock, masked
_RUNS = {}


def _run(shape, form):
    """The device result and the host loop's of one case, computed once."""
    key = (shape, form)
    if key not in _RUNS:
        from explainn_amd import design
        U, k, L, T, B, rounds = SHAPES[shape]
        both, lock, masked = form
        m, codes, rng = _model_case(U, k, L, T, B, seed=7 + U)
        w = rng.normal(size=(B, T) if masked else (T,)).astype(np.float32)
        mask = None
        if masked:
            mask = (rng.random((B, L)) < 0.6).astype(np.uint8)
            mask[2] = 0
        ref = dm.evolve(_host_ism(m), codes, w, rounds, mask, both, lock)
        ev = design.evolve(m, codes, target=w, rounds=rounds, mutable=mask, rev_complement=both, lock=lock)
        _RUNS[key] = dict(m=m, codes=codes, w=w, mask=mask, ref=ref, ev=ev)
    return _RUNS[key]


def _same(ev, ref):
    for name in ("pos", "ref", "alt"):
        assert np.array_equal(getattr(ev, name), ref[name]), name
    assert np.array_equal(_bits(ev.gain), _bits(ref["gain"]))
    assert np.array_equal(ev.codes, ref["codes"])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_evolve_matches_host_loop(shape, form):
    from explainn_amd.architectures import BaseCodes
    run = _run(shape, form)
    ev, ref, m = run["ev"], run["ref"], run["m"]
    U, k, L, T, B, rounds = SHAPES[shape]
    _same(ev, ref)
    assert (ev.pos >= 0).sum() >= B, "the case moves"
    assert np.array_equal(ev.logits, ref["logits"])
    with torch.no_grad():
        for r in range(rounds + 1):
            cr = torch.tensor(ref["rounds_codes"][r], device="cuda")
            for s in range(2 if form[0] else 1):
                assert torch.equal(torch.from_numpy(ev.logits[:, r, s]).cuda(), m(BaseCodes(cr, bool(s)))), (r, s)
    if shape == "small" and not form[0]:
        # one strand: position 60 reaches no pooled window (7 * 8 + 5 - 1 = 60) and is never picked.  (With both
        # strands it is position 0 of the reverse strand, which the objective does see.)
        assert np.all(ev.pos != 60)


@pytest.mark.parametrize("both", [False, True])
def test_result_does_not_depend_on_the_split(both):
    """B = 130 in Python-level batches of 64, and model.evolve on the whole batch on device tensors."""
    from explainn_amd import design
    form = (both, True, both)
    run = _run("wide", form)
    m, codes, w, mask, ev = run["m"], run["codes"], run["w"], run["mask"], run["ev"]
    U, k, L, T, B, rounds = SHAPES["wide"]
    _same(design.evolve(m, codes, target=w, rounds=rounds, mutable=mask, rev_complement=both, batch_size=64), run["ref"])
    cb, wb = torch.tensor(codes, device="cuda"), torch.tensor(w, device="cuda")
    mb = torch.tensor(mask, device="cuda") if mask is not None else None
    pos, rf, alt, gain, logits = m.evolve(cb, wb, rounds, mb, both, True, 0.0)
    assert np.array_equal(pos.cpu().numpy().T, ev.pos) and np.array_equal(alt.cpu().numpy().T, ev.alt)
    assert np.array_equal(rf.cpu().numpy().T, ev.ref) and np.array_equal(_bits(gain.cpu().numpy().T), _bits(ev.gain))
    assert np.array_equal(cb.cpu().numpy(), ev.codes)
    assert np.array_equal(logits.permute(2, 0, 1, 3).cpu().numpy(), ev.logits)
    if mb is not None:
        assert np.array_equal(mb.cpu().numpy(), mask), "the caller's mask is read only"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_consistency(shape, form):
    run = _run(shape, form)
    ev, codes, mask = run["ev"], run["codes"], run["mask"]
    both, lock, masked = form
    wsum = np.abs(np.broadcast_to(run["w"], (len(codes), run["w"].shape[-1]))).sum(axis=1)
    err = np.abs((ev.score[:, 1:] - ev.score[:, :-1]) - ev.gain)
    assert np.all(err <= TOL * wsum[:, None]), (err / wsum[:, None]).max()
    assert np.all(ev.gain[ev.pos >= 0] > 0.0) and np.all(ev.gain[ev.pos < 0] == 0.0)
    assert np.all((ev.pos >= 0) == (ev.alt < 4)) and np.all((ev.pos < 0) == (ev.ref == 255))
    for b in range(len(codes)):
        used = ev.pos[b][ev.pos[b] >= 0]
        if lock:
            assert len(set(used)) == len(used)
        if mask is not None:
            assert np.all(mask[b, used] != 0)
            assert np.array_equal(ev.codes[b][mask[b] == 0], codes[b][mask[b] == 0])
        untouched = np.setdiff1d(np.arange(codes.shape[1]), used)
        assert np.array_equal(ev.codes[b, untouched], codes[b, untouched])
    if masked:
        assert np.all(ev.pos[2] == -1)


# ---- 4. edges ------------------------------------------------------------------------------------
def test_zero_head_moves_nothing():
    from explainn_amd import design
    m, codes, _ = _model_case(6, 7, 50, 2, 20, seed=31)
    with torch.no_grad():
        m.final.weight.zero_()
    ev = design.evolve(m, codes, target=np.array([1.0, -2.0], np.float32), rounds=3, rev_complement=True)
    assert np.all(ev.pos == -1) and np.all(ev.ref == 255) and np.all(ev.alt == 255) and np.all(ev.gain == 0)
    assert np.array_equal(ev.codes, codes)
    assert np.all(ev.logits == ev.logits[:, :1, :1]) and np.array_equal(ev.logits[0, 0, 0], m.final.bias.detach().cpu().numpy())


def test_one_round_is_the_argmax_of_the_ism_map():
    from explainn_amd import design, interpret
    m, codes, _ = _model_case(9, 11, 80, 3, 40, seed=32)
    ev = design.evolve(m, codes, target=1, rounds=1)
    dmap = interpret.in_silico_mutagenesis(m, codes, target=1).astype(np.float64)          # (N,4,L)
    ok = (np.arange(4)[None, :, None] != codes[:, None, :]) & (dmap > 0)
    flat = np.where(ok, dmap, -np.inf).transpose(0, 2, 1).reshape(len(codes), -1)
    best = flat.argmax(axis=1)
    assert ok.any(axis=(1, 2)).all()
    assert np.array_equal(ev.pos[:, 0], best // 4) and np.array_equal(ev.alt[:, 0], best % 4)
    assert np.array_equal(ev.gain[:, 0], flat[np.arange(len(codes)), best])
    assert np.array_equal(ev.ref[:, 0], codes[np.arange(len(codes)), best // 4])


def test_minimize_determinism_and_context_reuse():
    from explainn_amd import design
    from explainn_amd.architectures import BaseCodes
    U, k, L, T, B = 8, 9, 70, 3, 70
    m, codes, rng = _model_case(U, k, L, T, B, seed=33)
    w = rng.normal(size=T).astype(np.float32)
    a = design.evolve(m, codes, target=w, rounds=3, maximize=False, rev_complement=True)
    b = design.evolve(m, codes, target=-w, rounds=3, rev_complement=True)
    c = design.evolve(m, codes, target=-w, rounds=3, rev_complement=True)
    for x in (b, c):
        _same(x, dict(pos=a.pos, ref=a.ref, alt=a.alt, gain=a.gain, codes=a.codes))
        assert np.array_equal(x.logits, a.logits) and np.array_equal(_bits(x.score), _bits(a.score))
    assert (a.pos >= 0).any() and np.all(a.score[:, -1] >= a.score[:, 0] - TOL * np.abs(w).sum())
    # the context that ran evolve answers like a fresh one
    fresh, _, _ = _model_case(U, k, L, T, B, seed=33)
    ct = torch.tensor(codes, device="cuda")
    with torch.no_grad():
        assert torch.equal(m(ct), fresh(ct))
        for rc in (False, True):
            l1, d1 = m.in_silico_mutagenesis(BaseCodes(ct, rc))
            l2, d2 = fresh.in_silico_mutagenesis(BaseCodes(ct, rc))
            assert torch.equal(l1, l2) and torch.equal(d1, d2)


# ---- 5. errors and surface -----------------------------------------------------------------------
def test_errors():
    from explainn_amd import ExplaiNNBank, _lib, design
    U, k, L, T, B = 6, 5, 40, 2, 6
    m, codes, _ = _model_case(U, k, L, T, B, seed=34)
    m.train()
    with pytest.raises(RuntimeError):
        design.evolve(m, codes, target=0)
    with pytest.raises(RuntimeError):
        m.evolve(torch.tensor(codes, device="cuda"), torch.ones(T))
    m.eval()
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=0, rounds=0)
    with pytest.raises(ValueError):
        design.evolve(m, codes)                                       # two tasks and no target
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=T)
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=np.ones(T + 1, np.float32))
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=np.ones((B + 1, T), np.float32))
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=0, mutable=np.ones(L + 1))
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=0, mutable=np.ones((B, L - 1)))
    with pytest.raises(ValueError):
        design.evolve(m, codes[:, :-1], target=0)
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=0, min_gain=-1.0)
    onehot = np.stack([(codes == a) for a in range(4)], axis=1).astype(np.float32)
    with pytest.raises(ValueError):
        design.evolve(m, onehot * 0.5, target=0)                      # soft input
    ev = design.evolve(m, onehot, target=0, rounds=2)                 # one-hot is converted
    _same(design.evolve(m, codes, target=0, rounds=2), dict(pos=ev.pos, ref=ev.ref, alt=ev.alt, gain=ev.gain,
                                                            codes=ev.codes))
    m.dense_input = True
    with pytest.raises(ValueError):
        design.evolve(m, codes, target=0)
    m.dense_input = None
    bank = ExplaiNNBank(2, U, k, L, T).cuda().eval()
    with pytest.raises(ValueError, match="member"):
        bank.evolve(torch.tensor(codes, device="cuda"), torch.ones(T))
    # C ABI: the selection refuses null maps or outputs and a bad min_gain; evolve ends a pending train forward
    lib, dev = _lib.load(), m._device()
    ct, wt = torch.tensor(codes, device=dev), torch.ones(T, device=dev)
    dmap = torch.zeros(B, T, 4, L, device=dev)
    pos = torch.empty(B, dtype=torch.int32, device=dev)
    ref, alt = torch.empty(B, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    gain = torch.empty(B, dtype=torch.float64, device=dev)
    st = m._stream(dev)

    def call(fwd=dmap.data_ptr(), min_gain=0.0, gain_ptr=gain.data_ptr(), nB=B):
        return lib.explainn_evolve_pick(fwd, None, ct.data_ptr(), None, wt.data_ptr(), 0, nB, T, L, 0, min_gain,
                                        pos.data_ptr(), ref.data_ptr(), alt.data_ptr(), gain_ptr, st)
    assert call(fwd=None) == _lib.E_ARG and call(gain_ptr=None) == _lib.E_ARG and call(nB=0) == _lib.E_ARG
    assert call(min_gain=-0.5) == _lib.E_ARG
    assert call(min_gain=float("nan")) == _lib.E_ARG and call(min_gain=float("inf")) == _lib.E_ARG
    _lib.check(call())
    torch.cuda.synchronize()
    assert np.all(pos.cpu().numpy() == -1) and np.array_equal(ct.cpu().numpy(), codes)      # an all-zero map moves nothing
    m.train()
    x = torch.tensor(onehot, device=dev)
    out = m(x)
    m.eval()
    m.evolve(ct, wt, 1)
    with pytest.raises(RuntimeError):
        out.sum().backward()
    torch.cuda.synchronize()


def test_cli(tmp_path):
    from explainn_amd import design
    U, k, L, T, B = 6, 9, 60, 2, 5
    m, codes, _ = _model_case(U, k, L, T, B, seed=35)
    ckpt = os.path.join(tmp_path, "model.pth.tar")
    torch.save({"options": dict(m._options), "state_dict": {key: v.cpu() for key, v in m.state_dict().items()}},
               ckpt)
    fa = os.path.join(tmp_path, "seqs.fa")
    with open(fa, "w") as fh:
        for i, row in enumerate(codes):
            fh.write(">s%d desc\n%s\n" % (i, "".join("ACGTN"[c] for c in row)))
    out, ofa = os.path.join(tmp_path, "design.tsv"), os.path.join(tmp_path, "design.fa")
    design.main([ckpt, fa, "--target", "1", "--minimize", "--rounds", "4", "-r", "--region", "10:50",
                 "--allow-revisit", "--min-gain", "0.001", "-b", "3", "-o", out, "--fasta", ofa])
    mutable = np.zeros(L, np.uint8)
    mutable[10:50] = 1
    ev = design.evolve(m, codes, target=1, rounds=4, maximize=False, mutable=mutable, rev_complement=True,
                       lock=False, min_gain=0.001)
    lines = open(out).read().splitlines()
    assert lines[0].split("\t") == ["SeqId", "Round", "Pos", "Ref", "Alt", "Gain", "Score"]
    rows = [ln.split("\t") for ln in lines[1:]]
    muts = ev.mutations()
    assert len(rows) == len(muts) == int((ev.pos >= 0).sum()) and len(rows) > 0
    for row, (i, r, p, ref, alt, gain, score) in zip(rows, muts):
        assert row[:5] == ["s%d" % i, str(r), str(p), ref, alt]
        assert float(row[5]) == gain and float(row[6]) == score and 10 <= p < 50
    fasta = open(ofa).read().split()
    assert fasta[0::2] == [">s%d" % i for i in range(B)] and fasta[1::2] == ev.sequences()
