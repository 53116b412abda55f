"""History independence of the device context.  -m gpu.

A model object owns one context: one allocation carved into scratch arrays that every entry point
shares, and state that lives from call to call (tests/history_model.py lists it).  Whatever a context
has been through, a call on it must return BIT FOR BIT what the same call returns on a fresh context of
the same geometry and max_batch, given the same parameters, buffers and inputs.  The project asserts
run-to-run determinism elsewhere, so the comparison is exact and inherits every oracle comparison the
fresh-context tests make.

test_fresh_contexts_agree: every op class and point event, run on two fresh contexts of equal capacity,
gives equal bits (the premise of the exact comparison), and is seen to call the entry points
history_model.OP_CLASSES says it drives (the library handle is wrapped for the count).

test_call_history: one long-lived model A per run of history_model.segments(geometry) is driven through
the run.  Before each op A's state_dict is cloned, a fresh model F is built from the clone and its context
pre-sized to A's max_batch; the op then runs on both with the same inputs, seeds and masks.  Compared,
as bit patterns: every returned tensor, every gradient, every caller-supplied output, every tensor of the
state_dict afterwards, and for an op that raises the exception's type and message.  A mismatch names the
position in the walk, the op, its predecessor, both batch sizes, the tensor and the first differing
element.  No op class is compared under a tolerance.
"""
import collections
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import history_model as hm  # noqa: E402
from oracle import explainn_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

IG_STEPS = 4
SITE_CAPACITY = 8192


def _L():
    from explainn_amd import _lib
    return _lib


class _NoSync:
    """The grad_sync of a one-rank run: makes StepEngine.step take its _fc / _conv halves."""

    def start_tail(self):
        return None

    def finish(self, work):
        pass


class _Spy:
    """The loaded library, remembering which explainn_* functions were looked up to be called."""

    def __init__(self, real):
        self.__dict__["real"] = real
        self.__dict__["calls"] = set()

    def __getattr__(self, name):
        if name.startswith("explainn_"):
            self.calls.add(name)
        return getattr(self.real, name)


# ---- models and inputs ------------------------------------------------------------------------
def _initial_state(g):
    if g.G == 1:
        sd = orc.random_state_dict(g.U, g.k, g.L, g.T, seed=7)
        return {key: torch.from_numpy(np.array(v)) for key, v in sd.items()}
    from explainn_amd.architectures import ExplaiNNBank
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7)
        return ExplaiNNBank(g.G, g.U, g.k, g.L, g.T).state_dict()


def _fresh(g, state, cap):
    """A new model holding `state`, its context pre-sized to `cap`."""
    from explainn_amd import ExplaiNN
    from explainn_amd.architectures import ExplaiNNBank
    with torch.random.fork_rng(devices=[]):
        m = ExplaiNNBank(g.G, g.U, g.k, g.L, g.T) if g.G > 1 else ExplaiNN(g.U, g.k, g.L, g.T)
    m.cuda()
    m.load_state_dict(state)
    dev = m._device()
    with torch.cuda.device(dev):
        m._context(cap, dev)
    return m


def _snapshot(m):
    return collections.OrderedDict((k, v.detach().clone()) for k, v in m.state_dict().items())


def _to_device(d):
    return {k: _to_device(v) if isinstance(v, dict) else torch.from_numpy(v).cuda() for k, v in d.items()}


def _cap(m):
    return m._rt.ctx.max_batch


def _targets(g, y, logits):
    return y[:, None, :].expand_as(logits) if g.G > 1 else y


def _zero_grads(m):
    for p in m.parameters():
        p.grad = None


def _edited(d, rc, B):
    from explainn_amd.architectures import EditedWindows
    e = d["edits"]
    return EditedWindows(d["seq"], e["row_start"], e["row_edit"], e["pos"], e["ref_len"], e["alt_len"], e["alt_off"],
                         e["alt"], reverse_complement=rc, sub_batch=B)


def _haplotypes(d, rc, B):
    from explainn_amd.architectures import HaplotypeWindows
    h = d["haps"]
    return HaplotypeWindows(d["seq"], h["row_start"], h["row_first"], h["row_count"], h["edit_index"], h["pos"],
                            h["ref_len"], h["alt_len"], h["alt_off"], h["alt"], reverse_complement=rc, sub_batch=B)


def _raw(m, B):
    """(context of at least B, params table, its tensors, stream) for calls at the C ABI; the token moves
    as it does in the front half of every launch of the Python layer."""
    dev = m._device()
    m._rt.token += 1
    with torch.cuda.device(dev):
        ctx = m._context(B, dev)
        ps, keep = m._params_struct(dev)
    return ctx, ps, keep, m._stream(dev)


# ---- the op classes ---------------------------------------------------------------------------
def _step(m, g, B, d, seed, split):
    from explainn_amd.engine import StepEngine
    m.train()
    m.dropout_p = 0.3
    eng = StepEngine(m, _cap(m), loss="binary")
    logits, loss = eng.step(d["x"], d["y"], seed=seed, grad_sync=_NoSync() if split else None)
    return {"logits": logits.clone(), "loss": loss.clone(), "flat_grad": eng.flat_grad.clone()}


def _autograd(m, g, B, d, seed, kind):
    m.train()
    m.dropout_p = 0.3
    _zero_grads(m)
    x = d["x"]
    if kind == "mask":
        m.set_dropout_mask(d["mask"])
    else:
        torch.manual_seed(seed)                 # the built-in generator's seed is drawn from torch's
    if kind == "dx":
        x = x.clone().requires_grad_(True)
    try:
        logits = m(x)
    finally:
        m._rt.pending = None                    # (a mask the forward did not consume must not reach the next one)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, _targets(g, d["y"], logits))
    loss.backward()
    out = collections.OrderedDict(logits=logits.detach().clone(), loss=loss.detach().clone())
    for key, p in m.named_parameters():
        out["grad " + key] = p.grad.clone()
    if kind == "dx":
        out["x.grad"] = x.grad.clone()
    _zero_grads(m)
    return out


def _train_nograd(m, g, B, d, seed):
    m.train()
    m.dropout_p = 0.3
    torch.manual_seed(seed)
    with torch.no_grad():
        logits = m(d["x"])
    ctx, dev = m._rt.ctx, m._device()
    bits = torch.zeros(m._units(), B, 4, device=dev, dtype=torch.int32)
    _L().check(ctx.lib.explainn_debug_keep_bits(ctx.handle, B, bits.data_ptr(), m._stream(dev)))
    return {"logits": logits, "keep_bits": bits}


def _eval(m, x):
    m.eval()
    with torch.no_grad():
        return m(x)


def _eval_codes(m, g, B, d, seed):
    from explainn_amd.architectures import BaseCodes
    return {"forward": _eval(m, BaseCodes(d["codes"], False)), "reverse": _eval(m, BaseCodes(d["codes"], True))}


def _eval_soft(m, g, B, d, seed):
    m.dense_input = True
    try:
        return {"logits": _eval(m, d["soft"])}
    finally:
        m.dense_input = None


def _ig(m, g, B, d, seed, shuffle):
    from explainn_amd.architectures import BaseCodes
    from explainn_amd.sequence import dinucleotide_shuffle_device
    m.eval()
    if shuffle:
        base = dinucleotide_shuffle_device(d["codes"], 1, seed)[:, 0, :].contiguous()
        ig, lx, lb = m.integrated_gradients(BaseCodes(d["codes"]), d["dl"], base, steps=IG_STEPS)
    else:
        ig, lx, lb = m.integrated_gradients(d["x"], d["dl"], "zero", steps=IG_STEPS)
    return {"ig": ig, "logits_x": lx, "logits_base": lb}


def _scan(m, g, B, d, seed):
    from explainn_amd.architectures import SequenceWindows
    m.eval()
    win = SequenceWindows(d["seq"], -3, B, 7, reverse_complement=bool(seed & 1), sub_batch=B)
    return {"windows": m._launch_scan(win, _L().SCAN_WINDOWS), "shared": m._launch_scan(win, _L().SCAN_SHARED)}


def _score(m, g, B, d, seed, haps):
    m.eval()
    rc = bool(seed & 1)
    if haps:
        logits, outs = m._launch_score_haplotypes(_haplotypes(d, rc, B), want_outs=True)
    else:
        logits, outs = m._launch_score_edits(_edited(d, rc, B), want_outs=True)
    return {"logits": logits, "outs": outs}


def _call_sites(m, g, B, d, seed):
    m.eval()
    pos = torch.zeros(SITE_CAPACITY, device="cuda", dtype=torch.int32)
    score = torch.zeros(SITE_CAPACITY, device="cuda", dtype=torch.float32)
    off, pos, score = m._launch_call_sites(d["seq"], d["thresholds"], capacity=SITE_CAPACITY, pos=pos, score=score,
                                           reverse_complement=bool(seed & 1))
    return {"offsets": off, "pos": pos, "score": score}


def _record_best(m, g, B, d, seed):
    m.eval()
    bits, site = m._launch_record_best(d["seq"], d["rec_offsets"], strands=2)
    return {"best_bits": bits, "best_site": site}


def _act_histogram(m, g, B, d, seed):
    m.eval()
    hist = torch.zeros(m._units(), _L().ACT_BINS, device="cuda", dtype=torch.int64)
    return {"hist": m._launch_activation_histogram(d["seq"], hist, reverse_complement=bool(seed & 1))}


def _filter_export(m, g, B, d, seed):
    m.eval()
    U = m._units()
    unit_max = torch.zeros(U, device="cuda")
    m.filter_act_max(d["x"], unit_max, d["select"])
    thresholds = (unit_max * 0.5).contiguous()
    total = torch.zeros(U, device="cuda", dtype=torch.int32)
    pfm = torch.zeros(U, g.k, 4, device="cuda", dtype=torch.int32)
    hit = m.filter_sites(d["x"], thresholds, total, pfm, d["select"], site_cap=50, want_hit=True)
    return {"unit_max": unit_max, "site_total": total, "pfm": pfm, "hit": hit}


def _sync_step(m, g, B, d, seed):
    from explainn_amd.engine import StepEngine
    m.train()
    m.dropout_p = 0.3
    eng = StepEngine(m, _cap(m), loss="binary")
    for _ in eng.sync_phases(d["x"], d["y"], B, seed=seed):
        pass                                    # one rank: the sum over the ranks is the buffer itself
    return {"logits": eng.logits[:B].clone(), "loss": eng.loss.clone(), "flat_grad": eng.flat_grad.clone()}


def _staged_raw(m, g, B, d, seed):
    from explainn_amd.engine import flat_grads
    lib_, chk = _L(), _L().check
    ctx, ps, keep, s = _raw(m, B)
    lib, h, dev, rc = ctx.lib, ctx.handle, m._device(), seed & 1
    seq, n = d["seq"].data_ptr(), d["seq"].numel()
    out = collections.OrderedDict()
    with torch.cuda.device(dev):
        chk(lib.explainn_dense_input(h, 0))
        out["windows logits"] = m._logits_empty(B, dev)
        chk(lib.explainn_stage_windows(h, seq, n, -3, 7, B, rc, s))
        chk(lib.explainn_forward_eval(h, None, B, C.byref(ps), out["windows logits"].data_ptr(), s))
        ew = _edited(d, bool(rc), B)
        ed = ew.struct()
        out["edited outs"] = torch.empty(B, m._units(), device=dev)
        chk(lib.explainn_stage_edited_windows(h, seq, n, C.byref(ed), 0, B, rc, s))
        chk(lib.explainn_unit_outputs(h, None, B, C.byref(ps), out["edited outs"].data_ptr(), s))
        hw = _haplotypes(d, bool(rc), B)
        hp = hw.struct()
        out["train logits"] = m._logits_empty(B, dev)
        chk(lib.explainn_stage_haplotype_windows(h, seq, n, C.byref(hp), 0, B, rc, s))
        try:
            chk(lib.explainn_forward_train(h, None, B, C.byref(ps), None, 0.3, C.c_uint64(seed),
                                           out["train logits"].data_ptr(), s))
        finally:
            m._touched()
            m._rt.token += 1
        out["loss"] = torch.zeros(g.G, device=dev)
        dl = torch.empty_like(out["train logits"])
        chk(lib.explainn_loss_grad(h, lib_.LOSS_BCE_WITH_LOGITS, out["train logits"].data_ptr(), d["y"].data_ptr(), B,
                                   out["loss"].data_ptr(), dl.data_ptr(), s))
        flat, _, gs = flat_grads(list(m.parameters()), dev, zero=True)
        chk(lib.explainn_backward(h, dl.data_ptr(), B, C.byref(ps), C.byref(gs), 0, s))
        out["dlogits"], out["flat_grad"] = dl, flat
    return out


# ---- the point events -------------------------------------------------------------------------
def _err_arg(m, g, B, d, seed):
    from explainn_amd.architectures import SequenceWindows
    m.eval()
    return m._launch_scan(SequenceWindows(d["seq"], 0, B, 5, sub_batch=B), _L().SCAN_SHARED)


def _err_state_conv(m, g, B, d, seed):
    from explainn_amd.engine import flat_grads
    ctx, ps, keep, s = _raw(m, B)
    _, _, gs = flat_grads(list(m.parameters()), m._device(), zero=True)
    _L().check(ctx.lib.explainn_train_step_conv(ctx.handle, B, C.byref(ps), C.byref(gs), 0, s))


def _err_state_backward(m, g, B, d, seed):
    from explainn_amd.engine import flat_grads
    m.train()
    m.dropout_p = 0.0
    _zero_grads(m)
    out = m(d["x"])
    _eval(m, d["x"])                                # same B: the batch-size check alone would pass
    m.train()
    res = collections.OrderedDict()
    try:
        out.sum().backward()
        res["python"] = "no error"
    except RuntimeError as e:
        res["python"] = "%s: %s" % (type(e).__name__, e)
    _zero_grads(m)
    ctx, ps, keep, s = _raw(m, B)
    lib, h, dev = ctx.lib, ctx.handle, m._device()
    logits = m._logits_empty(B, dev)
    with torch.cuda.device(dev):
        _L().check(lib.explainn_dense_input(h, 0))
        _L().check(lib.explainn_forward_train(h, d["x"].data_ptr(), B, C.byref(ps), None, 0.0, C.c_uint64(0),
                                              logits.data_ptr(), s))
        m._touched()
        m._rt.token += 1
        _L().check(lib.explainn_forward_eval(h, d["x"].data_ptr(), B, C.byref(ps), logits.data_ptr(), s))
        _, _, gs = flat_grads(list(m.parameters()), dev, zero=True)
        dl = torch.ones_like(logits)
        res["rc"] = lib.explainn_backward(h, dl.data_ptr(), B, C.byref(ps), C.byref(gs), 0, s)
    res["message"] = lib.explainn_last_error().decode()
    assert res["rc"] == _L().E_STATE and "stale forward" in res["python"], res
    return res


def _err_unsupported(m, g, B, d, seed):
    m.eval()
    if g.G == 1:
        # the filter export has no dense form; the context is left in dense input mode
        m.dense_input = True
        try:
            return m.filter_act_max(d["soft"], torch.zeros(m._units(), device="cuda"))
        finally:
            m.dense_input = None
    ctx, ps, keep, s = _raw(m, B)
    lib, h, p = ctx.lib, ctx.handle, C.byref(ps)
    calls = {
        "explainn_forward_eval_keep": lambda: lib.explainn_forward_eval_keep(h, None, B, p, None, s),
        "explainn_input_grad": lambda: lib.explainn_input_grad(h, None, B, p, None, s),
        "explainn_backward_input": lambda: lib.explainn_backward_input(h, None, B, p, None, 0, None, s),
        "explainn_ism": lambda: lib.explainn_ism(h, None, B, p, None, None, None, 0, s),
        "explainn_integrated_gradients": lambda: lib.explainn_integrated_gradients(h, None, B, p, 0, None, None, 1, None,
                                                                                    None, None, None, 0, s),
        "explainn_sync_phase": lambda: lib.explainn_sync_phase(h, 1, None, None, None, s),
    }
    res = collections.OrderedDict()
    for name in hm.BANK_UNSUPPORTED:
        rc = calls[name]()
        assert rc == _L().E_UNSUPPORTED, (name, rc)
        res[name] = lib.explainn_last_error().decode()
    return res


def _err_not_onehot(m, g, B, d, seed):
    m.dense_input, m.validate_input = False, "always"
    try:
        return _eval(m, d["soft"])
    finally:
        m.dense_input, m.validate_input = None, True


def _mode_switch(m, g, B, d, seed):
    from explainn_amd.architectures import BaseCodes
    out = _eval_soft(m, g, B, d, seed)
    out["codes"] = _eval(m, BaseCodes(d["codes"], True))
    out["onehot"] = _eval(m, d["x"])
    out["flags"] = m.input_flags()
    return out


RUN = {
    "step_fused": lambda *a: _step(*a, split=False),
    "step_split": lambda *a: _step(*a, split=True),
    "train_mask": lambda *a: _autograd(*a, kind="mask"),
    "train_seed": lambda *a: _autograd(*a, kind="seed"),
    "train_dx": lambda *a: _autograd(*a, kind="dx"),
    "train_nograd": _train_nograd,
    "eval_onehot": lambda m, g, B, d, seed: {"logits": _eval(m, d["x"])},
    "eval_codes": _eval_codes,
    "eval_soft": _eval_soft,
    "input_grad": lambda m, g, B, d, seed: {"dx": (m.eval(), m.input_gradient(d["x"], d["dl"]))[1]},
    "ism": lambda m, g, B, d, seed: dict(zip(("logits", "delta"), (m.eval(), m.in_silico_mutagenesis(d["x"]))[1])),
    "ig_zero": lambda *a: _ig(*a, shuffle=False),
    "ig_shuffle": lambda *a: _ig(*a, shuffle=True),
    "scan": _scan,
    "score_edits": lambda *a: _score(*a, haps=False),
    "score_haplotypes": lambda *a: _score(*a, haps=True),
    "call_sites": _call_sites,
    "record_best": _record_best,
    "act_histogram": _act_histogram,
    "unit_outputs": lambda m, g, B, d, seed: {"outs": (m.eval(), m.linears(d["x"]))[1]},
    "unit_activations": lambda m, g, B, d, seed: {"acts": (m.eval(), m.linears[:3](d["x"]))[1]},
    "filter_export": _filter_export,
    "sync_step": _sync_step,
    "staged_raw": _staged_raw,
    "err_arg": _err_arg,
    "err_state_conv": _err_state_conv,
    "err_state_backward": _err_state_backward,
    "err_unsupported": _err_unsupported,
    "err_not_onehot": _err_not_onehot,
    "mode_switch": _mode_switch,
}
_TRAIN_B1 = hm.TRAIN_CLASSES + ("err_state_backward",)
# the point events that must raise, and what
RAISES = {"err_arg": "ExplainnError", "err_state_conv": "ExplainnError", "err_not_onehot": "ValueError"}


def test_every_name_of_the_model_has_a_runner():
    assert set(RUN) == set(hm.OP_CLASSES) | set(hm.POINT_EVENTS)


# ---- running and comparing --------------------------------------------------------------------
def _outcome(cls, m, g, B, d, seed):
    """What the op returned -- {name: tensor or plain value} -- or {"raised": "Type: message"}."""
    try:
        out = RUN[cls](m, g, B, d, seed)
    except (ValueError, RuntimeError) as e:
        # the error is the op's result -- where the model expects one: a point event that fails, or a
        # train-mode batch of one sequence; anything else is a fault of the op or of this test
        if not (cls in RAISES or cls == "err_unsupported" or (B == 1 and cls in _TRAIN_B1)):
            raise
        out = {"raised": "%s: %s" % (type(e).__name__, e)}
        m._rt.pending = None
        _zero_grads(m)
    if cls in RAISES:
        assert str(out.get("raised", "")).startswith(RAISES[cls]), "%s must raise %s, got %r" % (cls, RAISES[cls], out)
        if cls == "err_arg":
            assert "(code %d)" % _L().E_ARG in out["raised"]
        if cls == "err_state_conv":
            assert "(code %d)" % _L().E_STATE in out["raised"]
    if cls == "err_unsupported" and g.G == 1:
        assert "(code %d)" % _L().E_UNSUPPORTED in str(out.get("raised")), out
    return out if isinstance(out, dict) else {"result": out}


def _bits(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def _differences(got, ref, what=""):
    """Sentences naming what differs between two outcomes / state dicts; tensors compare as bit patterns."""
    out = []
    if list(got) != list(ref):
        return ["%sthe used context gave %s, the fresh one %s" % (what, list(got), list(ref))]
    for key in got:
        a, b = got[key], ref[key]
        if not torch.is_tensor(a) or not torch.is_tensor(b):
            if torch.is_tensor(a) or torch.is_tensor(b) or a != b:
                out.append("%s%s: used context %r, fresh context %r" % (what, key, a, b))
            continue
        if a.shape != b.shape or a.dtype != b.dtype:
            out.append("%s%s: %s %s against %s %s" % (what, key, a.dtype, tuple(a.shape), b.dtype, tuple(b.shape)))
        elif not torch.equal(_bits(a), _bits(b)):
            bad = (_bits(a) != _bits(b)).reshape(-1).nonzero()
            i = int(bad[0])
            idx = tuple(int(v) for v in np.unravel_index(i, tuple(a.shape))) if a.dim() else ()
            out.append("%s%s: %d of %d elements differ, first at %s: used context %r, fresh context %r" % (
                what, key, bad.numel(), a.numel(), idx, a.reshape(-1)[i].item(), b.reshape(-1)[i].item()))
    return out


class _Driver:
    """One long-lived model A and the comparison of each of its ops with a fresh twin."""

    def __init__(self, g):
        self.g = g
        self.A = _fresh(g, _initial_state(g), g.cap)
        self.prev = "a fresh context"
        self.spy = None

    def compare(self, cls, B, seed, where, settings=None):
        g, A = self.g, self.A
        B_ctx = 1 if cls in hm.NO_BATCH else B
        d = _to_device(hm.build_inputs(g, B, seed))
        F = _fresh(g, _snapshot(A), max(_cap(A), B_ctx))
        for m in (A, F):
            for key, v in (settings or {}).items():
                setattr(m, key, v)
        got = _outcome(cls, A, g, B, d, seed)
        ref = _outcome(cls, F, g, B, d, seed)
        torch.cuda.synchronize()
        diff = _differences(got, ref) + _differences(A.state_dict(), F.state_dict(), "state_dict ")
        if _cap(A) != _cap(F):
            diff.append("max_batch %d on the used context, %d on the fresh one" % (_cap(A), _cap(F)))
        assert not diff, "%s: %s (B = %d, seed %d) after %s is not what a fresh context of max_batch %d gives:\n  %s" % (
            where, cls, B, seed, self.prev, _cap(F), "\n  ".join(diff))
        self.prev = "%s (B = %d)" % (cls, B)
        return F

    def mutate(self, route, where, seed):
        """Change A's parameters inside an eval_cache() scope by one of history_model.CACHE_ROUTES."""
        A = self.A
        if route == "inplace":
            with torch.no_grad():
                A.linears[0].weight.mul_(1.05)
                A.linears[7].running_var.add_(0.05)
        elif route == "train_step":
            self.compare("step_fused", 70, seed + 7, where + " [route train_step]")
        elif route == "adam":
            from explainn_amd import get_optimizer
            opt = get_optimizer(A.parameters(), 0.01)
            for i, p in enumerate(A.parameters()):
                p.grad = torch.full_like(p, 0.01 * (1 + i % 3))
            opt.step()
            _zero_grads(A)
        elif route == "load_state_dict":
            sd = _snapshot(A)
            sd["final.weight"] = sd["final.weight"] * 0.9
            sd["linears.1.running_mean"] = sd["linears.1.running_mean"] + 0.02
            A.load_state_dict(sd)
        elif route == "reassign":
            A.final.weight = torch.nn.Parameter(A.final.weight.detach() * 1.1)
        elif route == "data_invalidate":
            A.final.weight.data.mul_(-1.0)
            A.linears[0].weight.data[1] += 0.05
            A.invalidate()
        else:
            raise AssertionError("unknown cache route %r" % route)
        self.prev += " + parameters changed by %s" % route

    def grow(self, it, where):
        """Run the item's op at max_batch + 1: the context is closed and re-created inside the op."""
        B = _cap(self.A) + 1
        if it.cls in hm.NO_BATCH:               # takes no batch: an eval forward grows the context in front of it
            self.compare("eval_onehot", B, it.seed + 3, where + " [growth]")
            assert _cap(self.A) == B
            return self.compare(it.cls, it.B, it.seed, where)
        self.compare(it.cls, B, it.seed, where)
        assert _cap(self.A) == B

    def item(self, it, where):
        g, A = self.g, self.A
        if it.mod is None:
            self.compare(it.cls, it.B, it.seed, where)
        elif it.mod in ("cache_none", "cache_change"):
            with A.eval_cache():
                self.compare("eval_onehot", 70, it.seed + 1, where + " [eval forward that fills the tables]")
                if it.mod == "cache_change":
                    self.mutate(it.route, where, it.seed)
                self.compare(it.cls, it.B, it.seed, where + " [inside eval_cache()]")
                self.compare("eval_onehot", 70, it.seed + 1, where + " [eval forward after it, same scope]")
        elif it.mod == "pending_flag":
            # a bad batch whose validation is deferred: it is packed inside the launch, its columns read as
            # N, and the flag it raises stays on the device
            A.validate_input = False
            _eval(A, _to_device(hm.build_inputs(g, 70, it.seed + 2))["soft"])
            self.prev += " + a deferred bad batch"
            if it.cls in hm.READS_FLAG_FIRST:
                assert A.input_flags() & 1, where + ": the deferred batch raised no flag"
                A.validate_input = True
                self.compare(it.cls, it.B, it.seed, where)
            else:
                F = self.compare(it.cls, it.B, it.seed, where, settings={"validate_input": False})
                assert A.input_flags() & 1, where + ": the pending flag was lost while %s ran" % it.cls
                assert F.input_flags() == 0
                A.validate_input = True
            assert A.input_flags() == 0, where + ": the flag was not cleared by its read"
        elif it.mod == "growth":
            self.grow(it, where)
        elif it.mod == "growth_pending":
            A.train()
            A.dropout_p = 0.0
            pending = A(_to_device(hm.build_inputs(g, 64, it.seed + 4))["x"])
            self.prev += " + a train forward left pending"
            self.grow(it, where)
            A.train()
            # the host-side token check: it precedes every launch of _launch_backward
            with pytest.raises(RuntimeError, match="stale forward"):
                pending.sum().backward()
            _zero_grads(A)
        else:
            raise AssertionError("unknown modifier %r" % it.mod)


def _set_env(monkeypatch, g):
    for key in ("EXPLAINN_QCH", "EXPLAINN_ACH", "EXPLAINN_HEAD_PARTIALS", "EXPLAINN_BN1_AUX"):
        monkeypatch.delenv(key, raising=False)
    for key, v in g.env.items():
        monkeypatch.setenv(key, v)


@pytest.mark.parametrize("name", list(hm.GEOMETRIES))
def test_fresh_contexts_agree(name, monkeypatch):
    """The premise of the exact comparison: every op class and point event gives equal bits on two fresh
    contexts of equal capacity, at the largest batch and at a ragged one.  While at it, the op is seen to
    call the entry points history_model.OP_CLASSES / POINT_EVENTS say it drives."""
    g = hm.GEOMETRIES[name]
    _set_env(monkeypatch, g)
    spy = _Spy(_L().load())
    monkeypatch.setattr(_L(), "_lib", spy)
    state = _initial_state(g)
    declared = dict(hm.OP_CLASSES)
    declared.update(hm.POINT_EVENTS)
    not_reproducible, not_driven = [], []
    for cls in list(g.classes) + list(hm.POINT_EVENTS):
        for B in (g.cap, 70):
            d = _to_device(hm.build_inputs(g, B, 500 + B))
            one, two = _fresh(g, state, g.cap), _fresh(g, state, g.cap)
            spy.calls.clear()
            a = _outcome(cls, one, g, B, d, 500 + B)
            called = set(spy.calls)
            b = _outcome(cls, two, g, B, d, 500 + B)
            torch.cuda.synchronize()
            diff = _differences(a, b) + _differences(one.state_dict(), two.state_dict(), "state_dict ")
            if diff:
                not_reproducible.append("%s (B = %d): %s" % (cls, B, "; ".join(diff)))
            want = set(declared[cls][0])
            if cls == "err_unsupported" and g.G > 1:
                want = set(hm.BANK_UNSUPPORTED)
            if want - called:
                not_driven.append("%s (B = %d) did not call %s" % (cls, B, sorted(want - called)))
    assert not not_driven, "\n".join(not_driven)
    assert not not_reproducible, "not bitwise reproducible on two fresh contexts:\n" + "\n".join(not_reproducible)


RUNS = [(name, i) for name, g in hm.GEOMETRIES.items() for i in range(len(hm.segments(g)))]


@pytest.mark.parametrize("name,run", RUNS, ids=["%s-run%d" % r for r in RUNS])
def test_call_history(name, run, monkeypatch):
    g = hm.GEOMETRIES[name]
    _set_env(monkeypatch, g)
    drv = _Driver(g)
    for it in hm.segments(g)[run]:
        where = "%s walk, position %d%s" % (name, it.pos, " under %s%s" % (it.mod, ":" + it.route if it.route else "")
                                            if it.mod else "")
        drv.item(it, where)
