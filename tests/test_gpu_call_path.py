"""The context-bound call path: _lib.Context.call / Context.workspace, ExplaiNN._launch and the _lib.require
checks of architectures.py.  -m gpu.

Everything here is either about what happens BEFORE a launch -- a refusal raises and leaves nothing enqueued or
pending -- or an exact comparison, so one tiny shape serves: ExplaiNN(3, 5, 24, 2) in eval mode (3 units: a ragged
unit quad; k < 7; two tasks), B = 3, and a seeded sequence of 120 base codes with a few N.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import scan_model as sm  # noqa: E402
import variants_model as vm  # noqa: E402

pytestmark = pytest.mark.gpu

U, K, L, T, B = 3, 5, 24, 2, 3
SEQ = 120
CAPACITY = 512             # above the U * (SEQ - K + 1) sites a threshold of 0 calls
IG_STEPS = 4


def _L():
    from explainn_amd import _lib
    return _lib


def _model(state=None):
    from explainn_amd import ExplaiNN
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        m = ExplaiNN(U, K, L, T)
    if state is not None:
        m.load_state_dict(state)
    return m.cuda().eval()


class _Data:
    def __init__(self):
        rng = np.random.default_rng(0)
        seq = rng.integers(0, 4, size=SEQ).astype(np.uint8)
        seq[[7, 8, 50, 101]] = 4
        self.seq = seq
        self.codes = torch.from_numpy(seq).cuda()
        self.rows = torch.from_numpy(np.stack([seq[s:s + L] for s in (0, 31, 96)])).cuda()      # (B, L) codes
        self.x = torch.from_numpy(sm.onehot(self.rows.cpu().numpy())).cuda()                     # (B, 4, L) fp32
        self.dlogits = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def data():
    return _Data()


@pytest.fixture(scope="module")
def used():
    """The model every refusal below is provoked on; the last test compares it with a fresh one."""
    return _model()


# ---- Context.call ------------------------------------------------------------------------------------
def _bad_logits(kind):
    if kind == "strided":
        return torch.empty(T, B, device="cuda").t()
    if kind == "host":
        return torch.empty(B, T)
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    return torch.empty(B, T, device="cuda:1")


@pytest.mark.parametrize("kind,says", [("strided", "strided"), ("host", "cpu"), ("other device", "cuda:1")])
def test_context_call_refuses_before_anything_is_enqueued(data, kind, says):
    m = _model()
    before = m(data.x).clone()
    bad = _bad_logits(kind)
    assert tuple(bad.shape) == (B, T)
    with pytest.raises(RuntimeError, match=r"explainn_forward_eval: argument 3 .*%s" % says):
        with m._launch(data.x, m._device()) as (ctx, ps, xp):
            ctx.call("explainn_forward_eval", xp, B, ps, bad)
    assert torch.equal(m(data.x), before)


# ---- the require()d arguments ------------------------------------------------------------------------
def _zeros(*shape, dtype):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def _good_args(entry, m):
    """Fresh, correct tensors for the checked arguments of `entry` (accumulators zeroed)."""
    if entry == "_launch_call_sites":
        return dict(thresholds=_zeros(U, dtype=torch.float32), pos=_zeros(CAPACITY, dtype=torch.int32),
                    score=_zeros(CAPACITY, dtype=torch.float32))
    if entry == "_launch_record_best":
        return dict(rec_offsets=torch.tensor([0, 40, 80, SEQ], dtype=torch.int64, device="cuda"))
    if entry == "_launch_activation_histogram":
        return dict(hist=_zeros(U, _L().ACT_BINS, dtype=torch.int64))
    if entry == "filter_sites":
        return dict(thresholds=_zeros(U, dtype=torch.float32), site_total=_zeros(U, dtype=torch.int32),
                    pfm=_zeros(U, K, 4, dtype=torch.int32))
    if entry == "filter_act_max":
        return dict(unit_max=_zeros(U, dtype=torch.float32))
    assert entry == "integrated_gradients"
    return dict(workspace=_zeros(m.integrated_gradients_workspace_bytes(64), dtype=torch.uint8))


def _run(entry, m, d, a):
    """One call of `entry` with the arguments `a`; returns every tensor it wrote."""
    if entry == "_launch_call_sites":
        offsets, pos, score = m._launch_call_sites(d.codes, a["thresholds"], capacity=CAPACITY, pos=a["pos"],
                                                   score=a["score"])
        return offsets, pos, score
    if entry == "_launch_record_best":
        return m._launch_record_best(d.codes, a["rec_offsets"])
    if entry == "_launch_activation_histogram":
        return (m._launch_activation_histogram(d.codes, a["hist"]),)
    if entry == "filter_sites":
        hit = m.filter_sites(d.x, a["thresholds"], a["site_total"], a["pfm"], want_hit=True)
        return hit, a["site_total"], a["pfm"]
    if entry == "filter_act_max":
        return (m.filter_act_max(d.x, a["unit_max"]),)
    return m.integrated_gradients(d.x, d.dlogits, steps=IG_STEPS, workspace=a["workspace"])


# (entry point, argument, whether its length is free: shape (None,))
CHECKED = [("_launch_call_sites", "thresholds", False), ("_launch_call_sites", "pos", True),
           ("_launch_call_sites", "score", True), ("_launch_record_best", "rec_offsets", True),
           ("_launch_activation_histogram", "hist", False), ("filter_sites", "thresholds", False),
           ("filter_sites", "site_total", False), ("filter_sites", "pfm", False),
           ("filter_act_max", "unit_max", False), ("integrated_gradients", "workspace", True)]
ENTRIES = list(dict.fromkeys(entry for entry, _, _ in CHECKED))


def _defect(t, kind, free):
    if kind == "dtype":
        return t.to(torch.float64 if t.dtype != torch.float64 else torch.float32)
    if kind == "shape":                     # one dimension more where any length goes, one row more elsewhere
        return t.reshape(*t.shape, 1) if free else torch.cat([t, t[:1]])
    if kind == "strided":
        return torch.stack([t, t], dim=-1)[..., 0]
    if kind == "host":
        return t.cpu()
    assert kind == "short" and free
    return t[:CAPACITY - 1]


REFUSALS = [(entry, arg, free, kind) for entry, arg, free in CHECKED for kind in ("dtype", "shape", "strided", "host")]
REFUSALS += [("_launch_call_sites", arg, True, "short") for arg in ("pos", "score")]


@pytest.mark.parametrize("entry,arg,free,kind", REFUSALS, ids=["%s-%s-%s" % (e, a, k) for e, a, _, k in REFUSALS])
def test_checked_argument_is_refused(used, data, entry, arg, free, kind):
    a = _good_args(entry, used)
    good = a[arg]
    a[arg] = _defect(good, kind, free)
    if kind in ("shape", "strided", "short"):
        assert a[arg].dtype == good.dtype and a[arg].device == good.device
        assert a[arg].is_contiguous() == (kind != "strided")
    with pytest.raises(RuntimeError, match=r"\b%s must " % arg):
        _run(entry, used, data, a)


@pytest.mark.parametrize("entry", ENTRIES)
def test_correct_call_after_the_refusals_equals_a_fresh_model(used, data, entry):
    fresh = _model(used.state_dict())
    got = _run(entry, used, data, _good_args(entry, used))
    want = _run(entry, fresh, data, _good_args(entry, fresh))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.equal(g, w), "%s: result %d differs" % (entry, i)
    if entry == "_launch_call_sites":
        assert 0 < int(got[0][-1]) <= CAPACITY          # sites were called, none dropped


# ---- structures by reference -------------------------------------------------------------------------
def test_score_edits_equals_the_host_cut(data):
    """Params and Edits go to explainn_score_edits as instances: two rows of the sequence, one untouched and
    one with a three-base replacement, against model(BaseCodes(rows)) on the rows cut and edited on the host."""
    from explainn_amd.architectures import BaseCodes, EditedWindows
    tab = dict(row_start=np.array([10, 60], np.int64), row_edit=np.array([-1, 0], np.int32),
               pos=np.array([70], np.int64), ref_len=np.array([2], np.int32), alt_len=np.array([3], np.int32),
               alt_off=np.array([0], np.int32), alt=np.array([3, 4, 0], np.uint8))
    rows = vm.edited_matrix(data.seq, L=L, **tab)
    assert rows.shape == (2, L) and not np.array_equal(rows[1], data.seq[60:60 + L])
    m = _model()
    dev = {k: torch.from_numpy(v).cuda() for k, v in tab.items()}
    got = m._launch_score_edits(EditedWindows(data.codes, **dev))
    want = m(BaseCodes(torch.from_numpy(np.ascontiguousarray(rows)).cuda()))
    assert torch.equal(got, want)


# ---- Context.workspace -------------------------------------------------------------------------------
def test_scan_with_an_unknown_mode_raises_explainn_error(data):
    from explainn_amd.architectures import SequenceWindows
    m = _model()
    win = SequenceWindows(data.codes, 0, 5, 1)
    with pytest.raises(_L().ExplainnError):
        m._launch_scan(win, mode=99)
    assert torch.equal(m._launch_scan(win), _model()._launch_scan(win))          # ... and the next scan works
