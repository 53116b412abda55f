"""GPU: the fused Adam (csrc/adam.hip through explainn_adam_step, and optim.FusedAdam) at the edges of
its own constants: sizes around ADAM_CHUNK = 2048, more than ADAM_MAX_TENSORS = 32 tensors (several
tables), empty tensors, extreme step counts and gradient magnitudes, argument errors.

Reference: one Adam step in fp64 numpy (the rule of oracle.explainn_oracle.adam_step, written out for
a list of flat arrays and an arbitrary prior state).  Tolerance, the suite's convention:
torch.optim.Adam runs in fp32 from the same state on the same case; the kernel passes when its error
against the fp64 truth is within 3x torch's, per quantity -- parameters relative to max|p|, exp_avg
and exp_avg_sq relative to their own max, each maximum taken over all tensors of the call.

Guard bands: every p, g, m and v handed to the C ABI is a view into one device buffer with 64 sentinel
floats in front of it and behind it.  After the step every sentinel must hold its bit pattern and the
gradients must be unchanged, so a store one element past a tensor fails the test."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import record_margin  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
LR, B1, B2, EPS = 0.003, 0.9, 0.999, 1e-8
CHUNK, MAX_TENSORS = 2048, 32                                                # csrc/adam.hip


class Arena:
    """p, g, m, v of every tensor as views into one device buffer, each between two guard bands."""

    def __init__(self, host):
        """host: {"p"|"g"|"m"|"v": list of float32 arrays}."""
        self.sizes = [len(a) for a in host["p"]]
        self.off = {}
        at = 0
        for q in "pgmv":
            for i, n in enumerate(self.sizes):
                self.off[q, i] = at + GUARD
                at += GUARD + n
        at += GUARD
        # finite and all different: a step run on guard floats (g, m, v and p one past the end) changes
        # them, where equal values or NaNs could come back as the bit pattern they had
        self.before = (1e3 * np.random.default_rng(at).standard_normal(at)).astype(np.float32)
        self.data = np.zeros(at, dtype=bool)
        for (q, i), o in self.off.items():
            self.before[o:o + self.sizes[i]] = host[q][i]
            self.data[o:o + self.sizes[i]] = True
        self.buf = torch.from_numpy(self.before.copy()).cuda()
        self.base = self.buf.data_ptr()

    def ptrs(self, q, null_empty=True):
        n = len(self.sizes)
        return (C.c_void_p * n)(*[None if (null_empty and self.sizes[i] == 0) else self.base + 4 * self.off[q, i]
                                  for i in range(n)])

    def step(self, step, sizes=None, n=None, **over):
        from explainn_amd import _lib
        cnt = len(self.sizes) if n is None else n
        sz = (C.c_int64 * len(self.sizes))(*(self.sizes if sizes is None else sizes))
        arrs = {q: over.get(q, self.ptrs(q)) for q in "pgmv"}
        rc = _lib.load().explainn_adam_step(cnt, arrs["p"], arrs["g"], arrs["m"], arrs["v"], sz, step, LR, B1, B2,
                                            EPS, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def after(self):
        return self.buf.cpu().numpy()

    def get(self, after, q):
        return [after[self.off[q, i]:self.off[q, i] + n] for i, n in enumerate(self.sizes)]

    def check_guards(self, after, what):
        a, b = after.view(np.uint32), self.before.view(np.uint32)
        bad = np.flatnonzero((a != b) & ~self.data)
        assert bad.size == 0, "%s: %d guard floats overwritten, first at buffer offset %d" % (what, bad.size, bad[0])
        for i, n in enumerate(self.sizes):
            o = self.off["g", i]
            assert np.array_equal(a[o:o + n], b[o:o + n]), "%s: gradient %d was written" % (what, i)

    def unchanged(self, after):
        return np.array_equal(after.view(np.uint32), self.before.view(np.uint32))


def adam64(p, g, m, v, step):
    """One step of torch.optim.Adam's rule (no weight decay, no amsgrad) in fp64."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m = B1 * m + (1 - B1) * g
    v = B2 * v + (1 - B2) * g * g
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    return p - (LR / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + EPS), m, v


def torch32(host, step):
    """torch.optim.Adam in fp32 on the device from the same state: lists (p, m, v) of numpy arrays."""
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).cuda()) for a in host["p"]]
    opt = torch.optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS)
    for p, g, m, v in zip(ps, host["g"], host["m"], host["v"]):
        p.grad = torch.from_numpy(g.copy()).cuda()
        opt.state[p] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.copy()).cuda(),
                        "exp_avg_sq": torch.from_numpy(v.copy()).cuda()}
    opt.step()
    return ([p.detach().cpu().numpy() for p in ps], [opt.state[p]["exp_avg"].cpu().numpy() for p in ps],
            [opt.state[p]["exp_avg_sq"].cpu().numpy() for p in ps])


def _err(got, truth):
    """max|got - truth| over all tensors of the call, relative to max|truth| over all of them."""
    num = max((np.abs(a.astype(np.float64) - t).max() for a, t in zip(got, truth) if t.size), default=0.0)
    den = max((np.abs(t).max() for t in truth if t.size), default=0.0)
    return num / den if den > 0 else num


def make(sizes, seed, state="random", grad=None):
    """Host arrays of a case.  state: "zero", "random" (exp_avg of random sign) or "opposite" (exp_avg of
    the opposite sign to the gradient); grad: None for standard normal, or a function (rng, n) -> array."""
    r = np.random.default_rng(seed)
    host = {q: [] for q in "pgmv"}
    for n in sizes:
        g = r.standard_normal(n) if grad is None else grad(r, n)
        host["p"].append(r.standard_normal(n))
        host["g"].append(g)
        if state == "zero":
            m, v = np.zeros(n), np.zeros(n)
        else:
            m = 0.3 * r.standard_normal(n)
            if state == "opposite":
                m = -np.sign(g) * np.abs(m)
            v = (0.5 * r.standard_normal(n)) ** 2
        host["m"].append(m)
        host["v"].append(v)
    return {q: [np.asarray(a, dtype=np.float32) for a in host[q]] for q in "pgmv"}


def run_and_compare(what, host, step):
    """The C ABI step on guarded views of `host` against fp64, at 3x torch-fp32's own error."""
    arena = Arena(host)
    assert arena.step(step) == 0, what
    after = arena.after()
    arena.check_guards(after, what)
    live = [i for i, n in enumerate(arena.sizes) if n > 0]
    pick = lambda lst: [lst[i] for i in live]                                 # noqa: E731
    live_host = {q: pick(host[q]) for q in "pgmv"}
    truth = list(zip(*[adam64(p, g, m, v, step) for p, g, m, v in zip(*[live_host[q] for q in "pgmv"])]))
    ref32 = torch32(live_host, step)
    problems = []
    for qi, (q, label) in enumerate((("p", "param"), ("m", "exp_avg"), ("v", "exp_avg_sq"))):
        got = pick(arena.get(after, q))
        assert all(np.isfinite(a).all() for a in got), (what, label)
        mine, theirs = _err(got, truth[qi]), _err(ref32[qi], truth[qi])
        print("%s %s: kernel %.3e  torch fp32 %.3e" % (what, label, mine, theirs))
        record_margin("adam %s %s torch-fp32 itself" % (what, label), theirs, max(3 * theirs, 1e-300))
        record_margin("adam %s %s (bound 3x torch-fp32)" % (what, label), mine, max(3 * theirs, 1e-300))
        if mine > 3 * theirs:
            problems.append("%s: kernel %.3e > 3 x torch fp32 %.3e" % (label, mine, theirs))
    assert not problems, what + ": " + "; ".join(problems)
    return arena, after


# ---- C ABI -------------------------------------------------------------------------------------------
def test_sizes_around_the_chunk():
    sizes = [1, 255, 256, 2047, 2048, 2049, 4096, 4097]
    assert {CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1} <= set(sizes)
    run_and_compare("chunk edges", make(sizes, 1), step=2)


@pytest.mark.parametrize("n", [33, 65])
def test_more_tensors_than_one_table(n):
    """2 and 3 tables; most tensors are one block, some two; the last table holds a single tensor."""
    r = np.random.default_rng(n)
    sizes = [int(s) for s in r.integers(1, 400, size=n)]
    sizes[3], sizes[31], sizes[32] = CHUNK + 1, CHUNK, 2 * CHUNK + 5
    assert -(-n // MAX_TENSORS) == (2 if n == 33 else 3) and n % MAX_TENSORS == 1
    arena, after = run_and_compare("%d tensors" % n, make(sizes, 10 + n), step=3)
    # every tensor moved exactly once: none skipped (a table starting over would leave the tail as it was)
    for i, (a, b) in enumerate(zip(arena.get(after, "p"), arena.get(arena.before, "p"))):
        assert not np.array_equal(a, b), "tensor %d was not updated" % i


def test_empty_tensors_take_no_slot():
    n = 70
    empty = {0, 5, 6, 7, 32, 33, n - 1}
    r = np.random.default_rng(5)
    sizes = [0 if i in empty else int(s) for i, s in enumerate(r.integers(1, 300, size=n))]
    sizes[40] = CHUNK + 3
    assert n - len(empty) > MAX_TENSORS
    arena, after = run_and_compare("empty tensors", make(sizes, 6), step=4)
    assert all(p is None for i, p in enumerate(arena.ptrs("p")) if i in empty)
    for i, (a, b) in enumerate(zip(arena.get(after, "p"), arena.get(arena.before, "p"))):
        assert i in empty or not np.array_equal(a, b), "tensor %d was not updated" % i


def test_nothing_to_do_is_ok_and_touches_nothing():
    from explainn_amd import _lib
    arena = Arena(make([0, 0, 0, 0, 0], 7))
    assert arena.step(1) == _lib.OK                                          # all empty, null pointers
    arena2 = Arena(make([300, 17], 8))
    assert arena2.step(1, n=0) == _lib.OK                                    # n_tensors = 0 with tables given
    rc = _lib.load().explainn_adam_step(0, None, None, None, None, None, 1, LR, B1, B2, EPS, None)
    assert rc == _lib.OK                                                     # ... and without
    torch.cuda.synchronize()
    assert arena.unchanged(arena.after()) and arena2.unchanged(arena2.after())


@pytest.mark.parametrize("step", [1, 2, 1000, 10 ** 6])
def test_step_counts(step):
    run_and_compare("step %d" % step, make([CHUNK + 1, 300], 20 + step % 7), step=step)


def _magnitudes(scales):
    def grad(r, n):
        return r.choice(scales, size=n) * r.choice([-1.0, 1.0], size=n)
    return grad


@pytest.mark.parametrize("scales", [(0.0, 1e-30, 1e-10, 1.0, 1e4), (1e-30,), (1e-10,), (1e4,), (0.0,)],
                         ids=["mixed", "1e-30", "1e-10", "1e4", "zero"])
def test_gradient_magnitudes_from_zero_state(scales):
    """First step from zero state: denom = |g| + eps, so a zero or tiny gradient divides by eps alone.
    g^2 = 1e8 stays far below fp32 overflow; 1e-60 underflows to zero in fp32 in the kernel and in
    torch alike, which exp_avg_sq's own scale shows only in the tensors that hold nothing larger."""
    host = make([700, CHUNK + 1], 30, state="zero", grad=_magnitudes(np.array(scales)))
    arena, after = run_and_compare("magnitudes %s" % (scales,), host, step=1)
    if scales == (0.0,):
        for q in "pmv":
            for a, b in zip(arena.get(after, q), arena.get(arena.before, q)):
                assert np.array_equal(a, b)


def test_prior_state_of_the_opposite_sign():
    host = make([CHUNK - 1, 513], 40, state="opposite")
    assert all((np.sign(m) == -np.sign(g)).all() for m, g in zip(host["m"], host["g"]))
    run_and_compare("opposite-sign exp_avg", host, step=5)


@pytest.mark.parametrize("slot", [0, 40])
@pytest.mark.parametrize("error", ["step0", "negative_size", "null_pointer"])
def test_argument_errors_launch_nothing(error, slot):
    """E_ARG, and no tensor of the call is touched -- not even those of a table in front of the bad
    entry (slot 40 sits in the second table)."""
    from explainn_amd import _lib
    r = np.random.default_rng(9)
    arena = Arena(make([int(s) for s in r.integers(1, 200, size=45)], 50))
    if error == "step0":
        rc = arena.step(0)
    elif error == "negative_size":
        sizes = list(arena.sizes)
        sizes[slot] = -1
        rc = arena.step(1, sizes=sizes)
    else:
        m = arena.ptrs("m")
        m[slot] = None
        rc = arena.step(1, m=m)
    assert rc == _lib.E_ARG
    assert arena.unchanged(arena.after()), "a kernel ran before the argument error was reported"


# ---- FusedAdam ---------------------------------------------------------------------------------------
def test_fused_adam_plans_tables_and_late_parameters():
    """A trajectory next to torch.optim.Adam through every host path of optim.FusedAdam: 40 parameters
    (two tables), gradients refreshed in place (plan reuse) and replaced (plan rebuild), a parameter whose
    first gradient arrives at step 4 (per-tensor launches, its own step count), load_state_dict and
    add_param_group mid-run, a non-contiguous gradient in either group (torch's own step)."""
    from explainn_amd.optim import FusedAdam
    torch.manual_seed(11)
    shapes = [(CHUNK,), (CHUNK + 1,), (7, 3), (1,), (2 * CHUNK + 1,)] + [(int(n),) for n in
                                                                          torch.randint(1, 300, (35,))]
    assert len(shapes) == 40 > MAX_TENSORS
    pa = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes + [(33,)]]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa, ob = FusedAdam(pa, lr=LR), torch.optim.Adam(pb, lr=LR)
    late = len(pa) - 1
    it = [0]

    def step(in_place=False, with_late=True, transpose=None):
        it[0] += 1
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i == late and not with_late:
                continue
            g = torch.randn_like(a) * (10.0 ** ((it[0] + i) % 4 - 2))
            if i == transpose:
                g = torch.randn(a.shape[::-1], device="cuda").t()
                assert not g.is_contiguous()
            if in_place:
                a.grad.copy_(g); b.grad.copy_(g)
            else:
                a.grad, b.grad = g.clone() if i != transpose else g, g.clone()
        oa.step(); ob.step()
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert torch.allclose(a, b, rtol=2e-6, atol=2e-7), (it[0], i, float((a - b).detach().abs().max()))

    def same_state():
        sa, sb = oa.state_dict(), ob.state_dict()
        assert [g["params"] for g in sa["param_groups"]] == [g["params"] for g in sb["param_groups"]]
        assert sa["state"].keys() == sb["state"].keys()
        for i in sb["state"]:
            assert float(sa["state"][i]["step"]) == float(sb["state"][i]["step"]), (i, sa["state"][i]["step"])
            for k in ("exp_avg", "exp_avg_sq"):
                ref = sb["state"][i][k]
                assert torch.allclose(sa["state"][i][k], ref, rtol=2e-6, atol=1e-6 * float(ref.abs().max())), (i, k)
        return sa, sb

    step(with_late=False)
    plan = oa._plans[0]
    assert plan["uniform"] and plan["n"] == 40
    step(in_place=True, with_late=False)
    step(in_place=True, with_late=False)
    assert oa._plans[0] is plan and plan["count"] == 3              # reused, not rebuilt
    oa.zero_grad(set_to_none=True); ob.zero_grad(set_to_none=True)
    step()                                                          # fresh tensors, and the late parameter
    assert oa._plans[0] is not plan and not oa._plans[0]["uniform"]
    sa, _ = same_state()
    assert float(sa["state"][late]["step"]) == 1.0 and all(
        float(sa["state"][i]["step"]) == 4.0 for i in sa["state"] if i != late)
    step(in_place=True)
    _, sb = same_state()
    oa.load_state_dict(copy.deepcopy(sb))                           # torch's own state, mid-run
    step(); step(in_place=True)
    same_state()
    extra_a = [torch.nn.Parameter(torch.randn(CHUNK + 7, device="cuda")), torch.nn.Parameter(torch.randn(5, 4, device="cuda"))]
    extra_b = [torch.nn.Parameter(p.detach().clone()) for p in extra_a]
    oa.add_param_group({"params": extra_a}); ob.add_param_group({"params": extra_b})
    pa.extend(extra_a); pb.extend(extra_b)
    step(); step(in_place=True)
    sa, _ = same_state()
    assert float(sa["state"][len(pa) - 1]["step"]) == 2.0
    step(transpose=2)                                               # non-contiguous: torch's step, same numbers
    step()
    same_state()
    # ... and in the second group: the first group must not have been stepped by the kernel before
    # the whole step is handed to torch
    step(transpose=len(pa) - 1)
    step()
    same_state()
