"""GPU: the filter -> PWM export (csrc/interpret.hip) and the PWM scan (csrc/pwm.hip) away from the
200 bp shape they were written at.

Export: the cases of tests/export_model.py -- several position chunks, k and U at their limits, the cap
inside a later chunk / an earlier batch / the reverse strand, units that overflow and underflow
float16 -- against the fp64 oracle rounded to float16 and oracle/interpret_oracle.py.  The cases hold
no float16 knife edge (tests/test_export_model.py), so every comparison is array_equal.

PWM scan: against oracle.explainn_oracle.pwm_scan in fp64 at the kernel's own bound,
1e-4 x max(1, max|ref|)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import export_model as em  # noqa: E402
from conftest import record_margin  # noqa: E402
from oracle import explainn_oracle as eo  # noqa: E402
from parity_util import model  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- export ------------------------------------------------------------------------------------------
def _net(c):
    sd, codes, idxs = em.inputs(c)
    return model(sd, c["U"], c["k"], c["L"], 1).eval(), em.onehot(codes), idxs


def _through_filter_sites(net, x, rows, thr16, cap, batch):
    """What interpret.filter_pwms does after its thresholds, with thresholds given: batches in order
    into one pair of accumulators."""
    U, k = net._options["cnn_units"], net._options["kernel_size"]
    N = len(x)
    sel = np.zeros(N, dtype=np.uint8)
    sel[rows] = 1
    select = torch.from_numpy(sel).cuda()
    thr = torch.from_numpy(thr16.astype(np.float32)).cuda()
    total = torch.zeros(U, device="cuda", dtype=torch.int32)
    pfm = torch.zeros(U, k, 4, device="cuda", dtype=torch.int32)
    hit = np.zeros((N, U), dtype=bool)
    with net.eval_cache():
        for i in range(0, N, batch):
            h = net.filter_sites(torch.from_numpy(x[i:i + batch]).cuda(), thr, total, pfm, select[i:i + batch],
                                 site_cap=cap, want_hit=True)
            hit[i:i + batch] = h.cpu().numpy().astype(bool)
    return {"thresholds": thr16, "pfm": pfm.cpu().numpy().astype(np.int64),
            "nsites": total.cpu().numpy().astype(np.int64), "hit": hit}


def _same(what, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = int((got != ref).sum())
    record_margin("exact " + what, bad, 1.0)
    assert bad == 0, "%s: %d of %d entries differ\n%s\n%s" % (what, bad, ref.size, got.reshape(-1)[:16], ref.reshape(-1)[:16])


@pytest.mark.parametrize("name", [c["name"] for c in em.CASES])
def test_export_case_equals_the_fp64_reference(name):
    from explainn_amd import interpret as it
    c = em.case(name)
    ref = em.reference(c)
    net, x, idxs = _net(c)
    for batch in c["batch_sizes"]:
        if c["mode"] == "pwms":
            res = it.filter_pwms(net, x, idxs, c["rc"], batch_size=batch, site_cap=ref["cap"])
        else:
            res = _through_filter_sites(net, x, ref["rows"], ref["thresholds"], ref["cap"], batch)
        what = "export %s b%d " % (name, batch)
        _same(what + "thresholds", res["thresholds"], ref["thresholds"])
        _same(what + "nsites", res["nsites"], ref["nsites"])
        _same(what + "pfm", res["pfm"], ref["pfm"])
        _same(what + "hit", res["hit"], ref["hit"])


def test_site_lists_and_count_matrices_agree_at_600bp():
    """Two kernels, one answer: the k-mers under sites.hip's site list, counted, are interpret.hip's
    count matrix (3 position chunks; selection in runs, N bases, a sequence of only N)."""
    from explainn_amd import interpret as it
    c = em.case("c5_len")
    net, x, idxs = _net(c)
    res = it.filter_pwms(net, x, idxs, False, batch_size=4)
    lists = it.filter_site_list(net, x, idxs, res["thresholds"])
    pfm = np.zeros_like(res["pfm"])
    for u, lst in enumerate(lists):
        for kmer in it.site_kmers(x, lst, c["k"]):
            for t, ch in enumerate(kmer):
                if ch != "N":
                    pfm[u, t, "ACGT".index(ch)] += 1
    _same("export c5_len site lists nsites", np.array([len(lst) for lst in lists], dtype=np.int64), res["nsites"])
    _same("export c5_len site lists pfm", pfm, res["pfm"])
    assert res["nsites"].sum() > 0


# ---- PWM scan ----------------------------------------------------------------------------------------
def _codes_input(g, B, L, n_frac=0.0):
    codes = g.integers(0, 4, size=(B, L)).astype(np.uint8)
    if n_frac:
        codes[g.random((B, L)) < n_frac] = 4
    return em.onehot(codes)


def _pwm_cases():
    g = np.random.default_rng(17)
    neg = lambda G, k: -g.uniform(0.1, 2.0, size=(G, 4, k)).astype(np.float32)          # noqa: E731
    rnd = lambda G, k: g.standard_normal((G, 4, k)).astype(np.float32)                  # noqa: E731
    x_n = _codes_input(g, 7, 50, n_frac=0.1)
    x_n[3] = 0                                                   # a sequence of only N
    return {
        # max mode starts at -inf; with 2*Lo = 80 < 256 most threads never leave it
        "all_negative": (neg(5, 11), _codes_input(g, 6, 50)),
        "all_negative_k_eq_L": (neg(5, 12), _codes_input(g, 6, 12)),
        "windows_256": (rnd(4, 5), _codes_input(g, 3, 132)),
        "windows_258": (rnd(1, 5), _codes_input(g, 3, 133)),
        "lds_limit": (rnd(5, 19), _codes_input(g, 2, 2996, n_frac=0.01)),
        "soft_input": (rnd(4, 11), g.uniform(-1, 1, size=(5, 4, 50)).astype(np.float32)),
        "n_columns": (rnd(5, 11), x_n),
    }


PWM_CASES = _pwm_cases()


@pytest.mark.parametrize("scoring", ["max", "sum"])
@pytest.mark.parametrize("name", list(PWM_CASES))
def test_pwm_scan_edges_vs_fp64(name, scoring):
    from explainn_amd import PWM
    pwms, x = PWM_CASES[name]
    G, _, k = pwms.shape
    L = x.shape[2]
    assert 4 * L + 16 * k <= 12288
    ref = eo.pwm_scan(pwms, x, scoring)
    got = PWM(pwms, L, scoring).cuda()(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape == (len(x), G) and np.isfinite(got).all()
    scale = max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    record_margin("abs pwm_scan %s %s" % (name, scoring), err / scale, 1e-4)
    assert err <= 1e-4 * scale, (err, scale)
    # what the case is there for, on the reference alone
    if name.startswith("all_negative") and scoring == "max":
        assert ref.max() < -0.1 * k                              # a kernel starting its max at 0 returns 0
    if name == "all_negative_k_eq_L":
        assert L - k + 1 == 1
    if name == "windows_256":
        assert 2 * (L - k + 1) == 256
    if name == "windows_258":
        assert 2 * (L - k + 1) == 258
    if name == "lds_limit":
        assert 4 * L + 16 * k == 12288
    if name == "n_columns":
        assert not x[3].any() and (ref[3] == 0).all()
        assert (got[3] == 0).all(), got[3]                       # exactly 0 in both scorings, not -inf


def test_pwm_scan_refuses_one_base_past_the_lds_limit():
    """L = 2997 at k = 19 needs 4 bytes more than the tile: refused by the module and by the C ABI
    before anything is launched (the score buffer keeps its sentinel)."""
    from explainn_amd import PWM, _lib
    g = np.random.default_rng(18)
    pwms = g.standard_normal((2, 4, 19)).astype(np.float32)
    x = torch.zeros(1, 4, 2997, device="cuda")
    with pytest.raises(RuntimeError, match="LDS"):
        PWM(pwms, 2997, "max").cuda()(x)
    lib = _lib.load()
    w = torch.from_numpy(pwms).cuda()
    scores = torch.full((1, 2), -7.0, device="cuda")
    for scoring in (_lib.PWM_MAX, _lib.PWM_SUM):
        rc = lib.explainn_pwm_scan(x.data_ptr(), 1, 2997, w.data_ptr(), 2, 19, scoring, scores.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert (scores == -7.0).all()
