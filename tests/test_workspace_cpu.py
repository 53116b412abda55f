"""Caller workspaces (csrc/workspace.h): every context-free explainn_*_workspace_bytes export against a
restatement of its documented layout, and the shared check an entry point makes of its caller's workspace
before it launches anything.  The CPU half needs only the built library; two device cases show what the host
cannot: that _lib.call refuses a strided tensor, and that a 16-byte aligned workspace is as good as a
256-byte aligned one where the header promises so.  Every comparison here is exact."""
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from explainn_amd import _lib
    return _lib.load()


def up(v):
    return (v + 255) & ~255


# ---------------------------------------------------------------- the layouts, restated
def compare_bytes(M, wmax):
    """D [M][2][wmax] float4 | P [M][2][wmax+1] double | W [M] int32"""
    return up(M * 2 * wmax * 16) + up(M * 2 * (wmax + 1) * 8) + up(4 * M)


def significance_bytes(Q, T, wmax, bins, both):
    """the compare pieces of Q + T motifs | cs [Q*wmax][ld] uint8 | hist [Q*wmax][bins+1] int32 | sf [Q][sfq] double"""
    ld = (2 if both else 1) * wmax * ((T + 15) & ~15)
    sfq = bins * (wmax * (wmax + 1) * (wmax + 2) // 6) + wmax * (wmax + 1) // 2
    return compare_bytes(Q + T, wmax) + up(Q * wmax * ld) + up(Q * wmax * (bins + 1) * 4) + up(Q * sfq * 8)


def tree_bytes(M):
    """L [M][M] int64 | K [M][M] uint64 | size [M] int32 | slot [M] int32"""
    return 2 * up(8 * M * M) + 2 * up(4 * M)


def pwm_sites_bytes(M, npos):
    """cnt int32 [rows][tiles] | tot int64 [rows], a row per (motif, strand), a tile per 1024 starts"""
    rows, tiles = 2 * M, (npos + 1023) // 1024
    return up(4 * rows * tiles) + up(8 * rows)


def enrichment_bytes(units):
    return max(min(units, 256), 1) * 32768 * 4


METRICS_TILE = 4096        # items per block of csrc/metrics.hip (MT * MI)


def metrics_bytes(N, T, per_task, linear):
    """make_layout of csrc/metrics.hip: keys_a, keys_b u64 [cells] | hist u32 [segs][256][nblk] | hist_sums u32
    [segs][hist_nb] | run_sums u64 [segs][nblk] | part | (linear: means, end_at, d)"""
    n, S = (N, T) if per_task else (N * T, 1)
    segs = 2 * S if linear else S
    nblk = (n + METRICS_TILE - 1) // METRICS_TILE
    hist_nb = (256 * nblk + METRICS_TILE - 1) // METRICS_TILE
    cells = segs * n
    total = 2 * up(cells * 8) + up(segs * 256 * nblk * 4) + up(segs * hist_nb * 4) + up(segs * nblk * 8)
    if not linear:
        return total + up(S * nblk * 16)
    return total + up(S * nblk * 6 * 8) + up(S * 2 * 8) + 2 * up(cells * 4)


# ---------------------------------------------------------------- sizes
def test_motif_compare_bytes(lib):
    size = lib.explainn_motif_compare_workspace_bytes
    for Q, T, wmax in itertools.product((0, 1, 63, 64, 65), (0, 1, 63, 64, 65), (1, 19, 64)):
        assert size(Q, T, wmax) == compare_bytes(Q + T, wmax), (Q, T, wmax)
    assert size(-1, 1, 8) == size(1, -1, 8) == size(1, 1, 0) == 0


def test_motif_significance_bytes(lib):
    size = lib.explainn_motif_significance_workspace_bytes
    for Q, T, wmax, bins, both in itertools.product((1, 8, 65), (1, 8, 65), (1, 19, 64), (2, 100, 128), (0, 1)):
        assert size(Q, T, wmax, bins, both) == significance_bytes(Q, T, wmax, bins, both), (Q, T, wmax, bins, both)
    assert size(8, 8, 19, 1, 1) == size(8, 8, 19, 129, 1) == size(8, 8, 65, 100, 1) == 0


def test_motif_tree_bytes(lib):
    size = lib.explainn_motif_tree_workspace_bytes
    for M, linkage in itertools.product((0, 1, 2, 5, 64, 12288), (0, 1, 2)):
        assert size(M, linkage) == tree_bytes(M), (M, linkage)
    assert size(-1, 0) == size(12289, 0) == size(5, 3) == 0


def test_pwm_sites_bytes(lib):
    size = lib.explainn_pwm_sites_workspace_bytes
    for M, npos in itertools.product((0, 1, 16, 17), (0, 1, 1024, 1025)):
        assert size(M, npos) == pwm_sites_bytes(M, npos), (M, npos)
    assert size(-1, 10) == size(4, -1) == 0


def test_enrichment_bytes(lib):
    size = lib.explainn_enrichment_workspace_bytes
    for units in (0, 1, 256, 257):
        assert size(units, 100) == enrichment_bytes(units), units
    assert size(4, 2 ** 31) == size(-1, 100) == size(4, -1) == 0


def test_metrics_bytes(lib):
    size = lib.explainn_metrics_workspace_bytes
    for N, T, per_task, linear in itertools.product((1, 1024, 1025, 4096, 4097), (1, 3), (0, 1), (0, 1)):
        assert size(N, T, per_task, linear) == metrics_bytes(N, T, per_task, linear), (N, T, per_task, linear)
    col = 1 << 26
    assert size(col, 1, 0, 0) == metrics_bytes(col, 1, 0, 0)
    for over in ((col + 1, 1, 1, 0), (col // 2 + 1, 2, 0, 0), (1, 65536, 1, 0), (1, 32768, 1, 1), (0, 1, 0, 0),
                 (1, 0, 0, 0), (1, 1, 2, 0), (1, 1, 0, 2)):
        assert size(*over) < 0, over


# ---------------------------------------------------------------- the workspace check of the entry points
P = 4096                       # any non-null address: nothing is dereferenced on the host before the check


def _compare(Q=3, T=3, wmax=8):
    return "explainn_motif_compare", "explainn_motif_compare_workspace_bytes", (Q, T, wmax), \
        lambda ws, n: (P, P, Q, P, P, T, wmax, 0.0, 1, 1, P, P, P, ws, n, None)


def _significance(Q=3, T=3, wmax=8, bins=10):
    return "explainn_motif_significance", "explainn_motif_significance_workspace_bytes", (Q, T, wmax, bins, 1), \
        lambda ws, n: (P, P, Q, P, P, T, wmax, 0.0, 1, 1, bins, P, P, P, None, None, ws, n, None)


def _tree(M=5):
    return "explainn_motif_tree", "explainn_motif_tree_workspace_bytes", (M, 2), \
        lambda ws, n: (P, P, P, M, 2, P, P, P, P, P, ws, n, None)


def _pwm_sites(M=3, npos=2000, wmax=8):
    return "explainn_pwm_sites", "explainn_pwm_sites_workspace_bytes", (M, npos), \
        lambda ws, n: (P, npos + wmax, 0, npos, 0, 1, P, P, M, wmax, P, P, 10, P, None, None, None, 0, ws, n, None)


def _enrichment(units=3, n=50):
    return "explainn_enrichment_test", "explainn_enrichment_workspace_bytes", (units, n), \
        lambda ws, nb: (P, P, units, n) + (P,) * 9 + (None, ws, nb, None)


def _last_error(lib):
    return lib.explainn_last_error().decode()


@pytest.mark.parametrize("case", [_compare, _significance, _tree, _pwm_sites, _enrichment])
def test_missing_or_short_workspace_is_refused_before_any_launch(lib, case):
    from explainn_amd import _lib
    name, size_name, dims, args = case()
    need = getattr(lib, size_name)(*dims)
    assert need > 0
    who = name[len("explainn_"):]
    for ws, given in ((None, need), (1 << 20, need - 1)):
        assert getattr(lib, name)(*args(ws, given)) == _lib.E_ARG, (name, ws, given)
        msg = _last_error(lib)
        assert who in msg and str(given) in msg and str(need) in msg, msg


@pytest.mark.parametrize("case", [_compare, _significance, _tree])
def test_sixteen_byte_calls_refuse_an_eight_byte_aligned_workspace(lib, case):
    from explainn_amd import _lib
    name, size_name, dims, args = case()
    need = getattr(lib, size_name)(*dims)
    assert getattr(lib, name)(*args((1 << 20) + 8, need)) == _lib.E_ARG
    assert name[len("explainn_"):] in _last_error(lib) and "16-byte" in _last_error(lib)


@pytest.mark.parametrize("case", [_compare, _significance])
def test_sixteen_byte_aligned_workspace_passes_the_check(lib, case):
    """Both calls check the size of their grids right after the workspace and before the first launch: 2^21 x
    2^21 motifs exceed one launch, so E_UNSUPPORTED says that a workspace at 256 k + 16 passed the check (the
    same call with the workspace 8 bytes further on stops at it).  Nothing is allocated: the addresses are only
    compared."""
    from explainn_amd import _lib
    n = 1 << 21
    name, size_name, _, args = case(Q=n, T=n, wmax=1)
    # the call needs the workspace of Q + T motifs; so does the size export
    need = getattr(lib, size_name)(*case(Q=n, T=n, wmax=1)[2])
    assert need > 0
    assert getattr(lib, name)(*args((1 << 20) + 16, need)) == _lib.E_UNSUPPORTED, _last_error(lib)
    assert "exceed one launch" in _last_error(lib)
    assert getattr(lib, name)(*args((1 << 20) + 24, need)) == _lib.E_ARG


@pytest.mark.parametrize("case", [_pwm_sites, _enrichment])
def test_256_byte_calls_refuse_a_sixteen_byte_aligned_workspace(lib, case):
    from explainn_amd import _lib
    name, size_name, dims, args = case()
    need = getattr(lib, size_name)(*dims)
    assert getattr(lib, name)(*args((1 << 20) + 16, need)) == _lib.E_ARG
    assert "256-byte" in _last_error(lib)


def test_self_comparison_needs_the_workspace_of_the_queries_only(lib):
    """t == NULL: the call takes the workspace of Q motifs, the size export always reports Q + T."""
    from explainn_amd import _lib
    Q, wmax = 5, 8
    own = lib.explainn_motif_compare_workspace_bytes(Q, 0, wmax)
    assert own == compare_bytes(Q, wmax) < lib.explainn_motif_compare_workspace_bytes(Q, Q, wmax)
    args = lambda n: (P, P, Q, None, None, Q, wmax, 0.0, 1, 1, P, P, P, 1 << 20, n, None)
    assert lib.explainn_motif_compare(*args(own - 1)) == _lib.E_ARG
    assert str(own) in _last_error(lib) and str(own - 1) in _last_error(lib)


# ---------------------------------------------------------------- the Python call path, without a device
def test_device_for_refuses_the_host_before_the_library_is_loaded(monkeypatch):
    import torch

    from explainn_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    for device, candidates in (("cpu", ()), (torch.device("cpu"), (torch.zeros(2),)), ("meta", ())):
        with pytest.raises(RuntimeError, match=r"^x\.y runs only on a HIP device \(there is no CPU fallback\)$"):
            _lib.device_for(device, candidates, "x.y")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _lib.device_for(None, ((torch.zeros(2), torch.zeros(2)), None), "x.y")


def test_require_refuses_host_tensors():
    import torch

    from explainn_amd import _lib
    with pytest.raises(RuntimeError, match="bits must be a contiguous int16 tensor of shape"):
        _lib.require(torch.zeros((2, 3), dtype=torch.int16), torch.int16, (None, 3), None, "bits")
    with pytest.raises(RuntimeError, match="labels"):
        _lib.require(np.zeros(3), torch.uint8, (3,), None, "labels")


def test_arguments_convert_without_a_device(monkeypatch):
    """The conversion _lib.call and Context.call share: None is NULL, a Structure instance goes through untouched
    (ctypes takes it by reference where the signature says POINTER), numbers, byref()s and addresses stay, and a
    host tensor is refused for a HIP device -- all before the library is loaded."""
    import ctypes as C

    import torch

    from explainn_amd import _lib
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded"))
    dev = torch.device("cuda", 0)
    ps, flags = _lib.Params(), C.c_int(0)
    ref = C.byref(flags)
    argv = _lib.arguments("explainn_x", dev, (None, ps, 7, 0.5, ref, 4096))
    assert argv[0] is None and C.c_void_p(argv[0]).value is None
    assert argv[1] is ps and C.POINTER(_lib.Params).from_param(argv[1]) is not None
    assert argv[2:] == [7, 0.5, ref, 4096]
    with pytest.raises(RuntimeError, match=r"^explainn_x: argument 2 must be a contiguous tensor on cuda:0 .*on cpu"):
        _lib.arguments("explainn_x", dev, (None, ps, torch.zeros(3)))


# ---------------------------------------------------------------- on the device
@pytest.mark.gpu
def test_call_refuses_a_strided_tensor_and_one_on_the_host():
    import torch

    from explainn_amd import _lib, sites
    hist = torch.ones((4, 6), dtype=torch.float32, device="cuda").t()        # strided
    assert not hist.is_contiguous()
    with pytest.raises(RuntimeError, match=r"explainn_activation_null: argument 0 .*contiguous"):
        sites._null_stats(hist, 0.01)
    dev = torch.device("cuda", torch.cuda.current_device())
    with pytest.raises(RuntimeError, match=r"explainn_activation_null: argument 3 .*cpu"):
        _lib.call("explainn_activation_null", dev, hist.contiguous(), 6, 0.01, torch.zeros(6), None, None)
    torch.cuda.synchronize()                                                   # nothing was launched: nothing to fail


@pytest.mark.gpu
def test_compare_with_a_sixteen_byte_aligned_workspace():
    """Q = T = 5, wmax = 8: the workspace at 256 k + 16 gives motifs.compare's result bit for bit."""
    import torch

    from explainn_amd import _lib, motifs
    rng = np.random.default_rng(5)
    Q = T = 5
    wmax = 8
    q, t = (torch.from_numpy(rng.random((5, wmax, 4)).astype(np.float32)).cuda() for _ in range(2))
    qw = torch.tensor([8, 5, 6, 8, 7], dtype=torch.int32, device="cuda")
    tw = torch.tensor([6, 8, 8, 5, 7], dtype=torch.int32, device="cuda")
    want = motifs.compare((q, qw), (t, tw), min_overlap=3)
    nbytes = _lib.load().explainn_motif_compare_workspace_bytes(Q, T, wmax)
    ws = torch.empty((nbytes + 16,), dtype=torch.uint8, device="cuda")[16:]
    assert ws.data_ptr() % 256 == 16
    ncor, cor = (torch.empty((Q, T), dtype=torch.float32, device="cuda") for _ in range(2))
    align = torch.empty((Q, T, 3), dtype=torch.int16, device="cuda")
    _lib.call("explainn_motif_compare", q.device, q, qw, Q, t, tw, T, wmax, 0.0, 3, 1, ncor, cor, align, ws, nbytes)
    assert torch.equal(ncor.view(torch.int32), want.ncor.view(torch.int32))
    assert torch.equal(cor.view(torch.int32), want.cor.view(torch.int32))
    assert torch.equal(align[..., 0], want.offset) and torch.equal(align[..., 1], want.strand)
    assert torch.equal(align[..., 2], want.overlap)
