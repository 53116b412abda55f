"""CPU checks of the sync-BN C ABI (include/explainn_hip.h): the phase entry points are exported,
the ctypes argument struct lists the C struct's fields in order, and the Python switch exists.
No compute call is made."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "explainn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_sync_exports_in_library():
    import __graft_entry__ as g
    g.build()
    from explainn_amd import _lib
    lib = _lib.load()
    for name in ("explainn_sync_exchange_elems", "explainn_sync_phase"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), "missing export " + name


def test_sync_args_layout_matches_header():
    from explainn_amd import _lib
    text = _header()
    body = re.search(r"typedef struct explainn_sync_args \{(.*?)\} explainn_sync_args;", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += re.findall(r"([A-Za-z_][A-Za-z0-9_]*)\s*(?:,|$)", decl)
    assert tuple(fields) == _lib.SYNC_ARG_FIELDS
    assert tuple(f for f, _ in _lib.SyncArgs._fields_) == _lib.SYNC_ARG_FIELDS
    n = int(re.search(r"#define EXPLAINN_SYNC_PHASES (\d+)", text).group(1))
    assert n == _lib.SYNC_PHASES


def test_sync_batchnorm_switch():
    from explainn_amd import parallel

    class M:
        pass

    m = M()
    r = parallel.ProcessGroupReducer()
    assert parallel.sync_batchnorm(m, r) is m and m.sync_bn is r
    assert r.global_batch(7) == 7                     # no process group: one rank
    parallel.sync_batchnorm(m, None)
    assert m.sync_bn is None
