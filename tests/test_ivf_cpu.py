"""CPU-only: the IVF entry points' host side (csrc/ivf.hip) — workspace arithmetic and argument checks need no device."""
import ctypes

from cleora_amd import _hip


def test_ivf_workspaces_are_monotone_and_bad_arguments_are_refused_before_any_device_work():
    L = _hip.lib()
    base = (100_000, 64, 316, 8, 10, 1000)           # n, d, nlist, nprobe, k, n_queries
    for pos, bigger in enumerate([(200_000, 10**7), (65, 256, 257, 2048), (317, 1024, 4096), (9, 32), (11, 32),
                                  (1001, 40_000, 131_072, 131_073, 10**7)]):
        sizes = [L.cleora_ivf_search_workspace(*(base[:pos] + (v,) + base[pos + 1:])) for v in (base[pos],) + bigger]
        assert sizes == sorted(sizes) and sizes[0] >= 1000 * 8 * 10 * 8, (pos, sizes)
    for f, args in [(L.cleora_ivf_xs_bytes, (1000, 64, 30)), (L.cleora_ivf_build_workspace, (1000, 30))]:
        for pos in range(len(args)):
            assert f(*args) <= f(*(args[:pos] + (args[pos] * 3 + 1,) + args[pos + 1:])) and f(*args) > 0
    assert L.cleora_ivf_xs_bytes(1000, 64, 30) >= (1000 + 30 * 127) * 64 * 4       # every list may end with 127 padding rows

    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(ldx=4, n=100, d=4, nlist=10, dense=p, rows=None, nprobe=3, k=5, excl=0, oi=p, lp=p)

    def search(**kw):
        a = {**ok, **kw}
        return L.cleora_ivf_search_dev(a["lp"], p, p, p, a["ldx"], a["n"], a["d"], p, a["nlist"], a["dense"], a["rows"], 8, a["nprobe"], a["k"],
                                       a["excl"], a["oi"], p, None, p, 0, None)

    def build(**kw):
        a = {**ok, **kw}
        return L.cleora_ivf_build_dev(p, a["ldx"], a["n"], a["d"], p, a["nlist"], a["lp"], p, p, p, None)

    for bad, word in [(dict(nlist=1), "nlist"), (dict(nlist=101), "nlist"), (dict(nlist=4097, n=5000), "nlist"), (dict(n=1 << 32), "2^32"),
                      (dict(d=0), "d"), (dict(d=16385, ldx=16385), "d"), (dict(ldx=3), "ldx"), (dict(lp=None), "NULL")]:
        for call in (search, build):
            assert call(**bad) == _hip.E_INVALID and word in _hip.last_error(), (bad, _hip.last_error())
    for bad, word in [(dict(nprobe=0), "nprobe"), (dict(nprobe=11), "nprobe"), (dict(nprobe=33, nlist=40), "nprobe"), (dict(k=0), "k"),
                      (dict(k=33), "k"), (dict(rows=p), "exactly one"), (dict(dense=None), "exactly one"), (dict(excl=1), "exclude_self"),
                      (dict(oi=None), "NULL")]:
        assert search(**bad) == _hip.E_INVALID and word in _hip.last_error(), (bad, _hip.last_error())
