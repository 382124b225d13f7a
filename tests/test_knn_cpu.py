"""CPU-only: the fused kNN entry points' host side (csrc/knn.hip) — workspace arithmetic and argument checks need no device."""
import ctypes

import pytest

from cleora_amd import _hip


def test_knn_workspace_is_monotone_and_bad_arguments_are_refused_before_any_device_work():
    L = _hip.lib()
    base = (100_000, 64, 10, 1000)
    for pos, bigger in enumerate([(200_000, 10**7), (65, 256, 257, 2048), (11, 32), (1001, 40_000, 100_000, 10**7)]):
        sizes = [L.cleora_knn_workspace(*base)] + [L.cleora_knn_workspace(*(base[:pos] + (v,) + base[pos + 1:])) for v in bigger]
        assert sizes == sorted(sizes) and sizes[0] >= 4 * base[0], (pos, sizes)
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda g, k, n, excl, oi, os_: L.cleora_knn_cosine_dev(g, p, 4, n, 4, None, 8, k, 1, excl, oi, os_, p, None)
    for bad, word in [((None, 0, 100, 0, p, p), "k"), ((None, 33, 100, 0, p, p), "k"), ((None, 10, 9, 0, p, p), "k"),
                      ((None, 10, 100, 1, p, p), "graph"), ((None, 10, 100, 0, None, p), "NULL"), ((None, 10, 100, 0, p, None), "NULL")]:
        assert call(*bad) == _hip.E_INVALID and word in _hip.last_error()
    with pytest.raises(ValueError):
        _hip.check(L.cleora_knn_cosine_dev(None, p, 3, 100, 4, None, 8, 10, 1, 0, p, p, p, None))      # ldx < d
