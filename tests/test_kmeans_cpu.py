"""CPU-only: the device k-means' host side (csrc/kmeans.hip) — workspace arithmetic and argument checks need no device."""
import ctypes
import types

import numpy as np
import pytest

from cleora_amd import _hip, variants


def test_kmeans_workspace_is_monotone_in_every_argument():
    L = _hip.lib()
    base = (100_000, 64, 10)
    for pos, bigger in enumerate([(100_001, 200_000, 600_000, 10**7, 2**32 - 1), (65, 256, 257, 16384), (11, 128, 129, 4096)]):
        sizes = [L.cleora_kmeans_workspace(*base)] + [L.cleora_kmeans_workspace(*(base[:pos] + (v,) + base[pos + 1:])) for v in bigger]
        assert sizes == sorted(sizes) and sizes[0] >= 8 * base[0], (pos, sizes)


@pytest.mark.parametrize("n, k, ldx, null, word", [(100, 1, 4, None, "at least 2"), (100, 101, 4, None, "rows"), (10**6, 4097, 4, None, "MAX_K"),
                                                   (100, 10, 3, None, "ldx"), (100, 10, 4, "x", "NULL"), (100, 10, 4, "labels", "NULL"),
                                                   (100, 10, 4, "workspace", "NULL")])
def test_kmeans_bad_arguments_are_refused_before_any_device_work(n, k, ldx, null, word):
    L = _hip.lib()
    buf = (ctypes.c_float * 64)()
    p = {name: (None if name == null else ctypes.cast(buf, ctypes.c_void_p)) for name in ("x", "labels", "workspace")}
    c, ran = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_uint32(0)
    for rc in (L.cleora_kmeans_assign_dev(p["x"], ldx, n, 4, c, k, p["labels"], None, c, p["workspace"], None),
               L.cleora_kmeans_update_dev(p["x"], ldx, n, 4, p["labels"], c, k, p["workspace"], None),
               L.cleora_kmeans_cosine(p["x"], ldx, n, 4, c, k, 5, p["labels"], ctypes.byref(ran), p["workspace"], None)):
        assert rc == _hip.E_INVALID and word in _hip.last_error()


def test_detect_communities_kmeans_raises_the_reference_messages_without_a_device():
    graph, emb = types.SimpleNamespace(entity_ids=["a", "b", "c"]), np.ones((3, 4), np.float32)
    with pytest.raises(ValueError, match=r"^k must be at least 2$"):
        variants.detect_communities_kmeans(graph, emb, 1)
    with pytest.raises(ValueError, match=r"^k \(4\) cannot be larger than number of entities \(3\)$"):
        variants.detect_communities_kmeans(graph, emb, 4)
    with pytest.raises(ValueError, match="CLEORA_KMEANS_MAX_K"):
        variants.detect_communities_kmeans(graph, np.ones((5000, 1), np.float32), variants.KMEANS_MAX_K + 1)
