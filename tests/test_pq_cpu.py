"""CPU-only: the host side of the device product quantisation (cleora_amd/compress.py, csrc/pq.hip) — argument checks, the start
draw, the numpy statement for shapes the kernels do not take, workspace arithmetic.  None of it needs a device."""
import ctypes
import types

import numpy as np
import pytest

from cleora_amd import _hip, compress, variants


@pytest.mark.parametrize("shape, kwargs, text", [
    ((0, 4), {}, r"^embeddings must be a non-empty 2D array$"), ((8,), {}, r"^embeddings must be a non-empty 2D array$"),
    ((8, 4), {"num_subspaces": 0}, r"^num_subspaces must be positive, got 0$"),
    ((8, 4), {"num_centroids": -1}, r"^num_centroids must be positive, got -1$"),
    ((8, 4), {"max_iter": 0}, r"^max_iter must be positive, got 0$"),
    ((8, 6), {"num_subspaces": 4}, r"^Embedding dimension \(6\) must be divisible by num_subspaces \(4\)$")])
def test_product_quantize_raises_the_reference_messages_without_a_device(shape, kwargs, text):
    with pytest.raises(ValueError, match=text):
        compress.product_quantize(np.ones(shape, np.float32), **kwargs)
    with pytest.raises(ValueError, match=r"^top_k must be positive, got 0$"):
        compress.PQIndex(np.zeros((3, 1), np.uint8), np.ones((1, 2, 2), np.float32), 1, 2, (3, 2)).search(np.ones(2), top_k=0)


def test_start_draw_is_one_random_state_subspace_after_subspace():
    x = np.random.default_rng(0).standard_normal((50, 6)).astype(np.float32)
    rng = np.random.RandomState(7)
    want = [x[rng.choice(50, size=9, replace=False), 2 * m:2 * m + 2] for m in range(3)]
    assert np.array_equal(compress.initial_codebooks(x, 3, 9, 7), np.stack(want))
    assert compress.initial_codebooks(x[:4], 3, 9, 7).shape == (3, 9, 2)          # more centroids than rows: jittered repeats


def test_numpy_statement_on_a_hand_computed_case():
    """Two subspaces of one column; six rows; three centroids, so 3 > variants limits is not what forwards this — n < kc does
    not apply either: the statement is called directly.  Subspace 0: values 0, 0, 1, 10, 10, 11 from the start (0, 10, 100):
    codes 0 0 0 1 1 1, means 1/3 and 31/3, centroid 2 keeps 100.  Subspace 1: all 5, start (5, 6, 7): stops in iteration 1."""
    x = np.array([[0, 5], [0, 5], [1, 5], [10, 5], [10, 5], [11, 5]], np.float32)
    start = np.array([[[0], [10], [100]], [[5], [6], [7]]], np.float32)
    codes, cb = compress._train_numpy(x, start, 20)
    assert codes.dtype == np.uint8 and codes.tolist() == [[0, 0]] * 3 + [[1, 0]] * 3
    np.testing.assert_allclose(cb[:, :, 0], [[1 / 3, 31 / 3, 100], [5, 6, 7]], rtol=1e-6)
    index = compress.PQIndex(codes, cb, 2, 1, x.shape)
    assert np.array_equal(compress._reconstruct_numpy(index, [5, 0]), cb[[0, 1], [[1, 0], [0, 0]], 0])
    # query (1, 1) / sqrt 2 against unit centroids (all +1 in one column): every score is sqrt 2; ties to the larger row
    idx, scores = compress._search_numpy(index, np.ones((1, 2), np.float32), 4)
    assert idx.tolist() == [[5, 4, 3, 2]] and np.allclose(scores, np.sqrt(2.0), atol=1e-6)
    big = compress.PQIndex(np.zeros((3, 1), np.uint16), np.ones((1, 300, 2), np.float32), 1, 2, (3, 2))
    assert not big._on_device() and not compress._device_serves(10, 4, 16, 6) and not compress._device_serves(10 ** 6, 1, 8, 65)
    assert compress._device_serves(10 ** 6, 8, variants.PQ_MAX_CENTROIDS, variants.PQ_MAX_SUBSPACE_DIM // 2)


def test_pq_workspaces_are_monotone_and_bad_arguments_are_refused_before_any_device_work():
    L = _hip.lib()
    for pos, bigger in enumerate([(100_001, 600_000, 10 ** 7), (512, 1024), (16, 64), (17, 255, 256)]):
        base = (100_000, 256, 8, 16)
        args = [base] + [base[:pos] + (v,) + base[pos + 1:] for v in bigger]
        if pos == 1:
            args = [a[:2] + (8, 16) for a in args]
        sizes = [L.cleora_pq_workspace(*a) for a in args]
        assert sizes == sorted(sizes) and sizes[0] >= 8 * base[0], (pos, sizes)
    sizes = [L.cleora_pq_search_workspace(n, 8, 256, nq, 10) for n, nq in [(100, 1), (10 ** 4, 1), (10 ** 6, 1), (10 ** 6, 64), (10 ** 6, 4096)]]
    assert sizes == sorted(sizes)
    buf = (ctypes.c_float * 64)()
    p, ran = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_uint32(0)
    for n, d, M, kc, ldx, word in [(100, 6, 4, 8, 6, "multiple"), (100, 130, 2, 8, 130, "64"), (100, 8, 2, 257, 8, "256"), (100, 8, 2, 101, 8, "rows"),
                                   (100, 65, 65, 8, 65, "subspaces"), (100, 8, 2, 8, 7, "ldx"), (100, 8, 2, 0, 8, "256")]:
        for rc in (L.cleora_pq_assign_dev(p, ldx, n, d, p, M, kc, p, None, p, None), L.cleora_pq_update_dev(p, ldx, n, d, p, p, M, kc, p, p, None),
                   L.cleora_pq_train(p, ldx, n, d, p, M, kc, 5, p, ctypes.byref(ran), p, None)):
            assert rc == _hip.E_INVALID and word in _hip.last_error(), (word, _hip.last_error())
    assert L.cleora_pq_assign_dev(None, 8, 100, 8, p, 2, 8, p, None, p, None) == _hip.E_INVALID and "NULL" in _hip.last_error()
    assert L.cleora_pq_search_dev(p, 100, p, 2, 8, 4, p, 1, 33, p, p, None, p, None) == _hip.E_INVALID and "top_k" in _hip.last_error()
    assert L.cleora_pq_search_dev(p, 100, p, 2, 8, 4, p, 1, 10, p, None, None, p, None) == _hip.E_INVALID and "NULL" in _hip.last_error()
    assert L.cleora_pq_reconstruct_dev(p, 100, p, 2, 8, 4, None, 10, p, 7, None) == _hip.E_INVALID and "ldo" in _hip.last_error()
