"""Product quantisation of an embedding (pycleora/compress.py:32-181) on the device (csrc/pq.hip): `product_quantize` trains all
subspaces together with the fused encode kernel and the order-fixed update, `PQIndex.search_batch` scores many queries from the
codes through per-query lookup tables with the top-k kept inside the scan kernel.  A `PQIndex` holds the reference's private
attributes, so one built by the reference and one built here are interchangeable as data.

Shapes the kernels do not take (variants.PQ_MAX_CENTROIDS / PQ_MAX_SUBSPACE_DIM / PQ_MAX_SUBSPACES / PQ_MAX_TOP_K, or more
centroids than rows) go through the plain numpy statement of the same method at the end of this module."""
import ctypes

import numpy as np

from . import _hip
from . import variants as _var


def _device_serves(n, num_subspaces, num_centroids, subspace_dim):
    return (num_centroids <= min(_var.PQ_MAX_CENTROIDS, n) and 1 <= subspace_dim <= _var.PQ_MAX_SUBSPACE_DIM
            and num_subspaces <= _var.PQ_MAX_SUBSPACES and n * num_subspaces < 2 ** 32)


def _check_arguments(embeddings, num_subspaces, num_centroids, max_iter):
    if embeddings.ndim != 2 or embeddings.shape[0] == 0:                     # pycleora/compress.py:108-121
        raise ValueError("embeddings must be a non-empty 2D array")
    if num_subspaces <= 0:
        raise ValueError(f"num_subspaces must be positive, got {num_subspaces}")
    if num_centroids <= 0:
        raise ValueError(f"num_centroids must be positive, got {num_centroids}")
    if max_iter <= 0:
        raise ValueError(f"max_iter must be positive, got {max_iter}")
    if embeddings.shape[1] % num_subspaces != 0:
        raise ValueError(f"Embedding dimension ({embeddings.shape[1]}) must be divisible by num_subspaces ({num_subspaces})")


def initial_codebooks(x, num_subspaces, num_centroids, seed):
    """The reference's start (:124-144), drawn on the host from ONE RandomState, subspace after subspace: num_centroids distinct
    rows; when there are fewer rows than centroids, every row plus jittered repeats.  float32 [M, kc, ds]."""
    n, dim = x.shape
    ds = dim // num_subspaces
    rng = np.random.RandomState(seed)
    out = np.empty((num_subspaces, num_centroids, ds), np.float32)
    for m in range(num_subspaces):
        sub = x[:, m * ds:(m + 1) * ds].astype(np.float32)
        start = sub[rng.choice(n, size=min(num_centroids, n), replace=False)]
        if num_centroids > n:
            extra = num_centroids - n
            repeats = sub[rng.choice(n, size=extra, replace=True)]
            start = np.vstack([start, repeats + rng.randn(extra, ds).astype(np.float32) * 0.01])
        out[m] = start
    return out


def train(embeddings, codebooks, max_iter=20):
    """cleora_pq_train from the given start: (codes uint8[n, M], codebooks float32[M, kc, ds], iterations)."""
    x = np.ascontiguousarray(embeddings, dtype=np.float32)
    start = np.ascontiguousarray(codebooks, dtype=np.float32)
    (n, d), (M, kc, ds) = x.shape, start.shape
    if M * ds != d:
        raise ValueError(f"codebooks of shape {start.shape} do not cover {d} columns")
    L = _hip.lib()
    dx, dc = _hip.DevArray.from_host(x), _hip.DevArray.from_host(start)
    codes = _hip.DevArray((n, M), np.uint8)
    ws = _hip.DevArray((L.cleora_pq_workspace(n, d, M, kc),), np.uint8)
    ran = ctypes.c_uint32(0)
    _hip.check(L.cleora_pq_train(dx.ptr, d, n, d, dc.ptr, M, kc, int(max_iter), codes.ptr, ctypes.byref(ran), ws.ptr, None))
    return codes.to_host(), dc.to_host(), int(ran.value)


class PQIndex:
    """The reference's PQIndex (:32-98) with the scan on the device.  Codes and codebooks are uploaded once, on first use."""

    def __init__(self, codes, codebooks, num_subspaces, subspace_dim, original_shape):
        self._codes = codes
        self._codebooks = codebooks
        self._num_subspaces = num_subspaces
        self._subspace_dim = subspace_dim
        self._original_shape = original_shape
        self._dev = None

    def _on_device(self):
        kc = self._codebooks.shape[1]
        return self._codes.dtype == np.uint8 and _device_serves(len(self._codes), self._num_subspaces, kc, self._subspace_dim)

    def _device(self):
        if self._dev is None:
            self._dev = (_hip.DevArray.from_host(np.ascontiguousarray(self._codes, dtype=np.uint8)),
                         _hip.DevArray.from_host(np.ascontiguousarray(self._codebooks, dtype=np.float32)))
        return self._dev

    def reconstruct(self, indices=None):
        n, M, ds = len(self._codes), self._num_subspaces, self._subspace_dim
        rows = None if indices is None else np.asarray(indices)
        plain = rows is None or (rows.ndim == 1 and rows.dtype.kind in "iu" and (rows.size == 0 or (rows.min() >= 0 and rows.max() < n)))
        if not self._on_device() or not plain:                               # masks, negative or fancy indices: numpy's own rules
            return _reconstruct_numpy(self, indices)
        count = n if rows is None else rows.size
        out = _hip.DevArray((count, M * ds), np.float32)
        if count:
            L, (dcodes, dcb) = _hip.lib(), self._device()
            drows = None if rows is None else _hip.DevArray.from_host(rows.astype(np.uint32))
            _hip.check(L.cleora_pq_reconstruct_dev(dcodes.ptr, n, dcb.ptr, M, self._codebooks.shape[1], ds,
                                                   None if drows is None else drows.ptr, count, out.ptr, M * ds, None))
            _hip.check(L.cleora_stream_sync(None))
        return out.to_host()

    def search_batch(self, queries, top_k=10, return_all_scores=False):
        """(indices uint32[nq, k], scores float32[nq, k]) with k = min(top_k, n): score descending, ties to the larger row index.
        return_all_scores appends the float32[nq, n] scores of every row (a test hook: the kernel itself never stores them)."""
        if top_k <= 0:
            raise ValueError(f"top_k must be positive, got {top_k}")
        q = np.ascontiguousarray(queries, dtype=np.float32)
        n, M, ds = len(self._codes), self._num_subspaces, self._subspace_dim
        if q.ndim != 2 or q.shape[1] != M * ds:
            raise ValueError(f"queries must have shape (nq, {M * ds})")
        k, nq = min(int(top_k), n), len(q)
        if nq == 0 or k > _var.PQ_MAX_TOP_K or not self._on_device():
            return _search_numpy(self, q, k, return_all_scores)
        L, (dcodes, dcb), kc = _hip.lib(), self._device(), self._codebooks.shape[1]
        dq, oi, os_ = _hip.DevArray.from_host(q), _hip.DevArray((nq, k), np.uint32), _hip.DevArray((nq, k), np.float32)
        every = _hip.DevArray((nq, n), np.float32) if return_all_scores else None
        ws = _hip.DevArray((L.cleora_pq_search_workspace(n, M, kc, nq, k),), np.uint8)
        _hip.check(L.cleora_pq_search_dev(dcodes.ptr, n, dcb.ptr, M, kc, ds, dq.ptr, nq, k, oi.ptr, os_.ptr,
                                          None if every is None else every.ptr, ws.ptr, None))
        _hip.check(L.cleora_stream_sync(None))
        return (oi.to_host(), os_.to_host()) + ((every.to_host(),) if return_all_scores else ())

    def search(self, query, top_k=10):
        indices, scores = self.search_batch(np.asarray(query, dtype=np.float32).reshape(1, -1), top_k)
        return {"indices": indices[0].astype(np.int64), "scores": scores[0]}


def product_quantize(embeddings, num_subspaces=8, num_centroids=256, max_iter=20, seed=None):
    """(pycleora/compress.py:101-181).  The start is the reference's host-side draw; the iterations and the final encoding are
    one call of cleora_pq_train."""
    embeddings = np.asarray(embeddings)
    _check_arguments(embeddings, num_subspaces, num_centroids, max_iter)
    n, dim = embeddings.shape
    ds = dim // num_subspaces
    start = initial_codebooks(embeddings, num_subspaces, num_centroids, seed)
    if _device_serves(n, num_subspaces, num_centroids, ds):
        codes, codebooks, _ = train(embeddings, start, max_iter)
    else:
        codes, codebooks = _train_numpy(embeddings.astype(np.float32), start, max_iter)
    return PQIndex(codes=codes, codebooks=codebooks, num_subspaces=num_subspaces, subspace_dim=ds, original_shape=embeddings.shape)


# ---- the same method in plain numpy, for the shapes the kernels do not take

def _nearest(sub, centroids):
    return np.argmin((centroids ** 2).sum(axis=1)[None, :] - 2.0 * (sub @ centroids.T), axis=1)


def _train_numpy(x, start, max_iter):
    M, kc, ds = start.shape
    codes = np.empty((len(x), M), np.uint8 if kc <= 256 else np.uint16)
    codebooks = start.copy()
    for m in range(M):
        sub, cent = x[:, m * ds:(m + 1) * ds], codebooks[m]
        for _ in range(max_iter):
            labels, fresh = _nearest(sub, cent), cent.copy()
            sums, counts = np.zeros((kc, ds), np.float64), np.bincount(labels, minlength=kc)
            np.add.at(sums, labels, sub)
            fresh[counts > 0] = (sums[counts > 0] / counts[counts > 0, None]).astype(np.float32)
            done, cent = np.allclose(cent, fresh, atol=1e-6), fresh
            if done:
                break
        codes[:, m], codebooks[m] = _nearest(sub, cent), cent
    return codes, codebooks


def _reconstruct_numpy(index, indices):
    codes = index._codes if indices is None else index._codes[indices]
    parts = [index._codebooks[m, codes[:, m]] for m in range(index._num_subspaces)]
    return np.concatenate(parts, axis=1).astype(np.float32)


def _search_numpy(index, queries, k, return_all_scores=False):
    M, ds, n = index._num_subspaces, index._subspace_dim, len(index._codes)
    cb = index._codebooks.astype(np.float64)
    unit = cb / np.maximum(np.linalg.norm(cb, axis=2, keepdims=True), 1e-10)
    out_i, out_s, every = np.empty((len(queries), k), np.uint32), np.empty((len(queries), k), np.float32), []
    for i, q in enumerate(queries.astype(np.float64)):
        norm = np.linalg.norm(q)
        q = q / norm if norm > 1e-10 else q
        tables = np.einsum("mcj,mj->mc", unit, q.reshape(M, ds)).astype(np.float32)
        scores = np.zeros(n, np.float32)
        for m in range(M):
            scores += tables[m, index._codes[:, m]]
        order = np.lexsort((-np.arange(n), -scores))[:k]                     # score descending, ties to the larger row
        out_i[i], out_s[i] = order, scores[order]
        every.append(scores)
    return (out_i, out_s) + ((np.array(every, np.float32).reshape(len(queries), n),) if return_all_scores else ())
