"""Approximate nearest neighbours of an embedding on the device: an inverted-file (IVF) index over the fused kernels of
csrc/kmeans.hip (the coarse quantiser), csrc/knn.hip (probe selection) and csrc/ivf.hip (list layout and the grouped list scan).

  IVFIndex   batched search: arrays in, (index uint32[nq, k], score float32[nq, k]) out, like embed.nearest_neighbours
  ANNIndex   the reference's pycleora/search.py:101-215 interface (query / query_vector -> list of dicts) over IVFIndex

An IVF index answers from the lists of a query's `nprobe` nearest centroids only: its recall is below 1 and depends on nprobe (the
measured table is in DESIGN.md §2.8).  That is why accelerate() does not put this ANNIndex in the reference's place."""
import ctypes

import numpy as np

from . import _hip

MAX_K = 32             # CLEORA_KNN_MAX_K: the most neighbours (and probes) the scan kernels select per query
MAX_NLIST = 4096       # CLEORA_KMEANS_MAX_K
NO_ROW = 0xFFFFFFFF    # index of a result slot that the probed lists could not fill


class IVFIndex:
    """Spherical k-means of the rows into `nlist` lists (default round(sqrt(n)), within [2, 4096]), then the device layout of
    cleora_ivf_build_dev; rows, centroids and lists stay on the device for the life of the object.  train_size: train the centroids
    on that many rows drawn with `seed`, then assign every row once.  nprobe: how many lists a query reads unless a search says
    otherwise."""

    def __init__(self, embeddings, nlist=None, nprobe=8, seed=42, max_iterations=20, train_size=None):
        x = np.ascontiguousarray(embeddings, dtype=np.float32)
        if x.ndim != 2 or x.shape[0] < 2 or x.shape[1] < 1:
            raise ValueError("embeddings must be a 2-D array with at least 2 rows and 1 column")
        n, d = x.shape
        nlist = min(max(int(round(np.sqrt(n))), 2), MAX_NLIST) if nlist is None else int(nlist)
        if not 2 <= nlist <= min(n, MAX_NLIST):
            raise ValueError(f"nlist must be in [2, min(n, {MAX_NLIST})], got {nlist}")
        self.n, self.d, self.nlist = n, d, nlist
        self.nprobe = self._check_nprobe(nprobe)
        L = _hip.lib()
        rng = np.random.default_rng(seed)
        self._x = _hip.DevArray.from_host(x)
        if train_size is not None and nlist <= int(train_size) < n:
            sample = np.sort(rng.choice(n, size=int(train_size), replace=False))
            train, dtrain = x[sample], None
        else:
            train, dtrain = x, self._x
        start = train[rng.choice(len(train), size=nlist, replace=False)]
        start = np.ascontiguousarray(start / np.maximum(np.linalg.norm(start, axis=1, keepdims=True), 1e-10), dtype=np.float32)
        self._centroids = _hip.DevArray.from_host(start)
        labels = _hip.DevArray.from_host(np.zeros(n, np.uint32))
        ws = _hip.DevArray((L.cleora_kmeans_workspace(n, d, nlist),), np.uint8)
        ran = ctypes.c_uint32(0)
        if dtrain is None:
            dtrain, tl = _hip.DevArray.from_host(train), _hip.DevArray((len(train),), np.uint32)
            _hip.check(L.cleora_kmeans_cosine(dtrain.ptr, d, len(train), d, self._centroids.ptr, nlist, max(int(max_iterations), 0), tl.ptr,
                                              ctypes.byref(ran), ws.ptr, None))
            changed = _hip.DevArray((1,), np.uint64)
            _hip.check(L.cleora_kmeans_assign_dev(self._x.ptr, d, n, d, self._centroids.ptr, nlist, labels.ptr, None, changed.ptr, ws.ptr, None))
        else:
            _hip.check(L.cleora_kmeans_cosine(dtrain.ptr, d, n, d, self._centroids.ptr, nlist, max(int(max_iterations), 0), labels.ptr,
                                              ctypes.byref(ran), ws.ptr, None))
        self.iterations = int(ran.value)
        self._list_ptr = _hip.DevArray((nlist + 1,), np.uint64)
        self._list_rows = _hip.DevArray((n,), np.uint32)
        self._xs = _hip.DevArray((L.cleora_ivf_xs_bytes(n, d, nlist),), np.uint8)
        bws = _hip.DevArray((L.cleora_ivf_build_workspace(n, nlist),), np.uint8)
        _hip.check(L.cleora_ivf_build_dev(self._x.ptr, d, n, d, labels.ptr, nlist, self._list_ptr.ptr, self._list_rows.ptr, self._xs.ptr,
                                          bws.ptr, None))
        _hip.check(L.cleora_stream_sync(None))
        self.list_sizes = np.diff(self._list_ptr.to_host().astype(np.int64))

    @property
    def centroids(self):
        """The nlist x d unit centroids (a host copy)."""
        return self._centroids.to_host()

    def _check_nprobe(self, nprobe):
        nprobe = int(nprobe)
        if not 1 <= nprobe <= min(self.nlist, MAX_K):
            raise ValueError(f"nprobe must be in [1, min(nlist, {MAX_K})], got {nprobe}")
        return nprobe

    def _search(self, dense, rows, nq, k, nprobe, exclude_self):
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        nprobe = self.nprobe if nprobe is None else self._check_nprobe(nprobe)
        if nq == 0:
            return np.empty((0, k), np.uint32), np.empty((0, k), np.float32)
        L = _hip.lib()
        oi, os_ = _hip.DevArray((nq, k), np.uint32), _hip.DevArray((nq, k), np.float32)
        ws = _hip.DevArray((L.cleora_ivf_search_workspace(self.n, self.d, self.nlist, nprobe, k, nq),), np.uint8)
        _hip.check(L.cleora_ivf_search_dev(self._list_ptr.ptr, self._list_rows.ptr, self._xs.ptr, self._x.ptr, self.d, self.n, self.d,
                                           self._centroids.ptr, self.nlist, dense.ptr if dense else None, rows.ptr if rows else None, nq,
                                           nprobe, k, 1 if exclude_self else 0, oi.ptr, os_.ptr, None, ws.ptr, 0, None))
        _hip.check(L.cleora_stream_sync(None))
        return oi.to_host(), os_.to_host()

    def search(self, queries, k=10, nprobe=None):
        """The k most cosine-similar indexed rows of every query VECTOR (nq x d) among the lists it probes: descending score, ties
        to the larger row index; slots the probed lists cannot fill hold index 0xffffffff and score -inf."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.d:
            raise ValueError(f"queries must have shape (nq, {self.d})")
        return self._search(_hip.DevArray.from_host(q) if len(q) else None, None, len(q), k, nprobe, False)

    def search_rows(self, rows=None, k=10, nprobe=None, exclude_self=True):
        """The same for indexed rows as queries (None: every row): the kNN graph of the embedding, approximately.  exclude_self
        masks the query's own row (score -2: it only appears when the probed lists hold fewer than k others)."""
        r = np.arange(self.n, dtype=np.uint32) if rows is None else np.asarray(rows, dtype=np.int64).ravel()
        if r.size and (r.min() < 0 or r.max() >= self.n):
            raise ValueError("query row index out of range")
        return self._search(None, _hip.DevArray.from_host(r.astype(np.uint32)) if r.size else None, r.size, k, nprobe, exclude_self)


class ANNIndex:
    """pycleora/search.py's ANNIndex (:101-215) on the device.  method "ivf": an IVFIndex built with **ivf_options (approximate;
    top_k up to 32); "brute": exact, through the device top-k.  "hnsw" is not offered: this is not an HNSW graph and does not
    pretend to have its recall."""

    def __init__(self, graph, embeddings, method="ivf", **ivf_options):
        if method == "hnsw":
            raise ValueError("method 'hnsw' is not available on the device; use 'ivf' (inverted-file index, approximate) or 'brute'.")
        if method not in ("ivf", "brute"):
            raise ValueError(f"Unknown method: '{method}'. Use 'ivf' or 'brute'.")
        self._graph = graph
        self._embeddings = np.ascontiguousarray(embeddings, dtype=np.float32)
        self._method = method
        self._n, self._dim = self._embeddings.shape
        self._ivf = IVFIndex(self._embeddings, **ivf_options) if method == "ivf" else None

    def _results(self, indices, similarities, drop=None):
        ids = self._graph.entity_ids
        return [{"entity_id": ids[int(i)], "index": int(i), "similarity": float(s)}
                for i, s in zip(indices, similarities) if int(i) != NO_ROW and int(i) != drop]

    def _ivf_k(self, top_k):
        if top_k > MAX_K:
            raise ValueError(f"top_k must be at most {MAX_K} with method 'ivf', got {top_k}")
        return top_k

    def query(self, entity_id, top_k=10, exclude_self=True):
        if top_k <= 0:
            raise ValueError(f"top_k must be positive, got {top_k}")
        idx = self._graph.get_entity_index(entity_id)
        if self._method == "ivf":
            index, score = self._ivf.search_rows([idx], k=self._ivf_k(top_k), exclude_self=exclude_self)
        else:
            from . import embed
            fetch_k = top_k + 1 if exclude_self else top_k            # :142-147: one more, then drop the query itself
            index, score = embed.nearest_neighbours(self._embeddings, k=fetch_k, queries=[idx], exclude_self=False)
        return self._results(index[0], score[0], drop=idx if exclude_self else None)[:top_k]

    def query_vector(self, vector, top_k=10):
        if top_k <= 0:
            raise ValueError(f"top_k must be positive, got {top_k}")
        v = np.asarray(vector, dtype=np.float32).reshape(1, -1)
        if self._method == "ivf":
            index, score = self._ivf.search(v, k=self._ivf_k(top_k))
            return self._results(index[0], score[0])
        # exact: the row temporarily takes the place of a query row of the device top-k
        from . import embed
        both = np.concatenate([self._embeddings, v])
        index, score = embed.nearest_neighbours(both, k=min(top_k, self._n), queries=[self._n], exclude_self=True)
        return self._results(index[0], score[0])
