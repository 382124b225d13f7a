"""GPU: the fused cosine kNN kernel (csrc/knn.hip, cleora_knn_cosine_dev) and the public functions that reach it, against cosines
in float64 from the same f32 input, masks applied, np.lexsort on (row index, score): ties put the larger row index first.
Scores position by position and every returned index's own score to atol 3e-6 — the tolerance tests/test_gpu_variants.py
applies to the batched device top-k; indices exactly where the input has exact duplicates."""
import numpy as np
import pytest

from cleora_amd import _hip, embed, variants
from cleora_amd.pycleora import SparseMatrix

pytestmark = pytest.mark.gpu


def _run(x, d, k, queries=None, exclude_self=True, csr=None):
    """cleora_knn_cosine_dev on the leading d columns of x (ldx = x.shape[1]), twice: the outputs must be bit-equal."""
    L = _hip.lib()
    n, ldx = x.shape
    nq = n if queries is None else len(queries)
    dx = _hip.DevArray.from_host(x)
    dq = None if queries is None else _hip.DevArray.from_host(np.asarray(queries, np.uint32))
    g = None if csr is None else _hip.Graph.from_host(csr[0], csr[1], np.ones(len(csr[1]), np.float32))
    ws = _hip.DevArray((L.cleora_knn_workspace(n, d, k, nq),), np.uint8)
    runs = []
    for _ in range(2):
        oi, os_ = _hip.DevArray((nq, k), np.uint32), _hip.DevArray((nq, k), np.float32)
        _hip.check(L.cleora_knn_cosine_dev(g.handle if g else None, dx.ptr, ldx, n, d, dq.ptr if dq else None, nq, k,
                                           1 if exclude_self else 0, 1 if g else 0, oi.ptr, os_.ptr, ws.ptr, None))
        _hip.check(L.cleora_stream_sync(None))
        runs.append((oi.to_host(), os_.to_host()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))
    if g:
        g.close()
    return runs[0]


def _check(idx, sc, x, k, queries=None, exclude_self=True, csr=None, exact=False):
    """The two assertions of the batched top-k's test, per query, against the float64 reference; returns the reference."""
    n = x.shape[0]
    qs = np.arange(n) if queries is None else np.asarray(queries, np.int64)
    xd = x.astype(np.float64)
    xn = xd / np.maximum(np.linalg.norm(xd, axis=1, keepdims=True), 1e-10)
    sims = np.einsum("qd,nd->qn", np.ascontiguousarray(xn[qs]), xn)      # one summation order for every pair: duplicates tie exactly
    if exclude_self:
        sims[np.arange(len(qs)), qs] = -2.0
    if csr is not None:
        m = np.zeros((n, n), bool)
        m[np.repeat(np.arange(n), np.diff(csr[0].astype(np.int64))), csr[1]] = True
        sims[(m | m.T)[qs]] = -2.0
    want = np.lexsort((np.broadcast_to(np.arange(n), sims.shape), sims))[:, ::-1][:, :k]
    want_sc = np.take_along_axis(sims, want, 1)
    own = np.take_along_axis(sims, idx.astype(np.int64), 1)
    print(f"max |score - ref| {np.abs(sc - want_sc).max():.3g}, max |score - own| {np.abs(sc - own).max():.3g}")
    assert idx.shape == sc.shape == (len(qs), k)
    np.testing.assert_allclose(sc, want_sc, rtol=0, atol=3e-6)
    np.testing.assert_allclose(own, sc, rtol=0, atol=3e-6)
    if exact:
        assert np.array_equal(idx, want)
    return want, want_sc


@pytest.mark.parametrize("n,d,k", [(1061, 100, 10),                              # tails of every tile, d no multiple of a chunk
                                   (40, 1, 1), (40, 7, 1), (33, 1, 32), (33, 7, 32),   # d = 1, k = 1, k = n - 1 = 32
                                   (600, 256, 32), (600, 1024, 32), (600, 2048, 32),   # the resident-Q limit and the chunked form
                                   (500, 32, 10)])                                # zero rows as query and as candidate
def test_all_rows(n, d, k):
    x = np.random.default_rng(n + d).standard_normal((n, d)).astype(np.float32)
    if n == 500:
        x[[0, 77, 499]] = 0.0
    _check(*_run(x, d, k), x, k)


@pytest.mark.parametrize("queries", [[2999, 0, 0] + list(np.random.default_rng(1).integers(0, 3000, 62)), [5, 2999, 5, 0, 1234]])
def test_query_lists_with_repeats(queries):
    x = np.random.default_rng(3).standard_normal((3000, 64)).astype(np.float32)
    _check(*_run(x, 64, 10, queries), x, 10, queries)


def test_candidate_split_and_merge():
    x = np.random.default_rng(4).standard_normal((70_000, 32)).astype(np.float32)
    queries = np.random.default_rng(5).integers(0, 70_000, 300)
    _check(*_run(x, 32, 10, queries), x, 10, queries)


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("rising", [True, False])
def test_adversarial_order(k, rising):
    """cos(angle difference) grows with the row index up to the query's own row (every candidate survives, every step
    compacts), or falls from it on."""
    n = 5000
    t = np.linspace(0.0, 1.5, n)
    x = np.zeros((n, 16), np.float32)
    x[:, 0], x[:, 1] = np.cos(t), np.sin(t)
    queries = [n - 1] * 32 + list(range(n - 32, n)) if rising else [0] * 32 + list(range(32))
    _check(*_run(x, 16, k, queries), x, k, queries)


def test_exact_ties():
    x = np.repeat(np.random.default_rng(6).standard_normal((1000, 48)).astype(np.float32), 2, 0)
    x[300:400] = x[300]
    _check(*_run(x, 48, 10), x, 10, exact=True)


def test_leading_dimension():
    wide = np.random.default_rng(7).standard_normal((1000, 128)).astype(np.float32)
    _check(*_run(wide, 96, 10), np.ascontiguousarray(wide[:, :96]), 10)


@pytest.mark.parametrize("exclude_self", [True, False])
def test_masks(exclude_self):
    """Unsorted columns, edges in one direction only, an empty row, and row 5 linked to all but 6 rows: fewer than k stay unmasked."""
    n, k = 1500, 10
    rng = np.random.default_rng(8)
    cols = [rng.integers(0, n, rng.poisson(6)) for _ in range(n)]
    cols[5] = rng.permutation(n)[: n - 6]
    cols[9] = cols[9][:0]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.uint64)
    col = np.concatenate(cols).astype(np.uint32)
    x = rng.standard_normal((n, 64)).astype(np.float32)
    idx, sc = _run(x, 64, k, None, exclude_self, (rowptr, col))
    _check(idx, sc, x, k, None, exclude_self, (rowptr, col))
    assert (sc[5] == -2.0).sum() >= k - 6 and (sc[9] > -2.0).all()


def test_public_functions_above_the_routing_threshold(monkeypatch):
    """nearest_neighbours and predict_links on a SparseMatrix with n = 2000 sources; the routing threshold (measured: 16384
    queries) is set back to its floor of 257 so that predict_links takes the fused call at a size a float64 reference fits."""
    monkeypatch.setattr(variants, "KNN_FUSED_MIN_QUERIES", 257)
    monkeypatch.setattr(_hip.lib(), "cleora_topk_cosine_dev", None)          # the batched entry point is not an option here
    n, top_k = 2000, 15
    rng = np.random.default_rng(9)
    g = SparseMatrix.from_iterator(iter([f"{i} {j}" for i, j in zip(range(n), rng.integers(0, n, n))] +
                                        [f"{i} {j}" for i, j in rng.integers(0, n, (3 * n, 2))]), "complex::reflexive::node")
    assert variants.KNN_FUSED_MIN_QUERIES <= g.num_entities == n
    x = rng.standard_normal((n, 24)).astype(np.float32)
    rows, cols = g.to_sparse_csr()[:2]
    csr = (np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.uint64), cols)
    idx, sc = embed.nearest_neighbours(x, k=10)
    _check(idx, sc, x, 10)
    idx, sc = embed.nearest_neighbours(x, k=7, queries=[3, 1999, 3], graph=g, exclude_self=False, exclude_existing=True)
    _check(idx, sc, x, 7, [3, 1999, 3], False, csr)
    got = variants.predict_links(g, x, top_k=top_k, exclude_existing=True)
    want, want_sc = _check(*_run(x, 24, top_k, None, True, csr), x, top_k, None, True, csr)
    order = np.argsort(-want_sc.ravel(), kind="stable")[:top_k]
    ref_sc = want_sc.ravel()[order]
    np.testing.assert_allclose([p["score"] for p in got], ref_sc, rtol=0, atol=2e-6)
    ids, flat_sc, flat_t = g.entity_ids, want_sc.ravel(), want.ravel()
    for p in got:          # the pair is one of the reference's pairs at that score (pairs closer than 1e-5 may swap places)
        close = np.flatnonzero(np.abs(flat_sc - p["score"]) <= 1e-5)
        assert (p["source"], p["target"]) in {(ids[c // top_k], ids[flat_t[c]]) for c in close}
