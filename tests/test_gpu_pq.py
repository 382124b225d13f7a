"""GPU: the device product quantisation (csrc/pq.hip) — fused encode, order-fixed update, training loop, batched ADC search,
reconstruction and the public functions — against a float64 numpy restatement of pycleora/compress.py:146-173 and :64-98 on the
same f32 inputs.  Every device call runs twice and must give equal bits.  Sizes the shapes straddle: 128 rows per tile of the encode
kernel (4 waves x 32), subspace columns padded to 8, 64 centroids per step (two accumulators of 32); 256 members per chunk and 1024
rows per segment in the update; 1024 rows per pass, 256 rows per split and 8 / 4 / 2 queries per block in the scan.

Tolerances, u = 2^-24.  Assign: a score ||c||^2 - 2 x.c carries (ds + 1) u ||c||^2 from the norm, 2 ds u ||x|| ||c|| from the dot
product and u (||c||^2 + 2 ||x|| ||c||) from the subtraction; twice that (chosen and true best) is below
tol = (ds + 8) 2^-23 (2 ||x|| C + C^2), C = max ||c||.  The reported distance is a direct sum of ds squared differences, ds + 3
roundings of a value <= (||x|| + C)^2: (ds + 8) 2^-24 (||x|| + C)^2.  Update: one rounding of an f64 sum, rtol 2^-23.  Search: a
table entry is an f64 value rounded once, |entry| <= 1, u each; the M - 1 f32 additions round partial sums <= sqrt(M) (Cauchy-Schwarz
over the unit query's slices), u sqrt(M) each; M u + (M - 1) sqrt(M) u <= M (ds + 9) 2^-23 for every M <= 64."""
import types

import numpy as np
import pytest

import cleora_amd
from cleora_amd import _hip, compress, variants

pytestmark = pytest.mark.gpu


def _twice(call, outputs):
    """Runs the device call twice on fresh copies of its output arrays; returns the (bit-equal) host results."""
    runs = []
    for _ in range(2):
        dev = [_hip.DevArray.from_host(a) for a in outputs]
        _hip.check(call(*[a.ptr for a in dev]))
        _hip.check(_hip.lib().cleora_stream_sync(None))
        runs.append([a.to_host() for a in dev])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    return runs[0]


def _sqdist(x, d, cb):
    """float64 [M][n][kc] squared distances of the leading d columns' slices to the codebooks."""
    M, _, ds = cb.shape
    sub = x[:, :d].astype(np.float64).reshape(len(x), M, ds).transpose(1, 0, 2)
    return ((sub[:, :, None, :] - cb.astype(np.float64)[:, None, :, :]) ** 2).sum(axis=3)


def _assign(x, d, cb, shift=0):
    """cleora_pq_assign_dev on the leading d columns of x (ldx = x.shape[1]), the matrix `shift` floats into its buffer."""
    L, (n, ldx), (M, kc, _) = _hip.lib(), x.shape, cb.shape
    dx, dc = _hip.DevArray.from_host(np.concatenate([np.zeros(shift, np.float32), x.ravel()])), _hip.DevArray.from_host(cb)
    ws = _hip.DevArray((L.cleora_pq_workspace(n, d, M, kc),), np.uint8)
    return _twice(lambda cp, dp: L.cleora_pq_assign_dev(dx.offset(4 * shift), ldx, n, d, dc.ptr, M, kc, cp, dp, ws.ptr, None),
                  [np.full((n, M), 255, np.uint8), np.full((n, M), -1.0, np.float32)])


def _check_assign(codes, dist, x, d, cb):
    M, kc, ds = cb.shape
    D, big = _sqdist(x, d, cb), np.linalg.norm(cb.astype(np.float64), axis=2).max(axis=1)[:, None]
    xn = np.linalg.norm(x[:, :d].astype(np.float64).reshape(len(x), M, ds), axis=2).T
    assert (codes < kc).all()
    chosen = np.take_along_axis(D, codes.T.astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    tol, tol_d = (ds + 8) * 2.0 ** -23 * (2 * xn * big + big ** 2), (ds + 8) * 2.0 ** -24 * (xn + big) ** 2
    print(f"max (chosen - min) / tol {np.max((chosen - D.min(axis=2)) / tol):.3g}")
    assert (chosen <= D.min(axis=2) + tol).all()
    if dist is not None:
        print(f"max |dist - chosen| / tol {np.max(np.abs(dist.T - chosen) / tol_d):.3g}")
        assert (np.abs(dist.T - chosen) <= tol_d).all()


@pytest.mark.parametrize("n, ds, kc, M, pad, shift", [(33, 3, 33, 3, 0, 0), (127, 1, 2, 8, 0, 0), (129, 32, 31, 8, 0, 0), (300, 33, 255, 1, 0, 0),
                                                      (256, 64, 256, 1, 0, 0), (400, 64, 256, 3, 0, 0), (200, 4, 1, 64, 0, 0), (300, 32, 256, 8, 8, 0),
                                                      (300, 32, 33, 8, 0, 1), (1, 8, 1, 2, 0, 0), (500, 5, 2, 3, 3, 0)])
def test_assign(n, ds, kc, M, pad, shift):
    rng = np.random.default_rng(n + ds + kc + M)
    x = (rng.standard_normal((n, M * ds + pad)) * rng.uniform(0.1, 5.0, (n, 1))).astype(np.float32)
    cb = np.ascontiguousarray(x[rng.choice(n, kc, replace=False), :M * ds].reshape(kc, M, ds).transpose(1, 0, 2))
    codes, dist = _assign(x, M * ds, cb, shift)
    _check_assign(codes, dist, x, M * ds, cb)


def test_assign_exact_ties_take_the_lower_index():
    """Duplicate centroids (j, j') that meet in one lane, across the lane halves, the two accumulators and the steps of 64 (rows
    never span waves in this kernel: a wave owns its 32 rows for every centroid)."""
    rng = np.random.default_rng(2)
    pairs = np.array([(0, 1), (2, 6), (10, 42), (20, 90), (5, 200), (130, 255)])
    cb = rng.standard_normal((2, 256, 24)).astype(np.float32)
    cb[:, pairs[:, 1]] = cb[:, pairs[:, 0]]
    x = rng.standard_normal((400, 48)).astype(np.float32)
    copies = rng.permutation(400)[:120].reshape(6, 20)
    for (j, _), rows in zip(pairs, copies):
        x[rows] = cb[:, j].reshape(48)
    codes, dist = _assign(x, 48, cb)
    _check_assign(codes, dist, x, 48, cb)
    assert not np.isin(codes, pairs[:, 1]).any()
    for (j, _), rows in zip(pairs, copies):
        assert (codes[rows] == j).all() and (dist[rows] == 0.0).all()


def _mean_ref(x, d, codes, old):
    """float64: every centroid the mean of its members' slices, the old value without members."""
    M, kc, ds = old.shape
    sub, out = x[:, :d].astype(np.float64).reshape(len(x), M, ds), old.astype(np.float64).copy()
    for m in range(M):
        for c in np.unique(codes[:, m]):
            out[m, c] = sub[codes[:, m] == c, m].mean(axis=0)
    return out


@pytest.mark.parametrize("n, ds, kc, M, pad", [(600, 64, 1, 1, 0), (700, 5, 3, 2, 2), (1500, 32, 40, 8, 0), (1100, 3, 256, 64, 0)])
def test_update(n, ds, kc, M, pad):
    """Cluster 0 of every subspace holds more than two chunks of 256 members, cluster 1 (kc > 1) none.  Subspace 0 starts AT its
    means, so its allclose flag is 1; the others start elsewhere."""
    rng = np.random.default_rng(n + ds)
    x = (rng.standard_normal((n, M * ds + pad)) * rng.uniform(0.1, 5.0, (n, 1))).astype(np.float32)
    codes = rng.integers(0, kc, (n, M)).astype(np.uint8)
    codes[codes == 1] = 0
    codes[:520] = 0
    old = rng.standard_normal((M, kc, ds)).astype(np.float32)
    want = _mean_ref(x, M * ds, codes, old)
    old[0] = want[0].astype(np.float32)
    L, d = _hip.lib(), M * ds
    dx, dl = _hip.DevArray.from_host(x), _hip.DevArray.from_host(codes)
    ws = _hip.DevArray((L.cleora_pq_workspace(n, d, M, kc),), np.uint8)
    new, close = _twice(lambda cp, fp: L.cleora_pq_update_dev(dx.ptr, d + pad, n, d, dl.ptr, cp, M, kc, fp, ws.ptr, None),
                        [old, np.full(M, 7, np.uint32)])
    if kc > 1:
        assert np.array_equal(new[:, 1].view(np.uint32), old[:, 1].view(np.uint32))
    print(f"max relative error {np.max(np.abs(new - want) / np.maximum(np.abs(want), 1e-300)):.3g}, bound {2.0 ** -23:.3g}")
    np.testing.assert_allclose(new, want, rtol=2.0 ** -23, atol=0)
    assert close.tolist() == [int(np.allclose(old[m], new[m], atol=1e-6)) for m in range(M)] and close[0] == 1


def _restate(x, start, max_iter, margin=None):
    """The reference's loop in float64: (codes, codebooks, iterations per subspace).  margin: every assign decision and every
    allclose decision is asserted to be that clear (a factor 2 for allclose), so that f32 arithmetic cannot decide otherwise."""
    M, kc, ds = start.shape
    cb, its, codes = start.astype(np.float64).copy(), [], np.zeros((len(x), M), np.int64)

    def nearest(m):
        D = _sqdist(x, M * ds, cb)[m]
        if margin is not None and kc > 1:
            two = np.sort(D, axis=1)[:, :2]
            assert (two[:, 1] - two[:, 0] >= margin).all()
        return D.argmin(axis=1)

    for m in range(M):
        for it in range(1, max_iter + 1):
            codes[:, m] = nearest(m)
            fresh = _mean_ref(x, M * ds, codes, cb)[m]
            gap, bound = np.abs(cb[m] - fresh), 1e-6 + 1e-5 * np.abs(fresh)
            assert margin is None or ((gap <= bound / 2) | (gap >= bound * 2)).all()
            done, cb[m] = (gap <= bound).all(), fresh
            if done:
                break
        its.append(it)
        codes[:, m] = nearest(m)
    return codes, cb, its


@pytest.mark.parametrize("seed", [0, 42])
def test_train_one_iteration(seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((300, 15)).astype(np.float32)
    start = compress.initial_codebooks(x, 3, 8, seed)
    first, second = compress.train(x, start, 1), compress.train(x, start, 1)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    codes, cb, iterations = first
    assert iterations == 1 and codes.dtype == np.uint8 and cb.dtype == np.float32
    labels = _sqdist(x, 15, start).argmin(axis=2).T
    np.testing.assert_allclose(cb, _mean_ref(x, 15, labels, start), rtol=2.0 ** -23, atol=0)
    _check_assign(codes, None, x, 15, cb)


def test_train_planted_clusters_stop_per_subspace():
    """Subspace 0: noisy points around separated centres, the true centres as the start — stable after the first update, stops at
    iteration 2.  Subspace 1 (four equal columns): 40 points at -4 and 3 at 4.9 start with centre 0, 30 points at 10 with centre 10; the
    first update pulls centre 0 to about -3.4, the 4.9s change sides in iteration 2, it stops at iteration 3."""
    rng = np.random.default_rng(3)
    centres = (8.0 * np.eye(4)).astype(np.float32)
    planted = rng.permutation(np.repeat(np.arange(4), 19))[:73]
    line = rng.permutation(np.repeat([-4.0, 4.9, 10.0], [40, 3, 30]))
    x = np.concatenate([centres[planted] + 0.1 * rng.standard_normal((73, 4)), np.repeat(line[:, None], 4, axis=1)], axis=1).astype(np.float32)
    start = np.stack([centres, np.repeat(np.array([0.0, 10.0, 50.0, 90.0], np.float32)[:, None], 4, axis=1)])
    want_codes, want_cb, its = _restate(x, start, 20, margin=0.1)
    assert its == [2, 3] and (want_codes[:, 0] == planted).all()
    codes, cb, iterations = compress.train(x, start, 20)
    assert iterations == 3 and np.array_equal(codes, want_codes)
    np.testing.assert_allclose(cb, want_cb, rtol=2.0 ** -23, atol=0)
    _, early, stopped = compress.train(x, start, 2)
    assert stopped == 2 and np.array_equal(early[0].view(np.uint32), cb[0].view(np.uint32))             # frozen after iteration 2
    assert np.array_equal(cb[1, 2:].view(np.uint32), start[1, 2:].view(np.uint32))                      # centres without members


def _adc64(index, queries):
    """float64 ADC scores [nq][n] (:64-98)."""
    M, ds = index._num_subspaces, index._subspace_dim
    cb = index._codebooks.astype(np.float64)
    unit = cb / np.maximum(np.linalg.norm(cb, axis=2, keepdims=True), 1e-10)
    q = queries.astype(np.float64)
    norms = np.linalg.norm(q, axis=1, keepdims=True)
    q = np.where(norms > 1e-10, q / np.maximum(norms, 1e-300), q).reshape(len(q), M, ds)
    tables = np.einsum("mcj,qmj->qmc", unit, q)
    return sum(tables[:, m, index._codes[:, m]] for m in range(M))


def _random_index(n, M, ds, kc, seed, nq=5):
    rng = np.random.default_rng(seed)
    codes, cb = rng.integers(0, kc, (n, M)).astype(np.uint8), rng.standard_normal((M, kc, ds)).astype(np.float32)
    queries = rng.standard_normal((nq, M * ds)).astype(np.float32)
    queries[1] = 0.0
    return compress.PQIndex(codes, cb, M, ds, (n, M * ds)), queries


def _search_twice(index, queries, k, **kw):
    first, second = index.search_batch(queries, k, **kw), index.search_batch(queries, k, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    return first


@pytest.mark.parametrize("n, M, ds, kc, nq", [(20, 3, 5, 4, 5), (700, 8, 32, 256, 5), (300, 64, 4, 256, 5), (1500, 12, 3, 200, 5),
                                              (260, 1, 64, 7, 5), (20000, 8, 4, 16, 600)])
def test_search(n, M, ds, kc, nq):
    """The last case: 75 query tiles leave 7 row splits of 2880 rows — three passes of 1024 rows per block."""
    index, queries = _random_index(n, M, ds, kc, n + M, nq)
    exact, bound = _adc64(index, queries), M * (ds + 9) * 2.0 ** -23
    for top_k in (1, n if n <= 32 else 10, 32):
        k = min(top_k, n)
        idx, scores = _search_twice(index, queries, top_k)
        assert idx.shape == scores.shape == (nq, k) and idx.dtype == np.uint32 and scores.dtype == np.float32
        picked = np.take_along_axis(exact, idx.astype(np.int64), axis=1)
        print(f"top_k {top_k}: max |score - exact| {np.abs(scores - picked).max():.3g}, bound {bound:.3g}")
        assert (np.abs(scores - picked) <= bound).all() and (np.diff(scores, axis=1) <= 0).all()
        assert all(len(set(row)) == k for row in idx.tolist())
        assert (picked[:, -1] >= np.sort(exact, axis=1)[:, -k] - 2 * bound).all()
        assert idx[1].tolist() == list(range(n - 1, n - 1 - k, -1)) and (scores[1] == 0.0).all()            # the zero query: all ties
    single = index.search(queries[0], 10)
    assert single["indices"].tolist() == idx[0, :10].tolist() and np.array_equal(single["scores"], scores[0, :10])


@pytest.mark.parametrize("n, nq", [(700, 5), (20000, 600)])
def test_search_heavy_ties_across_row_splits(n, nq):
    """kc = 2, M = 2: four distinct scores — the list must be exactly 'score descending, larger row first' of the device's own f32
    scores.  700 rows: three row splits and the merge.  20000 rows x 600 queries: three passes per block in which a quarter of
    the rows beat every threshold, so the candidate lists overflow and are compacted again and again."""
    index, queries = _random_index(n, 2, 6, 2, 9, nq)
    idx, scores, every = _search_twice(index, queries, 32, return_all_scores=True)
    assert (np.abs(every - _adc64(index, queries)) <= 2 * 15 * 2.0 ** -23).all()
    for q in range(nq):
        assert len(np.unique(every[q])) <= 4
        order = np.lexsort((-np.arange(n), -every[q]))[:32]
        assert idx[q].tolist() == order.tolist() and np.array_equal(scores[q], every[q][order])


def test_reconstruct_public_path_and_accelerate():
    rng = np.random.default_rng(11)
    x = rng.standard_normal((500, 24)).astype(np.float32)
    first, second = compress.product_quantize(x, 4, 16, max_iter=5, seed=3), compress.product_quantize(x, 4, 16, max_iter=5, seed=3)
    assert np.array_equal(first._codes, second._codes) and np.array_equal(first._codebooks, second._codebooks)
    assert first._codes.dtype == np.uint8 and first._codes.shape == (500, 4) and first._codebooks.shape == (4, 16, 6)
    _check_assign(first._codes, None, x, 24, first._codebooks)
    want = np.concatenate([first._codebooks[m, first._codes[:, m]] for m in range(4)], axis=1)
    assert np.array_equal(first.reconstruct().view(np.uint32), want.view(np.uint32))
    rows = np.array([499, 0, 7, 7])
    assert np.array_equal(first.reconstruct(rows).view(np.uint32), want[rows].view(np.uint32))
    shaped = types.SimpleNamespace(_codes=first._codes, _codebooks=first._codebooks, _num_subspaces=4, _subspace_dim=6)
    _, host_scores = compress._search_numpy(shaped, x[:3], 10)
    assert (np.abs(first.search_batch(x[:3], 10)[1] - host_scores) <= 2 * 4 * 15 * 2.0 ** -23).all()
    calls = []
    original = types.SimpleNamespace(product_quantize=lambda emb, *a, **kw: calls.append(a or kw) or "original")
    pkg = cleora_amd.accelerate(types.SimpleNamespace(embed=lambda *a, **kw: None, compress=original))
    got = pkg.compress.product_quantize(x, 4, 16, max_iter=5, seed=3)
    assert np.array_equal(got._codes, first._codes) and calls == []
    assert pkg.compress.product_quantize(x, num_centroids=variants.PQ_MAX_CENTROIDS + 1) == "original"
    assert pkg.compress.product_quantize(x[:10], 4, 16) == "original" and len(calls) == 2
