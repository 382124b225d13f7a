"""GPU: the device k-means (csrc/kmeans.hip) — the fused assign kernel, the order-fixed update, the loop and the public functions —
against a float64 numpy restatement of pycleora/community.py:18-42 on the same f32 inputs.  Every device call runs twice and must
give equal bits.  Tile sizes the shapes straddle: 64 rows and 128 centroids per block of the assign kernel, the X tile resident up to
d = 256; 256 members per chunk, 256 columns per slab and 1024 rows per segment in the update.  k >= 2 and k <= n make n = 2 the
smallest problem.

Tolerances.  Assign: the chosen centroid's float64 cosine is within (d + 8) 2^-23 of the row's maximum, and the reported cosine
within the same bound of the chosen one — an f32 dot product errs by at most d 2^-24 on each of two candidates, plus a few roundings
for the 1 / ||x|| scale.  Update: atol 1e-6 — about six f32 roundings of 2^-24 at magnitude <= 1 are 3.6e-7."""
import types

import numpy as np
import pytest

import cleora_amd
from cleora_amd import _hip, embed, variants
from cleora_amd.pycleora import SparseMatrix

pytestmark = pytest.mark.gpu


def _unit(a):
    return (a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-10)).astype(a.dtype)


def _cosines(x, cent):
    return _unit(x.astype(np.float64)) @ cent.astype(np.float64).T


def _update_ref(x, labels, cent):
    xn, out = _unit(x.astype(np.float64)), cent.astype(np.float64).copy()
    for c in range(len(cent)):
        if (labels == c).any():
            mean = xn[labels == c].mean(axis=0)
            if np.linalg.norm(mean) > 1e-10:
                out[c] = mean / np.linalg.norm(mean)
    return out


def _twice(call, outputs):
    """Runs the device call twice on fresh copies of its in/out arrays; returns the (bit-equal) host results."""
    runs = []
    for _ in range(2):
        dev = [_hip.DevArray.from_host(a) for a in outputs]
        _hip.check(call(*[a.ptr for a in dev]))
        _hip.check(_hip.lib().cleora_stream_sync(None))
        runs.append([a.to_host() for a in dev])
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*runs))
    return runs[0]


def _assign(x, d, cent, previous):
    """cleora_kmeans_assign_dev on the leading d columns of x (ldx = x.shape[1]): (labels, cosine, changed)."""
    L, (n, ldx), k = _hip.lib(), x.shape, len(cent)
    dx, dc = _hip.DevArray.from_host(x), _hip.DevArray.from_host(cent)
    ws = _hip.DevArray((L.cleora_kmeans_workspace(n, d, k),), np.uint8)
    labels, cos, changed = _twice(lambda lp, cp, chp: L.cleora_kmeans_assign_dev(dx.ptr, ldx, n, d, dc.ptr, k, lp, cp, chp, ws.ptr, None),
                                  [previous.astype(np.uint32), np.full(n, 9.0, np.float32), np.full(2, 7, np.uint32)])
    return labels.astype(np.int64), cos, int(changed.view(np.uint64)[0])


def _check_assign(labels, cos, x, d, cent):
    s, tol = _cosines(x[:, :d], cent), (d + 8) * 2.0 ** -23
    chosen = s[np.arange(len(s)), labels]
    print(f"max (row max - chosen) {np.max(s.max(axis=1) - chosen):.3g}, tol {tol:.3g}")
    assert (labels >= 0).all() and (labels < len(cent)).all()
    assert (chosen >= s.max(axis=1) - tol).all()
    if cos is not None:
        np.testing.assert_allclose(cos, chosen, rtol=0, atol=tol)


@pytest.mark.parametrize("n, d, k, ldx", [(2, 7, 2, 7), (63, 1, 2, 1), (65, 7, 64, 7), (200, 100, 127, 100), (333, 256, 129, 256),
                                          (130, 260, 5, 260), (310, 1024, 300, 1024), (700, 96, 300, 128)])
def test_assign(n, d, k, ldx):
    rng = np.random.default_rng(n + d + k)
    x = (rng.standard_normal((n, ldx)) * rng.uniform(0.1, 5.0, (n, 1))).astype(np.float32)
    cent, previous = _unit(rng.standard_normal((k, d)).astype(np.float32)), rng.integers(0, k, n)
    labels, cos, changed = _assign(x, d, cent, previous)
    _check_assign(labels, cos, x, d, cent)
    assert changed == np.count_nonzero(labels != previous)


def test_assign_zero_rows_take_label_0_with_cosine_0():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((200, 40)).astype(np.float32)
    x[[0, 63, 64, 199]] = 0.0
    cent = _unit(rng.standard_normal((130, 40)).astype(np.float32))
    labels, cos, _ = _assign(x, 40, cent, np.full(200, 3))
    _check_assign(labels, cos, x, 40, cent)
    assert (labels[[0, 63, 64, 199]] == 0).all() and (cos[[0, 63, 64, 199]] == 0.0).all()


def test_assign_exact_ties_take_the_lower_index():
    """Duplicate centroids (j, j') that meet in one lane, across lane halves, accumulators, waves and centroid tiles."""
    rng = np.random.default_rng(2)
    pairs = np.array([(0, 1), (2, 6), (10, 40), (20, 90), (5, 200), (130, 299)])
    cent = _unit(rng.standard_normal((300, 48)).astype(np.float32))
    cent[pairs[:, 1]] = cent[pairs[:, 0]]
    x = rng.standard_normal((400, 48)).astype(np.float32)
    copies = rng.permutation(400)[:120].reshape(6, 20)
    for (j, _), rows in zip(pairs, copies):
        x[rows] = cent[j]
    labels, cos, _ = _assign(x, 48, cent, np.zeros(400, np.int64))
    _check_assign(labels, cos, x, 48, cent)
    assert not np.isin(labels, pairs[:, 1]).any()
    for (j, _), rows in zip(pairs, copies):
        assert (labels[rows] == j).all()


@pytest.mark.parametrize("n, d, k, ldx", [(63, 7, 2, 7), (1500, 100, 129, 100), (300, 260, 5, 264), (700, 1024, 140, 1024)])
def test_update(n, d, k, ldx):
    """k = 2: every row in cluster 1.  Else cluster 0 holds more than two chunks of members, cluster 1 none, cluster 2 zero rows."""
    rng = np.random.default_rng(n + d)
    x = (rng.standard_normal((n, ldx)) * rng.uniform(0.1, 5.0, (n, 1))).astype(np.float32)
    labels = rng.integers(0, k, n)
    if k == 2:
        labels[:] = 1
    else:
        labels[labels == 1] = 0
        labels[: n // 2] = 0
        labels[-3:] = 2
        x[labels == 2] = 0.0
    old = _unit(rng.standard_normal((k, d)).astype(np.float32))
    L = _hip.lib()
    dx, dl = _hip.DevArray.from_host(x), _hip.DevArray.from_host(labels.astype(np.uint32))
    ws = _hip.DevArray((L.cleora_kmeans_workspace(n, d, k),), np.uint8)
    new, = _twice(lambda cp: L.cleora_kmeans_update_dev(dx.ptr, ldx, n, d, dl.ptr, cp, k, ws.ptr, None), [old])
    kept = [0] if k == 2 else [1, 2]
    assert np.array_equal(new[kept].view(np.uint32), old[kept].view(np.uint32))
    want = _update_ref(x[:, :d], labels, old)
    print(f"max |centroid - ref| {np.abs(new - want).max():.3g}")
    np.testing.assert_allclose(new, want, rtol=0, atol=1e-6)


def _planted(n_per, d, k, seed):
    rng = np.random.default_rng(seed)
    centres = _unit(rng.standard_normal((k, d)))
    planted = rng.permutation(np.repeat(np.arange(k), n_per))
    x = _unit(centres[planted] + 0.05 * rng.standard_normal((len(planted), d)) / np.sqrt(d)) * rng.uniform(0.2, 4.0, (len(planted), 1))
    return x.astype(np.float32), centres.astype(np.float32), planted


@pytest.mark.parametrize("seed", [0, 42])
def test_loop_one_iteration(seed):
    x, _, _ = _planted(40, 33, 9, seed)
    n, k = len(x), 9
    first, second = embed.kmeans(x, k, max_iterations=1, seed=seed), embed.kmeans(x, k, max_iterations=1, seed=seed)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    labels, cent, iterations = first
    start = _unit(x[np.random.default_rng(seed).choice(n, size=k, replace=False)])
    assert iterations == 1 and labels.dtype == np.int32 and cent.dtype == np.float32
    _check_assign(labels.astype(np.int64), None, x, 33, start)
    np.testing.assert_allclose(cent, _update_ref(x, labels, start), rtol=0, atol=1e-6)


def test_loop_fixpoint():
    x, _, _ = _planted(60, 20, 12, 5)
    first, second = embed.kmeans(x, 12, max_iterations=50, seed=5), embed.kmeans(x, 12, max_iterations=50, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    labels, cent, iterations = first
    assert 2 <= iterations <= 50
    _check_assign(labels.astype(np.int64), None, x, 20, cent)
    np.testing.assert_allclose(cent, _update_ref(x, labels, cent), rtol=0, atol=1e-6)


@pytest.mark.parametrize("n_per, d, k", [(40, 16, 5), (5, 260, 140)])
def test_loop_exact_on_planted_clusters(n_per, d, k):
    x, centres, planted = _planted(n_per, d, k, 7)
    top2 = np.sort(_cosines(x, centres), axis=1)[:, -2:]
    assert (top2[:, 1] - top2[:, 0] >= 0.1).all()
    labels, cent, iterations = embed.kmeans(x, k, max_iterations=100, init=centres)
    assert np.array_equal(labels, planted) and iterations == 2
    np.testing.assert_allclose(cent, _update_ref(x, planted, centres), rtol=0, atol=1e-6)


def test_public_path_and_accelerate():
    rng = np.random.default_rng(11)
    g = SparseMatrix.from_iterator(iter([f"{i} {j}" for i, j in zip(range(300), rng.integers(0, 300, 300))]), "complex::reflexive::node")
    x, _, _ = _planted(50, 24, 6, 8)
    labels, _, _ = embed.kmeans(x, 6, max_iterations=30, seed=7)
    got = variants.detect_communities_kmeans(g, x, 6, max_iterations=30, seed=7)
    assert got == {eid: int(labels[i]) for i, eid in enumerate(g.entity_ids)} and len(set(got.values())) > 1
    calls = []
    community = types.SimpleNamespace(detect_communities_kmeans=lambda graph, emb, k, *a, **kw: calls.append(k) or "original")
    pkg = cleora_amd.accelerate(types.SimpleNamespace(embed=lambda *a, **kw: None, community=community))
    assert pkg.community.detect_communities_kmeans(g, x, 6, max_iterations=30, seed=7) == got and calls == []
    assert pkg.community.detect_communities_kmeans(g, x, variants.KMEANS_MAX_K + 1) == "original"
    assert pkg.community.detect_communities_kmeans(types.SimpleNamespace(entity_ids=g.entity_ids), x, 6) == "original"
    assert calls == [variants.KMEANS_MAX_K + 1, 6]
