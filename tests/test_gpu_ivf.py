"""GPU: the IVF index (csrc/ivf.hip: cleora_ivf_build_dev, cleora_ivf_search_dev) and cleora_amd.search on top of it, against
cosines in float64 from the same f32 input.  The device's own probes_out is the probe set P(q) (a near-tie between two centroids
cannot change the candidates under the test); candidates are the rows whose label is in P(q); expected: their cosines under
np.lexsort on (row, score), the query's own row at -2 with exclude_self.  Scores position by position and every returned index's
own score to atol 3e-6 (tests/test_gpu_knn.py's tolerance for the same arithmetic).  Labels and centroids are made here, not by
k-means, so the lists are exact.  Every call runs twice and must give the same bits."""
import numpy as np
import pytest

from cleora_amd import _hip, embed, search

pytestmark = pytest.mark.gpu
NO_ROW = 0xFFFFFFFF


def _twice(call, outs):
    runs = []
    for _ in range(2):
        bufs = [_hip.DevArray.from_host(np.zeros(shape, dt)) for shape, dt in outs]      # list_rows: unlisted rows leave a tail unwritten
        _hip.check(call(*[b.ptr for b in bufs]))
        _hip.check(_hip.lib().cleora_stream_sync(None))
        runs.append([b.to_host() for b in bufs])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return runs[0]


def _build(x, d, labels, nlist):
    """The layout of the leading d columns of x (ldx = x.shape[1]); list_ptr / list_rows are checked against the labels here."""
    L = _hip.lib()
    n, ldx = x.shape
    dev = {"x": _hip.DevArray.from_host(x), "n": n, "d": d, "ldx": ldx, "nlist": nlist}
    dl = _hip.DevArray.from_host(labels.astype(np.uint32))
    ws = _hip.DevArray((L.cleora_ivf_build_workspace(n, nlist),), np.uint8)
    dev["xs"] = _hip.DevArray((L.cleora_ivf_xs_bytes(n, d, nlist),), np.uint8)
    lp, lr = _twice(lambda p, r: L.cleora_ivf_build_dev(dev["x"].ptr, ldx, n, d, dl.ptr, nlist, p, r, dev["xs"].ptr, ws.ptr, None),
                    [((nlist + 1,), np.uint64), ((n,), np.uint32)])
    want = [np.flatnonzero(labels == c) for c in range(nlist)]
    assert np.array_equal(lp, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    assert np.array_equal(lr[:lp[-1]], np.concatenate(want))
    dev["list_ptr"], dev["list_rows"] = _hip.DevArray.from_host(lp), _hip.DevArray.from_host(lr)
    return dev


def _search(dev, cent, nprobe, k, dense=None, rows=None, exclude_self=False, ws_queries=0):
    L = _hip.lib()
    nq = len(dense) if rows is None else len(rows)
    dc = _hip.DevArray.from_host(cent)
    dq = _hip.DevArray.from_host(np.asarray(rows, np.uint32) if dense is None else dense)
    ws = _hip.DevArray((L.cleora_ivf_search_workspace(dev["n"], dev["d"], dev["nlist"], nprobe, k, ws_queries or nq),), np.uint8)
    return _twice(lambda oi, os_, pr: L.cleora_ivf_search_dev(
        dev["list_ptr"].ptr, dev["list_rows"].ptr, dev["xs"].ptr, dev["x"].ptr, dev["ldx"], dev["n"], dev["d"], dc.ptr, dev["nlist"],
        dq.ptr if dense is not None else None, dq.ptr if dense is None else None, nq, nprobe, k, 1 if exclude_self else 0, oi, os_, pr,
        ws.ptr, ws_queries, None), [((nq, k), np.uint32), ((nq, k), np.float32), ((nq, nprobe), np.uint32)])


def _unit(a):
    a = a.astype(np.float64)
    return a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-10)


def _check(got, x, labels, cent, nprobe, k, dense=None, rows=None, exclude_self=False, exact=False, all_lists=False):
    idx, sc, probes = got
    nlist, xn = len(cent), _unit(x)
    q = _unit(dense) if rows is None else xn[np.asarray(rows)]
    sims = np.einsum("qd,nd->qn", np.ascontiguousarray(q), xn)       # one summation order for every pair: duplicates tie exactly
    if exclude_self:
        sims[np.arange(len(q)), np.asarray(rows)] = -2.0
    cs = q @ _unit(cent).T
    assert probes.max() < nlist and all(len(set(p)) == nprobe for p in probes)
    assert (np.take_along_axis(cs, probes.astype(np.int64), 1) >= np.sort(cs, axis=1)[:, [-nprobe]] - 3e-6).all()
    worst = 0.0
    for j in range(len(q)):
        cand = np.flatnonzero(labels < nlist if all_lists else np.isin(labels, probes[j]))
        order = cand[np.lexsort((cand, sims[j, cand]))[::-1][:k]]
        m = len(order)
        assert (idx[j, m:] == NO_ROW).all() and (sc[j, m:] == -np.inf).all() and (idx[j, :m] != NO_ROW).all(), (j, m, idx[j], sc[j])
        assert np.isin(idx[j, :m], cand).all(), (j, idx[j])
        worst = max([worst] + list(np.abs(sc[j, :m] - sims[j, order])) + list(np.abs(sc[j, :m] - sims[j, idx[j, :m]])))
        if exact:
            assert np.array_equal(idx[j, :m], order), (j, idx[j], order)
    print(f"max |score - ref| {worst:.3g}")
    assert worst <= 3e-6


def _data(n, d, lengths, seed, ld=None, spare=0):
    """n rows in lists of the given lengths (the last takes what is left but `spare` rows, whose label is >= nlist), labels in a
    random order; centroid c = the normalised mean of its members' directions (a random unit row for an empty list)."""
    rng = np.random.default_rng(seed)
    lengths = list(lengths) + [n - spare - sum(lengths)]
    nlist = len(lengths)
    labels = rng.permutation(np.concatenate([np.repeat(np.arange(nlist), lengths), np.arange(spare) + nlist + 5])).astype(np.int64)
    cent = rng.standard_normal((nlist, d))
    x = (cent[np.minimum(labels, nlist - 1)] + 0.7 * rng.standard_normal((n, d))).astype(np.float32)
    if ld:
        x = np.concatenate([x, rng.standard_normal((n, ld - d)).astype(np.float32)], 1)
    for c in range(nlist):
        if lengths[c]:
            cent[c] = _unit(x[labels == c, :d]).mean(0)
    return x, labels, _unit(cent).astype(np.float32)


LENGTHS = [0, 1, 127, 128, 129, 1700, 500]       # + 400 in the last list and 15 rows in no list: n = 3000


@pytest.mark.parametrize("n,d,lengths,nprobe,k,form,nq,exclude_self", [
    pytest.param(3000, 100, LENGTHS, 3, 10, "rows", 150, True, id="list-lengths-rows-repeats-zero-rows"),
    pytest.param(3000, 100, LENGTHS, 1, 10, "centroids", 78, False, id="k-beyond-the-union"),
    pytest.param(3000, 100, LENGTHS, 8, 32, "dense", 70, False, id="nprobe-is-nlist-k32"),
    pytest.param(300, 7, [150], 2, 10, "dense", 1, False, id="one-query"),
    pytest.param(300, 7, [150], 2, 10, "dense", 64, False, id="64-queries-on-a-list"),
    pytest.param(300, 7, [150], 2, 10, "dense", 65, False, id="65-queries-on-a-list"),
    pytest.param(300, 7, [150], 2, 10, "rows", 200, True, id="200-queries-on-a-list"),
    pytest.param(600, 1, [100, 200, 50], 2, 32, "rows", 600, True, id="d1"),
    pytest.param(600, 256, [100, 200, 50], 2, 32, "rows", 600, False, id="d256-resident-limit"),
    pytest.param(600, 1024, [100, 200, 50], 2, 1, "dense", 90, False, id="d1024-chunked-k1"),
    pytest.param(1000, 32, [25] * 39, 32, 10, "dense", 100, False, id="nlist40-nprobe32"),
    pytest.param(1000, 96, [300, 300], 2, 10, "rows-ld128", 130, True, id="leading-dimension"),
])
def test_search(n, d, lengths, nprobe, k, form, nq, exclude_self):
    x, labels, cent = _data(n, d, lengths, n + d + nq, ld=128 if form.endswith("ld128") else None, spare=15 if n == 3000 else 0)
    rng = np.random.default_rng(nq)
    if n == 3000:
        x[[3, 1500, 2999]] = 0.0                                  # zero rows as candidates
    dense = rows = None
    if form.startswith("rows"):
        rows = np.concatenate([[n - 1, 0, 0, 3, 3], rng.integers(0, n, nq)])[:nq] if nq < n else np.arange(n)
    else:
        dense = rng.standard_normal((nq, d)).astype(np.float32)
        dense[-1] = 0.0                                           # a zero query
        if form == "centroids":                                   # the first queries ARE the centroids: each probes its own list
            dense[:len(cent)] = 3.0 * cent
    got = _search(_build(x, d, labels, len(cent)), cent, nprobe, k, dense, rows, exclude_self)
    _check(got, x[:, :d], labels, cent, nprobe, k, dense, rows, exclude_self)
    if form == "centroids":
        assert (got[0][0] == NO_ROW).all() and (got[0][1, 1:] == NO_ROW).all() and got[0][1, 0] != NO_ROW     # lists of 0 and 1 rows


def test_exact_duplicates():
    x, labels, cent = _data(500, 48, [100, 250], 6)
    x, labels = np.repeat(x, 2, 0), np.repeat(labels, 2)
    x[300:400], labels[300:400] = x[300], labels[300]
    rows = np.arange(0, 1000, 3)
    _check(_search(_build(x, 48, labels, 3), cent, 2, 10, rows=rows, exclude_self=True), x, labels, cent, 2, 10, rows=rows,
           exclude_self=True, exact=True)


def test_all_lists_probed_is_brute_force():
    x, labels, cent = _data(2000, 64, [10, 700, 0, 290], 11, spare=40)
    rows = np.arange(0, 2000, 7)
    got = _search(_build(x, 64, labels, 5), cent, 5, 10, rows=rows, exclude_self=True)
    _check(got, x, labels, cent, 5, 10, rows=rows, exclude_self=True, all_lists=True)


def test_more_queries_than_the_workspace_was_sized_for():
    x, labels, cent = _data(1500, 40, [200, 600, 90], 12)
    dense = np.random.default_rng(13).standard_normal((300, 40)).astype(np.float32)
    dev = _build(x, 40, labels, 4)
    got = _search(dev, cent, 2, 10, dense, ws_queries=100)        # batches of 128, 128 and 44 queries
    _check(got, x, labels, cent, 2, 10, dense)
    for a, b in zip(got, _search(dev, cent, 2, 10, dense)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_public_classes():
    class Graph:
        entity_ids = [f"e{i}" for i in range(2000)]
        def get_entity_index(self, e):
            return int(e[1:])
    x = _data(2000, 32, [60] * 30, 14)[0]
    ivf = search.IVFIndex(x, nlist=12, nprobe=3, train_size=500)
    assert ivf.nlist == 12 and ivf.list_sizes.sum() == 2000 and ivf.centroids.shape == (12, 32)
    want_i, want_s = embed.nearest_neighbours(x, k=10)
    idx, sc = ivf.search_rows(k=10, nprobe=12)                    # every list: the exact answer
    assert idx.dtype == np.uint32 and sc.dtype == np.float32 and idx.shape == sc.shape == (2000, 10)
    np.testing.assert_allclose(sc, want_s, rtol=0, atol=3e-6)
    own = np.einsum("qkd,qd->qk", _unit(x)[idx.astype(np.int64)], _unit(x))
    np.testing.assert_allclose(sc, own, rtol=0, atol=3e-6)
    idx3, sc3 = ivf.search(x[:70], k=5)                           # nprobe = 3: a row's best match is itself, in its own list
    assert idx3.shape == (70, 5) and (idx3[:, 0] == np.arange(70)).all() and (sc3[:, 0] > 1 - 1e-5).all()
    ann = search.ANNIndex(Graph(), x, method="ivf", nlist=12, nprobe=12)
    for res in (ann.query("e7", top_k=10), search.ANNIndex(Graph(), x, method="brute").query("e7", top_k=10)):
        assert [set(r) for r in res] == [{"entity_id", "index", "similarity"}] * 10 and all(r["entity_id"] == f"e{r['index']}" for r in res)
        np.testing.assert_allclose([r["similarity"] for r in res], want_s[7], rtol=0, atol=3e-6)
    assert ann.query_vector(x[7], top_k=3)[0]["index"] == 7
    with pytest.raises(ValueError, match="top_k must be positive"):
        ann.query("e7", top_k=0)
    with pytest.raises(ValueError, match="ivf"):
        search.ANNIndex(Graph(), x, method="hnsw")
