"""CLEORA_F_GATHER_F16: cleora_propagate_hf_dev (csrc/spmm_h.hip: gather f16, sum and store f32) bit for bit against the f32 CPU oracle
on the widened input; cleora_project_bounded_h_dev (csrc/project_f16.hip) bit for bit against the projection without the copy; the loop
against an f64 numpy model of the reorganised loop, with a bar taken from the model's own sensitivity to the rounding."""
import ctypes

import numpy as np
import pytest

import cleora_amd
import oracle
from cleora_amd import _hip, sharded
from cleora_amd import embed as dev_embed
from cleora_amd.pycleora import SparseMatrix
from tests.graphs import random_csr

gpu = pytest.mark.gpu
L2, L1 = _hip.F_L2NORM, _hip.F_L1NORM
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def model(rowptr, col, val, x16, flags):
    """widen exactly, the oracle's in-order f32 sums, then the epilogue in f32: nothing is rounded to f16 on the way out"""
    y = oracle.spmm(rowptr, col, val, x16.astype(np.float32))
    if flags & L2:
        y = oracle.l2_normalize(y)
    if flags & L1:       # s = sum |v| for j = 0 .. d-1 in f32, v / max(s, 1e-10): a true division
        s = np.cumsum(np.abs(y), axis=1, dtype=np.float32)[:, -1:]
        y = y / np.maximum(s, np.float32(1e-10))
    return y.astype(np.float32)


def run_hf(g, kind, x16, flags=0):
    dx, dy = _hip.DevArray.from_host(x16), _hip.DevArray((g.info().n_rows, x16.shape[1]), np.float32)
    _hip.lib().cleora_memset(dy.ptr, 0xFF, dy.nbytes, None)  # poison (NaN): every row must be written
    g.propagate_hf(kind, dx, dy, flags)
    _hip.check(_hip.lib().cleora_stream_sync(None))
    return dy.to_host()


@gpu
@pytest.mark.parametrize("flags,hot", [(0, False), (L2, False), (L1, False), (L2, True)])
@pytest.mark.parametrize("d", [4, 8, 64, 100, 256, 260, 512, 1024, 2048])
def test_ordinary_rows_bit_equal(d, flags, hot):
    n = 3000 if d <= 512 else 600
    rowptr, col, vl, vs = random_csr(n, 12, seed=d, empty_frac=0.05)
    assert np.diff(rowptr.astype(np.int64)).max() <= 256
    x16 = np.random.default_rng(d + 1).standard_normal((n, d)).astype(np.float16)
    g = _hip.Graph.from_host(rowptr, col, vl, vs)
    if hot:
        g.set_hot_cache(d * 2 * 200)
    for kind, val in ((_hip.LEFT, vl), (_hip.SYMMETRIC, vs)):
        np.testing.assert_array_equal(bits(run_hf(g, kind, x16, flags)), bits(model(rowptr, col, val, x16, flags)))


@gpu
@pytest.mark.parametrize("flags", [0, L2])
@pytest.mark.parametrize("d", [64, 256, 1024])
def test_long_rows_segmented(d, flags):
    n, hubs = 4000, [(17, 5000), (3999, 20000), (5, 257), (6, 256)]
    rowptr, col, vl, _ = random_csr(n, 8, seed=11, hubs=hubs)
    x16 = np.random.default_rng(12).standard_normal((n, d)).astype(np.float16)
    g = _hip.Graph.from_host(rowptr, col, vl)
    assert g.info().hub_threshold == 256 and g.info().n_hub_rows == 3
    got = run_hf(g, _hip.LEFT, x16, flags)
    np.testing.assert_array_equal(bits(run_hf(g, _hip.LEFT, x16, flags)), bits(got))      # deterministic
    long_rows = [r for r, deg in hubs if deg > 256]
    others = np.setdiff1d(np.arange(n), long_rows)
    x64 = x16.astype(np.float64)
    np.testing.assert_array_equal(bits(got[others]), bits(model(rowptr, col, vl, x16, flags)[others]))
    for r in long_rows:
        e = slice(int(rowptr[r]), int(rowptr[r + 1]))
        ref = vl[e].astype(np.float64) @ x64[col[e]]
        bar = 2e-6 * (np.abs(vl[e]).astype(np.float64) @ np.abs(x64[col[e]]))         # the segmented sum's bar
        if flags & L2:
            norm = np.sqrt((ref * ref).sum())
            ref, bar = ref / norm, bar / norm + (d + 4) * 2.0 ** -24 * np.abs(ref / norm)   # + in-order f32 sum of squares, scaling
        assert np.all(np.abs(got[r].astype(np.float64) - ref) <= bar + 2.0 ** -24), r
    # the same segments, the same order, the same f32 adds as the f32 kernel's segmented schedule on the widened input — where that
    # kernel's finish pass also adds the segments in four runs (a wavefront per row: d >= 256; at d = 64 its 16-lane groups make 16 runs)
    if d >= 256:
        dx, dy = _hip.DevArray.from_host(x16.astype(np.float32)), _hip.DevArray((n, d), np.float32)
        _hip.check(_hip.lib().cleora_propagate_dev(g.handle, _hip.LEFT, dx.ptr, d, d, dy.ptr, d, flags | _hip.F_HUB_SEGMENTS, 0.0, None,
                                                   None, None, None))
        _hip.check(_hip.lib().cleora_stream_sync(None))
        np.testing.assert_array_equal(bits(got), bits(dy.to_host()))


@gpu
@pytest.mark.parametrize("norm,scaled", [(1, True), (2, True), (1, False)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5003])
def test_projection_with_the_f16_copy(n, norm, scaled):
    """inputs as in test_bounded_projection_on_the_f16_matrix_cores (tests/test_gpu_whiten.py)"""
    L, d = _hip.lib(), 256
    rng = np.random.default_rng(n + 7 * norm + scaled)
    bound = np.where(rng.random(n) < 0.8, 1.0, 10 ** (rng.random(n) * 4 - 1)).astype(np.float32)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x *= (bound * (0.2 + 0.8 * rng.random(n)))[:, None].astype(np.float32)
    x = np.minimum(np.maximum(x, -bound[:, None]), bound[:, None]).astype(np.float32)
    rowscale = (bound * (2 * rng.random(n) - 1)).astype(np.float32)
    mean = np.clip(rng.standard_normal(d) * 0.05, -1, 1).astype(np.float32)
    t = (rng.standard_normal((d, d)) * 10 ** (rng.random(d) * 5 - 2)[None, :]).astype(np.float32)
    dx, dm, dt, ds, db = (_hip.DevArray.from_host(a) for a in (x, mean, t, rowscale, bound))
    outs = [_hip.DevArray.from_host(np.full((n + 1, d), 7.0, np.float32)) for _ in range(2)]    # one row more than a call may touch
    oh = _hip.DevArray.from_host(np.full((n + 1, d), 7.0, np.float16))
    form = ctypes.c_int(-1)
    _hip.check(L.cleora_project_bounded_dev(dx.ptr, d, n, d, dm.ptr, dt.ptr, d, outs[0].ptr, d, ds.ptr if scaled else None, db.ptr, norm,
                                            None, None, None))
    _hip.check(L.cleora_project_bounded_h_dev(dx.ptr, d, n, d, dm.ptr, dt.ptr, d, outs[1].ptr, d, ds.ptr if scaled else None, db.ptr,
                                              norm, None, ctypes.byref(form), oh.ptr, d, None))
    _hip.check(L.cleora_stream_sync(None))
    want, got, got_h = outs[0].to_host(), outs[1].to_host(), oh.to_host()
    assert form.value == 1 and np.isfinite(got).all()
    np.testing.assert_array_equal(bits(got), bits(want))
    assert (got[n] == 7.0).all() and (got_h[n] == 7.0).all(), "the ragged last tile wrote past row n"
    np.testing.assert_array_equal(got_h[:n].view(np.uint16), got[:n].astype(np.float16).view(np.uint16))


def spmm64(rowptr, col, val, x):
    out = np.zeros((rowptr.shape[0] - 1, x.shape[1]))
    np.add.at(out, np.repeat(np.arange(out.shape[0]), np.diff(rowptr.astype(np.int64))), val.astype(np.float64)[:, None] * x[col])
    return out


def loop_model(rowptr, col, val, x0, iters, rw, rn16):
    """f64: Y = norm(A E_0 [blend]); per iteration fit (mu, T) on Y, Y <- norm((alpha (A rn16(Y) - s mu^T) + rw (Y - mu)) T); whiten(Y)"""
    norm = lambda v: v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-10)

    def fit(y):
        mu = y.mean(axis=0)
        lam, vec = np.linalg.eigh((y - mu).T @ (y - mu) / (y.shape[0] - 1))
        return mu, vec[:, ::-1] / np.sqrt(np.maximum(lam[::-1], 1e-10))
    x0 = x0.astype(np.float64)
    s = spmm64(rowptr, col, val, np.ones((x0.shape[0], 1)))
    y = norm((1 - rw) * spmm64(rowptr, col, val, x0) + rw * x0)
    for _ in range(iters - 1):
        mu, t = fit(y)
        yg = y.astype(np.float16).astype(np.float64) if rn16 else y
        y = norm(((1 - rw) * (spmm64(rowptr, col, val, yg) - s * mu) + rw * (y - mu)) @ t)
    mu, t = fit(y)
    return (y - mu) @ t


@gpu
@pytest.mark.parametrize("n,d,iters,kind,rw", [(6000, 256, 4, 1, 0.0), (20000, 64, 6, 0, 0.0), (5000, 512, 3, 0, 0.0), (6000, 256, 4, 1, 0.3)])
def test_loop_against_the_f64_model(n, d, iters, kind, rw):
    """The fused copy (d = 256), the convert pass behind both forms of the split projection (d = 64, 512) and behind the blend.  delta =
    what rounding Y moves in the f64 model (measured on the GPU run: 1.5e-4, 3.9e-4, 1.0e-4, 7.3e-5; the GPU loop 1.4e-4, 4.0e-4, 9.0e-5,
    8.1e-5); the bar: 2 delta (another realisation of the rounding noise) + 1e-4 (this loop's existing bar) from the unrounded model."""
    rowptr, col, vl, vs = random_csr(n, 9, seed=n + d, empty_frac=0.02, hubs=[(13, 1400)])
    val = vs if kind else vl
    x0 = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    rows = np.random.default_rng(1).choice(n, 400, replace=False)
    cos = lambda e: (lambda u: u @ u.T)(e[rows].astype(np.float64) / np.linalg.norm(e[rows].astype(np.float64), axis=1, keepdims=True))
    exact = cos(loop_model(rowptr, col, val, x0, iters, rw, False))
    delta = np.abs(cos(loop_model(rowptr, col, val, x0, iters, rw, True)) - exact).max()
    g = _hip.Graph.from_host(rowptr, col, vl, vs)
    outs = [np.empty((n, d), np.float32) for _ in range(2)]
    for out, flag in zip(outs, (0, _hip.F_GATHER_F16)):
        _hip.check(_hip.lib().cleora_embed(g.handle, None, _hip.ptr(x0), kind, d, iters, 0, rw, 0.0, _hip.F_WHITEN | flag, _hip.ptr(out), None))
        assert np.isfinite(out).all()
    dev = [np.abs(cos(o) - exact).max() for o in outs]
    print(f"n={n} d={d} iters={iters} rw={rw}: delta(models)={delta:.3g}  gpu f32 gather={dev[0]:.3g}  gpu f16 gather={dev[1]:.3g}")
    assert not np.array_equal(outs[0], outs[1])
    assert dev[1] <= 2 * delta + 1e-4


@gpu
def test_install_gather_dtype_surface():
    rng = np.random.default_rng(3)
    lines = [f"u{int(a)} u{int(b)}" for a, b in zip(rng.integers(0, 1500, 12000), rng.integers(0, 1500, 12000))]
    g = SparseMatrix.from_iterator(iter(lines), "complex::reflexive::node")
    runs = lambda: [dev_embed.embed(g, 64, 4), dev_embed.embed(g, 64, 3, convergence_threshold=1e-30), dev_embed.embed(g, 6, 3)]
    f32 = runs()
    try:
        cleora_amd.install(gather_dtype="f16")
        f16 = runs()
        direct = np.empty_like(f16[0])
        _hip.check(_hip.lib().cleora_embed(g._graph().handle, _hip.ptr(g._arr["hashes"]), None, _hip.LEFT, 64, 4, 0, 0.0, 0.0,
                                           _hip.F_WHITEN | _hip.F_GATHER_F16, _hip.ptr(direct), None))
        np.testing.assert_array_equal(f16[0], direct)
        assert not np.array_equal(f16[0], f32[0])
        for a, b in zip(f16[1:], f32[1:]):            # a preference: with a threshold, or at d % 4 != 0, the call runs in f32 as before
            np.testing.assert_array_equal(a, b)
        cleora_amd.install(gather_dtype="f32")
        np.testing.assert_array_equal(dev_embed.embed(g, 64, 4), f32[0])
    finally:
        cleora_amd.install(gather_dtype="f32")


F = _hip.F_WHITEN | _hip.F_GATHER_F16
EMBED_REFUSALS = {"no_whiten": (8, _hip.F_GATHER_F16, 0.0), "threshold": (8, F, 1e-3), "d6": (6, F, 0.0), "d2052": (2052, F, 0.0),
                  "iterate_f16_whiten": (8, _hip.F_WHITEN | _hip.F_ITERATE_F16, 0.0)}


@gpu
@pytest.mark.parametrize("case", [*EMBED_REFUSALS, "sharded", "colsharded", "multi", "hf_residual", "hf_rowsq", "hf_odd_ldy"])
def test_refusals(case):
    n, L = 64, _hip.lib()
    rowptr, col, vl, _ = random_csr(n, 4, seed=1)
    g = _hip.Graph.from_host(rowptr, col, vl)
    d, flags, thr = EMBED_REFUSALS.get(case, (8, F, 0.0))
    x0, dx = np.zeros((n, d), np.float32), _hip.DevArray((n, d), np.float32)
    if case in EMBED_REFUSALS:
        rc = L.cleora_embed(g.handle, None, _hip.ptr(x0), _hip.LEFT, d, 2, 0, 0.0, thr, flags, _hip.ptr(x0), None)
    elif case == "sharded":
        rc = L.cleora_embed_sharded(sharded.DeviceShardedGraph(n, rowptr, col, vl).handle, dx.ptr, _hip.LEFT, d, 2, 0.0, 0.0, F, None)
    elif case == "colsharded":
        cg = sharded.DeviceColShardedGraph(n, rowptr, col, vl, None, d, None, 1)
        rc = L.cleora_embed_colsharded(cg.handle, dx.ptr, _hip.LEFT, 2, 0.0, 0.0, F, None)
    elif case == "multi":
        m = _hip.MultiGraph.from_host([0, 0], rowptr, col, vl)
        rc = L.cleora_multi_embed(m.handle, None, _hip.ptr(x0), _hip.LEFT, d, 2, 0, 0.0, 0.0, F, _hip.ptr(x0), None)
    else:
        ldy = 9 if case == "hf_odd_ldy" else 8
        x, y = _hip.DevArray((n, 8), np.float16), _hip.DevArray((n, ldy), np.float32)
        rc = L.cleora_propagate_hf_dev(g.handle, _hip.LEFT, x.ptr, 8, 8, y.ptr, ldy,
                                       {"hf_residual": _hip.F_RESIDUAL, "hf_rowsq": _hip.F_ROWSQ}.get(case, 0), None)
    assert rc == _hip.E_INVALID and _hip.last_error()


def test_install_rejects_unknown_gather_dtype():
    with pytest.raises(ValueError):
        cleora_amd.install(gather_dtype="bf16")
    with pytest.raises(ValueError):
        cleora_amd.install(devices=[0, 1], gather_dtype="f16")
