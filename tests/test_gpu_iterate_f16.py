"""f16-stored iterates (csrc/spmm_h.hip, CLEORA_F_ITERATE_F16) against a host model: widen the f16 input exactly, run the f32 CPU
oracle, round once to f16 (NumPy's cast: to nearest even, subnormals kept).  Ordinary rows must match the model's uint16 bits;
rows longer than hub_threshold are summed in segments and are held to the segmented sum's bar plus one f16 rounding."""
import ctypes

import numpy as np
import pytest

import cleora_amd
import oracle
from cleora_amd import _hip
from cleora_amd.pycleora import SparseMatrix
from tests.graphs import random_csr

gpu = pytest.mark.gpu
L2, RES, SQ, SQ64 = _hip.F_L2NORM, _hip.F_RESIDUAL, _hip.F_SQDIFF, _hip.F_SQDIFF64


def model(rowptr, col, val, x16, flags=0, rw=0.0):
    x = x16.astype(np.float32)
    y = oracle.spmm(rowptr, col, val, x)
    if 0.0 < rw < 1.0:
        y = (np.float32(1.0) - np.float32(rw)) * y + np.float32(rw) * x      # f32: alpha*dst + rw*src
    if flags & L2:
        y = oracle.l2_normalize(y)
    return y.astype(np.float16)


def run_h(g, kind, x16, flags=0, rw=0.0, want_sqdiff=False):
    n, d = g.info().n_rows, x16.shape[1]
    dx = _hip.DevArray.from_host(x16)
    dy = _hip.DevArray((n, d), np.float16)
    _hip.lib().cleora_memset(dy.ptr, 0xFF, dy.nbytes, None)  # poison: every row must be written
    dsq = _hip.DevArray((n,), np.float64) if want_sqdiff else None
    g.propagate_h(kind, dx, dy, flags, rw, row_sqdiff=dsq)
    _hip.check(_hip.lib().cleora_stream_sync(None))
    return (dy.to_host(), dsq.to_host()) if want_sqdiff else dy.to_host()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@gpu
@pytest.mark.parametrize("flags,scale,hot", [(0, 1.0, False), (L2, 1.0, False), (0, 2.0 ** -12, False), (L2, 1.0, True)])
@pytest.mark.parametrize("d", [4, 8, 64, 100, 256, 260, 512, 1024, 2048])
def test_ordinary_rows_bit_equal(d, flags, scale, hot):
    """Every shape of the dispatch (sub-wave groups, 8- and 16-byte chunks, partial last chunks), outputs in f16's subnormal range
    (scale 2^-12), and the marked-column path (hot)."""
    n = 3000 if d <= 512 else 600
    rowptr, col, vl, vs = random_csr(n, 12, seed=d, empty_frac=0.05)
    assert np.diff(rowptr.astype(np.int64)).max() <= 256
    x16 = (np.random.default_rng(d + 1).standard_normal((n, d)) * scale).astype(np.float16)
    g = _hip.Graph.from_host(rowptr, col, vl, vs)
    if hot:
        g.set_hot_cache(d * 2 * 200)
    for kind, val in ((_hip.LEFT, vl), (_hip.SYMMETRIC, vs)):
        want = model(rowptr, col, val, x16, flags)
        if scale != 1.0:
            tiny = np.abs(want.astype(np.float32))
            assert ((tiny > 0) & (tiny < 2.0 ** -14)).mean() > 0.1          # the case is about subnormal outputs
        np.testing.assert_array_equal(bits(run_h(g, kind, x16, flags)), bits(want))


@gpu
@pytest.mark.parametrize("sq64", [0, SQ64])
def test_residual_and_sqdiff_after_rounding(sq64):
    n, d, rw = 2000, 256, 0.3
    rowptr, col, vl, _ = random_csr(n, 10, seed=5)
    x16 = np.random.default_rng(6).standard_normal((n, d)).astype(np.float16)
    g = _hip.Graph.from_host(rowptr, col, vl)
    want = model(rowptr, col, vl, x16, L2, rw)
    got, sq = run_h(g, _hip.LEFT, x16, L2 | RES | SQ | sq64, rw, want_sqdiff=True)
    np.testing.assert_array_equal(bits(got), bits(want))
    w32, x32 = want.astype(np.float32), x16.astype(np.float32)
    delta = w32.astype(np.float64) - x32.astype(np.float64) if sq64 else (w32 - x32).astype(np.float64)
    np.testing.assert_allclose(sq, (delta * delta).sum(axis=1), rtol=1e-12)


@gpu
@pytest.mark.parametrize("flags", [0, L2])
@pytest.mark.parametrize("d", [256, 64, 1024])
def test_long_rows_segmented(d, flags):
    n, hubs = 4000, [(17, 5000), (3999, 20000), (5, 257), (6, 256)]
    rowptr, col, vl, _ = random_csr(n, 8, seed=11, hubs=hubs)
    x16 = np.random.default_rng(12).standard_normal((n, d)).astype(np.float16)
    g = _hip.Graph.from_host(rowptr, col, vl)
    assert g.info().hub_threshold == 256 and g.info().n_hub_rows == 3           # 256 edges: not a long row
    got = run_h(g, _hip.LEFT, x16, flags)
    np.testing.assert_array_equal(bits(run_h(g, _hip.LEFT, x16, flags)), bits(got))      # deterministic
    long_rows = [r for r, deg in hubs if deg > 256]
    others = np.setdiff1d(np.arange(n), long_rows)
    np.testing.assert_array_equal(bits(got[others]), bits(model(rowptr, col, vl, x16, flags)[others]))
    x64 = x16.astype(np.float64)
    for r in long_rows:
        e = slice(int(rowptr[r]), int(rowptr[r + 1]))
        ref = vl[e].astype(np.float64) @ x64[col[e]]
        bar = 2e-6 * (np.abs(vl[e]).astype(np.float64) @ np.abs(x64[col[e]]))         # the segmented sum's bar
        if flags & L2:
            norm = np.sqrt((ref * ref).sum())
            ref, bar = ref / norm, bar / norm + (d + 4) * 2.0 ** -24 * np.abs(ref / norm)   # + in-order f32 sum of squares, scaling
        g64 = got[r].astype(np.float64)
        assert np.all(np.abs(g64 - ref) <= bar + 2.0 ** -11 * np.maximum(np.abs(ref), np.abs(g64)) + 2.0 ** -24), r


def embed_f16(handle, hashes, d, iterations, rw=0.0, threshold=0.0, flags=0):
    out, ran = np.empty((hashes.shape[0], d), np.float32), ctypes.c_uint64(0)
    rc = _hip.lib().cleora_embed(handle, _hip.ptr(hashes), None, _hip.LEFT, d, iterations, 0, rw, threshold,
                                 _hip.F_ITERATE_F16 | flags, _hip.ptr(out), ctypes.byref(ran))
    return rc, out, int(ran.value)


def model_loop(rowptr, col, val, hashes, d, iterations, rw):
    """The iterates the loop holds (f16) and, from the second on, the RMSE its stop test computes (f32 difference, f64 sum)."""
    x16 = oracle.init(hashes, d, 0).astype(np.float16)
    rmse = {}
    for k in range(1, iterations + 1):
        new = model(rowptr, col, val, x16, L2, rw)
        if k >= 2:
            delta = (new.astype(np.float32) - x16.astype(np.float32)).astype(np.float64)
            rmse[k] = float(np.sqrt(np.float32((delta * delta).sum() / delta.size)))
        x16 = new
    return x16, rmse


@gpu
@pytest.mark.parametrize("d,rw", [(256, 0.0), (256, 0.3), (64, 0.0), (64, 0.3)])
def test_loop_bit_equal_to_iterated_model(d, rw):
    n = 2000
    rowptr, col, vl, _ = random_csr(n, 10, seed=21)
    hashes = np.random.default_rng(22).integers(0, 2 ** 63, n, dtype=np.uint64)
    g = _hip.Graph.from_host(rowptr, col, vl)
    rc, out, ran = embed_f16(g.handle, hashes, d, 4, rw)
    _hip.check(rc)
    want, _ = model_loop(rowptr, col, vl, hashes, d, 4, rw)
    assert ran == 4
    np.testing.assert_array_equal(out, want.astype(np.float32))


@gpu
def test_loop_convergence_stop():
    n, d = 2000, 64
    rowptr, col, vl, _ = random_csr(n, 10, seed=21)
    hashes = np.random.default_rng(22).integers(0, 2 ** 63, n, dtype=np.uint64)
    _, rmse = model_loop(rowptr, col, vl, hashes, d, 10, 0.0)
    k = next(k for k in range(2, 10) if rmse[k + 1] < 0.99 * rmse[k])       # first pair of iterations more than 1 % apart
    threshold = float(np.sqrt(rmse[k] * rmse[k + 1]))
    stop = next(j for j in range(2, 11) if rmse[j] < threshold)
    print(f"threshold between the RMSE of iterations {k} and {k + 1}: {rmse[k]:.6g} > {threshold:.6g} > {rmse[k + 1]:.6g}")
    g = _hip.Graph.from_host(rowptr, col, vl)
    rc, _, ran = embed_f16(g.handle, hashes, d, 10, 0.0, threshold)
    _hip.check(rc)
    assert ran == stop == k + 1


@gpu
def test_install_iterate_dtype_surface():
    rng = np.random.default_rng(3)
    lines = [f"u{int(a)} u{int(b)}" for a, b in zip(rng.integers(0, 1500, 12000), rng.integers(0, 1500, 12000))]
    g = SparseMatrix.from_iterator(iter(lines), "complex::reflexive::node")
    f32 = g.embed_fast(64, 4)
    try:
        cleora_amd.install(iterate_dtype="f16")
        f16 = g.embed_fast(64, 4)
        rc, direct, _ = embed_f16(g._graph().handle, g._arr["hashes"], 64, 4)
        _hip.check(rc)
        np.testing.assert_array_equal(f16, direct)
        assert not np.array_equal(f16, f32)
        np.testing.assert_allclose(f16, f32, rtol=0, atol=2.0 ** -9)            # 4 roundings of unit rows
        cleora_amd.install(iterate_dtype="f32")
        np.testing.assert_array_equal(g.embed_fast(64, 4), f32)
    finally:
        cleora_amd.install(iterate_dtype="f32")


@gpu
@pytest.mark.parametrize("case", ["whiten", "d6", "odd_ldx", "rowsq"])
def test_refusals(case):
    n = 64
    rowptr, col, vl, _ = random_csr(n, 4, seed=1)
    g = _hip.Graph.from_host(rowptr, col, vl)
    if case == "whiten":
        rc = embed_f16(g.handle, np.arange(n, dtype=np.uint64), 8, 2, flags=_hip.F_WHITEN)[0]
    else:
        d, ld = (6, 6) if case == "d6" else (8, 9) if case == "odd_ldx" else (8, 8)
        x, y, s = _hip.DevArray((n, ld), np.float16), _hip.DevArray((n, ld), np.float16), _hip.DevArray((n,), np.float32)
        rc = _hip.lib().cleora_propagate_h_dev(g.handle, _hip.LEFT, x.ptr, ld, d, y.ptr, ld, _hip.F_ROWSQ if case == "rowsq" else 0,
                                               0.0, None, s.ptr, None)
    assert rc == _hip.E_INVALID and _hip.last_error()


def test_install_rejects_unknown_iterate_dtype():
    with pytest.raises(ValueError):
        cleora_amd.install(iterate_dtype="bf16")
    with pytest.raises(ValueError):
        cleora_amd.install(devices=[0, 1], iterate_dtype="f16")
