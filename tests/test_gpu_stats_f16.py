"""CLEORA_F_STATS_F16: cleora_whiten_stats_h_dev (csrc/gram_h.hip: mean and centred Gram of f16-stored rows from v_mfma_f32_32x32x16_f16)
against numpy f64 on the same f16 values and beside the split-bf16 form; cleora_project_bounded_h_dev without the f32 rows bit for bit
against the copy variant; the loop on f16-only rows against an f64 model that fits and propagates the rounded rows."""
import numpy as np
import pytest

import cleora_amd
from cleora_amd import _hip, sharded
from cleora_amd import pycleora as _pyc
from tests.graphs import random_csr
from tests.test_gpu_gather_f16 import loop_model, spmm64

gpu = pytest.mark.gpu
F = _hip.F_WHITEN | _hip.F_GATHER_F16 | _hip.F_STATS_F16


@gpu
@pytest.mark.parametrize("d", [256, 512])
@pytest.mark.parametrize("n", [4096, 4099, 6151])
def test_statistics_from_f16_rows(n, d):
    """One slice of whole stages, a ragged 64-row stage, many folds; a diagonal block (d = 256) and diagonal + off-diagonal ones (512).
    e = ||G - G64||_F / ||G64||_F: the new form shares the split form's f32 accumulation (32 rows on the matrix cores, f32 over a fold)
    and lacks its shift, so e_new <= 4 e_old (a CPU model of the accumulation: 1.6e-7 uncentred against 8.6e-8 centred at n = 5003,
    plus one realisation of rounding).  Measured on an MI355X (profiles/stats_f16_c3.json): e_new 3.7e-8 .. 6.0e-8, e_old 2.2e-8 ..
    3.5e-8; with the split form's 2048-row folds the new form gave 2.8e-7 at n = 4096 — hence the 256-row folds below 2^20 rows."""
    L = _hip.lib()
    rng = np.random.default_rng(n + d)
    scales, off = np.linspace(0.3, 2.0, d), rng.standard_normal(d)
    off *= np.sqrt(0.25 * (scales ** 2).sum() / (off ** 2).sum())            # |mean|^2 ~ 0.2 after the normalisation
    x = rng.standard_normal((n, d)) * scales + off
    y16 = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)
    y64 = y16.astype(np.float64)
    mean = y64.mean(axis=0)
    gram = (y64 - mean).T @ (y64 - mean)
    assert 0.15 <= (mean ** 2).sum() <= 0.25
    dh, dx = _hip.DevArray.from_host(y16), _hip.DevArray.from_host(y16.astype(np.float32))
    ws = _hip.DevArray((L.cleora_whiten_workspace(n, d),), np.uint8)
    dm, dg = _hip.DevArray((d,), np.float64), _hip.DevArray((d, d), np.float64)

    def run(call):
        _hip.check(L.cleora_memset(dg.ptr, 0xFF, dg.nbytes, None))           # poison: every entry must be written
        _hip.check(call())
        _hip.check(L.cleora_stream_sync(None))
        return dm.to_host(), dg.to_host()
    m_new, g_new = run(lambda: L.cleora_whiten_stats_h_dev(dh.ptr, d, n, d, ws.ptr, dm.ptr, dg.ptr, None))
    m_again, g_again = run(lambda: L.cleora_whiten_stats_h_dev(dh.ptr, d, n, d, ws.ptr, dm.ptr, dg.ptr, None))
    _, g_old = run(lambda: L.cleora_whiten_stats_dev(dx.ptr, d, n, d, ws.ptr, 1, dm.ptr, dg.ptr, None))
    e_new, e_old = (float(np.linalg.norm(g - gram) / np.linalg.norm(gram)) for g in (g_new, g_old))
    print(f"n={n} d={d}: e_new={e_new:.3g} e_old={e_old:.3g} |d mean|={np.abs(m_new - mean).max():.3g}")
    assert np.abs(m_new - mean).max() <= 1e-12
    assert np.array_equal(g_new, g_new.T)
    assert e_new <= 4 * e_old
    assert np.array_equal(m_new, m_again) and np.array_equal(g_new, g_again)


@gpu
@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 5003])
def test_projection_storing_only_the_f16_rows(n, norm):
    L, d = _hip.lib(), 256
    rng = np.random.default_rng(n + norm)
    bound = np.where(rng.random(n) < 0.8, 1.0, 10 ** (rng.random(n) * 4 - 1)).astype(np.float32)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x *= (bound * (0.2 + 0.8 * rng.random(n)) / np.linalg.norm(x, axis=1))[:, None].astype(np.float32)
    rowscale = (bound * (2 * rng.random(n) - 1)).astype(np.float32)
    mean = np.clip(rng.standard_normal(d) * 0.05, -1, 1).astype(np.float32)
    t = (rng.standard_normal((d, d)) * 10 ** (rng.random(d) * 5 - 2)[None, :]).astype(np.float32)
    dx, dm, dt, ds, db = (_hip.DevArray.from_host(a) for a in (x, mean, t, rowscale, bound))
    out = _hip.DevArray((n, d), np.float32)
    oh = [_hip.DevArray.from_host(np.full((n + 1, d), 7.0, np.float16)) for _ in range(2)]     # one row more than a call may touch
    for o, h in ((out.ptr, oh[0]), (None, oh[1])):
        _hip.check(L.cleora_project_bounded_h_dev(dx.ptr, d, n, d, dm.ptr, dt.ptr, d, o, d, ds.ptr, db.ptr, norm, None, None, h.ptr, d, None))
    _hip.check(L.cleora_stream_sync(None))
    want, got = oh[0].to_host(), oh[1].to_host()
    assert np.isfinite(want[:n].astype(np.float32)).all()
    np.testing.assert_array_equal(got.view(np.uint16), want.view(np.uint16))
    assert (got[n] == 7.0).all(), "the ragged last tile wrote past row n"


def model_fit_on_rounded(rowptr, col, val, x0, iters):
    """loop_model (tests/test_gpu_gather_f16.py) with rw = 0, mean and transform fitted on the ROUNDED rows the SpMM gathers"""
    norm = lambda v: v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-10)

    def fit(y):
        mu = y.mean(axis=0)
        lam, vec = np.linalg.eigh((y - mu).T @ (y - mu) / (y.shape[0] - 1))
        return mu, vec[:, ::-1] / np.sqrt(np.maximum(lam[::-1], 1e-10))
    s = spmm64(rowptr, col, val, np.ones((x0.shape[0], 1)))
    y = norm(spmm64(rowptr, col, val, x0.astype(np.float64)))
    for _ in range(iters - 1):
        yg = y.astype(np.float16).astype(np.float64)
        mu, t = fit(yg)
        y = norm((spmm64(rowptr, col, val, yg) - s * mu) @ t)
    mu, t = fit(y)
    return (y - mu) @ t


@gpu
@pytest.mark.parametrize("n,d,iters,kind", [(6000, 256, 4, 1), (5000, 512, 3, 0), (20000, 64, 6, 0)])
def test_loop_on_f16_only_rows(n, d, iters, kind):
    """d = 256: gram_h.hip + the projection without f32 rows; 512: gram_h.hip's off-diagonal blocks + the split projection through the
    scratch buffer; 64: outside gram_h.hip's shapes, the rows are widened for the f32 statistics.  The bar of test_gpu_gather_f16.py:
    2 delta + 1e-4 on sampled pairwise cosines, delta = what rounding the rows moves in the f64 model."""
    rowptr, col, vl, vs = random_csr(n, 9, seed=n + d, empty_frac=0.02, hubs=[(13, 1400)])
    val = vs if kind else vl
    x0 = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    rows = np.random.default_rng(1).choice(n, 400, replace=False)
    cos = lambda e: (lambda u: u @ u.T)(e[rows].astype(np.float64) / np.linalg.norm(e[rows].astype(np.float64), axis=1, keepdims=True))
    exact = cos(loop_model(rowptr, col, val, x0, iters, 0.0, False))
    delta = np.abs(cos(model_fit_on_rounded(rowptr, col, val, x0, iters)) - exact).max()
    g = _hip.Graph.from_host(rowptr, col, vl, vs)
    outs = [np.empty((n, d), np.float32) for _ in range(2)]
    for out, flags in zip(outs, (F, F & ~_hip.F_STATS_F16)):
        _hip.check(_hip.lib().cleora_embed(g.handle, None, _hip.ptr(x0), kind, d, iters, 0, 0.0, 0.0, flags, _hip.ptr(out), None))
        assert np.isfinite(out).all()
    dev = [np.abs(cos(o) - exact).max() for o in outs]
    print(f"n={n} d={d} iters={iters}: delta(models)={delta:.3g}  gpu f16-only rows={dev[0]:.3g}  gpu f16 gather={dev[1]:.3g}")
    assert not np.array_equal(outs[0], outs[1])
    assert dev[0] <= 2 * delta + 1e-4


@gpu
@pytest.mark.parametrize("case", ["no_gather", "residual", "threshold", "d6", "sharded", "colsharded", "multi", "stats_d128", "stats_n100", "stats_ldy"])
def test_refusals(case):
    n, L = 64, _hip.lib()
    rowptr, col, vl, _ = random_csr(n, 4, seed=1)
    g = _hip.Graph.from_host(rowptr, col, vl)
    d = 6 if case == "d6" else 8
    x0, dx = np.zeros((n, d), np.float32), _hip.DevArray((n, d), np.float32)
    if case in ("no_gather", "residual", "threshold", "d6"):
        flags = _hip.F_WHITEN | _hip.F_STATS_F16 if case == "no_gather" else F
        rc = L.cleora_embed(g.handle, None, _hip.ptr(x0), _hip.LEFT, d, 2, 0, 0.3 if case == "residual" else 0.0,
                            1e-3 if case == "threshold" else 0.0, flags, _hip.ptr(x0), None)
    elif case == "sharded":
        rc = L.cleora_embed_sharded(sharded.DeviceShardedGraph(n, rowptr, col, vl).handle, dx.ptr, _hip.LEFT, d, 2, 0.0, 0.0, F, None)
    elif case == "colsharded":
        rc = L.cleora_embed_colsharded(sharded.DeviceColShardedGraph(n, rowptr, col, vl, None, d, None, 1).handle, dx.ptr, _hip.LEFT, 2, 0.0, 0.0, F, None)
    elif case == "multi":
        rc = L.cleora_multi_embed(_hip.MultiGraph.from_host([0, 0], rowptr, col, vl).handle, None, _hip.ptr(x0), _hip.LEFT, d, 2, 0, 0.0, 0.0, F, _hip.ptr(x0), None)
    else:
        ns, ds, ld = {"stats_d128": (4096, 128, 128), "stats_n100": (100, 256, 256), "stats_ldy": (4096, 256, 260)}[case]
        y, ws = _hip.DevArray((ns, ld), np.float16), _hip.DevArray((L.cleora_whiten_workspace(ns, ds),), np.uint8)
        dm, dg = _hip.DevArray((ds,), np.float64), _hip.DevArray((ds, ds), np.float64)
        rc = L.cleora_whiten_stats_h_dev(y.ptr, ld, ns, ds, ws.ptr, dm.ptr, dg.ptr, None)
    assert rc == _hip.E_INVALID and _hip.last_error()


def test_install_stats_dtype_surface():
    try:
        cleora_amd.install(stats_dtype="f16")
        assert _pyc.stats_f16()
        cleora_amd.install(stats_dtype="f32")
        assert not _pyc.stats_f16()
        for bad in ({"stats_dtype": "bf16"}, {"devices": [0, 1], "stats_dtype": "f16"}):
            with pytest.raises(ValueError):
                cleora_amd.install(**bad)
    finally:
        cleora_amd.install(stats_dtype="f32")
