"""The row kernels' leftover edges (csrc/spmm_rows.h: the cnt % U gathers behind the full batches, issued together where the source
policy has BATCH_TAIL, one by one elsewhere): every remainder of U = 8 and U = 16, behind zero, one and two 64-edge chunks, at every
shape of the dispatch, bit for bit against the oracle (f32) and against the models the f16-stored kernels are held to in
tests/test_gpu_iterate_f16.py and tests/test_gpu_gather_f16.py.  Every launch runs twice: the two results must be equal."""
import functools

import numpy as np
import pytest

import oracle
from cleora_amd import _hip
from tests.test_gpu_gather_f16 import model as model_hf, run_hf
from tests.test_gpu_iterate_f16 import model as model_h, run_h

pytestmark = pytest.mark.gpu
L2 = _hip.F_L2NORM
N = 300
U_MAX = 16


@functools.lru_cache(maxsize=None)
def tails_graph():
    """Row r has exactly r edges for r = 0 .. 2 * 16 + 1, then one 70-edge and one 135-edge row (a tail behind one and two 64-edge
    chunks); the rows after them repeat short lengths so that sub-wave groups sit beside ragged neighbours.  Random columns, normal
    weights."""
    deg = np.zeros(N, np.int64)
    deg[:2 * U_MAX + 2] = np.arange(2 * U_MAX + 2)
    deg[2 * U_MAX + 2], deg[2 * U_MAX + 3] = 70, 135
    rest = np.arange(2 * U_MAX + 4, N)
    deg[rest] = (rest * 7) % (2 * U_MAX + 2)
    rowptr = np.zeros(N + 1, np.uint64)
    rowptr[1:] = np.cumsum(deg).astype(np.uint64)
    rng = np.random.default_rng(41)
    nnz = int(rowptr[-1])
    col = rng.integers(0, N, nnz).astype(np.uint32)
    val = rng.standard_normal(nnz).astype(np.float32)
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return rowptr, col, val


@functools.lru_cache(maxsize=None)
def x_f32():
    x = np.random.default_rng(42).standard_normal((N, 1024)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def want_f32(d):
    rowptr, col, val = tails_graph()
    y = oracle.spmm(rowptr, col, val, np.ascontiguousarray(x_f32()[:, :d]))
    yn = oracle.l2_normalize(y)
    for a in (y, yn):
        a.setflags(write=False)
    return y, yn


def propagate(g, x, flags=0):
    L = _hip.lib()
    n_rows, d = g.info().n_rows, x.shape[1]
    dx, dy = _hip.DevArray.from_host(x), _hip.DevArray((n_rows, d), np.float32)
    L.cleora_memset(dy.ptr, 0xFF, dy.nbytes, None)       # poison: every row must be written
    _hip.check(L.cleora_propagate_dev(g.handle, _hip.LEFT, dx.ptr, d, d, dy.ptr, d, flags, 0.0, None, None, None, None))
    _hip.check(L.cleora_stream_sync(None))
    return dy.to_host()


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits16(a):
    return np.ascontiguousarray(a).view(np.uint16)


def twice(run):
    got, again = run(), run()
    np.testing.assert_array_equal(bits32(got) if got.dtype == np.float32 else bits16(got),
                                  bits32(again) if again.dtype == np.float32 else bits16(again))
    return got


# G = 64 with V = 1, 2, 4; sub-wave groups; partial last chunks (FULL = false); 20 = five 16-byte chunks on 8 lanes
WIDTHS = [256, 512, 1024, 128, 64, 32, 8, 100, 252, 20]


@pytest.mark.parametrize("flags", [0, L2])
@pytest.mark.parametrize("d", WIDTHS)
def test_f32_every_remainder_bit_equal(d, flags):
    rowptr, col, val = tails_graph()
    g = _hip.Graph.from_host(rowptr, col, val)
    x = np.ascontiguousarray(x_f32()[:, :d])
    got = twice(lambda: propagate(g, x, flags))
    np.testing.assert_array_equal(bits32(got), bits32(want_f32(d)[1 if flags else 0]))


@pytest.mark.parametrize("flags", [0, L2])
@pytest.mark.parametrize("d", [256, 64])
def test_f32_hot_marks_forced(d, flags):
    """cleora_graph_set_hot_cache with a budget of 100 rows: some gathered rows carry the hot mark, the others are loaded cold."""
    rowptr, col, val = tails_graph()
    g = _hip.Graph.from_host(rowptr, col, val)
    g.set_hot_cache(d * 4 * 100)
    x = np.ascontiguousarray(x_f32()[:, :d])
    got = twice(lambda: propagate(g, x, flags))
    assert 0 < g.info().hot_rows < N
    np.testing.assert_array_equal(bits32(got), bits32(want_f32(d)[1 if flags else 0]))


@functools.lru_cache(maxsize=None)
def special_case():
    """The tails graph with the last len % 8 edges of every row (which are also among its last len % 16) pointed at four rows of x
    that hold inf, nan, -0.0 and denormals, so such an element sits in tails of every length 1 .. 15.  Positive weights and only
    +inf: no sum forms inf - inf, whose NaN a CPU and a GPU sign differently; every NaN in the result is the planted one."""
    rowptr, col, val = tails_graph()
    col, val = col.copy(), np.abs(val)
    for r in range(N):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        for k in range(e - (e - b) % 8, e):
            col[k] = k % 4
    x = x_f32().copy()
    x[0, 0::4], x[0, 1::4], x[0, 2::4], x[0, 3::4] = np.inf, np.nan, -0.0, 1e-45
    x[1, 0::4], x[1, 1::4], x[1, 2::4], x[1, 3::4] = 1e-40, -1e-42, np.inf, -0.0
    x[2, 0::3], x[2, 1::3] = -0.0, -1e-39
    x[3, 0::5], x[3, 2::5] = np.nan, 0.0
    return rowptr, col, val, x


@pytest.mark.parametrize("d", [256, 64])
def test_f32_special_values_in_every_tail(d):
    rowptr, col, val, x = special_case()
    x = np.ascontiguousarray(x[:, :d])
    g = _hip.Graph.from_host(rowptr, col, val)
    got = twice(lambda: propagate(g, x))
    want = oracle.spmm(rowptr, col, val, x)
    assert np.isnan(want).any() and np.isinf(want).any()
    np.testing.assert_array_equal(bits32(got), bits32(want))


def test_f16_gather_special_values_in_every_tail():
    rowptr, col, val, x = special_case()
    x16 = np.ascontiguousarray(x[:, :256]).astype(np.float16)           # 1e-40 .. 1e-45 round to signed zeros; f16 denormals instead
    x16[1, 0::4], x16[2, 1::3] = np.float16(6e-8), np.float16(-3e-6)
    g = _hip.Graph.from_host(rowptr, col, val)
    got = twice(lambda: run_hf(g, _hip.LEFT, x16))
    np.testing.assert_array_equal(bits32(got), bits32(model_hf(rowptr, col, val, x16, 0)))


@functools.lru_cache(maxsize=None)
def x_f16():
    x = np.random.default_rng(43).standard_normal((N, 512)).astype(np.float16)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("flags,hot", [(0, False), (L2, False), (L2, True)])
@pytest.mark.parametrize("d", [256, 512, 64])
def test_f16_stored_rows_every_remainder_bit_equal(d, flags, hot):
    """propagate_h (f16 out) and propagate_hf (f32 out): the comparisons of test_ordinary_rows_bit_equal in their own test files."""
    rowptr, col, val = tails_graph()
    x16 = np.ascontiguousarray(x_f16()[:, :d])
    g = _hip.Graph.from_host(rowptr, col, val)
    if hot:
        g.set_hot_cache(d * 2 * 100)
    got_h = twice(lambda: run_h(g, _hip.LEFT, x16, flags))
    np.testing.assert_array_equal(bits16(got_h), bits16(model_h(rowptr, col, val, x16, flags)))
    got_hf = twice(lambda: run_hf(g, _hip.LEFT, x16, flags))
    np.testing.assert_array_equal(bits32(got_hf), bits32(model_hf(rowptr, col, val, x16, flags)))
