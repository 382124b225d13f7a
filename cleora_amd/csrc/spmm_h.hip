// spmm_h.hip — the SpMM of spmm.hip on f16-STORED iterates, for gfx950.
//
// Inside the plain loop every iterate after the first has unit rows, so every element lies in [-1, 1], where IEEE binary16 carries
// 11 significant bits.  95 % of the SpMM's bytes are the gathered rows of the iterate: stored as f16 they are half as many.  X,
// x_self and Y are f16 here; everything between the load and the store is f32.  Opt-in, and NOT the reference's bits.
//
// Arithmetic contract (what tests/test_gpu_iterate_f16.py holds the kernel to, bit for bit):
//   * a gathered f16 element is widened exactly to f32 (v_cvt_f32_f16; the kernel runs with f16 denormals on);
//   * the row sum is acc = fadd(acc, fmul(w, x)) in stored edge order — separate multiply and add like spmm.hip (-ffp-contract=off,
//     no v_fma_mix);
//   * the epilogue of row_epilogue.h runs on the f32 accumulators (residual blend, exact-order or FASTNORM L2, L1);
//   * every element is then rounded ONCE, to nearest even, to f16 (v_cvt_f16_f32, subnormals kept);
//   * SQDIFF / SQDIFF64 are taken AFTER that rounding, between the widened stored value and the widened x_self: the RMSE of the
//     iterates the loop actually holds.
//
// Mapping: the row kernel of spmm_rows.h (schedule of work items, edge loop, hot / cold gather).  What this file adds:
//   * the f16 source policy: a lane loads C = 4 halfs (8 bytes) per chunk, or C = 8 (16 bytes) where the row is >= 1 KiB and
//     everything is 16-byte aligned; at G = 64 the row always goes through the per-row buffer descriptor (num_records = d * 2 does the
//     tail check), with the hot marks sized by row bytes (hot.hip);
//   * 128 bytes of gathers per lane are in flight before the first use, 8 KiB per wavefront like the f32 kernel: U * V = 16 load
//     instructions at C = 4 (16 edges of a d = 256 row), 8 at C = 8;
//   * narrower d packs 64 / G rows per wavefront (G = 8, 16, 32 lanes per row, 8 bytes per lane);
//   * rows longer than hub_threshold ALWAYS take the segmented schedule (what CLEORA_F_HUB_SEGMENTS selects in spmm.hip), finished by
//     hub_finish_h_kernel with the f16 epilogue.  In-order f16 hub kernels are a follow-up.
//
// F32OUT variant (cleora_propagate_hf_dev; CLEORA_F_GATHER_F16 in the whitened loop): the same gather on an f16 X, but Y is f32 and
// nothing is rounded on the way out — the loop's Z = A Y, whose input rows are normalised (|Y| <= 1) and whose output the projection
// consumes in f32.  Same contract up to the epilogue (L2 / L1 / FASTNORM; no x_self flags); tests/test_gpu_gather_f16.py.
#include "common.h"
#include "row_epilogue.h"
#include "spmm_rows.h"

#include <type_traits>

namespace cleora {
namespace {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
template <int C> using halfs_t = raw_t<2 * C>;     // C halfs as they lie in memory

struct SpmmHArgs {
    RowSchedule s;
    const uint16_t *x;
    uint64_t ldx;
    uint64_t x_bytes;      // span of x (whole-matrix buffer descriptor of the sub-wave hot path)
    uint16_t *y;
    uint64_t ldy;
    const uint16_t *x_self;
    uint64_t ldxs;
    RowArgs r;             // flags, rw / alpha, d, row_sqdiff (its f32 pointers are not used)
    float *y32;            // the f32 output of the F32OUT kernels (y is not used there); ldy counts its elements
};

__device__ __forceinline__ float widen_lo(uint32_t t) { return (float)__builtin_bit_cast(f16x2, t).x; }
__device__ __forceinline__ float widen_hi(uint32_t t) { return (float)__builtin_bit_cast(f16x2, t).y; }
// two f32 -> two f16, each rounded to nearest even (never the round-toward-zero pack instruction)
__device__ __forceinline__ uint32_t round_pair(float lo, float hi) {
    const f16x2 p = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(uint32_t, p);
}

// The f16 source of the edge loop: a gathered row stays packed, V chunks of C halfs, until it is added.
template <int kG, int kV, int C, bool HOT>
struct RowsF16 {
    static constexpr int G = kG, V = kV, W = C;
    static constexpr int LOADS = C == 4 ? 16 : 8;                     // 128 bytes per lane in flight
    static constexpr int U = (LOADS / V) > 0 ? (LOADS / V) : 1;
    // every shape whose occupancy the batched tail leaves alone (scripts/kernel_resources.py): not 16 lanes per row with hot marks
    // (7 -> 6 waves per SIMD)
    static constexpr bool BATCH_TAIL = !(G == 16 && HOT);
    using row_t = halfs_t<C>[V];
    static_assert(G == 64 || C == 4, "sub-wave groups load 8 bytes per lane");

    static __device__ __forceinline__ void gather(const SpmmHArgs &a, uint32_t c, int gl, uint32_t d, row_t &r) {
        if constexpr (G == 64 || HOT) {
            gather_buffer<G, V, 2 * C, false, HOT>(a.x, a.ldx, a.x_bytes, c, gl, d, r);
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const uint32_t j = (uint32_t)(v * G + gl) * C;
                halfs_t<C> t = {};
                if (j < d) t = *reinterpret_cast<const halfs_t<C> *>(a.x + (uint64_t)c * a.ldx + j);
                r[v] = t;
            }
        }
    }
    // column q of chunk v, widened exactly
    static __device__ __forceinline__ float elem(const row_t &r, int v, int q) { return (q & 1) ? widen_hi(r[v][q / 2]) : widen_lo(r[v][q / 2]); }
};

// The row epilogue on f16 storage: x_self widened, the f32 arithmetic of row_epilogue.h, one rounding, SQDIFF on what is stored.
template <int G, int V, int C>
__device__ __forceinline__ void finish_row_h(const SpmmHArgs &a, uint64_t row, int gl, int gbase, float (&acc)[V][C]) {
    const RowArgs &ra = a.r;
    const uint32_t d = ra.d;
    float xs[V][C];
    if (ra.flags & (CLEORA_F_RESIDUAL | CLEORA_F_SQDIFF)) {
        const uint16_t *p = a.x_self + row * a.ldxs;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint32_t j = (uint32_t)(v * G + gl) * C;
            halfs_t<C> t = {};
            if (j < d) t = *reinterpret_cast<const halfs_t<C> *>(p + j);
#pragma unroll
            for (int i = 0; i < C / 2; ++i) {
                xs[v][2 * i] = widen_lo(t[i]);
                xs[v][2 * i + 1] = widen_hi(t[i]);
            }
        }
    }
    blend_and_normalize<G, V, C>(ra, row, gl, gbase, acc, xs);

    halfs_t<C> out[V];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int i = 0; i < C / 2; ++i) out[v][i] = round_pair(acc[v][2 * i], acc[v][2 * i + 1]);

    if (ra.flags & CLEORA_F_SQDIFF) {
        double ds = 0.0;
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int q = 0; q < C; ++q) {
                const uint32_t j = (uint32_t)(v * G + gl) * C + q;
                if (j < d) {
                    const float stored = (q & 1) ? widen_hi(out[v][q / 2]) : widen_lo(out[v][q / 2]);
                    const double delta = (ra.flags & CLEORA_F_SQDIFF64) ? (double)stored - (double)xs[v][q]
                                                                        : (double)fsub(stored, xs[v][q]);
                    ds += delta * delta;
                }
            }
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
        if (gl == 0) ra.row_sqdiff[row] = ds;
    }

    uint16_t *yr = a.y + row * a.ldy;
    const bool nt = (ra.flags & kStreamStores) != 0;                  // streaming store: see kStreamStores
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const uint32_t j = (uint32_t)(v * G + gl) * C;
        if (j < d) {
            if (nt) __builtin_nontemporal_store(out[v], reinterpret_cast<halfs_t<C> *>(yr + j));
            else *reinterpret_cast<halfs_t<C> *>(yr + j) = out[v];
        }
    }
}

// The row epilogue of the f16-gather / f32-output kernels (the whitened loop's Z = A Y, consumed in f32 by the projection): the f32
// arithmetic of row_epilogue.h on the sums and NO rounding — the accumulators leave as they are.  A lane's C consecutive columns are
// C / 4 16-byte stores: at C = 4 a store instruction writes 1 KiB of the row contiguously; at C = 8 (rows >= 1 KiB) the lane's two
// stores are 16 bytes apart and the lanes 32 bytes, so each instruction writes every other 16-byte piece of 2 KiB and the pair
// completes the lines (back to back from one wave).  No x_self: RESIDUAL / SQDIFF are refused by the launcher.
template <int G, int V, int C>
__device__ __forceinline__ void finish_row_hf(const SpmmHArgs &a, uint64_t row, int gl, int gbase, float (&acc)[V][C]) {
    const RowArgs &ra = a.r;
    const uint32_t d = ra.d;
    float xs[V][C];                                                   // never read: RESIDUAL is not set
    blend_and_normalize<G, V, C>(ra, row, gl, gbase, acc, xs);
    typedef float nt_f4 __attribute__((ext_vector_type(4)));
    float *yr = a.y32 + row * a.ldy;
    const bool nt = (ra.flags & kStreamStores) != 0;                  // streaming store: see kStreamStores
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const uint32_t j = (uint32_t)(v * G + gl) * C;
        if (j < d) {                                                  // (C = 8 only where d % 8 == 0: whole chunks)
#pragma unroll
            for (int q = 0; q < C; q += 4) {
                const nt_f4 o = {acc[v][q], acc[v][q + 1], acc[v][q + 2], acc[v][q + 3]};
                if (nt) __builtin_nontemporal_store(o, reinterpret_cast<nt_f4 *>(yr + j + q));
                else *reinterpret_cast<nt_f4 *>(yr + j + q) = o;
            }
        }
    }
}

// ---- main kernel ---------------------------------------------------------------------------
// A row item writes Y as f16, or as f32 with F32OUT.
template <int G, int V, int C, bool HOT, bool F32OUT = false>
__global__ __launch_bounds__(256) void spmm_rows_h_kernel(const SpmmHArgs a) {
    const int lane = threadIdx.x & 63;
    const int gl = lane & (G - 1);
    const int gbase = lane & ~(G - 1);
    uint64_t item = CLEORA_LINEAR_BLOCK() * (256 / G) + (threadIdx.x / G);
    bool active = item < a.s.n_items;
    if constexpr (G == 64) {
        if (!active) return;
        item = uniform_u64(item);
    }
    const bool is_seg = item < a.s.n_segments;
    uint64_t row = 0, beg = 0, end = 0;
    if (active) {
        if (is_seg) {
            row = a.s.seg_row[item];
            beg = a.s.seg_begin[item];
            const uint64_t rend = a.s.rowptr[row + 1];
            end = beg + a.s.hub_segment < rend ? beg + a.s.hub_segment : rend;
        } else {
            row = item - a.s.n_segments;
            beg = a.s.rowptr[row];
            end = a.s.rowptr[row + 1];
            if (end - beg > a.s.hub_threshold) active = false;
        }
    }
    if constexpr (G == 64) {
        if (!active) return;
        row = uniform_u64(row);
        beg = uniform_u64(beg);
        end = uniform_u64(end);
    } else if (!active) {
        beg = end = 0;
    }
    float acc[V][C];
#pragma unroll
    for (int v = 0; v < V; ++v)                                       // (not zero(acc): with it the d = 1024 shapes took 116 VGPRs for 71)
#pragma unroll
        for (int q = 0; q < C; ++q) acc[v][q] = 0.f;
    accumulate<RowsF16<G, V, C, HOT>>(a, beg, end, gl, gbase, acc);
    if (!active) return;
    if (is_seg) {
        float *p = a.s.partial + item * (uint64_t)a.r.d;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint32_t j = (uint32_t)(v * G + gl) * C;
            if (j < a.r.d) {
#pragma unroll
                for (int q = 0; q < C; q += 4)
                    *reinterpret_cast<float4 *>(p + j + q) = make_float4(acc[v][q], acc[v][q + 1], acc[v][q + 2], acc[v][q + 3]);
            }
        }
    } else if constexpr (F32OUT) {
        finish_row_hf<G, V, C>(a, row, gl, gbase, acc);
    } else {
        finish_row_h<G, V, C>(a, row, gl, gbase, acc);
    }
}

// ---- hub rows: in-order combine of the segment partials + epilogue -----------------------------
// hub_finish_kernel of spmm.hip with the f16 epilogue: one 256-thread block per hub row, four wavefronts each adding a contiguous
// run of the row's segments in order (8 loads in flight), the four sums added in wave order through LDS.  Fixed order => deterministic.
template <int V, bool F32OUT = false>
__global__ __launch_bounds__(256) void hub_finish_h_kernel(const SpmmHArgs a) {
    __shared__ float sm[4][64 * V * 4];
    const int gl = threadIdx.x & 63;
    const int grp = threadIdx.x >> 6;
    const uint64_t h = blockIdx.x;
    const uint64_t row = a.s.hub_rows[h];
    const uint64_t s0 = a.s.hub_seg_first[h], s1 = a.s.hub_seg_first[h + 1];
    const uint64_t per = (s1 - s0 + 3) / 4;
    const uint64_t b = s0 + grp * per < s1 ? s0 + grp * per : s1;
    const uint64_t e = b + per < s1 ? b + per : s1;
    const uint32_t d = a.r.d;
    float acc[V][4];
    zero(acc);
    constexpr int U = 8 / V;
    uint64_t s = b;
    for (; s + U <= e; s += U) {
        float p[U][V][4];
#pragma unroll
        for (int u = 0; u < U; ++u) load_row<64, V, 4, false>(a.s.partial + (s + u) * (uint64_t)d, gl, d, p[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int v = 0; v < V; ++v)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[v][q] = fadd(acc[v][q], p[u][v][q]);
    }
    if constexpr (U > 1) {
        if (s < e) {                                   // the last e - s < U partials: loaded together (spmm_rows.h, BATCH_TAIL), added in order
            const uint32_t m = (uint32_t)(e - s);
            float p[U - 1][V][4] = {};
#pragma unroll
            for (int u = 0; u < U - 1; ++u)
                if ((uint32_t)u < m) load_row<64, V, 4, false>(a.s.partial + (s + u) * (uint64_t)d, gl, d, p[u]);
#pragma unroll
            for (int u = 0; u < U - 1; ++u)
                if ((uint32_t)u < m) {
#pragma unroll
                    for (int v = 0; v < V; ++v)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[v][q] = fadd(acc[v][q], p[u][v][q]);
                }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int q = 0; q < 4; ++q) sm[grp][(v * 64 + gl) * 4 + q] = acc[v][q];
    __syncthreads();
    if (grp != 0) return;
    for (int g2 = 1; g2 < 4; ++g2)
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[v][q] = fadd(acc[v][q], sm[g2][(v * 64 + gl) * 4 + q]);
    if constexpr (F32OUT) finish_row_hf<64, V, 4>(a, row, gl, 0, acc);
    else finish_row_h<64, V, 4>(a, row, gl, 0, acc);
}

// ---- shape dispatch -----------------------------------------------------------------------------
template <int N> using I = std::integral_constant<int, N>;
constexpr uint32_t kMaxDH = 2048;     // widest register-resident row: 64 lanes x 4 chunks x 8 halfs (or 8 x 4)

// Calls f(G, V, C) with the compile-time shape for a row of d halfs (d % 4 == 0, d <= kMaxDH).  wide: 16-byte chunks are allowed
// (d % 8 == 0 and everything 16-byte aligned); they are taken where a row is >= 1 KiB.
template <class F>
void dispatch_shape_h(uint32_t d, bool wide, F &&f) {
    const uint32_t chunks = d / 4;
    if (chunks <= 8) f(I<8>{}, I<1>{}, I<4>{});
    else if (chunks <= 16) f(I<16>{}, I<1>{}, I<4>{});
    else if (chunks <= 32) f(I<32>{}, I<1>{}, I<4>{});
    else if (chunks <= 64) f(I<64>{}, I<1>{}, I<4>{});
    else if (wide && d >= 512) {
        if (chunks <= 128) f(I<64>{}, I<1>{}, I<8>{});
        else if (chunks <= 256) f(I<64>{}, I<2>{}, I<8>{});
        else f(I<64>{}, I<4>{}, I<8>{});
    } else if (chunks <= 128) f(I<64>{}, I<2>{}, I<4>{});
    else if (chunks <= 256) f(I<64>{}, I<4>{}, I<4>{});
    else f(I<64>{}, I<8>{}, I<4>{});
}

inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// The launches behind both entry points, arguments checked: y is uint16_t[n_rows][ldy], or float[n_rows][ldy] with F32OUT.
template <bool F32OUT>
static int launch_h(const cleora_graph *g, int kind, const uint16_t *x, uint64_t ldx, uint32_t d, void *y, uint64_t ldy, uint32_t flags,
                    float rw, const uint16_t *x_self, double *row_sqdiff, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(g->mu);
    CL_HIP(hipSetDevice(g->device));
    flags &= ~CLEORA_F_HUB_SEGMENTS;                       // implied: long rows always take the segmented schedule here
    if (g->n_hub_rows) {
        const int rc = ensure_hub_partial(g, d, true, stream);
        if (rc != CLEORA_OK) return rc;
    }

    SpmmHArgs a{};
    a.s = make_schedule(g, g->val[kind]);
    a.x = x;
    a.ldx = ldx;
    a.x_bytes = g->n_cols * ldx * sizeof(uint16_t);
    if constexpr (F32OUT) a.y32 = static_cast<float *>(y);
    else a.y = static_cast<uint16_t *>(y);
    a.ldy = ldy;
    a.x_self = x_self;
    a.ldxs = ldx;
    a.r.row_sqdiff = row_sqdiff;
    a.r.rw = rw;
    a.r.alpha = 1.0f - rw;
    const uint64_t y_bytes = g->n_rows * ldy * (F32OUT ? sizeof(float) : sizeof(uint16_t));
    a.r.flags = flags | (y_bytes >= kStreamStoreMinBytes ? kStreamStores : 0u);
    a.r.d = d;

    // 16-byte gathers: the f16 operands 16-byte aligned (an f32 y always is: its launcher requires it)
    const bool wide = d % 8 == 0 && ldx % 8 == 0 && aligned_to(x, 16) && (F32OUT || (ldy % 8 == 0 && aligned_to(y, 16))) &&
                      (!x_self || aligned_to(x_self, 16));
    dispatch_shape_h(d, wide, [&](auto G, auto V, auto C) {
        constexpr int kG = decltype(G)::value, kV = decltype(V)::value, kC = decltype(C)::value;
        const dim3 grid = grid_1d_as_2d((a.s.n_items + 256 / kG - 1) / (256 / kG));
        // hot-column cache policy, sized by row BYTES: needs the marked column copy and, for sub-wave groups, a matrix that one
        // buffer descriptor can span
        const uint32_t *hot = (kG == 64 || a.x_bytes < (1ull << 32)) ? ensure_hot_cols(g, d, ldx, stream, sizeof(uint16_t)) : nullptr;
        if (hot) {
            SpmmHArgs h = a;
            h.s.col = hot;
            hipLaunchKernelGGL((spmm_rows_h_kernel<kG, kV, kC, true, F32OUT>), grid, dim3(256), 0, stream, h);
        } else {
            hipLaunchKernelGGL((spmm_rows_h_kernel<kG, kV, kC, false, F32OUT>), grid, dim3(256), 0, stream, a);
        }
    });
    if (g->n_hub_rows) {
        const dim3 grid((unsigned)g->n_hub_rows);
        if (d <= 256) hipLaunchKernelGGL((hub_finish_h_kernel<1, F32OUT>), grid, dim3(256), 0, stream, a);
        else if (d <= 512) hipLaunchKernelGGL((hub_finish_h_kernel<2, F32OUT>), grid, dim3(256), 0, stream, a);
        else if (d <= 1024) hipLaunchKernelGGL((hub_finish_h_kernel<4, F32OUT>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((hub_finish_h_kernel<8, F32OUT>), grid, dim3(256), 0, stream, a);
    }
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

// What both entry points require of the graph, the f16 x and the shape.
static int check_h(const cleora_graph *g, int kind, const uint16_t *x, uint64_t ldx, uint32_t d, const void *y, uint64_t ldy, const char *d_msg,
                   const char *ld_msg) {
    CL_REQUIRE(g != nullptr, "graph handle is NULL");
    CL_REQUIRE(kind == CLEORA_LEFT || kind == CLEORA_SYMMETRIC, "unknown markov_type");
    CL_REQUIRE(g->val[kind] != nullptr, "graph has no values for this markov_type");
    CL_REQUIRE(d > 0 && ldx >= d && ldy >= d, "bad d / leading dimension");
    CL_REQUIRE(x != nullptr && y != nullptr, "x / y is NULL");
    CL_REQUIRE((const void *)x != y, "x and y must not alias");
    CL_REQUIRE(d % 4 == 0 && d <= kMaxDH, d_msg);
    CL_REQUIRE(ldx % 4 == 0 && ldy % 4 == 0, ld_msg);
    return CLEORA_OK;
}

int launch_propagate_h(const cleora_graph *g, int kind, const uint16_t *x, uint64_t ldx, uint32_t d, uint16_t *y, uint64_t ldy,
                       uint32_t flags, float rw, const uint16_t *x_self, double *row_sqdiff, hipStream_t stream) {
    if (int rc = check_h(g, kind, x, ldx, d, y, ldy, "f16 rows: d must be a multiple of 4, at most 2048",
                         "f16 rows: leading dimensions must be multiples of 4"))
        return rc;
    CL_REQUIRE(!(flags & (CLEORA_F_ROWSQ | CLEORA_F_SCALE | CLEORA_F_ROWSQ_CONT)), "f16 rows: ROWSQ / SCALE / ROWSQ_CONT are not served");
    CL_REQUIRE(!((flags & CLEORA_F_L1NORM) && (flags & CLEORA_F_L2NORM)), "L1NORM is exclusive with L2NORM");
    if ((flags & CLEORA_F_RESIDUAL) && !(rw > 0.0f && (rw < 1.0f || (flags & CLEORA_F_BLEND_ANY)))) flags &= ~CLEORA_F_RESIDUAL;
    if (flags & (CLEORA_F_RESIDUAL | CLEORA_F_SQDIFF)) {
        if (!x_self && g->n_rows == g->n_cols) x_self = x;
        CL_REQUIRE(x_self != nullptr, "x_self is required for RESIDUAL / SQDIFF on a row shard");
    }
    CL_REQUIRE(aligned_to(x, 8) && aligned_to(y, 8) && (!x_self || aligned_to(x_self, 8)), "f16 rows: x / y / x_self must be 8-byte aligned");
    if (flags & CLEORA_F_SQDIFF) CL_REQUIRE(row_sqdiff != nullptr, "row_sqdiff is NULL");
    if (g->n_rows == 0) return CLEORA_OK;
    return launch_h<false>(g, kind, x, ldx, d, y, ldy, flags, rw, x_self, row_sqdiff, stream);
}

// y (f32) = epilogue(A widen(x)): the gather of launch_propagate_h, nothing rounded on the way out.  flags: L2NORM / L1NORM / FASTNORM.
int launch_propagate_hf(const cleora_graph *g, int kind, const uint16_t *x, uint64_t ldx, uint32_t d, float *y, uint64_t ldy,
                        uint32_t flags, hipStream_t stream) {
    if (int rc = check_h(g, kind, x, ldx, d, y, ldy, "f16 gather: d must be a multiple of 4, at most 2048",
                         "f16 gather: leading dimensions must be multiples of 4"))
        return rc;
    CL_REQUIRE(!(flags & (CLEORA_F_RESIDUAL | CLEORA_F_SQDIFF | CLEORA_F_ROWSQ | CLEORA_F_SCALE | CLEORA_F_ROWSQ_CONT)),
               "f16 gather into f32 rows: RESIDUAL / SQDIFF / ROWSQ / SCALE / ROWSQ_CONT are not served");
    CL_REQUIRE(!((flags & CLEORA_F_L1NORM) && (flags & CLEORA_F_L2NORM)), "L1NORM is exclusive with L2NORM");
    CL_REQUIRE(aligned_to(x, 8) && aligned_to(y, 16), "f16 gather: x must be 8-byte, y 16-byte aligned");
    if (g->n_rows == 0) return CLEORA_OK;
    return launch_h<true>(g, kind, x, ldx, d, y, ldy, flags, 0.0f, nullptr, nullptr, stream);
}

}  // namespace cleora
