// spmm_rows.h — the row kernel shared by the f32 SpMM (spmm.hip) and the SpMM on f16-stored rows (spmm_h.hip): the schedule of
// work items, the edge loop and the hot / cold gather.  Each .hip file compiles it under its own flags and adds a source policy
// (what a gathered row is, how an element is read from it), its kernels' item decode, its row epilogue and its hub-finish kernel.
//
// Sharing is held to "same registers out of the compiler" (VGPRs, scratch, occupancy of every instantiation against the unshared
// text; scripts/kernel_resources.py shows the flags).  Recheck that after touching this file: the item decode, the hub-finish sum
// and even the f16 kernel's accumulator clearing moved registers when they were shared, and stayed in the .hip files.
//
// Mapping to the hardware:
//   * one GROUP of G lanes owns one output row; G = 64 (a whole wavefront) where a row is at least 1 KiB of f32 or 512 bytes of
//     f16, so one gathered row is ONE coalesced load per lane chunk (lane l reads bytes [B l, B l + B) of the row); narrower d
//     packs 64/G rows per wavefront.
//   * the row's (col, val) slice is fetched 64 (G) entries at a time with one coalesced load into registers and broadcast edge
//     by edge with v_readlane (G = 64: the column index lands in an SGPR, so the gather address is scalar-base + lane offset) or
//     ds_bpermute.
//   * U rows (U*V loads per lane, 128 bytes: the policy's number) are in flight before the first use; with 8 waves per SIMD that
//     is >= 256 KiB of gathers in flight per CU.
//   * edges are consumed in stored order with separate f32 multiply and add (-ffp-contract=off + __fmul_rn/__fadd_rn), so every
//     row that is not split is bit-identical to the reference's sequential accumulate (src/embedding.rs:80-82).
//   * work items: first the hub SEGMENTS — rows longer than hub_threshold cut into hub_segment-edge pieces, each on its own lane
//     group, so the longest work starts first — then one item per row.  A segment item writes its f32 partial sum to scratch; a
//     row item runs the epilogue and writes Y.  The files' hub-finish kernels then add a hub row's partials in a fixed order:
//     deterministic and immune to a pathological hub (a chain of 10^8 dependent adds), but not the reference's summation order.
#pragma once
#include "common.h"
#include "row_epilogue.h"

#include <type_traits>

namespace cleora {
namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// B bytes of a row as they lie in memory
template <int B> using raw_t = std::conditional_t<B == 4, uint32_t, std::conditional_t<B == 8, u32x2, u32x4>>;

struct RowSchedule {
    const uint64_t *rowptr;
    const uint32_t *col;
    const float *val;
    uint64_t n_items;      // hub segments + rows
    uint64_t n_segments;
    uint32_t hub_threshold;
    const uint32_t *seg_row;
    const uint64_t *seg_begin;
    uint32_t hub_segment;
    const uint32_t *hub_rows;
    const uint64_t *hub_seg_first;
    float *partial;
    const uint32_t *mid_rows;     // reference-order schedule (spmm.hip): the first n_segments items are these rows (longest first), not segments
};

// The segmented schedule of a graph: every hub segment, then every row.
inline RowSchedule make_schedule(const cleora_graph *g, const float *val) {
    RowSchedule s{};
    s.rowptr = g->rowptr;
    s.col = g->col;
    s.val = val;
    s.n_segments = g->n_hub_segments;
    s.n_items = s.n_segments + g->n_rows;
    s.hub_threshold = g->hub_threshold;
    s.seg_row = g->seg_row;
    s.seg_begin = g->seg_begin;
    s.hub_segment = g->hub_segment;
    s.hub_rows = g->hub_rows;
    s.hub_seg_first = g->hub_seg_first;
    s.partial = g->hub_partial;
    return s;
}

template <int V, int W>
__device__ __forceinline__ void zero(float (&acc)[V][W]) {
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
        for (int q = 0; q < W; ++q) acc[v][q] = 0.f;
}

// ---- hot / cold gather through a buffer descriptor -------------------------------------------
template <int B, int AUX>
__device__ __forceinline__ raw_t<B> buffer_load(__amdgpu_buffer_rsrc_t rs, int off) {
    if constexpr (B == 4) return __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, AUX);
    else if constexpr (B == 8) return __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, AUX);
    else return __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, AUX);
}

// One gathered row of elements T (E = sizeof(T) bytes each; a typed pointer, because byte arithmetic on the row address cost the
// non-hot f16 shapes 2-4 VGPRs), B bytes per lane and chunk, as raw dwords.  HOT: bit 31 of the column index marks a
// frequently referenced row; those are loaded with the default cache policy and every other (cold) row non-temporally (aux 2), so
// the cold stream does not evict the hot set (hot.hip: -10 % at C3).  The policy is an immediate of buffer_load, so the row goes
// through a buffer descriptor: built from the (wave-uniform) row pointer when a whole wavefront owns the row — its num_records =
// d * E also does the tail bounds check — or spanning the whole matrix (x_bytes < 4 GiB) for sub-wave groups.
template <int G, int V, int B, bool FULL, bool HOT, class T>
__device__ __forceinline__ void gather_buffer(const T *x, uint64_t ldx, uint64_t x_bytes, uint32_t c, int gl, uint32_t d,
                                              raw_t<B> (&r)[V]) {
    constexpr int E = sizeof(T);
    const uint32_t cc = HOT ? (c & 0x7fffffffu) : c;
    const bool cold = HOT && (c >> 31) == 0;
    if constexpr (G == 64) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)(x + (uint64_t)cc * ldx), 0, (int)(d * (uint32_t)E),
                                                          0x00020000);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int off = (v * 64 + gl) * B;
            if (cold) r[v] = buffer_load<B, 2>(rs, off);
            else r[v] = buffer_load<B, 0>(rs, off);
        }
    } else {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc((void *)x, 0, (int)(uint32_t)x_bytes, 0x00020000);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint32_t j = (uint32_t)(v * G + gl) * (B / E);
            const int off = (int)((uint32_t)((uint64_t)cc * ldx + j) * (uint32_t)E);
            raw_t<B> t = {};
            if (FULL || j < d) {
                if (cold) t = buffer_load<B, 2>(rs, off);
                else t = buffer_load<B, 0>(rs, off);
            }
            r[v] = t;
        }
    }
}

// ---- edge loop -------------------------------------------------------------------------------
// acc += sum over edges [beg, end) in stored order.  For G == 64 beg / end are wave-uniform.  Src is the source policy:
//   Src::G, V, W           the shape: G lanes per row, V chunks of W columns per lane
//   Src::U                 rows in flight before the first use
//   Src::BATCH_TAIL        the row's last cnt % U gathers are issued together (below)
//   Src::row_t             a gathered row while it is still in registers
//   Src::gather(a, c, gl, d, r)    gathers row c (bit 31: its hot mark, where the policy has one)
//   Src::elem(r, v, q)             column q of chunk v of a gathered row as f32; the loop forms acc += w * elem with separate
//                                  fmul and fadd
template <class Src, class Args>
__device__ __forceinline__ void accumulate(const Args &a, uint64_t beg, uint64_t end, int gl, int gbase,
                                           float (&acc)[Src::V][Src::W]) {
    constexpr int G = Src::G, U = Src::U;
    const uint32_t d = a.r.d;
    for (uint64_t e = beg; e < end; e += G) {
        const uint32_t cnt = (end - e) < (uint64_t)G ? (uint32_t)(end - e) : (uint32_t)G;
        uint32_t cv = 0;
        float wv = 0.f;
        if ((uint32_t)gl < cnt) {
            cv = a.s.col[e + gl];                     // (loaded non-temporally the edge stream measured no better in the fast placement
            wv = a.s.val[e + gl];                     //  class and 1-2 ms worse in the slow one: scripts/r06/store_policy_probe.py)
        }
        uint32_t k = 0;
        for (; k + U <= cnt; k += U) {
            typename Src::row_t r[U];
#pragma unroll
            for (int u = 0; u < U; ++u) Src::gather(a, bcast_u32<G>(cv, k + u, gbase), gl, d, r[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float w = bcast_f32<G>(wv, k + u, gbase);
#pragma unroll
                for (int v = 0; v < Src::V; ++v)
#pragma unroll
                    for (int q = 0; q < Src::W; ++q) acc[v][q] = fadd(acc[v][q], fmul(w, Src::elem(r[u], v, q)));
            }
        }
        // The m = cnt - k < U edges left over.  BATCH_TAIL: one predicated batch — every gather first, then the multiply-adds in
        // stored order — so a row's tail is one memory round trip, not m.  An absent edge is neither loaded nor added (the zeros only
        // give every r[u] a definition on every path: left undefined, the rows stayed live across the whole edge loop, +24 VGPRs).
        // m is wave-uniform at G == 64 (scalar branches); for sub-wave groups it is uniform within a group, so a group's broadcasts
        // read its own, live lanes.  Without BATCH_TAIL (shapes where the batch cost occupancy) the edges go one by one.
        if constexpr (Src::BATCH_TAIL && U > 1) {
            if (k < cnt) {
                const uint32_t m = cnt - k;
                typename Src::row_t r[U - 1] = {};
#pragma unroll
                for (int u = 0; u < U - 1; ++u)
                    if ((uint32_t)u < m) Src::gather(a, bcast_u32<G>(cv, k + u, gbase), gl, d, r[u]);
#pragma unroll
                for (int u = 0; u < U - 1; ++u)
                    if ((uint32_t)u < m) {
                        const float w = bcast_f32<G>(wv, k + u, gbase);
#pragma unroll
                        for (int v = 0; v < Src::V; ++v)
#pragma unroll
                            for (int q = 0; q < Src::W; ++q) acc[v][q] = fadd(acc[v][q], fmul(w, Src::elem(r[u], v, q)));
                    }
            }
        } else {
            for (; k < cnt; ++k) {
                typename Src::row_t r;
                const uint32_t c = bcast_u32<G>(cv, k, gbase);
                const float w = bcast_f32<G>(wv, k, gbase);
                Src::gather(a, c, gl, d, r);
#pragma unroll
                for (int v = 0; v < Src::V; ++v)
#pragma unroll
                    for (int q = 0; q < Src::W; ++q) acc[v][q] = fadd(acc[v][q], fmul(w, Src::elem(r, v, q)));
            }
        }
    }
}

}  // namespace
}  // namespace cleora
