// The selection that knn.hip's and ivf.hip's scan kernels share: the compaction of a query's survivor buffer (one wave) and the merge
// of a query's partial lists (one wave per query).  Order everywhere: score descending, ties -> the larger row index.  Internal
// linkage: every translation unit that includes this gets its own copy.
#pragma once

#include <cmath>

#include "common.h"

namespace cleora {
namespace {

constexpr int KCAP = 96;                    // entries of a query's survivor buffer
constexpr uint32_t KMAXSPLIT = 64;          // most partial lists of k entries one merge takes (x CLEORA_KNN_MAX_K entries of LDS)
constexpr uint32_t kNoRow = 0xffffffffu;

// One wave: the buffer of query slot q down to its k best, in order.  s / ix: the query's KCAP entries, c of them live, the first
// `tested` of them already through the edge test.  Returns the new count.
__device__ __forceinline__ uint32_t knn_compact(float *s, uint32_t *ix, uint32_t c, uint32_t tested, uint32_t k, uint32_t qr,
                                                const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ col, float *tau_q,
                                                int lane) {
    if (rowptr != nullptr && tested < c) {
        // (q, r) stored: row q once, a lane per column, against every new entry
        const uint64_t qb = rowptr[qr], qe = rowptr[qr + 1];
        for (uint64_t p = qb; p < qe; p += 64) {
            const uint32_t cv = p + lane < qe ? col[p + lane] : kNoRow;
            for (uint32_t e = tested; e < c; ++e)
                if (ix[e] == cv) s[e] = -2.0f;
        }
        // (r, q) stored: row r, per entry
        for (uint32_t e = tested; e < c; ++e) {
            const uint32_t r = ix[e];
            const uint64_t rb = rowptr[r], re = rowptr[r + 1];
            bool found = false;
            for (uint64_t p = rb; p < re && !found; p += 64) found = __any(p + lane < re && col[p + lane] == qr);
            if (found && lane == 0) s[e] = -2.0f;
        }
        __builtin_amdgcn_wave_barrier();
    }
    const bool live0 = (uint32_t)lane < c, live1 = (uint32_t)lane + 64 < c;
    const float s0 = live0 ? s[lane] : 0.f, s1 = live1 ? s[lane + 64] : 0.f;
    const uint32_t i0 = live0 ? ix[lane] : 0u, i1 = live1 ? ix[lane + 64] : 0u;
    uint32_t r0 = 0, r1 = 0;                         // how many entries come before this one: larger score, or equal and larger row
    for (uint32_t e = 0; e < c; ++e) {
        const float se = s[e];
        const uint32_t ie = ix[e];
        r0 += (se > s0 || (se == s0 && ie > i0)) ? 1u : 0u;
        r1 += (se > s1 || (se == s1 && ie > i1)) ? 1u : 0u;
    }
    __builtin_amdgcn_wave_barrier();
    if (live0 && r0 < k) { s[r0] = s0; ix[r0] = i0; }
    if (live1 && r1 < k) { s[r1] = s1; ix[r1] = i1; }
    if (c >= k) {
        if (live0 && r0 == k - 1) *tau_q = s0;
        if (live1 && r1 == k - 1) *tau_q = s1;
    }
    __builtin_amdgcn_wave_barrier();
    return c < k ? c : k;
}

// One wave per query: the k best of its splits x k partial entries, descending, ties -> larger row; -inf entries are padding.  A
// slot that no entry is left for: score -inf, index pad_index.
__global__ __launch_bounds__(64) void knn_merge_kernel(const float *__restrict__ part_score, const uint32_t *__restrict__ part_index,
                                                       uint64_t nq, uint32_t splits, uint32_t k, uint32_t pad_index,
                                                       float *__restrict__ out_score, uint32_t *__restrict__ out_index) {
    __shared__ float ms[KMAXSPLIT * CLEORA_KNN_MAX_K];
    __shared__ uint32_t mi[KMAXSPLIT * CLEORA_KNN_MAX_K];
    const uint64_t qi = CLEORA_LINEAR_BLOCK();
    if (qi >= nq) return;
    const uint32_t lane = threadIdx.x, len = splits * k;
    for (uint32_t e = lane; e < len; e += 64) {
        ms[e] = part_score[qi * len + e];
        mi[e] = part_index[qi * len + e];
    }
    __syncthreads();
    for (uint32_t round = 0; round < k; ++round) {
        float bv = -INFINITY;
        uint32_t bid = 0, bp = kNoRow;
        for (uint32_t e = lane; e < len; e += 64) {
            const float v = ms[e];
            const uint32_t id = mi[e];
            if (v > -INFINITY && (bp == kNoRow || v > bv || (v == bv && id > bid))) { bv = v; bid = id; bp = e; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const uint32_t oid = (uint32_t)__shfl_xor((int)bid, o, 64), op = (uint32_t)__shfl_xor((int)bp, o, 64);
            if (op != kNoRow && (bp == kNoRow || ov > bv || (ov == bv && oid > bid))) { bv = ov; bid = oid; bp = op; }
        }
        if (lane == 0) {
            out_score[qi * k + round] = bv;
            out_index[qi * k + round] = bp != kNoRow ? bid : pad_index;
            if (bp != kNoRow) ms[bp] = -INFINITY;
        }
        __syncthreads();
    }
}

}  // namespace
}  // namespace cleora
