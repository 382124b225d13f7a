// The ordered member lists of a labelling: members[] holds the rows of every cluster in ASCENDING row order, cluster after cluster,
// in an order that depends only on (labels, n, k).  What kmeans.hip's update sums over and what ivf.hip lays its lists out by (and
// regroups its (query, probe) pairs with).  Internal linkage: every translation unit that includes this gets its own kernels.
//     count    the rows are cut into at most 512 segments of consecutive rows; one wave per segment counts its labels in LDS
//              (integer atomics) -> table[segment][cluster];
//     scan     per cluster over the segments (exclusive, in place), then over the clusters: coff[c] = first member slot of
//              cluster c, choff[c] = first CHUNK (of CHUNK members) of cluster c;
//     place    one wave per segment walks its rows 64 at a time in row order; a lane's slot is its cluster's cursor plus the
//              number of lower lanes with the same label.
// Labels >= k belong to no cluster.  k * 4 bytes of LDS per wave: k <= 4096.
#pragma once

#include "common.h"

namespace cleora {
namespace {

constexpr uint64_t USEGS = 512;           // most row segments of count / place
constexpr uint64_t USEG_MIN_ROWS = 1024;  // fewest rows per segment (a multiple of 64)
constexpr uint32_t kNoLabel = 0xffffffffu;

struct MemberSegs {
    uint64_t seg_rows;      // rows per segment
    uint32_t segs;          // segments
    uint64_t segs_bound;    // a bound on segs that is monotone in n (segs itself is not): what the table is sized by
};

inline MemberSegs member_segs(uint64_t n) {
    MemberSegs s;
    s.seg_rows = ((n + USEGS - 1) / USEGS + 63) / 64 * 64;
    if (s.seg_rows < USEG_MIN_ROWS) s.seg_rows = USEG_MIN_ROWS;
    s.segs = (uint32_t)((n + s.seg_rows - 1) / s.seg_rows);
    if (s.segs < 1) s.segs = 1;
    const uint64_t by_rows = (n + USEG_MIN_ROWS - 1) / USEG_MIN_ROWS;
    s.segs_bound = by_rows < 1 ? 1 : (by_rows < USEGS ? by_rows : USEGS);
    return s;
}

// One wave per segment of consecutive rows: table[segment][c] = rows of the segment with label c.
__global__ __launch_bounds__(64) void kmeans_count_kernel(const uint32_t *__restrict__ labels, uint64_t n, uint64_t seg_rows, uint32_t k,
                                                          uint32_t *__restrict__ table) {
    extern __shared__ uint32_t kmeans_cnt[];
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = lane; c < k; c += 64) kmeans_cnt[c] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * seg_rows, end = begin + seg_rows < n ? begin + seg_rows : n;
    for (uint64_t r = begin + lane; r < end; r += 64) {
        const uint32_t l = labels[r];
        if (l < k) atomicAdd(&kmeans_cnt[l], 1u);
    }
    __syncthreads();
    for (uint32_t c = lane; c < k; c += 64) table[(uint64_t)blockIdx.x * k + c] = kmeans_cnt[c];
}

// One thread per cluster: its column of the table becomes the exclusive scan over the segments; count[c] = its total.
__global__ __launch_bounds__(256) void kmeans_segscan_kernel(uint32_t *__restrict__ table, uint32_t segs, uint32_t k, uint32_t *__restrict__ count) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    uint32_t run = 0;
    for (uint32_t b = 0; b < segs; b += 8) {
        uint32_t v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u) v[u] = b + u < segs ? table[(uint64_t)(b + u) * k + c] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < 8; ++u)
            if (b + u < segs) {
                table[(uint64_t)(b + u) * k + c] = run;
                run += v[u];
            }
    }
    count[c] = run;
}

// One block: coff[c] = members before cluster c, choff[c] = chunks of CHUNK members before it; [k] = the totals.
template <uint32_t CHUNK>
__global__ __launch_bounds__(256) void kmeans_offsets_kernel(const uint32_t *__restrict__ count, uint32_t k, uint32_t *__restrict__ coff,
                                                             uint32_t *__restrict__ choff) {
    __shared__ uint32_t sa[256], sb[256];
    const uint32_t t = threadIdx.x, per = (k + 255) / 256;
    const uint32_t c0 = t * per, c1 = c0 + per < k ? c0 + per : k;
    uint32_t ma = 0, mb = 0;
    for (uint32_t c = c0; c < c1; ++c) {
        ma += count[c];
        mb += (count[c] + CHUNK - 1) / CHUNK;
    }
    sa[t] = ma;
    sb[t] = mb;
    __syncthreads();
    for (uint32_t o = 1; o < 256; o <<= 1) {
        const uint32_t va = t >= o ? sa[t - o] : 0u, vb = t >= o ? sb[t - o] : 0u;
        __syncthreads();
        sa[t] += va;
        sb[t] += vb;
        __syncthreads();
    }
    uint32_t ra = sa[t] - ma, rb = sb[t] - mb;
    for (uint32_t c = c0; c < c1; ++c) {
        coff[c] = ra;
        choff[c] = rb;
        ra += count[c];
        rb += (count[c] + CHUNK - 1) / CHUNK;
    }
    if (t == 255) {
        coff[k] = sa[255];
        choff[k] = sb[255];
    }
}

// One wave per segment, 64 rows at a time in row order: members[coff[c] ..] = the rows of cluster c, ascending.
__global__ __launch_bounds__(64) void kmeans_place_kernel(const uint32_t *__restrict__ labels, uint64_t n, uint64_t seg_rows, uint32_t k,
                                                          const uint32_t *__restrict__ table, const uint32_t *__restrict__ coff,
                                                          uint32_t *__restrict__ members) {
    extern __shared__ uint32_t kmeans_cur[];
    const int lane = threadIdx.x;
    for (uint32_t c = lane; c < k; c += 64) kmeans_cur[c] = coff[c] + table[(uint64_t)blockIdx.x * k + c];
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * seg_rows, end = begin + seg_rows < n ? begin + seg_rows : n;
    for (uint64_t base = begin; base < end; base += 64) {
        const uint64_t r = base + lane;
        uint32_t l = r < end ? labels[r] : kNoLabel;
        if (l >= k) l = kNoLabel;
        uint32_t before = 0;
        bool later = false;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const bool same = (uint32_t)__shfl((int)l, j, 64) == l;
            before += (same && j < lane) ? 1u : 0u;
            later = later || (same && j > lane);
        }
        uint32_t pos = 0;
        if (l != kNoLabel) {
            pos = kmeans_cur[l] + before;
            if (pos < n) members[pos] = (uint32_t)r;      // always true while nobody rewrites the labels under this call
        }
        __syncthreads();
        if (l != kNoLabel && !later) kmeans_cur[l] = pos + 1;    // the last lane of a label moves its cursor
        __syncthreads();
    }
}

// table: [segs_bound][k], count: [k], coff / choff: [k + 1], members: [n].  Only enqueues.
template <uint32_t CHUNK>
inline void enqueue_member_lists(const uint32_t *labels, uint64_t n, uint32_t k, uint32_t *table, uint32_t *count, uint32_t *coff,
                                 uint32_t *choff, uint32_t *members, hipStream_t stream) {
    const MemberSegs s = member_segs(n);
    const size_t lds = (size_t)k * 4;
    hipLaunchKernelGGL(kmeans_count_kernel, dim3(s.segs), dim3(64), lds, stream, labels, n, s.seg_rows, k, table);
    hipLaunchKernelGGL(kmeans_segscan_kernel, dim3((k + 255) / 256), dim3(256), 0, stream, table, s.segs, k, count);
    hipLaunchKernelGGL(kmeans_offsets_kernel<CHUNK>, dim3(1), dim3(256), 0, stream, count, k, coff, choff);
    hipLaunchKernelGGL(kmeans_place_kernel, dim3(s.segs), dim3(64), lds, stream, labels, n, s.seg_rows, k, table, coff, members);
}

}  // namespace
}  // namespace cleora
