// pq.hip — product quantisation of an embedding on the device (pycleora/compress.py:32-181): a fused encode kernel for all
// subspaces at once, an order-fixed Euclidean update, the training loop, a batched ADC search and the reconstruction.
// Nothing proportional to n x kc or to n_queries x n is ever stored.
//
//   assign     code[r][m] = argmin_c ||c_mc||^2 - 2 x_rm . c_mc over the kc centroids of subspace m (x_rm: columns m ds .. of row
//              r); ||x_rm||^2 is the same for every c and left out.  Ties go to the LOWER centroid index (numpy's argmin).
//     grid     (row-tile groups, M).  A block of 256 threads = 4 waves stages the WHOLE codebook of its subspace in LDS once
//              ([kc padded to 64][ds padded to 8, + 4] floats, zeros in the padding; at most 256 x 68 floats) with every
//              ||c||^2 behind it, and then walks tiles of PR = 128 rows (tile, tile + gridDim.x, ..): the codebook is read from
//              L2 once per block, X from HBM once.
//     operands wave w owns rows 32 w .. 32 w + 31 of the tile for ALL centroids, so no two waves ever share a row.  Its X
//              fragments never pass through LDS: lane (h = lane >> 5, l = lane & 31) loads columns 8 j + 4 h .. + 3 of row l
//              (one float4 per 8 columns, at most 8 of them = 32 VGPRs; a row's 128-byte slice is consumed whole by the lane pair)
//              and keeps them for every centroid step.  A step is 64 centroids: two 16-register accumulators of
//              v_mfma_f32_32x32x2_f32 (A = centroid rows from LDS, B = the resident X fragment, read once for both).
//     arg-min  every lane visits its 32 scores of a step in ascending centroid index with a strict <, steps ascending, so the
//              lowest index of equal scores stays; padding centroids are skipped by index (c < kc).  The two lanes of a row
//              (h = 0 / 1) meet by one cross-lane exchange under (score ascending, index ascending).
//     store    the block owns ONE byte column of codes[n][M], so writing it in place would scatter single bytes 1 : M.  Instead
//              four lanes' codes are packed into one 32-bit word and stored into a subspace-major plane planes[m][n padded to 128]
//              in the workspace (a wave writes 32 consecutive bytes); pq_pack_kernel then interleaves the planes into codes[n][M]
//              with consecutive lanes on consecutive bytes.  The detour moves 2 M bytes per row against M ds 4 bytes of X (1.6 %
//              at ds = 32), and the training loop skips it: its update reads the planes, coalesced.  Looping the subspaces inside
//              a block was the alternative; it re-stages a 68 KiB codebook M times per block.
//     distance optional: sum_j (x_j - c_j)^2 to the chosen centroid, straight from the resident fragment and the LDS codebook
//              (no cancellation), the lane pair's halves added in a fixed order.
//   update     centroid_mc = mean of its members' sub-rows (plain Euclidean, :154-160), f64 sums in ascending row order, one
//              rounding to f32; no members: the old bits stay.  The chain is kmeans.hip's (count / scan / place / chunked sum /
//              finish) over the M kc clusters (m, c) in ONE pass, written again here: sharing it would template every kernel of
//              kmeans.hip on the label type (bytes with two strides), on a cluster -> column-window map and on the finish
//              (normalise there, compare here), and the k-means results have to stay bit-equal — more risk than the ~150 lines save.
//     count    grid (segments, M): one wave counts the codes of its rows in LDS -> table[m][segment][c];
//     scan     per cluster over the segments, then over all M kc clusters: coff = first member slot, choff = first chunk;
//     place    grid (segments, M): members[] holds every cluster's rows in ascending row order;
//     sum      one 256-thread block per chunk of 256 members: thread (column t & 63, quarter t >> 6) adds its 64 members in
//              order, the four quarters are added in order -> part[chunk][ds] (f64);
//     finish   one wave per cluster: the chunk partials in order, / count, rounded once; |old - new| <= 1e-6 + 1e-5 |new| in f32
//              (np.allclose(old, new, atol=1e-6), :162) is collected per subspace with an integer atomic OR.
//     frozen   a subspace whose flag is set is skipped by every kernel above (the training loop's early stop per subspace).
//   search     ADC (:64-98): table[q][m][c] = c_mc / max(||c_mc||, 1e-10) . q_m / ||q|| (q unscaled when ||q|| <= 1e-10), computed
//              in f64 and rounded once (pq_table_kernel, one block per query, written in the scan's LDS layout), then
//     scan     grid (query tiles of QB, row splits), 1024 threads.  The tables of QB queries sit in LDS as [m][code][QB], so one
//              16-byte read serves four queries for one code.  QB = 8 while M kc <= 2048 (64 KiB of tables + 19 KiB of lists: one
//              block of 16 waves per CU), 4 up to 8192 (128 KiB), 2 beyond (M kc <= 16384: 128 KiB).  A thread takes one row at a
//              time: its M code bytes by the widest load M allows (16 / 8 / 4 / 1 bytes), the M table values added IN SUBSPACE
//              ORDER in f32 from +0 (the reference's scores += dist_tables[m, codes[:, m]]).
//     top-k    a candidate is the 64-bit key (score as an order-preserving u32) << 32 | row: larger key = better under "score
//              descending, ties to the larger row", a STRICT total order, so the result does not depend on the order in which
//              threads meet candidates.  Keys above the query's threshold (its k-th best so far) are appended to an LDS list
//              (integer atomic cursor); a list that reaches 128 entries — or overflows its 256, in which case the thread retries —
//              is compacted by one wave: k rounds of "largest key below the previous pick".  Every block leaves k keys per query;
//     merge    one wave per query picks the k best keys of its splits the same way and decodes them.
//   reconstruct  out[r][m ds + j] = codebooks[m][codes[row][m]][j], one thread per element.
// Deterministic: no floating-point atomics; integer atomics for counts, cursors and flags only.
#include <cmath>
#include <type_traits>

#include "common.h"

namespace cleora {
namespace {

constexpr int PR = 128;               // rows per tile of the assign kernel: 4 waves x 32
constexpr int PTHREADS = 256;
constexpr uint32_t PQ_MAX_KC = 256, PQ_MAX_DS = 64, PQ_MAX_M = 64, PQ_MAX_TOPK = 32;
constexpr uint32_t PQ_ASSIGN_BLOCKS = 2048;   // blocks of one assign launch (2 fit a CU by LDS: 4 rounds on 256 CUs)
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t UCHUNK = 256;          // members per chunk of the update's sum
constexpr uint64_t USEGS = 512;           // most row segments of count / place
constexpr uint64_t USEG_MIN_ROWS = 1024;  // fewest rows per segment (a multiple of 64)
constexpr int STHREADS = 1024;            // threads of a scan block
constexpr uint32_t SLIST = 32;            // slots of a query's kept list (>= PQ_MAX_TOPK)
constexpr uint32_t SCAP = 256;            // candidate slots per query behind it
constexpr uint32_t STRIG = 128;           // a list this long is compacted
constexpr uint64_t SPLIT_MIN_ROWS = 256;  // fewest rows of a row split
constexpr uint64_t SCAN_BLOCKS = 512;     // blocks a scan launch aims for when it has few query tiles

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline uint64_t up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------------------------------------------------------- assign

struct PqAssignArgs {
    const float *x;
    uint64_t ldx, n, npad;
    uint32_t M, ds, dsp, kc, kcp;
    const float *cb;               // [M][kc][ds]
    uint8_t *planes;               // [M][npad]
    float *dist;                   // [n][M] or nullptr
    const uint32_t *frozen;        // [M] or nullptr: subspaces to skip
};

template <bool VEC>
__global__ __launch_bounds__(PTHREADS) void pq_assign_kernel(const PqAssignArgs a) {
    extern __shared__ float4 pq_lds[];
    float *Cs = reinterpret_cast<float *>(pq_lds);          // [kcp][dsp + 4]
    const uint32_t cs = a.dsp + 4;
    float *cn = Cs + a.kcp * cs;                            // [kcp] ||c||^2
    const uint32_t m = blockIdx.y;
    if (a.frozen != nullptr && a.frozen[m] != 0u) return;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, h = lane >> 5, l32 = lane & 31;

    const float *cb = a.cb + (uint64_t)m * a.kc * a.ds;
    for (uint32_t i = t; i < a.kcp * cs; i += PTHREADS) {
        const uint32_t c = i / cs, j = i - c * cs;
        Cs[i] = (c < a.kc && j < a.ds) ? cb[c * a.ds + j] : 0.0f;
    }
    __syncthreads();
    for (uint32_t c = t; c < a.kcp; c += PTHREADS) {
        float s = 0.f;
        for (uint32_t j = 0; j < a.ds; ++j) s += Cs[c * cs + j] * Cs[c * cs + j];
        cn[c] = s;
    }
    __syncthreads();

    // columns c .. c + 3 of the subspace's slice of row r, zeros outside
    auto load_x4 = [&](uint64_t r, uint32_t c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < a.n && c < a.ds) {
            const float *p = a.x + r * a.ldx + (uint64_t)m * a.ds + c;
            if constexpr (VEC) {
                v = *reinterpret_cast<const float4 *>(p);
            } else {
                v.x = p[0];
                if (c + 1 < a.ds) v.y = p[1];
                if (c + 2 < a.ds) v.z = p[2];
                if (c + 3 < a.ds) v.w = p[3];
            }
        }
        return v;
    };

    const uint64_t ntiles = (a.n + PR - 1) / PR;
    const uint32_t nsteps = a.kcp / 64;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t r = tile * PR + w * 32 + l32;
        float4 xf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xf[j] = (uint32_t)(j * 8) < a.dsp ? load_x4(r, j * 8 + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);

        float best = 0.f;
        uint32_t bidx = kNone;               // kNone: this lane has not seen a centroid yet
        for (uint32_t s = 0; s < nsteps; ++s) {
            floatx16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
            const float *ca = Cs + (s * 64 + l32) * cs + 4 * h;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if ((uint32_t)(j * 8) < a.dsp) {
                    const float4 fa0 = *reinterpret_cast<const float4 *>(ca + j * 8);
                    const float4 fa1 = *reinterpret_cast<const float4 *>(ca + 32 * cs + j * 8);
                    const float4 fb = xf[j];
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.x, fb.x, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.x, fb.x, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.y, fb.y, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.y, fb.y, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.z, fb.z, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.z, fb.z, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.w, fb.w, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.w, fb.w, acc1, 0, 0, 0);
                }
            }
            // accumulator 4 j + i of acc0: centroid 64 s + 8 j + 4 h + i, of acc1: 32 more; row l32 of the wave.
            // Ascending index and a strict <: the lowest index of equal scores stays
            const uint32_t cbase = s * 64 + 4 * h;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t c = cbase + 8 * (e >> 2) + (e & 3);
                const float sc = cn[c] - 2.0f * acc0[e];
                if (c < a.kc && (bidx == kNone || sc < best)) { best = sc; bidx = c; }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const uint32_t c = cbase + 32 + 8 * (e >> 2) + (e & 3);
                const float sc = cn[c] - 2.0f * acc1[e];
                if (c < a.kc && (bidx == kNone || sc < best)) { best = sc; bidx = c; }
            }
        }
        // the two lanes of a row
        const float ob = __shfl_xor(best, 32, 64);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bidx, 32, 64);
        if (oi != kNone && (bidx == kNone || ob < best || (ob == best && oi < bidx))) { best = ob; bidx = oi; }
        if (bidx == kNone) bidx = 0;         // cannot happen for kc >= 1: the lane of centroid 0 always has an entry

        if (a.dist != nullptr) {
            const float *cc = Cs + bidx * cs + 4 * h;
            float part = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if ((uint32_t)(j * 8) < a.dsp) {
                    const float4 c4 = *reinterpret_cast<const float4 *>(cc + j * 8);
                    const float dx = xf[j].x - c4.x, dy = xf[j].y - c4.y, dz = xf[j].z - c4.z, dw = xf[j].w - c4.w;
                    part += dx * dx;
                    part += dy * dy;
                    part += dz * dz;
                    part += dw * dw;
                }
            }
            const float other = __shfl_xor(part, 32, 64);
            if (h == 0 && r < a.n) a.dist[r * a.M + m] = part + other;
        }
        // four rows' codes per 32-bit word; rows beyond n land in the plane's padding
        uint32_t word = bidx;
        word |= (uint32_t)__shfl_down((int)bidx, 1, 64) << 8;
        word |= (uint32_t)__shfl_down((int)bidx, 2, 64) << 16;
        word |= (uint32_t)__shfl_down((int)bidx, 3, 64) << 24;
        if (h == 0 && (l32 & 3) == 0) *reinterpret_cast<uint32_t *>(a.planes + (uint64_t)m * a.npad + tile * PR + w * 32 + l32) = word;
    }
}

// codes[r][m] = planes[m][r]: one thread per byte, consecutive lanes on consecutive bytes.
__global__ __launch_bounds__(256) void pq_pack_kernel(const uint8_t *__restrict__ planes, uint64_t n, uint64_t npad, uint32_t M,
                                                      uint8_t *__restrict__ codes) {
    const uint64_t i = CLEORA_LINEAR_BLOCK() * 256 + threadIdx.x;
    if (i >= n * M) return;
    const uint64_t r = i / M;
    const uint32_t m = (uint32_t)(i - r * M);
    codes[i] = planes[m * npad + r];
}

// ---------------------------------------------------------------------------------------------------------------- update
// The label of (row r, subspace m) is lab[r * rs + m * ms]: codes[n][M] (rs = M, ms = 1) or the planes (rs = 1, ms = npad).

__global__ __launch_bounds__(256) void pq_fill_kernel(uint32_t *__restrict__ v, uint32_t n, uint32_t value) {
    for (uint32_t i = threadIdx.x; i < n; i += 256) v[i] = value;
}

__global__ __launch_bounds__(64) void pq_count_kernel(const uint8_t *__restrict__ lab, uint64_t rs, uint64_t ms, uint64_t n, uint64_t seg_rows,
                                                      uint32_t kc, const uint32_t *__restrict__ frozen, uint32_t *__restrict__ table) {
    __shared__ uint32_t cnt[PQ_MAX_KC];
    const uint32_t lane = threadIdx.x, m = blockIdx.y;
    if (frozen != nullptr && frozen[m] != 0u) return;
    for (uint32_t c = lane; c < kc; c += 64) cnt[c] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * seg_rows, end = begin + seg_rows < n ? begin + seg_rows : n;
    for (uint64_t r = begin + lane; r < end; r += 64) {
        const uint32_t l = lab[r * rs + m * ms];
        if (l < kc) atomicAdd(&cnt[l], 1u);
    }
    __syncthreads();
    for (uint32_t c = lane; c < kc; c += 64) table[((uint64_t)m * gridDim.x + blockIdx.x) * kc + c] = cnt[c];
}

// One thread per cluster (m, c): its column of the table becomes the exclusive scan over the segments; count = its total.
__global__ __launch_bounds__(256) void pq_segscan_kernel(uint32_t *__restrict__ table, uint32_t segs, uint32_t M, uint32_t kc,
                                                         const uint32_t *__restrict__ frozen, uint32_t *__restrict__ count) {
    const uint32_t L = blockIdx.x * 256 + threadIdx.x;
    if (L >= M * kc) return;
    const uint32_t m = L / kc, c = L - m * kc;
    uint32_t run = 0;
    if (frozen == nullptr || frozen[m] == 0u) {
        for (uint32_t b = 0; b < segs; ++b) {
            const uint64_t at = ((uint64_t)m * segs + b) * kc + c;
            const uint32_t v = table[at];
            table[at] = run;
            run += v;
        }
    }
    count[L] = run;
}

// One block: coff[L] = members before cluster L, choff[L] = chunks of UCHUNK members before it; [K] = the totals.  Also clears
// the subspaces' "not close" flags.
__global__ __launch_bounds__(256) void pq_offsets_kernel(const uint32_t *__restrict__ count, uint32_t K, uint32_t *__restrict__ coff,
                                                         uint32_t *__restrict__ choff, uint32_t *__restrict__ notclose, uint32_t M) {
    __shared__ uint32_t sa[256], sb[256];
    const uint32_t t = threadIdx.x, per = (K + 255) / 256;
    const uint32_t c0 = t * per < K ? t * per : K, c1 = c0 + per < K ? c0 + per : K;
    if (t < M) notclose[t] = 0u;
    uint32_t ma = 0, mb = 0;
    for (uint32_t c = c0; c < c1; ++c) {
        ma += count[c];
        mb += (count[c] + UCHUNK - 1) / UCHUNK;
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
        rb += (count[c] + UCHUNK - 1) / UCHUNK;
    }
    if (t == 255) {
        coff[K] = sa[255];
        choff[K] = sb[255];
    }
}

// One wave per (segment, subspace), 64 rows at a time in row order: members[coff[L] ..] = the rows of cluster L, ascending.
__global__ __launch_bounds__(64) void pq_place_kernel(const uint8_t *__restrict__ lab, uint64_t rs, uint64_t ms, uint64_t n, uint64_t seg_rows,
                                                      uint32_t kc, const uint32_t *__restrict__ frozen, const uint32_t *__restrict__ table,
                                                      const uint32_t *__restrict__ coff, uint64_t slots, uint32_t *__restrict__ members) {
    __shared__ uint32_t cur[PQ_MAX_KC];
    const int lane = threadIdx.x;
    const uint32_t m = blockIdx.y;
    if (frozen != nullptr && frozen[m] != 0u) return;
    for (uint32_t c = lane; c < kc; c += 64) cur[c] = coff[m * kc + c] + table[((uint64_t)m * gridDim.x + blockIdx.x) * kc + c];
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * seg_rows, end = begin + seg_rows < n ? begin + seg_rows : n;
    for (uint64_t base = begin; base < end; base += 64) {
        const uint64_t r = base + lane;
        uint32_t l = r < end ? (uint32_t)lab[r * rs + m * ms] : kNone;
        if (l >= kc) l = kNone;
        uint32_t before = 0;
        bool later = false;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const bool same = (uint32_t)__shfl((int)l, j, 64) == l;
            before += (same && j < lane) ? 1u : 0u;
            later = later || (same && j > lane);
        }
        uint32_t pos = 0;
        if (l != kNone) {
            pos = cur[l] + before;
            if (pos < slots) members[pos] = (uint32_t)r;      // always true while nobody rewrites the labels under this call
        }
        __syncthreads();
        if (l != kNone && !later) cur[l] = pos + 1;           // the last lane of a label moves its cursor
        __syncthreads();
    }
}

// One block per chunk: part[chunk][col] = sum over the chunk's members, in member order, of the member's sub-row (f64).
__global__ __launch_bounds__(256) void pq_sum_kernel(const float *__restrict__ x, uint64_t ldx, uint32_t ds, uint32_t kc, uint32_t K,
                                                     const uint32_t *__restrict__ members, const uint32_t *__restrict__ coff,
                                                     const uint32_t *__restrict__ choff, double *__restrict__ part) {
    __shared__ uint32_t mrow[UCHUNK];
    __shared__ double red[4][64];
    const uint64_t q = CLEORA_LINEAR_BLOCK();
    if (q >= choff[K]) return;
    uint32_t lo = 0, hi = K;                 // the cluster of chunk q: the last L with choff[L] <= q (empty clusters have no chunk)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (choff[mid] <= q) lo = mid; else hi = mid;
    }
    const uint32_t t = threadIdx.x, col = t & 63, quarter = t >> 6;
    const uint32_t m0 = coff[lo] + ((uint32_t)q - choff[lo]) * UCHUNK;
    const uint32_t m1 = coff[lo + 1] - m0 < UCHUNK ? coff[lo + 1] : m0 + UCHUNK;
    const uint32_t cnt = m1 - m0;
    if (t < cnt) mrow[t] = members[m0 + t];
    __syncthreads();
    double acc = 0.0;
    if (col < ds) {
        const float *xc = x + (uint64_t)(lo / kc) * ds + col;
        const uint32_t e = quarter * 64 + 64 < cnt ? quarter * 64 + 64 : cnt;
        for (uint32_t i = quarter * 64; i < e; ++i) acc += (double)xc[(uint64_t)mrow[i] * ldx];
    }
    red[quarter][col] = acc;
    __syncthreads();
    if (quarter == 0 && col < ds) part[q * ds + col] = ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
}

// One wave per cluster: chunk partials in chunk order -> mean, rounded once; the allclose test against the old centroid.
__global__ __launch_bounds__(64) void pq_finish_kernel(const double *__restrict__ part, const uint32_t *__restrict__ coff,
                                                       const uint32_t *__restrict__ choff, uint32_t ds, uint32_t kc,
                                                       const uint32_t *__restrict__ frozen, float *__restrict__ cb, uint32_t *__restrict__ notclose) {
    const uint32_t L = blockIdx.x, t = threadIdx.x, m = L / kc;
    if (frozen != nullptr && frozen[m] != 0u) return;
    const uint32_t cnt = coff[L + 1] - coff[L];
    if (cnt == 0) return;                                   // no members: the old centroid stays (and is close to itself)
    bool far = false;
    if (t < ds) {
        double s = 0.0;
        for (uint64_t q = choff[L]; q < choff[L + 1]; ++q) s += part[q * ds + t];
        const float fresh = (float)(s / (double)cnt), old = cb[(uint64_t)L * ds + t];
        const float bound = 1e-6f + 1e-5f * fabsf(fresh);   // np.isclose on float32 arrays: f32 arithmetic throughout
        far = !(fabsf(old - fresh) <= bound || old == fresh);
        cb[(uint64_t)L * ds + t] = fresh;
    }
    if (__ballot(far) != 0ull && t == 0) atomicOr(&notclose[m], 1u);
}

// close[m] = the subspace's update passed np.allclose (a frozen one stays 1); passing freezes it.
__global__ __launch_bounds__(64) void pq_freeze_kernel(const uint32_t *__restrict__ notclose, uint32_t M, uint32_t *__restrict__ frozen,
                                                       uint32_t *__restrict__ close) {
    const uint32_t m = threadIdx.x;
    if (m >= M) return;
    uint32_t c = 1u;
    if (frozen == nullptr || frozen[m] == 0u) {
        c = notclose[m] == 0u ? 1u : 0u;
        if (frozen != nullptr && c != 0u) frozen[m] = 1u;
    }
    if (close != nullptr) close[m] = c;
}

// ---------------------------------------------------------------------------------------------------------------- search

__device__ inline uint32_t score_bits(float f) {            // order-preserving: a < b  <=>  score_bits(a) < score_bits(b)
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) != 0u ? 0xffffffffu : 0x80000000u);
}
__device__ inline float bits_score(uint32_t o) { return __uint_as_float((o & 0x80000000u) != 0u ? o ^ 0x80000000u : ~o); }
__device__ inline u64 shfl_u64(u64 v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ inline u64 wave_max_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
        const u64 other = ((u64)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

// One wave: lane j < k ends up with the j-th largest of keys[0 .. total) (0 = none; keys are distinct or 0).  k rounds of "the
// largest key below the previous pick": exact under the strict order of the keys, whatever order they were stored in.
template <typename Load>
__device__ inline u64 select_keys(Load load, uint32_t total, uint32_t k, int lane) {
    u64 prev = ~0ull, mine = 0ull;
    for (uint32_t j = 0; j < k; ++j) {
        u64 best = 0ull;
        for (uint32_t i = lane; i < total; i += 64) {
            const u64 v = load(i);
            if (v < prev && v > best) best = v;
        }
        best = wave_max_u64(best);
        if ((uint32_t)lane == j) mine = best;
        prev = best;
    }
    return mine;
}

// One block per (padded) query: its lookup tables in the scan's layout T[tile][m][c][QB].  f64 throughout, one rounding.
__global__ __launch_bounds__(256) void pq_table_kernel(const float *__restrict__ queries, uint64_t nq, const float *__restrict__ cb, uint32_t M,
                                                       uint32_t kc, uint32_t ds, uint32_t QB, float *__restrict__ tables) {
    extern __shared__ float4 pq_q_lds[];
    float *qs = reinterpret_cast<float *>(pq_q_lds);        // [d]
    __shared__ double red[256];
    const uint64_t q = CLEORA_LINEAR_BLOCK();
    const uint32_t t = threadIdx.x, d = M * ds;
    const uint64_t tile = q / QB;
    const uint32_t qi = (uint32_t)(q - tile * QB);
    float *out = tables + tile * ((uint64_t)M * kc * QB) + qi;
    if (q >= nq) {                                          // the padding of the last tile scores 0 and is never read back
        for (uint32_t i = t; i < M * kc; i += 256) out[(uint64_t)i * QB] = 0.0f;
        return;
    }
    double sq = 0.0;
    for (uint32_t j = t; j < d; j += 256) {
        const float v = queries[q * d + j];
        qs[j] = v;
        sq += (double)v * (double)v;
    }
    red[t] = sq;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const double qn = sqrt(red[0]), qscale = qn > 1e-10 ? 1.0 / qn : 1.0;      // :68-72
    for (uint32_t i = t; i < M * kc; i += 256) {
        const uint32_t m = i / kc;
        const float *c = cb + (uint64_t)i * ds, *qm = qs + m * ds;
        double dot = 0.0, cn = 0.0;
        for (uint32_t j = 0; j < ds; ++j) {
            dot += (double)c[j] * (double)qm[j];
            cn += (double)c[j] * (double)c[j];
        }
        const double norm = sqrt(cn);
        out[(uint64_t)i * QB] = (float)(dot * qscale / (norm > 1e-10 ? norm : 1e-10));
    }
}

struct PqScanArgs {
    const uint8_t *codes;          // [n][M]
    uint64_t n, nq, split_rows;
    uint32_t M, kc, k, splits;
    const float *tables;           // [tiles][M][kc][QB]
    u64 *lists;                    // [tiles][splits][QB][SLIST]
    float *all_scores;             // [nq][n] or nullptr
};

template <int QB, int W>
__global__ __launch_bounds__(STHREADS) void pq_scan_kernel(const PqScanArgs a) {
    extern __shared__ float4 pq_scan_lds[];
    float *T = reinterpret_cast<float *>(pq_scan_lds);                         // [M][kc][QB]
    const uint32_t tsize = a.M * a.kc * QB;
    u64 *items = reinterpret_cast<u64 *>(T + ((tsize + 3u) & ~3u));            // [QB][SLIST kept + SCAP candidates]
    u64 *thr = items + QB * (SLIST + SCAP);                                    // [QB] the k-th best key so far, 0 = fewer than k
    uint32_t *cnt = reinterpret_cast<uint32_t *>(thr + QB);                    // [QB] candidates in the list
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t tile = blockIdx.x, sp = blockIdx.y;

    const float *tg = a.tables + tile * tsize;
    for (uint32_t i = t; i < tsize; i += STHREADS) T[i] = tg[i];
    for (uint32_t i = t; i < QB * (SLIST + SCAP); i += STHREADS) items[i] = 0ull;
    if (t < QB) {
        thr[t] = 0ull;
        cnt[t] = 0u;
    }
    __syncthreads();

    auto compact = [&](uint32_t q, uint32_t c) {             // one wave
        u64 *it = items + q * (SLIST + SCAP);
        const u64 mine = select_keys([&](uint32_t i) { return it[i]; }, SLIST + c, a.k, (int)lane);
        if (lane < SLIST) it[lane] = mine;
        const u64 kth = shfl_u64(mine, (int)a.k - 1);
        if (lane == 0) {
            thr[q] = kth;
            cnt[q] = 0u;
        }
    };

    const uint64_t rb = sp * a.split_rows, re = rb + a.split_rows < a.n ? rb + a.split_rows : a.n;
    const uint32_t kmax = a.kc - 1;
    for (uint64_t base = rb; base < re; base += STHREADS) {
        const uint64_t r = base + t;
        const bool valid = r < re;
        float sc[QB];
#pragma unroll
        for (int q = 0; q < QB; ++q) sc[q] = 0.0f;
        if (valid) {
            const uint8_t *p = a.codes + r * a.M;
            for (uint32_t m0 = 0; m0 < a.M; m0 += W) {
                uint32_t wv[W >= 4 ? W / 4 : 1];
                if constexpr (W == 16) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(p + m0);
                    wv[0] = v.x; wv[1] = v.y; wv[2] = v.z; wv[3] = v.w;
                } else if constexpr (W == 8) {
                    const uint2 v = *reinterpret_cast<const uint2 *>(p + m0);
                    wv[0] = v.x; wv[1] = v.y;
                } else if constexpr (W == 4) {
                    wv[0] = *reinterpret_cast<const uint32_t *>(p + m0);
                } else {
                    wv[0] = p[m0];
                }
#pragma unroll
                for (int b = 0; b < W; ++b) {                // subspace order
                    uint32_t code = (wv[b >> 2] >> (8 * (b & 3))) & 0xffu;
                    code = code < kmax ? code : kmax;        // a byte beyond the codebook never leaves the table
                    const float *e = T + ((m0 + b) * a.kc + code) * QB;
                    if constexpr (QB == 2) {
                        const float2 v = *reinterpret_cast<const float2 *>(e);
                        sc[0] += v.x;
                        sc[1] += v.y;
                    } else {
#pragma unroll
                        for (int g = 0; g < QB / 4; ++g) {
                            const float4 v = *reinterpret_cast<const float4 *>(e + 4 * g);
                            sc[4 * g] += v.x;
                            sc[4 * g + 1] += v.y;
                            sc[4 * g + 2] += v.z;
                            sc[4 * g + 3] += v.w;
                        }
                    }
                }
            }
            if (a.all_scores != nullptr) {
#pragma unroll
                for (int q = 0; q < QB; ++q)
                    if (tile * QB + q < a.nq) a.all_scores[(tile * QB + q) * a.n + r] = sc[q];
            }
        }
        uint32_t pending = 0;
        if (valid) {
#pragma unroll
            for (int q = 0; q < QB; ++q)
                if ((((u64)score_bits(sc[q]) << 32) | (uint32_t)r) > thr[q]) pending |= 1u << q;
        }
        // every pass: pending keys go into their lists, full lists are compacted, keys that found no slot try again
        while (__syncthreads_or((int)pending)) {
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                if ((pending >> q) & 1u) {
                    const u64 key = ((u64)score_bits(sc[q]) << 32) | (uint32_t)r;
                    if (key <= thr[q]) {
                        pending &= ~(1u << q);
                    } else {
                        const uint32_t slot = atomicAdd(&cnt[q], 1u);
                        if (slot < SCAP) {
                            items[q * (SLIST + SCAP) + SLIST + slot] = key;
                            pending &= ~(1u << q);
                        }
                    }
                }
            }
            __syncthreads();
            for (uint32_t q = w; q < (uint32_t)QB; q += STHREADS / 64) {
                const uint32_t c = cnt[q];
                if (c >= STRIG) compact(q, c < SCAP ? c : SCAP);
            }
        }
    }
    __syncthreads();
    for (uint32_t q = w; q < (uint32_t)QB; q += STHREADS / 64) {
        const uint32_t c = cnt[q];
        if (c > 0u) compact(q, c < SCAP ? c : SCAP);
    }
    __syncthreads();
    u64 *out = a.lists + (tile * a.splits + sp) * (QB * SLIST);
    for (uint32_t i = t; i < QB * SLIST; i += STHREADS) out[i] = items[(i / SLIST) * (SLIST + SCAP) + (i % SLIST)];
}

// One wave per query: the k best keys of its splits' lists, decoded.
__global__ __launch_bounds__(64) void pq_merge_kernel(const u64 *__restrict__ lists, uint32_t QB, uint32_t splits, uint32_t k,
                                                      uint32_t *__restrict__ out_index, float *__restrict__ out_score) {
    const uint64_t q = CLEORA_LINEAR_BLOCK();
    const int lane = threadIdx.x;
    const uint64_t tile = q / QB;
    const uint32_t qi = (uint32_t)(q - tile * QB);
    const u64 *base = lists + tile * splits * (QB * SLIST) + qi * SLIST;
    const u64 mine = select_keys([&](uint32_t i) { return base[(uint64_t)(i / k) * (QB * SLIST) + (i % k)]; }, splits * k, k, lane);
    if ((uint32_t)lane < k) {
        out_index[q * k + lane] = mine != 0ull ? (uint32_t)mine : kNone;
        out_score[q * k + lane] = mine != 0ull ? bits_score((uint32_t)(mine >> 32)) : -INFINITY;
    }
}

// ---------------------------------------------------------------------------------------------------------------- reconstruct

__global__ __launch_bounds__(256) void pq_reconstruct_kernel(const uint8_t *__restrict__ codes, uint64_t n, const float *__restrict__ cb, uint32_t M,
                                                             uint32_t kc, uint32_t ds, const uint32_t *__restrict__ rows, uint64_t n_rows,
                                                             float *__restrict__ out, uint64_t ldo) {
    const uint64_t i = CLEORA_LINEAR_BLOCK() * 256 + threadIdx.x, d = (uint64_t)M * ds;
    if (i >= n_rows * d) return;
    const uint64_t r = i / d;
    const uint32_t col = (uint32_t)(i - r * d), m = col / ds, j = col - m * ds;
    const uint64_t row = rows != nullptr ? rows[r] : r;
    float v = 0.0f;
    if (row < n) {
        const uint32_t code = codes[row * M + m];
        if (code < kc) v = cb[((uint64_t)m * kc + code) * ds + j];
    }
    out[r * ldo + col] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host

struct PqPlan {
    uint32_t ds, dsp, kcp, segs, K;
    uint64_t npad, seg_rows, max_chunks;
    uint64_t off_frozen, off_notclose, off_close, off_members, off_table, off_count, off_coff, off_choff, off_part, bytes;
};

PqPlan pq_plan(uint64_t n, uint32_t d, uint32_t M, uint32_t kc) {
    PqPlan p;
    M = M ? M : 1;
    p.ds = d / M ? d / M : 1;
    p.dsp = (uint32_t)up(p.ds, 8);
    p.kcp = (uint32_t)up(kc ? kc : 1, 64);
    p.K = M * kc;
    p.npad = up(n ? n : 1, PR);
    p.seg_rows = up((n + USEGS - 1) / USEGS, 64);
    if (p.seg_rows < USEG_MIN_ROWS) p.seg_rows = USEG_MIN_ROWS;
    p.segs = (uint32_t)((n + p.seg_rows - 1) / p.seg_rows);
    if (p.segs < 1) p.segs = 1;
    p.max_chunks = (n * M + UCHUNK - 1) / UCHUNK + p.K;        // sum over clusters of ceil(count / UCHUNK) is at most this
    // the table is sized by a bound on segs that is monotone in n (segs itself is not)
    const uint64_t by_rows = (n + USEG_MIN_ROWS - 1) / USEG_MIN_ROWS;
    const uint64_t segs_bound = by_rows < 1 ? 1 : (by_rows < USEGS ? by_rows : USEGS);
    p.off_frozen = up(p.npad * M, 256);                        // [0, ..): the code planes
    p.off_notclose = p.off_frozen + 256;
    p.off_close = p.off_notclose + 256;
    p.off_members = p.off_close + 256;
    p.off_table = p.off_members + up(n * M * 4, 256);
    p.off_count = p.off_table + up(segs_bound * p.K * 4, 256);
    p.off_coff = p.off_count + up((uint64_t)p.K * 4, 256);
    p.off_choff = p.off_coff + up(((uint64_t)p.K + 1) * 4, 256);
    p.off_part = p.off_choff + up(((uint64_t)p.K + 1) * 4, 256);
    p.bytes = p.off_part + p.max_chunks * p.ds * 8;
    return p;
}

int pq_check_shape(uint64_t n, uint32_t d, uint32_t M, uint32_t kc) {
    CL_REQUIRE(M >= 1 && M <= PQ_MAX_M, "need 1 <= M <= 64 subspaces");
    CL_REQUIRE(d >= 1 && d % M == 0, "d must be a positive multiple of the number of subspaces M");
    CL_REQUIRE(d / M <= PQ_MAX_DS, "the subspace width d / M is larger than 64");
    CL_REQUIRE(kc >= 1 && kc <= PQ_MAX_KC, "need 1 <= kc <= 256 centroids per subspace (codes are uint8)");
    CL_REQUIRE(n < (1ull << 32), "more than 2^32 rows");
    CL_REQUIRE((uint64_t)kc <= n, "kc cannot be larger than the number of rows n");
    return CLEORA_OK;
}

int pq_check(const void *x, uint64_t ldx, uint64_t n, uint32_t d, const void *codebooks, uint32_t M, uint32_t kc, const void *codes,
             const void *workspace) {
    CL_REQUIRE(x != nullptr && codebooks != nullptr && codes != nullptr && workspace != nullptr,
               "x / codebooks / codes / workspace is NULL");
    const int rc = pq_check_shape(n, d, M, kc);
    if (rc != CLEORA_OK) return rc;
    CL_REQUIRE(ldx >= d, "need ldx >= d");
    return CLEORA_OK;
}

// codes == nullptr: the planes in the workspace are the only output (the training loop's iterations)
int enqueue_pq_assign(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const float *cb, uint32_t M, uint32_t kc, uint8_t *codes,
                      float *dist, const uint32_t *frozen, void *workspace, hipStream_t stream) {
    const PqPlan p = pq_plan(n, d, M, kc);
    PqAssignArgs a;
    a.x = x;
    a.ldx = ldx;
    a.n = n;
    a.npad = p.npad;
    a.M = M;
    a.ds = p.ds;
    a.dsp = p.dsp;
    a.kc = kc;
    a.kcp = p.kcp;
    a.cb = cb;
    a.planes = static_cast<uint8_t *>(workspace);
    a.dist = dist;
    a.frozen = frozen;
    const bool vec = p.ds % 4 == 0 && ldx % 4 == 0 && aligned16(x);
    const size_t lds = ((size_t)p.kcp * (p.dsp + 4) + p.kcp) * 4;
    const uint64_t ntiles = p.npad / PR, want = PQ_ASSIGN_BLOCKS / M ? PQ_ASSIGN_BLOCKS / M : 1;
    const dim3 blocks((unsigned)(ntiles < want ? ntiles : want), M);
    auto go = [&](auto kernel) {
        // per DEVICE and cheap: set on every call
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) hipLaunchKernelGGL(kernel, blocks, dim3(PTHREADS), lds, stream, a);
        return e;
    };
    CL_HIP(vec ? go(pq_assign_kernel<true>) : go(pq_assign_kernel<false>));
    if (codes != nullptr)
        hipLaunchKernelGGL(pq_pack_kernel, grid_1d_as_2d((n * M + 255) / 256), dim3(256), 0, stream, a.planes, n, p.npad, M, codes);
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

int enqueue_pq_update(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const uint8_t *lab, uint64_t rs, uint64_t ms, float *cb,
                      uint32_t M, uint32_t kc, uint32_t *frozen, uint32_t *close, void *workspace, hipStream_t stream) {
    const PqPlan p = pq_plan(n, d, M, kc);
    char *ws = static_cast<char *>(workspace);
    uint32_t *notclose = reinterpret_cast<uint32_t *>(ws + p.off_notclose);
    uint32_t *members = reinterpret_cast<uint32_t *>(ws + p.off_members), *table = reinterpret_cast<uint32_t *>(ws + p.off_table);
    uint32_t *count = reinterpret_cast<uint32_t *>(ws + p.off_count), *coff = reinterpret_cast<uint32_t *>(ws + p.off_coff);
    uint32_t *choff = reinterpret_cast<uint32_t *>(ws + p.off_choff);
    double *part = reinterpret_cast<double *>(ws + p.off_part);

    hipLaunchKernelGGL(pq_count_kernel, dim3(p.segs, M), dim3(64), 0, stream, lab, rs, ms, n, p.seg_rows, kc, frozen, table);
    hipLaunchKernelGGL(pq_segscan_kernel, dim3((p.K + 255) / 256), dim3(256), 0, stream, table, p.segs, M, kc, frozen, count);
    hipLaunchKernelGGL(pq_offsets_kernel, dim3(1), dim3(256), 0, stream, count, p.K, coff, choff, notclose, M);
    hipLaunchKernelGGL(pq_place_kernel, dim3(p.segs, M), dim3(64), 0, stream, lab, rs, ms, n, p.seg_rows, kc, frozen, table, coff, n * M, members);
    CL_HIP(hipGetLastError());
    hipLaunchKernelGGL(pq_sum_kernel, grid_1d_as_2d(p.max_chunks), dim3(256), 0, stream, x, ldx, p.ds, kc, p.K, members, coff, choff, part);
    hipLaunchKernelGGL(pq_finish_kernel, dim3(p.K), dim3(64), 0, stream, part, coff, choff, p.ds, kc, frozen, cb, notclose);
    hipLaunchKernelGGL(pq_freeze_kernel, dim3(1), dim3(64), 0, stream, notclose, M, frozen, close);
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

struct PqSearchPlan {
    uint32_t QB, splits;
    uint64_t tiles, split_rows, off_lists, bytes;
};

PqSearchPlan pq_search_plan(uint64_t n, uint32_t M, uint32_t kc, uint64_t nq) {
    PqSearchPlan p;
    const uint64_t entries = (uint64_t)(M ? M : 1) * (kc ? kc : 1);
    p.QB = entries <= 2048 ? 8 : (entries <= 8192 ? 4 : 2);
    p.tiles = (nq + p.QB - 1) / p.QB;
    if (p.tiles < 1) p.tiles = 1;
    const uint64_t by_rows = (n + SPLIT_MIN_ROWS - 1) / SPLIT_MIN_ROWS, by_tiles = (SCAN_BLOCKS + p.tiles - 1) / p.tiles;
    uint64_t splits = by_rows < by_tiles ? by_rows : by_tiles;
    if (splits < 1) splits = 1;
    p.split_rows = up((n + splits - 1) / splits ? (n + splits - 1) / splits : 1, 64);
    p.splits = (uint32_t)((n + p.split_rows - 1) / p.split_rows);
    if (p.splits < 1) p.splits = 1;
    p.off_lists = up(p.tiles * entries * p.QB * 4, 256);
    // sized by the bound on the splits, which is monotone in n (splits itself is not)
    p.bytes = p.off_lists + p.tiles * (by_tiles < 1 ? 1 : by_tiles) * p.QB * SLIST * 8;
    return p;
}

}  // namespace

uint64_t pq_workspace_bytes(uint64_t n, uint32_t d, uint32_t M, uint32_t kc) { return pq_plan(n, d, M, kc).bytes; }

int launch_pq_assign(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const float *codebooks, uint32_t M, uint32_t kc, uint8_t *codes_out,
                     float *sqdist_out, void *workspace, hipStream_t stream) {
    const int rc = pq_check(x, ldx, n, d, codebooks, M, kc, codes_out, workspace);
    if (rc != CLEORA_OK) return rc;
    return enqueue_pq_assign(x, ldx, n, d, codebooks, M, kc, codes_out, sqdist_out, nullptr, workspace, stream);
}

int launch_pq_update(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const uint8_t *codes, float *codebooks_io, uint32_t M, uint32_t kc,
                     uint32_t *close_out, void *workspace, hipStream_t stream) {
    const int rc = pq_check(x, ldx, n, d, codebooks_io, M, kc, codes, workspace);
    if (rc != CLEORA_OK) return rc;
    CL_REQUIRE(n * M < (1ull << 32), "n * M must stay below 2^32 (the update's member slots are 32-bit)");
    return enqueue_pq_update(x, ldx, n, d, codes, M, 1, codebooks_io, M, kc, nullptr, close_out, workspace, stream);
}

int pq_train(const float *x, uint64_t ldx, uint64_t n, uint32_t d, float *codebooks_io, uint32_t M, uint32_t kc, uint32_t max_iterations,
             uint8_t *codes_out, uint32_t *iterations_out, void *workspace, hipStream_t stream) {
    CL_REQUIRE(iterations_out != nullptr, "iterations_out is NULL");
    const int rc = pq_check(x, ldx, n, d, codebooks_io, M, kc, codes_out, workspace);
    if (rc != CLEORA_OK) return rc;
    CL_REQUIRE(n * M < (1ull << 32), "n * M must stay below 2^32 (the update's member slots are 32-bit)");
    const PqPlan p = pq_plan(n, d, M, kc);
    char *ws = static_cast<char *>(workspace);
    uint32_t *frozen = reinterpret_cast<uint32_t *>(ws + p.off_frozen);
    hipLaunchKernelGGL(pq_fill_kernel, dim3(1), dim3(256), 0, stream, frozen, M, 0u);
    CL_HIP(hipGetLastError());
    uint32_t done = 0;
    while (done < max_iterations) {                                                                          // :146-165
        int e = enqueue_pq_assign(x, ldx, n, d, codebooks_io, M, kc, nullptr, nullptr, frozen, workspace, stream);
        if (e != CLEORA_OK) return e;
        e = enqueue_pq_update(x, ldx, n, d, static_cast<const uint8_t *>(workspace), 1, p.npad, codebooks_io, M, kc, frozen, nullptr,
                              workspace, stream);
        if (e != CLEORA_OK) return e;
        ++done;
        uint32_t flags[PQ_MAX_M];
        CL_HIP(hipMemcpyAsync(flags, frozen, M * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        CL_HIP(hipStreamSynchronize(stream));
        bool all = true;
        for (uint32_t m = 0; m < M; ++m) all = all && flags[m] != 0u;
        if (all) break;
    }
    const int e = enqueue_pq_assign(x, ldx, n, d, codebooks_io, M, kc, codes_out, nullptr, nullptr, workspace, stream);   // :167-173
    if (e != CLEORA_OK) return e;
    CL_HIP(hipStreamSynchronize(stream));
    *iterations_out = done;
    return CLEORA_OK;
}

uint64_t pq_search_workspace_bytes(uint64_t n, uint32_t M, uint32_t kc, uint64_t nq, uint32_t top_k) {
    (void)top_k;                                             // every list has SLIST slots
    return pq_search_plan(n, M, kc, nq).bytes;
}

int launch_pq_search(const uint8_t *codes, uint64_t n, const float *codebooks, uint32_t M, uint32_t kc, uint32_t ds, const float *queries,
                     uint64_t nq, uint32_t top_k, uint32_t *out_index, float *out_score, float *all_scores_out, void *workspace,
                     hipStream_t stream) {
    CL_REQUIRE(codes != nullptr && codebooks != nullptr && queries != nullptr && out_index != nullptr && out_score != nullptr &&
                   workspace != nullptr, "codes / codebooks / queries / out_index / out_score / workspace is NULL");
    CL_REQUIRE(ds >= 1 && ds <= PQ_MAX_DS, "the subspace width is larger than 64");
    const int rc = pq_check_shape(n, M * ds, M, kc);
    if (rc != CLEORA_OK) return rc;
    CL_REQUIRE(top_k >= 1 && top_k <= PQ_MAX_TOPK, "need 1 <= top_k <= 32");
    CL_REQUIRE((uint64_t)top_k <= n, "top_k cannot be larger than the number of rows n");
    CL_REQUIRE(nq >= 1 && nq <= (1ull << 22), "need 1 <= n_queries <= 2^22");
    const PqSearchPlan p = pq_search_plan(n, M, kc, nq);
    char *ws = static_cast<char *>(workspace);
    float *tables = reinterpret_cast<float *>(ws);
    u64 *lists = reinterpret_cast<u64 *>(ws + p.off_lists);
    hipLaunchKernelGGL(pq_table_kernel, grid_1d_as_2d(p.tiles * p.QB), dim3(256), (size_t)up((uint64_t)M * ds * 4, 16), stream, queries, nq,
                       codebooks, M, kc, ds, p.QB, tables);
    CL_HIP(hipGetLastError());

    PqScanArgs a;
    a.codes = codes;
    a.n = n;
    a.nq = nq;
    a.split_rows = p.split_rows;
    a.M = M;
    a.kc = kc;
    a.k = top_k;
    a.splits = p.splits;
    a.tables = tables;
    a.lists = lists;
    a.all_scores = all_scores_out;
    const size_t lds = (size_t)up((uint64_t)M * kc * p.QB, 4) * 4 + (size_t)p.QB * ((SLIST + SCAP) * 8 + 8 + 4);
    const dim3 blocks((unsigned)p.tiles, p.splits);
    auto go = [&](auto kernel) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) hipLaunchKernelGGL(kernel, blocks, dim3(STHREADS), lds, stream, a);
        return e;
    };
    // the widest load that M and the codes' alignment allow
    const bool al = aligned16(codes);
    const int W = (al && M % 16 == 0) ? 16 : (al && M % 8 == 0) ? 8 : (al && M % 4 == 0) ? 4 : 1;
    auto by_w = [&](auto qb) {
        constexpr int Q = decltype(qb)::value;
        return W == 16 ? go(pq_scan_kernel<Q, 16>) : W == 8 ? go(pq_scan_kernel<Q, 8>) : W == 4 ? go(pq_scan_kernel<Q, 4>) : go(pq_scan_kernel<Q, 1>);
    };
    CL_HIP(p.QB == 8 ? by_w(std::integral_constant<int, 8>()) : p.QB == 4 ? by_w(std::integral_constant<int, 4>())
                                                                          : by_w(std::integral_constant<int, 2>()));
    hipLaunchKernelGGL(pq_merge_kernel, grid_1d_as_2d(nq), dim3(64), 0, stream, lists, p.QB, p.splits, top_k, out_index, out_score);
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

int launch_pq_reconstruct(const uint8_t *codes, uint64_t n, const float *codebooks, uint32_t M, uint32_t kc, uint32_t ds, const uint32_t *rows,
                          uint64_t n_rows, float *out, uint64_t ldo, hipStream_t stream) {
    CL_REQUIRE(codes != nullptr && codebooks != nullptr && out != nullptr, "codes / codebooks / out is NULL");
    CL_REQUIRE(M >= 1 && M <= PQ_MAX_M && ds >= 1 && ds <= PQ_MAX_DS && kc >= 1 && kc <= PQ_MAX_KC,
               "need 1 <= M <= 64, 1 <= d / M <= 64, 1 <= kc <= 256");
    CL_REQUIRE(n < (1ull << 32) && n_rows < (1ull << 32), "more than 2^32 rows");
    CL_REQUIRE(ldo >= (uint64_t)M * ds, "need ldo >= d");
    if (n_rows == 0) return CLEORA_OK;
    hipLaunchKernelGGL(pq_reconstruct_kernel, grid_1d_as_2d((n_rows * M * ds + 255) / 256), dim3(256), 0, stream, codes, n, codebooks, M, kc, ds,
                       rows, n_rows, out, ldo);
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

}  // namespace cleora
