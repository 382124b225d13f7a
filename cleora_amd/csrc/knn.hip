// knn.hip — fused all-pairs cosine top-k (the kNN graph of an embedding): the scores of MANY query rows against every row of X
// on the f32 matrix cores with the selection inside the kernel.  Nothing proportional to n_queries x n is ever stored: the only
// things that leave a block are its queries' k (score, row) pairs.  Same contract as cleora_topk_cosine_dev (similarity.hip),
// which serves a batch as GEMM -> n x batch scores in HBM -> mask pass over the CSR -> selection passes -> host check.
//
//   prepare    knn_inv_norm_kernel (row_inv_norm.h, shared with kmeans.hip): 1 / max(||x_r||, 1e-10) per row (O(n) workspace,
//              padded with zeros to whole tiles);
//              knn_pack_kernel: the normalised query rows, [n_queries padded to 64][d padded to 32] (zero padding), and the
//              row index of every query slot.
//   block      512 threads = 8 waves own a tile of KQ = 64 queries and walk the candidate rows of their split in tiles of
//              KC = 128.  Wave w computes the 32 x 32 block (candidates 32 (w & 3) .., queries 32 (w >> 2) ..) of the tile with
//              v_mfma_f32_32x32x2_f32: A = candidate rows, B = query rows, one 16-register accumulator, so a lane ends up with
//              ONE query (lane & 31) and 16 candidate rows.
//   operands   X goes through LDS in chunks of 32 columns ([128][32 + 4] floats, two buffers: the chunk after the current one
//              is fetched into registers before the MFMAs of the current one and stored after them; one barrier per chunk).
//              A lane reads its fragment as one float4: columns kb + 4 (lane >> 5) .. + 3, so MFMA j of a group of four
//              multiplies the column pair (kb + j, kb + 4 + j) — the same assignment on both operands, and the row stride of
//              36 floats keeps the 16-byte reads of 8 consecutive rows on distinct banks.
//              Q: for d <= 256 the block's 64 normalised query rows stay RESIDENT in LDS for its lifetime ([64][d + 4]).
//              Wider rows: Q is re-staged with X — the same 32-column chunk of the packed queries (L2-resident, 8 KiB per
//              chunk next to X's 16 KiB) goes through a second pair of [64][36] buffers, once per (candidate tile, chunk).
//   selection  tau[q] (LDS) is query q's current k-th best, -inf until k candidates were seen.  After a tile's last chunk every
//              lane scales its accumulators by 1 / ||x_r|| and compares them with tau[q]; survivors (score >= tau: a later row
//              with an equal score wins the tie) append (score, row) to the query's LDS buffer through an LDS counter.  The 16
//              rows of a lane are handled in four steps of 4: one step adds at most 32 entries to a query (4 waves x 8 rows),
//              and after each step the waves compact every buffer that could not take another step (count > KCAP - 32).
//              Compaction (one wave per query): mask tests for the new entries, then every entry's rank under
//              (score, row index) descending by comparing it with all others; rank < k moves to slot `rank`, tau = the score of
//              rank k - 1.  The result does not depend on the order in which lanes appended.  With scores rising in the row
//              index every candidate survives and every step compacts: correct, only slow.
//   masks      the query itself: a row-index compare when a score survives.  Stored edges: tested for survivors only, at
//              compaction, before an entry can hold one of the k slots: row q of the CSR is walked once per compaction (a lane
//              per column, compared with all new entries: a hub query costs one walk per ~50 survivors, not one per
//              survivor), row r once per entry with an early exit.  Columns need not be sorted.  Masked entries keep
//              competing with score -2 like the reference's.
//   splits     with fewer query tiles than 2 blocks per CU the candidate rows are split over gridDim.y; every split writes
//              its own [query][split][k] list (padded with -inf) and knn_merge_kernel (one wave per query) selects under the
//              same order.  blockIdx.x is the query tile: the blocks that run together walk the same candidate rows.
// Deterministic: no float atomics; the only atomics are the LDS slot counters, and ranks do not depend on slots.
#include <cmath>

#include "common.h"
#include "knn_select.h"
#include "row_inv_norm.h"

namespace cleora {
namespace {

constexpr int KQ = 64;            // queries per block
constexpr int KC = 128;           // candidate rows per tile
constexpr int KK = 32;            // columns per staged chunk
constexpr int KS = KK + 4;        // LDS row stride of a staged chunk (floats)
constexpr int KD = 256;           // widest padded d whose query tile stays resident
constexpr int KSTEP = 32;         // most entries one selection step can add to a query
constexpr int KTHREADS = 512;
constexpr uint32_t KTARGET_BLOCKS = 512;     // two blocks per CU
constexpr uint32_t KSPLIT_MIN_TILES = 8;     // a split walks at least this many candidate tiles
constexpr uint32_t kKnnMaxD = 16384;
constexpr uint64_t kKnnMaxQueries = 1ull << 29;   // query tiles x 512 threads must fit the dispatch's 32-bit x extent

typedef float floatx16 __attribute__((ext_vector_type(16)));

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// One wave per query slot j: qn[j][0 .. dpad) = x[row_j] / max(||x[row_j]||, 1e-10), zeros beyond d; qrow[j] = row_j.
// Slots beyond n_queries (the padding of the last tile): a zero row and kNoRow.  A row index >= n is clamped to n - 1.
__global__ __launch_bounds__(64) void knn_pack_kernel(const float *__restrict__ x, uint64_t ldx, uint64_t n, uint32_t d, uint32_t dpad,
                                                      const uint32_t *__restrict__ queries, uint64_t nq, uint64_t nq_pad,
                                                      float *__restrict__ qn, uint32_t *__restrict__ qrow) {
    const uint64_t j = CLEORA_LINEAR_BLOCK();
    const uint32_t lane = threadIdx.x;
    if (j >= nq_pad) return;
    float *out = qn + j * dpad;
    if (j >= nq) {
        for (uint32_t c = lane; c < dpad; c += 64) out[c] = 0.0f;
        if (lane == 0) qrow[j] = kNoRow;
        return;
    }
    uint64_t r = queries ? (uint64_t)queries[j] : j;
    if (r >= n) r = n - 1;
    const float *xq = x + r * ldx;
    float sq = 0.f;
    for (uint32_t c = lane; c < d; c += 64) sq += xq[c] * xq[c];
    const float inv = 1.0f / fmaxf(sqrtf(wsum(sq)), 1e-10f);
    for (uint32_t c = lane; c < dpad; c += 64) out[c] = c < d ? xq[c] * inv : 0.0f;
    if (lane == 0) qrow[j] = (uint32_t)r;
}

// The same slots from DENSE query rows (ivf.hip's probe selection): qn[j] = queries[j] / max(||queries[j]||, 1e-10); qrow[j] = j,
// which only tells the slot from padding (the caller runs without exclude_self).
__global__ __launch_bounds__(64) void knn_pack_dense_kernel(const float *__restrict__ queries, uint64_t ldq, uint32_t d, uint32_t dpad,
                                                            uint64_t nq, uint64_t nq_pad, float *__restrict__ qn, uint32_t *__restrict__ qrow) {
    const uint64_t j = CLEORA_LINEAR_BLOCK();
    const uint32_t lane = threadIdx.x;
    if (j >= nq_pad) return;
    float *out = qn + j * dpad;
    if (j >= nq) {
        for (uint32_t c = lane; c < dpad; c += 64) out[c] = 0.0f;
        if (lane == 0) qrow[j] = kNoRow;
        return;
    }
    const float *xq = queries + j * ldq;
    float sq = 0.f;
    for (uint32_t c = lane; c < d; c += 64) sq += xq[c] * xq[c];
    const float inv = 1.0f / fmaxf(sqrtf(wsum(sq)), 1e-10f);
    for (uint32_t c = lane; c < dpad; c += 64) out[c] = c < d ? xq[c] * inv : 0.0f;
    if (lane == 0) qrow[j] = (uint32_t)j;
}

struct KnnArgs {
    const float *x;
    uint64_t ldx, n;
    uint32_t d, dpad, k, splits;
    const float *qn;           // [nq_pad][dpad]
    const uint32_t *qrow;      // [nq_pad]
    const float *inv;          // [n_pad]
    uint64_t nq, rows_per_split;
    int exclude_self;
    const uint64_t *rowptr;    // nullptr: stored edges are not masked
    const uint32_t *col;
    float *out_score;          // [nq][splits][k]
    uint32_t *out_index;
};

template <bool RESIDENT, bool VEC>
__global__ __launch_bounds__(KTHREADS) void knn_kernel(const KnnArgs a) {
    extern __shared__ float4 knn_lds[];
    float *Qs = reinterpret_cast<float *>(knn_lds);
    const uint32_t qstride = RESIDENT ? a.dpad + 4 : (uint32_t)KS;
    float *Xs = Qs + (RESIDENT ? KQ * qstride : 2 * KQ * KS);
    float *bs = Xs + 2 * KC * KS;
    uint32_t *bi = reinterpret_cast<uint32_t *>(bs + KQ * KCAP);
    float *tau = reinterpret_cast<float *>(bi + KQ * KCAP);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(tau + KQ);
    uint32_t *kept = cnt + KQ;
    uint32_t *qrow = kept + KQ;

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int cg = w & 3, qh = w >> 2, h = lane >> 5, l32 = lane & 31;
    const uint64_t q0 = (uint64_t)blockIdx.x * KQ;
    const uint64_t r_begin = (uint64_t)blockIdx.y * a.rows_per_split;
    const uint64_t r_end = r_begin + a.rows_per_split < a.n ? r_begin + a.rows_per_split : a.n;
    const uint32_t nchunks = a.dpad / KK;
    const uint32_t k = a.k;

    if (t < KQ) {
        const uint32_t qr = a.qrow[q0 + t];
        qrow[t] = qr;
        cnt[t] = 0;
        kept[t] = 0;
        tau[t] = qr == kNoRow ? INFINITY : -INFINITY;       // a padding slot takes nothing
    }
    if constexpr (RESIDENT) {
        const uint32_t w4 = a.dpad / 4;
        for (uint32_t i = t; i < KQ * w4; i += KTHREADS) {
            const uint32_t q = i / w4, c4 = i - q * w4;
            *reinterpret_cast<float4 *>(Qs + q * qstride + c4 * 4) = *reinterpret_cast<const float4 *>(a.qn + (q0 + q) * a.dpad + c4 * 4);
        }
    }

    // this thread's share of a staged chunk: two float4 of X (rows t / 8 and 64 + t / 8, columns 4 (t & 7) ..), one of Q
    const int srow = t >> 3, sc4 = (t & 7) * 4;
    float4 xr[2], qr4;
    auto fetch = [&](uint64_t base, uint32_t kc) {
        const uint32_t c = kc * KK + sc4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint64_t r = base + srow + 64 * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < r_end) {
                const float *p = a.x + r * a.ldx + c;
                if constexpr (VEC) {
                    if (c < a.d) v = *reinterpret_cast<const float4 *>(p);
                } else {
                    if (c < a.d) v.x = p[0];
                    if (c + 1 < a.d) v.y = p[1];
                    if (c + 2 < a.d) v.z = p[2];
                    if (c + 3 < a.d) v.w = p[3];
                }
            }
            xr[i] = v;
        }
        if constexpr (!RESIDENT) qr4 = *reinterpret_cast<const float4 *>(a.qn + (q0 + srow) * a.dpad + c);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<float4 *>(Xs + buf * KC * KS + (srow + 64 * i) * KS + sc4) = xr[i];
        if constexpr (!RESIDENT) *reinterpret_cast<float4 *>(Qs + buf * KQ * KS + srow * KS + sc4) = qr4;
    };

    const uint32_t q = qh * 32 + l32;                    // the query slot of this lane's accumulators
    if (r_begin < r_end) {
        fetch(r_begin, 0);
        stage(0);
    }
    __syncthreads();

    floatx16 acc;
    int buf = 0;
    for (uint64_t base = r_begin; base < r_end; base += KC) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (uint32_t kc = 0; kc < nchunks; ++kc, buf ^= 1) {
            const bool last_chunk = kc + 1 == nchunks;
            const bool has_next = !last_chunk || base + KC < r_end;
            if (has_next) fetch(last_chunk ? base + KC : base, last_chunk ? 0 : kc + 1);
            const float *xa = Xs + buf * KC * KS + (cg * 32 + l32) * KS + 4 * h;
            const float *qb = RESIDENT ? Qs + q * qstride + kc * KK + 4 * h : Qs + buf * KQ * KS + q * KS + 4 * h;
#pragma unroll
            for (int kb = 0; kb < KK; kb += 8) {
                const float4 fa = *reinterpret_cast<const float4 *>(xa + kb), fb = *reinterpret_cast<const float4 *>(qb + kb);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc, 0, 0, 0);
            }
            if (has_next) stage(buf ^ 1);
            if (last_chunk) {
                // accumulator 4 j + i of this lane: candidate row base + 32 cg + 8 j + 4 h + i, query slot q
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t rr = base + cg * 32 + 8 * j + 4 * h;
                    const float4 iv = *reinterpret_cast<const float4 *>(a.inv + rr);
                    const float ivs[4] = {iv.x, iv.y, iv.z, iv.w};
                    const float tq = tau[q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float s = acc[4 * j + i] * ivs[i];
                        if (s >= tq && rr + i < r_end) {
                            if (a.exclude_self && (uint32_t)(rr + i) == qrow[q]) s = -2.0f;
                            if (s >= tq) {
                                const uint32_t slot = atomicAdd(&cnt[q], 1u);
                                if (slot < (uint32_t)KCAP) {
                                    bs[q * KCAP + slot] = s;
                                    bi[q * KCAP + slot] = (uint32_t)(rr + i);
                                }
                            }
                        }
                    }
                    __syncthreads();
                    for (int i = 0; i < KQ / 8; ++i) {
                        const uint32_t qq = w * (KQ / 8) + i;
                        const uint32_t c = cnt[qq];
                        if (c > (uint32_t)(KCAP - KSTEP)) {
                            const uint32_t left = knn_compact(bs + qq * KCAP, bi + qq * KCAP, c < (uint32_t)KCAP ? c : (uint32_t)KCAP, kept[qq],
                                                              k, qrow[qq], a.rowptr, a.col, tau + qq, lane);
                            if (lane == 0) { cnt[qq] = left; kept[qq] = left; }
                        }
                    }
                    __syncthreads();
                }
            }
            __syncthreads();
        }
    }

    // what is left in the buffers, in order, is the result of this split
    for (int i = 0; i < KQ / 8; ++i) {
        const uint32_t qq = w * (KQ / 8) + i;
        if (q0 + qq >= a.nq) continue;
        const uint32_t c = cnt[qq];
        const uint32_t left = knn_compact(bs + qq * KCAP, bi + qq * KCAP, c < (uint32_t)KCAP ? c : (uint32_t)KCAP, kept[qq], k, qrow[qq],
                                          a.rowptr, a.col, tau + qq, lane);
        if ((uint32_t)lane < k) {
            const uint64_t o = ((q0 + qq) * a.splits + blockIdx.y) * k + lane;
            a.out_score[o] = (uint32_t)lane < left ? bs[qq * KCAP + lane] : -INFINITY;
            a.out_index[o] = (uint32_t)lane < left ? bi[qq * KCAP + lane] : 0u;
        }
    }
}

struct KnnPlan {
    uint64_t n_pad, nq_pad, qtiles, rows_per_split;
    uint32_t dpad, splits;
    uint64_t off_qrow, off_qn, off_part, bytes;
};

inline uint64_t up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

KnnPlan knn_plan(uint64_t n, uint32_t d, uint32_t k, uint64_t nq) {
    KnnPlan p;
    p.n_pad = up(n, KC);
    p.nq_pad = up(nq ? nq : 1, KQ);
    p.qtiles = p.nq_pad / KQ;
    p.dpad = (uint32_t)up(d ? d : 1, KK);
    const uint64_t tiles = p.n_pad / KC ? p.n_pad / KC : 1;
    uint64_t splits = p.qtiles >= KTARGET_BLOCKS ? 1 : (KTARGET_BLOCKS + p.qtiles - 1) / p.qtiles;
    if (splits > tiles / KSPLIT_MIN_TILES) splits = tiles / KSPLIT_MIN_TILES;
    if (splits > KMAXSPLIT) splits = KMAXSPLIT;
    if (splits < 1) splits = 1;
    const uint64_t tiles_per_split = (tiles + splits - 1) / splits;
    p.splits = (uint32_t)((tiles + tiles_per_split - 1) / tiles_per_split);      // no empty split
    p.rows_per_split = tiles_per_split * KC;
    p.off_qrow = up(p.n_pad * 4, 256);
    p.off_qn = p.off_qrow + up(p.nq_pad * 4, 256);
    p.off_part = p.off_qn + up(p.nq_pad * p.dpad * 4, 256);
    // the partial lists of any split count the plan can choose: qtiles x splits <= KTARGET_BLOCKS + qtiles
    p.bytes = p.off_part + (KTARGET_BLOCKS + p.qtiles) * KQ * (uint64_t)k * 8;
    return p;
}

}  // namespace

uint64_t knn_workspace_bytes(uint64_t n, uint32_t d, uint32_t k, uint64_t n_queries) { return knn_plan(n, d, k, n_queries).bytes; }

int launch_knn_cosine(const cleora_graph *g, const float *x, uint64_t ldx, uint64_t n, uint32_t d, const uint32_t *queries_dev,
                      uint64_t n_queries, uint32_t k, int exclude_self, int exclude_edges, uint32_t *out_index, float *out_score,
                      void *workspace, hipStream_t stream) {
    CL_REQUIRE(out_index != nullptr && out_score != nullptr, "out_index / out_score is NULL");
    CL_REQUIRE(x != nullptr && workspace != nullptr, "x / workspace is NULL");
    CL_REQUIRE(k >= 1 && k <= CLEORA_KNN_MAX_K && (uint64_t)k <= n, "need 1 <= k <= min(n, CLEORA_KNN_MAX_K = 32)");
    CL_REQUIRE(n < (1ull << 32), "more than 2^32 rows");
    CL_REQUIRE(d >= 1 && d <= kKnnMaxD && ldx >= d, "need 1 <= d <= 16384 and ldx >= d");
    CL_REQUIRE(n_queries < kKnnMaxQueries, "more than 2^29 queries in one call");
    CL_REQUIRE(!exclude_edges || (g != nullptr && g->n_rows == n && g->n_cols == n), "exclude_existing needs the square graph of X");
    if (n_queries == 0) return CLEORA_OK;
    const KnnPlan p = knn_plan(n, d, k, n_queries);
    char *ws = static_cast<char *>(workspace);
    hipLaunchKernelGGL(knn_pack_kernel, grid_1d_as_2d(p.nq_pad), dim3(64), 0, stream, x, ldx, n, d, p.dpad, queries_dev, n_queries, p.nq_pad,
                       reinterpret_cast<float *>(ws + p.off_qn), reinterpret_cast<uint32_t *>(ws + p.off_qrow));
    CL_HIP(hipGetLastError());
    return launch_knn_packed(g, x, ldx, n, d, n_queries, k, exclude_self, exclude_edges, out_index, out_score, workspace, stream);
}

KnnSlots knn_query_slots(void *workspace, uint64_t n, uint32_t d, uint32_t k, uint64_t n_queries) {
    const KnnPlan p = knn_plan(n, d, k, n_queries);
    char *ws = static_cast<char *>(workspace);
    return KnnSlots{reinterpret_cast<float *>(ws + p.off_qn), reinterpret_cast<uint32_t *>(ws + p.off_qrow), p.dpad, p.nq_pad};
}

int launch_knn_pack(const float *src, uint64_t lds, uint64_t n_src, uint32_t d, const uint32_t *rows_dev, uint64_t n_queries,
                    const KnnSlots &slots, hipStream_t stream) {
    if (rows_dev != nullptr)
        hipLaunchKernelGGL(knn_pack_kernel, grid_1d_as_2d(slots.nq_pad), dim3(64), 0, stream, src, lds, n_src, d, slots.dpad, rows_dev,
                           n_queries, slots.nq_pad, slots.qn, slots.qrow);
    else
        hipLaunchKernelGGL(knn_pack_dense_kernel, grid_1d_as_2d(slots.nq_pad), dim3(64), 0, stream, src, lds, d, slots.dpad, n_queries,
                           slots.nq_pad, slots.qn, slots.qrow);
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

int launch_knn_packed(const cleora_graph *g, const float *x, uint64_t ldx, uint64_t n, uint32_t d, uint64_t n_queries, uint32_t k,
                      int exclude_self, int exclude_edges, uint32_t *out_index, float *out_score, void *workspace, hipStream_t stream) {
    const KnnPlan p = knn_plan(n, d, k, n_queries);
    char *ws = static_cast<char *>(workspace);
    float *inv = reinterpret_cast<float *>(ws);
    uint32_t *qrow = reinterpret_cast<uint32_t *>(ws + p.off_qrow);
    float *qn = reinterpret_cast<float *>(ws + p.off_qn);
    float *part_score = reinterpret_cast<float *>(ws + p.off_part);
    uint32_t *part_index = reinterpret_cast<uint32_t *>(part_score + n_queries * p.splits * k);

    launch_row_inv_norm(x, ldx, n, p.n_pad, d, inv, stream);
    CL_HIP(hipGetLastError());

    KnnArgs a;
    a.x = x;
    a.ldx = ldx;
    a.n = n;
    a.d = d;
    a.dpad = p.dpad;
    a.k = k;
    a.splits = p.splits;
    a.qn = qn;
    a.qrow = qrow;
    a.inv = inv;
    a.nq = n_queries;
    a.rows_per_split = p.rows_per_split;
    a.exclude_self = exclude_self ? 1 : 0;
    a.rowptr = exclude_edges ? g->rowptr : nullptr;
    a.col = exclude_edges ? g->col : nullptr;
    a.out_score = p.splits > 1 ? part_score : out_score;
    a.out_index = p.splits > 1 ? part_index : out_index;
    const bool resident = p.dpad <= (uint32_t)KD;
    const bool vec = d % 4 == 0 && ldx % 4 == 0 && aligned16(x);
    const size_t lds = ((resident ? (size_t)KQ * (p.dpad + 4) : (size_t)2 * KQ * KS) + (size_t)2 * KC * KS + (size_t)2 * KQ * KCAP + 4 * KQ) * 4;
    const dim3 blocks((unsigned)p.qtiles, p.splits);
    auto go = [&](auto kernel) {
        // per DEVICE and cheap: set on every call
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) hipLaunchKernelGGL(kernel, blocks, dim3(KTHREADS), lds, stream, a);
        return e;
    };
    CL_HIP(resident ? (vec ? go(knn_kernel<true, true>) : go(knn_kernel<true, false>))
                    : (vec ? go(knn_kernel<false, true>) : go(knn_kernel<false, false>)));
    CL_HIP(hipGetLastError());
    if (p.splits > 1) {
        hipLaunchKernelGGL(knn_merge_kernel, grid_1d_as_2d(n_queries), dim3(64), 0, stream, part_score, part_index, n_queries, p.splits, k,
                           0u, out_score, out_index);
        CL_HIP(hipGetLastError());
    }
    return CLEORA_OK;
}

}  // namespace cleora
