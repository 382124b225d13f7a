// ivf.hip — approximate cosine kNN through an inverted-file (IVF) index: the rows are grouped into nlist lists by a coarse quantiser
// (the labels and unit centroids of kmeans.hip), a query probes the nprobe lists whose centroids are nearest and its result is the
// top k over the union of those lists.  A list is read once per TILE OF 64 QUERIES that probe it, not once per query.
//
//   build      the ordered member lists of member_lists.h (shared with kmeans.hip's update) -> list_rows: every list's rows in
//              ascending row order; list_ptr = their offsets.  ivf_layout_kernel (one wave per slot) copies the rows in that order
//              into xs, each scaled by 1 / max(||x_r||, 1e-10) and zero-padded to dpad = d rounded up to 32 columns; every list
//              starts on a tile of IC = 128 slots and its last tile is filled with zero rows, so the scan fetches whole tiles with
//              no bounds test (at most 127 padding slots per list: n / 128 + nlist tiles in all).
//   search     per batch of queries (the partial lists bound the batch: ivf_search_workspace_bytes):
//     probes   the queries are packed like knn.hip's ([64-padded][dpad], normalised) and knn.hip's own scan runs with the centroids
//              as candidates and k = nprobe (launch_knn_packed): probes[q][0 .. nprobe).
//     group    the (query, probe slot) pairs are regrouped by list with member_lists.h once more — the pairs are the "rows", the
//              probed list is the "label": a counting sort whose scatter is in ascending pair order, so pairs[] depends on the input
//              alone.  The label is the list's RANK by length (ivf_order_kernel: longest first, ties to the lower list), and the
//              chunk offsets of member_lists.h with chunks of 64 pairs are the work-item table: item_off[rank] = first item of that
//              list, one item per (list, tile of <= 64 probing queries).  Items of the longest lists have the lowest indices and
//              start first.  The number of items is only known on the device: the grid is launched at its bound,
//              ceil(pairs / 64) + nlist, a block finds its (list, tile) by a binary search in item_off and surplus blocks exit.
//     scan     ivf_scan_kernel, 512 threads = 8 waves per item: gathers the item's <= 64 packed query rows into LDS (resident for
//              dpad <= 256: [64][dpad + 4]; wider rows re-staged in 32-column chunks next to the list's rows, as knn.hip does),
//              streams the list's tiles of 128 rows through a double-buffered [128][36] LDS stage onto v_mfma_f32_32x32x2_f32
//              (wave w: rows 32 (w & 3) .. x queries 32 (w >> 2) .., one 16-register accumulator; fragments one float4 per operand
//              per four MFMAs) and selects in the kernel with knn.hip's scheme: tau per query, survivors (score >= tau) appended
//              to the query's LDS buffer with their ORIGINAL row index (list_rows, read for survivors only), compaction by rank
//              under (score, original row) descending (knn_select.h).  The rows are unit length: the accumulator is the score.
//              exclude_self: an index compare on survivors (the own row keeps competing with -2, as in knn.hip).  The k best go
//              to part[query][probe slot][k], padded with (-inf, 0xffffffff).
//     merge    knn_select.h's merge, one wave per query over its nprobe lists of k.
// Deterministic: no floating-point atomics; integer atomics only for counts and LDS slot counters, and nothing depends on slots.
#include <cmath>

#include "common.h"
#include "knn_select.h"
#include "member_lists.h"
#include "row_inv_norm.h"

namespace cleora {
namespace {

constexpr int IQ = 64;            // queries per work item
constexpr int IC = 128;           // list rows per tile
constexpr int IK = 32;            // columns per staged chunk
constexpr int IS = IK + 4;        // LDS row stride of a staged chunk (floats)
constexpr int ID = 256;           // widest padded d whose query tile stays resident
constexpr int ISTEP = 32;         // most entries one selection step can add to a query
constexpr int ITHREADS = 512;
constexpr uint32_t kIvfMaxD = 16384;
constexpr uint64_t kIvfMaxQueries = 1ull << 29;
// Queries per batch: bounds the partial lists (batch x nprobe x k x 8 bytes: 1 GiB at 32 x 32, 84 MB at 8 x 10) and the pairs of one
// grouping (batch x nprobe <= 2^22 < 2^32).  Larger batches only make query tiles fuller: at 131072 queries and 4096 lists a list
// is probed by 32 nprobe queries on average.
constexpr uint64_t kIvfBatch = 131072;

typedef float floatx16 __attribute__((ext_vector_type(16)));

inline uint64_t up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// ----------------------------------------------------------------------------------------------------------------- build

__global__ __launch_bounds__(256) void ivf_list_ptr_kernel(const uint32_t *__restrict__ coff, uint32_t nlist, uint64_t *__restrict__ list_ptr) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c <= nlist) list_ptr[c] = coff[c];
}

// One wave per slot s of xs: tile s / IC belongs to the last list c with choff[c] <= tile (empty lists have no tile); slots beyond the
// list's members are zero rows.  Slots beyond the last list's tiles are never read and stay unwritten.
__global__ __launch_bounds__(256) void ivf_layout_kernel(const float *__restrict__ x, uint64_t ldx, uint32_t d, uint32_t dpad, uint32_t nlist,
                                                         const uint32_t *__restrict__ coff, const uint32_t *__restrict__ choff,
                                                         const uint32_t *__restrict__ members, float *__restrict__ xs) {
    const uint64_t s = CLEORA_LINEAR_BLOCK() * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = s / IC;
    if (tile >= choff[nlist]) return;
    uint32_t lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (choff[mid] <= tile) lo = mid; else hi = mid;
    }
    const uint32_t pos = ((uint32_t)tile - choff[lo]) * IC + (uint32_t)(s % IC);
    float *out = xs + s * dpad;
    if (pos >= coff[lo + 1] - coff[lo]) {
        for (uint32_t c = lane; c < dpad; c += 64) out[c] = 0.0f;
        return;
    }
    const float *xr = x + (uint64_t)members[coff[lo] + pos] * ldx;
    float sq = 0.f;
    for (uint32_t c = lane; c < d; c += 64) sq += xr[c] * xr[c];
    const float inv = 1.0f / fmaxf(sqrtf(wsum(sq)), 1e-10f);
    for (uint32_t c = lane; c < dpad; c += 64) out[c] = c < d ? xr[c] * inv : 0.0f;
}

// ---------------------------------------------------------------------------------------------------------------- search

// One thread per list c: rank[c] = lists that come before it (longer, or as long with a lower index), order[rank] = c,
// tile_off[c] = tiles of xs before list c.
__global__ __launch_bounds__(256) void ivf_order_kernel(const uint64_t *__restrict__ list_ptr, uint32_t nlist, uint32_t *__restrict__ rank,
                                                        uint32_t *__restrict__ order, uint32_t *__restrict__ tile_off) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nlist) return;
    const uint64_t len = list_ptr[c + 1] - list_ptr[c];
    uint32_t before = 0, tiles = 0;
    for (uint32_t o = 0; o < nlist; ++o) {
        const uint64_t lo = list_ptr[o + 1] - list_ptr[o];
        before += (lo > len || (lo == len && o < c)) ? 1u : 0u;
        tiles += o < c ? (uint32_t)((lo + IC - 1) / IC) : 0u;
    }
    rank[c] = before;
    order[before] = c;
    tile_off[c] = tiles;
}

// ranked[i] = rank of the list that pair i = (query i / nprobe, slot i % nprobe) probes; the probes themselves to probes_out.
__global__ __launch_bounds__(256) void ivf_rank_pairs_kernel(const uint32_t *__restrict__ probes, uint64_t pairs, uint32_t nlist,
                                                             const uint32_t *__restrict__ rank, uint32_t *__restrict__ ranked,
                                                             uint32_t *__restrict__ probes_out) {
    const uint64_t i = CLEORA_LINEAR_BLOCK() * 256 + threadIdx.x;
    if (i >= pairs) return;
    const uint32_t c = probes[i];
    ranked[i] = c < nlist ? rank[c] : kNoLabel;
    if (probes_out != nullptr) probes_out[i] = c;
}

struct IvfScanArgs {
    const float *xs;               // [tiles x IC][dpad]
    const uint64_t *list_ptr;      // [nlist + 1]
    const uint32_t *list_rows;     // original row of every list member
    const uint32_t *tile_off;      // [nlist] first tile of a list
    const uint32_t *order;         // [nlist] rank -> list
    const uint32_t *pair_off;      // [nlist + 1] by rank: first pair of the list in pairs[]
    const uint32_t *item_off;      // [nlist + 1] by rank: first work item of the list
    const uint32_t *pairs;         // pair ids (query x nprobe + slot) grouped by list rank, ascending within a list
    const float *qn;               // [batch padded][dpad] packed queries
    const uint32_t *qrow;          // their original rows
    uint32_t dpad, k, nprobe, nlist;
    int exclude_self;
    float *part_score;             // [batch][nprobe][k]
    uint32_t *part_index;
};

template <bool RESIDENT>
__global__ __launch_bounds__(ITHREADS) void ivf_scan_kernel(const IvfScanArgs a) {
    extern __shared__ float4 ivf_lds[];
    float *Qs = reinterpret_cast<float *>(ivf_lds);
    const uint32_t qstride = RESIDENT ? a.dpad + 4 : (uint32_t)IS;
    float *Xs = Qs + (RESIDENT ? IQ * qstride : 2 * IQ * IS);
    float *bs = Xs + 2 * IC * IS;
    uint32_t *bi = reinterpret_cast<uint32_t *>(bs + IQ * KCAP);
    float *tau = reinterpret_cast<float *>(bi + IQ * KCAP);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(tau + IQ);
    uint32_t *kept = cnt + IQ;
    uint32_t *qrow = kept + IQ;
    uint32_t *qpair = qrow + IQ;

    // the work item of this block: list order[lo], its (item - item_off[lo])-th tile of probing queries
    const uint64_t item = CLEORA_LINEAR_BLOCK();
    if (item >= a.item_off[a.nlist]) return;
    uint32_t lo = 0, hi = a.nlist;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (a.item_off[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t list = a.order[lo];
    const uint32_t first = a.pair_off[lo] + ((uint32_t)item - a.item_off[lo]) * IQ;
    const uint32_t left = a.pair_off[lo + 1] - first;
    const uint32_t nq_here = left < (uint32_t)IQ ? left : (uint32_t)IQ;
    const uint64_t row0 = a.list_ptr[list];
    const uint32_t len = (uint32_t)(a.list_ptr[list + 1] - row0);
    const float *xl = a.xs + (uint64_t)a.tile_off[list] * IC * a.dpad;

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int cg = w & 3, qh = w >> 2, h = lane >> 5, l32 = lane & 31;
    const uint32_t nchunks = a.dpad / IK;
    const uint32_t k = a.k;

    if (t < IQ) {
        uint32_t pair = kNoRow, qr = kNoRow;
        if ((uint32_t)t < nq_here) {
            pair = a.pairs[first + t];
            qr = a.qrow[pair / a.nprobe];
        }
        qpair[t] = pair;
        qrow[t] = qr;
        cnt[t] = 0;
        kept[t] = 0;
        tau[t] = pair == kNoRow ? INFINITY : -INFINITY;       // a padding slot takes nothing
    }
    __syncthreads();
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (RESIDENT) {
        const uint32_t w4 = a.dpad / 4;
        for (uint32_t i = t; i < IQ * w4; i += ITHREADS) {
            const uint32_t q = i / w4, c4 = i - q * w4;
            const uint32_t pair = qpair[q];
            *reinterpret_cast<float4 *>(Qs + q * qstride + c4 * 4) =
                pair != kNoRow ? *reinterpret_cast<const float4 *>(a.qn + (uint64_t)(pair / a.nprobe) * a.dpad + c4 * 4) : zero4;
        }
    }

    // this thread's share of a staged chunk: two float4 of the list (slots t / 8 and 64 + t / 8, columns 4 (t & 7) ..), one of Q
    const int srow = t >> 3, sc4 = (t & 7) * 4;
    const uint32_t spair = qpair[srow];
    const float *qsrc = spair != kNoRow ? a.qn + (uint64_t)(spair / a.nprobe) * a.dpad : nullptr;
    float4 xr[2], qr4 = zero4;
    auto fetch = [&](uint32_t base, uint32_t kc) {
        const uint32_t c = kc * IK + sc4;
#pragma unroll
        for (int i = 0; i < 2; ++i) xr[i] = *reinterpret_cast<const float4 *>(xl + (uint64_t)(base + srow + 64 * i) * a.dpad + c);
        if constexpr (!RESIDENT) qr4 = qsrc != nullptr ? *reinterpret_cast<const float4 *>(qsrc + c) : zero4;
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<float4 *>(Xs + buf * IC * IS + (srow + 64 * i) * IS + sc4) = xr[i];
        if constexpr (!RESIDENT) *reinterpret_cast<float4 *>(Qs + buf * IQ * IS + srow * IS + sc4) = qr4;
    };

    const uint32_t q = qh * 32 + l32;                    // the query slot of this lane's accumulators
    if (len > 0) {
        fetch(0, 0);
        stage(0);
    }
    __syncthreads();

    floatx16 acc;
    int buf = 0;
    for (uint32_t base = 0; base < len; base += IC) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (uint32_t kc = 0; kc < nchunks; ++kc, buf ^= 1) {
            const bool last_chunk = kc + 1 == nchunks;
            const bool has_next = !last_chunk || base + IC < len;
            if (has_next) fetch(last_chunk ? base + IC : base, last_chunk ? 0 : kc + 1);
            const float *xa = Xs + buf * IC * IS + (cg * 32 + l32) * IS + 4 * h;
            const float *qb = RESIDENT ? Qs + q * qstride + kc * IK + 4 * h : Qs + buf * IQ * IS + q * IS + 4 * h;
#pragma unroll
            for (int kb = 0; kb < IK; kb += 8) {
                const float4 fa = *reinterpret_cast<const float4 *>(xa + kb), fb = *reinterpret_cast<const float4 *>(qb + kb);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc, 0, 0, 0);
            }
            if (has_next) stage(buf ^ 1);
            if (last_chunk) {
                // accumulator 4 j + i of this lane: list slot base + 32 cg + 8 j + 4 h + i, query slot q
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t rr = base + cg * 32 + 8 * j + 4 * h;
                    const float tq = tau[q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float s = acc[4 * j + i];
                        if (s >= tq && rr + i < len) {
                            const uint32_t orig = a.list_rows[row0 + rr + i];
                            if (a.exclude_self && orig == qrow[q]) s = -2.0f;
                            if (s >= tq) {
                                const uint32_t slot = atomicAdd(&cnt[q], 1u);
                                if (slot < (uint32_t)KCAP) {
                                    bs[q * KCAP + slot] = s;
                                    bi[q * KCAP + slot] = orig;
                                }
                            }
                        }
                    }
                    __syncthreads();
                    for (int i = 0; i < IQ / 8; ++i) {
                        const uint32_t qq = w * (IQ / 8) + i;
                        const uint32_t c = cnt[qq];
                        if (c > (uint32_t)(KCAP - ISTEP)) {
                            const uint32_t now = knn_compact(bs + qq * KCAP, bi + qq * KCAP, c < (uint32_t)KCAP ? c : (uint32_t)KCAP, kept[qq],
                                                             k, qrow[qq], nullptr, nullptr, tau + qq, lane);
                            if (lane == 0) { cnt[qq] = now; kept[qq] = now; }
                        }
                    }
                    __syncthreads();
                }
            }
            __syncthreads();
        }
    }

    // what is left in the buffers, in order, is this list's answer to the pair
    for (int i = 0; i < IQ / 8; ++i) {
        const uint32_t qq = w * (IQ / 8) + i;
        if (qq >= nq_here) continue;
        const uint32_t c = cnt[qq];
        const uint32_t now = knn_compact(bs + qq * KCAP, bi + qq * KCAP, c < (uint32_t)KCAP ? c : (uint32_t)KCAP, kept[qq], k, qrow[qq], nullptr,
                                         nullptr, tau + qq, lane);
        if ((uint32_t)lane < k) {
            const uint64_t o = (uint64_t)qpair[qq] * k + lane;
            a.part_score[o] = (uint32_t)lane < now ? bs[qq * KCAP + lane] : -INFINITY;
            a.part_index[o] = (uint32_t)lane < now ? bi[qq * KCAP + lane] : kNoRow;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host

inline uint64_t ivf_tiles_bound(uint64_t n, uint32_t nlist) { return (n + IC - 1) / IC + nlist; }   // sum of ceil(len / IC) is at most this

struct IvfBuildPlan {
    uint64_t off_count, off_coff, off_choff, bytes;      // [0, ..): the segment table
};

IvfBuildPlan ivf_build_plan(uint64_t n, uint32_t nlist) {
    IvfBuildPlan p;
    p.off_count = up(member_segs(n).segs_bound * nlist * 4, 256);
    p.off_coff = p.off_count + up((uint64_t)nlist * 4, 256);
    p.off_choff = p.off_coff + up(((uint64_t)nlist + 1) * 4, 256);
    p.bytes = p.off_choff + up(((uint64_t)nlist + 1) * 4, 256);
    return p;
}

struct IvfSearchPlan {
    uint64_t batch;
    uint64_t off_probes, off_pscore, off_ranked, off_pairs, off_table, off_count, off_coff, off_choff, off_rank, off_order, off_tile,
        off_part, bytes;                                 // [0, ..): the probe selection's knn workspace
};

IvfSearchPlan ivf_search_plan(uint32_t d, uint32_t nlist, uint32_t nprobe, uint32_t k, uint64_t n_queries) {
    IvfSearchPlan p;
    p.batch = up(n_queries ? n_queries : 1, IQ);
    if (p.batch > kIvfBatch) p.batch = kIvfBatch;
    const uint64_t pairs = p.batch * nprobe, lists = up(((uint64_t)nlist + 1) * 4, 256);
    p.off_probes = up(knn_workspace_bytes(nlist, d, nprobe, p.batch), 256);
    p.off_pscore = p.off_probes + up(pairs * 4, 256);
    p.off_ranked = p.off_pscore + up(pairs * 4, 256);
    p.off_pairs = p.off_ranked + up(pairs * 4, 256);
    p.off_table = p.off_pairs + up(pairs * 4, 256);
    p.off_count = p.off_table + up(member_segs(pairs).segs_bound * nlist * 4, 256);
    p.off_coff = p.off_count + lists;
    p.off_choff = p.off_coff + lists;
    p.off_rank = p.off_choff + lists;
    p.off_order = p.off_rank + lists;
    p.off_tile = p.off_order + lists;
    p.off_part = p.off_tile + lists;
    p.bytes = p.off_part + pairs * k * 8;
    return p;
}

int ivf_check(uint64_t n, uint32_t d, uint64_t ldx, uint32_t nlist) {
    CL_REQUIRE(nlist >= 2, "nlist must be at least 2");
    CL_REQUIRE(nlist <= CLEORA_KMEANS_MAX_K, "nlist is larger than CLEORA_KMEANS_MAX_K = 4096");
    CL_REQUIRE((uint64_t)nlist <= n, "nlist cannot be larger than the number of rows n");
    CL_REQUIRE(n < (1ull << 32), "more than 2^32 rows");
    CL_REQUIRE(d >= 1 && d <= kIvfMaxD, "need 1 <= d <= 16384");
    CL_REQUIRE(ldx >= d, "need ldx >= d");
    return CLEORA_OK;
}

}  // namespace

uint64_t ivf_xs_bytes(uint64_t n, uint32_t d, uint32_t nlist) { return ivf_tiles_bound(n, nlist) * IC * up(d ? d : 1, IK) * 4; }

uint64_t ivf_build_workspace_bytes(uint64_t n, uint32_t nlist) { return ivf_build_plan(n, nlist).bytes; }

int launch_ivf_build(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const uint32_t *labels, uint32_t nlist, uint64_t *list_ptr,
                     uint32_t *list_rows, float *xs, void *workspace, hipStream_t stream) {
    CL_REQUIRE(x != nullptr && labels != nullptr && list_ptr != nullptr && list_rows != nullptr && xs != nullptr && workspace != nullptr,
               "x / labels / list_ptr / list_rows / xs / workspace is NULL");
    const int rc = ivf_check(n, d, ldx, nlist);
    if (rc != CLEORA_OK) return rc;
    CL_REQUIRE(aligned16(xs), "xs must be 16-byte aligned");
    const IvfBuildPlan p = ivf_build_plan(n, nlist);
    char *ws = static_cast<char *>(workspace);
    uint32_t *table = reinterpret_cast<uint32_t *>(ws), *count = reinterpret_cast<uint32_t *>(ws + p.off_count);
    uint32_t *coff = reinterpret_cast<uint32_t *>(ws + p.off_coff), *choff = reinterpret_cast<uint32_t *>(ws + p.off_choff);
    enqueue_member_lists<IC>(labels, n, nlist, table, count, coff, choff, list_rows, stream);
    hipLaunchKernelGGL(ivf_list_ptr_kernel, dim3(nlist / 256 + 1), dim3(256), 0, stream, coff, nlist, list_ptr);
    CL_HIP(hipGetLastError());
    const uint32_t dpad = (uint32_t)up(d, IK);
    hipLaunchKernelGGL(ivf_layout_kernel, grid_1d_as_2d(ivf_tiles_bound(n, nlist) * IC / 4), dim3(256), 0, stream, x, ldx, d, dpad, nlist, coff,
                       choff, list_rows, xs);
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

uint64_t ivf_search_workspace_bytes(uint64_t n, uint32_t d, uint32_t nlist, uint32_t nprobe, uint32_t k, uint64_t n_queries) {
    (void)n;    // the search reads the index and never anything proportional to n of its own
    return ivf_search_plan(d, nlist, nprobe, k, n_queries).bytes;
}

int launch_ivf_search(const uint64_t *list_ptr, const uint32_t *list_rows, const float *xs, const float *x, uint64_t ldx, uint64_t n,
                      uint32_t d, const float *centroids, uint32_t nlist, const float *queries, const uint32_t *query_rows,
                      uint64_t n_queries, uint32_t nprobe, uint32_t k, int exclude_self, uint32_t *out_index, float *out_score,
                      uint32_t *probes_out, void *workspace, uint64_t workspace_queries, hipStream_t stream) {
    CL_REQUIRE(out_index != nullptr && out_score != nullptr, "out_index / out_score is NULL");
    CL_REQUIRE(list_ptr != nullptr && list_rows != nullptr && xs != nullptr && centroids != nullptr && workspace != nullptr,
               "list_ptr / list_rows / xs / centroids / workspace is NULL");
    const int rc = ivf_check(n, d, ldx, nlist);
    if (rc != CLEORA_OK) return rc;
    CL_REQUIRE(nprobe >= 1 && nprobe <= nlist && nprobe <= CLEORA_KNN_MAX_K, "need 1 <= nprobe <= min(nlist, 32)");
    CL_REQUIRE(k >= 1 && k <= CLEORA_KNN_MAX_K, "need 1 <= k <= CLEORA_KNN_MAX_K = 32");
    CL_REQUIRE((queries != nullptr) != (query_rows != nullptr), "exactly one of queries / query_rows must be given");
    CL_REQUIRE(query_rows == nullptr || x != nullptr, "query_rows needs x");
    CL_REQUIRE(queries == nullptr || !exclude_self, "exclude_self needs query_rows");
    CL_REQUIRE(n_queries < kIvfMaxQueries, "more than 2^29 queries in one call");
    CL_REQUIRE(aligned16(xs), "xs must be 16-byte aligned");
    if (n_queries == 0) return CLEORA_OK;

    const IvfSearchPlan p = ivf_search_plan(d, nlist, nprobe, k, workspace_queries ? workspace_queries : n_queries);
    char *ws = static_cast<char *>(workspace);
    auto u32 = [&](uint64_t off) { return reinterpret_cast<uint32_t *>(ws + off); };
    uint32_t *probes = u32(p.off_probes), *ranked = u32(p.off_ranked), *pairs = u32(p.off_pairs), *table = u32(p.off_table);
    uint32_t *count = u32(p.off_count), *coff = u32(p.off_coff), *choff = u32(p.off_choff), *rank = u32(p.off_rank);
    uint32_t *order = u32(p.off_order), *tile_off = u32(p.off_tile);
    float *pscore = reinterpret_cast<float *>(ws + p.off_pscore), *part_score = reinterpret_cast<float *>(ws + p.off_part);
    const uint32_t dpad = (uint32_t)up(d, IK);
    const bool resident = dpad <= (uint32_t)ID;
    const size_t lds = ((resident ? (size_t)IQ * (dpad + 4) : (size_t)2 * IQ * IS) + (size_t)2 * IC * IS + (size_t)2 * IQ * KCAP + 5 * IQ) * 4;

    hipLaunchKernelGGL(ivf_order_kernel, dim3((nlist + 255) / 256), dim3(256), 0, stream, list_ptr, nlist, rank, order, tile_off);
    CL_HIP(hipGetLastError());
    for (uint64_t base = 0; base < n_queries; base += p.batch) {
        const uint64_t nqb = n_queries - base < p.batch ? n_queries - base : p.batch, npairs = nqb * nprobe;
        // probe selection: the centroids as the candidates of knn.hip's scan
        const KnnSlots slots = knn_query_slots(workspace, nlist, d, nprobe, nqb);
        int e = queries != nullptr ? launch_knn_pack(queries + base * d, d, nqb, d, nullptr, nqb, slots, stream)
                                   : launch_knn_pack(x, ldx, n, d, query_rows + base, nqb, slots, stream);
        if (e != CLEORA_OK) return e;
        e = launch_knn_packed(nullptr, centroids, d, nlist, d, nqb, nprobe, 0, 0, probes, pscore, workspace, stream);
        if (e != CLEORA_OK) return e;
        // grouping: pairs by the rank of their list, work items of 64 pairs
        hipLaunchKernelGGL(ivf_rank_pairs_kernel, grid_1d_as_2d((npairs + 255) / 256), dim3(256), 0, stream, probes, npairs, nlist, rank, ranked,
                           probes_out != nullptr ? probes_out + base * nprobe : nullptr);
        enqueue_member_lists<IQ>(ranked, npairs, nlist, table, count, coff, choff, pairs, stream);
        CL_HIP(hipGetLastError());

        IvfScanArgs a;
        a.xs = xs;
        a.list_ptr = list_ptr;
        a.list_rows = list_rows;
        a.tile_off = tile_off;
        a.order = order;
        a.pair_off = coff;
        a.item_off = choff;
        a.pairs = pairs;
        a.qn = slots.qn;
        a.qrow = slots.qrow;
        a.dpad = dpad;
        a.k = k;
        a.nprobe = nprobe;
        a.nlist = nlist;
        a.exclude_self = exclude_self ? 1 : 0;
        a.part_score = part_score;
        a.part_index = reinterpret_cast<uint32_t *>(part_score + npairs * k);
        const dim3 blocks = grid_1d_as_2d((npairs + IQ - 1) / IQ + nlist);      // the bound on the number of work items
        auto go = [&](auto kernel) {
            // per DEVICE and cheap: set on every call
            const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (err == hipSuccess) hipLaunchKernelGGL(kernel, blocks, dim3(ITHREADS), lds, stream, a);
            return err;
        };
        CL_HIP(resident ? go(ivf_scan_kernel<true>) : go(ivf_scan_kernel<false>));
        CL_HIP(hipGetLastError());
        hipLaunchKernelGGL(knn_merge_kernel, grid_1d_as_2d(nqb), dim3(64), 0, stream, part_score, a.part_index, nqb, nprobe, k, kNoRow,
                           out_score + base * k, out_index + base * k);
        CL_HIP(hipGetLastError());
    }
    return CLEORA_OK;
}

}  // namespace cleora
