// kmeans.hip — spherical k-means of an embedding on the device (pycleora/community.py:5-48): a fused assign kernel and an
// order-fixed update.  Nothing proportional to n x k is ever stored; one iteration reads back 8 bytes.
//
//   assign     label[r] = argmax_c x_r . c_c over k unit centroids, ties to the LOWER centroid index (numpy's argmax).
//     prepare  kmeans_pack_kernel: the centroids as [k padded to 128][d padded to 32] with zero padding (tens of KiB to a few MiB:
//              every block re-reads them from L2), and the changed count cleared.
//     block    256 threads = 4 waves own a tile of MR = 64 rows of X and let every centroid stream past it in tiles of MC = 128.
//              Wave w computes rows 32 (w & 1) .. of the tile against centroids 64 (w >> 1) .. of the centroid tile with
//              v_mfma_f32_32x32x2_f32 into TWO 16-register accumulators (centroids .. + 31 and + 32 .. + 63): A = centroid rows,
//              B = X rows, so the B fragment is read once for two MFMAs and a lane ends up with ONE X row (lane & 31) and 32
//              centroids.  Why 64 x 128 and not the 128- or 256-row tile of knn.hip's closing note: the resident X tile of
//              d = 256 is 65 KiB for 64 rows; 128 rows (130 KiB) leave no room for a 128-centroid double-buffered stage, and the
//              second accumulator is what that note asks for — it comes from the centroid side here.
//     operands for d <= 256 the X tile stays RESIDENT in LDS ([64][d + 4] floats, rows beyond n and columns beyond d zero); wider rows
//              are re-staged in 32-column chunks beside the centroids ([64][36], two buffers).  The centroids go through
//              [128][32 + 4] floats, two buffers: the chunk after the current one is fetched into registers before the MFMAs of the
//              current one and stored after them, one barrier per chunk.  Fragments are one float4 per operand per four MFMAs
//              (columns kb + 4 (lane >> 5) .. + 3 — the same assignment on both operands, as in knn.hip).
//     arg-max  every lane keeps ONE running (best score, best index) over its 32 accumulator entries per tile, visited in ascending
//              centroid index with a strict >, so the lowest index of equal scores stays.  Padding centroids are skipped by index
//              (c < k), never by score.  After the last tile the four lanes that share an X row (2 waves x 2 lane halves) meet in
//              LDS and one thread per row picks under (score descending, index ascending), compares with the previous label,
//              writes label and cosine (score / max(||x_r||, 1e-10)); padding rows are never written.  The changed count is one
//              integer atomic per block.  X is not normalised for the arg-max: ||x_r|| > 0 scales a row's scores alike, a zero row
//              scores 0 everywhere and takes label 0.
//   update     centroid_c = normalise(mean over members of x_r / max(||x_r||, 1e-10)), in f64, in an order that depends only on
//              (labels, n, k, d); count, scan and place are member_lists.h (shared with ivf.hip):
//     count    the rows are cut into at most 512 segments of consecutive rows; one wave per segment counts its labels in LDS
//              (integer atomics) -> table[segment][cluster];
//     scan     per cluster over the segments (exclusive, in place), then over the clusters: coff[c] = first member slot of
//              cluster c, choff[c] = first CHUNK (256 members) of cluster c;
//     place    one wave per segment walks its rows 64 at a time in row order; a lane's slot is its cluster's cursor plus the
//              number of lower lanes with the same label: members[] holds every cluster's rows in ASCENDING row order;
//     sum      one 256-thread block per (chunk, 256-column slab): a thread owns a column and adds its chunk's members in member
//              order -> part[chunk][d] (f64);
//     finish   one block per cluster adds the chunk partials in chunk order, divides by the count, takes the norm with a fixed
//              tree, and rounds mean / norm to f32 once.  No members, or a norm <= 1e-10: the old centroid is not touched.
//              Labels >= k belong to no cluster.
// Deterministic: no floating-point atomics anywhere in this file; integer atomics only for counts.
#include <cmath>

#include "common.h"
#include "member_lists.h"
#include "row_inv_norm.h"

namespace cleora {
namespace {

constexpr int MR = 64;            // rows of X per block
constexpr int MC = 128;           // centroids per streamed tile
constexpr int MK = 32;            // columns per staged chunk
constexpr int MS = MK + 4;        // LDS row stride of a staged chunk (floats)
constexpr int MD = 256;           // widest padded d whose X tile stays resident
constexpr int MTHREADS = 256;
constexpr uint32_t kKmeansMaxD = 16384;
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t UCHUNK = 256;          // members per chunk of the update's sum
constexpr uint32_t USLAB = 256;           // columns per slab = threads per block of the sum

typedef float floatx16 __attribute__((ext_vector_type(16)));

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline uint64_t up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------------------------------------------------------- assign

// One wave per centroid slot j < kpad: cp[j][0 .. dpad) = centroids[j] (zeros beyond d and beyond k).  Also clears the changed count.
__global__ __launch_bounds__(64) void kmeans_pack_kernel(const float *__restrict__ cent, uint32_t k, uint32_t d, uint32_t dpad,
                                                         float *__restrict__ cp, unsigned long long *__restrict__ changed) {
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    float *out = cp + (uint64_t)j * dpad;
    const float *in = cent + (uint64_t)j * d;
    for (uint32_t c = lane; c < dpad; c += 64) out[c] = (j < k && c < d) ? in[c] : 0.0f;
    if (j == 0 && lane == 0 && changed != nullptr) *changed = 0ull;
}

struct AssignArgs {
    const float *x;
    uint64_t ldx, n;
    uint32_t d, dpad, k, kpad;
    const float *cp;               // [kpad][dpad]
    const float *inv;              // [n]; only read when cosine != nullptr
    uint32_t *labels;              // [n] previous labels in, new labels out
    float *cosine;                 // [n] or nullptr
    unsigned long long *changed;
};

template <bool RESIDENT, bool VEC>
__global__ __launch_bounds__(MTHREADS) void kmeans_assign_kernel(const AssignArgs a) {
    extern __shared__ float4 kmeans_lds[];
    float *Xs = reinterpret_cast<float *>(kmeans_lds);
    const uint32_t xstride = RESIDENT ? a.dpad + 4 : (uint32_t)MS;
    float *Cs = Xs + (RESIDENT ? MR * xstride : 2 * MR * MS);
    float *rs = Cs;                                                  // after the last tile the stage is free: the four
    uint32_t *ri = reinterpret_cast<uint32_t *>(Cs + MR * 4);        // (score, index) candidates of every row

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int rh = w & 1, ch = w >> 1, h = lane >> 5, l32 = lane & 31;
    const uint64_t r0 = CLEORA_LINEAR_BLOCK() * MR;
    if (r0 >= a.n) return;
    const uint32_t nchunks = a.dpad / MK, ntiles = a.kpad / MC;

    // columns c .. c + 3 of row r, zeros outside the matrix
    auto load_x4 = [&](uint64_t r, uint32_t c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < a.n && c < a.d) {
            const float *p = a.x + r * a.ldx + c;
            if constexpr (VEC) {
                v = *reinterpret_cast<const float4 *>(p);
            } else {
                v.x = p[0];
                if (c + 1 < a.d) v.y = p[1];
                if (c + 2 < a.d) v.z = p[2];
                if (c + 3 < a.d) v.w = p[3];
            }
        }
        return v;
    };
    if constexpr (RESIDENT) {
        const uint32_t w4 = a.dpad / 4;
        for (uint32_t i = t; i < MR * w4; i += MTHREADS) {
            const uint32_t r = i / w4, c4 = i - r * w4;
            *reinterpret_cast<float4 *>(Xs + r * xstride + c4 * 4) = load_x4(r0 + r, c4 * 4);
        }
    }

    // this thread's share of a staged chunk: four float4 of the centroids (rows t / 8 + 32 i, columns 4 (t & 7) ..), two of X
    const int srow = t >> 3, sc4 = (t & 7) * 4;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 cr0 = zero4, cr1 = zero4, cr2 = zero4, cr3 = zero4, xr0 = zero4, xr1 = zero4;
    auto fetch = [&](uint32_t tile, uint32_t kc) {
        const uint32_t c = kc * MK + sc4;
        const float *p = a.cp + ((uint64_t)tile * MC + srow) * a.dpad + c;
        cr0 = *reinterpret_cast<const float4 *>(p);
        cr1 = *reinterpret_cast<const float4 *>(p + (uint64_t)32 * a.dpad);
        cr2 = *reinterpret_cast<const float4 *>(p + (uint64_t)64 * a.dpad);
        cr3 = *reinterpret_cast<const float4 *>(p + (uint64_t)96 * a.dpad);
        if constexpr (!RESIDENT) {
            xr0 = load_x4(r0 + srow, c);
            xr1 = load_x4(r0 + srow + 32, c);
        }
    };
    auto stage = [&](int buf) {
        float *cs = Cs + buf * MC * MS + srow * MS + sc4;
        *reinterpret_cast<float4 *>(cs) = cr0;
        *reinterpret_cast<float4 *>(cs + 32 * MS) = cr1;
        *reinterpret_cast<float4 *>(cs + 64 * MS) = cr2;
        *reinterpret_cast<float4 *>(cs + 96 * MS) = cr3;
        if constexpr (!RESIDENT) {
            float *xs = Xs + buf * MR * MS + srow * MS + sc4;
            *reinterpret_cast<float4 *>(xs) = xr0;
            *reinterpret_cast<float4 *>(xs + 32 * MS) = xr1;
        }
    };

    fetch(0, 0);
    stage(0);
    __syncthreads();

    float best = 0.f;
    uint32_t bidx = kNone;               // kNone: this lane has not seen a centroid yet
    floatx16 acc0, acc1;
    int buf = 0;
    for (uint32_t tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
        for (uint32_t kc = 0; kc < nchunks; ++kc, buf ^= 1) {
            const bool last_chunk = kc + 1 == nchunks;
            const bool has_next = !last_chunk || tile + 1 < ntiles;
            if (has_next) fetch(last_chunk ? tile + 1 : tile, last_chunk ? 0 : kc + 1);
            const float *ca = Cs + buf * MC * MS + (ch * 64 + l32) * MS + 4 * h;
            const float *xb = RESIDENT ? Xs + (rh * 32 + l32) * xstride + kc * MK + 4 * h : Xs + buf * MR * MS + (rh * 32 + l32) * MS + 4 * h;
#pragma unroll
            for (int kb = 0; kb < MK; kb += 8) {
                const float4 fa0 = *reinterpret_cast<const float4 *>(ca + kb), fa1 = *reinterpret_cast<const float4 *>(ca + 32 * MS + kb);
                const float4 fb = *reinterpret_cast<const float4 *>(xb + kb);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.x, fb.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.x, fb.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.y, fb.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.y, fb.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.z, fb.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.z, fb.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa0.w, fb.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(fa1.w, fb.w, acc1, 0, 0, 0);
            }
            if (has_next) stage(buf ^ 1);
            if (last_chunk) {
                // accumulator 4 j + i of acc0: centroid tile MC + 64 ch + 8 j + 4 h + i, of acc1: 32 more; row rh 32 + l32.
                // Ascending index and a strict >: the lowest index of equal scores stays
                const uint32_t cbase = tile * MC + ch * 64 + 4 * h;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint32_t c = cbase + 8 * (e >> 2) + (e & 3);
                    if (c < a.k && (bidx == kNone || acc0[e] > best)) { best = acc0[e]; bidx = c; }
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint32_t c = cbase + 32 + 8 * (e >> 2) + (e & 3);
                    if (c < a.k && (bidx == kNone || acc1[e] > best)) { best = acc1[e]; bidx = c; }
                }
            }
            __syncthreads();
        }
    }

    // the four lanes of a row: (wave pair ch) x (lane half h)
    rs[(rh * 32 + l32) * 4 + ch * 2 + h] = best;
    ri[(rh * 32 + l32) * 4 + ch * 2 + h] = bidx;
    __syncthreads();
    if (t < MR) {                        // wave 0, one lane per row
        const uint64_t r = r0 + t;
        float s = 0.f;
        uint32_t b = kNone;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float se = rs[t * 4 + e];
            const uint32_t be = ri[t * 4 + e];
            if (be != kNone && (b == kNone || se > s || (se == s && be < b))) { s = se; b = be; }
        }
        bool moved = false;
        if (r < a.n) {
            if (b == kNone) { b = 0; s = 0.f; }      // cannot happen for k >= 1: the lane of centroid 0 always has an entry
            moved = a.labels[r] != b;
            a.labels[r] = b;
            if (a.cosine != nullptr) a.cosine[r] = s * a.inv[r];
        }
        const unsigned long long votes = __ballot(moved);
        if (t == 0 && votes != 0ull) atomicAdd(a.changed, (unsigned long long)__popcll(votes));
    }
}

// ---------------------------------------------------------------------------------------------------------------- update

__global__ __launch_bounds__(256) void kmeans_fill_kernel(uint32_t *__restrict__ v, uint64_t n, uint32_t value) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) v[i] = value;
}

// One block per (chunk, column slab): part[chunk][col] = sum over the chunk's members, in member order, of x[m][col] / ||x_m|| (f64).
__global__ __launch_bounds__(USLAB) void kmeans_sum_kernel(const float *__restrict__ x, uint64_t ldx, uint32_t d, const float *__restrict__ inv,
                                                           const uint32_t *__restrict__ members, const uint32_t *__restrict__ coff,
                                                           const uint32_t *__restrict__ choff, uint32_t k, double *__restrict__ part) {
    __shared__ uint32_t mrow[UCHUNK];
    __shared__ float minv[UCHUNK];
    const uint64_t q = CLEORA_LINEAR_BLOCK();
    if (q >= choff[k]) return;
    uint32_t lo = 0, hi = k;                 // the cluster of chunk q: the last c with choff[c] <= q (empty clusters have no chunk)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (choff[mid] <= q) lo = mid; else hi = mid;
    }
    const uint32_t t = threadIdx.x;
    const uint32_t m0 = coff[lo] + ((uint32_t)q - choff[lo]) * UCHUNK;
    const uint32_t m1 = coff[lo + 1] - m0 < UCHUNK ? coff[lo + 1] : m0 + UCHUNK;
    const uint32_t cnt = m1 - m0;
    if (t < cnt) {
        const uint32_t r = members[m0 + t];
        mrow[t] = r;
        minv[t] = inv[r];
    }
    __syncthreads();
    const uint32_t col = blockIdx.z * USLAB + t;
    if (col >= d) return;
    const float *xc = x + col;
    double acc = 0.0;
#pragma unroll 8
    for (uint32_t m = 0; m < cnt; ++m) acc += (double)(xc[(uint64_t)mrow[m] * ldx] * minv[m]);
    part[q * d + col] = acc;
}

// One block per cluster: chunk partials in chunk order -> mean -> norm (fixed tree) -> the new unit centroid, rounded once.
__global__ __launch_bounds__(256) void kmeans_finish_kernel(double *__restrict__ part, const uint32_t *__restrict__ coff,
                                                            const uint32_t *__restrict__ choff, uint32_t d, float *__restrict__ cent) {
    __shared__ double red[256];
    const uint32_t c = blockIdx.x, t = threadIdx.x;
    const uint32_t cnt = coff[c + 1] - coff[c];
    if (cnt == 0) return;                                   // no members: the old centroid stays
    const uint64_t q0 = choff[c], q1 = choff[c + 1];
    double sq = 0.0;
    for (uint32_t col = t; col < d; col += 256) {
        double s = 0.0;
        for (uint64_t q = q0; q < q1; ++q) s += part[q * d + col];
        s /= (double)cnt;
        part[q0 * d + col] = s;                             // this thread's own column: kept for the second pass
        sq += s * s;
    }
    red[t] = sq;
    __syncthreads();
    for (uint32_t o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    const double norm = sqrt(red[0]);
    if (!(norm > 1e-10)) return;                            // e.g. all members are zero rows: the old centroid stays
    for (uint32_t col = t; col < d; col += 256) cent[(uint64_t)c * d + col] = (float)(part[q0 * d + col] / norm);
}

// ---------------------------------------------------------------------------------------------------------------- host

struct KmeansPlan {
    uint32_t dpad, kpad;
    uint64_t max_chunks;
    uint64_t off_changed, off_cp, off_members, off_table, off_count, off_coff, off_choff, off_part, bytes;
};

KmeansPlan kmeans_plan(uint64_t n, uint32_t d, uint32_t k) {
    KmeansPlan p;
    p.dpad = (uint32_t)up(d ? d : 1, MK);
    p.kpad = (uint32_t)up(k ? k : 1, MC);
    p.max_chunks = (n + UCHUNK - 1) / UCHUNK + k;            // sum over clusters of ceil(count / UCHUNK) is at most this
    const uint64_t segs_bound = member_segs(n).segs_bound;
    p.off_changed = up(n * 4, 256);                          // [0, ..): 1 / ||x_r||
    p.off_cp = p.off_changed + 256;
    p.off_members = p.off_cp + up((uint64_t)p.kpad * p.dpad * 4, 256);
    p.off_table = p.off_members + up(n * 4, 256);
    p.off_count = p.off_table + up(segs_bound * k * 4, 256);
    p.off_coff = p.off_count + up((uint64_t)k * 4, 256);
    p.off_choff = p.off_coff + up(((uint64_t)k + 1) * 4, 256);
    p.off_part = p.off_choff + up(((uint64_t)k + 1) * 4, 256);
    p.bytes = p.off_part + p.max_chunks * d * 8;
    return p;
}

int kmeans_check(const void *x, uint64_t ldx, uint64_t n, uint32_t d, const void *centroids, uint32_t k, const void *labels,
                 const void *workspace) {
    CL_REQUIRE(x != nullptr && centroids != nullptr && labels != nullptr && workspace != nullptr,
               "x / centroids / labels / workspace is NULL");
    CL_REQUIRE(k >= 2, "k must be at least 2");
    CL_REQUIRE(k <= CLEORA_KMEANS_MAX_K, "k is larger than CLEORA_KMEANS_MAX_K = 4096");
    CL_REQUIRE((uint64_t)k <= n, "k cannot be larger than the number of rows n");
    CL_REQUIRE(n < (1ull << 32), "more than 2^32 rows");
    CL_REQUIRE(d >= 1 && d <= kKmeansMaxD, "need 1 <= d <= 16384");
    CL_REQUIRE(ldx >= d, "need ldx >= d");
    return CLEORA_OK;
}

float *kmeans_inv(void *workspace) { return static_cast<float *>(workspace); }

int enqueue_assign(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const float *centroids, uint32_t k, uint32_t *labels,
                   float *cosine, unsigned long long *changed, void *workspace, hipStream_t stream, bool inv_ready) {
    const KmeansPlan p = kmeans_plan(n, d, k);
    char *ws = static_cast<char *>(workspace);
    float *cp = reinterpret_cast<float *>(ws + p.off_cp);
    if (cosine != nullptr && !inv_ready) launch_row_inv_norm(x, ldx, n, n, d, kmeans_inv(workspace), stream);
    hipLaunchKernelGGL(kmeans_pack_kernel, dim3(p.kpad), dim3(64), 0, stream, centroids, k, d, p.dpad, cp, changed);
    CL_HIP(hipGetLastError());

    AssignArgs a;
    a.x = x;
    a.ldx = ldx;
    a.n = n;
    a.d = d;
    a.dpad = p.dpad;
    a.k = k;
    a.kpad = p.kpad;
    a.cp = cp;
    a.inv = kmeans_inv(workspace);
    a.labels = labels;
    a.cosine = cosine;
    a.changed = changed;
    const bool resident = p.dpad <= (uint32_t)MD;
    const bool vec = d % 4 == 0 && ldx % 4 == 0 && aligned16(x);
    const size_t lds = ((resident ? (size_t)MR * (p.dpad + 4) : (size_t)2 * MR * MS) + (size_t)2 * MC * MS) * 4;
    const dim3 blocks = grid_1d_as_2d((n + MR - 1) / MR);
    auto go = [&](auto kernel) {
        // per DEVICE and cheap: set on every call
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) hipLaunchKernelGGL(kernel, blocks, dim3(MTHREADS), lds, stream, a);
        return e;
    };
    CL_HIP(resident ? (vec ? go(kmeans_assign_kernel<true, true>) : go(kmeans_assign_kernel<true, false>))
                    : (vec ? go(kmeans_assign_kernel<false, true>) : go(kmeans_assign_kernel<false, false>)));
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

int enqueue_update(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const uint32_t *labels, float *centroids, uint32_t k,
                   void *workspace, hipStream_t stream, bool inv_ready) {
    const KmeansPlan p = kmeans_plan(n, d, k);
    char *ws = static_cast<char *>(workspace);
    float *inv = kmeans_inv(workspace);
    uint32_t *members = reinterpret_cast<uint32_t *>(ws + p.off_members), *table = reinterpret_cast<uint32_t *>(ws + p.off_table);
    uint32_t *count = reinterpret_cast<uint32_t *>(ws + p.off_count), *coff = reinterpret_cast<uint32_t *>(ws + p.off_coff);
    uint32_t *choff = reinterpret_cast<uint32_t *>(ws + p.off_choff);
    double *part = reinterpret_cast<double *>(ws + p.off_part);

    if (!inv_ready) launch_row_inv_norm(x, ldx, n, n, d, inv, stream);
    enqueue_member_lists<UCHUNK>(labels, n, k, table, count, coff, choff, members, stream);
    CL_HIP(hipGetLastError());
    dim3 grid = grid_1d_as_2d(p.max_chunks);
    grid.z = (d + USLAB - 1) / USLAB;
    hipLaunchKernelGGL(kmeans_sum_kernel, grid, dim3(USLAB), 0, stream, x, ldx, d, inv, members, coff, choff, k, part);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(k), dim3(256), 0, stream, part, coff, choff, d, centroids);
    CL_HIP(hipGetLastError());
    return CLEORA_OK;
}

}  // namespace

uint64_t kmeans_workspace_bytes(uint64_t n, uint32_t d, uint32_t k) { return kmeans_plan(n, d, k).bytes; }

int launch_kmeans_assign(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const float *centroids, uint32_t k, uint32_t *labels_io,
                         float *best_cosine_out, uint64_t *changed_out, void *workspace, hipStream_t stream) {
    CL_REQUIRE(changed_out != nullptr, "changed_out is NULL");
    const int rc = kmeans_check(x, ldx, n, d, centroids, k, labels_io, workspace);
    if (rc != CLEORA_OK) return rc;
    return enqueue_assign(x, ldx, n, d, centroids, k, labels_io, best_cosine_out, reinterpret_cast<unsigned long long *>(changed_out),
                          workspace, stream, false);
}

int launch_kmeans_update(const float *x, uint64_t ldx, uint64_t n, uint32_t d, const uint32_t *labels, float *centroids_io, uint32_t k,
                         void *workspace, hipStream_t stream) {
    const int rc = kmeans_check(x, ldx, n, d, centroids_io, k, labels, workspace);
    if (rc != CLEORA_OK) return rc;
    return enqueue_update(x, ldx, n, d, labels, centroids_io, k, workspace, stream, false);
}

int kmeans_cosine(const float *x, uint64_t ldx, uint64_t n, uint32_t d, float *centroids_io, uint32_t k, uint32_t max_iterations,
                  uint32_t *labels_out, uint32_t *iterations_out, void *workspace, hipStream_t stream) {
    CL_REQUIRE(iterations_out != nullptr, "iterations_out is NULL");
    const int rc = kmeans_check(x, ldx, n, d, centroids_io, k, labels_out, workspace);
    if (rc != CLEORA_OK) return rc;
    const KmeansPlan p = kmeans_plan(n, d, k);
    unsigned long long *changed = reinterpret_cast<unsigned long long *>(static_cast<char *>(workspace) + p.off_changed);
    const unsigned fill_blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(kmeans_fill_kernel, dim3(fill_blocks), dim3(256), 0, stream, labels_out, n, 0u);      // :26
    launch_row_inv_norm(x, ldx, n, n, d, kmeans_inv(workspace), stream);
    CL_HIP(hipGetLastError());
    uint32_t done = 0;
    while (done < max_iterations) {                                                                          // :28-42
        int e = enqueue_assign(x, ldx, n, d, centroids_io, k, labels_out, nullptr, changed, workspace, stream, true);
        if (e != CLEORA_OK) return e;
        ++done;
        unsigned long long moved = 0;
        CL_HIP(hipMemcpyAsync(&moved, changed, sizeof(moved), hipMemcpyDeviceToHost, stream));
        CL_HIP(hipStreamSynchronize(stream));
        if (moved == 0) break;
        e = enqueue_update(x, ldx, n, d, labels_out, centroids_io, k, workspace, stream, true);
        if (e != CLEORA_OK) return e;
    }
    CL_HIP(hipStreamSynchronize(stream));
    *iterations_out = done;
    return CLEORA_OK;
}

}  // namespace cleora
