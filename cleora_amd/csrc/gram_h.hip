// gram_h.hip — the whitened loop's statistics from f16-STORED rows (CLEORA_F_STATS_F16), for gfx950:
//     mean = sum_r y_r / n            Gram = sum_r (y_r - mean)(y_r - mean)^T            both f64, y = the f16 values as stored
// on v_mfma_f32_32x32x16_f16, ONE MFMA per tile and k-step.
//
// Why another kernel beside gram16_kernel (whiten.hip).  That kernel reads f32 rows, centres them with an f32 shift and splits every
// value into two or three bf16 pieces: it is bound by issuing those instructions (0.37 of the HBM roof at the C3 shape), runs three or
// six MFMAs per product and stages two or three fragment pieces per element through LDS.  A product of two f16 values is exact in f32,
// so rows that are STORED as f16 need no split — and must get no centring either: y - c is not an f16 value.  The kernel therefore
// accumulates the UNCENTRED Gram sum_r y_r y_r^T and the exact column sums, and the reducer (launch_gram32_finish, whiten.hip: the
// existing `delta` correction with a zero shift) forms  sum y y^T - n mean mean^T  in f64.  What that costs: the f32 stage sums are
// rounded relative to the uncentred entries, which are larger than the centred ones by up to 1 / (1 - |mean|^2 / mean |y|^2) — a small
// factor for normalised rows (measured beside the split form in tests/test_gpu_stats_f16.py); eigh.hip's guard is tightened for it.
//
// Kept from gram16_kernel (gram32_common.h): 256-column super-tiles — a DIAGONAL block owns the 36 upper 32x32 tiles of one, dealt to
// eight waves as 4 4 4 4 5 5 5 5; an OFF-DIAGONAL pair (I < J) is two blocks, 128 columns of I against all 256 of J, wave w owning tile
// row w >> 1 and four tile columns —, row slices with private f64 partials (gram32_fold: every element belongs to one lane, no atomics),
// the slices added in a fixed order: deterministic.  Accumulation: the matrix cores sum 32 rows (two k-steps) from zero — the chain
// length whose bias was measured for the f32-accumulating MFMAs (gram16_diag_stage_sums) —, the vector unit adds those sums in f32 over
// at most 2048 rows (256 below 2^20 rows: launch_gram_h), f64 across.
//
// New: the operand path.  Both MFMA operands of G = Y^T Y are "column i, eight consecutive ROWS" while memory is row-major, so staging
// transposes 2-byte elements:
//   * a wave owns ONE ROW OCTET of a stage (wave w: rows 8 w .. 8 w + 7 of its 64) and every 128-column group of the block (two in a
//     diagonal block, three in an off-diagonal one).  Lane l loads the dword of columns 2 l, 2 l + 1 of each of the eight rows: a wave
//     reads 256 contiguous bytes per row and group — the whole 512-byte row of a diagonal block at d = 256 — through a scalar row base;
//   * two v_perm_b32 per row pair separate the columns: the low halves of rows 2 j, 2 j + 1 make dword j of column 2 l's fragment, the
//     high halves that of column 2 l + 1.  8 loads, 8 perms and two ds_write_b128 per 16 x 8 elements; nothing else touches the values;
//   * LDS: [k-step][column block][lane] x 16 B, lane (i, h) = column i of the block, rows 8 h .. 8 h + 7 of the k-step — lane-linear
//     for ds_read_b128; 8 KiB (diagonal) / 12 KiB (off-diagonal) per k-step, a third of the split form's, so a stage is 64 rows (four
//     k-steps) instead of 32: half the barriers per row; two stages, 64 / 96 KiB;
//   * column sums beside the diagonal blocks: the sixteen values of a lane widened to f32 (exact) and added pairwise over the octet —
//     exact while the octet's sum stays below 1 (normalised rows), f64 across; the eight octets of a column meet in LDS at the end.
// 512 threads, one block per CU, two waves per SIMD in opposite phases (the lower four waves stage the next rows before their MFMAs,
// the upper four after).  Registers, LDS and occupancy: DESIGN.md §2.3 (scripts/kernel_resources.py prints them).
#include "common.h"
#include "gram32_common.h"

namespace cleora {
namespace {

constexpr int GH_KR = 64;                     // rows per stage
constexpr int GH_KS = GH_KR / 16;             // k-steps per stage
constexpr int GH_CHAIN = 2;                   // k-steps the matrix cores sum from zero
constexpr int GH_THREADS = 512;
constexpr uint64_t GH_MIN_SLICE_ROWS = 4096;  // a slice shorter than this does not repay its partials

struct GramHArgs {
    const uint16_t *y;
    uint64_t ldy, n;         // ldy in f16 elements
    double *colsum;          // [slices][d]
    double *partial;         // [slices][tiles_per_slice][32][32]: S x 36 diagonal tiles, then S (S - 1) / 2 x 64 off-diagonal ones
    uint64_t rows_per_slice; // a multiple of the stage
    uint32_t sub_rows;       // fold period, a multiple of the stage
    uint32_t d, S, tiles_per_slice;
};

typedef const char __attribute__((address_space(1))) *gh_bytes;
typedef const uint32_t __attribute__((address_space(1))) *gh_u32;
// a dword through a wave-uniform row base held as an SGPR pair + the lane's 32-bit byte offset (global_load with a scalar base)
__device__ __forceinline__ uint32_t gh_load(const uint16_t *row, uint32_t byte_offset) {
    const uint64_t v = reinterpret_cast<uint64_t>(row);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return *reinterpret_cast<gh_u32>(reinterpret_cast<gh_bytes>(((uint64_t)hi << 32) | lo) + byte_offset);
}

template <int NCB>
__device__ __forceinline__ uint32_t gh_slot(int ks, int cbk, int lane) { return (uint32_t)(((ks * NCB + cbk) * 64 + lane) * 16); }

// the tiles of wave W: column block of the A / B fragment inside the stage, index of the tile in the block's partial
template <int W, bool DIAG> __host__ __device__ constexpr int gh_ntiles() { return DIAG ? g16_ntiles(W) : 4; }
template <int W, bool DIAG> __host__ __device__ constexpr int gh_a(int q) { return DIAG ? G16_TR[W][q] : W >> 1; }
template <int W, bool DIAG> __host__ __device__ constexpr int gh_b(int q) { return DIAG ? G16_TC[W][q] : 4 + 4 * (W & 1) + q; }
template <int W, bool DIAG> __host__ __device__ constexpr bool gh_uses(int blk) {
    for (int q = 0; q < gh_ntiles<W, DIAG>(); ++q)
        if (gh_a<W, DIAG>(q) == blk || gh_b<W, DIAG>(q) == blk) return true;
    return false;
}

// DIAG: `c0` = first column of the super-tile, groups c0, c0 + 128.  Otherwise groups c0 (128 columns of I), c1, c1 + 128 (J).
template <int W, bool DIAG>
__device__ __forceinline__ void gramh_body(const GramHArgs &a, char *lds, uint32_t c0, uint32_t c1, uint32_t tile_base) {
    constexpr int NG = DIAG ? 2 : 3, NCB = 4 * NG, STAGE = GH_KS * NCB * 1024, NT = gh_ntiles<W, DIAG>();
    const int t = threadIdx.x, lane = t & 63, i = lane & 31, h = lane >> 5;
    const uint64_t r_begin = (uint64_t)blockIdx.y * a.rows_per_slice;
    const uint64_t r_end = r_begin + a.rows_per_slice < a.n ? r_begin + a.rows_per_slice : a.n;
    uint32_t col[NG];                                       // first of this lane's two columns in each group
    col[0] = c0 + 2 * lane;
    col[1] = (DIAG ? c0 + 128 : c1) + 2 * lane;
    if constexpr (!DIAG) col[2] = c1 + 128 + 2 * lane;

    f16v acc[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    double cs[DIAG ? NG : 1][2] = {};
    uint32_t pre[NG][8];
    int nv = 0;                                             // valid rows of the prefetched octet
    auto prefetch = [&](uint64_t row0) {
        const uint64_t ra = row0 + 8 * W;
        if (row0 + GH_KR <= r_end) {                        // a whole stage: one scalar row base, the eight rows by additions
            nv = 8;
            const uint16_t *rowp = a.y + ra * a.ldy;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
#pragma unroll
                for (int g = 0; g < NG; ++g) pre[g][j] = gh_load(rowp, 2u * col[g]);
                rowp += a.ldy;
            }
            return;
        }
        nv = ra >= r_end ? 0 : (r_end - ra >= 8 ? 8 : (int)(r_end - ra));
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint16_t *rowp = a.y + (j < nv ? ra + j : r_begin) * a.ldy;        // always a valid row
#pragma unroll
            for (int g = 0; g < NG; ++g) pre[g][j] = *reinterpret_cast<const uint32_t *>(rowp + col[g]);
        }
    };
    auto stage = [&](int buf) {
        char *const sb = lds + buf * STAGE;
        const int ks = W >> 1, ln = (W & 1) * 32 + 2 * (lane & 15);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            uint32_t v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < nv ? pre[g][j] : 0u;             // rows past the slice count as zeros
            u32x4 even, odd;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                even[jj] = __builtin_amdgcn_perm(v[2 * jj + 1], v[2 * jj], 0x05040100u);     // low halves: column 2 l, rows 2 jj, 2 jj + 1
                odd[jj] = __builtin_amdgcn_perm(v[2 * jj + 1], v[2 * jj], 0x07060302u);      // high halves: column 2 l + 1
            }
            const int cbk = 4 * g + (lane >> 4);
            *reinterpret_cast<u32x4 *>(sb + gh_slot<NCB>(ks, cbk, ln)) = even;
            *reinterpret_cast<u32x4 *>(sb + gh_slot<NCB>(ks, cbk, ln + 1)) = odd;
            if constexpr (DIAG) {
                float lo[8], hi[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const h2v p = __builtin_bit_cast(h2v, v[j]);
                    lo[j] = (float)p[0];
                    hi[j] = (float)p[1];
                }
                cs[g][0] += (double)(((lo[0] + lo[1]) + (lo[2] + lo[3])) + ((lo[4] + lo[5]) + (lo[6] + lo[7])));
                cs[g][1] += (double)(((hi[0] + hi[1]) + (hi[2] + hi[3])) + ((hi[4] + hi[5]) + (hi[6] + hi[7])));
            }
        }
    };
    // acc += the sums of one staged 64-row stage over this wave's tiles, in chains of GH_CHAIN k-steps from zero
    auto stage_sums = [&](int buf) {
        const char *const sb = lds + buf * STAGE;
#pragma unroll
        for (int c = 0; c < GH_KS / GH_CHAIN; ++c) {
            f16v tmp[NT];
#pragma unroll
            for (int kk = 0; kk < GH_CHAIN; ++kk) {
                h8v f[NCB];
#pragma unroll
                for (int blk = 0; blk < NCB; ++blk)
                    if (gh_uses<W, DIAG>(blk)) f[blk] = *reinterpret_cast<const h8v *>(sb + gh_slot<NCB>(c * GH_CHAIN + kk, blk, lane));
#pragma unroll
                for (int q = 0; q < NT; ++q)
                    tmp[q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[gh_a<W, DIAG>(q)], f[gh_b<W, DIAG>(q)], kk == 0 ? zero16 : tmp[q], 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < NT; ++q) acc[q] += tmp[q];
        }
    };
    double *const out = a.partial + ((uint64_t)blockIdx.y * a.tiles_per_slice + tile_base) * 1024;
    auto tile_index = [](int q) { return DIAG ? upper_tile_index(gh_a<W, DIAG>(q), gh_b<W, DIAG>(q)) : q; };
    gram32_fold<NT>(out, acc, i, h, true, tile_index);

    if (r_begin < r_end) {
        prefetch(r_begin);
        stage(0);
        if (r_begin + GH_KR < r_end) prefetch(r_begin + GH_KR);
    }
    __syncthreads();
    int buf = 0;
    uint32_t in_sub = 0;
    constexpr bool STAGE_FIRST = W < 4;                      // opposite phases for the two waves of a SIMD (w and w + 4)
    auto stage_next = [&](uint64_t row0, int b) {
        if (row0 + GH_KR < r_end) {
            stage(b ^ 1);
            if (row0 + 2 * GH_KR < r_end) prefetch(row0 + 2 * GH_KR);
        }
    };
    for (uint64_t row0 = r_begin; row0 < r_end; row0 += GH_KR, buf ^= 1) {
        if constexpr (STAGE_FIRST) stage_next(row0, buf);
        stage_sums(buf);
        in_sub += GH_KR;
        if (in_sub >= a.sub_rows || row0 + GH_KR >= r_end) {
            gram32_fold<NT>(out, acc, i, h, false, tile_index);
            in_sub = 0;
        }
        if constexpr (!STAGE_FIRST) stage_next(row0, buf);
        __syncthreads();
    }

    if constexpr (DIAG) {
        // column sums: wave w summed octet w of every stage for its 2 x 2 columns; the eight octets of a column meet in LDS
        double *red = reinterpret_cast<double *>(lds);      // the loop ended on a barrier: the stages are free (16 of 64 KiB)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            red[W * G32_D + 128 * g + 2 * lane] = cs[g][0];
            red[W * G32_D + 128 * g + 2 * lane + 1] = cs[g][1];
        }
        __syncthreads();
        if (t < G32_D) {
            double s = red[t];
#pragma unroll
            for (int w = 1; w < 8; ++w) s += red[w * G32_D + t];
            a.colsum[(uint64_t)blockIdx.y * a.d + c0 + t] = s;
        }
    }
}

// grid = (S + S (S - 1), slices): block x < S is the diagonal block of super-tile x; the others come in pairs per (I < J).
// 512 threads; dynamic LDS: two stages of 4 k-steps x (8 or 12) KiB
__global__ __launch_bounds__(GH_THREADS, 1) void gramh_kernel(const GramHArgs a) {
    extern __shared__ __attribute__((aligned(16))) char gh_lds[];
    const uint32_t b = blockIdx.x;
    if (b < a.S) {
        const uint32_t c0 = b * G32_D, tb = b * G32_TILES;
        switch (threadIdx.x >> 6) {                          // whole waves take each arm; every arm meets the same barriers
            case 0: gramh_body<0, true>(a, gh_lds, c0, 0, tb); break;
            case 1: gramh_body<1, true>(a, gh_lds, c0, 0, tb); break;
            case 2: gramh_body<2, true>(a, gh_lds, c0, 0, tb); break;
            case 3: gramh_body<3, true>(a, gh_lds, c0, 0, tb); break;
            case 4: gramh_body<4, true>(a, gh_lds, c0, 0, tb); break;
            case 5: gramh_body<5, true>(a, gh_lds, c0, 0, tb); break;
            case 6: gramh_body<6, true>(a, gh_lds, c0, 0, tb); break;
            default: gramh_body<7, true>(a, gh_lds, c0, 0, tb); break;
        }
        return;
    }
    const uint32_t pair = (b - a.S) >> 1, half = (b - a.S) & 1;
    uint32_t q = pair, rowlen = a.S - 1, I = 0;
    while (q >= rowlen) { q -= rowlen; ++I; --rowlen; }
    const uint32_t J = I + 1 + q;
    const uint32_t w = threadIdx.x >> 6;
    // wave w's four tiles: row 4 half + (w >> 1) of the pair's 8 x 8 grid, columns 4 (w & 1) .. + 3
    const uint32_t c0 = I * G32_D + half * 128, c1 = J * G32_D, tb = a.S * G32_TILES + pair * G32_OFF_TILES + (4 * half + (w >> 1)) * 8 + 4 * (w & 1);
    switch (w) {
        case 0: gramh_body<0, false>(a, gh_lds, c0, c1, tb); break;
        case 1: gramh_body<1, false>(a, gh_lds, c0, c1, tb); break;
        case 2: gramh_body<2, false>(a, gh_lds, c0, c1, tb); break;
        case 3: gramh_body<3, false>(a, gh_lds, c0, c1, tb); break;
        case 4: gramh_body<4, false>(a, gh_lds, c0, c1, tb); break;
        case 5: gramh_body<5, false>(a, gh_lds, c0, c1, tb); break;
        case 6: gramh_body<6, false>(a, gh_lds, c0, c1, tb); break;
        default: gramh_body<7, false>(a, gh_lds, c0, c1, tb); break;
    }
}

}  // namespace

bool gramh_applies(const uint16_t *y, uint64_t ldy, uint64_t n, uint32_t d) {
    return d % G32_D == 0 && d > 0 && d <= 2048 && ldy >= d && ldy % 8 == 0 && (reinterpret_cast<uintptr_t>(y) & 15u) == 0 && n >= 4096;
}

// mean and centred Gram (both f64) of the f16 rows y; ws: gram_workspace(n, d) doubles (the split form's sizing covers this one)
int launch_gram_h(const uint16_t *y, uint64_t ldy, uint64_t n, uint32_t d, double *ws, double *gram, hipStream_t stream, double *mean_out64,
                  float *mean_out32) {
    CL_REQUIRE(y != nullptr && ws != nullptr && gram != nullptr && mean_out64 != nullptr && mean_out32 != nullptr, "y / workspace / gram / mean is NULL");
    CL_REQUIRE(gramh_applies(y, ldy, n, d), "internal: the f16 Gram does not apply to this shape");
    const Gram32Plan q = gram32_plan(n, d);
    uint64_t slices = n / GH_MIN_SLICE_ROWS;
    slices = slices > q.slices ? q.slices : slices;          // (n >= 4096: at least one; never more than the workspace was sized for)
    CL_REQUIRE(slices >= 1 && slices <= 65535, "internal: bad number of Gram slices");
    GramHArgs a{};
    a.y = y;
    a.ldy = ldy;
    a.n = n;
    a.d = d;
    a.S = q.S;
    a.tiles_per_slice = q.tiles_per_slice;
    a.partial = ws;
    a.colsum = ws + slices * q.tiles_per_slice * 1024;
    a.rows_per_slice = ((n + slices - 1) / slices + GH_KR - 1) / GH_KR * GH_KR;
    // The fold period.  The stage sums are added in f32 to accumulators that grow with the UNCENTRED entries (n mean_i mean_j + the
    // centred part), so every add rounds relative to a larger number than in the split form; over a fold of K adds and F folds the
    // error relative to the Gram goes as K sqrt(32 / n) (independent across folds).  Measured at n = 4096, d = 256, |mean|^2 = 0.2:
    // 2.8e-7 with 2048-row folds against the split form's 2.6e-8.  Short matrices therefore fold every 256 rows (a fold is an f64
    // read-modify-write of the block's partials: 4.5 bytes of cache traffic per input byte — nothing at these sizes); from 2^20 rows
    // (launch_gram32's own threshold) 2048-row folds give <= 2e-8 by the same law and cost 0.6 bytes per input byte.
    a.sub_rows = n < (1ull << 20) ? 256 : 2048;
    const size_t lds = (size_t)2 * GH_KS * (q.S == 1 ? 8 : 12) * 1024;
    // per DEVICE and cheap: set on every call
    CL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(gramh_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(gramh_kernel, dim3(q.blocks, (unsigned)slices), dim3(GH_THREADS), lds, stream, a);
    CL_HIP(hipGetLastError());
    return launch_gram32_finish(ws, (uint32_t)slices, q, n, d, nullptr, false, gram, mean_out64, mean_out32, stream);
}

}  // namespace cleora
