// gram32_common.h — what the matrix-core Gram kernels of the whitened loop's intermediate iterations share: the 256-column super-tile
// layout, the deal of a diagonal block's 36 upper tiles to eight waves, and the fold of f32 accumulators into f64 partials
// (gram16_kernel in whiten.hip: split f32 operands on the bf16 matrix cores; gramh_kernel in gram_h.hip: f16 rows as stored).
#pragma once
#include "common.h"
#include "project_common.h"

namespace cleora {

// the plan both kernels' workspaces are sized for (gram_workspace) and the pass that finishes either kernel's partials (whiten.hip)
struct Gram32Plan { uint32_t S, blocks, tiles_per_slice, slices; };
Gram32Plan gram32_plan(uint64_t n, uint32_t d);
// mean = shift + colsum / n (shift64 == nullptr: zero), gram = sum of the slices' partials [+ diagfix on the diagonal] - n delta delta^T.
// ws: [slices][tiles_per_slice][32][32] partials, then [slices][d] column sums, [slices][d] diagonal corrections, [d] delta.
int launch_gram32_finish(double *ws, uint32_t slices, const Gram32Plan &q, uint64_t n, uint32_t d, const double *shift64, bool diagfix,
                         double *gram, double *mean_out64, float *mean_out32, hipStream_t stream);

namespace {

constexpr int G32_D = 256, G32_TILES = 36, G32_OFF_TILES = 64;

__host__ __device__ constexpr int upper_tile_index(int tr, int tc) { return tr * 8 - tr * (tr - 1) / 2 + (tc - tr); }

// The block's partial starts as zeros (written by the lanes that own the elements) so that every fold is the same
// unconditional read-modify-write: a "first fold stores, later folds add" flag makes the compiler branch around each of the
// loads.  The lane offset is made opaque inside the fold, or the element addresses are computed ahead of the main loop and
// live across it in scratch; tile by tile behind sched_barrier, or all loads are batched ahead of the adds and spill.
template <int NT, class TileIndex>
__device__ __forceinline__ void gram32_fold(double *out, f16v (&acc)[NT], int i, int h, bool zero, TileIndex tile_index) {
    uint32_t lo = (uint32_t)((4 * h) * 32 + i) * 8u;
    asm volatile("" : "+v"(lo));
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        // 32x32 C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        char *p = reinterpret_cast<char *>(out) + tile_index(q) * 8192 + lo;
        if (zero) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) *reinterpret_cast<double *>(p + ((reg & 3) + 8 * (reg >> 2)) * 256) = 0.0;
        } else {
            double old[16];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) old[reg] = *reinterpret_cast<const double *>(p + ((reg & 3) + 8 * (reg >> 2)) * 256);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                *reinterpret_cast<double *>(p + ((reg & 3) + 8 * (reg >> 2)) * 256) = old[reg] + (double)acc[q][reg];
                acc[q][reg] = 0.f;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// DIAGONAL block: the 36 upper tiles of a 256-column super-tile dealt to the 8 waves as 4 4 4 4 5 5 5 5 (waves w and w + 4 share a
// SIMD: 9 tiles per SIMD, the matrix pipes are evenly loaded)
constexpr int G16_TR[8][5] = {{0, 0, 0, 0, -1}, {0, 0, 0, 0, -1}, {1, 1, 1, 1, -1}, {1, 1, 1, 7, -1},
                              {2, 2, 2, 2, 2},  {2, 3, 3, 3, 3},  {3, 4, 4, 4, 4},  {5, 5, 5, 6, 6}};
constexpr int G16_TC[8][5] = {{0, 1, 2, 3, -1}, {4, 5, 6, 7, -1}, {1, 2, 3, 4, -1}, {5, 6, 7, 7, -1},
                              {2, 3, 4, 5, 6},  {7, 3, 4, 5, 6},  {7, 4, 5, 6, 7},  {5, 6, 7, 6, 7}};
__host__ __device__ constexpr int g16_ntiles(int w) { return w < 4 ? 4 : 5; }
__host__ __device__ constexpr bool g16_uses(int w, int blk) {
    for (int q = 0; q < g16_ntiles(w); ++q)
        if (G16_TR[w][q] == blk || G16_TC[w][q] == blk) return true;
    return false;
}
constexpr f16v zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

}  // namespace
}  // namespace cleora
