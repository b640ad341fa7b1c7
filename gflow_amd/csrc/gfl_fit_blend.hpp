// Fused fit iteration: what the forward blend (fused_blend_fwd_kernel, gfl_fit_fwd.hip) and the backward blend
// (fused_blend_bwd_kernel, gfl_fit_bwd.hip) agree on, written once -- which 8x8 block of a tile a wave walks (block plan), the
// cull of staged splats against the box of the pixels still alive, and the layout of the checkpoints the forward leaves at the
// segment boundaries of a heavy tile for the backward (fit_regions, gfl_fit.hip, sizes the region from the same constants).
#pragma once
#include "gfl_fit.hpp"

namespace gfl {

// ------------------------------------------------------------------ block plan (gfl_sched.hpp)
// Which SIMD is this wave on?  The scheduler plans which SIMD walks which 8x8 block of every item; the plan is followed only
// if the workgroup's four waves sit on four different SIMDs (they do: the dispatcher deals a workgroup's waves round the
// SIMDs) and the item's plan is a permutation, otherwise wave k walks block k.
__device__ __forceinline__ unsigned wave_hw_id() { unsigned v; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v)); return v; }
__device__ __forceinline__ unsigned wave_xcc_id() { unsigned v; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v)); return v; }
__device__ __forceinline__ int wave_simd() { return (wave_hw_id() >> 4) & 3; }
// s_simd: four ints of LDS; holds a barrier, so every wave of the workgroup calls it
__device__ __forceinline__ bool simds_distinct(int32_t* s_simd, int simd) {
    if ((threadIdx.x & 63) == 0) s_simd[threadIdx.x >> 6] = simd;
    __syncthreads();
    return ((1 << s_simd[0]) | (1 << s_simd[1]) | (1 << s_simd[2]) | (1 << s_simd[3])) == 15;
}
// the 8x8 block of the tile this wave walks
__device__ __forceinline__ int plan_block(unsigned plan, int simd, bool simds_ok, int wave) {
    const bool plan_ok = simds_ok && ((1 << (plan & 3)) | (1 << ((plan >> 2) & 3)) | (1 << ((plan >> 4) & 3)) | (1 << ((plan >> 6) & 3))) == 15;
    return plan_ok ? (int)((plan >> (2 * simd)) & 3u) : wave;
}

// ------------------------------------------------------------------ alive box
// Once pixels have stopped (forward) or lie in front of every remaining contributor (backward), only splats that reach the
// bounding box of the pixels still ALIVE matter: the test of block_mask on that smaller box drops only work that contributes
// exactly nothing.  alive: a ballot over the wave's 8x8 block, lane = (y << 3) | x, not zero.
struct AliveBox { int xl, xh, yl, yh; };
__device__ __forceinline__ AliveBox alive_box(unsigned long long alive) {
    unsigned long long a = alive | (alive >> 32);
    a |= a >> 16;
    a |= a >> 8;
    const unsigned cols = (unsigned)a & 0xffu;               // columns with an alive pixel
    AliveBox b;
    b.xl = __builtin_ctz(cols); b.xh = 31 - __builtin_clz(cols);
    b.yl = (int)__builtin_ctzll(alive) >> 3; b.yh = (63 - (int)__builtin_clzll(alive)) >> 3;
    return b;
}
// hit &= "the staged record's alpha >= 1/255 disc reaches the box"; (px0, py0): the block's first pixel
__device__ __forceinline__ void cull_to_alive_box(bool& hit, unsigned long long alive, const RecLDS& r, int px0, int py0) {
    const AliveBox b = alive_box(alive);
    if (hit) {
        const BlockTest t = block_test(r.p0, r.p1, r.p2.z);
        hit = box_hit(t, (float)(px0 + b.xl), (float)(px0 + b.xh), (float)(py0 + b.yl), (float)(py0 + b.yh));
    }
}
// The quarter walk's variant (forward, long first tiles): a wave owns a 4x4 quarter, lane >> 4 = its pixel column, bit g of a
// lane's `alive` = pixel (column, row g) is in the image and has not stopped; (qx0, qy0): the quarter's first pixel.
struct QuarterBox { float x_lo, x_hi, y_lo, y_hi; };
__device__ __forceinline__ QuarterBox alive_box_quarter(unsigned alive, int qx0, int qy0) {
    unsigned arows = alive;
    arows |= (unsigned)__shfl_xor((int)arows, 16);
    arows |= (unsigned)__shfl_xor((int)arows, 32);           // pixel rows with an alive pixel (wave-uniform)
    const unsigned long long acol = __ballot(alive != 0);   // lanes of the columns with an alive pixel
    const unsigned cols = (unsigned)((acol & 1ull) | ((acol >> 15) & 2ull) | ((acol >> 30) & 4ull) | ((acol >> 45) & 8ull));
    QuarterBox b;
    b.x_lo = (float)(qx0 + __builtin_ctz(cols | 16u)); b.x_hi = (float)(qx0 + 31 - __builtin_clz(cols | 1u));
    b.y_lo = (float)(qy0 + __builtin_ctz(arows | 16u)); b.y_hi = (float)(qy0 + 31 - __builtin_clz(arows | 1u));
    return b;
}

// ------------------------------------------------------------------ checkpoints
// [queue][boundary][T C0 C1 C2 C3][the tile's pixels, block-major]: the forward's per-pixel state at the split positions of the
// first (heaviest) tile of each of the BACKWARD's queues, which walks it in up to HEAVY_PARTS segments.
constexpr int TILE_PIXELS = GFL_TILE * GFL_TILE;
constexpr int CKPT_PLANE = TILE_PIXELS;                   // floats between T, C0, .., C3 of a pixel
constexpr int CKPT_FLOATS = 5 * CKPT_PLANE;               // floats per boundary
constexpr size_t CKPT_REGION_FLOATS = (size_t)SCHED_MAX_QUEUES * (HEAVY_PARTS - 1) * CKPT_FLOATS;
// a pixel's place among its tile's: the 8x8 blocks one after the other, in_block = (y << 3) | x inside one
__device__ __forceinline__ int tile_place(int blk, int in_block) { return blk * 64 + in_block; }
template <typename F>        // F: float or const float
__device__ __forceinline__ F* ckpt_at(F* base, int queue_slot, int boundary) {
    return base + ((size_t)queue_slot * (HEAVY_PARTS - 1) + boundary) * CKPT_FLOATS;
}
// c: ckpt_at(..) + the pixel's tile_place
__device__ __forceinline__ void ckpt_store(float* c, float T, float c0, float c1, float c2, float c3) {
    c[0] = T; c[CKPT_PLANE] = c0; c[2 * CKPT_PLANE] = c1; c[3 * CKPT_PLANE] = c2; c[4 * CKPT_PLANE] = c3;
}
__device__ __forceinline__ void ckpt_load(const float* c, float& T, float (&C)[4]) {
    T = c[0]; C[0] = c[CKPT_PLANE]; C[1] = c[2 * CKPT_PLANE]; C[2] = c[3 * CKPT_PLANE]; C[3] = c[4 * CKPT_PLANE];
}

}  // namespace gfl
