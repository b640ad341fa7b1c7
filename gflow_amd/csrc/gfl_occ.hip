// Occlusion masks from a forward and a backward flow (include/gflow_hip.h, "occlusion masks from the flows"): the
// forward-backward consistency check, both directions of every pair in ONE launch.  One lane per pixel; a workgroup is
// 64 x 4 pixels, so a wave reads and writes one row segment of 512 B (a float2 per lane) and its four gathers stay within
// the few rows the flow reaches.  No workspace, no atomics: a pixel's outputs depend on the inputs alone.
#include <cmath>

#include "gfl_common.hpp"

namespace gfl {

constexpr int OCC_BX = 64, OCC_BY = 4;
constexpr int OCC_MAX_GRID = 1 << 16;              // workgroups per launch; the tiles beyond are walked in a stride
constexpr float OCC_FLOW_MAX = 1048576.0f;         // 2^20: from here on every corner counts as outside the image

// S(img, x + f.x, y + f.y): bilinear, a corner outside the image contributes zero.  The weights come from the flow's own
// fraction (f - floor(f) and floor(f) are exact in float32; x + f.x is not), a corner inside always enters the sum, so a
// NaN there poisons the sample even at weight 0.
__device__ __forceinline__ float2 occ_sample(const float2* __restrict__ img, int W, int H, int x, int y, float2 f) {
    float2 acc = make_float2(0.f, 0.f);
    if (!(fabsf(f.x) < OCC_FLOW_MAX && fabsf(f.y) < OCC_FLOW_MAX)) return acc;      // (a NaN component lands here too)
    const float fx = floorf(f.x), fy = floorf(f.y);
    const float tx = f.x - fx, ty = f.y - fy;
    const int x0 = x + (int)fx, y0 = y + (int)fy;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int xx = x0 + dx, yy = y0 + dy;
            if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
            const float w = (dx ? tx : 1.f - tx) * (dy ? ty : 1.f - ty);
            const float2 v = img[yy * W + xx];
            acc.x += w * v.x;
            acc.y += w * v.y;
        }
    }
    return acc;
}

__device__ __forceinline__ float occ_norm(float x, float y) { return sqrtf(x * x + y * y); }

__global__ void __launch_bounds__(OCC_BX* OCC_BY)
    occ_kernel(const float2* __restrict__ fwd, const float2* __restrict__ bwd, int n_pairs, int W, int H, int tiles_x,
               int tiles_y, float alpha, float beta, float* __restrict__ diff_fwd, float* __restrict__ diff_bwd,
               uint8_t* __restrict__ occ_fwd, uint8_t* __restrict__ occ_bwd) {
    const int per_pair = tiles_x * tiles_y;                        // (< 2^28: W, H >= 2 and H W <= 2^30)
    const long long tiles = (long long)per_pair * n_pairs;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int pair = (int)(t / per_pair), r = (int)(t - (long long)pair * per_pair);
        const int x = (r % tiles_x) * OCC_BX + threadIdx.x, y = (r / tiles_x) * OCC_BY + threadIdx.y;
        if (x >= W || y >= H) continue;
        const int base = pair * (H * W);                           // n_pairs H W <= 2^30
        const int p = base + y * W + x;
        const float2 a = fwd[p], b = bwd[p];
        const float thr = alpha * (occ_norm(a.x, a.y) + occ_norm(b.x, b.y)) + beta;
        const bool thr_ok = isfinite(thr);
        if (diff_fwd || occ_fwd) {
            const float2 s = occ_sample(bwd + base, W, H, x, y, a);
            float d = occ_norm(a.x + s.x, a.y + s.y);
            const bool known = thr_ok && isfinite(d);
            if (!known) d = 0.f;
            if (diff_fwd) diff_fwd[p] = d;
            if (occ_fwd) occ_fwd[p] = (known && d > thr) ? 255 : 0;
        }
        if (diff_bwd || occ_bwd) {
            const float2 s = occ_sample(fwd + base, W, H, x, y, b);
            float d = occ_norm(b.x + s.x, b.y + s.y);
            const bool known = thr_ok && isfinite(d);
            if (!known) d = 0.f;
            if (diff_bwd) diff_bwd[p] = d;
            if (occ_bwd) occ_bwd[p] = (known && d > thr) ? 255 : 0;
        }
    }
}

}  // namespace gfl

using namespace gfl;

extern "C" {

int gfl_flow_occlusion(const float* fwd, const float* bwd, int n_pairs, int W, int H, float alpha, float beta,
                       float* diff_fwd, float* diff_bwd, uint8_t* occ_fwd, uint8_t* occ_bwd, gfl_stream_t stream) {
    if (W < 2 || H < 2 || n_pairs < 1) return GFL_ERR_INVALID;
    const size_t limit = (size_t)1 << 30, hw = (size_t)W * H;
    if (hw > limit || hw * (size_t)n_pairs > limit) return GFL_ERR_INVALID;
    if (!std::isfinite(alpha) || !std::isfinite(beta) || alpha < 0.f || beta < 0.f) return GFL_ERR_INVALID;
    if (!fwd || !bwd || ((uintptr_t)fwd & 7) || ((uintptr_t)bwd & 7)) return GFL_ERR_INVALID;      // (read as float2)
    if (!diff_fwd && !diff_bwd && !occ_fwd && !occ_bwd) return GFL_OK;
    const int tiles_x = (W + OCC_BX - 1) / OCC_BX, tiles_y = (H + OCC_BY - 1) / OCC_BY;
    const long long tiles = (long long)tiles_x * tiles_y * n_pairs;
    const int grid = (int)(tiles < OCC_MAX_GRID ? tiles : OCC_MAX_GRID);
    occ_kernel<<<grid, dim3(OCC_BX, OCC_BY), 0, (hipStream_t)stream>>>((const float2*)fwd, (const float2*)bwd, n_pairs, W, H,
                                                                         tiles_x, tiles_y, alpha, beta, diff_fwd, diff_bwd,
                                                                         occ_fwd, occ_bwd);
    return check_launch();
}

}  // extern "C"
