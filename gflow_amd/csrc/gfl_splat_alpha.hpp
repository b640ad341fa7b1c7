// The operator blend's rule: the alpha of one splat at one pixel (splat_alpha), shared by every kernel that walks a sorted
// tile list under it (gfl_blend.hip forward and backward, gfl_flow.hip, gfl_label.hip) -- a variant build of the rasteriser
// constants then changes all of them together -- and the front-to-back walk itself (operator_tile_walk), the one copy
// gfl_flow.hip and gfl_label.hip run: a pixel of the flow and label maps is made of the same splats with the same weights
// as in the render.  blend_fwd_kernel keeps the same loop written out (it is a little slower through the callables: the
// note there); tests/test_gpu_operator_walk.py holds the two to each other bit for bit.
// Also what the kernels share around the walk: the staging batch, the head of a fit record, a tile's list range, the
// entry-point checks.
#pragma once
#include "gfl_common.hpp"

namespace gfl {

constexpr int WALK_BATCH = 256;                     // records staged through LDS at a time: one per lane of the workgroup
constexpr int LIST_MAX_TILES = 16384;               // the largest tile grid of the kernels that take a fit's lists

// identical instruction sequence wherever it is inlined (explicit fma, contraction off) so that every walk takes the same
// skip/keep decision.  Returns false when the splat is skipped.
__device__ __forceinline__ bool splat_alpha(float u, float v, float A, float B, float C, float o, float fx, float fy,
                                            float& alpha, float& G) {
#pragma clang fp contract(off)
    const float dx = u - fx, dy = v - fy;
    const float q = __builtin_fmaf(A * dx, dx, (C * dy) * dy);
    const float power = __builtin_fmaf(-0.5f, q, -((B * dx) * dy));
    if (power > 0.f) return false;
    G = __expf(power);
    alpha = fminf(GFL_ALPHA_MAX, o * G);
    return alpha >= GFL_ALPHA_MIN;
}

// The pixel (fx, fy) of the calling lane walks list entries [start, end) front to back; whole workgroup of WALK_BATCH lanes.
//   stage(idx, slot)       lane `slot` puts entry idx into the caller's LDS arrays (between two barriers)
//   head(j, p0, p1)        the staged record j: p0 = u, v, conic a, conic b; p1 = conic c, opacity, and two of the caller's
//   add(j, w, p1, count)   the splat contributes with weight w = alpha T; count = its 1-based position in the list
// A splat whose alpha would take T below T_MIN ends the pixel BEFORE it is added; the walk ends when every pixel has.
// T is updated in place (start it at 1); lanes outside the image pass inside = false and only stage.
template <typename Stage, typename Head, typename Add>
__device__ __forceinline__ void operator_tile_walk(int start, int end, bool inside, float fx, float fy, float& T,
                                                   Stage&& stage, Head&& head, Add&& add) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    bool done = !inside;
    for (int base = start; base < end; base += WALK_BATCH) {
        if (__syncthreads_and(done)) break;
        const int idx = base + tid;
        if (idx < end) stage(idx, tid);
        __syncthreads();
        const int cnt = min(WALK_BATCH, end - base);
        if (!done) {
            for (int j = 0; j < cnt; ++j) {
                float4 p0, p1;
                head(j, p0, p1);
                float alpha, G;
                if (!splat_alpha(p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, fx, fy, alpha, G)) continue;
                const float test_T = T * (1.f - alpha);
                if (test_T < GFL_T_MIN) { done = true; break; }
                add(j, alpha * T, p1, base - start + j + 1);
                T = test_T;
            }
        }
    }
}

// the head of fit record g, (u, v, A, B | C, opacity), as the fused forward wrote it: one float4 and one float2 load
__device__ __forceinline__ void fit_record_head(const float* __restrict__ rec, int g, float4& p0, float2& co) {
    const float* r = rec + (size_t)g * REC;
    p0 = *reinterpret_cast<const float4*>(r);
    co = *reinterpret_cast<const float2*>(r + 4);
}

// list entries [start, end) of a tile; without rows there are no lists (tile_range may be null)
struct ListRange { int start, end; };
__device__ __forceinline__ ListRange list_range(const int32_t* __restrict__ tile_range, int tile, int n) {
    if (n <= 0) return {0, 0};
    return {tile_range[2 * tile], tile_range[2 * tile + 1]};
}

// entry points that take a fit's records and lists: rows are read as float4 + float2, the lists as int32
inline bool list_state_ok(const float* rec, int n, const int32_t* ids, const int32_t* tile_range) {
    if (n > 0 && (!rec || !ids || !tile_range)) return false;
    return !(((uintptr_t)rec & 15) || ((uintptr_t)ids & 3) || ((uintptr_t)tile_range & 3));
}

}  // namespace gfl
