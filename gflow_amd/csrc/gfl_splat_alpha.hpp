// alpha of one splat at one pixel: the one statement of the operator blend's rule, shared by every kernel that walks a
// sorted tile list under it (gfl_blend.hip forward and backward, gfl_flow.hip) -- a variant build of the rasteriser
// constants then changes all of them together.
#pragma once
#include "gfl_common.hpp"

namespace gfl {

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

}  // namespace gfl
