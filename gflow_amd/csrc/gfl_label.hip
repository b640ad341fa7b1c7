// Object labels through a clip fit (gfl_label_frame, gfl_label_assign; include/gflow_hip.h, gflow_amd/propagation.py).
//
// gfl_label_frame: the label map the labelled splats of one frame imply.  Every pixel walks its tile's sorted list front to
// back under exactly the operator blend's rule (operator_tile_walk of gfl_splat_alpha.hpp, the blend's own loop), as
// flow_pair_kernel does, with the splat's class as the feature:
//   w = alpha T;   acc[label] += w   for rows that carry a label;   T *= 1 - alpha always
// and the pixel's label is the class of the largest sum where the sums together reach min_weight.
//
// One workgroup (4 wave64) per 16x16 tile, A WAVE OWNS AN 8x8 BLOCK; the tile's list is staged through LDS WALK_BATCH
// records at a time: two wide LDS reads per splat (all lanes the same address = broadcast), the label -- already resolved
// to "a class below K, or 255" -- rides in the second one.  Within a step of the walk the label is the same for every
// lane: it is moved to a scalar register and the accumulator is chosen by a UNIFORM branch over unrolled cases, so the
// sums are K named registers and never an indexed array.  One kernel per K <= 4 / 8 / 16.  No atomics, no reduction
// across lanes: the same bits on every call.
//
// gfl_label_assign: a lane per row; an unlabelled row takes the label of the pixel its centre lies on.
#pragma clang fp contract(off)
#include "gfl_common.hpp"
#include "gfl_splat_alpha.hpp"

namespace gfl {

constexpr int LABEL_NONE = 255;                     // the canonical "unlabelled"
constexpr int LABEL_MAX_K = 16;

// acc[label] += w for a label that is the same in every lane (a scalar register): a uniform branch to one add
template <int KMAX>
__device__ __forceinline__ void add_to_class(float (&acc)[KMAX], int label, float w) {
#define GFL_LABEL_CASE(k) case k: if constexpr (k < KMAX) acc[k < KMAX ? k : 0] += w; break;
    switch (label) {
        GFL_LABEL_CASE(0) GFL_LABEL_CASE(1) GFL_LABEL_CASE(2) GFL_LABEL_CASE(3)
        GFL_LABEL_CASE(4) GFL_LABEL_CASE(5) GFL_LABEL_CASE(6) GFL_LABEL_CASE(7)
        GFL_LABEL_CASE(8) GFL_LABEL_CASE(9) GFL_LABEL_CASE(10) GFL_LABEL_CASE(11)
        GFL_LABEL_CASE(12) GFL_LABEL_CASE(13) GFL_LABEL_CASE(14) GFL_LABEL_CASE(15)
        default: break;                             // unlabelled: the row only occludes
    }
#undef GFL_LABEL_CASE
}

template <int KMAX>
__global__ void __launch_bounds__(256) label_frame_kernel(
        const float* __restrict__ rec, int n, const int32_t* __restrict__ ids, const int32_t* __restrict__ tile_range,
        const uint8_t* __restrict__ labels, int n_labels, int K, int W, int H, int gx, float min_weight, int unknown,
        uint8_t* __restrict__ label_out, float* __restrict__ conf_out) {
    __shared__ float4 s_p0[WALK_BATCH];             // u, v, conic a, conic b
    __shared__ float4 s_p1[WALK_BATCH];             // conic c, opacity, the label (an int's bits), -
    const int tile = blockIdx.x;
    const int tx = tile % gx, ty = tile / gx;
    const auto [lx, ly, px, py, inside] = tile_pixel(tx, ty, W, H);
    const float fx = pixf(px), fy = pixf(py);
    const auto [start, end] = list_range(tile_range, tile, n);

    float T = 1.f;
    float acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
    operator_tile_walk(
        start, end, inside, fx, fy, T,
        [&](int idx, int slot) {
            const int g = ids[idx];
            float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f);                                             // (opacity 0: skipped)
            float4 p1 = make_float4(0.f, 0.f, __int_as_float(LABEL_NONE), 0.f);
            if ((unsigned)g < (unsigned)n) {
                float2 co;
                fit_record_head(rec, g, p0, co);
                int lab = g < n_labels ? (int)labels[g] : LABEL_NONE;
                if (lab >= K) lab = LABEL_NONE;
                p1 = make_float4(co.x, co.y, __int_as_float(lab), 0.f);
            }
            s_p0[slot] = p0;
            s_p1[slot] = p1;
        },
        [&](int j, float4& p0, float4& p1) { p0 = s_p0[j]; p1 = s_p1[j]; },
        [&](int, float w, const float4& p1, int) {
            add_to_class<KMAX>(acc, __builtin_amdgcn_readfirstlane(__float_as_int(p1.z)), w);         // (the same for every lane)
        });

    if (!inside) return;
    float den = 0.f, best = 0.f;
    int arg = 0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
            den = k == 0 ? acc[0] : den + acc[k];
            if (k == 0 || acc[k] > best) { best = acc[k]; arg = k; }           // (strict: the smallest k among equals)
        }
    }
    const bool known = den >= min_weight;
    const size_t pix = (size_t)py * W + px;
    label_out[pix] = (uint8_t)(known ? arg : unknown);
    if (conf_out) conf_out[pix] = known ? best / den : 0.f;
}

__global__ void __launch_bounds__(256) label_assign_kernel(const float* __restrict__ rec, int n,
                                                           const uint8_t* __restrict__ map, int W, int H,
                                                           uint8_t* __restrict__ labels) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n || labels[j] != LABEL_NONE) return;
    const float* r = rec + (size_t)j * REC;
    const float u = r[0], v = r[1], depth = r[9];
    // geometry.within: strict on both sides, false for NaN
    if (depth != 0.f && u > 0.f && u < (float)(W - 1) && v > 0.f && v < (float)(H - 1)) {
        const uint8_t m = map[(size_t)(int)v * W + (int)u];                    // (0 <= (int)u <= W - 2: truncation, as .long())
        if (m != LABEL_NONE) labels[j] = m;
    }
}

}  // namespace gfl

using namespace gfl;

extern "C" {

int gfl_label_frame(const float* rec, int n, const int32_t* ids, const int32_t* tile_range, const uint8_t* labels,
                    int n_labels, int K, int W, int H, float min_weight, int unknown, uint8_t* label_out, float* conf_out,
                    gfl_stream_t stream) {
    if (K < 2 || K > LABEL_MAX_K || W < 1 || H < 1 || n < 0 || n_labels < 0 || n_labels > n) return GFL_ERR_INVALID;
    if (!(min_weight > 0.f && min_weight <= 1.f)) return GFL_ERR_INVALID;                 // (a NaN is refused too)
    if (unknown < 0 || unknown > 255) return GFL_ERR_INVALID;
    const TileGrid grid = tile_grid(W, H);
    if (grid.tiles() > (size_t)LIST_MAX_TILES) return GFL_ERR_INVALID;
    if (!label_out) return GFL_ERR_INVALID;
    if (!list_state_ok(rec, n, ids, tile_range)) return GFL_ERR_INVALID;
    if (n_labels > 0 && !labels) return GFL_ERR_INVALID;
    if ((uintptr_t)conf_out & 3) return GFL_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
#define GFL_LABEL_LAUNCH(KMAX)                                                                                   \
    label_frame_kernel<KMAX><<<grid.T, 256, 0, s>>>(rec, n, ids, tile_range, labels, n_labels, K, W, H, grid.gx, \
                                                    min_weight, unknown, label_out, conf_out)
    if (K <= 4) GFL_LABEL_LAUNCH(4);
    else if (K <= 8) GFL_LABEL_LAUNCH(8);
    else GFL_LABEL_LAUNCH(16);
#undef GFL_LABEL_LAUNCH
    return check_launch();
}

int gfl_label_assign(const float* rec, int n, const uint8_t* map, int W, int H, uint8_t* labels_inout, gfl_stream_t stream) {
    if (W < 1 || H < 1 || n < 0) return GFL_ERR_INVALID;
    if (n == 0) return GFL_OK;
    if (!rec || !map || !labels_inout || ((uintptr_t)rec & 3)) return GFL_ERR_INVALID;
    label_assign_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(rec, n, map, W, H, labels_inout);
    return check_launch();
}

}  // extern "C"
