// Dense optical flow of a frame pair and its end-point error (gfl_flow_pair; include/gflow_hip.h, gflow_amd/flow.py).
//
// The motion field the fitted splats imply from frame A to frame B, on A's pixel grid: every pixel walks A's sorted tile
// list front to back under exactly the operator blend's rule (operator_tile_walk of gfl_splat_alpha.hpp, the blend's own
// loop) with the splat's own motion d = uv_B - uv_A as the feature,
//   w = alpha T;   num += w d, den += w   for rows that still exist in B (row < n_b, depth_b != 0);   T *= 1 - alpha always
// and F = num / den where den >= min_weight.  Against gt_flow the end-point error in float64, summed per class of
// move_mask.
//
// Launch 1: one workgroup (4 wave64) per 16x16 tile, A WAVE OWNS AN 8x8 BLOCK as in blend_fwd_kernel; the tile's list is
// staged through LDS WALK_BATCH records at a time (two wide LDS reads and a narrow one per splat, all lanes the same address
// = broadcast).  The counts of a wave are popcounts of ballots, its epe sum a fixed xor tree over the lanes; the four waves'
// 18 numbers are added in wave order and stored as the tile's row of the workspace.  Launch 2: one workgroup, thread t
// adds the rows t, t + 256, ... in that order, thread k < 18 then adds the 256 partial sums of number k in thread order.
// No atomics: the same bits on every call.
#pragma clang fp contract(off)
#include "gfl_common.hpp"
#include "gfl_splat_alpha.hpp"

namespace gfl {

constexpr int FLOW_NV = 18;                         // 3 classes x {n_pixels, n_valid, epe_sum, n<1, n<3, n<5}

__global__ void __launch_bounds__(256) flow_pair_kernel(
        const float* __restrict__ rec_a, int n_a, const int32_t* __restrict__ ids, const int32_t* __restrict__ tile_range,
        const float* __restrict__ uv_b, int uv_b_stride, const float* __restrict__ depth_b, int depth_b_stride, int n_b,
        const float* __restrict__ gt_flow, const uint8_t* __restrict__ move_mask, int W, int H, int gx, float min_weight,
        double* __restrict__ partial, float* __restrict__ flow_out, uint8_t* __restrict__ valid_out) {
    __shared__ float4 s_p0[WALK_BATCH];             // u, v, conic a, conic b
    __shared__ float4 s_p1[WALK_BATCH];             // conic c, opacity, dx, dy
    __shared__ float s_has[WALK_BATCH];             // 1: the row has a future, 0: it only occludes
    __shared__ double s_red[4][FLOW_NV];
    const int tile = blockIdx.x;
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const auto [lx, ly, px, py, inside] = tile_pixel(tx, ty, W, H);
    const float fx = pixf(px), fy = pixf(py);
    const auto [start, end] = list_range(tile_range, tile, n_a);

    float T = 1.f, nx = 0.f, ny = 0.f, den = 0.f;
    operator_tile_walk(
        start, end, inside, fx, fy, T,
        [&](int idx, int slot) {
            const int g = ids[idx];
            float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f), p1 = make_float4(0.f, 0.f, 0.f, 0.f);      // (opacity 0: skipped)
            float has = 0.f;
            if ((unsigned)g < (unsigned)n_a) {
                float2 co;
                fit_record_head(rec_a, g, p0, co);
                float dx = 0.f, dy = 0.f;
                if (g < n_b && depth_b[(size_t)g * depth_b_stride] != 0.f) {
                    const float* q = uv_b + (size_t)g * uv_b_stride;
                    dx = q[0] - p0.x;
                    dy = q[1] - p0.y;
                    has = 1.f;
                }
                p1 = make_float4(co.x, co.y, dx, dy);
            }
            s_p0[slot] = p0;
            s_p1[slot] = p1;
            s_has[slot] = has;
        },
        [&](int j, float4& p0, float4& p1) { p0 = s_p0[j]; p1 = s_p1[j]; },
        [&](int j, float w, const float4& p1, int) {
            if (s_has[j] != 0.f) {                  // (the same for every lane)
                nx = fmaf(w, p1.z, nx);
                ny = fmaf(w, p1.w, ny);
                den += w;
            }
        });

    // the pixel's flow, its error and its class
    const size_t pix = inside ? (size_t)py * W + px : 0;
    float2 gt = make_float2(0.f, 0.f);
    int cls = 0;                                    // 0: no mask, 1: still, 2: moving
    if (inside) {
        gt = reinterpret_cast<const float2*>(gt_flow)[pix];
        if (move_mask) cls = move_mask[pix] ? 2 : 1;
    }
    const bool valid = inside && den >= min_weight && isfinite(gt.x) && isfinite(gt.y);
    float Fx = 0.f, Fy = 0.f;
    double epe = 0.0;
    if (valid) {
        Fx = nx / den;
        Fy = ny / den;
        const double ex = (double)Fx - (double)gt.x, ey = (double)Fy - (double)gt.y;
        const double exx = ex * ex, eyy = ey * ey;
        epe = sqrt(exx + eyy);
    }
    if (inside) {
        if (flow_out) reinterpret_cast<float2*>(flow_out)[pix] = make_float2(Fx, Fy);
        if (valid_out) valid_out[pix] = valid ? 1 : 0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const bool in_c = inside && (c == 0 || cls == c);
        const bool v_c = in_c && valid;
        const double n_px = (double)__popcll(__ballot(in_c));
        const double n_v = (double)__popcll(__ballot(v_c));
        const double n1 = (double)__popcll(__ballot(v_c && epe < 1.0));
        const double n3 = (double)__popcll(__ballot(v_c && epe < 3.0));
        const double n5 = (double)__popcll(__ballot(v_c && epe < 5.0));
        const double e = wave_sum_f64(v_c ? epe : 0.0);
        if (lane == 0) {
            double* row = &s_red[wave][6 * c];
            row[0] = n_px; row[1] = n_v; row[2] = e; row[3] = n1; row[4] = n3; row[5] = n5;
        }
    }
    __syncthreads();
    if (tid < FLOW_NV)
        partial[(size_t)tile * FLOW_NV + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

__global__ void __launch_bounds__(256) flow_fold_kernel(const double* __restrict__ partial, int tiles,
                                                        double* __restrict__ row) {
    __shared__ double red[256][FLOW_NV + 1];
    const int tid = threadIdx.x;
    double acc[FLOW_NV];
#pragma unroll
    for (int k = 0; k < FLOW_NV; ++k) acc[k] = 0.0;
    for (int t = tid; t < tiles; t += 256) {
#pragma unroll
        for (int k = 0; k < FLOW_NV; ++k) acc[k] += partial[(size_t)t * FLOW_NV + k];
    }
#pragma unroll
    for (int k = 0; k < FLOW_NV; ++k) red[tid][k] = acc[k];
    __syncthreads();
    if (tid < FLOW_NV) {
        double s = 0.0;
        for (int t = 0; t < 256; ++t) s += red[t][tid];
        row[tid] = s;
    }
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_flow_workspace_bytes(int W, int H) {
    if (W < 1 || H < 1) return 0;
    const size_t tiles = tile_grid(W, H).tiles();
    if (tiles > (size_t)LIST_MAX_TILES) return 0;
    return tiles * FLOW_NV * sizeof(double);
}

int gfl_flow_pair(const float* rec_a, int n_a, const int32_t* ids, const int32_t* tile_range, const float* uv_b,
                  int uv_b_stride, const float* depth_b, int depth_b_stride, int n_b, const float* gt_flow,
                  const uint8_t* move_mask, int W, int H, float min_weight, int pair, int n_pairs, double* sums,
                  float* flow_out, uint8_t* valid_out, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (W < 1 || H < 1 || n_a < 0 || n_b < 0 || pair < 0 || pair >= n_pairs) return GFL_ERR_INVALID;
    if (!(min_weight > 0.f && min_weight <= 1.f)) return GFL_ERR_INVALID;                 // (a NaN is refused too)
    if (uv_b_stride < 2 || depth_b_stride < 1) return GFL_ERR_INVALID;
    const size_t need = gfl_flow_workspace_bytes(W, H);
    if (need == 0) return GFL_ERR_INVALID;                                                // more than 16384 tiles
    if (!gt_flow || !sums || !workspace || workspace_bytes < need) return GFL_ERR_INVALID;
    if (!list_state_ok(rec_a, n_a, ids, tile_range)) return GFL_ERR_INVALID;
    if (n_a > 0 && n_b > 0 && (!uv_b || !depth_b)) return GFL_ERR_INVALID;
    if (((uintptr_t)gt_flow & 7) || ((uintptr_t)flow_out & 7) || ((uintptr_t)workspace & 7)) return GFL_ERR_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const auto [gx, gy, tiles] = tile_grid(W, H);
    double* partial = (double*)workspace;
    flow_pair_kernel<<<tiles, 256, 0, s>>>(rec_a, n_a, ids, tile_range, uv_b, uv_b_stride, depth_b, depth_b_stride, n_b,
                                           gt_flow, move_mask, W, H, gx, min_weight, partial, flow_out, valid_out);
    int rc = check_launch();
    if (rc != GFL_OK) return rc;
    flow_fold_kernel<<<1, 256, 0, s>>>(partial, tiles, sums + (size_t)pair * FLOW_NV);
    return check_launch();
}

}  // extern "C"
