// Reconstruction score of one frame on the device (gfl_recon_frame; include/gflow_hip.h, gflow_amd/quality.py).
//
// What the reference's benchmark computes with piqa.PSNR() / piqa.SSIM() on the saved PNG (gflow/benchmark.py:191-230): the
// prediction is the saved byte k = uint8(clamp(x, 0, 1) * 255) read back as (float)k / 255.0f, the target is clamp(gt, 0, 1);
// everything after that is float64.  Per frame two sums: the squared error over all 3 H W values, and the SSIM map (11-tap
// normalised Gaussian window of sigma 1.5, no padding, C1 = 1e-4, C2 = 9e-4) over the 3 (H - 10)(W - 10) window positions.
//
// Grid (RC_TW-column tiles, RC_TH-row tiles of WINDOW POSITIONS, 3 channels).  A workgroup
//   1. stages its tile's (RC_TH + 10) x (RC_TW + 10) pixels of both images in LDS as doubles (a window position (y, x)
//      covers the pixels y .. y + 10, x .. x + 10: the tile plus a 5-pixel halo around the windows' centres) and sums the
//      squared error of the pixels it owns -- the tile's own RC_TH x RC_TW, and for the last tile of a direction the rest
//      of the image, so that every pixel is counted once;
//   2. row pass: the five maps x, y, x^2, y^2, xy under the window along x;
//   3. column pass: the window along y, the SSIM map, the sum of its valid positions;
//   4. folds the two per-thread sums in a fixed tree and writes them to its slot of the workspace.
// A second one-workgroup launch folds the slots in a fixed order into sums[frame].  No atomics: the same bits on every call.
#include <cmath>

#include "gfl_common.hpp"

namespace gfl {

constexpr int RC_BLOCK = 256;
constexpr int RC_TW = 32, RC_TH = 16;                       // window positions per tile
constexpr int RC_K = 11, RC_HALO = RC_K - 1;
constexpr int RC_IW = RC_TW + RC_HALO, RC_IH = RC_TH + RC_HALO;
// static LDS: 2 * 26 * 42 * 8 + 5 * 26 * 32 * 8 + 2 * 256 * 8 = 54 848 bytes
static_assert((2 * RC_IH * RC_IW + 5 * RC_IH * RC_TW + 2 * RC_BLOCK) * sizeof(double) <= 64 * 1024, "LDS budget");

struct ReconWindow {
    double g[RC_K];
};

// the saved byte, read back: render2img's clamp, x 255 and truncation in float32, then uint8 / 255 in float32
__device__ __forceinline__ double recon_pred(float x) {
    const float c = fminf(fmaxf(x, 0.0f), 1.0f);
    const int k = (int)(c * 255.0f);
    return (double)((float)k / 255.0f);
}

// fixed tree over the block's threads; the result is in a[0], b[0]
__device__ __forceinline__ void recon_block_fold(double* a, double* b, int tid) {
    for (int s = RC_BLOCK / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            a[tid] += a[tid + s];
            b[tid] += b[tid + s];
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(RC_BLOCK) recon_tile_kernel(
        const float* __restrict__ render, const float* __restrict__ gt, int W, int H, ReconWindow win,
        double* __restrict__ partial) {
    __shared__ double X[RC_IH][RC_IW], Y[RC_IH][RC_IW];
    __shared__ double R5[5][RC_IH][RC_TW];
    __shared__ double red[2][RC_BLOCK];
    const int tid = threadIdx.x, ch = blockIdx.z;
    const int x0 = blockIdx.x * RC_TW, y0 = blockIdx.y * RC_TH;
    const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
    const float* plane = render + (size_t)ch * H * W;
    // 1. the pixels (zero outside the image: only window positions that are not valid read them)
    double sse = 0.0;
    for (int i = tid; i < RC_IH * RC_IW; i += RC_BLOCK) {
        const int r = i / RC_IW, c = i - r * RC_IW;
        const int y = y0 + r, x = x0 + c;
        double p = 0.0, g = 0.0;
        if (y < H && x < W) {
            const size_t at = (size_t)y * W + x;
            p = recon_pred(plane[at]);
            g = (double)fminf(fmaxf(gt[at * 3 + ch], 0.0f), 1.0f);
            if ((r < RC_TH || last_y) && (c < RC_TW || last_x)) {
                const double d = p - g;
                sse += d * d;
            }
        }
        X[r][c] = p;
        Y[r][c] = g;
    }
    __syncthreads();
    // 2. row pass
    for (int i = tid; i < RC_IH * RC_TW; i += RC_BLOCK) {
        const int r = i / RC_TW, c = i - r * RC_TW;
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < RC_K; ++k) {
            const double w = win.g[k], x = X[r][c + k], y = Y[r][c + k];
            a[0] += w * x;
            a[1] += w * y;
            a[2] += w * (x * x);
            a[3] += w * (y * y);
            a[4] += w * (x * y);
        }
#pragma unroll
        for (int m = 0; m < 5; ++m) R5[m][r][c] = a[m];
    }
    __syncthreads();
    // 3. column pass and the map
    double ssim = 0.0;
    for (int i = tid; i < RC_TH * RC_TW; i += RC_BLOCK) {
        const int r = i / RC_TW, c = i - r * RC_TW;
        if (y0 + r >= H - RC_HALO || x0 + c >= W - RC_HALO) continue;
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < RC_K; ++k) {
            const double w = win.g[k];
#pragma unroll
            for (int m = 0; m < 5; ++m) a[m] += w * R5[m][r + k][c];
        }
        const double C1 = 1e-4, C2 = 9e-4;
        const double mxx = a[0] * a[0], myy = a[1] * a[1], mxy = a[0] * a[1];
        const double sxx = a[2] - mxx, syy = a[3] - myy, sxy = a[4] - mxy;
        ssim += ((2.0 * mxy + C1) * (2.0 * sxy + C2)) / ((mxx + myy + C1) * (sxx + syy + C2));
    }
    // 4. the block's two sums
    red[0][tid] = sse;
    red[1][tid] = ssim;
    recon_block_fold(red[0], red[1], tid);
    if (tid == 0) {
        const size_t slot = ((size_t)ch * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * slot] = red[0][0];
        partial[2 * slot + 1] = red[1][0];
    }
}

// one workgroup: thread t sums the slots t, t + RC_BLOCK, ... in that order, then the fixed tree
__global__ void __launch_bounds__(RC_BLOCK) recon_fold_kernel(const double* __restrict__ partial, int n,
                                                             double* __restrict__ row) {
    __shared__ double red[2][RC_BLOCK];
    const int tid = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = tid; i < n; i += RC_BLOCK) {
        a += partial[2 * (size_t)i];
        b += partial[2 * (size_t)i + 1];
    }
    red[0][tid] = a;
    red[1][tid] = b;
    recon_block_fold(red[0], red[1], tid);
    if (tid == 0) {
        row[0] = red[0][0];
        row[1] = red[1][0];
    }
}

inline int recon_tiles_x(int W) { return (W - RC_HALO + RC_TW - 1) / RC_TW; }
inline int recon_tiles_y(int H) { return (H - RC_HALO + RC_TH - 1) / RC_TH; }

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_recon_workspace_bytes(int W, int H) {
    if (W < RC_K || H < RC_K) return 0;
    return (size_t)3 * recon_tiles_x(W) * recon_tiles_y(H) * 2 * sizeof(double);
}

int gfl_recon_frame(const float* render, const float* gt_rgb, int W, int H, int frame, int T, double* sums, void* workspace,
                    size_t workspace_bytes, gfl_stream_t stream) {
    if (W < RC_K || H < RC_K || frame < 0 || frame >= T) return GFL_ERR_INVALID;
    if (!render || !gt_rgb || !sums || !workspace) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_recon_workspace_bytes(W, H)) return GFL_ERR_INVALID;
    const int ntx = recon_tiles_x(W), nty = recon_tiles_y(H);
    if (nty > 65535) return GFL_ERR_INVALID;
    ReconWindow win;
    double total = 0.0;
    for (int i = 0; i < RC_K; ++i) {
        const double d = (double)(i - RC_K / 2);
        win.g[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        total += win.g[i];
    }
    for (int i = 0; i < RC_K; ++i) win.g[i] /= total;
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    recon_tile_kernel<<<dim3(ntx, nty, 3), RC_BLOCK, 0, s>>>(render, gt_rgb, W, H, win, partial);
    int rc = check_launch();
    if (rc != GFL_OK) return rc;
    recon_fold_kernel<<<1, RC_BLOCK, 0, s>>>(partial, 3 * ntx * nty, sums + 2 * (size_t)frame);
    return check_launch();
}

}  // extern "C"
