// Point tracking through a clip fit (gfl_track_anchor, gfl_track_frame; include/gflow_hip.h, gflow_amd/tracking.py).
//
// gfl_track_anchor: for every new query (x, y) in float64 the index of the splat whose float32 uv lies closest -- exactly
// np.argmin of ((uv - q) ** 2).sum(-1) in float64 (gflow/utils/tracking.py's find_closest_point).  The distance is
// dx * dx + dy * dy with every product and the sum rounded on their own (contraction off: an FMA moves near-ties to another
// index).  The minimum is taken over the key (distance, index) ordered lexicographically, with NaN distances in front of
// every number (np.argmin returns the first NaN): a total order, so the fold order never enters the result.
//
// Launch 1: grid (slices of the rows, blocks of TRK_QB queries).  A workgroup keeps its queries in registers (TRK_QPT per
// lane), streams its slice of uv through LDS as doubles, TRK_TILE rows at a time, and leaves the best (key, index) of the
// slice per query in the workspace.  The rows are split over up to TRK_MAX_SLICES workgroups so that a frame with a handful
// of new queries still spreads over the chip.  Launch 2: one lane per query folds the slices' partials and writes the
// anchor and the float64 shift q - uv[anchor].  No atomics.
//
// gfl_track_frame: one lane per anchored query writes its track (float32 of uv[anchor] + shift, the sum in float64) and its
// occlusion flag (|depth_map[rint(v)][rint(u)] - depth[anchor]| > threshold in float32; a pixel outside the image is
// occluded) into column `frame` of the [Q][T] outputs.
#pragma clang fp contract(off)
#include "gfl_common.hpp"

namespace gfl {

constexpr int TRK_BLOCK = 256;
constexpr int TRK_QPT = 2;                          // queries per lane
constexpr int TRK_QB = TRK_BLOCK * TRK_QPT;         // queries per workgroup
constexpr int TRK_TILE = 1024;                      // rows per LDS tile (16 KB of double2)
constexpr int TRK_MAX_SLICES = 256;

struct TrackSlices {
    int n, rows;
};

__host__ __device__ inline TrackSlices track_slices(int N) {
    int n = (N + TRK_TILE - 1) / TRK_TILE;
    if (n > TRK_MAX_SLICES) n = TRK_MAX_SLICES;
    if (n < 1) n = 1;
    const int rows = (N + n - 1) / n;
    return {rows > 0 ? (N + rows - 1) / rows : 1, rows > 0 ? rows : 1};       // (every slice holds at least one row)
}

// the distance as an ordered integer key: NaN -> 0 (in front of everything), d >= +0 -> its bits + 1
__device__ __forceinline__ unsigned long long dist_key(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d) & 0x7fffffffffffffffull;
    return b > 0x7ff0000000000000ull ? 0ull : b + 1ull;
}

__global__ void __launch_bounds__(TRK_BLOCK) track_anchor_partial_kernel(
        const float* __restrict__ uv, int stride, int N, const double* __restrict__ q, int n_new, int rows,
        unsigned long long* __restrict__ pkey, int* __restrict__ pidx) {
    __shared__ double2 tile[TRK_TILE];
    const int slice = blockIdx.x;
    const int qbase = blockIdx.y * TRK_QB + threadIdx.x;
    double qx[TRK_QPT], qy[TRK_QPT];
    unsigned long long bk[TRK_QPT];
    int bi[TRK_QPT];
#pragma unroll
    for (int k = 0; k < TRK_QPT; ++k) {
        const int qi = qbase + k * TRK_BLOCK;
        qx[k] = qi < n_new ? q[2 * (size_t)qi] : 0.0;
        qy[k] = qi < n_new ? q[2 * (size_t)qi + 1] : 0.0;
        bk[k] = ~0ull;
        bi[k] = 0x7fffffff;
    }
    const int r0 = slice * rows;
    const int r1 = min(N, r0 + rows);
    for (int t0 = r0; t0 < r1; t0 += TRK_TILE) {
        const int nt = min(TRK_TILE, r1 - t0);
        __syncthreads();
        for (int j = threadIdx.x; j < nt; j += TRK_BLOCK) {
            const float* p = uv + (size_t)(t0 + j) * stride;
            tile[j] = make_double2((double)p[0], (double)p[1]);
        }
        __syncthreads();
        for (int j = 0; j < nt; ++j) {
            const double2 r = tile[j];
#pragma unroll
            for (int k = 0; k < TRK_QPT; ++k) {
                const double dx = r.x - qx[k], dy = r.y - qy[k];
                const double ddx = dx * dx, ddy = dy * dy;
                const unsigned long long key = dist_key(ddx + ddy);
                if (key < bk[k]) {                  // (rows in ascending order: a tie keeps the lower index)
                    bk[k] = key;
                    bi[k] = t0 + j;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < TRK_QPT; ++k) {
        const int qi = qbase + k * TRK_BLOCK;
        if (qi < n_new) {
            pkey[(size_t)slice * n_new + qi] = bk[k];
            pidx[(size_t)slice * n_new + qi] = bi[k];
        }
    }
}

__global__ void __launch_bounds__(TRK_BLOCK) track_anchor_fold_kernel(
        const unsigned long long* __restrict__ pkey, const int* __restrict__ pidx, int n_slices, int n_new,
        const float* __restrict__ uv, int stride, const double* __restrict__ q, int32_t* __restrict__ anchor,
        double* __restrict__ shift) {
    const int qi = blockIdx.x * TRK_BLOCK + threadIdx.x;
    if (qi >= n_new) return;
    unsigned long long bk = ~0ull;
    int bi = 0x7fffffff;
    for (int s = 0; s < n_slices; ++s) {
        const unsigned long long k = pkey[(size_t)s * n_new + qi];
        const int i = pidx[(size_t)s * n_new + qi];
        if (k < bk || (k == bk && i < bi)) {
            bk = k;
            bi = i;
        }
    }
    anchor[qi] = bi;
    const float* p = uv + (size_t)bi * stride;
    shift[2 * (size_t)qi] = q[2 * (size_t)qi] - (double)p[0];
    shift[2 * (size_t)qi + 1] = q[2 * (size_t)qi + 1] - (double)p[1];
}

__global__ void __launch_bounds__(TRK_BLOCK) track_frame_kernel(
        const float* __restrict__ uv, int uv_stride, const float* __restrict__ depth, int depth_stride, int N,
        const float* __restrict__ depth_map, int W, int H, const int32_t* __restrict__ anchor,
        const double* __restrict__ shift, int n_anchored, int frame, int T, float thr, float* __restrict__ tracks,
        uint8_t* __restrict__ occluded) {
    const int qi = blockIdx.x * TRK_BLOCK + threadIdx.x;
    if (qi >= n_anchored) return;
    const int a = anchor[qi];
    float tx = __builtin_nanf(""), ty = __builtin_nanf("");
    uint8_t occ = 1;
    if (a >= 0 && a < N) {
        const float u = uv[(size_t)a * uv_stride], v = uv[(size_t)a * uv_stride + 1];
        const float d = depth[(size_t)a * depth_stride];
        tx = __double2float_rn((double)u + shift[2 * (size_t)qi]);
        ty = __double2float_rn((double)v + shift[2 * (size_t)qi + 1]);
        const float ru = rintf(u), rv = rintf(v);  // (half to even, as np.round)
        if (ru >= 0.f && ru < (float)W && rv >= 0.f && rv < (float)H) {
            const float dm = depth_map[(size_t)(int)rv * W + (int)ru];
            occ = fabsf(dm - d) > thr ? 1 : 0;
        }
    }
    const size_t o = (size_t)qi * T + frame;
    tracks[2 * o] = tx;
    tracks[2 * o + 1] = ty;
    occluded[o] = occ;
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_track_anchor_workspace_bytes(int n_new, int N) {
    if (n_new <= 0 || N <= 0) return 0;
    const TrackSlices s = track_slices(N);
    return (size_t)s.n * n_new * (sizeof(unsigned long long) + sizeof(int)) + 16;
}

int gfl_track_anchor(const float* uv, int uv_stride, int N, const double* query_xy, int n_new, int32_t* anchor,
                     double* shift_xy, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (n_new < 0 || N < 0 || uv_stride < 2) return GFL_ERR_INVALID;
    if (n_new == 0) return GFL_OK;
    if (N == 0 || !uv || !query_xy || !anchor || !shift_xy || !workspace) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_track_anchor_workspace_bytes(n_new, N)) return GFL_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const TrackSlices sl = track_slices(N);
    unsigned long long* pkey = (unsigned long long*)workspace;
    int* pidx = (int*)(pkey + (size_t)sl.n * n_new);
    const dim3 grid(sl.n, (n_new + TRK_QB - 1) / TRK_QB);
    track_anchor_partial_kernel<<<grid, TRK_BLOCK, 0, s>>>(uv, uv_stride, N, query_xy, n_new, sl.rows, pkey, pidx);
    track_anchor_fold_kernel<<<(n_new + TRK_BLOCK - 1) / TRK_BLOCK, TRK_BLOCK, 0, s>>>(pkey, pidx, sl.n, n_new, uv, uv_stride,
                                                                                       query_xy, anchor, shift_xy);
    return check_launch();
}

int gfl_track_frame(const float* uv, int uv_stride, const float* depth, int depth_stride, int N, const float* depth_map,
                    int W, int H, const int32_t* anchor, const double* shift_xy, int n_anchored, int frame, int T,
                    float occ_threshold, float* tracks, uint8_t* occluded, gfl_stream_t stream) {
    if (n_anchored < 0 || N < 0 || W <= 0 || H <= 0 || T <= 0 || frame < 0 || frame >= T || uv_stride < 2 || depth_stride < 1)
        return GFL_ERR_INVALID;
    if (n_anchored == 0) return GFL_OK;
    if (!uv || !depth || !depth_map || !anchor || !shift_xy || !tracks || !occluded) return GFL_ERR_INVALID;
    track_frame_kernel<<<(n_anchored + TRK_BLOCK - 1) / TRK_BLOCK, TRK_BLOCK, 0, (hipStream_t)stream>>>(
        uv, uv_stride, depth, depth_stride, N, depth_map, W, H, anchor, shift_xy, n_anchored, frame, T, occ_threshold, tracks,
        occluded);
    return check_launch();
}

}  // extern "C"
