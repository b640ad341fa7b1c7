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
//
// Backward tracking (gfl_track_history, gfl_track_backward): the frames BEFORE a query's frame.  gfl_track_history keeps a
// frame's (u, v) and the occlusion bit of EVERY row (track_frame's rule at the row's own pixel) in the clip's ragged history.
// gfl_track_backward then needs, per query of frame t and per frame i < t, the argmin over the rows n < N_i of the distance
// to uv_t[n]: a prefix argmin at the breakpoints N_0 <= N_1 <= ... of ONE pass over frame t's rows.  Launch 1: grid (slices
// of the rows below N_{t-1}, blocks of TRK_QB queries, query frame t); a workgroup whose block holds no query of frame t
// leaves at once (the queries come sorted by frame, so a block meets few frames -- but nothing depends on the order).  It
// works as the anchor's partial launch does, segment by segment: segment s is rows [N_{s-1}, N_s), cut to the slice, and its
// best (key, index) goes to the workspace at [slice][s][query] (nothing there: the sentinel).  Launch 2: one lane per
// (segment, query) folds the slices.  Launch 3: one lane per query takes the running lexicographic minimum over the
// segments in order and writes frame s's track, flag and back_anchor after segment s.  No atomics.
#pragma clang fp contract(off)
#include "gfl_common.hpp"

namespace gfl {

constexpr int TRK_BLOCK = 256;
constexpr int TRK_QPT = 2;                          // queries per lane
constexpr int TRK_QB = TRK_BLOCK * TRK_QPT;         // queries per workgroup
constexpr int TRK_TILE = 1024;                      // rows per LDS tile (16 KB of double2)
constexpr int TRK_MAX_SLICES = 256;
constexpr int TRKB_SLICES = 64;                     // backward pass: slices of a query frame's rows (the host does not know N)
constexpr unsigned long long TRK_NO_KEY = ~0ull;    // "no row": behind every distance
constexpr int TRK_NO_ROW = 0x7fffffff;

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

// the occlusion flag of a splat at (u, v) with depth d: float32, rint half to even (as np.round), outside the image: occluded
__device__ __forceinline__ uint8_t track_occluded(float u, float v, float d, const float* __restrict__ depth_map, int W, int H,
                                                  float thr) {
    const float ru = rintf(u), rv = rintf(v);
    if (ru >= 0.f && ru < (float)W && rv >= 0.f && rv < (float)H) {
        const float dm = depth_map[(size_t)(int)rv * W + (int)ru];
        return fabsf(dm - d) > thr ? 1 : 0;
    }
    return 1;
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
        occ = track_occluded(u, v, d, depth_map, W, H, thr);
    }
    const size_t o = (size_t)qi * T + frame;
    tracks[2 * o] = tx;
    tracks[2 * o + 1] = ty;
    occluded[o] = occ;
}

__global__ void __launch_bounds__(TRK_BLOCK) track_history_kernel(
        const float* __restrict__ uv, int uv_stride, const float* __restrict__ depth, int depth_stride, int N,
        const float* __restrict__ depth_map, int W, int H, float thr, float* __restrict__ hist_uv,
        uint8_t* __restrict__ hist_occ) {
    const int n = blockIdx.x * TRK_BLOCK + threadIdx.x;
    if (n >= N) return;
    const float u = uv[(size_t)n * uv_stride], v = uv[(size_t)n * uv_stride + 1];
    hist_uv[2 * (size_t)n] = u;
    hist_uv[2 * (size_t)n + 1] = v;
    hist_occ[n] = track_occluded(u, v, depth[(size_t)n * depth_stride], depth_map, W, H, thr);
}

// rows of frame s in the ragged history, as an int (a count below 0 or above INT_MAX: clamped)
__device__ __forceinline__ int track_rows_of(const int64_t* __restrict__ row_start, int s) {
    const int64_t n = row_start[s + 1] - row_start[s];
    return n < 0 ? 0 : n > 0x7ffffffe ? 0x7ffffffe : (int)n;
}

__global__ void __launch_bounds__(TRK_BLOCK) track_back_partial_kernel(
        const float* __restrict__ hist_uv, const int64_t* __restrict__ row_start, int T, const double* __restrict__ q,
        const int32_t* __restrict__ qframe, int Q, unsigned long long* __restrict__ pkey, int* __restrict__ pidx) {
    __shared__ double2 tile[TRK_TILE];
    const int t = blockIdx.z + 1;                   // the query frame this workgroup serves
    const int slice = blockIdx.x;
    const int qbase = blockIdx.y * TRK_QB + threadIdx.x;
    double qx[TRK_QPT], qy[TRK_QPT];
    bool mine[TRK_QPT];
    int any = 0;
#pragma unroll
    for (int k = 0; k < TRK_QPT; ++k) {
        const int qi = qbase + k * TRK_BLOCK;
        mine[k] = qi < Q && qframe[qi] == t;
        qx[k] = mine[k] ? q[2 * (size_t)qi] : 0.0;
        qy[k] = mine[k] ? q[2 * (size_t)qi + 1] : 0.0;
        any |= mine[k] ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;             // (uniform: the whole workgroup leaves)
    const float* __restrict__ uv = hist_uv + 2 * (size_t)row_start[t];
    // only rows an earlier frame already had can be chosen: n < N_{t-1}; never past frame t's own rows
    const int lim = min(track_rows_of(row_start, t - 1), track_rows_of(row_start, t));
    const int rows = max(1, (lim + TRKB_SLICES - 1) / TRKB_SLICES);
    const long long r0l = (long long)slice * rows;
    const int r0 = r0l < lim ? (int)r0l : lim;
    const int r1 = (int)min((long long)lim, (long long)r0 + rows);
    int prev = 0;                                   // N_{s-1}
    for (int s = 0; s < t; ++s) {
        const int ns = track_rows_of(row_start, s);
        const int a = max(r0, prev), b = min(r1, ns);
        prev = ns;
        unsigned long long bk[TRK_QPT];
        int bi[TRK_QPT];
#pragma unroll
        for (int k = 0; k < TRK_QPT; ++k) {
            bk[k] = TRK_NO_KEY;
            bi[k] = TRK_NO_ROW;
        }
        for (int t0 = a; t0 < b; t0 += TRK_TILE) {  // (a, b are uniform: every lane takes the barriers)
            const int nt = min(TRK_TILE, b - t0);
            __syncthreads();
            for (int j = threadIdx.x; j < nt; j += TRK_BLOCK) {
                const float2 p = *reinterpret_cast<const float2*>(uv + 2 * (size_t)(t0 + j));
                tile[j] = make_double2((double)p.x, (double)p.y);
            }
            __syncthreads();
            for (int j = 0; j < nt; ++j) {
                const double2 r = tile[j];
#pragma unroll
                for (int k = 0; k < TRK_QPT; ++k) {
                    const double dx = r.x - qx[k], dy = r.y - qy[k];
                    const double ddx = dx * dx, ddy = dy * dy;
                    const unsigned long long key = dist_key(ddx + ddy);
                    if (key < bk[k]) {              // (rows in ascending order: a tie keeps the lower index)
                        bk[k] = key;
                        bi[k] = t0 + j;
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < TRK_QPT; ++k) {
            const int qi = qbase + k * TRK_BLOCK;
            if (mine[k]) {
                const size_t o = ((size_t)slice * T + s) * Q + qi;
                pkey[o] = bk[k];
                pidx[o] = bi[k];
            }
        }
    }
}

// one lane per (segment, query): the segment's best over the slices, left in slice 0's place
__global__ void __launch_bounds__(TRK_BLOCK) track_back_fold_kernel(
        unsigned long long* __restrict__ pkey, int* __restrict__ pidx, int T, const int32_t* __restrict__ qframe, int Q) {
    const size_t e = (size_t)blockIdx.x * TRK_BLOCK + threadIdx.x;
    if (e >= (size_t)(T - 1) * Q) return;
    const int qi = (int)(e % Q), s = (int)(e / Q);
    const int t = qframe[qi];
    if (s >= t || t >= T) return;
    unsigned long long bk = TRK_NO_KEY;
    int bi = TRK_NO_ROW;
    for (int sl = 0; sl < TRKB_SLICES; ++sl) {
        const size_t o = ((size_t)sl * T + s) * Q + qi;
        const unsigned long long k = pkey[o];
        const int i = pidx[o];
        if (k < bk || (k == bk && i < bi)) {
            bk = k;
            bi = i;
        }
    }
    const size_t o = (size_t)s * Q + qi;
    pkey[o] = bk;
    pidx[o] = bi;
}

// one lane per query: the running minimum over the segments in order; frame s's outputs after segment s
__global__ void __launch_bounds__(TRK_BLOCK) track_back_write_kernel(
        const unsigned long long* __restrict__ pkey, const int* __restrict__ pidx, const float* __restrict__ hist_uv,
        const uint8_t* __restrict__ hist_occ, const int64_t* __restrict__ row_start, int T, const double* __restrict__ q,
        const int32_t* __restrict__ qframe, int Q, float* __restrict__ tracks, uint8_t* __restrict__ occluded,
        int32_t* __restrict__ back_anchor) {
    const int qi = blockIdx.x * TRK_BLOCK + threadIdx.x;
    if (qi >= Q) return;
    const int t = qframe[qi];
    if (t <= 0 || t >= T) return;
    const double x = q[2 * (size_t)qi], y = q[2 * (size_t)qi + 1];
    const int64_t base_t = row_start[t];
    const int nt = track_rows_of(row_start, t);
    unsigned long long bk = TRK_NO_KEY;
    int bi = TRK_NO_ROW;
    for (int s = 0; s < t; ++s) {
        const unsigned long long k = pkey[(size_t)s * Q + qi];
        const int i = pidx[(size_t)s * Q + qi];
        if (k < bk || (k == bk && i < bi)) {
            bk = k;
            bi = i;
        }
        float tx = __builtin_nanf(""), ty = __builtin_nanf("");
        uint8_t occ = 1;
        int32_t b = -1;
        if (bi < track_rows_of(row_start, s) && bi < nt) {         // (a row that exists in frame s and in frame t)
            b = bi;
            const float* here = hist_uv + 2 * (size_t)(row_start[s] + bi);
            const float* then = hist_uv + 2 * (size_t)(base_t + bi);
            const double sx = x - (double)then[0], sy = y - (double)then[1];
            tx = __double2float_rn((double)here[0] + sx);
            ty = __double2float_rn((double)here[1] + sy);
            occ = hist_occ[(size_t)(row_start[s] + bi)];
        }
        const size_t o = (size_t)qi * T + s;
        tracks[2 * o] = tx;
        tracks[2 * o + 1] = ty;
        occluded[o] = occ;
        if (back_anchor) back_anchor[o] = b;
    }
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

int gfl_track_history(const float* uv, int uv_stride, const float* depth, int depth_stride, int N, const float* depth_map,
                      int W, int H, float occ_threshold, float* hist_uv, uint8_t* hist_occ, gfl_stream_t stream) {
    if (N < 0 || W <= 0 || H <= 0 || uv_stride < 2 || depth_stride < 1) return GFL_ERR_INVALID;
    if (!uv || !depth || !depth_map || !hist_uv || !hist_occ) return GFL_ERR_INVALID;
    if (N == 0) return GFL_OK;
    track_history_kernel<<<(N + TRK_BLOCK - 1) / TRK_BLOCK, TRK_BLOCK, 0, (hipStream_t)stream>>>(
        uv, uv_stride, depth, depth_stride, N, depth_map, W, H, occ_threshold, hist_uv, hist_occ);
    return check_launch();
}

size_t gfl_track_backward_workspace_bytes(int Q, int T) {
    if (Q <= 0 || T <= 1) return 0;
    return (size_t)TRKB_SLICES * T * Q * (sizeof(unsigned long long) + sizeof(int)) + 16;
}

int gfl_track_backward(const float* hist_uv, const uint8_t* hist_occ, const int64_t* row_start, int T,
                       const double* query_xy, const int32_t* query_frame, int Q, float* tracks, uint8_t* occluded,
                       int32_t* back_anchor, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (T <= 0 || Q < 0) return GFL_ERR_INVALID;
    if (!hist_uv || !hist_occ || !row_start || !query_xy || !query_frame || !tracks || !occluded) return GFL_ERR_INVALID;
    if (Q == 0 || T == 1) return GFL_OK;            // (no query, or no frame before any query)
    if (T - 1 > 65535 || (Q + TRK_QB - 1) / TRK_QB > 65535) return GFL_ERR_INVALID;      // (the grid's y and z)
    if (!workspace || ((uintptr_t)hist_uv & 7)) return GFL_ERR_INVALID;              // (rows are read as float2)
    if (workspace_bytes < gfl_track_backward_workspace_bytes(Q, T)) return GFL_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* pkey = (unsigned long long*)workspace;
    int* pidx = (int*)(pkey + (size_t)TRKB_SLICES * T * Q);
    const dim3 grid(TRKB_SLICES, (Q + TRK_QB - 1) / TRK_QB, T - 1);
    track_back_partial_kernel<<<grid, TRK_BLOCK, 0, s>>>(hist_uv, row_start, T, query_xy, query_frame, Q, pkey, pidx);
    const size_t pairs = (size_t)(T - 1) * Q;
    track_back_fold_kernel<<<(unsigned)((pairs + TRK_BLOCK - 1) / TRK_BLOCK), TRK_BLOCK, 0, s>>>(pkey, pidx, T, query_frame, Q);
    track_back_write_kernel<<<(Q + TRK_BLOCK - 1) / TRK_BLOCK, TRK_BLOCK, 0, s>>>(
        pkey, pidx, hist_uv, hist_occ, row_start, T, query_xy, query_frame, Q, tracks, occluded, back_anchor);
    return check_launch();
}

}  // extern "C"
