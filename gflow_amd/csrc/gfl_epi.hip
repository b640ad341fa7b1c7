// Move masks from the flow: a deterministic LMedS fit of the fundamental matrix and the Sampson-error mask
// (gfl_epi_fundamental, gfl_epi_mask; include/gflow_hip.h, gflow_amd/move_seg.py, tests/move_seg_ref.py).
//
// What the reference's utility/move_seg.py computes with cv2.findFundamentalMat(FM_LMEDS) and skimage.morphology, as this
// project's own algorithm (cv2's sampler and iteration rule are not observable: unpinned against cv2; the morphology is
// skimage's as recalled: unpinned too).  Correspondences are formed in float32 exactly as the script forms them; everything
// after that is float64, with every product and sum rounded on its own (no contraction), so that the numpy restatement
// evaluates the same expression.
//
// gfl_epi_fundamental
//   solve     one thread per hypothesis: Hartley-normalised 8-point, null vector by cyclic Jacobi on A^T A (9 x 9, fully
//             unrolled so that the matrices live in registers), rank 2 by Jacobi on F^T F, de-normalise, scale, sign
//   6 x (hist, select)   exact lower median of the Sampson errors per hypothesis by radix selection on their order keys,
//             11 bits a pass, 9 in the last: the errors are recomputed in every pass, never stored.  hist: grid (pixel
//             chunks, hypotheses), F and the 2048 bins in LDS, LDS integer atomics, one global integer atomic per
//             non-empty bin; select: one workgroup per hypothesis finds the bin that holds the wanted rank (pass 0 learns
//             the number of known pixels from the row's total).  Integer sums do not depend on their order: the same bits
//             on every call.
//   final     medians, the smallest (ties: lowest index), F_best
// gfl_epi_mask
//   err (Sampson error x ((H + W) / 2)^2 per pixel, the maximum by an integer atomic on the bit pattern), norm (err / max,
//   threshold), then erosions / dilations with disc footprints.
// The Jacobi, the tail of the 8-point fit, the Sampson error and the selection are gfl_epipolar.hpp's.
#include <algorithm>
#include <cmath>

#include "gfl_epipolar.hpp"

namespace gfl {

constexpr int EPI_BLOCK = 256;
constexpr int EPI_SOLVE_BLOCK = 64;
constexpr int EPI_PER_BLOCK = EPI_BLOCK * 16;                   // pixels per workgroup of the hist pass
constexpr int EPI_OPEN_R = 2, EPI_ERODE_R = 5, EPI_DILATE_R = 3;
static_assert(EPI_BLOCK == SELECT_BLOCK, "the hist pass flushes its bins with the selection's workgroup");
static_assert(SELECT_BINS * sizeof(uint32_t) + 9 * sizeof(double) <= 64 * 1024, "LDS budget");

struct EpiPoint {
    double x1, y1, x2, y2;
    bool known;
};

// move_seg.py:185-203 in float32: x1 = 2 (x + 0.5) / W - 1, x2 = x1 + 2 flow / (W - 1) (one rounding per operation).  Known:
// both components of x2 are finite (a non-finite flow, or one so large that 2 flow overflows float32, is not).
__host__ __device__ inline EpiPoint epi_point(const float* __restrict__ flow, int i, int W, int H) {
#pragma clang fp contract(off)
    const int y = i / W, x = i - y * W;
    const float fx = flow[2 * (size_t)i], fy = flow[2 * (size_t)i + 1];
    const float x1 = (2.0f * ((float)x + 0.5f)) / (float)W - 1.0f;
    const float y1 = (2.0f * ((float)y + 0.5f)) / (float)H - 1.0f;
    const float x2 = x1 + (2.0f * fx) / (float)(W - 1);
    const float y2 = y1 + (2.0f * fy) / (float)(H - 1);
    EpiPoint p;
    p.x1 = (double)x1; p.y1 = (double)y1; p.x2 = (double)x2; p.y2 = (double)y2;
    p.known = std::isfinite(x2) && std::isfinite(y2);
    return p;
}

// Hartley: centroid to 0, mean distance to sqrt(2).  Returns the scale; c is the centroid.
__host__ __device__ inline double epi_normalise(double (&x)[8], double (&y)[8], double& cx, double& cy) {
    cx = 0.0; cy = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) { cx += x[r]; cy += y[r]; }
    cx *= 0.125; cy *= 0.125;
    double d = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        x[r] -= cx; y[r] -= cy;
        d += sqrt(x[r] * x[r] + y[r] * y[r]);
    }
    const double s = sqrt(2.0) / (d * 0.125);
#pragma unroll
    for (int r = 0; r < 8; ++r) { x[r] *= s; y[r] *= s; }
    return s;
}

// The normalised 8-point fit of eight correspondences; F row-major, ||F||_F = 1, its entry of largest magnitude positive.
// Returns false (and F = 0) if F is not finite.
__host__ __device__ inline bool epi_solve8(double (&x1)[8], double (&y1)[8], double (&x2)[8], double (&y2)[8], double (&F)[9]) {
    double c1x, c1y, c2x, c2y;
    const double s1 = epi_normalise(x1, y1, c1x, c1y), s2 = epi_normalise(x2, y2, c2x, c2y);
    // A^T A of the rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]: x2^T F x1 = 0 with F row-major
    double M[81];
#pragma unroll
    for (int i = 0; i < 81; ++i) M[i] = 0.0;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const double a[9] = {x2[r] * x1[r], x2[r] * y1[r], x2[r], y2[r] * x1[r], y2[r] * y1[r], y2[r], x1[r], y1[r], 1.0};
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = i; j < 9; ++j) M[i * 9 + j] += a[i] * a[j];
    }
    const bool ok = fundamental_from_normal(M, s1, c1x, c1y, s2, c2x, c2y, F);
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = 0.0;
    }
    return ok;
}

// ---------------------------------------------------------------------------------------------------------- fundamental
__global__ void __launch_bounds__(EPI_SOLVE_BLOCK) epi_solve_kernel(const float* __restrict__ flow, int W, int H, int n,
                                                                    const int32_t* __restrict__ samples, int K,
                                                                    double* __restrict__ Fk, int32_t* __restrict__ degenerate) {
    const int k = blockIdx.x * EPI_SOLVE_BLOCK + threadIdx.x;
    if (k >= K) return;
    int idx[8];
    bool ok = true;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        idx[r] = samples[(size_t)k * 8 + r];
        ok = ok && idx[r] >= 0 && idx[r] < n;
    }
#pragma unroll
    for (int r = 1; r < 8; ++r)
#pragma unroll
        for (int q = 0; q < r; ++q) ok = ok && idx[r] != idx[q];
    double x1[8], y1[8], x2[8], y2[8], F[9];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        EpiPoint p;
        p.x1 = p.y1 = p.x2 = p.y2 = 0.0;
        p.known = false;
        if (ok) p = epi_point(flow, idx[r], W, H);             // (only indices inside the image are read)
        ok = ok && p.known;
        x1[r] = p.x1; y1[r] = p.y1; x2[r] = p.x2; y2[r] = p.y2;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = 0.0;
    if (ok) ok = epi_solve8(x1, y1, x2, y2, F);
#pragma unroll
    for (int i = 0; i < 9; ++i) Fk[(size_t)k * 9 + i] = F[i];
    degenerate[k] = ok ? 0 : 1;
}

// grid (pixel chunks, K).  Counts, per hypothesis, the errors whose key agrees with the prefix found so far, by digit.
__global__ void __launch_bounds__(EPI_BLOCK) epi_hist_kernel(const float* __restrict__ flow, int W, int H, int n,
                                                             const double* __restrict__ Fk,
                                                             const int32_t* __restrict__ degenerate,
                                                             const unsigned long long* __restrict__ prefix,
                                                             uint32_t* __restrict__ hist, int pass) {
    __shared__ double sF[9];
    __shared__ uint32_t bins[SELECT_BINS];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1);
    if (degenerate[k]) return;                                   // (the whole workgroup: the row stays zero)
    if (tid < 9) sF[tid] = Fk[(size_t)k * 9 + tid];
    for (int b = tid; b < (1 << select_width(pass)); b += EPI_BLOCK) bins[b] = 0;
    __syncthreads();
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = sF[i];
    const unsigned long long want = pass == 0 ? 0ull : prefix[k];
    const int start = blockIdx.x * EPI_PER_BLOCK, end = min(start + EPI_PER_BLOCK, n);   // (start < n: the grid is ceil(n / per))
    for (int base = start; base < end; base += EPI_BLOCK) {     // (the same trips for every lane: ballots inside)
        const int i = base + tid;
        bool active = false;
        uint32_t digit = 0;
        if (i < end) {
            const EpiPoint p = epi_point(flow, i, W, H);
            if (p.known) {
                const double e = sampson_error(F, p.x1, p.y1, p.x2, p.y2);
                __builtin_assume(__builtin_bit_cast(long long, e) >= 0);     // (>= +0: the key is the bit pattern, sign bit set)
                active = select_digit(order_key(e), want, pass, digit);
            }
        }
        select_lane_add(bins, active, digit, lane);
    }
    select_flush(bins, hist + (size_t)k * SELECT_BINS, pass);
}

// one workgroup: the medians, the smallest of them (the lowest index among equals), its F
__global__ void __launch_bounds__(EPI_BLOCK) epi_final_kernel(const double* __restrict__ Fk, const int32_t* __restrict__ degenerate,
                                                              const unsigned long long* __restrict__ prefix, int K,
                                                              double* __restrict__ medians, double* __restrict__ F_best,
                                                              int32_t* __restrict__ best) {
    __shared__ double val[EPI_BLOCK];
    __shared__ int arg[EPI_BLOCK];
    const int tid = threadIdx.x;
    double v = INFINITY;
    int a = -1;
    for (int k = tid; k < K; k += EPI_BLOCK) {
        const double m = degenerate[k] ? INFINITY : order_unkey(prefix[k]);
        if (medians) medians[k] = m;
        if (!degenerate[k] && (a < 0 || m < v)) { v = m; a = k; }    // (ascending k: the first of equal medians stays)
    }
    val[tid] = v;
    arg[tid] = a;
    for (int s = EPI_BLOCK / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) {
            const double v2 = val[tid + s];
            const int a2 = arg[tid + s];
            const int a1 = arg[tid];
            if (a2 >= 0 && (a1 < 0 || v2 < val[tid] || (v2 == val[tid] && a2 < a1))) { val[tid] = v2; arg[tid] = a2; }
        }
    }
    __syncthreads();
    const int b = arg[0];
    if (tid == 0) best[0] = b;
    if (tid < 9) F_best[tid] = b >= 0 ? Fk[(size_t)b * 9 + tid] : 0.0;
}

// ----------------------------------------------------------------------------------------------------------------- mask
__global__ void __launch_bounds__(EPI_BLOCK) epi_err_kernel(const float* __restrict__ flow, int W, int H, int n,
                                                            const double* __restrict__ Fdev, double fac2,
                                                            double* __restrict__ err, unsigned long long* __restrict__ max_bits) {
    __shared__ unsigned long long smax;
    if (threadIdx.x == 0) smax = 0ull;
    __syncthreads();
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = Fdev[i];
    unsigned long long mine = 0ull;
    for (int i = blockIdx.x * EPI_BLOCK + threadIdx.x; i < n; i += gridDim.x * EPI_BLOCK) {
        const EpiPoint p = epi_point(flow, i, W, H);
        double e = 0.0;
        if (p.known) {
            e = sampson_error(F, p.x1, p.y1, p.x2, p.y2) * fac2;
            if (!std::isfinite(e)) e = 0.0;                      // (an F that is not finite)
        }
        err[i] = e;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(e);   // e >= +0: ordered like the values
        mine = bits > mine ? bits : mine;
    }
    if (mine) atomicMax(&smax, mine);
    __syncthreads();
    if (threadIdx.x == 0 && smax) atomicMax(max_bits, smax);
}

__global__ void __launch_bounds__(EPI_BLOCK) epi_norm_kernel(const float* __restrict__ flow, int W, int H, int n,
                                                             const double* __restrict__ err,
                                                             const unsigned long long* __restrict__ max_bits, double threshold,
                                                             float* __restrict__ err_norm, uint8_t* __restrict__ mask) {
    const double m = __longlong_as_double((long long)*max_bits);
    for (int i = blockIdx.x * EPI_BLOCK + threadIdx.x; i < n; i += gridDim.x * EPI_BLOCK) {
        double r = 0.0;
        bool set = false;
        if (m > 0.0 && epi_point(flow, i, W, H).known) {
            r = err[i] / m;
            set = r > threshold;
        }
        if (err_norm) err_norm[i] = (float)r;
        mask[i] = set ? 255 : 0;
    }
}

// disc footprint dx^2 + dy^2 <= r^2; erosion: every pixel of the footprint inside the image is set (outside counts as
// set); dilation: any is (outside counts as unset)
__global__ void __launch_bounds__(EPI_BLOCK) epi_morph_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int W,
                                                              int H, int n, int r, int erode) {
    for (int i = blockIdx.x * EPI_BLOCK + threadIdx.x; i < n; i += gridDim.x * EPI_BLOCK) {
        const int y = i / W, x = i - y * W;
        bool all = true, any = false;
        for (int dy = -r; dy <= r; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -r; dx <= r; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W || dx * dx + dy * dy > r * r) continue;
                const bool s = src[(size_t)yy * W + xx] != 0;
                all = all && s;
                any = any || s;
            }
        }
        dst[i] = (erode ? all : any) ? 255 : 0;
    }
}

// the workspace of both entries: the regions of gfl_epi_mask first (they do not depend on K)
struct EpiWorkspace {
    double* err; unsigned long long* max_bits; uint8_t* mask; uint8_t* tmp;
    double* Fk; int32_t* degenerate; Select sel;
};
inline EpiWorkspace epi_carve(Arena& a, int W, int H, int K) {
    const size_t n = (size_t)W * H;
    EpiWorkspace w;
    w.err = a.take<double>("err", n);
    w.max_bits = a.take<unsigned long long>("max_bits", 1);
    w.mask = a.take<uint8_t>("mask", n);
    w.tmp = a.take<uint8_t>("tmp", n);
    w.Fk = a.take<double>("F", (size_t)K * 9);
    w.degenerate = a.take<int32_t>("degenerate", K);
    w.sel = select_carve(a, K);
    return w;
}
// (2^30 pixels at most: pixel indices and the strides added to them stay inside an int)
inline bool epi_size_ok(int W, int H) { return W >= 2 && H >= 2 && (size_t)W * H >= 8 && (size_t)W * H <= ((size_t)1 << 30); }
inline int epi_stride_grid(int n) { return std::min((n + EPI_BLOCK - 1) / EPI_BLOCK, 2048); }

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_epi_workspace_bytes(int W, int H, int K) {
    if (!epi_size_ok(W, H) || K < 1 || K > 65535) return 0;
    Arena a;
    epi_carve(a, W, H, K);
    return a.off;
}

int gfl_epi_fundamental(const float* flow, int W, int H, const int32_t* samples, int K, double* F_all, double* medians,
                        double* F_best, int32_t* best, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!epi_size_ok(W, H) || K < 1 || K > 65535) return GFL_ERR_INVALID;
    if (!flow || !samples || !F_best || !best || !workspace) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_epi_workspace_bytes(W, H, K)) return GFL_ERR_WORKSPACE;
    Arena a;
    a.base = (char*)workspace;
    const EpiWorkspace w = epi_carve(a, W, H, K);
    const int n = W * H;
    double* Fk = F_all ? F_all : w.Fk;
    hipStream_t s = (hipStream_t)stream;
    int rc = check(hipMemsetAsync(w.sel.hist, 0, (size_t)K * SELECT_BINS * sizeof(uint32_t), s));
    if (rc != GFL_OK) return rc;
    epi_solve_kernel<<<(K + EPI_SOLVE_BLOCK - 1) / EPI_SOLVE_BLOCK, EPI_SOLVE_BLOCK, 0, s>>>(flow, W, H, n, samples, K, Fk,
                                                                                           w.degenerate);
    if ((rc = check_launch()) != GFL_OK) return rc;
    const int chunks = (n + EPI_PER_BLOCK - 1) / EPI_PER_BLOCK;
    for (int pass = 0; pass < SELECT_PASSES; ++pass) {
        epi_hist_kernel<<<dim3(chunks, K), EPI_BLOCK, 0, s>>>(flow, W, H, n, Fk, w.degenerate, w.sel.prefix, w.sel.hist, pass);
        if ((rc = check_launch()) != GFL_OK) return rc;
        select_launch(w.sel, K, pass, s);
        if ((rc = check_launch()) != GFL_OK) return rc;
    }
    epi_final_kernel<<<1, EPI_BLOCK, 0, s>>>(Fk, w.degenerate, w.sel.prefix, K, medians, F_best, best);
    return check_launch();
}

int gfl_epi_mask(const float* flow, int W, int H, const double* F, double threshold, float* err_norm, uint8_t* mask,
                 uint8_t* open, uint8_t* erode, uint8_t* dilate, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!epi_size_ok(W, H) || !std::isfinite(threshold)) return GFL_ERR_INVALID;
    if (!flow || !F || !workspace) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_epi_workspace_bytes(W, H, 1)) return GFL_ERR_WORKSPACE;
    Arena a;
    a.base = (char*)workspace;
    const EpiWorkspace w = epi_carve(a, W, H, 1);
    const int n = W * H, grid = epi_stride_grid(n);
    const double fac = (double)(H + W) / 2.0;
    uint8_t* m = mask ? mask : w.mask;
    hipStream_t s = (hipStream_t)stream;
    int rc = check(hipMemsetAsync(w.max_bits, 0, sizeof(unsigned long long), s));
    if (rc != GFL_OK) return rc;
    epi_err_kernel<<<grid, EPI_BLOCK, 0, s>>>(flow, W, H, n, F, fac * fac, w.err, w.max_bits);
    if ((rc = check_launch()) != GFL_OK) return rc;
    epi_norm_kernel<<<grid, EPI_BLOCK, 0, s>>>(flow, W, H, n, w.err, w.max_bits, threshold, err_norm, m);
    if ((rc = check_launch()) != GFL_OK) return rc;
    if (open) {
        epi_morph_kernel<<<grid, EPI_BLOCK, 0, s>>>(m, w.tmp, W, H, n, EPI_OPEN_R, 1);
        if ((rc = check_launch()) != GFL_OK) return rc;
        epi_morph_kernel<<<grid, EPI_BLOCK, 0, s>>>(w.tmp, open, W, H, n, EPI_OPEN_R, 0);
        if ((rc = check_launch()) != GFL_OK) return rc;
    }
    if (erode) {
        epi_morph_kernel<<<grid, EPI_BLOCK, 0, s>>>(m, erode, W, H, n, EPI_ERODE_R, 1);
        if ((rc = check_launch()) != GFL_OK) return rc;
    }
    if (dilate) {
        epi_morph_kernel<<<grid, EPI_BLOCK, 0, s>>>(m, dilate, W, H, n, EPI_DILATE_R, 0);
        if ((rc = check_launch()) != GFL_OK) return rc;
    }
    return GFL_OK;
}

}  // extern "C"
