// Depth and camera from the flows: classical two-view geometry for P pair problems at once (gfl_sfm_*; include/gflow_hip.h
// "depth and camera from the flows", gflow_amd/sfm.py, tests/sfm_ref.py).  NOT MASt3R and unpinned against it: depth comes from
// parallax alone, and what moves or is occluded is filled from its surroundings.
//
// gfl_sfm_refit        rounds x (Sampson error per pixel, exact lower median by radix selection, inliers, Hartley-normalised
//                      8-point fit over the inliers: three passes of per-workgroup float64 partials folded in a fixed order,
//                      then one thread per pair: 9 x 9 cyclic Jacobi, rank 2, de-normalise), then the errors, the median and
//                      the inlier bytes of the final F
// gfl_sfm_pose         E = K^T F K, the four (R, t), the cheirality vote in integers, the parallax median, the flags
// gfl_sfm_triangulate  per pixel: z1 (R x1) + t = z2 x2 by least squares; inverse depth and sin^2 of the parallax angle
// gfl_sfm_median       exact lower median of a / b over the pixels whose weights exceed w_min (baseline ratios, lambda, scale)
// gfl_sfm_fuse         the weighted mean of a frame's two inverse depths
// gfl_sfm_fill         pull-push fill, weighted Jacobi sweeps (several per launch on an LDS tile with a ring), depth
//
// The small dense algebra is float64 and one thread per pair does it; the per-pixel geometry is evaluated in float64 too (its
// cross products cancel: in float32 the error would grow with 1 / sin of the parallax angle) and stored as float32 -- the
// kernels stay bound by the bytes they move.  Fusion, fill and sweeps are float32, products and sums rounded separately.
// The only atomics are integer ones (histograms, votes, counts), whose sums do not depend on their order.
// The Jacobi, the tail of the 8-point fit, the Sampson error and the selection are gfl_epipolar.hpp's.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "gfl_epipolar.hpp"

namespace gfl {

constexpr int SFM_BLOCK = 256;
constexpr int SFM_PER_BLOCK = SFM_BLOCK * 16;                   // pixels per workgroup of a histogram or sum pass
constexpr int SFM_NSUM = 48;                                    // a row of partial sums (45 used)
constexpr int SFM_SUMS = 64;                                    // per pair: [0..4] count and coordinate sums, [5..6] distances, [8..52] A^T A
constexpr int SFM_MAX_LEVELS = 16;
constexpr int SFM_R = 32, SFM_S = 4, SFM_PPT = 4;               // fused sweeps: region side, sweeps per launch = ring, rows per lane
constexpr int SFM_MAX_Z = 65535;

static_assert(SFM_BLOCK == SELECT_BLOCK, "the hist pass flushes its bins with the selection's workgroup");

// ------------------------------------------------------------------------------------------ exact lower median, M rows
// val [M][n] float64, NaN = absent.  grid (chunks, M): counts the values whose key agrees with the prefix found so far, by digit.
__global__ void __launch_bounds__(SFM_BLOCK) sfm_hist_kernel(const double* __restrict__ val, int n,
                                                             const unsigned long long* __restrict__ prefix,
                                                             const uint32_t* __restrict__ count, uint32_t* __restrict__ hist,
                                                             int pass) {
    __shared__ uint32_t bins[SELECT_BINS];
    const int m = blockIdx.y, tid = threadIdx.x, lane = tid & (WAVE - 1);
    if (pass > 0 && count[m] == 0) return;                       // (the whole workgroup)
    for (int b = tid; b < (1 << select_width(pass)); b += SFM_BLOCK) bins[b] = 0;
    __syncthreads();
    const unsigned long long want = pass == 0 ? 0ull : prefix[m];
    const double* v = val + (size_t)m * n;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int base = start; base < end; base += SFM_BLOCK) {     // (the same trips for every lane: ballots inside)
        const int i = base + tid;
        bool active = false;
        uint32_t digit = 0;
        if (i < end) {
            const double e = v[i];
            if (e == e) active = select_digit(order_key(e), want, pass, digit);
        }
        select_lane_add(bins, active, digit, lane);
    }
    select_flush(bins, hist + (size_t)m * SELECT_BINS, pass);
}

static int sfm_run_select(const double* val, int M, int n, const Select& s, hipStream_t st) {
    int rc = check(hipMemsetAsync(s.hist, 0, (size_t)M * SELECT_BINS * sizeof(uint32_t), st));
    if (rc != GFL_OK) return rc;
    const int chunks = (n + SFM_PER_BLOCK - 1) / SFM_PER_BLOCK;
    for (int pass = 0; pass < SELECT_PASSES; ++pass) {
        sfm_hist_kernel<<<dim3(chunks, M), SFM_BLOCK, 0, st>>>(val, n, s.prefix, s.count, s.hist, pass);
        select_launch(s, M, pass, st);
    }
    return check_launch();
}

// ---------------------------------------------------------------------------------------------------------------- refit
struct SfmPoint { double x1, y1, x2, y2; bool known; };

// pixel centres at integer coordinates; x2 = x + flow in float64; known: both components of the flow are finite
__device__ inline SfmPoint sfm_point(const float* __restrict__ flow, int i, int W) {
    const int y = i / W, x = i - y * W;
    const float fx = flow[2 * (size_t)i], fy = flow[2 * (size_t)i + 1];
    SfmPoint p;
    p.x1 = (double)x; p.y1 = (double)y;
    p.x2 = (double)x + (double)fx; p.y2 = (double)y + (double)fy;
    p.known = std::isfinite(fx) && std::isfinite(fy);
    return p;
}

// val = the Sampson error of every known, unexcluded pixel, NaN elsewhere (and everywhere under an F that is not finite)
__global__ void __launch_bounds__(SFM_BLOCK) sfm_error_kernel(const float* __restrict__ flow, const double* __restrict__ Fp,
                                                              const uint8_t* __restrict__ exclude, int W, int n,
                                                              double* __restrict__ val) {
    const int p = blockIdx.y;
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = Fp[(size_t)p * 9 + i];
    const bool ok = finite9(F);
    const float* f = flow + (size_t)p * n * 2;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        double e = NAN;
        if (ok && !(exclude && exclude[(size_t)p * n + i])) {
            const SfmPoint pt = sfm_point(f, i, W);
            if (pt.known) {
                e = sampson_error(F, pt.x1, pt.y1, pt.x2, pt.y2);
                if (!std::isfinite(e)) e = NAN;
            }
        }
        val[(size_t)p * n + i] = e;
    }
}

// thr = max(k^2 median, e_floor); median and the number of usable pixels go out
__global__ void sfm_threshold_kernel(const unsigned long long* __restrict__ prefix, const uint32_t* __restrict__ count, int P,
                                     double k2, double e_floor, double* __restrict__ thr, double* __restrict__ median,
                                     int32_t* __restrict__ counts) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const double med = median_of(prefix, count, p);
    thr[p] = count[p] ? fmax(k2 * med, e_floor) : -1.0;          // (no usable pixel: nothing is an inlier)
    median[p] = med;
    counts[2 * p] = (int32_t)count[p];
}

template <int NV>
__device__ inline void sfm_block_sum(double (&v)[NV], double* __restrict__ out) {
    __shared__ double red[SFM_BLOCK / WAVE][NV];
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double s = v[k];
        for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off);
        if (lane == 0) red[wid][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) out[threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// the three sum passes of the normalised 8-point fit over the inliers (val <= thr): STAGE 0 the count and the coordinate
// sums, 1 the distances to the centroids, 2 the 45 unique sums of A^T A.  grid (chunks, P); one row of partials per workgroup.
template <int STAGE>
__global__ void __launch_bounds__(SFM_BLOCK) sfm_sum_kernel(const float* __restrict__ flow, const double* __restrict__ val,
                                                            const double* __restrict__ thr, const double* __restrict__ sums,
                                                            int W, int n, double* __restrict__ partial) {
    constexpr int NV = STAGE == 0 ? 5 : (STAGE == 1 ? 2 : 45);
    const int p = blockIdx.y;
    const double th = thr[p];
    const double* sm = sums + (size_t)p * SFM_SUMS;
    double c1x = 0, c1y = 0, c2x = 0, c2y = 0, s1 = 0, s2 = 0;
    if (STAGE >= 1) {
        const double cnt = sm[0];
        c1x = sm[1] / cnt; c1y = sm[2] / cnt; c2x = sm[3] / cnt; c2y = sm[4] / cnt;
        if (STAGE == 2) { s1 = sqrt(2.0) / (sm[5] / cnt); s2 = sqrt(2.0) / (sm[6] / cnt); }
    }
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.0;
    const float* f = flow + (size_t)p * n * 2;
    const double* v = val + (size_t)p * n;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        if (!(v[i] <= th)) continue;
        const SfmPoint pt = sfm_point(f, i, W);
        if (STAGE == 0) {
            acc[0] += 1.0; acc[1] += pt.x1; acc[2] += pt.y1; acc[3] += pt.x2; acc[4] += pt.y2;
        } else if (STAGE == 1) {
            const double ax = pt.x1 - c1x, ay = pt.y1 - c1y, bx = pt.x2 - c2x, by = pt.y2 - c2y;
            acc[0] += sqrt(ax * ax + ay * ay);
            acc[1] += sqrt(bx * bx + by * by);
        } else {
            const double x1 = (pt.x1 - c1x) * s1, y1 = (pt.y1 - c1y) * s1, x2 = (pt.x2 - c2x) * s2, y2 = (pt.y2 - c2y) * s2;
            const double a[9] = {x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, 1.0};
            int k = 0;
#pragma unroll
            for (int r = 0; r < 9; ++r)
#pragma unroll
                for (int c = r; c < 9; ++c) acc[k++] += a[r] * a[c];
        }
    }
    sfm_block_sum<NV>(acc, partial + ((size_t)p * gridDim.x + blockIdx.x) * SFM_NSUM);
}

// grid P: thread k folds channel k of the pair's rows in ascending order
__global__ void sfm_fold_kernel(const double* __restrict__ partial, int chunks, int nv, int at, double* __restrict__ sums) {
    const int p = blockIdx.x, k = threadIdx.x;
    if (k >= nv) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += partial[((size_t)p * chunks + c) * SFM_NSUM + k];
    sums[(size_t)p * SFM_SUMS + at + k] = s;
}

// one thread per pair: the null vector of A^T A, rank 2, de-normalised, ||F||_F = 1 with its largest entry positive.  A pair
// with fewer than 8 inliers, or whose fit is not finite, keeps its F.
__global__ void __launch_bounds__(WAVE) sfm_solve_kernel(const double* __restrict__ sums, int P, double* __restrict__ Fio) {
    const int p = blockIdx.x * WAVE + threadIdx.x;
    if (p >= P) return;
    const double* sm = sums + (size_t)p * SFM_SUMS;
    const double cnt = sm[0];
    if (!(cnt >= 8.0)) return;
    const double c1x = sm[1] / cnt, c1y = sm[2] / cnt, c2x = sm[3] / cnt, c2y = sm[4] / cnt;
    const double s1 = sqrt(2.0) / (sm[5] / cnt), s2 = sqrt(2.0) / (sm[6] / cnt);
    double M[81], F[9];
#pragma unroll
    for (int i = 0; i < 81; ++i) M[i] = 0.0;
    {
        int k = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int c = r; c < 9; ++c) M[r * 9 + c] = sm[8 + k++];
    }
    if (fundamental_from_normal(M, s1, c1x, c1y, s2, c2x, c2y, F)) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Fio[(size_t)p * 9 + i] = F[i];
    }
}

// the inlier bytes of the final F and their number (integer atomics)
__global__ void __launch_bounds__(SFM_BLOCK) sfm_inlier_kernel(const double* __restrict__ val, const double* __restrict__ thr, int n,
                                                               uint8_t* __restrict__ inlier, int32_t* __restrict__ counts) {
    __shared__ uint32_t cnt;
    const int p = blockIdx.y;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const double th = thr[p];
    uint32_t mine = 0;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        const bool in = val[(size_t)p * n + i] <= th;
        inlier[(size_t)p * n + i] = in ? 1 : 0;
        mine += in;
    }
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(&counts[2 * p + 1], (int32_t)cnt);
}

// ----------------------------------------------------------------------------------------------------------------- pose
struct SfmIntr { double fx, fy, cx, cy; };

__device__ inline void sfm_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ inline double sfm_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ inline void sfm_unit(double* a) {
    const double n = sqrt(sfm_dot(a, a));
    a[0] /= n; a[1] /= n; a[2] /= n;
}

// the bearing of pixel (x, y) and R times it
__device__ inline void sfm_bearing(const SfmIntr& K, double x, double y, double* b) {
    b[0] = (x - K.cx) / K.fx; b[1] = (y - K.cy) / K.fy; b[2] = 1.0;
}
__device__ inline void sfm_rotate(const double* R, const double* b, double* a) {
    a[0] = (R[0] * b[0] + R[1] * b[1]) + R[2] * b[2];
    a[1] = (R[3] * b[0] + R[4] * b[1]) + R[5] * b[2];
    a[2] = (R[6] * b[0] + R[7] * b[1]) + R[8] * b[2];
}
// z1 a + t = z2 b by least squares: with c = a x b, z1 = c . (b x t) / |c|^2, z2 = c . (a x t) / |c|^2 (the normal equations'
// solution with every difference of products written as a product of cross products); w = |c|^2 / (|a|^2 |b|^2)
__device__ inline void sfm_depths(const double* a, const double* b, const double* t, double& z1, double& z2, double& w) {
    double c[3], bt[3], at[3];
    sfm_cross(a, b, c);
    sfm_cross(b, t, bt);
    sfm_cross(a, t, at);
    const double cc = sfm_dot(c, c);
    z1 = sfm_dot(c, bt) / cc;
    z2 = sfm_dot(c, at) / cc;
    w = cc / (sfm_dot(a, a) * sfm_dot(b, b));
}

// one thread per pair: E = K^T F K, its singular vectors by Jacobi on E^T E, the two rotations (the one with the larger trace
// first) and the direction t0 = u3 with its entry of largest magnitude positive.  cand [P][21] = Ra, Rb, t0.
__global__ void __launch_bounds__(WAVE) sfm_candidates_kernel(const double* __restrict__ Fp, int P, SfmIntr K,
                                                              double* __restrict__ cand) {
    const int p = blockIdx.x * WAVE + threadIdx.x;
    if (p >= P) return;
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = Fp[(size_t)p * 9 + i];
    // K = [fx 0 cx; 0 fy cy; 0 0 1]:  F K, then K^T (F K)
    double FK[9], E[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        FK[r * 3] = F[r * 3] * K.fx;
        FK[r * 3 + 1] = F[r * 3 + 1] * K.fy;
        FK[r * 3 + 2] = (F[r * 3] * K.cx + F[r * 3 + 1] * K.cy) + F[r * 3 + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        E[c] = K.fx * FK[c];
        E[3 + c] = K.fy * FK[3 + c];
        E[6 + c] = (K.cx * FK[c] + K.cy * FK[3 + c]) + FK[6 + c];
    }
    double G[9], V[9], v3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) G[i * 3 + j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
    jacobi_sym<3>(G, V);
    smallest_column<3>(G, V, v3);
    // which column was the smallest: the other two, in cyclic order, span the plane of the two large singular values
    int js = 0;
    {
        double best = G[0];
        if (G[4] < best) { best = G[4]; js = 1; }
        if (G[8] < best) js = 2;
    }
    const int j1 = (js + 1) % 3, j2 = (js + 2) % 3;
    double v1[3], v2[3], u1[3], u2[3], u3[3];
    for (int i = 0; i < 3; ++i) { v1[i] = V[i * 3 + j1]; v2[i] = V[i * 3 + j2]; }
    sfm_cross(v1, v2, v3);
    sfm_rotate(E, v1, u1);
    sfm_rotate(E, v2, u2);
    sfm_unit(u1);
    const double d = sfm_dot(u1, u2);
    for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
    sfm_unit(u2);
    sfm_cross(u1, u2, u3);
    // U W V^T = u2 v1^T - u1 v2^T + u3 v3^T and U W^T V^T = -u2 v1^T + u1 v2^T + u3 v3^T
    double Ra[9], Rb[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double s = u2[i] * v1[j] - u1[i] * v2[j], z = u3[i] * v3[j];
            Ra[i * 3 + j] = s + z;
            Rb[i * 3 + j] = z - s;
        }
    const double tra = (Ra[0] + Ra[4]) + Ra[8], trb = (Rb[0] + Rb[4]) + Rb[8];
    const bool swap = trb > tra;
    double big = 0.0;
    for (int i = 0; i < 3; ++i) big = fabs(u3[i]) > fabs(big) ? u3[i] : big;
    const double sg = big < 0.0 ? -1.0 : 1.0;
    double* out = cand + (size_t)p * 21;
    for (int i = 0; i < 9; ++i) {
        out[i] = swap ? Rb[i] : Ra[i];
        out[9 + i] = swap ? Ra[i] : Rb[i];
    }
    for (int i = 0; i < 3; ++i) out[18 + i] = sg * u3[i];
}

// the cheirality vote: candidate c = (R_{c / 2}, +t0 for even c, -t0 for odd c); a pixel votes for c when both depths are > 0
__global__ void __launch_bounds__(SFM_BLOCK) sfm_vote_kernel(const float* __restrict__ flow, const uint8_t* __restrict__ inlier,
                                                             const double* __restrict__ cand, SfmIntr K, int W, int n,
                                                             int32_t* __restrict__ votes) {
    __shared__ uint32_t cnt[4];
    const int p = blockIdx.y;
    if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
    __syncthreads();
    double C[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) C[i] = cand[(size_t)p * 21 + i];
    const double tn[3] = {-C[18], -C[19], -C[20]};
    uint32_t mine[4] = {0, 0, 0, 0};
    const float* f = flow + (size_t)p * n * 2;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        if (!inlier[(size_t)p * n + i]) continue;
        const SfmPoint pt = sfm_point(f, i, W);
        double b1[3], b2[3], a[3], z1, z2, w;
        sfm_bearing(K, pt.x1, pt.y1, b1);
        sfm_bearing(K, pt.x2, pt.y2, b2);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            sfm_rotate(C + 9 * r, b1, a);
            sfm_depths(a, b2, C + 18, z1, z2, w);
            mine[2 * r] += (z1 > 0.0 && z2 > 0.0);
            sfm_depths(a, b2, tn, z1, z2, w);
            mine[2 * r + 1] += (z1 > 0.0 && z2 > 0.0);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (mine[c]) atomicAdd(&cnt[c], mine[c]);
    __syncthreads();
    if (threadIdx.x < 4 && cnt[threadIdx.x]) atomicAdd(&votes[4 * p + threadIdx.x], (int32_t)cnt[threadIdx.x]);
}

// one thread per pair: the candidate with the most votes (the lowest index among equals) becomes (R, t)
__global__ void sfm_pick_kernel(const double* __restrict__ cand, const int32_t* __restrict__ votes, int P, double* __restrict__ R,
                                double* __restrict__ t) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    int best = 0;
    for (int c = 1; c < 4; ++c)
        if (votes[4 * p + c] > votes[4 * p + best]) best = c;
    const double* C = cand + (size_t)p * 21;
    for (int i = 0; i < 9; ++i) R[(size_t)p * 9 + i] = C[9 * (best / 2) + i];
    for (int i = 0; i < 3; ++i) t[(size_t)p * 3 + i] = (best & 1) ? -C[18 + i] : C[18 + i];
}

// val = the pixel distance between x2 and the projection of R x1 for every inlier, NaN elsewhere
__global__ void __launch_bounds__(SFM_BLOCK) sfm_parallax_kernel(const float* __restrict__ flow, const uint8_t* __restrict__ inlier,
                                                                 const double* __restrict__ Rp, SfmIntr K, int W, int n,
                                                                 double* __restrict__ val) {
    const int p = blockIdx.y;
    double R[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rp[(size_t)p * 9 + i];
    const float* f = flow + (size_t)p * n * 2;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        double e = NAN;
        if (inlier[(size_t)p * n + i]) {
            const SfmPoint pt = sfm_point(f, i, W);
            double b1[3], a[3];
            sfm_bearing(K, pt.x1, pt.y1, b1);
            sfm_rotate(R, b1, a);
            const double dx = (K.fx * (a[0] / a[2]) + K.cx) - pt.x2, dy = (K.fy * (a[1] / a[2]) + K.cy) - pt.y2;
            e = sqrt(dx * dx + dy * dy);
            if (!std::isfinite(e)) e = NAN;
        }
        val[(size_t)p * n + i] = e;
    }
}

// one thread per pair: the parallax, the degenerate flag, and what a degenerate pair keeps
__global__ void sfm_flags_kernel(const double* __restrict__ Fp, const int32_t* __restrict__ counts,
                                 const unsigned long long* __restrict__ prefix, const uint32_t* __restrict__ count, int P,
                                 double min_parallax, double min_share, double* __restrict__ R, double* __restrict__ t,
                                 double* __restrict__ parallax, int32_t* __restrict__ degenerate) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double par = median_of(prefix, count, p);
    if (!(par == par)) par = 0.0;
    const int usable = counts[2 * p], inl = counts[2 * p + 1];
    bool bad = usable < 8 || (double)inl < min_share * (double)usable || !finite9(Fp + (size_t)p * 9) || !(par >= min_parallax);
    const bool rok = finite9(R + (size_t)p * 9);
    bad = bad || !rok || !(std::isfinite(t[3 * p]) && std::isfinite(t[3 * p + 1]) && std::isfinite(t[3 * p + 2]));
    if (bad) {
        for (int i = 0; i < 3; ++i) t[(size_t)p * 3 + i] = 0.0;
        if (!rok)
            for (int i = 0; i < 9; ++i) R[(size_t)p * 9 + i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    parallax[p] = par;
    degenerate[p] = bad ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------- triangulation
__global__ void __launch_bounds__(SFM_BLOCK) sfm_triangulate_kernel(const float* __restrict__ flow, const uint8_t* __restrict__ inlier,
                                                                    const double* __restrict__ Rp, const double* __restrict__ tp,
                                                                    const int32_t* __restrict__ degenerate, SfmIntr K, int W, int n,
                                                                    float* __restrict__ rho, float* __restrict__ weight) {
    const int p = blockIdx.y;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rp[(size_t)p * 9 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tp[(size_t)p * 3 + i];
    const bool dead = degenerate[p] != 0;
    const float* f = flow + (size_t)p * n * 2;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        float r = 0.f, w = 0.f;
        if (!dead && inlier[(size_t)p * n + i]) {
            const SfmPoint pt = sfm_point(f, i, W);
            if (pt.known) {
                double b1[3], b2[3], a[3], z1, z2, wd;
                sfm_bearing(K, pt.x1, pt.y1, b1);
                sfm_bearing(K, pt.x2, pt.y2, b2);
                sfm_rotate(R, b1, a);
                sfm_depths(a, b2, t, z1, z2, wd);
                const float rf = (float)(1.0 / z1), wf = (float)wd;
                if (z1 > 0.0 && z2 > 0.0 && std::isfinite(rf) && std::isfinite(wf)) { r = rf; w = wf; }
            }
        }
        rho[(size_t)p * n + i] = r;
        weight[(size_t)p * n + i] = w;
    }
}

// ----------------------------------------------------------------------------------------------------- median of a quotient
// val = a / b in float32 (b NULL: a) where wa > w_min and wb > w_min (a NULL weight always passes), NaN elsewhere
__global__ void __launch_bounds__(SFM_BLOCK) sfm_quotient_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ wa, const float* __restrict__ wb,
                                                                 float w_min, int n, double* __restrict__ val) {
    const size_t base = (size_t)blockIdx.y * n;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        double q = NAN;
        if ((!wa || wa[base + i] > w_min) && (!wb || wb[base + i] > w_min)) {
            const float qf = b ? a[base + i] / b[base + i] : a[base + i];
            if (std::isfinite(qf)) q = (double)qf;
        }
        val[base + i] = q;
    }
}

__global__ void sfm_median_out_kernel(const unsigned long long* __restrict__ prefix, const uint32_t* __restrict__ count, int M,
                                      double* __restrict__ median, int32_t* __restrict__ counts) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    median[m] = median_of(prefix, count, m);
    counts[m] = (int32_t)count[m];
}

// ------------------------------------------------------------------------------------------------------- fusion and fill
// rho = (wf (rf sf) + wb (rb sb)) / (wf + wb), w = wf + wb; rho = 0 where w = 0
__global__ void __launch_bounds__(SFM_BLOCK) sfm_fuse_kernel(const float* __restrict__ rf, const float* __restrict__ wf,
                                                             const float* __restrict__ rb, const float* __restrict__ wb,
                                                             const double* __restrict__ sf, const double* __restrict__ sb, int n,
                                                             float* __restrict__ rho, float* __restrict__ w) {
#pragma clang fp contract(off)
    const int t = blockIdx.y;
    const float s0 = (float)sf[t], s1 = (float)sb[t];
    const size_t base = (size_t)t * n;
    const int start = blockIdx.x * SFM_PER_BLOCK, end = min(start + SFM_PER_BLOCK, n);
    for (int i = start + threadIdx.x; i < end; i += SFM_BLOCK) {
        const float a = wf[base + i], b = wb[base + i];
        const float ws = a + b;
        const float num = a * (rf[base + i] * s0) + b * (rb[base + i] * s1);
        rho[base + i] = ws > 0.f ? num / ws : 0.f;
        w[base + i] = ws;
    }
}

// pull: a coarse pixel is the weighted mean of its 2 x 2 fine pixels (indices clamped to the fine grid), its weight a quarter
// of their weights' sum
__global__ void __launch_bounds__(SFM_BLOCK) sfm_pull_kernel(const float* __restrict__ vs, const float* __restrict__ ws, int T,
                                                             int Ws, int Hs, int Wd, int Hd, float* __restrict__ vd,
                                                             float* __restrict__ wd) {
#pragma clang fp contract(off)
    const int pix = blockIdx.x * SFM_BLOCK + threadIdx.x;
    if (pix >= Wd * Hd) return;
    const int Y = pix / Wd, X = pix - Y * Wd;
    const int x0 = 2 * X, x1 = min(2 * X + 1, Ws - 1), y0 = 2 * Y, y1 = min(2 * Y + 1, Hs - 1);
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const float* v = vs + (size_t)t * Ws * Hs;
        const float* w = ws + (size_t)t * Ws * Hs;
        const float w00 = w[y0 * Ws + x0], w01 = w[y0 * Ws + x1], w10 = w[y1 * Ws + x0], w11 = w[y1 * Ws + x1];
        const float sum = ((w00 + w01) + w10) + w11;
        const float num = ((w00 * v[y0 * Ws + x0] + w01 * v[y0 * Ws + x1]) + w10 * v[y1 * Ws + x0]) + w11 * v[y1 * Ws + x1];
        vd[(size_t)t * Wd * Hd + pix] = sum > 0.f ? num / sum : 0.f;
        wd[(size_t)t * Wd * Hd + pix] = 0.25f * sum;
    }
}

// push: a fine pixel without weight takes the bilinear sample of the (filled) coarse level at (x / 2 - 1/4, y / 2 - 1/4),
// clamped to the coarse grid; one with weight keeps its value
// (vf and out are the same array above level 0: a lane reads and writes its own pixel only)
__global__ void __launch_bounds__(SFM_BLOCK) sfm_push_kernel(const float* __restrict__ vc, int T, int Wc, int Hc, int Wf, int Hf,
                                                             const float* vf, const float* __restrict__ wf, float* out) {
#pragma clang fp contract(off)
    const int pix = blockIdx.x * SFM_BLOCK + threadIdx.x;
    if (pix >= Wf * Hf) return;
    const int y = pix / Wf, x = pix - y * Wf;
    const float cx = fminf(fmaxf(0.5f * (float)x - 0.25f, 0.f), (float)(Wc - 1));
    const float cy = fminf(fmaxf(0.5f * (float)y - 0.25f, 0.f), (float)(Hc - 1));
    const int x0 = (int)cx, y0 = (int)cy, x1 = min(x0 + 1, Wc - 1), y1 = min(y0 + 1, Hc - 1);
    const float tx = cx - (float)x0, ty = cy - (float)y0;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const size_t i = (size_t)t * Wf * Hf + pix;
        float r = vf[i];
        if (!(wf[i] > 0.f)) {
            const float* c = vc + (size_t)t * Wc * Hc;
            const float top = (1.f - tx) * c[y0 * Wc + x0] + tx * c[y0 * Wc + x1];
            const float bot = (1.f - tx) * c[y1 * Wc + x0] + tx * c[y1 * Wc + x1];
            r = (1.f - ty) * top + ty * bot;
        }
        out[i] = r;
    }
}

// one weighted Jacobi update: S and cnt are the sum and the number of the 4-neighbours inside the image (left, right, top,
// bottom).  w > 0: r0 + lam (S - cnt r0) / (w + lam cnt); w = 0: S / cnt, or the old value when lam = 0.
__device__ __forceinline__ float sfm_jacobi_update(float r0, float w, float lam, float S, float cnt, float old) {
#pragma clang fp contract(off)
    if (w > 0.f) return r0 + (lam * (S - cnt * r0)) / (w + lam * cnt);
    return lam > 0.f ? S / cnt : old;
}

__global__ void __launch_bounds__(SFM_BLOCK) sfm_sweep_plain(const float* __restrict__ rho0, const float* __restrict__ w,
                                                             const double* __restrict__ lam, const float* __restrict__ in,
                                                             float* __restrict__ out, int T, int W, int H) {
#pragma clang fp contract(off)
    const int pix = blockIdx.x * SFM_BLOCK + threadIdx.x;
    if (pix >= W * H) return;
    const int y = pix / W, x = pix - y * W;
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const size_t base = (size_t)t * W * H;
        const float* v = in + base;
        float S = 0.f, cnt = 0.f;
        if (x > 0) { S += v[pix - 1]; cnt += 1.f; }
        if (x < W - 1) { S += v[pix + 1]; cnt += 1.f; }
        if (y > 0) { S += v[pix - W]; cnt += 1.f; }
        if (y < H - 1) { S += v[pix + W]; cnt += 1.f; }
        out[base + pix] = sfm_jacobi_update(rho0[base + pix], w[base + pix], (float)lam[t], S, cnt, v[pix]);
    }
}

// `nsweeps` <= SFM_S sweeps of a SFM_R x SFM_R region in one launch; a workgroup writes its region minus a ring of SFM_S
// pixels.  Lane t owns column t % SFM_R, rows SFM_PPT (t / SFM_R) .. + SFM_PPT - 1.  A cell on the region's edge reads itself
// in place of the neighbour it lacks: what that spoils travels one cell per sweep and stays inside the ring.
__global__ void __launch_bounds__(SFM_BLOCK) sfm_sweep_fused(const float* __restrict__ rho0, const float* __restrict__ w,
                                                             const double* __restrict__ lam, const float* __restrict__ in,
                                                             float* __restrict__ out, int T, int W, int H, int tiles_x, int nsweeps) {
#pragma clang fp contract(off)
    __shared__ float sV[2][SFM_R * SFM_R];
    const int tid = threadIdx.x, cx = tid & (SFM_R - 1), r0 = (tid / SFM_R) * SFM_PPT;
    constexpr int inner = SFM_R - 2 * SFM_S;
    const int ox = (blockIdx.x % tiles_x) * inner - SFM_S, oy = (blockIdx.x / tiles_x) * inner - SFM_S;
    const int gx = ox + cx;
    const int cl = max(cx - 1, 0), cr = min(cx + 1, SFM_R - 1);
    for (int t = blockIdx.y; t < T; t += gridDim.y) {
        const size_t base = (size_t)t * W * H;
        const float lm = (float)lam[t];
        float d0[SFM_PPT], wt[SFM_PPT], cur_v[SFM_PPT];
        bool in_img[SFM_PPT];
#pragma unroll
        for (int k = 0; k < SFM_PPT; ++k) {
            const int gy = oy + r0 + k;
            in_img[k] = gx >= 0 && gx < W && gy >= 0 && gy < H;
            float v = 0.f;
            d0[k] = 0.f; wt[k] = 0.f;
            if (in_img[k]) {
                const size_t i = base + (size_t)gy * W + gx;
                v = in[i]; d0[k] = rho0[i]; wt[k] = w[i];
            }
            cur_v[k] = v;
            sV[0][(r0 + k) * SFM_R + cx] = v;                       // a cell outside the image stays 0 in both copies and
            sV[1][(r0 + k) * SFM_R + cx] = v;                       // is never added to a sum
        }
        __syncthreads();
        for (int s = 0; s < nsweeps; ++s) {
            const float* cur = sV[s & 1];
            float* nxt = sV[(s & 1) ^ 1];
#pragma unroll
            for (int k = 0; k < SFM_PPT; ++k) {
                if (!in_img[k]) continue;
                const int row = r0 + k, gy = oy + row, rt = max(row - 1, 0), rb = min(row + 1, SFM_R - 1);
                float S = 0.f, cnt = 0.f;
                if (gx > 0) { S += cur[row * SFM_R + cl]; cnt += 1.f; }
                if (gx < W - 1) { S += cur[row * SFM_R + cr]; cnt += 1.f; }
                if (gy > 0) { S += cur[rt * SFM_R + cx]; cnt += 1.f; }
                if (gy < H - 1) { S += cur[rb * SFM_R + cx]; cnt += 1.f; }
                cur_v[k] = sfm_jacobi_update(d0[k], wt[k], lm, S, cnt, cur_v[k]);
                nxt[row * SFM_R + cx] = cur_v[k];
            }
            __syncthreads();
        }
        if (cx >= SFM_S && cx < SFM_R - SFM_S) {
#pragma unroll
            for (int k = 0; k < SFM_PPT; ++k) {
                const int row = r0 + k;
                if (in_img[k] && row >= SFM_S && row < SFM_R - SFM_S) out[base + (size_t)(oy + row) * W + gx] = cur_v[k];
            }
        }
        __syncthreads();                                           // (the next frame refills both copies)
    }
}

__global__ void __launch_bounds__(SFM_BLOCK) sfm_depth_kernel(const float* __restrict__ rho, float rho_min, size_t n,
                                                              float* __restrict__ depth) {
    const size_t i = (size_t)blockIdx.x * SFM_BLOCK + threadIdx.x;
    if (i < n) depth[i] = 1.0f / fmaxf(rho[i], rho_min);
}

// ------------------------------------------------------------------------------------------------------------ host side
static bool sfm_shape_ok(int P, int H, int W) {
    if (P < 1 || P > SFM_MAX_Z || H < 8 || W < 8 || H > 16384 || W > 16384) return false;
    return (size_t)P * H * W <= ((size_t)1 << 30);
}

static int sfm_levels(int H, int W, int* hs, int* ws) {
    int n = 1;
    hs[0] = H; ws[0] = W;
    while (n < SFM_MAX_LEVELS && (hs[n - 1] > 1 || ws[n - 1] > 1)) {
        hs[n] = (hs[n - 1] + 1) / 2; ws[n] = (ws[n - 1] + 1) / 2;
        ++n;
    }
    return n;
}

struct SfmWorkspace {
    double* val; Select sel; double* thr; double* partial; double* sums; double* cand;
    float* x0; float* x1; float* pv[SFM_MAX_LEVELS]; float* pw[SFM_MAX_LEVELS];
};

static SfmWorkspace sfm_carve(Arena& a, int P, int H, int W) {
    const size_t n = (size_t)H * W, N = (size_t)P * n;
    const size_t chunks = (n + SFM_PER_BLOCK - 1) / SFM_PER_BLOCK;
    SfmWorkspace w;
    w.val = a.take<double>("sfm val", N);
    w.sel = select_carve(a, P);
    w.thr = a.take<double>("sfm thr", P);
    w.partial = a.take<double>("sfm partial", (size_t)P * chunks * SFM_NSUM);
    w.sums = a.take<double>("sfm sums", (size_t)P * SFM_SUMS);
    w.cand = a.take<double>("sfm cand", (size_t)P * 21);
    w.x0 = a.take<float>("sfm x0", N);
    w.x1 = a.take<float>("sfm x1", N);
    int hs[SFM_MAX_LEVELS], ws[SFM_MAX_LEVELS];
    const int L = sfm_levels(H, W, hs, ws);
    for (int l = 0; l < SFM_MAX_LEVELS; ++l) { w.pv[l] = nullptr; w.pw[l] = nullptr; }
    for (int l = 1; l < L; ++l) {
        w.pv[l] = a.take<float>("sfm pyramid v", (size_t)P * hs[l] * ws[l]);
        w.pw[l] = a.take<float>("sfm pyramid w", (size_t)P * hs[l] * ws[l]);
    }
    return w;
}

static bool sfm_fused_on() {
    const char* e = std::getenv("GFL_SFM_FUSED");
    return !(e && e[0] == '0');
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_sfm_workspace_bytes(int P, int H, int W) {
    if (!sfm_shape_ok(P, H, W)) return 0;
    Arena a;
    sfm_carve(a, P, H, W);
    return a.off;
}

int gfl_sfm_refit(const float* flow, const double* F_init, const uint8_t* exclude, int P, int H, int W, int rounds,
                  double e_floor, double* F_out, int32_t* counts, double* median, uint8_t* inlier, void* workspace,
                  size_t workspace_bytes, gfl_stream_t stream) {
    if (!sfm_shape_ok(P, H, W) || rounds < 0 || rounds > 16 || !(e_floor >= 0.0) || !std::isfinite(e_floor)) return GFL_ERR_INVALID;
    if (!flow || !F_init || !F_out || !counts || !median || !inlier || !workspace) return GFL_ERR_INVALID;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)F_out & 7) || ((uintptr_t)F_init & 7)) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_sfm_workspace_bytes(P, H, W)) return GFL_ERR_WORKSPACE;
    Arena a;
    a.base = (char*)workspace;
    const SfmWorkspace w = sfm_carve(a, P, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, chunks = (n + SFM_PER_BLOCK - 1) / SFM_PER_BLOCK;
    const dim3 grid(chunks, P);
    const int pg = (P + 63) / 64;
    const double k2 = (2.5 * 2.5) * (1.4826 * 1.4826);
    int rc;
    if (F_out != F_init && (rc = check(hipMemcpyAsync(F_out, F_init, (size_t)P * 9 * sizeof(double), hipMemcpyDeviceToDevice, st))) != GFL_OK)
        return rc;
    if ((rc = check(hipMemsetAsync(counts, 0, (size_t)P * 2 * sizeof(int32_t), st))) != GFL_OK) return rc;
    for (int r = 0; r <= rounds; ++r) {
        sfm_error_kernel<<<grid, SFM_BLOCK, 0, st>>>(flow, F_out, exclude, W, n, w.val);
        if ((rc = sfm_run_select(w.val, P, n, w.sel, st)) != GFL_OK) return rc;
        sfm_threshold_kernel<<<pg, 64, 0, st>>>(w.sel.prefix, w.sel.count, P, k2, e_floor, w.thr, median, counts);
        if (r == rounds) break;
        sfm_sum_kernel<0><<<grid, SFM_BLOCK, 0, st>>>(flow, w.val, w.thr, w.sums, W, n, w.partial);
        sfm_fold_kernel<<<P, 64, 0, st>>>(w.partial, chunks, 5, 0, w.sums);
        sfm_sum_kernel<1><<<grid, SFM_BLOCK, 0, st>>>(flow, w.val, w.thr, w.sums, W, n, w.partial);
        sfm_fold_kernel<<<P, 64, 0, st>>>(w.partial, chunks, 2, 5, w.sums);
        sfm_sum_kernel<2><<<grid, SFM_BLOCK, 0, st>>>(flow, w.val, w.thr, w.sums, W, n, w.partial);
        sfm_fold_kernel<<<P, 64, 0, st>>>(w.partial, chunks, 45, 8, w.sums);
        sfm_solve_kernel<<<pg, WAVE, 0, st>>>(w.sums, P, F_out);
        if ((rc = check_launch()) != GFL_OK) return rc;
    }
    sfm_inlier_kernel<<<grid, SFM_BLOCK, 0, st>>>(w.val, w.thr, n, inlier, counts);
    return check_launch();
}

int gfl_sfm_pose(const float* flow, const double* F, const uint8_t* inlier, const int32_t* counts, int P, int H, int W, double fx,
                 double fy, double cx, double cy, double min_parallax, double min_share, double* R, double* t, int32_t* votes,
                 double* parallax, int32_t* degenerate, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!sfm_shape_ok(P, H, W)) return GFL_ERR_INVALID;
    if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)) || !(fx > 0.0) || !(fy > 0.0))
        return GFL_ERR_INVALID;
    if (!std::isfinite(min_parallax) || !std::isfinite(min_share)) return GFL_ERR_INVALID;
    if (!flow || !F || !inlier || !counts || !R || !t || !votes || !parallax || !degenerate || !workspace) return GFL_ERR_INVALID;
    if ((uintptr_t)workspace & 15) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_sfm_workspace_bytes(P, H, W)) return GFL_ERR_WORKSPACE;
    Arena a;
    a.base = (char*)workspace;
    const SfmWorkspace w = sfm_carve(a, P, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, chunks = (n + SFM_PER_BLOCK - 1) / SFM_PER_BLOCK;
    const dim3 grid(chunks, P);
    const int pg = (P + 63) / 64;
    const SfmIntr K = {fx, fy, cx, cy};
    int rc;
    if ((rc = check(hipMemsetAsync(votes, 0, (size_t)P * 4 * sizeof(int32_t), st))) != GFL_OK) return rc;
    sfm_candidates_kernel<<<pg, WAVE, 0, st>>>(F, P, K, w.cand);
    sfm_vote_kernel<<<grid, SFM_BLOCK, 0, st>>>(flow, inlier, w.cand, K, W, n, votes);
    sfm_pick_kernel<<<pg, 64, 0, st>>>(w.cand, votes, P, R, t);
    sfm_parallax_kernel<<<grid, SFM_BLOCK, 0, st>>>(flow, inlier, R, K, W, n, w.val);
    if ((rc = sfm_run_select(w.val, P, n, w.sel, st)) != GFL_OK) return rc;
    sfm_flags_kernel<<<pg, 64, 0, st>>>(F, counts, w.sel.prefix, w.sel.count, P, min_parallax, min_share, R, t, parallax, degenerate);
    return check_launch();
}

int gfl_sfm_triangulate(const float* flow, const uint8_t* inlier, const double* R, const double* t, const int32_t* degenerate,
                        int P, int H, int W, double fx, double fy, double cx, double cy, float* rho, float* weight,
                        gfl_stream_t stream) {
    if (!sfm_shape_ok(P, H, W)) return GFL_ERR_INVALID;
    if (!(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy)) || !(fx > 0.0) || !(fy > 0.0))
        return GFL_ERR_INVALID;
    if (!flow || !inlier || !R || !t || !degenerate || !rho || !weight) return GFL_ERR_INVALID;
    const int n = H * W, chunks = (n + SFM_PER_BLOCK - 1) / SFM_PER_BLOCK;
    const SfmIntr K = {fx, fy, cx, cy};
    sfm_triangulate_kernel<<<dim3(chunks, P), SFM_BLOCK, 0, (hipStream_t)stream>>>(flow, inlier, R, t, degenerate, K, W, n, rho, weight);
    return check_launch();
}

int gfl_sfm_median(const float* a, const float* b, const float* wa, const float* wb, float w_min, int M, int H, int W,
                   double* median, int32_t* count, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!sfm_shape_ok(M, H, W) || !(w_min >= 0.f) || !std::isfinite(w_min)) return GFL_ERR_INVALID;
    if (!a || !median || !count || !workspace || ((uintptr_t)workspace & 15)) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_sfm_workspace_bytes(M, H, W)) return GFL_ERR_WORKSPACE;
    Arena ar;
    ar.base = (char*)workspace;
    const SfmWorkspace w = sfm_carve(ar, M, H, W);
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, chunks = (n + SFM_PER_BLOCK - 1) / SFM_PER_BLOCK;
    sfm_quotient_kernel<<<dim3(chunks, M), SFM_BLOCK, 0, st>>>(a, b, wa, wb, w_min, n, w.val);
    const int rc = sfm_run_select(w.val, M, n, w.sel, st);
    if (rc != GFL_OK) return rc;
    sfm_median_out_kernel<<<(M + 63) / 64, 64, 0, st>>>(w.sel.prefix, w.sel.count, M, median, count);
    return check_launch();
}

int gfl_sfm_fuse(const float* rho_f, const float* w_f, const float* rho_b, const float* w_b, const double* scale_f,
                 const double* scale_b, int T, int H, int W, float* rho, float* weight, gfl_stream_t stream) {
    if (!sfm_shape_ok(T, H, W)) return GFL_ERR_INVALID;
    if (!rho_f || !w_f || !rho_b || !w_b || !scale_f || !scale_b || !rho || !weight) return GFL_ERR_INVALID;
    const int n = H * W, chunks = (n + SFM_PER_BLOCK - 1) / SFM_PER_BLOCK;
    sfm_fuse_kernel<<<dim3(chunks, T), SFM_BLOCK, 0, (hipStream_t)stream>>>(rho_f, w_f, rho_b, w_b, scale_f, scale_b, n, rho, weight);
    return check_launch();
}

int gfl_sfm_fill(const float* rho0, const float* weight, const double* lambda, int T, int H, int W, int sweeps, float rho_min,
                 float* depth, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!sfm_shape_ok(T, H, W) || sweeps < 0 || sweeps > 100000 || !(rho_min > 0.f) || !std::isfinite(rho_min)) return GFL_ERR_INVALID;
    if (!rho0 || !weight || !lambda || !depth || !workspace || ((uintptr_t)workspace & 15)) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_sfm_workspace_bytes(T, H, W)) return GFL_ERR_WORKSPACE;
    Arena a;
    a.base = (char*)workspace;
    const SfmWorkspace w = sfm_carve(a, T, H, W);
    hipStream_t st = (hipStream_t)stream;
    int hs[SFM_MAX_LEVELS], ws[SFM_MAX_LEVELS];
    const int L = sfm_levels(H, W, hs, ws);
    const int zmax = T < SFM_MAX_Z ? T : SFM_MAX_Z;
    for (int l = 1; l < L; ++l) {
        const float* vs = l == 1 ? rho0 : w.pv[l - 1];
        const float* wsrc = l == 1 ? weight : w.pw[l - 1];
        sfm_pull_kernel<<<dim3((hs[l] * ws[l] + SFM_BLOCK - 1) / SFM_BLOCK, zmax), SFM_BLOCK, 0, st>>>(vs, wsrc, T, ws[l - 1], hs[l - 1],
                                                                                                    ws[l], hs[l], w.pv[l], w.pw[l]);
    }
    for (int l = L - 2; l >= 0; --l) {
        const float* vf = l == 0 ? rho0 : w.pv[l];
        const float* wf = l == 0 ? weight : w.pw[l];
        float* out = l == 0 ? w.x0 : w.pv[l];
        sfm_push_kernel<<<dim3((hs[l] * ws[l] + SFM_BLOCK - 1) / SFM_BLOCK, zmax), SFM_BLOCK, 0, st>>>(w.pv[l + 1], T, ws[l + 1], hs[l + 1],
                                                                                                    ws[l], hs[l], vf, wf, out);
    }
    int rc = check_launch();
    if (rc != GFL_OK) return rc;
    float *cur = w.x0, *other = w.x1;
    const bool fused = sfm_fused_on();
    constexpr int inner = SFM_R - 2 * SFM_S;
    const int tiles_x = (W + inner - 1) / inner, tiles_y = (H + inner - 1) / inner;
    for (int done = 0; done < sweeps;) {
        if (fused) {
            const int n = sweeps - done < SFM_S ? sweeps - done : SFM_S;
            sfm_sweep_fused<<<dim3(tiles_x * tiles_y, zmax), SFM_BLOCK, 0, st>>>(rho0, weight, lambda, cur, other, T, W, H, tiles_x, n);
            done += n;
        } else {
            sfm_sweep_plain<<<dim3((H * W + SFM_BLOCK - 1) / SFM_BLOCK, zmax), SFM_BLOCK, 0, st>>>(rho0, weight, lambda, cur, other, T, W, H);
            done += 1;
        }
        float* tmp = cur; cur = other; other = tmp;
    }
    const size_t N = (size_t)T * H * W;
    sfm_depth_kernel<<<(unsigned)((N + SFM_BLOCK - 1) / SFM_BLOCK), SFM_BLOCK, 0, st>>>(cur, rho_min, N, depth);
    return check_launch();
}

}  // extern "C"
