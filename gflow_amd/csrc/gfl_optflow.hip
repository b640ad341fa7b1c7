// Optical flow from two images (include/gflow_hip.h, "optical flow"): a coarse-to-fine variational estimate.  Grey, a 5-tap
// binomial pyramid, and per level `warps` linearisations x `outer` re-weightings x `sweeps` Jacobi sweeps of the per-pixel
// 2 x 2 systems.  The problems of a call (a clip's forward and backward pairs) are the slow axis of every grid.
//
// Where the time goes is the sweeps (warps x outer x sweeps = 750 per level at the defaults), so they are fused:
// of_sweep_fused keeps a region of OF_RX x OF_RY pixels in a workgroup -- the nine coefficients, u and du of a pixel in the
// registers of the lane that owns it, u + du of the region in LDS, twice (a sweep reads one copy and writes the other) --
// does up to OF_S sweeps there and writes the region minus a ring of OF_S pixels.  A Jacobi sweep reads only the previous
// sweep's values, so after s sweeps exactly the pixels nearer than s to the region's edge are wrong, and the written interior
// has the bits of s plain sweeps (of_sweep_plain, one launch per sweep: GFL_OPTFLOW_FUSED=0, kept for the comparison).
// A ring pixel outside the image is never used: the edge weights towards it are zero.  A level of at most OF_RX x OF_RY
// pixels needs no ring: one workgroup per problem runs all the sweeps of a re-weighting in one launch.
//
// Everything is float32 in the order the header writes it, products and sums rounded separately (no contraction), so the
// fused and the plain sweeps agree bit for bit and both follow tests/optflow_ref.py run in float32.
// No atomics, no allocation, no host synchronisation.
#include <cmath>
#include <cstdlib>

#include "gfl_common.hpp"

#pragma clang fp contract(off)

namespace gfl {

// the region of a workgroup (pixels), the sweeps per launch of the tiled path = the ring's width, and the lanes that share
// the region ("Optical flow", has the measurements behind the three)
#ifndef GFL_OF_RY
#define GFL_OF_RY 64
#endif
#ifndef GFL_OF_S
#define GFL_OF_S 6
#endif
#ifndef GFL_OF_THREADS
#define GFL_OF_THREADS 1024
#endif
constexpr int OF_RX = 64, OF_RY = GFL_OF_RY;
constexpr int OF_S = GFL_OF_S;
constexpr int OF_THREADS = GFL_OF_THREADS;
constexpr int OF_PPT = OF_RX * OF_RY / OF_THREADS; // pixels per lane: a column segment
static_assert(OF_PPT * OF_THREADS == OF_RX * OF_RY && OF_THREADS % OF_RX == 0 && 2 * OF_S < OF_RY, "region / lanes / ring");
constexpr int OF_TX = OF_RX - 2 * OF_S, OF_TY = OF_RY - 2 * OF_S;      // what a launch of the tiled path writes per workgroup
constexpr int OF_MAX_Z = 65535;                    // problems per grid; the ones beyond are walked in a stride
constexpr int OF_MAX_LEVELS = 32;
constexpr float OF_EPS2 = 1e-6f;                   // epsilon^2, epsilon = 1e-3
constexpr int OF_NCOEF = 9;                        // wl wr wt wb a11 a22 a12 c1 c2
constexpr int OF_DOWN_BX = 32, OF_DOWN_BY = 8;

__device__ __forceinline__ float of_clampf(float v, float hi) { return fminf(fmaxf(v, 0.f), hi); }      // (NaN -> 0)

// the correctly rounded float32 square root (sqrtf on the device is documented to 1 ulp, and the robust weights
// 1 / sqrt(r^2 + 1e-6) would carry that ulp into every coefficient).  A float's root is never nearer than 2^-50 (relative) to the middle of two
// floats, so rounding the double root is exact.  Only the coefficient launch takes roots: once per re-weighting.
__device__ __forceinline__ float of_sqrt(float x) { return (float)sqrt((double)x); }

__device__ __forceinline__ float of_bilerp(float f00, float f01, float f10, float f11, float tx, float ty) {
    const float top = (1.f - tx) * f00 + tx * f01;
    const float bot = (1.f - tx) * f10 + tx * f11;
    return (1.f - ty) * top + ty * bot;
}

// ---- grey: both images of every problem, out [2 P][H W] (the a's, then the b's)
__global__ void __launch_bounds__(256)
    of_grey_kernel(const void* __restrict__ a, const void* __restrict__ b, int is_u8, int P, int hw, float* __restrict__ out) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    for (int img = blockIdx.y; img < 2 * P; img += gridDim.y) {
        const void* src = img < P ? a : b;
        const size_t i = ((size_t)(img < P ? img : img - P) * hw + pix) * 3;
        float r, g, bl;
        if (is_u8) {
            const uint8_t* s = (const uint8_t*)src;
            r = (float)s[i] / 255.f; g = (float)s[i + 1] / 255.f; bl = (float)s[i + 2] / 255.f;
        } else {
            const float* s = (const float*)src;
            r = s[i]; g = s[i + 1]; bl = s[i + 2];
        }
        out[(size_t)img * hw + pix] = 255.f * ((0.299f * r + 0.587f * g) + 0.114f * bl);
    }
}

// ---- one pyramid level: [1 4 6 4 1] / 16 along the rows, then along the columns, sampled at (2x, 2y); border replicated.
// A workgroup makes 32 x 8 outputs: the 19 source rows it needs are filtered along x into LDS, then along y from there.
__device__ __forceinline__ float of_binomial(float a, float b, float c, float d, float e) {
    return ((((a + 4.f * b) + 6.f * c) + 4.f * d) + e) * 0.0625f;
}

__global__ void __launch_bounds__(OF_DOWN_BX* OF_DOWN_BY)
    of_down_kernel(const float* __restrict__ src, float* __restrict__ dst, int n_img, int Ws, int Hs, int Wd, int Hd,
                   int tiles_x) {
    constexpr int ROWS = 2 * OF_DOWN_BY + 3;
    __shared__ float h[ROWS][OF_DOWN_BX];
    const int ox = (blockIdx.x % tiles_x) * OF_DOWN_BX, oy = (blockIdx.x / tiles_x) * OF_DOWN_BY;
    const int tid = threadIdx.x, lx = tid % OF_DOWN_BX, ly = tid / OF_DOWN_BX;
    for (int img = blockIdx.y; img < n_img; img += gridDim.y) {
        const float* s = src + (size_t)img * Hs * Ws;
        for (int i = tid; i < ROWS * OF_DOWN_BX; i += OF_DOWN_BX * OF_DOWN_BY) {
            const int ry = i / OF_DOWN_BX, cx = i % OF_DOWN_BX;
            const int sy = min(max(2 * oy - 2 + ry, 0), Hs - 1);
            const int xc = min(2 * (ox + cx), Ws - 1);             // (a column past the level is not used)
            const float* row = s + (size_t)sy * Ws;
            h[ry][cx] = of_binomial(row[max(xc - 2, 0)], row[max(xc - 1, 0)], row[xc], row[min(xc + 1, Ws - 1)],
                                    row[min(xc + 2, Ws - 1)]);
        }
        __syncthreads();
        const int x = ox + lx, y = oy + ly;
        if (x < Wd && y < Hd)
            dst[((size_t)img * Hd + y) * Wd + x] =
                of_binomial(h[2 * ly][lx], h[2 * ly + 1][lx], h[2 * ly + 2][lx], h[2 * ly + 3][lx], h[2 * ly + 4][lx]);
        __syncthreads();
    }
}

// ---- flow of level l from level l + 1: 2 bilinear(coarse, x / 2, y / 2), coordinates clamped to the coarse grid
__global__ void __launch_bounds__(256)
    of_upsample_kernel(const float2* __restrict__ coarse, float2* __restrict__ fine, int P, int wc, int hc, int W, int H) {
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= W * H) return;
    const int x = pix % W, y = pix / W;
    const float xs = of_clampf((float)x / 2.f, (float)(wc - 1)), ys = of_clampf((float)y / 2.f, (float)(hc - 1));
    const float fx = floorf(xs), fy = floorf(ys);
    const float tx = xs - fx, ty = ys - fy;
    const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, wc - 1), y1 = min(y0 + 1, hc - 1);
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const float2* c = coarse + (size_t)p * wc * hc;
        const float2 f00 = c[y0 * wc + x0], f01 = c[y0 * wc + x1], f10 = c[y1 * wc + x0], f11 = c[y1 * wc + x1];
        fine[(size_t)p * W * H + pix] = make_float2(2.f * of_bilerp(f00.x, f01.x, f10.x, f11.x, tx, ty),
                                                    2.f * of_bilerp(f00.y, f01.y, f10.y, f11.y, tx, ty));
    }
}

// ---- one linearisation: the warped image and its three derivatives.  Iw of the four neighbours is sampled again here
// (five bilinear reads per pixel, one launch per warp) rather than kept in a plane of its own.
__device__ __forceinline__ float of_warped(const float* __restrict__ Ib, const float2* __restrict__ uv, int W, int H, int x,
                                           int y, float* inside) {
    const float2 f = uv[y * W + x];
    const float xs = (float)x + f.x, ys = (float)y + f.y;
    if (inside) *inside = (xs >= 0.f && xs <= (float)(W - 1) && ys >= 0.f && ys <= (float)(H - 1)) ? 1.f : 0.f;
    const float xc = of_clampf(xs, (float)(W - 1)), yc = of_clampf(ys, (float)(H - 1));
    const float fx = floorf(xc), fy = floorf(yc);
    const int x0 = (int)fx, y0 = (int)fy, x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    return of_bilerp(Ib[y0 * W + x0], Ib[y0 * W + x1], Ib[y1 * W + x0], Ib[y1 * W + x1], xc - fx, yc - fy);
}

__global__ void __launch_bounds__(256)
    of_warp_kernel(const float* __restrict__ Ia, const float* __restrict__ Ib, const float2* __restrict__ uv, int P, int W,
                   int H, float* __restrict__ terms, float2* __restrict__ d) {
    const int hw = W * H, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int x = pix % W, y = pix / W;
    const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yt = max(y - 1, 0), yb = min(y + 1, H - 1);
    const size_t N = (size_t)P * hw;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const size_t base = (size_t)p * hw;
        const float *a = Ia + base, *b = Ib + base;
        const float2* f = uv + base;
        float inside;
        const float iw = of_warped(b, f, W, H, x, y, &inside);
        const float wx = 0.5f * (of_warped(b, f, W, H, xr, y, nullptr) - of_warped(b, f, W, H, xl, y, nullptr));
        const float wy = 0.5f * (of_warped(b, f, W, H, x, yb, nullptr) - of_warped(b, f, W, H, x, yt, nullptr));
        const float ax = 0.5f * (a[y * W + xr] - a[y * W + xl]), ay = 0.5f * (a[yb * W + x] - a[yt * W + x]);
        terms[base + pix] = 0.5f * (wx + ax);
        terms[N + base + pix] = 0.5f * (wy + ay);
        terms[2 * N + base + pix] = iw - a[pix];
        terms[3 * N + base + pix] = inside;
        d[base + pix] = make_float2(0.f, 0.f);
    }
}

// ---- one re-weighting: the nine planes the sweeps read
__device__ __forceinline__ float2 of_total(const float2* __restrict__ uv, const float2* __restrict__ d, int i) {
    const float2 a = uv[i], b = d[i];
    return make_float2(a.x + b.x, a.y + b.y);
}
__device__ __forceinline__ float of_smooth_weight(const float2* __restrict__ uv, const float2* __restrict__ d, int W, int H,
                                                  int x, int y, float alpha) {
    const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yt = max(y - 1, 0), yb = min(y + 1, H - 1);
    const float2 l = of_total(uv, d, y * W + xl), r = of_total(uv, d, y * W + xr);
    const float2 t = of_total(uv, d, yt * W + x), b = of_total(uv, d, yb * W + x);
    const float ux = 0.5f * (r.x - l.x), uy = 0.5f * (b.x - t.x), vx = 0.5f * (r.y - l.y), vy = 0.5f * (b.y - t.y);
    return alpha / of_sqrt(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + OF_EPS2);
}

__global__ void __launch_bounds__(256)
    of_coef_kernel(const float* __restrict__ terms, const float2* __restrict__ uv, const float2* __restrict__ d, int P, int W,
                   int H, float alpha, float* __restrict__ coef) {
    const int hw = W * H, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int x = pix % W, y = pix / W;
    const size_t N = (size_t)P * hw;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const size_t base = (size_t)p * hw, i = base + pix;
        const float2 *f = uv + base, *dd = d + base;
        const float Ix = terms[i], Iy = terms[N + i], It = terms[2 * N + i], inside = terms[3 * N + i];
        const float2 dp = dd[pix];
        const float r = (It + Ix * dp.x) + Iy * dp.y;
        const float pd = inside / of_sqrt(r * r + OF_EPS2);
        const float ps = of_smooth_weight(f, dd, W, H, x, y, alpha);
        const float wl = x > 0 ? 0.5f * (ps + of_smooth_weight(f, dd, W, H, x - 1, y, alpha)) : 0.f;
        const float wr = x < W - 1 ? 0.5f * (ps + of_smooth_weight(f, dd, W, H, x + 1, y, alpha)) : 0.f;
        const float wt = y > 0 ? 0.5f * (ps + of_smooth_weight(f, dd, W, H, x, y - 1, alpha)) : 0.f;
        const float wb = y < H - 1 ? 0.5f * (ps + of_smooth_weight(f, dd, W, H, x, y + 1, alpha)) : 0.f;
        const float ws = ((wl + wr) + wt) + wb;
        const float pix_ = pd * Ix, piy = pd * Iy;
        coef[i] = wl;
        coef[N + i] = wr;
        coef[2 * N + i] = wt;
        coef[3 * N + i] = wb;
        coef[4 * N + i] = pix_ * Ix + ws;
        coef[5 * N + i] = piy * Iy + ws;
        coef[6 * N + i] = pix_ * Iy;
        coef[7 * N + i] = pix_ * It;
        coef[8 * N + i] = piy * It;
    }
}

// ---- the Jacobi update of one pixel from its neighbours' u + du of the previous sweep
struct OfCoef { float wl, wr, wt, wb, ws, a11, a22, a12, c1, c2; };

__device__ __forceinline__ OfCoef of_load_coef(const float* __restrict__ coef, size_t N, size_t i) {
    OfCoef c;
    c.wl = coef[i]; c.wr = coef[N + i]; c.wt = coef[2 * N + i]; c.wb = coef[3 * N + i];
    c.a11 = coef[4 * N + i]; c.a22 = coef[5 * N + i]; c.a12 = coef[6 * N + i]; c.c1 = coef[7 * N + i]; c.c2 = coef[8 * N + i];
    c.ws = ((c.wl + c.wr) + c.wt) + c.wb;
    return c;
}

__device__ __forceinline__ float2 of_jacobi(const OfCoef& c, float2 u, float2 l, float2 r, float2 t, float2 b) {
    const float su = (((c.wl * l.x + c.wr * r.x) + c.wt * t.x) + c.wb * b.x) - c.ws * u.x;
    const float sv = (((c.wl * l.y + c.wr * r.y) + c.wt * t.y) + c.wb * b.y) - c.ws * u.y;
    const float b1 = su - c.c1, b2 = sv - c.c2;
    const float det = c.a11 * c.a22 - c.a12 * c.a12;
    return make_float2((c.a22 * b1 - c.a12 * b2) / det, (c.a11 * b2 - c.a12 * b1) / det);
}

// one sweep per launch, one lane per pixel: the comparison path
__global__ void __launch_bounds__(256)
    of_sweep_plain(const float* __restrict__ coef, const float2* __restrict__ uv, const float2* __restrict__ din,
                   float2* __restrict__ dout, int P, int W, int H) {
    const int hw = W * H, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= hw) return;
    const int x = pix % W, y = pix / W;
    const int xl = max(x - 1, 0), xr = min(x + 1, W - 1), yt = max(y - 1, 0), yb = min(y + 1, H - 1);
    const size_t N = (size_t)P * hw;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const size_t base = (size_t)p * hw;
        const OfCoef c = of_load_coef(coef, N, base + pix);
        const float2 *f = uv + base, *d = din + base;
        dout[base + pix] = of_jacobi(c, f[pix], of_total(f, d, y * W + xl), of_total(f, d, y * W + xr),
                                     of_total(f, d, yt * W + x), of_total(f, d, yb * W + x));
    }
}

// `nsweeps` sweeps of a region in one launch.  halo = OF_S (nsweeps <= OF_S): the image is tiled, a workgroup writes its region
// minus the ring.  halo = 0: the level is one region, any nsweeps.  Lane t owns column t % 64, rows OF_PPT (t / 64) .. + OF_PPT - 1.
__global__ void __launch_bounds__(OF_THREADS)
    of_sweep_fused(const float* __restrict__ coef, const float2* __restrict__ uv, const float2* __restrict__ din,
                   float2* __restrict__ dout, int P, int W, int H, int tiles_x, int halo, int nsweeps) {
    __shared__ float2 sU[2][OF_RY * OF_RX];
    const int tid = threadIdx.x, cx = tid & (OF_RX - 1), r0 = (tid / OF_RX) * OF_PPT;
    const int ox = (blockIdx.x % tiles_x) * (OF_RX - 2 * halo) - halo, oy = (blockIdx.x / tiles_x) * (OF_RY - 2 * halo) - halo;
    const int gx = ox + cx;
    const int cl = max(cx - 1, 0), cr = min(cx + 1, OF_RX - 1);
    const int hw = W * H;
    const size_t N = (size_t)P * hw;
    for (int p = blockIdx.y; p < P; p += gridDim.y) {
        const size_t base = (size_t)p * hw;
        OfCoef c[OF_PPT];
        float2 u[OF_PPT], d[OF_PPT];
        bool in[OF_PPT];
#pragma unroll
        for (int k = 0; k < OF_PPT; ++k) {
            const int gy = oy + r0 + k;
            in[k] = gx >= 0 && gx < W && gy >= 0 && gy < H;
            float2 tot = make_float2(0.f, 0.f);
            if (in[k]) {
                const int pix = gy * W + gx;
                c[k] = of_load_coef(coef, N, base + pix);
                u[k] = uv[base + pix];
                d[k] = din[base + pix];
                tot = make_float2(u[k].x + d[k].x, u[k].y + d[k].y);
            }
            sU[0][(r0 + k) * OF_RX + cx] = tot;                    // a cell outside the image stays 0 in both copies:
            sU[1][(r0 + k) * OF_RX + cx] = tot;                    // only ever read at weight zero
        }
        __syncthreads();
        for (int s = 0; s < nsweeps; ++s) {
            const float2* cur = sU[s & 1];
            float2* nxt = sU[(s & 1) ^ 1];
#pragma unroll
            for (int k = 0; k < OF_PPT; ++k) {
                if (!in[k]) continue;
                const int row = r0 + k, rt = max(row - 1, 0), rb = min(row + 1, OF_RY - 1);
                d[k] = of_jacobi(c[k], u[k], cur[row * OF_RX + cl], cur[row * OF_RX + cr], cur[rt * OF_RX + cx],
                                 cur[rb * OF_RX + cx]);
                nxt[row * OF_RX + cx] = make_float2(u[k].x + d[k].x, u[k].y + d[k].y);
            }
            __syncthreads();
        }
        if (cx >= halo && cx < OF_RX - halo) {
#pragma unroll
            for (int k = 0; k < OF_PPT; ++k) {
                const int row = r0 + k;
                if (in[k] && row >= halo && row < OF_RY - halo) dout[base + (oy + row) * W + gx] = d[k];
            }
        }
        __syncthreads();                                           // (the next problem refills both copies)
    }
}

__global__ void __launch_bounds__(256) of_add_kernel(float2* __restrict__ uv, const float2* __restrict__ d, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 a = uv[i], b = d[i];
    uv[i] = make_float2(a.x + b.x, a.y + b.y);
}

// ---- host side
struct OfLevelWs { float2 *d0, *d1; float *terms, *coef; };

static OfLevelWs of_level_carve(Arena& ar, size_t N) {
    OfLevelWs w;
    w.d0 = ar.take<float2>("optflow d0", N);
    w.d1 = ar.take<float2>("optflow d1", N);
    w.terms = ar.take<float>("optflow terms", 4 * N);
    w.coef = ar.take<float>("optflow coef", OF_NCOEF * N);
    return w;
}

static bool of_shape_ok(int P, int H, int W) {
    if (P < 1 || H < 8 || W < 8) return false;
    const size_t limit = (size_t)1 << 30, hw = (size_t)H * W;
    return hw <= limit && hw * (size_t)P <= limit;
}
static bool of_params_ok(float alpha, int warps, int outer, int sweeps) {
    return std::isfinite(alpha) && alpha > 0.f && warps >= 1 && outer >= 1 && sweeps >= 1;
}

// (H_l, W_l) of the pyramid; returns the number of levels
static int of_levels(int H, int W, int min_side, int* hs, int* ws) {
    int n = 1;
    hs[0] = H; ws[0] = W;
    while (n < OF_MAX_LEVELS && (hs[n - 1] < ws[n - 1] ? hs[n - 1] : ws[n - 1]) / 2 >= min_side) {
        hs[n] = (hs[n - 1] + 1) / 2; ws[n] = (ws[n - 1] + 1) / 2;
        ++n;
    }
    return n;
}

static bool of_fused_on() {
    const char* e = std::getenv("GFL_OPTFLOW_FUSED");
    return !(e && e[0] == '0');
}

// step 4 on one level; every launch on `stream`
static int of_run_level(const float* Ia, const float* Ib, float2* uv, int P, int H, int W, float alpha, int warps, int outer,
                        int sweeps, const OfLevelWs& w, bool fused, hipStream_t stream) {
    const int hw = H * W;
    const size_t N = (size_t)P * hw;
    const dim3 pix_grid((hw + 255) / 256, P < OF_MAX_Z ? P : OF_MAX_Z);
    const bool whole = W <= OF_RX && H <= OF_RY;
    const int tiles_x = (W + OF_TX - 1) / OF_TX, tiles_y = (H + OF_TY - 1) / OF_TY;
    for (int iw = 0; iw < warps; ++iw) {
        float2 *cur = w.d0, *other = w.d1;
        of_warp_kernel<<<pix_grid, 256, 0, stream>>>(Ia, Ib, uv, P, W, H, w.terms, cur);
        for (int io = 0; io < outer; ++io) {
            of_coef_kernel<<<pix_grid, 256, 0, stream>>>(w.terms, uv, cur, P, W, H, alpha, w.coef);
            if (fused && whole) {
                of_sweep_fused<<<dim3(1, pix_grid.y), OF_THREADS, 0, stream>>>(w.coef, uv, cur, other, P, W, H, 1, 0, sweeps);
                float2* t = cur; cur = other; other = t;
            } else if (fused) {
                for (int done = 0; done < sweeps; done += OF_S) {
                    const int n = sweeps - done < OF_S ? sweeps - done : OF_S;
                    of_sweep_fused<<<dim3(tiles_x * tiles_y, pix_grid.y), OF_THREADS, 0, stream>>>(w.coef, uv, cur, other, P, W,
                                                                                                   H, tiles_x, OF_S, n);
                    float2* t = cur; cur = other; other = t;
                }
            } else {
                for (int s = 0; s < sweeps; ++s) {
                    of_sweep_plain<<<pix_grid, 256, 0, stream>>>(w.coef, uv, cur, other, P, W, H);
                    float2* t = cur; cur = other; other = t;
                }
            }
            if (check_launch() != GFL_OK) return GFL_ERR_HIP;
        }
        of_add_kernel<<<(unsigned)((N + 255) / 256), 256, 0, stream>>>(uv, cur, N);
    }
    return check_launch();
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_optflow_workspace_bytes(int P, int H, int W, int min_side) {
    if (!of_shape_ok(P, H, W) || min_side < 2) return 0;
    int hs[OF_MAX_LEVELS], ws[OF_MAX_LEVELS];
    const int n = of_levels(H, W, min_side, hs, ws);
    Arena ar;
    for (int l = 0; l < n; ++l) ar.take<float>("optflow grey", (size_t)2 * P * hs[l] * ws[l]);
    for (int l = 1; l < n; ++l) ar.take<float2>("optflow flow", (size_t)P * hs[l] * ws[l]);
    of_level_carve(ar, (size_t)P * H * W);
    return ar.off;
}

int gfl_optflow_level(const float* Ia, const float* Ib, float* flow_inout, int P, int H, int W, float alpha, int warps,
                      int outer, int sweeps, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!of_shape_ok(P, H, W) || !of_params_ok(alpha, warps, outer, sweeps)) return GFL_ERR_INVALID;
    if (!Ia || !Ib || !flow_inout || !workspace) return GFL_ERR_INVALID;
    if (((uintptr_t)Ia & 3) || ((uintptr_t)Ib & 3) || ((uintptr_t)flow_inout & 7) || ((uintptr_t)workspace & 15))
        return GFL_ERR_INVALID;
    Arena count;
    of_level_carve(count, (size_t)P * H * W);
    if (workspace_bytes < count.off) return GFL_ERR_WORKSPACE;
    Arena ar;
    ar.base = (char*)workspace;
    const OfLevelWs w = of_level_carve(ar, (size_t)P * H * W);
    return of_run_level(Ia, Ib, (float2*)flow_inout, P, H, W, alpha, warps, outer, sweeps, w, of_fused_on(), (hipStream_t)stream);
}

int gfl_optflow(const void* a, const void* b, int src_is_u8, int P, int H, int W, float alpha, int warps, int outer, int sweeps,
                int min_side, float* flow_out, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!of_shape_ok(P, H, W) || !of_params_ok(alpha, warps, outer, sweeps) || min_side < 2) return GFL_ERR_INVALID;
    if ((src_is_u8 != 0 && src_is_u8 != 1) || !a || !b || !flow_out || !workspace) return GFL_ERR_INVALID;
    if (!src_is_u8 && (((uintptr_t)a & 3) || ((uintptr_t)b & 3))) return GFL_ERR_INVALID;
    if (((uintptr_t)flow_out & 7) || ((uintptr_t)workspace & 15)) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_optflow_workspace_bytes(P, H, W, min_side)) return GFL_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int hs[OF_MAX_LEVELS], ws[OF_MAX_LEVELS];
    const int n = of_levels(H, W, min_side, hs, ws);
    Arena ar;
    ar.base = (char*)workspace;
    float* grey[OF_MAX_LEVELS];
    float2* flow[OF_MAX_LEVELS];
    for (int l = 0; l < n; ++l) grey[l] = ar.take<float>("optflow grey", (size_t)2 * P * hs[l] * ws[l]);
    flow[0] = (float2*)flow_out;
    for (int l = 1; l < n; ++l) flow[l] = ar.take<float2>("optflow flow", (size_t)P * hs[l] * ws[l]);
    const OfLevelWs w = of_level_carve(ar, (size_t)P * H * W);
    const bool fused = of_fused_on();
    const int zmax = 2 * P < OF_MAX_Z ? 2 * P : OF_MAX_Z;

    of_grey_kernel<<<dim3((H * W + 255) / 256, zmax), 256, 0, st>>>(a, b, src_is_u8, P, H * W, grey[0]);
    for (int l = 1; l < n; ++l) {
        const int tiles_x = (ws[l] + OF_DOWN_BX - 1) / OF_DOWN_BX, tiles_y = (hs[l] + OF_DOWN_BY - 1) / OF_DOWN_BY;
        of_down_kernel<<<dim3(tiles_x * tiles_y, zmax), OF_DOWN_BX * OF_DOWN_BY, 0, st>>>(grey[l - 1], grey[l], 2 * P, ws[l - 1],
                                                                                         hs[l - 1], ws[l], hs[l], tiles_x);
    }
    if (check(hipMemsetAsync(flow[n - 1], 0, (size_t)P * hs[n - 1] * ws[n - 1] * sizeof(float2), st)) != GFL_OK)
        return GFL_ERR_HIP;
    if (check_launch() != GFL_OK) return GFL_ERR_HIP;
    for (int l = n - 1; l >= 0; --l) {
        const size_t hw = (size_t)hs[l] * ws[l];
        const int rc = of_run_level(grey[l], grey[l] + (size_t)P * hw, flow[l], P, hs[l], ws[l], alpha, warps, outer, sweeps, w,
                                    fused, st);
        if (rc != GFL_OK) return rc;
        if (l > 0)
            of_upsample_kernel<<<dim3((hs[l - 1] * ws[l - 1] + 255) / 256, P < OF_MAX_Z ? P : OF_MAX_Z), 256, 0, st>>>(
                flow[l], flow[l - 1], P, ws[l], hs[l], ws[l - 1], hs[l - 1]);
    }
    return check_launch();
}

}  // extern "C"
