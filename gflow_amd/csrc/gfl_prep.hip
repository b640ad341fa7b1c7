// Frame preparation (include/gflow_hip.h, "frame preparation"): uint8 / float32 frames -> float32, torchvision's antialiased
// Resize with exact weights, the Gaussian blur, depth's scale and offset or the mask test, for T frames in one call.
// Bandwidth work: one lane per (frame, row, output column) carrying all C channels, so a wave writes one contiguous run of
// 64 C floats; the taps come from a per-output table (lo, count, weights) that one small launch fills in float64.  The
// passes are separate launches over intermediates in the workspace -- a few 1080p frames stay in the Infinity Cache.
// No atomics, no allocation, no host synchronisation: an output depends on the inputs alone.
#include <cmath>

#include "gfl_common.hpp"

// every operation below is rounded on its own: the float64 weights are the definition, and the float32 sums must not
// depend on what the compiler fuses
#pragma clang fp contract(off)

namespace gfl {

constexpr int PREP_BLOCK = 256;
constexpr int PREP_MAX_GRID = 4096;                // workgroups per launch; the pixels beyond are walked in a stride
constexpr int PREP_MAX_EXTENT = 16384, PREP_MAX_SCALE = 64, PREP_MAX_BLUR = 31, PREP_MAX_C = 4;
constexpr size_t PREP_MAX_ELEMS = 2147483647u;     // 2^31 - 1 elements in src, in the intermediate and in dst

struct PrepAxis {                                  // the taps of one axis: output i reads [lo[i], lo[i] + cnt[i])
    int n_in, n_out, K;                            // K = 2 ceil(support) + 2 weights kept per output,
    int* lo;                                       // w[j * n_out + i] = weight of tap j of output i (0 behind cnt[i])
    int* cnt;
    float* w;
};
struct PrepBlur { int k; float w[PREP_MAX_BLUR]; };

inline int prep_axis_taps(int n_in, int n_out) {
    const int sup = n_in > n_out ? (n_in + n_out - 1) / n_out : 1;
    return 2 * sup + 2;
}

// (float)x / div, correctly rounded: the quotient of two float32 in float64 carries 53 >= 2 * 24 + 2 bits, so rounding it
// again to float32 gives the correctly rounded float32 quotient
__device__ __forceinline__ float prep_div(float x, float div) { return (float)((double)x / (double)div); }

// ---- the tables: the uint8 conversion and the two axes, one launch
__device__ __forceinline__ double prep_tap_weight(int j, double c, double inv) {
    const double d = fabs(((double)j - c + 0.5) * inv);
    const double w = 1.0 - d;
    return w > 0.0 ? w : 0.0;
}

__device__ void prep_axis_row(const PrepAxis& ax, int i) {
    const double s = (double)ax.n_in / (double)ax.n_out;
    const double support = s > 1.0 ? s : 1.0;
    const double inv = 1.0 / support;
    const double c = s * ((double)i + 0.5);
    int lo = (int)(c - support + 0.5), hi = (int)(c + support + 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > ax.n_in ? ax.n_in : hi;
    int cnt = hi - lo;
    cnt = cnt < 0 ? 0 : (cnt > ax.K ? ax.K : cnt);              // (2 support + 1 at the most: never clipped)
    double sum = 0.0;
    for (int j = 0; j < cnt; ++j) sum += prep_tap_weight(lo + j, c, inv);
    for (int j = 0; j < ax.K; ++j) {
        double w = j < cnt ? prep_tap_weight(lo + j, c, inv) : 0.0;
        if (sum != 0.0) w = w / sum;
        ax.w[(size_t)j * ax.n_out + i] = (float)w;
    }
    ax.lo[i] = lo;
    ax.cnt[i] = cnt;
}

__global__ void __launch_bounds__(PREP_BLOCK)
    prep_tables_kernel(float* __restrict__ lut, float div, PrepAxis h, PrepAxis v) {
    const int n = 256 + h.n_out + v.n_out;                         // (n_out is 0 for an axis table that is not needed)
    for (int i = blockIdx.x * PREP_BLOCK + threadIdx.x; i < n; i += gridDim.x * PREP_BLOCK) {
        if (i < 256) lut[i] = prep_div((float)i, div);
        else if (i < 256 + h.n_out) prep_axis_row(h, i - 256);
        else prep_axis_row(v, i - 256 - h.n_out);
    }
}

// ---- pixels
// a pixel of a float32 array [.][C]; `vec`: the array starts on a multiple of 4 C bytes (C = 2, 4: one wide access)
template <int C>
__device__ __forceinline__ void load_px(const float* __restrict__ a, size_t pix, bool vec, float (&v)[C]) {
    const float* q = a + pix * C;
    if constexpr (C == 4) {
        if (vec) {
            const float4 t = *reinterpret_cast<const float4*>(q);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            return;
        }
    }
    if constexpr (C == 2) {
        if (vec) {
            const float2 t = *reinterpret_cast<const float2*>(q);
            v[0] = t.x; v[1] = t.y;
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = q[c];
}
template <int C>
__device__ __forceinline__ void store_px(float* __restrict__ a, size_t pix, bool vec, const float (&v)[C]) {
    float* q = a + pix * C;
    if constexpr (C == 4) {
        if (vec) {
            *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
            return;
        }
    }
    if constexpr (C == 2) {
        if (vec) {
            *reinterpret_cast<float2*>(q) = make_float2(v[0], v[1]);
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = v[c];
}
// a source pixel, converted: step (a).  uint8 goes through the table (in LDS), float32 is divided where div is not 1
template <int C, bool U8>
__device__ __forceinline__ void load_src(const void* __restrict__ src, size_t pix, const float* lut_s, float div,
                                         float (&v)[C]) {
    if (U8) {
        const uint8_t* q = (const uint8_t*)src + pix * C;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = lut_s[q[c]];
    } else {
        const float* q = (const float*)src + pix * C;
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = div == 1.0f ? q[c] : prep_div(q[c], div);
    }
}
// step (d) on pixel p of the output
struct PrepOut { void* dst; float mul, add; int affine, vec; };
template <int C, bool MASK>
__device__ __forceinline__ void prep_emit(const PrepOut& o, size_t p, float (&r)[C]) {
    if (MASK) {
        float s = r[0];
#pragma unroll
        for (int c = 1; c < C; ++c) s += r[c];
        ((uint8_t*)o.dst)[p] = s > 0.f ? 1 : 0;
    } else {
        if (o.affine) {
#pragma unroll
            for (int c = 0; c < C; ++c) r[c] = r[c] * o.mul + o.add;
        }
        store_px<C>((float*)o.dst, p, o.vec != 0, r);
    }
}

template <bool U8>
__device__ __forceinline__ void prep_stage_lut(float* lut_s, const float* __restrict__ lut) {
    if (U8) {
        lut_s[threadIdx.x] = lut[threadIdx.x];                     // (PREP_BLOCK == 256 entries)
        __syncthreads();
    }
}

// no resize: convert and emit.  pixels = T H W
template <int C, bool U8, bool MASK>
__global__ void __launch_bounds__(PREP_BLOCK)
    prep_convert_kernel(const void* __restrict__ src, const float* __restrict__ lut, float div, long long pixels, PrepOut o) {
    __shared__ float lut_s[256];
    prep_stage_lut<U8>(lut_s, lut);
    for (long long p = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x; p < pixels; p += (long long)gridDim.x * PREP_BLOCK) {
        float v[C];
        load_src<C, U8>(src, (size_t)p, lut_s, div, v);
        prep_emit<C, MASK>(o, (size_t)p, v);
    }
}

// horizontal resize: src [rows][Ws][C] -> out [rows][Wd][C] float32, rows = T Hs
template <int C, bool U8>
__global__ void __launch_bounds__(PREP_BLOCK)
    prep_hresize_kernel(const void* __restrict__ src, const float* __restrict__ lut, float div, long long rows, PrepAxis ax,
                        float* __restrict__ out) {
    __shared__ float lut_s[256];
    prep_stage_lut<U8>(lut_s, lut);
    const int Ws = ax.n_in, Wd = ax.n_out;
    const long long pixels = rows * Wd;
    for (long long p = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x; p < pixels; p += (long long)gridDim.x * PREP_BLOCK) {
        const long long row = p / Wd;
        const int i = (int)(p - row * Wd);
        const int lo = ax.lo[i], cnt = ax.cnt[i];
        const size_t base = (size_t)row * Ws + lo;                  // (lo + cnt <= Ws)
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float w = ax.w[(size_t)j * Wd + i];
            float v[C];
            load_src<C, U8>(src, base + j, lut_s, div, v);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += w * v[c];
        }
        store_px<C>(out, (size_t)p, true, acc);
    }
}

// vertical resize: in [T][Hs][Wd][C] float32 -> [T][Hd][Wd] pixels, emitted
template <int C, bool MASK>
__global__ void __launch_bounds__(PREP_BLOCK)
    prep_vresize_kernel(const float* __restrict__ in, int T, int Wd, PrepAxis ax, PrepOut o) {
    const int Hs = ax.n_in, Hd = ax.n_out;
    const long long pixels = (long long)T * Hd * Wd;
    for (long long p = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x; p < pixels; p += (long long)gridDim.x * PREP_BLOCK) {
        const long long q = p / Wd;
        const int x = (int)(p - q * Wd);
        const int t = (int)(q / Hd), y = (int)(q - (long long)t * Hd);
        const int lo = ax.lo[y], cnt = ax.cnt[y];
        const size_t base = ((size_t)t * Hs + lo) * Wd + x;         // (lo + cnt <= Hs)
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        for (int j = 0; j < cnt; ++j) {
            const float w = ax.w[(size_t)j * Hd + y];
            float v[C];
            load_px<C>(in, base + (size_t)j * Wd, true, v);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += w * v[c];
        }
        prep_emit<C, MASK>(o, (size_t)p, acc);
    }
}

// reflect padding without repeating the edge; r < n, so one reflection brings every index of [-r, n - 1 + r] inside
__device__ __forceinline__ int prep_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// blur along x: in, out [rows][W][C] float32 (both in the workspace)
template <int C>
__global__ void __launch_bounds__(PREP_BLOCK)
    prep_hblur_kernel(const float* __restrict__ in, long long rows, int W, PrepBlur b, float* __restrict__ out) {
    const long long pixels = rows * W;
    const int r = b.k / 2;
    for (long long p = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x; p < pixels; p += (long long)gridDim.x * PREP_BLOCK) {
        const long long row = p / W;
        const int x = (int)(p - row * W);
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        for (int j = 0; j < b.k; ++j) {
            float v[C];
            load_px<C>(in, (size_t)row * W + prep_reflect(x + j - r, W), true, v);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += b.w[j] * v[c];
        }
        store_px<C>(out, (size_t)p, true, acc);
    }
}

// blur along y: in [T][H][W][C] float32 -> the output
template <int C>
__global__ void __launch_bounds__(PREP_BLOCK)
    prep_vblur_kernel(const float* __restrict__ in, int T, int H, int W, PrepBlur b, PrepOut o) {
    const long long pixels = (long long)T * H * W;
    const int r = b.k / 2;
    for (long long p = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x; p < pixels; p += (long long)gridDim.x * PREP_BLOCK) {
        const long long q = p / W;
        const int x = (int)(p - q * W);
        const int t = (int)(q / H), y = (int)(q - (long long)t * H);
        float acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.f;
        for (int j = 0; j < b.k; ++j) {
            float v[C];
            load_px<C>(in, ((size_t)t * H + prep_reflect(y + j - r, H)) * W + x, true, v);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += b.w[j] * v[c];
        }
        prep_emit<C, false>(o, (size_t)p, acc);
    }
}

// ---- host side
struct PrepShape { int T, C, Hs, Ws, Hd, Wd, blur_k; };
struct PrepWorkspace {
    float* lut;
    PrepAxis h, v;
    float* a;              // the horizontal intermediate [T][Hs][Wd][C]; with a blur also its horizontal pass [T][Hd][Wd][C]
    float* b;              // with a blur: what is blurred [T][Hd][Wd][C]
};

inline bool prep_resizes(const PrepShape& s) { return s.Hd != s.Hs || s.Wd != s.Ws; }

static bool prep_shape_ok(const PrepShape& s) {
    if (s.T < 1 || s.C < 1 || s.C > PREP_MAX_C) return false;
    for (int e : {s.Hs, s.Ws, s.Hd, s.Wd})
        if (e < 1 || e > PREP_MAX_EXTENT) return false;
    if ((long long)s.Hs > (long long)PREP_MAX_SCALE * s.Hd || (long long)s.Ws > (long long)PREP_MAX_SCALE * s.Wd) return false;
    const size_t tc = (size_t)s.T * s.C;
    if (tc * s.Hs * s.Ws > PREP_MAX_ELEMS || tc * s.Hs * s.Wd > PREP_MAX_ELEMS || tc * s.Hd * s.Wd > PREP_MAX_ELEMS) return false;
    if (s.blur_k != 0) {
        if (s.blur_k < 3 || s.blur_k > PREP_MAX_BLUR || s.blur_k % 2 == 0) return false;
        if (s.blur_k / 2 >= (s.Hd < s.Wd ? s.Hd : s.Wd)) return false;
    }
    return true;
}

static PrepWorkspace prep_carve(Arena& ar, const PrepShape& s) {
    PrepWorkspace w{};
    w.lut = ar.take<float>("lut", 256);
    const size_t tc = (size_t)s.T * s.C, out_elems = tc * s.Hd * s.Wd;
    size_t a_elems = 0;
    if (prep_resizes(s)) {
        w.h = {s.Ws, s.Wd, prep_axis_taps(s.Ws, s.Wd), nullptr, nullptr, nullptr};
        w.v = {s.Hs, s.Hd, prep_axis_taps(s.Hs, s.Hd), nullptr, nullptr, nullptr};
        for (PrepAxis* ax : {&w.h, &w.v}) {
            ax->lo = ar.take<int>("axis_lo", ax->n_out);
            ax->cnt = ar.take<int>("axis_count", ax->n_out);
            ax->w = ar.take<float>("axis_weights", (size_t)ax->K * ax->n_out);
        }
        a_elems = tc * s.Hs * s.Wd;
    }
    if (s.blur_k) a_elems = a_elems > out_elems ? a_elems : out_elems;
    if (a_elems) w.a = ar.take<float>("pass_a", a_elems);
    if (s.blur_k) w.b = ar.take<float>("pass_b", out_elems);
    return w;
}

inline int prep_grid(long long work) {
    const long long blocks = (work + PREP_BLOCK - 1) / PREP_BLOCK;
    return (int)(blocks < PREP_MAX_GRID ? blocks : PREP_MAX_GRID);
}

// the taps of step (c): exp(-0.5 (x / sigma)^2) at x = -(k - 1) / 2 ..., normalised in float64, rounded to float32
static PrepBlur prep_blur_taps(int k, float sigma) {
    PrepBlur b{};
    b.k = k;
    double pdf[PREP_MAX_BLUR], sum = 0.0;
    for (int j = 0; j < k; ++j) {
        const double x = ((double)j - (double)(k - 1) * 0.5) / (double)sigma;
        pdf[j] = std::exp(-0.5 * (x * x));
        sum += pdf[j];
    }
    for (int j = 0; j < k; ++j) b.w[j] = (float)(pdf[j] / sum);
    return b;
}

template <int C>
static int prep_launch(const void* src, bool u8, const PrepShape& s, float div, const PrepBlur& blur, bool mask,
                       const PrepWorkspace& w, PrepOut out, hipStream_t st) {
    const bool resize = prep_resizes(s);
    const long long out_pixels = (long long)s.T * s.Hd * s.Wd;
    if (u8 || resize) {
        PrepAxis none{};
        prep_tables_kernel<<<prep_grid(256 + (resize ? s.Wd + s.Hd : 0)), PREP_BLOCK, 0, st>>>(w.lut, div, resize ? w.h : none,
                                                                                               resize ? w.v : none);
        if (int rc = check_launch()) return rc;
    }
    // what the last launch of the resize (or of the conversion) writes: the output, or what the blur reads
    PrepOut mid = out;
    if (s.blur_k) mid = {w.b, 1.f, 0.f, 0, 1};
    if (resize) {
        const long long rows = (long long)s.T * s.Hs;
        if (u8) prep_hresize_kernel<C, true><<<prep_grid(rows * s.Wd), PREP_BLOCK, 0, st>>>(src, w.lut, div, rows, w.h, w.a);
        else prep_hresize_kernel<C, false><<<prep_grid(rows * s.Wd), PREP_BLOCK, 0, st>>>(src, w.lut, div, rows, w.h, w.a);
        if (int rc = check_launch()) return rc;
        if (mask) prep_vresize_kernel<C, true><<<prep_grid(out_pixels), PREP_BLOCK, 0, st>>>(w.a, s.T, s.Wd, w.v, mid);
        else prep_vresize_kernel<C, false><<<prep_grid(out_pixels), PREP_BLOCK, 0, st>>>(w.a, s.T, s.Wd, w.v, mid);
    } else {
        const int g = prep_grid(out_pixels);
        if (u8 && mask) prep_convert_kernel<C, true, true><<<g, PREP_BLOCK, 0, st>>>(src, w.lut, div, out_pixels, mid);
        else if (u8) prep_convert_kernel<C, true, false><<<g, PREP_BLOCK, 0, st>>>(src, w.lut, div, out_pixels, mid);
        else if (mask) prep_convert_kernel<C, false, true><<<g, PREP_BLOCK, 0, st>>>(src, w.lut, div, out_pixels, mid);
        else prep_convert_kernel<C, false, false><<<g, PREP_BLOCK, 0, st>>>(src, w.lut, div, out_pixels, mid);
    }
    if (int rc = check_launch()) return rc;
    if (s.blur_k) {
        prep_hblur_kernel<C><<<prep_grid(out_pixels), PREP_BLOCK, 0, st>>>(w.b, (long long)s.T * s.Hd, s.Wd, blur, w.a);
        if (int rc = check_launch()) return rc;
        prep_vblur_kernel<C><<<prep_grid(out_pixels), PREP_BLOCK, 0, st>>>(w.a, s.T, s.Hd, s.Wd, blur, out);
        if (int rc = check_launch()) return rc;
    }
    return GFL_OK;
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_prep_workspace_bytes(int T, int C, int Hs, int Ws, int Hd, int Wd, int blur_k) {
    const PrepShape s{T, C, Hs, Ws, Hd, Wd, blur_k};
    if (!prep_shape_ok(s)) return 0;
    Arena ar;
    prep_carve(ar, s);
    return ar.off;
}

int gfl_prep_frames(const void* src, int src_is_u8, int T, int C, int Hs, int Ws, int Hd, int Wd, float div, float mul,
                    float add, int blur_k, float blur_sigma, int as_mask, void* dst, void* workspace, size_t workspace_bytes,
                    gfl_stream_t stream) {
    const PrepShape s{T, C, Hs, Ws, Hd, Wd, blur_k};
    if (!prep_shape_ok(s)) return GFL_ERR_INVALID;
    if ((src_is_u8 != 0 && src_is_u8 != 1) || (as_mask != 0 && as_mask != 1)) return GFL_ERR_INVALID;
    if (!std::isfinite(div) || !(div > 0.f) || !std::isfinite(mul) || !std::isfinite(add)) return GFL_ERR_INVALID;
    if (blur_k && (!std::isfinite(blur_sigma) || !(blur_sigma > 0.f))) return GFL_ERR_INVALID;
    if (as_mask && (blur_k != 0 || mul != 1.f || add != 0.f)) return GFL_ERR_INVALID;
    if (!src || !dst || !workspace) return GFL_ERR_INVALID;
    if (!src_is_u8 && ((uintptr_t)src & 3)) return GFL_ERR_INVALID;
    if (!as_mask && ((uintptr_t)dst & 3)) return GFL_ERR_INVALID;
    if ((uintptr_t)workspace & 15) return GFL_ERR_INVALID;          // (the intermediates are read as float2 / float4)
    Arena ar;
    ar.base = (char*)workspace;
    const PrepWorkspace w = prep_carve(ar, s);
    if (workspace_bytes < ar.off) return GFL_ERR_INVALID;
    const PrepBlur blur = blur_k ? prep_blur_taps(blur_k, blur_sigma) : PrepBlur{};
    const PrepOut out{dst, mul, add, (mul != 1.f || add != 0.f) ? 1 : 0, ((uintptr_t)dst % (4 * (size_t)C)) == 0 ? 1 : 0};
    const hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: return prep_launch<1>(src, src_is_u8 != 0, s, div, blur, as_mask != 0, w, out, st);
        case 2: return prep_launch<2>(src, src_is_u8 != 0, s, div, blur, as_mask != 0, w, out, st);
        case 3: return prep_launch<3>(src, src_is_u8 != 0, s, div, blur, as_mask != 0, w, out, st);
        default: return prep_launch<4>(src, src_is_u8 != 0, s, div, blur, as_mask != 0, w, out, st);
    }
}

}  // extern "C"
