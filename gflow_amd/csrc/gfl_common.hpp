// Shared device/host helpers for libgflow_hip (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/gflow_hip.h"

namespace gfl {

extern thread_local int g_last_hip_error;

inline int check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return GFL_ERR_HIP;
    }
    return GFL_OK;
}
inline int check(hipError_t e) {
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return GFL_ERR_HIP;
    }
    return GFL_OK;
}

constexpr int WAVE = 64;
constexpr int REC = 12;   // floats per rec row (the fit's layout: gfl_fit.hpp)

// where pixel p is sampled (include/gflow_hip.h: GFL_PIXEL_CENTER).  With the default 0 this is (float)p and the kernels are
// instruction for instruction what they were without the constant.
constexpr float PIXEL_CENTER = GFL_PIXEL_CENTER;
__host__ __device__ __forceinline__ float pixf(int p) {
    if constexpr (PIXEL_CENTER != 0.0f) return (float)p + PIXEL_CENTER;
    return (float)p;
}
// a splat centre as the pixel GRID sees it (tests of a centre against boxes of pixel indices)
__host__ __device__ __forceinline__ float gridf(float u) {
    if constexpr (PIXEL_CENTER != 0.0f) return u - PIXEL_CENTER;
    return u;
}
// the pixel of the calling lane when the 256 lanes of a workgroup are the pixels of tile (tx, ty): a wave owns an 8x8 block
struct TilePixel { int lx, ly, px, py; bool inside; };       // (lx, ly): inside the tile; inside: of the W x H image
__device__ __forceinline__ TilePixel tile_pixel(int tx, int ty, int W, int H) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    TilePixel p;
    p.lx = (wave & 1) * 8 + (lane & 7); p.ly = (wave >> 1) * 8 + (lane >> 3);
    p.px = tx * GFL_TILE + p.lx; p.py = ty * GFL_TILE + p.ly;
    p.inside = p.px < W && p.py < H;
    return p;
}
// tile sort: lists longer than SORT_SPLIT_MIN keys are cut at a pivot and sorted by two workgroups; at most SORT_MAX_SPLIT
// tiles per launch (gfl_tile_sort.hpp; the list of such tiles is the trailer of the sort's order: gfl_fused.hip build_sort_order)
#ifndef GFL_SORT_SPLIT_MIN
#define GFL_SORT_SPLIT_MIN 768
#endif
constexpr int SORT_SPLIT_MIN = GFL_SORT_SPLIT_MIN;
constexpr int SORT_MAX_SPLIT = 64;
constexpr int SORT_ORDER_TRAILER = SORT_MAX_SPLIT + 4;      // ints behind order[T][4]: count, positions
constexpr int SLOT_MAX = 32;   // fused backward: list positions kept per splat (tile rect <= 32 tiles)

// Camera in wave-uniform registers: the 16 floats are read with scalar loads.
struct Cam {
    float fx, fy, cx, cy;
    float r00, r01, r02, t0;
    float r10, r11, r12, t1;
    float r20, r21, r22, t2;
};

__device__ __forceinline__ Cam load_cam(const float* __restrict__ intr, const float* __restrict__ extr) {
    Cam c;
    c.fx = intr[0]; c.fy = intr[1]; c.cx = intr[2]; c.cy = intr[3];
    c.r00 = extr[0]; c.r01 = extr[1]; c.r02 = extr[2]; c.t0 = extr[3];
    c.r10 = extr[4]; c.r11 = extr[5]; c.r12 = extr[6]; c.t1 = extr[7];
    c.r20 = extr[8]; c.r21 = extr[9]; c.r22 = extr[10]; c.t2 = extr[11];
    return c;
}

// ---- wave64 reductions on DPP (no LDS traffic) -------------------------------
// After the six steps lane 63 holds the sum of all 64 lanes.
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
    // quad_perm [1,0,3,2] = 0xB1, [2,3,0,1] = 0x4E, row_half_mirror = 0x141,
    // row_mirror = 0x140, row_bcast:15 = 0x142, row_bcast:31 = 0x143
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xC, 0xF, true));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    v = wave_sum_to_lane63(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// XCD-aware block order.  The dispatcher is observed to place workgroup b on XCD b % 8
// (MI355X_MICROARCH.md, "Workgroup dispatch"); each XCD has its own 4 MB L2.  Kernels whose
// neighbouring blocks share data (stencil halos, splat records of adjacent tiles) therefore walk
// their work in this order: XCD x owns one contiguous range of logical block ids.  Speed only --
// the map is a bijection on [0, nb) whatever the real placement is.
__device__ __forceinline__ int xcd_logical_block(int b, int nb) {
    const int q = nb >> 3, r = nb & 7;
    const int x = b & 7, i = b >> 3;
    return x * q + min(x, r) + i;
}

// Reduce-scatter of N per-lane values over the wave (blend backward): N = 10, the five conic/centre moments, do, df0..3 of the
// first frame; N = 7, later frames, whose colours are frozen (trainer.py:537-540) -- the moments, the opacity's and the depth
// feature's gradient; N = 6, the camera-only stage -- nobody reads the opacity / colour gradients of frozen splats.
// gfx950's v_permlane32_swap / v_permlane16_swap exchange half-waves / rows between two
// registers, so "swap + add" halves the number of live values while summing lane pairs:
//   stage 1  10 -> 5 values (lanes i, i+32),  stage 2  5 -> 3 values (rows 2k, 2k+1),
//   stage 3  the three values folded over the 16 lanes of a row (9 ops, below).
//   ~27 VALU ops instead of 10 x 6 dependent DPP adds.
// Afterwards, in row r = (hi, odd) = (lane>>5, (lane>>4)&1) every lane holds
//   x0 = sum of component 2*odd + hi,  x1 = sum of component 4 + 2*odd + hi,
//   x2 = sum of component 8 + hi (even rows only).
// Six and seven values take eight slots {c0 .. c6, 0}: 8 -> 4 -> 2 values (six: 6 -> 3 -> 2), then the two folded over the 16
// lanes of a row: 16 / 18 VALU ops.  Afterwards lanes with bit 0 clear hold component 2 * odd + hi, lanes with bit 0 set
// component 4 + hi in even rows and (seven) component 6 in row (hi = 0, odd = 1).
// Returns the value this lane ends up with; reduce_scatter_component<N>(lane) says which component it is.
// NOTE (ROCm 7.2 hipcc): __builtin_amdgcn_permlane{16,32}_swap returns the updated vdst in BOTH
// elements of its result (verified on hardware), so the swaps are issued as inline asm; the
// leading s_nop covers the VALU-write -> permlane-read hazard that hipcc does not pad inside asm.
__device__ __forceinline__ void permlane32_swap(float& a, float& b) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void permlane16_swap(float& a, float& b) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}

// five (four, three, two) independent swaps behind ONE hazard nop: the operands of all of them are written
// before the block, and no swap reads what another one wrote
__device__ __forceinline__ void permlane32_swap(float (&a)[5], float (&b)[5]) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %5\n\tv_permlane32_swap_b32 %1, %6\n\tv_permlane32_swap_b32 %2, %7\n\t"
        "v_permlane32_swap_b32 %3, %8\n\tv_permlane32_swap_b32 %4, %9"
        : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]));
}
__device__ __forceinline__ void permlane32_swap(float (&a)[4], float (&b)[4]) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %4\n\tv_permlane32_swap_b32 %1, %5\n\tv_permlane32_swap_b32 %2, %6\n\t"
        "v_permlane32_swap_b32 %3, %7"
        : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}
__device__ __forceinline__ void permlane32_swap(float (&a)[3], float (&b)[3]) {
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %3\n\tv_permlane32_swap_b32 %1, %4\n\tv_permlane32_swap_b32 %2, %5"
        : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]));
}
__device__ __forceinline__ void permlane16_swap(float (&a)[3], float (&b)[3]) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %3\n\tv_permlane16_swap_b32 %1, %4\n\tv_permlane16_swap_b32 %2, %5"
        : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]));
}
__device__ __forceinline__ void permlane16_swap(float (&a)[2], float (&b)[2]) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3"
        : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]));
}

#define GFL_DPP(val, ctrl) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (val)), ctrl, 0xF, 0xF, true))

template <int N>
__device__ __forceinline__ float wave_reduce_scatter(const float (&v)[N], int lane) {
    static_assert(N == 10 || N == 7 || N == 6, "ten, seven or six sums per pair");
    constexpr int H = (N + 1) / 2;
    float w[H];
    {
        float a[H], b[H];
#pragma unroll
        for (int m = 0; m < H; ++m) { a[m] = v[2 * m]; b[m] = 2 * m + 1 < N ? v[2 * m + 1] : 0.f; }
        permlane32_swap(a, b);        // a = {a_lo, b_lo}, b = {a_hi, b_hi}
#pragma unroll
        for (int m = 0; m < H; ++m) w[m] = a[m] + b[m];   // lanes 0-31: component 2m, lanes 32-63: component 2m+1
    }
    float t;
    if constexpr (N == 10) {
        float x[3];
        {
            float a[3] = {w[0], w[2], w[4]}, b[3] = {w[1], w[3], 0.f};
            permlane16_swap(a, b);    // a = {a_r0, b_r0, a_r2, b_r2}, b = {a_r1, b_r1, a_r3, b_r3}
            x[0] = a[0] + b[0];
            x[1] = a[1] + b[1];
            x[2] = a[2] + b[2];
        }
        // stage 3: the three values of a 16-lane row.  Instead of three independent 4-step reductions
        // (12 DPP adds) the values are folded onto lane classes on the way: after the xor-1 step the
        // even lanes carry x0 and the odd lanes x1, after the xor-2 step lanes with bit 1 set carry x2;
        // two rotations by 4 and 8 lanes (which keep the low two lane bits) finish the sums: 9 ops.
        const bool b0 = lane & 1, b1 = lane & 2;
        const float keep01 = b0 ? x[1] : x[0], send01 = b0 ? x[0] : x[1];
        const float y = keep01 + GFL_DPP(send01, 0xB1);          // quad_perm [1,0,3,2]
        const float z = x[2] + GFL_DPP(x[2], 0xB1);
        const float keep = b1 ? z : y, send = b1 ? y : z;
        t = keep + GFL_DPP(send, 0x4E);                          // quad_perm [2,3,0,1]
        // lane & 3 == 0: x0 total, == 1: x1 total, >= 2: x2 total
    } else {
        float x[2];
        {
            float a[2] = {w[0], w[2]}, b[2] = {w[1], H > 3 ? w[H - 1] : 0.f};
            permlane16_swap(a, b);
            x[0] = a[0] + b[0];                                // even rows: w0, odd rows: w1
            x[1] = a[1] + b[1];                                // even rows: w2, odd rows: w3 (seven)
        }
        const bool b0 = lane & 1;
        const float keep = b0 ? x[1] : x[0], send = b0 ? x[0] : x[1];
        t = keep + GFL_DPP(send, 0xB1);                        // quad_perm [1,0,3,2]
        t += GFL_DPP(t, 0x4E);                                 // quad_perm [2,3,0,1]
    }
    t += GFL_DPP(t, 0x124);                                    // row_ror:4
    t += GFL_DPP(t, 0x128);                                    // row_ror:8
    return t;
}

// which of the N components the value returned to this lane belongs to (-1: a duplicate, not to
// be used).  Depends on the lane only: callers evaluate it ONCE, outside their loops (inside, the
// compiler turned the nested selects into a dozen exec-mask instructions per call).
template <int N>
__device__ __forceinline__ int reduce_scatter_component(int lane) {
    const int hi = lane >> 5, odd = (lane >> 4) & 1, sel = lane & 15;
    if constexpr (N == 10) return sel == 0 ? 2 * odd + hi : (sel == 1 ? 4 + 2 * odd + hi : ((sel == 2 && odd == 0) ? 8 + hi : -1));
    if constexpr (N == 7) return sel == 0 ? 2 * odd + hi : (sel == 1 ? (odd == 0 ? 4 + hi : (hi == 0 ? 6 : -1)) : -1);
    return sel == 0 ? 2 * odd + hi : ((sel == 1 && odd == 0) ? 4 + hi : -1);
}

// ---- wave64 scans, integer reductions and lane exchange: the ONE copy every kernel uses ----
struct OpAdd {
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
// inclusive scan over the wave: lane l ends with op over lanes 0 .. l (six __shfl_up steps)
template <typename T, typename Op = OpAdd>
__device__ __forceinline__ T wave_scan_incl(T v, Op op = Op{}) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T n = __shfl_up(v, off);
        if (lane >= off) v = op(v, n);
    }
    return v;
}
// the value of lane - 1 (lane 0: its own)
template <typename T>
__device__ __forceinline__ T wave_prev_lane(T v) { return __shfl_up(v, 1); }

// max / min / sum of one int per lane, to every lane (xor butterfly, off = 32 .. 1)
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {       // fixed shape: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Exclusive scan of one value per thread over the workgroup of BLOCK threads: returns the sum of the threads in front of
// this one; `total` = the sum over all threads, to every thread.  wsum: BLOCK / 64 values of LDS.  Whole workgroup.
// Barrier contract: barrier, wave totals written, barrier, totals read -- so
//   1. it may be called back to back on the same wsum (the leading barrier ends the previous call's reads), and
//   2. LDS (and global) writes the caller made before the call are visible to the whole workgroup when it returns.
// There is NO barrier behind the last read of wsum: a caller that writes wsum itself puts one first.
// int: inclusive - v.  double: the inclusive value of the lane before (v subtracted again would not be exact); the fold
// order -- lanes of a wave by the shuffle ladder, then the waves in wave order -- is part of gfl_scan_f64's bits.
template <int BLOCK, typename T>
__device__ __forceinline__ T block_scan_excl(T v, T* wsum, T& total) {
    static_assert(BLOCK % 64 == 0, "whole waves");
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const T sc = wave_scan_incl(v);
    __syncthreads();
    if (lane == 63) wsum[wid] = sc;
    __syncthreads();
    T wprefix = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / 64; ++w) {
        const T x = wsum[w];
        if (w < wid) wprefix += x;
        total += x;
    }
    if constexpr (std::is_floating_point<T>::value) {
        const T prev = wave_prev_lane(sc);
        return wprefix + (lane > 0 ? prev : T(0));
    } else {
        return wprefix + sc - v;
    }
}

// Value of lane (lane ^ D) for a wave-uniform D in {1, 2, 4, 8, 16, 32}, on the VALU only: DPP
// quad permutes / row shifts / row rotate inside a 16-lane row, v_permlane16_swap / v_permlane32_swap
// (gfx950) across rows.  __shfl_xor goes through ds_bpermute (address VGPR + an LDS-pipe round trip
// per 32 bits); with ~40 dependent exchange steps per tile the sort network cost 14 of the
// launch's 24 us that way.
template <int D>
__device__ __forceinline__ unsigned xor_lane(unsigned v, int lane) {
    static_assert(D == 1 || D == 2 || D == 4 || D == 8 || D == 16 || D == 32, "a power of two below the wave size");
    const int x = (int)v;
    if constexpr (D == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    else if constexpr (D == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    else if constexpr (D == 4) {
        int t = __builtin_amdgcn_update_dpp(x, x, 0x104, 0xF, 0x5, false);               // row_shl:4 -> banks 0, 2
        t = __builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);                   // row_shr:4 -> banks 1, 3
        return (unsigned)t;
    } else if constexpr (D == 8) return (unsigned)__builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, true);   // row_ror:8
    else if constexpr (D == 16) {
        float a = __builtin_bit_cast(float, v), b = a;
        permlane16_swap(a, b);               // a = rows {0,0,2,2} of v, b = rows {1,1,3,3}
        return __builtin_bit_cast(unsigned, (lane & 16) ? a : b);
    } else {
        float a = __builtin_bit_cast(float, v), b = a;
        permlane32_swap(a, b);               // a = {lo, lo}, b = {hi, hi}
        return __builtin_bit_cast(unsigned, (lane & 32) ? a : b);
    }
}

// floats as unsigned keys of the same order (atomicMin / atomicMax on floats of either sign), and back
__device__ __forceinline__ unsigned f2ord(float f) {
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// min of lo and max of hi over the wave, to every lane
__device__ __forceinline__ void wave_range_ord(unsigned& lo, unsigned& hi) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, off));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, off));
    }
}
// The range of apply_float_colormap(non_zero=True) (color.py:28-31) as keys: lo = the smallest key of a non-zero value, hi
// = the largest key of any.  Start from RangeOrd{}, add() every value of the lane, then wave(): the range over the wave, to
// every lane; lane 0 of every wave folds it into global memory with the caller's own atomics.
struct RangeOrd {
    unsigned lo = 0xffffffffu, hi = 0u;
    __device__ __forceinline__ void add(float x) {
        const unsigned k = f2ord(x);
        if (x != 0.f) lo = min(lo, k);
        hi = max(hi, k);
    }
    __device__ __forceinline__ void wave() { wave_range_ord(lo, hi); }
};


// Deterministic block-level reduction of NV values -> one partial row per block.
// partial[blockIdx.x * NV + k]; a second tiny kernel folds the rows in order.
// AGENT: the row is stored with agent-scope atomic stores (write-through), for a reader in ANOTHER workgroup of the
// same launch (camera_tail of gfl_fused.hip).
template <int NV, int BLOCK, bool AGENT = false>
__device__ __forceinline__ void block_reduce_store(float (&vals)[NV], float* __restrict__ partial) {
    __shared__ float red[BLOCK / WAVE][NV];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float s = wave_sum_to_lane63(vals[k]);
        if (lane == 63) red[wid][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < BLOCK / WAVE; ++w) s += red[w][threadIdx.x];
        if (AGENT) __hip_atomic_store(&partial[(size_t)blockIdx.x * NV + threadIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else partial[(size_t)blockIdx.x * NV + threadIdx.x] = s;
    }
}

// one block; thread t folds rows t, t+256, ... in order, then a fixed-shape
// wave/LDS tree combines the 256 partials: bitwise reproducible run to run.
// Returns channel threadIdx.x's total to the threads below NV.
template <int NV>
__device__ __forceinline__ float fold_partials_block(const float* __restrict__ partial, int rows) {
    float acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.f;
    for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] += partial[(size_t)r * NV + k];
    }
    __shared__ float red[4][NV];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x / WAVE;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float s = wave_sum_to_lane63(acc[k]);
        if (lane == 63) red[wid][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) return red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    return 0.f;
}

template <int NV>
__global__ void __launch_bounds__(256) fold_partials_kernel(const float* __restrict__ partial, int rows,
                                                            float* __restrict__ out) {
    const float t = fold_partials_block<NV>(partial, rows);
    if (threadIdx.x < NV) out[threadIdx.x] = t;
}

// rows that hold two gradients side by side (N0 + N1 channels; 12 extr + 4 intr): the same fold, each to its own output.
// A channel's sum is formed exactly as fold_partials_kernel forms it: out0 has the bits fold_partials_kernel<N0> gives for
// rows of N0 alone.
template <int N0, int N1>
__global__ void __launch_bounds__(256) fold_partials_split_kernel(const float* __restrict__ partial, int rows,
                                                                  float* __restrict__ out0, float* __restrict__ out1) {
    const float t = fold_partials_block<N0 + N1>(partial, rows);
    if (threadIdx.x < N0) out0[threadIdx.x] = t;
    else if (threadIdx.x < N0 + N1) out1[threadIdx.x - N0] = t;
}

constexpr int REDUCE_BLOCK = 256;
inline int reduce_rows(int N) { return (N + REDUCE_BLOCK - 1) / REDUCE_BLOCK; }

// ---- host side: the tile grid of an image, and workspaces described once
struct TileGrid {
    int gx, gy, T;
    size_t tiles() const { return (size_t)gx * gy; }      // (for sizes: no 32-bit product)
};
inline TileGrid tile_grid(int W, int H) {
    const int gx = (W + GFL_TILE - 1) / GFL_TILE, gy = (H + GFL_TILE - 1) / GFL_TILE;
    return {gx, gy, (int)((size_t)gx * gy)};
}

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// A workspace is ONE walk that take()s its regions in address order: over a base pointer the walk carves, without one it
// only counts (`off` ends as the size to ask for), and with a table it also lists the regions (gfl_fit_workspace_layout).
// Every region starts on a 256-byte boundary.  Nothing is allocated; the names are literals.
struct Arena {
    char* base = nullptr;
    size_t off = 0;
    const char** names = nullptr; size_t* offsets = nullptr; size_t* bytes = nullptr;      // rows [0, max) are written,
    int max = 0, n = 0;                                                                    // n counts every region
    template <typename T>
    T* take(const char* name, size_t count) {
        if (n < max) { names[n] = name; offsets[n] = off; bytes[n] = count * sizeof(T); }
        ++n;
        T* p = base ? (T*)(base + off) : nullptr;
        off += up256(count * sizeof(T));
        return p;
    }
};

}  // namespace gfl
