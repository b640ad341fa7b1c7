// PNG decoded on the device (include/gflow_hip.h, "PNG files": Decoding), the counterpart of gfl_png.hip: the zlib streams of
// T images of one shape -> [T][H][W][bpp] uint8 with the bits of PIL.  The decoder proper is gfl_inflate.hpp's; here are the
// two launches around it:
//   inflate    a stream is serial, so the unit of parallel work is an image: one 64-lane workgroup each.  All decode state
//              is the same in every lane (scalar registers); the lanes share the work that is wide: the input is staged
//              through LDS 2 KiB at a time (16 bytes a lane and load), literals and matches go to a sliding window in LDS
//              -- a match is copied by all lanes at once, for a distance below 64 lane i takes byte i % distance --, and the
//              window is written to the workspace in whole-wave stores of 1 KiB, whose Adler-32 the lanes sum on the way.
//              Nothing the wave has stored to global memory is read back: matches come from the window.
//   unfilter   a workgroup of 64 lanes per image, a lane per row, each lane one pixel behind the lane above it: the pixel
//              above is the upper lane's last result (one cross-lane shift per step), the other two neighbours are the
//              lane's own registers.  64 rows a pass; loads and stores go 16 pixels at a time.
// The images are zeroed by a memset on the same stream: an image whose status is not 0 stays zero.  No allocation, no host
// synchronisation.
#include "gfl_common.hpp"
#include "gfl_inflate.hpp"

namespace gfl {

constexpr int PD_CHUNK = 1024;                      // bytes a flush stores: 16 a lane
constexpr int PD_WIN = 32768 + 4 * PD_CHUNK;        // 32 KiB of history, < 1 KiB not yet flushed, one match ahead (258)
constexpr int PD_INBUF = 2048;                      // staged input: 32 bytes a lane
constexpr int PD_STORED = 256;                      // bytes of a stored block moved per step
constexpr int PD_PIXELS = 16;                       // pixels a lane loads and stores at a time (unfilter)
static_assert(PD_WIN % PD_CHUNK == 0 && PD_CHUNK == 16 * WAVE && PD_INBUF == 32 * WAVE, "whole-wave pieces");
static_assert(PD_WIN >= 32768 + PD_CHUNK + 258 + PD_STORED, "the window holds every byte a match may reach");

// The two wide steps, kept out of line: they run once per 2 KiB read and once per 1 KiB written, and inlined at every place the
// decoder may need a byte they would make its loops long.
// inbuf[i] = data[in_base + i] for the bytes of [lo, hi), 0 for the others; the address of data[in_base] is a multiple of 16
__device__ __noinline__ void stage_input(const uint8_t* data, long long lo, long long hi, long long in_base, uint8_t* inbuf,
                                         int lane) {
    __syncthreads();                                        // (the reads of the old contents are done)
#pragma unroll
    for (int k = 0; k < PD_INBUF / (16 * WAVE); ++k) {
        const int at = (k * WAVE + lane) * 16;
        const long long q = in_base + at;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q >= lo && q + 16 <= hi) {
            v = *reinterpret_cast<const uint4*>(data + q);
        } else if (q + 16 > lo && q < hi) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (q + j >= lo && q + j < hi) w[j >> 2] |= (uint32_t)data[q + j] << ((j & 3) * 8);
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(inbuf + at) = v;
    }
    __syncthreads();
}
// PD_CHUNK bytes of the window (16-byte aligned, no wrap inside) to global memory, 16 a lane: (their sum, their weighted sum
// -- byte i times PD_CHUNK - i) over the wave, for inf::adler_add
__device__ __noinline__ uint2 store_chunk(const uint8_t* from, uint8_t* to, int lane) {
    __syncthreads();                                        // (the window's bytes are written)
    const uint4 v = *reinterpret_cast<const uint4*>(from + lane * 16);
    *reinterpret_cast<uint4*>(to + lane * 16) = v;
    const uint32_t word[4] = {v.x, v.y, v.z, v.w};
    int a = 0, w = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int b = (int)((word[j >> 2] >> ((j & 3) * 8)) & 255u);
        a += b;
        w += (16 - j) * b;
    }
    w += (PD_CHUNK - 16 - lane * 16) * a;
    return make_uint2((uint32_t)wave_sum_int(a), (uint32_t)wave_sum_int(w));
}

// the Io of gfl_inflate.hpp for one workgroup of one wave.  Every member but `lane` is the same in all lanes.
struct DeviceIo {
    const uint8_t* data;
    long long lo, hi;           // the stream is data[lo, hi)
    uint8_t* win;               // LDS [PD_WIN], 16-byte aligned
    uint8_t* inbuf;             // LDS [PD_INBUF], 16-byte aligned
    uint8_t* dst;               // the image's filtered bytes (16-byte aligned, `expect` bytes the core never exceeds)
    long long in_base;          // inbuf[i] is data[in_base + i]; the ADDRESS of data[in_base] is a multiple of 16
    long long flushed;          // bytes stored to dst: a multiple of PD_CHUNK until finish()
    int pending, wpos, fpos;    // bytes in the window not stored yet; window index of the next byte / of the first pending
    uint32_t s1, s2;            // Adler-32 of the flushed bytes
    int lane;

    __device__ __forceinline__ static int wrap(int i) { return i >= PD_WIN ? i - PD_WIN : i; }

    __device__ __forceinline__ void refill(long long abs) {
        in_base = abs - (long long)(((uintptr_t)data + (uintptr_t)abs) & 15);
        stage_input(data, lo, hi, in_base, inbuf, lane);
    }
    // index of stream byte pos in inbuf, with 8 bytes behind it staged
    __device__ __forceinline__ int staged(long long pos) {
        const long long abs = lo + pos;
        long long idx = abs - in_base;
        if (idx < 0 || idx + 8 > PD_INBUF) {
            refill(abs);
            idx = abs - in_base;
        }
        return (int)idx;
    }
    __device__ __forceinline__ uint32_t in_byte(long long pos) { return (uint32_t)GFL_INF_UNIFORM(inbuf[staged(pos)]); }
    __device__ __forceinline__ uint32_t in_word(long long pos) {
        const int idx = staged(pos), sh = (idx & 3) * 8;
        const uint32_t* w = reinterpret_cast<const uint32_t*>(inbuf) + (idx >> 2);
        const uint32_t w0 = w[0], w1 = w[1];
        return (uint32_t)GFL_INF_UNIFORM(sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0);
    }

    __device__ __forceinline__ void flush_chunk() {
        const uint2 sums = store_chunk(win + fpos, dst + flushed, lane);
        inf::adler_add(s1, s2, PD_CHUNK, sums.x, sums.y);
        fpos = wrap(fpos + PD_CHUNK);
        flushed += PD_CHUNK;
        pending -= PD_CHUNK;
    }
    __device__ __forceinline__ void advance(int n) {
        wpos = wrap(wpos + n);
        pending += n;
        while (pending >= PD_CHUNK) flush_chunk();
    }
    __device__ __forceinline__ void put(uint32_t byte) {
        win[wpos] = (uint8_t)byte;
        advance(1);
    }
    __device__ __forceinline__ void copy(int dist, int len) {
        __syncthreads();
        int src = wpos - dist;
        if (src < 0) src += PD_WIN;
        if (dist >= WAVE) {
            // 64 bytes a step: a step's sources were written before the match or by an earlier step
            for (int k = 0; k < len; k += WAVE) {
                const int i = k + lane;
                if (i < len) win[wrap(wpos + i)] = win[wrap(src + i)];
                __syncthreads();
            }
        } else {
            // the match repeats its first `dist` bytes: every lane keeps one of them and writes it once per period
            const int period = (WAVE / dist) * dist;
            const uint8_t v = win[wrap(src + lane % dist)];
            for (int k = 0; k < len; k += period) {
                const int i = k + lane;
                if (lane < period && i < len) win[wrap(wpos + i)] = v;
            }
        }
        advance(len);
    }
    __device__ __forceinline__ void stored(long long pos, int n) {
        while (n > 0) {
            const int idx = staged(pos);
            const int c = min(n, min(PD_INBUF - idx, PD_STORED));
            for (int i = lane; i < c; i += WAVE) win[wrap(wpos + i)] = inbuf[idx + i];
            advance(c);
            pos += c;
            n -= c;
        }
    }
    __device__ __forceinline__ uint32_t finish() {
        __syncthreads();
        const int cnt = max(0, min(16, pending - lane * 16));      // (fpos is a multiple of PD_CHUNK: no wrap inside)
        int a = 0, w = 0;
        for (int j = 0; j < cnt; ++j) {
            const int b = win[fpos + lane * 16 + j];
            dst[flushed + lane * 16 + j] = (uint8_t)b;
            a += b;
            w += (cnt - j) * b;
        }
        w += max(0, pending - lane * 16 - cnt) * a;
        inf::adler_add(s1, s2, (uint32_t)pending, (uint32_t)wave_sum_int(a), (uint32_t)wave_sum_int(w));
        flushed += pending;
        pending = 0;
        return (s2 << 16) | s1;
    }
};

__global__ void __launch_bounds__(WAVE)
    png_inflate_kernel(const uint8_t* __restrict__ data, long long n_bytes, const int64_t* __restrict__ offsets, long long expect,
                       long long stride, uint8_t* __restrict__ filtered, int32_t* __restrict__ status) {
    __shared__ alignas(16) uint8_t win[PD_WIN];
    __shared__ alignas(16) uint8_t inbuf[PD_INBUF];
    __shared__ inf::Tables tables;
    const int t = blockIdx.x;
    // the image's own extent, clipped to the array whatever the offsets say
    long long lo = offsets[t], hi = offsets[t + 1];
    lo = lo < 0 ? 0 : (lo > n_bytes ? n_bytes : lo);
    hi = hi < lo ? lo : (hi > n_bytes ? n_bytes : hi);
    DeviceIo io;
    io.data = data; io.lo = lo; io.hi = hi;
    io.win = win; io.inbuf = inbuf;
    io.dst = filtered + (size_t)t * (size_t)stride;
    io.in_base = lo - 2 * PD_INBUF;                         // (nothing staged)
    io.flushed = 0; io.pending = 0; io.wpos = 0; io.fpos = 0;
    io.s1 = 1u; io.s2 = 0u;
    io.lane = threadIdx.x;
    const int32_t rc = inf::inflate(io, hi - lo, expect, tables);
    if (threadIdx.x == 0) status[t] = rc;
}

template <int BPP>
__device__ __forceinline__ uint32_t unfilter_pixel(int ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
#pragma unroll
    for (int ch = 0; ch < BPP; ++ch) {
        const int sh = ch * 8;
        r |= inf::unfilter(ft, (x >> sh) & 255u, (a >> sh) & 255u, (b >> sh) & 255u, (c >> sh) & 255u) << sh;
    }
    return r;
}

// PD_PIXELS pixels from p, pixel k of them being pixel x0 + k of a row of W: 0 outside the row
template <int BPP>
__device__ __forceinline__ void load_pixels(const uint8_t* p, int x0, int W, bool live, uint32_t (&px)[PD_PIXELS]) {
    uint8_t raw[PD_PIXELS * BPP];
    if (live && x0 >= 0 && x0 + PD_PIXELS <= W) {
        __builtin_memcpy(raw, p + (long long)x0 * BPP, PD_PIXELS * BPP);
    } else {
#pragma unroll
        for (int k = 0; k < PD_PIXELS; ++k) {
            const bool in = live && x0 + k >= 0 && x0 + k < W;
#pragma unroll
            for (int ch = 0; ch < BPP; ++ch) raw[k * BPP + ch] = in ? p[(long long)(x0 + k) * BPP + ch] : (uint8_t)0;
        }
    }
#pragma unroll
    for (int k = 0; k < PD_PIXELS; ++k) {
        px[k] = 0;
#pragma unroll
        for (int ch = 0; ch < BPP; ++ch) px[k] |= (uint32_t)raw[k * BPP + ch] << (ch * 8);
    }
}

template <int BPP>
__global__ void __launch_bounds__(WAVE)
    png_unfilter_kernel(const uint8_t* __restrict__ filtered, long long stride, int W, int H, uint8_t* images, int32_t* status) {
    const int t = blockIdx.x, lane = threadIdx.x;
    const long long rowb = (long long)W * BPP;
    const uint8_t* src = filtered + (size_t)t * (size_t)stride;
    uint8_t* img = images + (size_t)t * (size_t)H * (size_t)rowb;
    if (status[t] != 0) return;
    int bad = 0;
    for (int r = lane; r < H; r += WAVE) bad |= src[(long long)r * (1 + rowb)] > 4;
    if (wave_max(bad)) {
        if (lane == 0) status[t] = inf::BAD_FILTER;
        return;
    }
    for (int band = 0; band < H; band += WAVE) {
        const int r = band + lane;
        const bool live = r < H;
        const int ft = live ? src[(long long)r * (1 + rowb)] : 0;
        const uint8_t* in = src + (long long)r * (1 + rowb) + 1;
        uint8_t* out = img + (long long)r * rowb;
        const bool from_memory = lane == 0 && r > 0;        // the row above the band: the last row of the pass before
        const int steps = W + min(WAVE, H - band) - 1;
        uint32_t left = 0, above_left = 0;
        for (int s0 = 0; s0 < steps; s0 += PD_PIXELS) {
            const int x0 = s0 - lane;
            uint32_t px[PD_PIXELS], up[PD_PIXELS], res[PD_PIXELS];
            load_pixels<BPP>(in, x0, W, live, px);
            load_pixels<BPP>(out - rowb, x0, W, from_memory, up);
#pragma unroll
            for (int k = 0; k < PD_PIXELS; ++k) {
                uint32_t above = wave_prev_lane(left);      // the upper lane's last result is the pixel above this one
                if (lane == 0) above = up[k];
                const bool in_row = live && x0 + k >= 0 && x0 + k < W;
                res[k] = in_row ? unfilter_pixel<BPP>(ft, px[k], left, above, above_left) : 0u;
                above_left = above;
                left = res[k];
            }
            uint8_t raw[PD_PIXELS * BPP];
#pragma unroll
            for (int k = 0; k < PD_PIXELS; ++k)
#pragma unroll
                for (int ch = 0; ch < BPP; ++ch) raw[k * BPP + ch] = (uint8_t)(res[k] >> (ch * 8));
            if (live && x0 >= 0 && x0 + PD_PIXELS <= W) {
                __builtin_memcpy(out + (long long)x0 * BPP, raw, PD_PIXELS * BPP);
            } else if (live) {
#pragma unroll
                for (int k = 0; k < PD_PIXELS; ++k)
                    if (x0 + k >= 0 && x0 + k < W)
#pragma unroll
                        for (int ch = 0; ch < BPP; ++ch) out[(long long)(x0 + k) * BPP + ch] = raw[k * BPP + ch];
            }
        }
        __syncthreads();                                    // (lane 63's row is written before lane 0 reads it)
    }
}

static uint8_t* png_dec_carve(Arena& ar, int T, int bpp, int W, int H, size_t& stride) {
    stride = up256((size_t)inf::filtered_bytes(bpp, W, H));
    return ar.take<uint8_t>("filtered rows", (size_t)T * stride);
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_png_decode_workspace_bytes(int T, int bpp, int W, int H) {
    if (!inf::shape_ok(T, bpp, W, H)) return 0;
    Arena ar;
    size_t stride;
    png_dec_carve(ar, T, bpp, W, H, stride);
    return ar.off;
}

int gfl_png_decode(const uint8_t* data, int64_t n_bytes, const int64_t* offsets, int T, int bpp, int W, int H, uint8_t* images,
                   int32_t* status, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (!data || !offsets || !images || !status || !workspace || n_bytes < 0) return GFL_ERR_INVALID;
    if (!inf::shape_ok(T, bpp, W, H)) return GFL_ERR_INVALID;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)offsets & 7) || ((uintptr_t)status & 3)) return GFL_ERR_INVALID;
    Arena ar;
    ar.base = (char*)workspace;
    size_t stride;
    uint8_t* filtered = png_dec_carve(ar, T, bpp, W, H, stride);
    if (workspace_bytes < ar.off) return GFL_ERR_WORKSPACE;
    const hipStream_t st = (hipStream_t)stream;
    const long long expect = inf::filtered_bytes(bpp, W, H);
    if (int rc = check(hipMemsetAsync(images, 0, (size_t)T * (size_t)H * (size_t)W * (size_t)bpp, st))) return rc;
    png_inflate_kernel<<<T, WAVE, 0, st>>>(data, (long long)n_bytes, offsets, expect, (long long)stride, filtered, status);
    if (int rc = check_launch()) return rc;
    switch (bpp) {
        case 1: png_unfilter_kernel<1><<<T, WAVE, 0, st>>>(filtered, (long long)stride, W, H, images, status); break;
        case 2: png_unfilter_kernel<2><<<T, WAVE, 0, st>>>(filtered, (long long)stride, W, H, images, status); break;
        case 3: png_unfilter_kernel<3><<<T, WAVE, 0, st>>>(filtered, (long long)stride, W, H, images, status); break;
        default: png_unfilter_kernel<4><<<T, WAVE, 0, st>>>(filtered, (long long)stride, W, H, images, status); break;
    }
    return check_launch();
}

}  // extern "C"
