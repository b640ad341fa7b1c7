// Track overlays (include/gflow_hip.h, "track overlays"; INTEGRATION.md section 2, "Track overlays"): the reference's
// trajectory visualiser -- coloured polylines of every track up to the frame, a disc where a point is visible, a cross where
// it is occluded -- painted over all T frames of a clip in one call.
//
// The drawing rule.  video (T,H,W,3) uint8, tracks (T,N,2) float32 (x, y), occluded (T,N) uint8, still_length.
//   coordinates  c = (int)clamp(v, -2^20, 2^20), truncated toward zero; a NaN gives -2^20.  With W, H <= 16384 every
//                non-finite coordinate lies outside the image.  A point is USABLE when 0 <= x < W, 0 <= y < H, x != 0, y != 0.
//   colours      track n: byte c = trunc(255 * lut[idx][c]) (the float32 table entry times 255 in float64: exact),
//                idx = min(int(v * 256), 255), v = (y0[n] - ymin) / (ymax - ymin) over the integer y of frame 0 (every track,
//                usable or not), v = 0 when ymax == ymin.  With 0 < still_length < N the tracks still_length .. N-1 take ymin,
//                ymax over themselves.  (int(v * 256) is formed as the integer quotient 256 (y0 - ymin) / (ymax - ymin): the same
//                number, a quotient of integers below 2^22 is never within float64's rounding of a multiple of 1/256.)
//   frame t      1. for s = 0 .. t-1 (outer), i = 0 .. N-1 (inner): the segment tracks[s,i] -> tracks[s+1,i], width 2, if both
//                   ends are inside the image and its first end is usable;
//                2. for i = 0 .. N-1: the marker at tracks[t,i] if usable -- occluded: a cross, the segments (x-4, y) ->
//                   (x+4, y) and (x, y-4) -> (x, y+4), width 4; visible: the disc dx^2 + dy^2 <= 4^2 + 2.
//                Later paint overwrites earlier paint.
//   coverage     pixel p is on the segment (a, b, w), d = b - a, when 0 <= (p-a).d <= d.d and 4 cross(p-a, d)^2 <= w^2 d.d
//                (the squares in 64-bit integers); a == b is the single pixel a.
// Because paint is opaque, a pixel's colour is that of the covering primitive with the HIGHEST PAINT INDEX -- segment (s, i):
// s N + i; marker i: (T-1) N + i, above every segment -- or the video's where nothing covers it.  That is what the kernels
// compute, so the order in which a list was filled never enters the result.
//
// Launches (a memset and six kernels, whatever the data): the integer points; the colours (one workgroup: the y range is a
// small reduction over N); the segments counted into the 16 x 16 tiles their bounding box, grown by the width, touches; a scan
// of the tiles (one workgroup), which also raises overflow[0] when the clip's pairs exceed K_cap; the fill of the lists (skipped
// on overflow); the paint, one workgroup per (tile, frame): ONE list per tile serves every frame, frame t takes its entries with
// s < t.  The paint kernel stages candidates -- the frame's N markers, then the tile's list -- 256 at a time; the staging lane
// drops what cannot touch the tile or belongs to a later frame and appends the rest to an LDS list (a cross is two entries),
// which all 256 pixels then walk, every lane reading the same entry (an LDS broadcast).  Plain C++ and vector stores only.
#include <climits>

#include "gfl_common.hpp"

namespace gfl {

constexpr int TV_TILE = GFL_TILE;
constexpr int TV_THREADS = TV_TILE * TV_TILE;
constexpr int TV_STAGE = TV_THREADS;               // candidates per staging round, one per lane
constexpr int TV_PRIMS = 2 * TV_STAGE;             // LDS entries of a round (a cross: two)
constexpr int TV_MAX_SIDE = 16384;                 // W, H: keeps (p-a).d, d.d and the cross product within int32
constexpr int TV_COORD_MAX = 1 << 20;
constexpr int TV_LINE_W = 2, TV_CROSS_W = 4, TV_MARK_R = 4;
constexpr int TV_MAX_GRID = 1 << 16;
constexpr int TV_SCAN_THREADS = 1024;

__device__ __forceinline__ int tv_coord(float v) {
    if (!(v == v)) return -TV_COORD_MAX;
    return (int)fminf(fmaxf(v, -(float)TV_COORD_MAX), (float)TV_COORD_MAX);
}
__device__ __forceinline__ bool tv_inside(int2 p, int W, int H) { return p.x >= 0 && p.x < W && p.y >= 0 && p.y < H; }
__device__ __forceinline__ bool tv_usable(int2 p, int W, int H) { return tv_inside(p, W, H) && p.x != 0 && p.y != 0; }

// pixel (px, py) on the segment a -> b of width w; all points within [-8, TV_MAX_SIDE + 8)
__device__ __forceinline__ bool tv_on_segment(int px, int py, int4 g, int w) {
    const int dx = g.z - g.x, dy = g.w - g.y, qx = px - g.x, qy = py - g.y;
    if ((dx | dy) == 0) return (qx | qy) == 0;
    const int dot = qx * dx + qy * dy, dd = dx * dx + dy * dy;
    if (dot < 0 || dot > dd) return false;
    const long long cr = (long long)(qx * dy - qy * dx);
    return 4 * cr * cr <= (long long)(w * w) * dd;
}

__global__ void __launch_bounds__(256) tv_points_kernel(const float* __restrict__ tracks, long long n, int2* __restrict__ pts) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
        pts[e] = make_int2(tv_coord(tracks[2 * e]), tv_coord(tracks[2 * e + 1]));
}

// one workgroup: the y range of frame 0 over all tracks and over the tracks from `split` on, then every track's colour
__global__ void __launch_bounds__(256) tv_colours_kernel(const int2* __restrict__ pts, int N, int still_length,
                                                          const float* __restrict__ lut, uint32_t* __restrict__ colours) {
    __shared__ int s_mm[4][256];
    const int tid = threadIdx.x;
    const int split = (still_length > 0 && still_length < N) ? still_length : N;
    int lo_a = INT_MAX, hi_a = INT_MIN, lo_b = INT_MAX, hi_b = INT_MIN;
    for (int n = tid; n < N; n += 256) {
        const int y = pts[n].y;
        lo_a = min(lo_a, y);
        hi_a = max(hi_a, y);
        if (n >= split) {
            lo_b = min(lo_b, y);
            hi_b = max(hi_b, y);
        }
    }
    s_mm[0][tid] = lo_a;
    s_mm[1][tid] = hi_a;
    s_mm[2][tid] = lo_b;
    s_mm[3][tid] = hi_b;
    __syncthreads();
    for (int step = 128; step > 0; step >>= 1) {
        if (tid < step) {
            s_mm[0][tid] = min(s_mm[0][tid], s_mm[0][tid + step]);
            s_mm[1][tid] = max(s_mm[1][tid], s_mm[1][tid + step]);
            s_mm[2][tid] = min(s_mm[2][tid], s_mm[2][tid + step]);
            s_mm[3][tid] = max(s_mm[3][tid], s_mm[3][tid + step]);
        }
        __syncthreads();
    }
    for (int n = tid; n < N; n += 256) {
        const int g = n >= split ? 2 : 0;
        const long long lo = s_mm[g][0], hi = s_mm[g + 1][0];
        long long idx = hi == lo ? 0 : ((long long)pts[n].y - lo) * 256 / (hi - lo);
        if (idx > 255) idx = 255;
        const float* c = lut + 3 * idx;
        const uint32_t r = (uint32_t)(255.0 * (double)c[0]), gr = (uint32_t)(255.0 * (double)c[1]),
                       b = (uint32_t)(255.0 * (double)c[2]);
        colours[n] = (r & 255u) | (gr & 255u) << 8 | (b & 255u) << 16;
    }
}

// the tiles a drawn segment is binned into: its bounding box grown by the line width, cut to the image
struct TvRect {
    int x0, x1, y0, y1;
    bool drawn;
};
__device__ __forceinline__ TvRect tv_segment_tiles(const int2* __restrict__ pts, long long e, int N, int W, int H) {
    const int2 a = pts[e], b = pts[e + N];
    TvRect r;
    r.drawn = tv_usable(a, W, H) && tv_inside(b, W, H);
    r.x0 = max(min(a.x, b.x) - TV_LINE_W, 0) / TV_TILE;
    r.x1 = min(max(a.x, b.x) + TV_LINE_W, W - 1) / TV_TILE;
    r.y0 = max(min(a.y, b.y) - TV_LINE_W, 0) / TV_TILE;
    r.y1 = min(max(a.y, b.y) + TV_LINE_W, H - 1) / TV_TILE;
    return r;
}

// FILL = false: counts[tile] += 1 per touched tile; FILL = true: the paint index s N + i into the tile's list (any order)
template <bool FILL>
__global__ void __launch_bounds__(256)
    tv_bin_kernel(const int2* __restrict__ pts, long long n_seg, int N, int W, int H, int tiles_x, int32_t* __restrict__ counts,
                  const int32_t* __restrict__ offsets, int32_t* __restrict__ pairs, const int32_t* __restrict__ overflow) {
    if (FILL && overflow[0]) return;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_seg; e += (long long)gridDim.x * blockDim.x) {
        const TvRect r = tv_segment_tiles(pts, e, N, W, H);
        if (!r.drawn) continue;
        for (int ty = r.y0; ty <= r.y1; ++ty)
            for (int tx = r.x0; tx <= r.x1; ++tx) {
                const int tile = ty * tiles_x + tx;
                const int k = atomicAdd(&counts[tile], 1);
                if (FILL) pairs[offsets[tile] + k] = (int32_t)e;
            }
    }
}

// one workgroup: offsets[tile] = the pairs of the tiles before it, offsets[tiles] = all; overflow[0] = they exceed K_cap
__global__ void __launch_bounds__(TV_SCAN_THREADS)
    tv_scan_kernel(const int32_t* __restrict__ counts, int tiles, int K_cap, int32_t* __restrict__ offsets,
                   int32_t* __restrict__ overflow) {
    __shared__ unsigned long long s_part[TV_SCAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (tiles + TV_SCAN_THREADS - 1) / TV_SCAN_THREADS;
    const int lo = min(tid * per, tiles), hi = min(lo + per, tiles);
    unsigned long long sum = 0;
    for (int j = lo; j < hi; ++j) sum += (unsigned long long)counts[j];
    s_part[tid] = sum;
    __syncthreads();
    for (int step = 1; step < TV_SCAN_THREADS; step <<= 1) {
        const unsigned long long add = tid >= step ? s_part[tid - step] : 0ull;
        __syncthreads();
        s_part[tid] += add;
        __syncthreads();
    }
    // (beyond K_cap the lists are never filled or read: the offsets only have to stay ints)
    unsigned long long run = s_part[tid] - sum;
    for (int j = lo; j < hi; ++j) {
        offsets[j] = (int32_t)(run < (unsigned long long)INT_MAX ? run : (unsigned long long)INT_MAX);
        run += (unsigned long long)counts[j];
    }
    if (tid == TV_SCAN_THREADS - 1) {
        const unsigned long long total = s_part[tid];
        offsets[tiles] = (int32_t)(total < (unsigned long long)INT_MAX ? total : (unsigned long long)INT_MAX);
        overflow[0] = total > (unsigned long long)K_cap ? 1 : 0;
    }
}

__global__ void __launch_bounds__(TV_THREADS)
    tv_paint_kernel(const uint8_t* __restrict__ video, const int2* __restrict__ pts, const uint8_t* __restrict__ occluded,
                    const uint32_t* __restrict__ colours, const int32_t* __restrict__ offsets, const int32_t* __restrict__ pairs,
                    const int32_t* __restrict__ overflow, int T, int N, int W, int H, int tiles_x, int tiles,
                    uint8_t* __restrict__ out) {
    __shared__ int4 s_geo[TV_PRIMS];               // ax ay bx by (a disc: its centre twice)
    __shared__ int2 s_meta[TV_PRIMS];              // paint index, width (0: the disc)
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const bool traces = overflow[0] == 0;
    const int marker_base = (T - 1) * N;
    const long long items = (long long)tiles * T;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int t = (int)(item / tiles), tile = (int)(item - (long long)t * tiles);
        const int tx0 = (tile % tiles_x) * TV_TILE, ty0 = (tile / tiles_x) * TV_TILE;
        const int px = tx0 + (tid & (TV_TILE - 1)), py = ty0 + tid / TV_TILE;
        const int start = offsets[tile];
        const int len = (traces && t > 0) ? offsets[tile + 1] - start : 0;
        const int total = N + len;                 // (N + len <= T N: a segment is binned at most once per tile)
        int best = -1;
        for (int base = 0; base < total; base += TV_STAGE) {
            if (tid == 0) s_n = 0;
            __syncthreads();
            const int c = base + tid;
            if (c < N) {
                const int2 p = pts[(long long)t * N + c];
                if (tv_usable(p, W, H) && p.x + TV_MARK_R >= tx0 && p.x - TV_MARK_R < tx0 + TV_TILE && p.y + TV_MARK_R >= ty0 &&
                    p.y - TV_MARK_R < ty0 + TV_TILE) {
                    if (occluded[(long long)t * N + c]) {
                        const int k = atomicAdd(&s_n, 2);
                        s_geo[k] = make_int4(p.x - TV_MARK_R, p.y, p.x + TV_MARK_R, p.y);
                        s_geo[k + 1] = make_int4(p.x, p.y - TV_MARK_R, p.x, p.y + TV_MARK_R);
                        s_meta[k] = s_meta[k + 1] = make_int2(marker_base + c, TV_CROSS_W);
                    } else {
                        const int k = atomicAdd(&s_n, 1);
                        s_geo[k] = make_int4(p.x, p.y, p.x, p.y);
                        s_meta[k] = make_int2(marker_base + c, 0);
                    }
                }
            } else if (c < total) {
                const int e = pairs[start + (c - N)];
                if (e / N < t) {
                    const int2 a = pts[e], b = pts[(long long)e + N];
                    const int k = atomicAdd(&s_n, 1);
                    s_geo[k] = make_int4(a.x, a.y, b.x, b.y);
                    s_meta[k] = make_int2(e, TV_LINE_W);
                }
            }
            __syncthreads();
            const int n = s_n;
            for (int k = 0; k < n; ++k) {
                const int2 m = s_meta[k];
                if (m.x <= best) continue;
                const int4 g = s_geo[k];
                bool hit;
                if (m.y == 0) {
                    const int dx = px - g.x, dy = py - g.y;
                    hit = dx * dx + dy * dy <= TV_MARK_R * TV_MARK_R + 2;
                } else {
                    hit = tv_on_segment(px, py, g, m.y);
                }
                if (hit) best = m.x;
            }
            __syncthreads();
        }
        if (px < W && py < H) {
            const long long o = (((long long)t * H + py) * W + px) * 3;
            uint8_t r, g, b;
            if (best >= 0) {
                const uint32_t c = colours[best % N];
                r = (uint8_t)(c & 255u), g = (uint8_t)(c >> 8 & 255u), b = (uint8_t)(c >> 16 & 255u);
            } else {
                r = video[o], g = video[o + 1], b = video[o + 2];
            }
            out[o] = r;
            out[o + 1] = g;
            out[o + 2] = b;
        }
    }
}

struct TvWorkspace {
    int2* pts;                 // [T N]
    uint32_t* colours;         // [N]
    int32_t* counts;           // [tiles] pairs per tile, then [tiles] the fill's cursors: zeroed together
    int32_t* offsets;          // [tiles + 1]
    int32_t* pairs;            // [K_cap]
    size_t bytes;
};

static bool tv_sizes_ok(int T, int N, int W, int H, int K_cap) {
    return T >= 0 && N >= 0 && W > 0 && H > 0 && K_cap > 0 && W <= TV_MAX_SIDE && H <= TV_MAX_SIDE &&
           (long long)T * N <= (long long)INT_MAX;
}

static TvWorkspace tv_carve(void* base, int T, int N, int W, int H, int K_cap) {
    const size_t tiles = tile_grid(W, H).tiles();
    Arena a;
    a.base = (char*)base;
    TvWorkspace w;
    w.pts = a.take<int2>("pts", (size_t)T * N);
    w.colours = a.take<uint32_t>("colours", (size_t)N);
    w.counts = a.take<int32_t>("counts", 2 * tiles);
    w.offsets = a.take<int32_t>("offsets", tiles + 1);
    w.pairs = a.take<int32_t>("pairs", (size_t)K_cap);
    w.bytes = a.off;
    return w;
}

static int tv_grid(long long n, int block) {
    const long long g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : (g < TV_MAX_GRID ? g : TV_MAX_GRID));
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_track_vis_workspace_bytes(int T, int N, int W, int H, int K_cap) {
    if (!tv_sizes_ok(T, N, W, H, K_cap)) return 0;
    return tv_carve(nullptr, T, N, W, H, K_cap).bytes;
}

int gfl_track_vis(const uint8_t* video, const float* tracks, const uint8_t* occluded, int T, int N, int W, int H,
                  int still_length, const float* lut, int K_cap, uint8_t* out, int32_t* overflow, void* workspace,
                  size_t workspace_bytes, gfl_stream_t stream) {
    if (!tv_sizes_ok(T, N, W, H, K_cap)) return GFL_ERR_INVALID;
    if (!video || !lut || !out || !overflow || !workspace) return GFL_ERR_INVALID;
    if ((long long)T * N > 0 && (!tracks || !occluded)) return GFL_ERR_INVALID;
    const TvWorkspace w = tv_carve(workspace, T, N, W, H, K_cap);
    if (workspace_bytes < w.bytes) return GFL_ERR_INVALID;
    if (T == 0) return GFL_OK;
    hipStream_t s = (hipStream_t)stream;
    const TileGrid tg = tile_grid(W, H);
    const int tiles = tg.T;
    const long long n_pts = (long long)T * N, n_seg = (long long)(T - 1) * N;
    int rc = check(hipMemsetAsync(w.counts, 0, 2 * (size_t)tiles * sizeof(int32_t), s));
    if (rc) return rc;
    tv_points_kernel<<<tv_grid(n_pts, 256), 256, 0, s>>>(tracks, n_pts, w.pts);
    tv_colours_kernel<<<1, 256, 0, s>>>(w.pts, N, still_length, lut, w.colours);
    tv_bin_kernel<false><<<tv_grid(n_seg, 256), 256, 0, s>>>(w.pts, n_seg, N, W, H, tg.gx, w.counts, nullptr, nullptr, nullptr);
    tv_scan_kernel<<<1, TV_SCAN_THREADS, 0, s>>>(w.counts, tiles, K_cap, w.offsets, overflow);
    tv_bin_kernel<true><<<tv_grid(n_seg, 256), 256, 0, s>>>(w.pts, n_seg, N, W, H, tg.gx, w.counts + tiles, w.offsets, w.pairs,
                                                            overflow);
    tv_paint_kernel<<<tv_grid((long long)tiles * T, 1), TV_THREADS, 0, s>>>(video, w.pts, occluded, w.colours, w.offsets, w.pairs,
                                                                           overflow, T, N, W, H, tg.gx, tiles, out);
    return check_launch();
}

}  // extern "C"
