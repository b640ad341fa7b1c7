// Batched inference rasteriser: many (splat range, camera) jobs per call, uint8 written by the blend itself
// (gfl_render_batch, include/gflow_hip.h -- the call sites it replaces are viewer.py:201-228 and render.py:6-108).
//
// A (job, tile) pair is a VIRTUAL TILE vt = job * T + tile; everything below is the single-image pipeline over J * T of them.
// Six launches per call, whatever J, the row counts or the data are:
//   setup      : the jobs' row ranges become record offsets (a prefix over the jobs), the virtual tiles' counters are cleared;
//   preprocess : one lane per (job, row): projection, covariance, EWA, the 12-float record -- the device functions and the order
//                of preprocess_block's op_mode (gfl_fit_bin.hip), with the camera of the ROW'S JOB -- and one integer add per
//                (splat, tile) pair into the virtual tile's counter: the fit's tile walk (walk_tiles_lane / _wave, gfl_fit.hpp);
//   scan       : one workgroup turns the counters into list offsets in (job, tile) order, cuts the pool at K_cap and flags the
//                jobs that lost pairs;
//   scatter    : the lanes of the preprocess walk their tiles again and write the keys pair_key(depth, record row);
//   tile sort  : gfl_tile_sort_only over the J * T segments (gfl_tile_sort.hpp: unique keys, so arrival order is irrelevant);
//   blend      : a workgroup per virtual tile: the plain tile composite (plain_tile_blend, gfl_fit.hpp -- center_blend_kernel's,
//                gfl_fit_snap.hip) over the true records, four sums per pixel.  No checkpoints, no n_contrib / final_T, no
//                queues: nothing here is for a backward.
//
// Truncation.  Lists are laid out in (job, tile) order.  A list that does not fit below K_cap WHOLE gets no room at all, and
// neither does any list behind it: which keys of a cut list survive would depend on the order the scatter's lanes arrive in,
// and an image must not.  So a truncated job is reproducible too, every job before the cut is untouched by it, and
// overflow[j] = 1 exactly for the jobs that own a non-empty list at or behind the cut.
#include "gfl_fit.hpp"

namespace gfl {

constexpr int RB_BLOCK = 256;
constexpr int RB_CAM = 17;            // floats per job: fx fy cx cy | extr 3x4 | bg
constexpr int RB_SCAN = 1024;
constexpr int RB_VT_MAX = 1 << 28;    // virtual tiles per call

__device__ __forceinline__ int rb_sat_add(int a, int b) {
    const long long s = (long long)a + (long long)b;
    return s > 0x7fffffffLL ? 0x7fffffff : (int)s;
}

// the job of record row v: the largest j with off[j] <= v (meta[j] = {record offset, first params row}; offsets do not decrease,
// v < meta[J].x, so that job has v inside its range even when jobs of count 0 share its offset)
__device__ __forceinline__ int rb_find_job(const int2* __restrict__ meta, int J, int v) {
    int lo = 0, hi = J;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (meta[mid].x <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------- setup
// block 0: record offsets.  A range that leaves [0, R), or records beyond rows_total, are dropped and flagged 2.
__global__ void __launch_bounds__(RB_BLOCK) rb_setup_kernel(const int32_t* __restrict__ job_rows, int J, int R, int rows_total,
                                                            int2* __restrict__ meta, int32_t* __restrict__ overflow,
                                                            int32_t* __restrict__ vt_count, int VT) {
    for (int i = blockIdx.x * RB_BLOCK + threadIdx.x; i < VT; i += gridDim.x * RB_BLOCK) vt_count[i] = 0;
    if (blockIdx.x != 0) return;
    __shared__ int32_t s_sum[RB_BLOCK];
    const int tid = threadIdx.x;
    const int per = (J + RB_BLOCK - 1) / RB_BLOCK;
    const int j0 = min(J, tid * per), j1 = min(J, j0 + per);
    auto count_of = [&](int j, int& first) {
        first = job_rows[2 * j];
        const int cnt = job_rows[2 * j + 1];
        const bool ok = first >= 0 && cnt >= 0 && first <= R && cnt <= R - first;
        if (!ok) first = 0;
        return ok ? cnt : -1;
    };
    int local = 0;
    for (int j = j0; j < j1; ++j) {
        int first;
        local = rb_sat_add(local, max(count_of(j, first), 0));
    }
    s_sum[tid] = local;
    __syncthreads();
    int run = 0;
    for (int t = 0; t < tid; ++t) run = rb_sat_add(run, s_sum[t]);
    for (int j = j0; j < j1; ++j) {
        int first;
        const int cnt = count_of(j, first);
        const int end = rb_sat_add(run, max(cnt, 0));
        const int off_c = min(run, rows_total), end_c = min(end, rows_total);
        meta[j] = make_int2(off_c, first);
        overflow[j] = (cnt < 0 || end_c - off_c < cnt) ? 2 : 0;
        run = end;
    }
    if (tid == RB_BLOCK - 1) meta[J] = make_int2(min(run, rows_total), 0);
}

// ---------------------------------------------------------------- preprocess
__global__ void __launch_bounds__(RB_BLOCK) rb_preprocess_kernel(const float* __restrict__ params, const int2* __restrict__ meta,
                                                                 const float* __restrict__ job_cam, int J, int W, int H, int gx,
                                                                 int gy, float* __restrict__ rec, float* __restrict__ out_rec,
                                                                 int32_t* __restrict__ vt_count) {
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    const int total = meta[J].x;
    float u = 0.f, v = 0.f, cutoff = 0.f;
    TileSpan span = {};
    int base = 0;                                 // the first virtual tile of the row's job
    if (i < total) {
        const int job = rb_find_job(meta, J, i);
        const int2 m = meta[job];
        const float4* prow = reinterpret_cast<const float4*>(params + (size_t)(m.y + (i - m.x)) * ROW);
        const float4 r0 = prow[0], r1 = prow[1], r2 = prow[2], r3 = prow[3];
        const float* cam = job_cam + (size_t)job * RB_CAM;
        const Cam c = load_cam(cam, cam + 4);
        // ---- preprocess_block's op_mode, term for term
        const Splat s = splat_from_row(r0, r1, r2, r3, true);
        const Proj p = project_fwd(c, s.x, s.y, s.z, W, H, GFL_NEAREST, GFL_EXTENT);
        float depth = 0.f, A = 0.f, B = 0.f, C = 0.f;
        int rad = 0;
        if (p.vis) {
            float cov[6];
            cov3d_fwd(s.s, s.q, cov);
            u = p.u; v = p.v; depth = p.pz;
            const Ewa e = ewa_fwd(c, p.px, p.py, p.pz, cov, W, H);
            if (e.ok) {
                const int r = ewa_radius(e);
                const TileSpan sp = tile_span(u, v, r, gx, gy);
                if (sp.nt() > 0) {
                    rad = r;
                    A = e.c / e.det; B = -e.b / e.det; C = e.a / e.det;
                    cutoff = alpha_cutoff(s.o, e.lam);
                    span = sp;
                }
            }
        }
        base = job * (gx * gy);
        const float4 q0 = make_float4(u, v, A, B), q1 = make_float4(C, s.o, s.c[0], s.c[1]),
                     q2 = make_float4(s.c[2], depth, cutoff, __int_as_float(rad));
        float4* r4 = reinterpret_cast<float4*>(rec + (size_t)i * REC);
        r4[0] = q0; r4[1] = q1; r4[2] = q2;
        if (out_rec) {
            float4* o4 = reinterpret_cast<float4*>(out_rec + (size_t)i * REC);
            o4[0] = q0; o4[1] = q1; o4[2] = q2;
        }
    }
    // (integer adds: the counts do not depend on the order they arrive in)
    const bool wide = span.nt() > WIDE_TILES;
    if (!wide) walk_tiles_lane(u, v, cutoff, span, gx, [&](int t) { atomicAdd(&vt_count[base + t], 1); });
    walk_tiles_wave(wide, u, v, cutoff, span, gx, WalkTag{0ull, base},
                    [&](int t, const WalkTag& src) { atomicAdd(&vt_count[src.base + t], 1); });
}

// ---------------------------------------------------------------- scan
// counts -> offsets in (job, tile) order, cut at the last list that ends at or below K_cap; the counters become the scatter's
// cursors (zero).  One workgroup: a lane owns a run of consecutive virtual tiles.
__global__ void __launch_bounds__(RB_SCAN) rb_scan_kernel(int32_t* __restrict__ vt_count, int VT, int T, int K_cap,
                                                          int32_t* __restrict__ vt_off, int32_t* __restrict__ overflow) {
    __shared__ int32_t s_wave[RB_SCAN / 64];
    __shared__ int32_t s_cut;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int per = (VT + RB_SCAN - 1) / RB_SCAN;
    const int i0 = (int)min((long long)VT, (long long)tid * per), i1 = min(VT, i0 + per);
    if (tid == 0) s_cut = 0;
    int local = 0;
    for (int i = i0; i < i1; ++i) local = rb_sat_add(local, vt_count[i]);
    // (saturating: the ladder of wave_scan_incl with rb_sat_add; the wave totals are folded with it too, so not block_scan_excl)
    const int sc = wave_scan_incl(local, [](int a, int b) { return rb_sat_add(a, b); });
    if (lane == 63) s_wave[wid] = sc;
    __syncthreads();
    int wprefix = 0;
    for (int w = 0; w < wid; ++w) wprefix = rb_sat_add(wprefix, s_wave[w]);
    const int prev = wave_prev_lane(sc);
    const int start = lane == 0 ? wprefix : rb_sat_add(wprefix, prev);
    // the cut: the largest list end that is still <= K_cap (ends do not decrease: this lane's last such end)
    {
        int run = start, cut = start <= K_cap ? start : 0;
        for (int i = i0; i < i1; ++i) {
            run = rb_sat_add(run, vt_count[i]);
            if (run <= K_cap) cut = run;
        }
        atomicMax(&s_cut, cut);
    }
    __syncthreads();
    const int cut = s_cut;
    int run = start;
    for (int i = i0; i < i1; ++i) {
        const int c = vt_count[i];
        vt_off[i] = min(run, cut);
        run = rb_sat_add(run, c);
        if (c > 0 && run > K_cap) atomicOr(&overflow[i / T], 1);      // (the rare path: a list without room)
        vt_count[i] = 0;
    }
    // (every lane whose run ends at VT holds the grand total in `run`: they write the same value)
    if (i1 == VT) vt_off[VT] = min(run, cut);
}

// ---------------------------------------------------------------- scatter
__global__ void __launch_bounds__(RB_BLOCK) rb_scatter_kernel(const float* __restrict__ rec, const int2* __restrict__ meta, int J,
                                                              int gx, int gy, int32_t* __restrict__ cursor,
                                                              const int32_t* __restrict__ vt_off,
                                                              unsigned long long* __restrict__ keys) {
    const int i = blockIdx.x * RB_BLOCK + threadIdx.x;
    const int total = meta[J].x;
    float u = 0.f, v = 0.f, cutoff = 0.f, depth = 0.f;
    TileSpan span = {};
    int base = 0;
    if (i < total) {
        const float4* r4 = reinterpret_cast<const float4*>(rec + (size_t)i * REC);
        const float4 p0 = r4[0], p2 = r4[2];
        const int rad = __float_as_int(p2.w);
        u = p0.x; v = p0.y; cutoff = p2.z; depth = p2.y;
        if (rad > 0) span = tile_span(u, v, rad, gx, gy);
        base = rb_find_job(meta, J, i) * (gx * gy);
    }
    const WalkTag own = {pair_key(depth, i), base};
    auto put = [&](int t, const WalkTag& src) {
        const int vt = src.base + t;
        const int lo = vt_off[vt], hi = vt_off[vt + 1];
        if (hi > lo) {                                     // (a list behind the cut has no room: nothing is written)
            const int pos = lo + atomicAdd(&cursor[vt], 1);
            if (pos < hi) keys[pos] = src.key;
        }
    };
    const bool wide = span.nt() > WIDE_TILES;
    if (!wide) walk_tiles_lane(u, v, cutoff, span, gx, [&](int t) { put(t, own); });
    walk_tiles_wave(wide, u, v, cutoff, span, gx, own, put);
}

// ---------------------------------------------------------------- blend
// LDS per workgroup: 257 records x 48 B + 256 mask bytes + the tile's 16 x 48 uint8 image = 13.4 KB -> eleven workgroups per CU
// by LDS; the register count allows eight, 32 waves per CU.
__global__ void __launch_bounds__(256) rb_blend_kernel(const float* __restrict__ rec, const int32_t* __restrict__ ids,
                                                       const int32_t* __restrict__ tile_range, const float* __restrict__ job_cam,
                                                       int W, int H, int gx, int T, float* __restrict__ out_f32,
                                                       uint8_t* __restrict__ out_u8) {
    __shared__ RecLDS recs[FB + 1];
    __shared__ unsigned char s_mask[FB];
    __shared__ unsigned char s_img[GFL_TILE][GFL_TILE * 3];
    // (neighbouring virtual tiles -- the tiles of one job -- on one XCD: they read the same records)
    const int vt = xcd_logical_block((int)blockIdx.x, (int)gridDim.x);
    const int job = vt / T, tile = vt - job * T;
    const int tx = tile % gx, ty = tile / gx;
    const int tid = threadIdx.x;
    const auto [lx, ly, px, py, inside] = tile_pixel(tx, ty, W, H);
    const float bg = job_cam[(size_t)job * RB_CAM + 16];
    float Tr, a[4];
    plain_tile_blend<4>(ids, tile_range[2 * vt], tile_range[2 * vt + 1], tx, ty, pixf(px), pixf(py), inside, recs, s_mask,
                        [&](int g, float4& p0, float4& p1, float4& p2) {
                            const float4* r4 = reinterpret_cast<const float4*>(rec + (size_t)g * REC);
                            p0 = r4[0]; p1 = r4[1]; p2 = r4[2];
                        }, Tr, a);
    const float o0 = fmaf(Tr, bg, a[0]), o1 = fmaf(Tr, bg, a[1]), o2 = fmaf(Tr, bg, a[2]), o3 = fmaf(Tr, bg, a[3]);
    const size_t plane = (size_t)H * W;
    if (out_f32 && inside) {
        float* o = out_f32 + (size_t)job * 4 * plane + (size_t)py * W + px;
        o[0] = o0; o[plane] = o1; o[2 * plane] = o2; o[3 * plane] = o3;
    }
    if (out_u8) {
        // Three bytes per pixel, made wide: the tile's 16 rows of up to 48 bytes are assembled in LDS (the bytes of the very
        // floats above), then sixteen lanes per row store the row's aligned middle as dwords -- up to twelve -- and the up to
        // three bytes before and behind it one by one (a row starts at byte 3 (py W + 16 tx) of its image: any alignment).
        s_img[ly][lx * 3 + 0] = img_u8(o0); s_img[ly][lx * 3 + 1] = img_u8(o1); s_img[ly][lx * 3 + 2] = img_u8(o2);
        __syncthreads();
        const int r = tid >> 4, k = tid & 15;
        const int ry = ty * GFL_TILE + r;
        if (ry < H) {
            uint8_t* p = out_u8 + ((size_t)job * plane + (size_t)ry * W + (size_t)tx * GFL_TILE) * 3;
            const int L = 3 * min(GFL_TILE, W - tx * GFL_TILE);
            const int head = min((int)((4u - (unsigned)((uintptr_t)p & 3u)) & 3u), L);
            const int ndw = (L - head) >> 2, tail = L - head - 4 * ndw;
            const unsigned char* s = s_img[r];
            if (k < ndw) {
                const int o = head + 4 * k;
                const uint32_t word = (uint32_t)s[o] | ((uint32_t)s[o + 1] << 8) | ((uint32_t)s[o + 2] << 16) | ((uint32_t)s[o + 3] << 24);
                *reinterpret_cast<uint32_t*>(p + o) = word;
            } else if (k >= 12 && k < 15) {
                if (k - 12 < head) p[k - 12] = s[k - 12];
            } else if (k == 15) {
                for (int b = 0; b < tail; ++b) p[head + 4 * ndw + b] = s[head + 4 * ndw + b];
            }
        }
    }
}

struct RbWs {
    int2* meta; float* rec; int32_t* vt_count; int32_t* vt_off; int32_t* tile_range; unsigned long long* keys; int32_t* ids;
    size_t bytes;
};
// (the pair pool -- keys, ids -- comes last: what lies behind the workspace lies behind the pool)
static RbWs rb_ws(void* base, int J, int rows_total, int K_cap, int W, int H) {
    Arena a{(char*)base};
    const size_t VT = (size_t)J * tile_grid(W, H).tiles();
    RbWs w;
    w.meta = a.take<int2>("meta", (size_t)J + 1);
    w.rec = a.take<float>("rec", (size_t)rows_total * REC);
    w.vt_count = a.take<int32_t>("vt_count", VT);
    w.vt_off = a.take<int32_t>("vt_off", VT + 1);
    w.tile_range = a.take<int32_t>("tile_range", 2 * VT);
    w.keys = a.take<unsigned long long>("keys", (size_t)K_cap);
    w.ids = a.take<int32_t>("ids", (size_t)K_cap);
    w.bytes = a.off;
    return w;
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_render_batch_workspace_bytes(int J, int rows_total, int K_cap, int W, int H) {
    if (J < 0 || rows_total < 0 || K_cap <= 0 || W <= 0 || H <= 0) return 0;
    return rb_ws(nullptr, J, rows_total, K_cap, W, H).bytes;
}

int gfl_render_batch(const float* params, int R, const int32_t* job_rows, const float* job_cam, int J, int rows_total, int W,
                     int H, int K_cap, float* out_f32, uint8_t* out_u8, float* out_rec, int32_t* overflow, void* workspace,
                     size_t workspace_bytes, gfl_stream_t stream) {
    if (J < 0 || R < 0 || rows_total < 0 || W <= 0 || H <= 0 || K_cap <= 0) return GFL_ERR_INVALID;
    if (!out_f32 && !out_u8) return GFL_ERR_INVALID;
    if (J == 0) return GFL_OK;
    if (!job_rows || !job_cam || !overflow || !workspace || (rows_total > 0 && !params)) return GFL_ERR_INVALID;
    const auto [gx, gy, T] = tile_grid(W, H);
    if ((long long)J * T > (long long)RB_VT_MAX) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_render_batch_workspace_bytes(J, rows_total, K_cap, W, H)) return GFL_ERR_INVALID;
    const RbWs w = rb_ws(workspace, J, rows_total, K_cap, W, H);
    hipStream_t s = (hipStream_t)stream;
    const int VT = J * T;
    const int row_blocks = max(1, (rows_total + RB_BLOCK - 1) / RB_BLOCK);
    rb_setup_kernel<<<min(1024, 1 + (VT + 4 * RB_BLOCK - 1) / (4 * RB_BLOCK)), RB_BLOCK, 0, s>>>(job_rows, J, R, rows_total, w.meta,
                                                                                               overflow, w.vt_count, VT);
    rb_preprocess_kernel<<<row_blocks, RB_BLOCK, 0, s>>>(params, w.meta, job_cam, J, W, H, gx, gy, w.rec, out_rec, w.vt_count);
    rb_scan_kernel<<<1, RB_SCAN, 0, s>>>(w.vt_count, VT, T, K_cap, w.vt_off, overflow);
    rb_scatter_kernel<<<row_blocks, RB_BLOCK, 0, s>>>(w.rec, w.meta, J, gx, gy, w.vt_count, w.vt_off, w.keys);
    int rc = check_launch();
    if (rc) return rc;
    rc = gfl_tile_sort_only(w.vt_off, VT, K_cap, w.keys, w.ids, w.tile_range, stream);
    if (rc) return rc;
    rb_blend_kernel<<<VT, 256, 0, s>>>(w.rec, w.ids, w.tile_range, job_cam, W, H, gx, T, out_f32, out_u8);
    return check_launch();
}

}  // extern "C"
