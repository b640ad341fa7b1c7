// Row composer of the viewer: (frame a, frame b, s, per-group edits) -> row blocks for the batched inference rasteriser
// (gfl_compose_rows, include/gflow_hip.h).  A job blends the rows of two frames of one clip -- a clip's rows keep their index,
// densification only appends --, applies its group's edit to every row and keeps the rows that are still visible, compacted
// in source order.  What it writes is what gfl_render_batch reads: params = out_rows, job_rows = out_job_rows.
//
// A (job, chunk of 256 source rows) pair is a workgroup; three launches per call, whatever J, the counts or the data are:
//   count : one lane per (job, source row): the row's opacity after blend and gain decides whether it stays; a wave's ballot
//           is its keep mask, the four popcounts of a workgroup its chunk's count;
//   scan  : a workgroup per job: the exclusive prefix of the job's chunk counts, its out_job_rows entry and its flag;
//   write : the lanes of the count again: the whole row is blended and edited, and lands at
//           j * rows_max + chunk offset + popcounts of the waves before + popcount of the lanes before.
// A position is a function of the keep masks alone: no atomic decides one, and nothing depends on the order lanes arrive in.
// The write trusts the masks the count stored (it does not decide a second time), so the two launches cannot disagree.
#include "gfl_math.hpp"

namespace gfl {

constexpr int CR_BLOCK = 256;
constexpr int CR_WAVES = CR_BLOCK / WAVE;
constexpr int CR_ROW = 16;                     // floats per row (rows_block's layout)
constexpr int CR_EDIT = 16;                    // floats per edit: gain | size | q wxyz | pivot | shift | tint | mix
constexpr long long CR_CHUNKS_MAX = 1ll << 30; // (job, chunk) pairs per call

struct CrJob {
    int first_a, count_a, first_b, count_b;
    int n;                                     // source rows max(count_a, count_b); -1: the job is refused (flag 2, no rows)
};

__device__ __forceinline__ CrJob cr_job(const int32_t* __restrict__ job_src, int j, int R, int rows_max) {
    CrJob b;
    b.first_a = job_src[4 * j]; b.count_a = job_src[4 * j + 1]; b.first_b = job_src[4 * j + 2]; b.count_b = job_src[4 * j + 3];
    auto inside = [&](int first, int cnt) { return first >= 0 && cnt >= 0 && first <= R && cnt <= R - first; };
    const int n = max(b.count_a, b.count_b);
    b.n = (inside(b.first_a, b.count_a) && inside(b.first_b, b.count_b) && n <= rows_max) ? n : -1;
    return b;
}

// the blended opacity: count and write call this one function
__device__ __forceinline__ float cr_opacity(bool in_a, bool in_b, float s, float oa, float ob) {
#pragma clang fp contract(off)
    if (in_a && in_b) return s == 0.f ? oa : (s == 1.f ? ob : fmaf(s, ob - oa, oa));
    return in_b ? ob * s : oa * (1.f - s);
}
__device__ __forceinline__ float cr_gain(float o, float gain) { return fminf(o * gain, 1.f); }

__device__ __forceinline__ const float* cr_edit_of(const float* __restrict__ job_edit, int G, int j, int group) {
    return (job_edit && group < G) ? job_edit + ((size_t)j * G + group) * CR_EDIT : nullptr;
}

__device__ __forceinline__ void cr_normalise(float (&q)[4]) {
#pragma clang fp contract(off)
    const float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (n2 > 0.f) {
        const float inv = 1.f / sqrtf(n2);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] *= inv;
    }
}

__device__ __forceinline__ void cr_load_row(const float* __restrict__ params, int row, float (&v)[CR_ROW]) {
    const float4* p = reinterpret_cast<const float4*>(params + (size_t)row * CR_ROW);
    const float4 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3];
    v[0] = r0.x; v[1] = r0.y; v[2] = r0.z; v[3] = r0.w; v[4] = r1.x; v[5] = r1.y; v[6] = r1.z; v[7] = r1.w;
    v[8] = r2.x; v[9] = r2.y; v[10] = r2.z; v[11] = r2.w; v[12] = r3.x; v[13] = r3.y; v[14] = r3.z; v[15] = r3.w;
}

// ---------------------------------------------------------------- count
__global__ void __launch_bounds__(CR_BLOCK) cr_count_kernel(const float* __restrict__ params, const uint8_t* __restrict__ labels,
                                                            int R, const int32_t* __restrict__ job_src,
                                                            const float* __restrict__ job_s, const float* __restrict__ job_edit,
                                                            int G, int rows_max, int C, unsigned long long* __restrict__ masks,
                                                            int32_t* __restrict__ counts) {
    __shared__ int32_t s_cnt[CR_WAVES];
    const int j = (int)blockIdx.x / C, c = (int)blockIdx.x - j * C;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const CrJob job = cr_job(job_src, j, R, rows_max);
    const int i = c * CR_BLOCK + tid;
    bool keep = false;
    if (i < job.n) {
        const bool in_a = i < job.count_a, in_b = i < job.count_b;
        const int ra = job.first_a + i, rb = job.first_b + i;
        const float oa = in_a ? params[(size_t)ra * CR_ROW + 10] : 0.f, ob = in_b ? params[(size_t)rb * CR_ROW + 10] : 0.f;
        float o = cr_opacity(in_a, in_b, job_s[j], oa, ob);
        const int group = labels ? (int)labels[in_a ? ra : rb] : 0;
        const float* e = cr_edit_of(job_edit, G, j, group);
        if (e) o = cr_gain(o, e[0]);
        keep = !(o <= 0.f);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) {
        masks[(size_t)blockIdx.x * CR_WAVES + wid] = m;
        s_cnt[wid] = __popcll(m);
    }
    __syncthreads();
    if (tid == 0) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// ---------------------------------------------------------------- scan
// a workgroup per job; a lane owns a run of consecutive chunks (a job's counts sum to at most rows_max: no 32-bit overflow)
__global__ void __launch_bounds__(CR_BLOCK) cr_scan_kernel(const int32_t* __restrict__ job_src, int R, int rows_max, int C,
                                                           const int32_t* __restrict__ counts, int32_t* __restrict__ offs,
                                                           int32_t* __restrict__ out_job_rows, int32_t* __restrict__ flags) {
    __shared__ int32_t s_sum[CR_BLOCK];
    const int j = blockIdx.x, tid = threadIdx.x;
    const int per = (C + CR_BLOCK - 1) / CR_BLOCK;
    const int i0 = (int)min((long long)C, (long long)tid * per), i1 = min(C, i0 + per);
    const int32_t* cnt = counts + (size_t)j * C;
    int32_t* off = offs + (size_t)j * C;
    int local = 0;
    for (int i = i0; i < i1; ++i) local += cnt[i];
    s_sum[tid] = local;
    __syncthreads();
    int run = 0;
    for (int t = 0; t < tid; ++t) run += s_sum[t];
    for (int i = i0; i < i1; ++i) {
        off[i] = run;
        run += cnt[i];
    }
    if (tid == CR_BLOCK - 1) {                  // (the last lane's run ends at the job's total)
        out_job_rows[2 * j] = j * rows_max;
        out_job_rows[2 * j + 1] = run;
        flags[j] = cr_job(job_src, j, R, rows_max).n < 0 ? 2 : 0;
    }
}

// ---------------------------------------------------------------- write
__global__ void __launch_bounds__(CR_BLOCK) cr_write_kernel(const float* __restrict__ params, const uint8_t* __restrict__ labels,
                                                            int R, const int32_t* __restrict__ job_src,
                                                            const float* __restrict__ job_s, const float* __restrict__ job_edit,
                                                            int G, int rows_max, int C,
                                                            const unsigned long long* __restrict__ masks,
                                                            const int32_t* __restrict__ offs, float* __restrict__ out_rows) {
#pragma clang fp contract(off)     // (every fused multiply-add below is written out: one operation order, the one the tests restate)
    const int j = (int)blockIdx.x / C, c = (int)blockIdx.x - j * C;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const unsigned long long* bm = masks + (size_t)blockIdx.x * CR_WAVES;
    const unsigned long long m = bm[wid];
    if (!((m >> lane) & 1ull)) return;          // (a set bit: i < job.n of an accepted job, and the row stays)
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wid; ++w) rank += __popcll(bm[w]);
    const CrJob job = cr_job(job_src, j, R, rows_max);
    const int i = c * CR_BLOCK + tid;
    const bool in_a = i < job.count_a, in_b = i < job.count_b;
    const int ra = job.first_a + i, rb = job.first_b + i;
    const float s = job_s[j];
    float v[CR_ROW];
    if (in_a && in_b) {
        float a[CR_ROW], b[CR_ROW];
        cr_load_row(params, ra, a);
        cr_load_row(params, rb, b);
        if (s == 0.f || s == 1.f) {
#pragma unroll
            for (int k = 0; k < CR_ROW; ++k) v[k] = s == 0.f ? a[k] : b[k];
        } else {
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = fmaf(s, b[k] - a[k], a[k]);
            const float dot = a[6] * b[6] + a[7] * b[7] + a[8] * b[8] + a[9] * b[9];
            float q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = fmaf(s, (dot < 0.f ? -b[6 + k] : b[6 + k]) - a[6 + k], a[6 + k]);
            cr_normalise(q);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[6 + k] = q[k];
            v[10] = cr_opacity(true, true, s, a[10], b[10]);
#pragma unroll
            for (int k = 11; k < 14; ++k) v[k] = fmaf(s, b[k] - a[k], a[k]);
            v[14] = a[14]; v[15] = a[15];
        }
    } else {
        cr_load_row(params, in_a ? ra : rb, v);
        v[10] = cr_opacity(in_a, in_b, s, v[10], v[10]);
    }
    const int group = labels ? (int)labels[in_a ? ra : rb] : 0;
    const float* ep = cr_edit_of(job_edit, G, j, group);
    if (ep) {
        float e[CR_EDIT];
        cr_load_row(ep, 0, e);
        const float size = e[1];
        v[10] = cr_gain(v[10], e[0]);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[11 + k] = fmaf(e[15], e[12 + k] - v[11 + k], v[11 + k]);
        const bool still = size == 1.f && fabsf(e[2]) == 1.f && e[3] == 0.f && e[4] == 0.f && e[5] == 0.f && e[9] == 0.f &&
                           e[10] == 0.f && e[11] == 0.f;
        if (!still) {
            float Rm[9];
            quat_rot(e[2], e[3], e[4], e[5], Rm);
            const float d0 = v[0] - e[6], d1 = v[1] - e[7], d2 = v[2] - e[8];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float r = fmaf(Rm[3 * k + 2], d2, fmaf(Rm[3 * k + 1], d1, Rm[3 * k] * d0));
                v[k] = fmaf(size, r, e[6 + k]) + e[9 + k];
                v[3 + k] = size * v[3 + k];
            }
            // q (x) rotate, Hamilton product in wxyz
            const float qw = e[2], qx = e[3], qy = e[4], qz = e[5], rw = v[6], rx = v[7], ry = v[8], rz = v[9];
            float p[4];
            p[0] = qw * rw - qx * rx - qy * ry - qz * rz;
            p[1] = qw * rx + qx * rw + qy * rz - qz * ry;
            p[2] = qw * ry - qx * rz + qy * rw + qz * rx;
            p[3] = qw * rz + qx * ry - qy * rx + qz * rw;
            cr_normalise(p);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[6 + k] = p[k];
        }
    }
    float4* o = reinterpret_cast<float4*>(out_rows + ((size_t)j * rows_max + (size_t)(offs[blockIdx.x] + rank)) * CR_ROW);
    o[0] = make_float4(v[0], v[1], v[2], v[3]);
    o[1] = make_float4(v[4], v[5], v[6], v[7]);
    o[2] = make_float4(v[8], v[9], v[10], v[11]);
    o[3] = make_float4(v[12], v[13], v[14], v[15]);
}

static int cr_chunks(int rows_max) { return max(1, (rows_max + CR_BLOCK - 1) / CR_BLOCK); }

// J >= 0, rows_max >= 0; false where the call's extents do not fit (out_job_rows is 32-bit, a grid has a limit)
static bool cr_extents_ok(int J, int rows_max) {
    return (long long)J * rows_max <= 0x7fffffffLL && (long long)J * cr_chunks(rows_max) <= CR_CHUNKS_MAX;
}

struct CrWs {
    int32_t* counts; int32_t* offs; unsigned long long* masks;
    size_t bytes;
};
static CrWs cr_ws(void* base, int J, int rows_max) {
    Arena a{(char*)base};
    const size_t chunks = (size_t)J * cr_chunks(rows_max);
    CrWs w;
    w.counts = a.take<int32_t>("counts", chunks);
    w.offs = a.take<int32_t>("offs", chunks);
    w.masks = a.take<unsigned long long>("masks", chunks * CR_WAVES);
    w.bytes = a.off;
    return w;
}

}  // namespace gfl

using namespace gfl;

extern "C" {

size_t gfl_compose_rows_workspace_bytes(int J, int rows_max) {
    if (J < 0 || rows_max < 0 || !cr_extents_ok(J, rows_max)) return 0;
    return cr_ws(nullptr, J, rows_max).bytes;
}

int gfl_compose_rows(const float* params, const uint8_t* labels, int R, const int32_t* job_src, const float* job_s,
                     const float* job_edit, int G, int J, int rows_max, float* out_rows, int32_t* out_job_rows, int32_t* flags,
                     void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    if (J < 0 || R < 0 || rows_max < 0) return GFL_ERR_INVALID;
    if (job_edit && (G < 1 || G > 8)) return GFL_ERR_INVALID;
    if (J == 0) return GFL_OK;
    if (!job_src || !job_s || !out_job_rows || !flags || !workspace || (R > 0 && !params) || (rows_max > 0 && !out_rows))
        return GFL_ERR_INVALID;
    if (!cr_extents_ok(J, rows_max)) return GFL_ERR_INVALID;
    if (workspace_bytes < gfl_compose_rows_workspace_bytes(J, rows_max)) return GFL_ERR_INVALID;
    const CrWs w = cr_ws(workspace, J, rows_max);
    hipStream_t s = (hipStream_t)stream;
    const int C = cr_chunks(rows_max);
    cr_count_kernel<<<J * C, CR_BLOCK, 0, s>>>(params, labels, R, job_src, job_s, job_edit, G, rows_max, C, w.masks, w.counts);
    cr_scan_kernel<<<J, CR_BLOCK, 0, s>>>(job_src, R, rows_max, C, w.counts, w.offs, out_job_rows, flags);
    cr_write_kernel<<<J * C, CR_BLOCK, 0, s>>>(params, labels, R, job_src, job_s, job_edit, G, rows_max, C, w.masks, w.offs,
                                               out_rows);
    return check_launch();
}

}  // extern "C"
