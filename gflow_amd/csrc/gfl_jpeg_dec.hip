// Baseline JPEG decoded on the device (include/gflow_hip.h, "video files": Decoding), the counterpart of gfl_jpeg.hip: the
// entropy-coded data of T images of one shape -> [T][H][W][C] uint8 with libjpeg's bits.  The arithmetic is gfl_jpeg_dec.hpp's;
// here are the three launches around it:
//   entropy   a lane per unit (a restart interval of a frame), a workgroup's lanes all of ONE frame, whose four Huffman
//             tables are built in LDS.  Latency-bound and divergent by nature: every lane walks its own bit stream, and a file
//             without restart markers is one lane.
//   idct      eight lanes per 8x8 block: a lane per column (dequantise, pass 1, through LDS), then a lane per row (pass 2,
//             + 128, clamp), eight samples stored at once into the component's plane.
//   pixels    a lane per four pixels of a row: chroma upsampled from the cropped planes, the colour transform, 12 bytes
//             written as three words where the row allows it.
// The coefficients are zeroed and the status array set to "never run" by two memsets on the same stream.  No allocation, no
// host synchronisation.
#include <algorithm>

#include "gfl_common.hpp"
#include "gfl_jpeg_dec.hpp"

namespace gfl {

constexpr int JD_ENTROPY_BLOCK = 64;
constexpr int JD_BLOCK = 256;
constexpr int JD_IDCT_PER_GROUP = JD_BLOCK / 8;     // 8x8 blocks per workgroup

__global__ void __launch_bounds__(JD_ENTROPY_BLOCK)
    jpeg_dec_entropy_kernel(const uint8_t* __restrict__ bytes, long long n_bytes, const gfl_jpeg_unit* __restrict__ units,
                            long long n_units, const gfl_jpeg_frame_tables* __restrict__ tables, jd::Shape s,
                            int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    __shared__ jd::Huff huff[4];
    const int t = blockIdx.x;
    const gfl_jpeg_frame_tables& ft = tables[t];
    if (threadIdx.x < 4) jd::build_huff(ft.huff[threadIdx.x], huff[threadIdx.x]);
    __syncthreads();
    // the frame's units, clipped to the array whatever the record says
    long long first = ft.first_unit, n = ft.n_units;
    if (first < 0 || n < 0 || first > n_units) return;
    if (n > n_units - first) n = n_units - first;
    for (long long i = (long long)blockIdx.y * JD_ENTROPY_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.y * JD_ENTROPY_BLOCK) {
        const gfl_jpeg_unit u = units[first + i];
        status[first + i] = jd::decode_unit(bytes, n_bytes, u, t, ft, huff, s, coef + (size_t)t * s.nblk * 64);
    }
}

__global__ void __launch_bounds__(JD_BLOCK)
    jpeg_dec_idct_kernel(const int16_t* __restrict__ coef, const gfl_jpeg_frame_tables* __restrict__ tables, jd::Shape s,
                         uint8_t* __restrict__ planes) {
    __shared__ int32_t ws[JD_IDCT_PER_GROUP][64 + 8];
    const int g = threadIdx.x >> 3, l = threadIdx.x & 7;
    const long long blk = (long long)blockIdx.x * JD_IDCT_PER_GROUP + g;
    const bool live = blk < (long long)s.T * s.nblk;
    int t = 0, b = 0;
    if (live) {
        t = (int)(blk / s.nblk);
        b = (int)(blk - (long long)t * s.nblk);
    }
    const jd::BlockAt at = jd::block_at(s, b);
    if (live) {
        const gfl_jpeg_frame_tables& ft = tables[t];
        jd::idct_column(coef + (size_t)blk * 64, ft.q[ft.qsel[at.c] & 3], l, ws[g]);
    }
    __syncthreads();
    if (live) {
        alignas(8) uint8_t row[8];
        jd::idct_row(ws[g], l, row);
        uint8_t* dst = planes + (size_t)t * s.plane_bytes + at.sample + (size_t)l * at.stride;
        *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(row);      // (planes are whole blocks: 8-byte aligned)
    }
}

__global__ void __launch_bounds__(JD_BLOCK)
    jpeg_dec_pixels_kernel(const uint8_t* __restrict__ planes, jd::Shape s, uint8_t* __restrict__ images) {
    const int w4 = (s.W + 3) >> 2;
    const long long i = (long long)blockIdx.x * JD_BLOCK + threadIdx.x;
    if (i >= (long long)w4 * s.H) return;
    const int y = (int)(i / w4), x0 = (int)(i - (long long)y * w4) * 4;
    const int n = min(4, s.W - x0);
    for (int t = blockIdx.y; t < s.T; t += gridDim.y) {
        const uint8_t* pl = planes + (size_t)t * s.plane_bytes;
        uint8_t* dst = images + (((size_t)t * s.H + y) * s.W + x0) * s.C;
        alignas(4) uint8_t px[12];
        for (int k = 0; k < n; ++k) jd::pixel_at(pl, s, x0 + k, y, px + k * s.C);
        const int nb = n * s.C;
        if (((uintptr_t)dst & 3) == 0 && (nb & 3) == 0) {
            for (int k = 0; k < nb; k += 4) *reinterpret_cast<uint32_t*>(dst + k) = *reinterpret_cast<const uint32_t*>(px + k);
        } else {
            for (int k = 0; k < nb; ++k) dst[k] = px[k];
        }
    }
}

struct JpegDecWorkspace { int16_t* coef; uint8_t* planes; };
static JpegDecWorkspace jpeg_dec_carve(Arena& ar, const jd::Shape& s) {
    JpegDecWorkspace w;
    w.coef = ar.take<int16_t>("coefficients", (size_t)s.T * s.nblk * 64);
    w.planes = ar.take<uint8_t>("planes", (size_t)s.T * (size_t)s.plane_bytes);
    return w;
}

}  // namespace gfl

using namespace gfl;

extern "C" {

int gfl_jpeg_decode_struct_bytes(int* sizeof_unit, int* sizeof_frame_tables) {
    if (!sizeof_unit || !sizeof_frame_tables) return GFL_ERR_INVALID;
    *sizeof_unit = (int)sizeof(gfl_jpeg_unit);
    *sizeof_frame_tables = (int)sizeof(gfl_jpeg_frame_tables);
    return GFL_OK;
}

size_t gfl_jpeg_decode_workspace_bytes(int T, int C, int W, int H, int hs, int vs, int64_t n_units) {
    jd::Shape s;
    if (n_units < 1 || !jd::make_shape(T, C, W, H, hs, vs, s)) return 0;
    Arena ar;
    jpeg_dec_carve(ar, s);
    return ar.off;
}

int gfl_jpeg_decode(const uint8_t* bytes, int64_t n_bytes, const gfl_jpeg_unit* units, int64_t n_units,
                    const gfl_jpeg_frame_tables* tables, int T, int C, int W, int H, int hs, int vs, uint8_t* images,
                    int32_t* unit_status, void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    jd::Shape s;
    if (!bytes || !units || !tables || !images || !unit_status || !workspace || n_bytes < 0 || n_units < 1) return GFL_ERR_INVALID;
    if (!jd::make_shape(T, C, W, H, hs, vs, s)) return GFL_ERR_INVALID;
    if (((uintptr_t)workspace & 15) || ((uintptr_t)units & 7) || ((uintptr_t)tables & 3) || ((uintptr_t)unit_status & 3))
        return GFL_ERR_INVALID;
    Arena ar;
    ar.base = (char*)workspace;
    const JpegDecWorkspace w = jpeg_dec_carve(ar, s);
    if (workspace_bytes < ar.off) return GFL_ERR_WORKSPACE;
    const hipStream_t st = (hipStream_t)stream;
    if (int rc = check(hipMemsetAsync(w.coef, 0, (size_t)s.T * s.nblk * 64 * sizeof(int16_t), st))) return rc;
    if (int rc = check(hipMemsetAsync(unit_status, 0xff, (size_t)n_units * sizeof(int32_t), st))) return rc;       // -1
    const long long per_frame = (n_units + T - 1) / T;
    const int gy = (int)std::min<long long>(std::max<long long>((per_frame + JD_ENTROPY_BLOCK - 1) / JD_ENTROPY_BLOCK, 1), 1024);
    jpeg_dec_entropy_kernel<<<dim3(T, gy), JD_ENTROPY_BLOCK, 0, st>>>(bytes, (long long)n_bytes, units, (long long)n_units, tables,
                                                                      s, w.coef, unit_status);
    if (int rc = check_launch()) return rc;
    const long long blocks = (long long)s.T * s.nblk;
    jpeg_dec_idct_kernel<<<(unsigned)((blocks + JD_IDCT_PER_GROUP - 1) / JD_IDCT_PER_GROUP), JD_BLOCK, 0, st>>>(w.coef, tables, s,
                                                                                                                 w.planes);
    if (int rc = check_launch()) return rc;
    const long long quads = (long long)((W + 3) / 4) * H;
    jpeg_dec_pixels_kernel<<<dim3((unsigned)((quads + JD_BLOCK - 1) / JD_BLOCK), (unsigned)std::min(T, 65535)), JD_BLOCK, 0, st>>>(
        w.planes, s, images);
    return check_launch();
}

}  // extern "C"
