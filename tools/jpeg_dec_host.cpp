// The JPEG decode core on the CPU, for the sanitizers: gflow_amd/csrc/gfl_jpeg_dec.hpp is the source the device kernels are
// made of, and this program runs every unit and every block of a call through the same routines.  Build and run:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_dec_host.cpp -o jpeg_dec_host
//   jpeg_dec_host IN OUT
// IN (little endian; tests/test_jpeg_dec_host.py writes it) holds what gfl_jpeg_decode takes:
//   "GJD1", int32 T, C, W, H, hs, vs, int64 n_units, int64 n_bytes, units [n_units], tables [T], bytes [n_bytes]
// OUT: images [T][H][W][C] uint8, then unit_status [n_units] int32.  Exit 0 whatever the data held; 2 on a file or arguments
// the library call would reject.  The byte buffer is allocated at exactly n_bytes, so a read past a unit is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gflow_amd/csrc/gfl_jpeg_dec.hpp"

using namespace gfl;

template <class T>
static bool read_n(FILE* f, T* dst, size_t n) { return n == 0 || fread(dst, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    int32_t head[6];
    int64_t n_units = 0, n_bytes = 0;
    if (!read_n(f, magic, 4) || memcmp(magic, "GJD1", 4) || !read_n(f, head, 6) || !read_n(f, &n_units, 1) || !read_n(f, &n_bytes, 1)) {
        fprintf(stderr, "%s: not a decode container\n", argv[1]);
        return 2;
    }
    jd::Shape s;
    if (n_units < 1 || n_bytes < 0 || !jd::make_shape(head[0], head[1], head[2], head[3], head[4], head[5], s)) {
        fprintf(stderr, "%s: arguments gfl_jpeg_decode rejects\n", argv[1]);
        return 2;
    }
    std::vector<gfl_jpeg_unit> units((size_t)n_units);
    std::vector<gfl_jpeg_frame_tables> tables((size_t)s.T);
    uint8_t* bytes = (uint8_t*)malloc(n_bytes ? (size_t)n_bytes : 1);         // (exactly: the sanitizer guards its end)
    if (!read_n(f, units.data(), units.size()) || !read_n(f, tables.data(), tables.size()) || !read_n(f, bytes, (size_t)n_bytes)) {
        fprintf(stderr, "%s: short file\n", argv[1]);
        return 2;
    }
    fclose(f);

    std::vector<int16_t> coef((size_t)s.T * s.nblk * 64, 0);
    std::vector<uint8_t> planes((size_t)s.T * (size_t)s.plane_bytes, 0);
    std::vector<uint8_t> images((size_t)s.T * s.H * s.W * s.C, 0);
    std::vector<int32_t> status((size_t)n_units, jd::UNIT_NOT_RUN);

    // entropy: frame by frame, the frame's tables, its units clipped to the array as the kernel clips them
    for (int t = 0; t < s.T; ++t) {
        const gfl_jpeg_frame_tables& ft = tables[t];
        jd::Huff huff[4];
        for (int i = 0; i < 4; ++i) jd::build_huff(ft.huff[i], huff[i]);
        long long first = ft.first_unit, n = ft.n_units;
        if (first < 0 || n < 0 || first > n_units) continue;
        if (n > n_units - first) n = n_units - first;
        for (long long i = 0; i < n; ++i)
            status[first + i] = jd::decode_unit(bytes, n_bytes, units[first + i], t, ft, huff, s, coef.data() + (size_t)t * s.nblk * 64);
    }
    // idct: block by block, columns then rows
    for (long long blk = 0; blk < (long long)s.T * s.nblk; ++blk) {
        const int t = (int)(blk / s.nblk), b = (int)(blk - (long long)t * s.nblk);
        const jd::BlockAt at = jd::block_at(s, b);
        const gfl_jpeg_frame_tables& ft = tables[t];
        int32_t ws[64];
        for (int j = 0; j < 8; ++j) jd::idct_column(coef.data() + (size_t)blk * 64, ft.q[ft.qsel[at.c] & 3], j, ws);
        for (int r = 0; r < 8; ++r)
            jd::idct_row(ws, r, planes.data() + (size_t)t * s.plane_bytes + at.sample + (size_t)r * at.stride);
    }
    // pixels
    for (int t = 0; t < s.T; ++t)
        for (int y = 0; y < s.H; ++y)
            for (int x = 0; x < s.W; ++x)
                jd::pixel_at(planes.data() + (size_t)t * s.plane_bytes, s, x, y, images.data() + (((size_t)t * s.H + y) * s.W + x) * s.C);
    free(bytes);

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(images.data(), 1, images.size(), o);
    fwrite(status.data(), sizeof(int32_t), status.size(), o);
    fclose(o);
    return 0;
}
