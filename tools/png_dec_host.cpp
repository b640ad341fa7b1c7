// The PNG decode core on the CPU, for the sanitizers: gflow_amd/csrc/gfl_inflate.hpp is the source the device kernels are made
// of, and this program runs every stream and every row of a call through the same routines.  Build and run:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/png_dec_host.cpp -o png_dec_host
//   png_dec_host IN OUT
// IN (little endian; tests/test_png_dec_host.py writes it) holds what gfl_png_decode takes:
//   "GPD1", int32 T, bpp, W, H, int64 n_bytes, offsets [T + 1] int64, data [n_bytes]
// OUT: images [T][H][W][bpp] uint8, then status [T] int32.  Exit 0 whatever the data held; 2 on a file or arguments the
// library call would reject.  The byte buffer is allocated at exactly n_bytes and every image's rows at exactly
// H * (1 + W * bpp), so a read or a write past either is a report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gflow_amd/csrc/gfl_inflate.hpp"

using namespace gfl;

template <class T>
static bool read_n(FILE* f, T* dst, size_t n) { return n == 0 || fread(dst, sizeof(T), n, f) == n; }

// the Io of the core over plain arrays
struct HostIo {
    const uint8_t* in;          // the stream's first byte
    uint8_t* out;               // `expect` bytes
    int64_t n = 0;
    uint32_t in_byte(int64_t pos) { return in[pos]; }
    uint32_t in_word(int64_t pos) {
        return (uint32_t)in[pos] | ((uint32_t)in[pos + 1] << 8) | ((uint32_t)in[pos + 2] << 16) | ((uint32_t)in[pos + 3] << 24);
    }
    void put(uint32_t byte) { out[n++] = (uint8_t)byte; }
    void copy(int dist, int len) {
        for (int i = 0; i < len; ++i, ++n) out[n] = out[n - dist];
    }
    void stored(int64_t pos, int len) {
        for (int i = 0; i < len; ++i) out[n++] = in[pos + i];
    }
    uint32_t finish() {
        uint32_t s1 = 1, s2 = 0;
        for (int64_t i = 0; i < n; ++i) inf::adler_add(s1, s2, 1, out[i], out[i]);
        return (s2 << 16) | s1;
    }
};

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[4];
    int32_t head[4];
    int64_t n_bytes = 0;
    if (!read_n(f, magic, 4) || memcmp(magic, "GPD1", 4) || !read_n(f, head, 4) || !read_n(f, &n_bytes, 1)) {
        fprintf(stderr, "%s: not a decode container\n", argv[1]);
        return 2;
    }
    const int T = head[0], bpp = head[1], W = head[2], H = head[3];
    if (n_bytes < 0 || !inf::shape_ok(T, bpp, W, H)) {
        fprintf(stderr, "%s: arguments gfl_png_decode rejects\n", argv[1]);
        return 2;
    }
    std::vector<int64_t> offsets((size_t)T + 1);
    uint8_t* data = (uint8_t*)malloc(n_bytes ? (size_t)n_bytes : 1);         // (exactly: the sanitizer guards its end)
    if (!read_n(f, offsets.data(), offsets.size()) || !read_n(f, data, (size_t)n_bytes)) {
        fprintf(stderr, "%s: short file\n", argv[1]);
        return 2;
    }
    fclose(f);

    const int64_t expect = inf::filtered_bytes(bpp, W, H), rowb = (int64_t)W * bpp;
    std::vector<uint8_t> images((size_t)T * H * rowb, 0);
    std::vector<int32_t> status((size_t)T, inf::NOT_RUN);
    inf::Tables* tables = new inf::Tables;
    for (int t = 0; t < T; ++t) {
        // the image's own extent, clipped to the array as the kernel clips it
        int64_t lo = offsets[t], hi = offsets[t + 1];
        lo = lo < 0 ? 0 : (lo > n_bytes ? n_bytes : lo);
        hi = hi < lo ? lo : (hi > n_bytes ? n_bytes : hi);
        uint8_t* stream = (uint8_t*)malloc(hi > lo ? (size_t)(hi - lo) : 1);  // (its own block: a read past the STREAM is a report)
        memcpy(stream, data + lo, (size_t)(hi - lo));
        uint8_t* rows = (uint8_t*)malloc((size_t)expect);
        memset(rows, 0, (size_t)expect);
        HostIo io;
        io.in = stream;
        io.out = rows;
        int32_t rc = inf::inflate(io, hi - lo, expect, *tables);
        if (rc == inf::OK)
            for (int r = 0; r < H; ++r)
                if (rows[r * (1 + rowb)] > 4) rc = inf::BAD_FILTER;
        if (rc == inf::OK) {
            uint8_t* img = images.data() + (size_t)t * H * rowb;
            for (int r = 0; r < H; ++r) {
                const int ft = rows[r * (1 + rowb)];
                const uint8_t* in = rows + r * (1 + rowb) + 1;
                uint8_t* out = img + r * rowb;
                for (int64_t i = 0; i < rowb; ++i) {
                    const uint32_t a = i >= bpp ? out[i - bpp] : 0u, b = r ? out[i - rowb] : 0u;
                    const uint32_t c = (r && i >= bpp) ? out[i - rowb - bpp] : 0u;
                    out[i] = (uint8_t)inf::unfilter(ft, in[i], a, b, c);
                }
            }
        }
        status[t] = rc;
        free(rows);
        free(stream);
    }
    delete tables;
    free(data);

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(images.data(), 1, images.size(), o);
    fwrite(status.data(), sizeof(int32_t), status.size(), o);
    fclose(o);
    return 0;
}
