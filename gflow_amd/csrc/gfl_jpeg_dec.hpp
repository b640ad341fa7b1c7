// The baseline JPEG decode core (include/gflow_hip.h, "video files": Decoding): the per-unit entropy decoder and the block
// arithmetic, as plain C++ that hipcc and a host compiler both take.  The kernels of gfl_jpeg_dec.hip and the host harness
// tools/jpeg_dec_host.cpp (which runs under the address and undefined-behaviour sanitizers) call the SAME routines, so what
// the harness shows about a malformed file holds for the device.  Integers only: int32 throughout, >> arithmetic.
#pragma once
#include <stdint.h>

#include "../../include/gflow_hip.h"

#if defined(__HIPCC__)
#define GFL_JD_HD __host__ __device__
#else
#define GFL_JD_HD
#endif

namespace gfl {
namespace jd {

enum Status : int32_t {
    UNIT_OK = 0, UNIT_BAD_RECORD = 1, UNIT_NO_CODE = 2, UNIT_INDEX = 3, UNIT_SHORT = 4, UNIT_LEFT_OVER = 5, UNIT_SYMBOL = 6,
    UNIT_NOT_RUN = -1
};

constexpr int MAX_SIDE = 65535;
constexpr long long MAX_BLOCKS = 1ll << 30;

// natural index (row * 8 + column) of the k-th coefficient in zigzag order (T.81 figure A.6)
struct Zigzag { uint8_t n[64]; };
GFL_JD_HD inline int zigzag_natural(int k) {
    constexpr Zigzag z = {{0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}};
    return z.n[k & 63];
}

// ---- the shape of a call: everything the three stages index with
struct Shape {
    int T, C, W, H, hs, vs;
    int mx, my;                 // MCUs per row / column
    int bw[3], bh[3];           // blocks per row / column of component c's coefficient plane (whole MCUs)
    int cw[3], ch[3];           // the component's real size in samples: ceil(W h / hmax), ceil(H v / vmax)
    int base[3];                // the component's first block inside a frame
    int nblk;                   // blocks per frame
    long long plane[3];         // the component's first sample inside a frame's planes (a plane is bh * 8 rows of bw * 8)
    long long plane_bytes;      // samples per frame
};

GFL_JD_HD inline bool make_shape(int T, int C, int W, int H, int hs, int vs, Shape& s) {
    if (T < 1 || W < 1 || H < 1 || W > MAX_SIDE || H > MAX_SIDE) return false;
    if (C == 1) {
        if (hs != 1 || vs != 1) return false;
    } else if (C == 3) {
        if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2))) return false;
    } else {
        return false;
    }
    s.T = T; s.C = C; s.W = W; s.H = H; s.hs = hs; s.vs = vs;
    s.mx = (W + 8 * hs - 1) / (8 * hs);
    s.my = (H + 8 * vs - 1) / (8 * vs);
    s.nblk = 0;
    s.plane_bytes = 0;
    for (int c = 0; c < 3; ++c) {
        const int h = c == 0 ? hs : 1, v = c == 0 ? vs : 1;
        const bool used = c < C;
        s.bw[c] = used ? s.mx * h : 0;
        s.bh[c] = used ? s.my * v : 0;
        s.cw[c] = used ? (W * h + hs - 1) / hs : 0;
        s.ch[c] = used ? (H * v + vs - 1) / vs : 0;
        s.base[c] = s.nblk;
        s.plane[c] = s.plane_bytes;
        s.nblk += s.bw[c] * s.bh[c];
        s.plane_bytes += (long long)s.bw[c] * s.bh[c] * 64;
    }
    return (long long)T * s.nblk <= MAX_BLOCKS;
}

// ---- Huffman tables in the form of T.81 F.2.2.3: a code of length l is one of this table's iff code <= maxcode[l], and
// its value is vals[valoff[l] + code].  A length without codes has maxcode -1.
struct Huff {
    int32_t maxcode[17];        // [1 .. 16]
    int32_t valoff[17];         // valptr - mincode
    uint8_t vals[256];
};

// Whatever the BITS list holds, the table it gives is safe to decode with: value indices are checked when they are used.
GFL_JD_HD inline void build_huff(const gfl_jpeg_huff_spec& spec, Huff& h) {
    int32_t code = 0, k = 0;
    h.maxcode[0] = -1;
    h.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int32_t n = spec.bits[l - 1];
        h.valoff[l] = k - code;
        h.maxcode[l] = n ? code + n - 1 : -1;
        code = (code + n) << 1;             // (at most (255 * 16) << 16: no overflow)
        k += n;
    }
    for (int i = 0; i < 256; ++i) h.vals[i] = spec.vals[i];
}

// ---- the bit reader of ONE unit: never looks at a byte outside [p, p + len).  Behind the end -- and behind a marker, which
// cannot stand inside a unit of a well-formed file -- it supplies 1-bits and counts them, so the caller can tell when it has
// consumed bits that were never there.
struct BitReader {
    const uint8_t* p;
    int32_t len, pos;
    uint32_t acc;               // the next `n` bits of the stream are the low n bits of acc
    int32_t n;
    int32_t made_up;            // of those n bits, the last made_up were supplied, not read

    GFL_JD_HD inline void open(const uint8_t* data, int32_t length) {
        p = data; len = length; pos = 0; acc = 0; n = 0; made_up = 0;
    }
    // (fetching eight bytes per load instead of one was tried and measured: no gain -- the lane's time goes into the
    // symbol-by-symbol walk, not into the loads)
    GFL_JD_HD inline void fill() {                    // up to 32 bits in acc
        while (n <= 24) {
            uint32_t b = 0xffu;
            if (pos < len) {
                b = p[pos++];
                if (b == 0xffu) {
                    if (pos < len && p[pos] == 0) ++pos;          // FF 00: a stuffed FF
                    else pos = len;                               // a marker or a lone FF: the data ends here
                }
            } else {
                made_up += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    GFL_JD_HD inline uint32_t peek16() {
        fill();
        return (acc >> (n - 16)) & 0xffffu;
    }
    GFL_JD_HD inline void skip(int k) { n -= k; }
    GFL_JD_HD inline uint32_t get(int k) {            // k in 0 .. 16
        if (k == 0) return 0u;
        fill();
        n -= k;
        return (acc >> n) & ((1u << k) - 1u);
    }
    GFL_JD_HD inline bool short_of_data() const { return n < made_up; }       // a consumed bit was made up
    // after the last MCU: every byte read, fewer than 8 bits left, all of them the 1-bits of the padding
    GFL_JD_HD inline bool ends_clean() const {
        const int real = n - made_up;
        if (pos < len || real < 0 || real >= 8) return false;
        const uint32_t rest = real ? (acc >> made_up) & ((1u << real) - 1u) : 0u;
        return rest == (real ? (1u << real) - 1u : 0u);
    }
};

// one Huffman symbol; -1: no code of 1 .. 16 bits matches; -2: the table points outside its values
GFL_JD_HD inline int decode_symbol(BitReader& br, const Huff& h) {
    const uint32_t look = br.peek16();
    for (int l = 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(look >> (16 - l));
        if (code <= h.maxcode[l]) {
            br.skip(l);
            const int32_t i = h.valoff[l] + code;
            if (i < 0 || i > 255) return -2;
            return h.vals[i];
        }
    }
    return -1;
}

// T.81 F.2.2.1: the value of `s` extra bits
GFL_JD_HD inline int32_t extend(uint32_t v, int s) {
    return s == 0 ? 0 : ((int32_t)v < (1 << (s - 1)) ? (int32_t)v - (1 << s) + 1 : (int32_t)v);
}

// One block into blk[64] (natural order, zeroed here), the DC predictor updated.  UNIT_OK or the reason it stopped.
GFL_JD_HD inline int32_t decode_block(BitReader& br, const Huff& dc, const Huff& ac, int32_t& pred, int16_t* blk) {
    for (int i = 0; i < 64; ++i) blk[i] = 0;
    int s = decode_symbol(br, dc);
    if (s < 0) return s == -1 ? UNIT_NO_CODE : UNIT_SYMBOL;
    if (s > 15) return UNIT_SYMBOL;
    pred = (int32_t)((uint32_t)pred + (uint32_t)extend(br.get(s), s));
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64; ++k) {
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return rs == -1 ? UNIT_NO_CODE : UNIT_SYMBOL;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;                       // EOB
            k += 15;                                  // ZRL (the loop adds the sixteenth)
            if (k > 63) return UNIT_INDEX;
            continue;
        }
        k += r;
        if (k > 63) return UNIT_INDEX;
        blk[zigzag_natural(k)] = (int16_t)extend(br.get(s), s);
    }
    return br.short_of_data() ? UNIT_SHORT : UNIT_OK;
}

// Is the unit record one this call can run?  (frame t's units are listed by tables[t])
GFL_JD_HD inline bool unit_in_range(const gfl_jpeg_unit& u, int t, const Shape& s, long long n_bytes) {
    const long long mcus = (long long)s.mx * s.my;
    return u.frame == t && u.first_mcu >= 0 && u.n_mcu >= 1 && (long long)u.first_mcu + u.n_mcu <= mcus && u.n_bytes >= 0 &&
           u.offset >= 0 && u.offset <= n_bytes && (long long)u.n_bytes <= n_bytes - u.offset;
}

// One unit of frame t: its MCUs' blocks into the frame's coefficients (coef: the frame's nblk * 64 int16).  A block is
// stored only once it is decoded whole; nothing outside the unit's MCUs is written.  huff: [0], [1] DC, [2], [3] AC.
GFL_JD_HD inline int32_t decode_unit(const uint8_t* bytes, long long n_bytes, const gfl_jpeg_unit& u, int t,
                                     const gfl_jpeg_frame_tables& ft, const Huff* huff, const Shape& s, int16_t* coef) {
    if (!unit_in_range(u, t, s, n_bytes)) return UNIT_BAD_RECORD;
    BitReader br;
    br.open(bytes + u.offset, u.n_bytes);
    int32_t pred[3] = {0, 0, 0};
    int16_t blk[64];
    for (int m = u.first_mcu; m < u.first_mcu + u.n_mcu; ++m) {
        const int my = m / s.mx, mx = m - my * s.mx;
        for (int c = 0; c < s.C; ++c) {
            const int h = c == 0 ? s.hs : 1, v = c == 0 ? s.vs : 1;
            const Huff& dc = huff[ft.dcsel[c] & 1];
            const Huff& ac = huff[2 + (ft.acsel[c] & 1)];
            for (int j = 0; j < v; ++j) {
                for (int i = 0; i < h; ++i) {
                    const int32_t st = decode_block(br, dc, ac, pred[c], blk);
                    if (st != UNIT_OK) return st;
                    const long long b = s.base[c] + (long long)(my * v + j) * s.bw[c] + (mx * h + i);
                    int16_t* dst = coef + b * 64;
                    for (int q = 0; q < 64; ++q) dst[q] = blk[q];
                }
            }
        }
    }
    return br.ends_clean() ? UNIT_OK : UNIT_LEFT_OVER;
}

// ---- the inverse DCT: one pass of the 13-bit-constant LL&M butterfly over eight values
// (int32 products and sums as libjpeg forms them; the unsigned detour only keeps a malformed file's overflow defined;
// descale_w(x, n) is DESCALE(x, n) = (x + (1 << (n - 1))) >> n)
GFL_JD_HD inline int32_t mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
GFL_JD_HD inline int32_t add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
GFL_JD_HD inline int32_t sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
GFL_JD_HD inline int32_t shl13(int32_t a) { return (int32_t)((uint32_t)a << 13); }
GFL_JD_HD inline int32_t descale_w(int32_t x, int n) { return add(x, 1 << (n - 1)) >> n; }

GFL_JD_HD inline void idct_pass(const int32_t* in, int32_t* out, int shift) {
    // even part
    int32_t z1 = mul(add(in[2], in[6]), 4433);
    const int32_t t2 = add(z1, mul(in[6], -15137));
    const int32_t t3 = add(z1, mul(in[2], 6270));
    const int32_t t0 = shl13(add(in[0], in[4]));
    const int32_t t1 = shl13(sub(in[0], in[4]));
    const int32_t t10 = add(t0, t3), t13 = sub(t0, t3), t11 = add(t1, t2), t12 = sub(t1, t2);
    // odd part
    int32_t a = in[7], b = in[5], c = in[3], d = in[1];
    const int32_t z5 = mul(add(add(a, c), add(b, d)), 9633);
    z1 = mul(add(a, d), -7373);
    const int32_t z2 = mul(add(b, c), -20995);
    const int32_t z3 = add(mul(add(a, c), -16069), z5);
    const int32_t z4 = add(mul(add(b, d), -3196), z5);
    a = add(add(mul(a, 2446), z1), z3);
    b = add(add(mul(b, 16819), z2), z4);
    c = add(add(mul(c, 25172), z2), z3);
    d = add(add(mul(d, 12299), z1), z4);
    out[0] = descale_w(add(t10, d), shift); out[7] = descale_w(sub(t10, d), shift);
    out[1] = descale_w(add(t11, c), shift); out[6] = descale_w(sub(t11, c), shift);
    out[2] = descale_w(add(t12, b), shift); out[5] = descale_w(sub(t12, b), shift);
    out[3] = descale_w(add(t13, a), shift); out[4] = descale_w(sub(t13, a), shift);
}
constexpr int IDCT_SHIFT_COLUMNS = 11, IDCT_SHIFT_ROWS = 18;

GFL_JD_HD inline int32_t clamp255(int32_t v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// column j of a block: dequantise (natural order), pass 1 -> ws[k * 8 + j]
GFL_JD_HD inline void idct_column(const int16_t* coef, const uint8_t* q, int j, int32_t* ws) {
    int32_t in[8], out[8];
    for (int k = 0; k < 8; ++k) in[k] = (int32_t)coef[k * 8 + j] * (int32_t)q[k * 8 + j];
    idct_pass(in, out, IDCT_SHIFT_COLUMNS);
    for (int k = 0; k < 8; ++k) ws[k * 8 + j] = out[k];
}
// row r of a block: pass 2, + 128, clamp -> eight samples
GFL_JD_HD inline void idct_row(const int32_t* ws, int r, uint8_t* out8) {
    int32_t out[8];
    idct_pass(ws + r * 8, out, IDCT_SHIFT_ROWS);
    for (int k = 0; k < 8; ++k) out8[k] = (uint8_t)clamp255(add(out[k], 128));
}

// where block b of a frame lies: its component, and its first sample in the frame's planes
struct BlockAt { int c; long long sample; int stride; };
GFL_JD_HD inline BlockAt block_at(const Shape& s, int b) {
    int c = 0;
    if (s.C == 3 && b >= s.base[1]) c = b >= s.base[2] ? 2 : 1;
    const int i = b - s.base[c], by = i / s.bw[c], bx = i - by * s.bw[c];
    BlockAt at;
    at.c = c;
    at.stride = s.bw[c] * 8;
    at.sample = s.plane[c] + (long long)by * 8 * at.stride + bx * 8;
    return at;
}

// ---- upsampling: the sample of a chroma plane (cropped to cw x ch; rows outside repeat the nearest) at pixel (x, y)
GFL_JD_HD inline int32_t chroma_at(const uint8_t* p, int stride, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(long long)y * stride + x];
    const int j = x >> 1;
    if (vs == 1) {                                                        // 2 x 1
        const int32_t v = p[(long long)y * stride + j];
        if (x & 1) return j + 1 < cw ? (3 * v + p[(long long)y * stride + j + 1] + 2) >> 2 : v;
        return j > 0 ? (3 * v + p[(long long)y * stride + j - 1] + 1) >> 2 : v;
    }
    const int r = y >> 1;                                                 // 2 x 2
    int rn = (y & 1) ? r + 1 : r - 1;
    rn = rn < 0 ? 0 : (rn > ch - 1 ? ch - 1 : rn);
    const uint8_t* near = p + (long long)r * stride;
    const uint8_t* far = p + (long long)rn * stride;
    const int32_t sj = 3 * near[j] + far[j];
    if (x & 1) return j + 1 < cw ? (3 * sj + (3 * near[j + 1] + far[j + 1]) + 7) >> 4 : (4 * sj + 7) >> 4;
    return j > 0 ? (3 * sj + (3 * near[j - 1] + far[j - 1]) + 8) >> 4 : (4 * sj + 8) >> 4;
}

// ---- colour: 16-bit fixed-point YCbCr -> RGB
GFL_JD_HD inline void ycc_rgb(int32_t y, int32_t cb, int32_t cr, uint8_t* rgb) {
    cb -= 128;
    cr -= 128;
    rgb[0] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = (uint8_t)clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
}

// pixel (x, y) of a frame from its planes -> C bytes
GFL_JD_HD inline void pixel_at(const uint8_t* planes, const Shape& s, int x, int y, uint8_t* out) {
    const int32_t lum = planes[s.plane[0] + (long long)y * (s.bw[0] * 8) + x];
    if (s.C == 1) {
        out[0] = (uint8_t)lum;
        return;
    }
    const int32_t cb = chroma_at(planes + s.plane[1], s.bw[1] * 8, s.cw[1], s.ch[1], s.hs, s.vs, x, y);
    const int32_t cr = chroma_at(planes + s.plane[2], s.bw[2] * 8, s.cw[2], s.ch[2], s.hs, s.vs, x, y);
    ycc_rgb(lum, cb, cr, out);
}

}  // namespace jd
}  // namespace gfl
