// The inflate core (RFC 1950 / 1951) and the PNG filter arithmetic (include/gflow_hip.h, "PNG files": Decoding): the part
// of the decoder that reads untrusted data and indexes its tables by it -- the bit reader, the block headers, the code-length
// decoding, the canonical table construction and the symbol decode, each with its checks -- as plain C++ that hipcc and a host
// compiler both take.
// The kernel of gfl_png_dec.hip and the host harness tools/png_dec_host.cpp (which runs under the address and
// undefined-behaviour sanitizers) call the SAME routines (__host__ __device__ under hipcc), so what the harness shows about
// a malformed stream holds for the device's use of THESE routines.  Where the bytes come from and where they go is the
// caller's `Io`, which the harness does not share with the device: the device's (DeviceIo in gfl_png_dec.hip) relies on the
// bounds stated below and is covered by the GPU tests alone.
//   uint32_t in_byte(int64_t pos)          byte pos of the stream, 0 <= pos < n_in (the core never asks for another)
//   uint32_t in_word(int64_t pos)          bytes pos .. pos + 3, little endian, pos + 4 <= n_in
//   void     put(uint32_t byte)            one literal
//   void     copy(int dist, int len)       a match: 1 <= dist <= bytes put so far, 3 <= len <= 258, may overlap itself
//   void     stored(int64_t pos, int n)    n bytes of the stream, from pos, as they are
//   uint32_t finish()                      the Adler-32 of everything put
// The core bounds the output: an Io is never asked to hold more than `expect` bytes.  All state is the same in every lane of
// a wave: on the device every value read from a table passes GFL_INF_UNIFORM, which tells the compiler so.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GFL_INF_HD __host__ __device__
#else
#define GFL_INF_HD
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define GFL_INF_UNIFORM(x) ((int32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define GFL_INF_UNIFORM(x) ((int32_t)(x))
#endif

// the table builder runs once per block: kept out of line, the symbol loops stay short
#define GFL_INF_NOINLINE __attribute__((noinline))

namespace gfl {
namespace inf {

// status of an image (include/gflow_hip.h: GFL_PNG_*): 0, or the FIRST error in stream order
enum Status : int32_t {
    OK = 0, INPUT_END = 1, BAD_HEADER = 2, BLOCK_TYPE = 3, STORED_LEN = 4, TOO_MANY_CODES = 5, BAD_REPEAT = 6, BAD_CODE = 7,
    NO_END_OF_BLOCK = 8, BAD_SYMBOL = 9, FAR_DISTANCE = 10, OUTPUT_SIZE = 11, BAD_ADLER = 12, BAD_FILTER = 13, NOT_RUN = -1
};

constexpr int FAST_BITS = 10;               // codes up to this length are one table look
constexpr int MAX_BITS = 15;
constexpr int MAX_LITLEN = 288, MAX_DIST = 32, MAX_LENS = 320;

// One canonical prefix code (RFC 1951, 3.2.2).  A code of length l read most significant bit first is one of this table's
// iff 0 <= code - first[l] < count[l]; its symbol is sorted[offset[l] + code - first[l]].  fast[the next FAST_BITS bits of
// the stream] = symbol | length << 9 for the codes that short, 0 otherwise.
struct Code {
    uint16_t count[MAX_BITS + 1], first[MAX_BITS + 1], offset[MAX_BITS + 1], next[MAX_BITS + 1];
    uint16_t sorted[MAX_LITLEN];
    uint16_t fast[1 << FAST_BITS];
};

struct Tables {
    Code lit, dist;
    uint8_t lens[MAX_LENS];
    uint8_t cl[19];
};

struct Pair { uint16_t base; uint8_t extra; };
struct LengthTable { Pair p[29]; };
struct DistTable { Pair p[30]; };
GFL_INF_HD inline Pair length_of(int k) {             // symbol 257 + k
    constexpr LengthTable t = {{{3, 0},  {4, 0},  {5, 0},  {6, 0},  {7, 0},  {8, 0},  {9, 0},  {10, 0},  {11, 1},  {13, 1},
                                {15, 1}, {17, 1}, {19, 2}, {23, 2}, {27, 2}, {31, 2}, {35, 3}, {43, 3},  {51, 3},  {59, 3},
                                {67, 4}, {83, 4}, {99, 4}, {115, 4}, {131, 5}, {163, 5}, {195, 5}, {227, 5}, {258, 0}}};
    return t.p[k];
}
GFL_INF_HD inline Pair distance_of(int k) {
    constexpr DistTable t = {{{1, 0},    {2, 0},    {3, 0},    {4, 0},    {5, 1},    {7, 1},     {9, 2},     {13, 2},
                              {17, 3},   {25, 3},   {33, 4},   {49, 4},   {65, 5},   {97, 5},    {129, 6},   {193, 6},
                              {257, 7},  {385, 7},  {513, 8},  {769, 8},  {1025, 9}, {1537, 9},  {2049, 10}, {3073, 10},
                              {4097, 11}, {6145, 11}, {8193, 12}, {12289, 12}, {16385, 13}, {24577, 13}}};
    return t.p[k];
}
struct OrderTable { uint8_t o[19]; };
GFL_INF_HD inline int code_length_order(int i) {
    constexpr OrderTable t = {{16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}};
    return t.o[i];
}

// ---- the bit reader: least significant bit first, never asks the Io for a byte at or behind `end`
struct Bits {
    uint64_t acc;               // the next n bits of the stream are the low n bits of acc; the bits above are 0
    int32_t n;
    int64_t pos, end;

    GFL_INF_HD inline void open(int64_t n_in) { acc = 0; n = 0; pos = 0; end = n_in; }
    // At least 32 bits afterwards, or all the stream has left: one word where the stream still has one (the usual case: one
    // read per four bytes), single bytes at its end.  No step of the decoder needs more than 28 bits between two fills.
    template <class Io>
    GFL_INF_HD inline void fill(Io& io) {
        if (n > 32) return;
        if (pos + 4 <= end) {
            acc |= (uint64_t)io.in_word(pos) << n;
            pos += 4;
            n += 32;
            return;
        }
        while (n <= 56 && pos < end) {
            acc |= (uint64_t)io.in_byte(pos++) << n;
            n += 8;
        }
    }
    GFL_INF_HD inline uint32_t take(int k) {          // k <= n, k <= 16
        const uint32_t v = (uint32_t)acc & ((1u << k) - 1u);
        acc >>= k;
        n -= k;
        return v;
    }
    GFL_INF_HD inline void to_byte_boundary() { take(n & 7); }
    // give whole buffered bytes back to the stream (before a stored block's bytes are taken from it directly)
    GFL_INF_HD inline void unread() { pos -= n >> 3; acc = 0; n = 0; }
};

GFL_INF_HD inline uint32_t reverse_bits(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
    return r;
}

// The code of n lengths (each 0 .. 15; 0: the symbol is not used).  BAD_CODE for an over-subscribed set and for an incomplete
// one -- but for a set without any code or with a single code of length 1, which zlib lets pass where `strict` is not set
// (the literal / length and the distance code; never the code-length code).
GFL_INF_NOINLINE GFL_INF_HD inline int32_t build(Code& c, const uint8_t* lens, int n, bool strict) {
    for (int l = 0; l <= MAX_BITS; ++l) c.count[l] = 0;
    for (int i = 0; i < n; ++i) {
        const int l = GFL_INF_UNIFORM(lens[i]) & MAX_BITS;
        c.count[l] = (uint16_t)(c.count[l] + 1);
    }
    int left = 1, maxlen = 0;
    for (int l = 1; l <= MAX_BITS; ++l) {
        const int k = GFL_INF_UNIFORM(c.count[l]);
        left = left * 2 - k;
        if (left < 0) return BAD_CODE;
        if (k) maxlen = l;
    }
    if (left > 0 && (strict || maxlen > 1)) return BAD_CODE;
    int code = 0, index = 0;
    c.count[0] = 0;
    c.first[0] = c.offset[0] = c.next[0] = 0;
    for (int l = 1; l <= MAX_BITS; ++l) {
        code = (code + GFL_INF_UNIFORM(c.count[l - 1])) << 1;
        c.first[l] = (uint16_t)code;                        // (not over-subscribed: code <= 2^l)
        c.offset[l] = c.next[l] = (uint16_t)index;
        index += GFL_INF_UNIFORM(c.count[l]);
    }
    for (int i = 0; i < (1 << FAST_BITS); ++i) c.fast[i] = 0;
    for (int i = 0; i < n; ++i) {
        const int l = GFL_INF_UNIFORM(lens[i]) & MAX_BITS;
        if (l == 0) continue;
        const int at = GFL_INF_UNIFORM(c.next[l]);          // < index <= n
        c.next[l] = (uint16_t)(at + 1);
        c.sorted[at] = (uint16_t)i;
        if (l <= FAST_BITS) {
            const uint32_t word = (uint32_t)(GFL_INF_UNIFORM(c.first[l]) + at - GFL_INF_UNIFORM(c.offset[l]));
            for (uint32_t k = reverse_bits(word, l); k < (1u << FAST_BITS); k += 1u << l) c.fast[k] = (uint16_t)(i | (l << 9));
        }
    }
    return OK;
}

// the next symbol of code c, or minus a Status.  The reader has been filled: fewer than 15 bits mean the stream has no more.
GFL_INF_HD inline int32_t decode(const Code& c, Bits& b) {
    int32_t sym = -1, len = 0;
    const int32_t e = GFL_INF_UNIFORM(c.fast[(uint32_t)b.acc & ((1u << FAST_BITS) - 1u)]);
    if (e) {
        sym = e & 511;
        len = e >> 9;
    } else {
        int32_t code = 0;
        for (int l = 1; l <= MAX_BITS; ++l) {
            code = (code << 1) | (int32_t)((b.acc >> (l - 1)) & 1u);
            const int32_t k = code - GFL_INF_UNIFORM(c.first[l]);
            if (k >= 0 && k < GFL_INF_UNIFORM(c.count[l])) {
                sym = GFL_INF_UNIFORM(c.sorted[GFL_INF_UNIFORM(c.offset[l]) + k]);
                len = l;
                break;
            }
        }
    }
    if (sym < 0 || len > b.n) return b.n < MAX_BITS ? -(int32_t)INPUT_END : -(int32_t)BAD_SYMBOL;
    b.take(len);
    return sym;
}

GFL_INF_HD inline void fixed_lengths(Tables& tb) {
    for (int i = 0; i < 288; ++i) tb.lens[i] = (uint8_t)(i < 144 ? 8 : (i < 256 ? 9 : (i < 280 ? 7 : 8)));
    for (int i = 0; i < 32; ++i) tb.lens[288 + i] = 5;
}

// the header of a dynamic block: both codes built, or the first error
template <class Io>
GFL_INF_HD inline int32_t dynamic_header(Io& io, Bits& b, Tables& tb) {
    b.fill(io);
    if (b.n < 14) return INPUT_END;
    const int nlen = (int)b.take(5) + 257, ndist = (int)b.take(5) + 1, ncode = (int)b.take(4) + 4;
    if (nlen > 286 || ndist > 30) return TOO_MANY_CODES;
    for (int i = 0; i < 19; ++i) tb.cl[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        b.fill(io);
        if (b.n < 3) return INPUT_END;
        tb.cl[code_length_order(i)] = (uint8_t)b.take(3);
    }
    if (int32_t rc = build(tb.lit, tb.cl, 19, true)) return rc;
    const int total = nlen + ndist;                        // <= 316
    int i = 0;
    while (i < total) {
        b.fill(io);
        const int32_t sym = decode(tb.lit, b);             // 0 .. 18
        if (sym < 0) return -sym;
        if (sym < 16) {
            tb.lens[i++] = (uint8_t)sym;
            continue;
        }
        int prev = 0, rep, extra;
        if (sym == 16) {
            if (i == 0) return BAD_REPEAT;
            prev = GFL_INF_UNIFORM(tb.lens[i - 1]);
            rep = 3; extra = 2;
        } else if (sym == 17) {
            rep = 3; extra = 3;
        } else {
            rep = 11; extra = 7;
        }
        if (b.n < extra) return INPUT_END;
        rep += (int)b.take(extra);
        if (i + rep > total) return BAD_REPEAT;
        for (int k = 0; k < rep; ++k) tb.lens[i++] = (uint8_t)prev;
    }
    if (GFL_INF_UNIFORM(tb.lens[256]) == 0) return NO_END_OF_BLOCK;
    if (int32_t rc = build(tb.lit, tb.lens, nlen, false)) return rc;
    return build(tb.dist, tb.lens + nlen, ndist, false);
}

// the symbols of a block up to its end-of-block code
template <class Io>
GFL_INF_HD inline int32_t block_symbols(Io& io, Bits& b, const Tables& tb, int64_t& out, int64_t expect) {
    for (;;) {
        b.fill(io);                                        // 32 bits cover a literal or a length (15 + 5)
        const int32_t sym = decode(tb.lit, b);
        if (sym < 0) return -sym;
        if (sym < 256) {
            if (out >= expect) return OUTPUT_SIZE;
            io.put((uint32_t)sym);
            ++out;
            continue;
        }
        if (sym == 256) return OK;
        if (sym > 285) return BAD_SYMBOL;
        const Pair lp = length_of(sym - 257);
        if (b.n < lp.extra) return INPUT_END;
        const int len = lp.base + (int)b.take(lp.extra);
        b.fill(io);                                        // ... and a distance (15 + 13)
        const int32_t dsym = decode(tb.dist, b);
        if (dsym < 0) return -dsym;
        if (dsym > 29) return BAD_SYMBOL;
        const Pair dp = distance_of(dsym);
        if (b.n < dp.extra) return INPUT_END;
        const int dist = dp.base + (int)b.take(dp.extra);
        if (dist > out) return FAR_DISTANCE;
        if (len > expect - out) return OUTPUT_SIZE;
        io.copy(dist, len);
        out += len;
    }
}

// One zlib stream of n_in bytes that must give exactly `expect` bytes: 0, or the first error in stream order.
template <class Io>
GFL_INF_HD inline int32_t inflate(Io& io, int64_t n_in, int64_t expect, Tables& tb) {
    if (n_in < 2) return INPUT_END;
    const uint32_t cmf = io.in_byte(0), flg = io.in_byte(1);
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return BAD_HEADER;
    Bits b;
    b.open(n_in);
    b.pos = 2;
    int64_t out = 0;
    for (;;) {
        b.fill(io);
        if (b.n < 3) return INPUT_END;
        const uint32_t last = b.take(1), type = b.take(2);
        if (type == 3) return BLOCK_TYPE;
        if (type == 0) {
            b.to_byte_boundary();
            b.unread();
            if (b.pos + 4 > b.end) return INPUT_END;
            const uint32_t len = io.in_byte(b.pos) | (io.in_byte(b.pos + 1) << 8);
            const uint32_t nlen = io.in_byte(b.pos + 2) | (io.in_byte(b.pos + 3) << 8);
            if ((len ^ 0xffffu) != nlen) return STORED_LEN;
            b.pos += 4;
            if ((int64_t)len > b.end - b.pos) return INPUT_END;
            if ((int64_t)len > expect - out) return OUTPUT_SIZE;
            if (len) io.stored(b.pos, (int)len);
            b.pos += len;
            out += len;
        } else {
            if (type == 1) {
                fixed_lengths(tb);
                if (int32_t rc = build(tb.lit, tb.lens, 288, false)) return rc;
                if (int32_t rc = build(tb.dist, tb.lens + 288, 32, false)) return rc;
            } else if (int32_t rc = dynamic_header(io, b, tb)) {
                return rc;
            }
            if (int32_t rc = block_symbols(io, b, tb, out, expect)) return rc;
        }
        if (last) break;
    }
    if (out != expect) return OUTPUT_SIZE;
    b.to_byte_boundary();
    b.fill(io);
    if (b.n < 32) return INPUT_END;
    uint32_t want = 0;
    for (int i = 0; i < 4; ++i) want = (want << 8) | b.take(8);
    return io.finish() == want ? OK : BAD_ADLER;
}

// ---- Adler-32 by pieces: (s1, s2) moved over L bytes whose plain sum is a and whose weighted sum, sum of (L - i) * byte i,
// is w.  a <= 255 L and w <= 255 L (L + 1) / 2: for L <= 1024 no 32-bit overflow.
constexpr uint32_t ADLER_MOD = 65521u;
GFL_INF_HD inline void adler_add(uint32_t& s1, uint32_t& s2, uint32_t L, uint32_t a, uint32_t w) {
    s2 = (s2 + (L * s1) % ADLER_MOD + w % ADLER_MOD) % ADLER_MOD;
    s1 = (s1 + a) % ADLER_MOD;
}

// ---- the PNG filters (PNG specification, 9.2): the byte from its filtered value x, with a = the byte bpp to the left,
// b = the byte above, c = the byte above a; all 0 outside the image.  ft is 0 .. 4.
GFL_INF_HD inline uint32_t paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}
GFL_INF_HD inline uint32_t unfilter(int ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    const uint32_t add = ft == 0 ? 0u : (ft == 1 ? a : (ft == 2 ? b : (ft == 3 ? (a + b) >> 1 : paeth((int)a, (int)b, (int)c))));
    return (x + add) & 255u;
}

// the shape of a call: what gfl_png_decode and gfl_png_decode_workspace_bytes accept
constexpr int64_t MAX_FILTERED = (int64_t)1 << 31;         // filtered bytes of one image (positions stay below 2^31)
GFL_INF_HD inline bool shape_ok(int T, int bpp, int W, int H) {
    if (T < 1 || W < 1 || H < 1 || bpp < 1 || bpp > 4) return false;
    const int64_t row = 1 + (int64_t)W * bpp;
    return row * H < MAX_FILTERED && (int64_t)T * ((row * H + 255) / 256 * 256) < ((int64_t)1 << 40);
}
GFL_INF_HD inline int64_t filtered_bytes(int bpp, int W, int H) { return (int64_t)H * (1 + (int64_t)W * bpp); }

}  // namespace inf
}  // namespace gfl
