// Baseline JPEG on the device (include/gflow_hip.h, "video files"): T frames of (H, W, C) uint8 -> the entropy-coded scan of
// T baseline sequential JPEG images (ITU-T T.81, 8 bits, YCbCr 4:4:4 or one grey component, Annex K's Huffman tables).
// The scan is cut into restart intervals of JPEG_RI MCUs in scan order: an interval is a byte-aligned bit stream of its own
// whose DC prediction starts from 0, so ONE workgroup codes one (frame, interval) from the pixels to the stuffed bytes:
//   pixels -> colour transform + row DCT in registers -> column DCT + quantisation -> zigzag coefficients in LDS
//   -> a thread per 8x8 block counts its bits -> prefix sum -> the thread ORs its codes into an LDS bit buffer at its offset
//   -> 1-bits to the byte boundary -> a byte pass counts the FF bytes per 64-byte segment, scans, and writes FF as FF 00.
// Two passes over the same routine (jpeg_interval): gfl_jpeg_sizes keeps only every interval's stuffed length and scans them
// into offsets, gfl_jpeg_emit codes again and writes at the offset.  Integer LDS atomics only: the bytes do not depend on the
// order in which blocks arrive.  No allocation, no host synchronisation.
#include "gfl_common.hpp"

namespace gfl {

constexpr int JPEG_RI = GFL_JPEG_RI;               // MCUs per restart interval
constexpr int JPEG_BLOCK = 256;
constexpr int JPEG_MAX_SIDE = 65535;               // SOF0 holds 16-bit sizes
constexpr long long JPEG_MAX_INTERVALS = 1ll << 30;
static_assert(JPEG_RI >= 1 && JPEG_RI * 8 <= JPEG_BLOCK, "a lane per (MCU, pixel row) of an interval");

// ---- Annex K: the four Huffman tables as BITS / HUFFVAL, turned into (code << 8 | length) per symbol at compile time
struct HuffSpec { uint8_t bits[16]; uint8_t vals[162]; };
struct HuffTable { uint32_t e[256]; };

constexpr HuffTable make_huff(const HuffSpec& s) {
    HuffTable t{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i) t.e[s.vals[k++]] = (code++ << 8) | (unsigned)len;
        code <<= 1;
    }
    return t;
}

constexpr HuffSpec DC_LUM = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec DC_CHR = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec AC_LUM = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
constexpr HuffSpec AC_CHR = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// [0], [1]: DC luminance, chrominance (symbols 0 .. 11); [2], [3]: AC
__constant__ HuffTable JPEG_HUFF[4] = {make_huff(DC_LUM), make_huff(DC_CHR), make_huff(AC_LUM), make_huff(AC_CHR)};

// zigzag position of the natural index v * 8 + u
__constant__ uint8_t JPEG_ZZ[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// the 1-D DCT-II of T.81 A.3.3: G[u] = C(u) / 2 sum_x f[x] cos((2 x + 1) u pi / 16); the row u of weights, w = cos(k pi / 16)
template <int U>
__device__ __forceinline__ float dct8(const float (&f)[8]) {
    constexpr float w[9] = {1.0f, 0.98078528040323043f, 0.92387953251128674f, 0.83146961230254524f, 0.70710678118654757f,
                            0.55557023301960229f, 0.38268343236508984f, 0.19509032201612833f, 0.0f};
    float s = 0.f;
#pragma unroll
    for (int x = 0; x < 8; ++x) {
        const int k = ((2 * x + 1) * U) & 31;                     // cos(k pi / 16), folded into the first quadrant
        const int m = k > 16 ? 32 - k : k;
        const float c = m > 8 ? -w[16 - m] : w[m];
        s += (U == 0 ? 0.35355339059327379f : 0.5f * c) * f[x];
    }
    return s;
}
__device__ __forceinline__ void dct8_all(const float (&f)[8], float (&g)[8]) {
    g[0] = dct8<0>(f); g[1] = dct8<1>(f); g[2] = dct8<2>(f); g[3] = dct8<3>(f);
    g[4] = dct8<4>(f); g[5] = dct8<5>(f); g[6] = dct8<6>(f); g[7] = dct8<7>(f);
}

// ---- block -> symbols: the ONE routine both passes code a block with.  A sink takes (bits, count), count <= 26
struct BitCount {
    int bits = 0;
    __device__ __forceinline__ void put(uint32_t, int n) { bits += n; }
};
struct BitWriter {                                   // ORs into words that hold the stream MSB first, from bit `pos`
    uint32_t* buf;
    int w, n;
    unsigned long long acc = 0;
    __device__ BitWriter(uint32_t* b, int pos) : buf(b), w(pos >> 5), n(pos & 31) {}
    __device__ __forceinline__ void put(uint32_t v, int len) {
        acc = (acc << len) | v;
        n += len;
        if (n >= 32) {
            n -= 32;
            atomicOr(&buf[w++], (uint32_t)(acc >> n));
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n > 0) atomicOr(&buf[w], (uint32_t)(acc << (32 - n)));
    }
};

__device__ __forceinline__ int jpeg_category(int v) {
    const int a = v < 0 ? -v : v;
    return a ? 32 - __clz(a) : 0;
}
// the code of `sym` followed by the low `cat` bits of v (v - 1 for a negative v): T.81 F.1.2.1, F.1.2.2
template <class Sink>
__device__ __forceinline__ void jpeg_put(Sink& s, uint32_t entry, int v, int cat) {
    const uint32_t extra = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1u);
    s.put(((entry >> 8) << cat) | extra, (int)(entry & 0xffu) + cat);
}
// zz: the block's 64 quantised coefficients in zigzag order (|AC| <= 1023); dc_diff in [-2047, 2047]
template <class Sink>
__device__ void jpeg_block_symbols(const int16_t* zz, int dc_diff, const uint32_t* dc_tab, const uint32_t* ac_tab, Sink& s) {
    const int dcat = jpeg_category(dc_diff);
    jpeg_put(s, dc_tab[dcat], dc_diff, dcat);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) jpeg_put(s, ac_tab[0xF0], 0, 0);         // ZRL
        const int cat = jpeg_category(v);
        jpeg_put(s, ac_tab[(run << 4) | cat], v, cat);
        run = 0;
    }
    if (run) jpeg_put(s, ac_tab[0x00], 0, 0);                                // EOB
}

// ---- the LDS of a workgroup, by component count
template <int C>
struct JpegLds {
    static constexpr int NB = JPEG_RI * C;           // 8x8 blocks of a full interval, in scan order: MCU major, component minor
    static constexpr int PX_STRIDE = 72;             // floats per block: 64 and 8 of padding, so eight blocks' rows miss each other's banks
    // a block is at most 20 bits of DC and 63 x 26 bits of AC = 1658 bits < 208 bytes
    static constexpr int BIT_WORDS = NB * 208 / 4 + 1;
    static constexpr int SEGS = (BIT_WORDS * 4 + 63) / 64;                    // 64-byte segments of the bit buffer
    static constexpr int SEG_SLOTS = 2 * JPEG_BLOCK;
    static_assert(SEGS <= SEG_SLOTS, "two segments per lane in the scan");
    static_assert(BIT_WORDS <= NB * PX_STRIDE, "the bit buffer lies over the samples");
    union {
        float px[NB * PX_STRIDE];                    // row-transformed samples [block][u][y], until the column pass has read them
        uint32_t bits[NB * PX_STRIDE];               // then the interval's bit stream
    };
    int16_t coef[NB * 66];                           // zigzag coefficients, 66 per block (33 words: a lane per block, no conflicts)
    float q[2][64];
    uint32_t huff[4][256];
    int seg[SEG_SLOTS];                              // FF bytes per segment, then their exclusive prefix
    int tot[JPEG_BLOCK / WAVE];
    uint8_t zz[64];
};

struct JpegShape { int T, C, W, H, mx, my, ni; };    // mx, my: MCUs per row / column; ni: intervals per frame
struct JpegCoded { int nbytes, nff; };               // the interval before stuffing, and the FF bytes in it

// code interval `iv` of frame `t` into L.bits (unstuffed, padded with 1-bits) and L.seg (the stuffing prefix)
template <int C>
__device__ JpegCoded jpeg_interval(JpegLds<C>& L, const uint8_t* __restrict__ images, const uint16_t* __restrict__ qtables,
                                   const JpegShape& s, int t, int iv) {
    constexpr int PS = JpegLds<C>::PX_STRIDE;
    const int tid = threadIdx.x;
    const int mcu0 = iv * JPEG_RI;
    const int nmcu = min(JPEG_RI, s.mx * s.my - mcu0);
    const int nb = nmcu * C;
    // tables
    for (int i = tid; i < 128; i += JPEG_BLOCK) (&L.q[0][0])[i] = fmaxf((float)qtables[i], 1.f);
    for (int i = tid; i < 4 * 256; i += JPEG_BLOCK) (&L.huff[0][0])[i] = JPEG_HUFF[i >> 8].e[i & 255];
    if (tid < 64) L.zz[tid] = JPEG_ZZ[tid];
    // a lane per (MCU, pixel row): colour transform, level shift and the row DCT in registers; overhanging blocks repeat
    // the last column / row
    if (tid < nmcu * 8) {
        const int m = tid >> 3, row = tid & 7;
        const int g = mcu0 + m, bx = g % s.mx, by = g / s.mx;
        const int y = min(by * 8 + row, s.H - 1);
        const uint8_t* line = images + ((size_t)t * s.H + y) * (size_t)s.W * C;
        float f[C][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint8_t* p = line + (size_t)min(bx * 8 + i, s.W - 1) * C;
            if constexpr (C == 3) {
                const float r = p[0], gr = p[1], b = p[2];
                f[0][i] = 0.299f * r + 0.587f * gr + 0.114f * b - 128.f;
                f[1][i] = -0.168736f * r - 0.331264f * gr + 0.5f * b;
                f[2][i] = 0.5f * r - 0.418688f * gr - 0.081312f * b;
            } else {
                f[0][i] = (float)p[0] - 128.f;
            }
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float gq[8];
            dct8_all(f[c], gq);
#pragma unroll
            for (int u = 0; u < 8; ++u) L.px[(m * C + c) * PS + u * 8 + row] = gq[u];
        }
    }
    __syncthreads();
    // a lane per (block, u): the column DCT, quantisation (round half away from zero), zigzag
    for (int j = tid; j < nb * 8; j += JPEG_BLOCK) {
        const int blk = j >> 3, u = j & 7;
        float gq[8], F[8];
#pragma unroll
        for (int y = 0; y < 8; ++y) gq[y] = L.px[blk * PS + u * 8 + y];
        dct8_all(gq, F);
        const float* q = L.q[(C == 3 && blk % C != 0) ? 1 : 0];
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const float lim_lo = (u | v) ? -1023.f : -1024.f;              // what 8-bit samples can reach; a safety net only
            L.coef[blk * 66 + L.zz[v * 8 + u]] = (int16_t)fminf(fmaxf(roundf(F[v] / q[v * 8 + u]), lim_lo), 1023.f);
        }
    }
    __syncthreads();
    // the samples are spent: their LDS becomes the bit buffer
    for (int i = tid; i < JpegLds<C>::BIT_WORDS; i += JPEG_BLOCK) L.bits[i] = 0u;
    // a lane per block, in scan order
    int dc_diff = 0;
    const int16_t* zz = L.coef + (tid < nb ? tid : 0) * 66;
    const int comp = tid % C;
    const uint32_t* dc_tab = L.huff[comp ? 1 : 0];
    const uint32_t* ac_tab = L.huff[comp ? 3 : 2];
    BitCount cnt;
    if (tid < nb) {
        dc_diff = (int)zz[0] - (tid >= C ? (int)L.coef[(tid - C) * 66] : 0);
        dc_diff = max(-2047, min(2047, dc_diff));
        jpeg_block_symbols(zz, dc_diff, dc_tab, ac_tab, cnt);
    }
    int total_bits;
    const int at = block_scan_excl<JPEG_BLOCK>(cnt.bits, L.tot, total_bits);            // (its barriers also cover the zeroing)
    if (tid < nb) {
        BitWriter wr(L.bits, at);
        jpeg_block_symbols(zz, dc_diff, dc_tab, ac_tab, wr);
        wr.flush();
    }
    const int pad = (8 - (total_bits & 7)) & 7;
    if (tid == 0 && pad) {
        BitWriter wr(L.bits, total_bits);
        wr.put((1u << pad) - 1u, pad);
        wr.flush();
    }
    __syncthreads();
    // FF bytes per 64-byte segment (a wave per segment), and their exclusive prefix
    JpegCoded out;
    out.nbytes = (total_bits + 7) >> 3;
    const int nseg = (out.nbytes + 63) >> 6;
    const int lane = tid & (WAVE - 1);
    for (int sg = tid / WAVE; sg < nseg; sg += JPEG_BLOCK / WAVE) {
        const int k = sg * 64 + lane;
        const uint32_t b = k < out.nbytes ? (L.bits[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu : 0u;
        const unsigned long long m = __ballot(b == 0xffu);
        if (lane == 0) L.seg[sg] = __popcll(m);
    }
    __syncthreads();
    const int a = 2 * tid < nseg ? L.seg[2 * tid] : 0, b2 = 2 * tid + 1 < nseg ? L.seg[2 * tid + 1] : 0;
    const int ex = block_scan_excl<JPEG_BLOCK>(a + b2, L.tot, out.nff);
    L.seg[2 * tid] = ex;
    L.seg[2 * tid + 1] = ex + a;
    __syncthreads();
    return out;
}

// EMIT = false: sizes[t ni + iv] = the interval's stuffed bytes and its RSTm.  EMIT = true: the bytes at offsets[t ni + iv]
template <int C, bool EMIT>
__global__ void __launch_bounds__(JPEG_BLOCK)
    jpeg_kernel(const uint8_t* __restrict__ images, const uint16_t* __restrict__ qtables, JpegShape s, int32_t* __restrict__ sizes,
                const long long* __restrict__ offsets, uint8_t* __restrict__ out, long long out_bytes) {
    __shared__ JpegLds<C> L;
    const int t = blockIdx.x / s.ni, iv = blockIdx.x - t * s.ni;
    const JpegCoded c = jpeg_interval<C>(L, images, qtables, s, t, iv);
    const int marker = iv + 1 < s.ni ? 2 : 0;
    const int len = c.nbytes + c.nff + marker;
    if (!EMIT) {
        if (threadIdx.x == 0) sizes[blockIdx.x] = len;
        return;
    }
    const long long at = offsets[blockIdx.x];
    if (at < 0 || at + len > out_bytes) return;                            // never past `out`, whatever the caller passed
    uint8_t* dst = out + at;
    const int lane = threadIdx.x & (WAVE - 1);
    const int nseg = (c.nbytes + 63) >> 6;
    for (int sg = threadIdx.x / WAVE; sg < nseg; sg += JPEG_BLOCK / WAVE) {
        const int k = sg * 64 + lane;
        const bool valid = k < c.nbytes;
        const uint32_t b = valid ? (L.bits[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu : 0u;
        const unsigned long long m = __ballot(b == 0xffu);
        const int p = k + L.seg[sg] + __popcll(m & ((1ull << lane) - 1ull));
        if (valid) {
            dst[p] = (uint8_t)b;
            if (b == 0xffu) dst[p + 1] = 0;
        }
    }
    if (marker && threadIdx.x == 0) {
        dst[len - 2] = 0xff;
        dst[len - 1] = (uint8_t)(0xd0 + (iv & 7));
    }
}

// one workgroup: offsets[i] = sum of sizes[0 .. i), offsets[n] = the total; frame_offsets[t] = offsets[t ni]
__global__ void __launch_bounds__(JPEG_BLOCK)
    jpeg_scan_kernel(const int32_t* __restrict__ sizes, int n, int ni, long long* __restrict__ offsets,
                     long long* __restrict__ frame_offsets) {
    __shared__ int tot[JPEG_BLOCK / WAVE];
    long long carry = 0;
    for (int base = 0; base < n; base += JPEG_BLOCK) {
        const int i = base + threadIdx.x;
        int total;
        const int ex = block_scan_excl<JPEG_BLOCK>(i < n ? sizes[i] : 0, tot, total);
        if (i < n) {
            offsets[i] = carry + ex;
            if (i % ni == 0) frame_offsets[i / ni] = carry + ex;
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        offsets[n] = carry;
        frame_offsets[n / ni] = carry;
    }
}

// ---- host side
static bool jpeg_shape(int T, int C, int W, int H, JpegShape& s) {
    if (T < 1 || (C != 1 && C != 3) || W < 1 || H < 1 || W > JPEG_MAX_SIDE || H > JPEG_MAX_SIDE) return false;
    s = {T, C, W, H, (W + 7) / 8, (H + 7) / 8, 0};
    s.ni = (s.mx * s.my + JPEG_RI - 1) / JPEG_RI;
    return (long long)T * s.ni <= JPEG_MAX_INTERVALS;
}
struct JpegWorkspace { int32_t* sizes; long long* offsets; };
static JpegWorkspace jpeg_carve(Arena& ar, const JpegShape& s) {
    JpegWorkspace w;
    const size_t n = (size_t)s.T * s.ni;
    w.sizes = ar.take<int32_t>("interval_sizes", n);
    w.offsets = ar.take<long long>("interval_offsets", n + 1);
    return w;
}

}  // namespace gfl

using namespace gfl;

extern "C" {

int gfl_jpeg_restart_interval(void) { return JPEG_RI; }

size_t gfl_jpeg_workspace_bytes(int T, int C, int W, int H) {
    JpegShape s;
    if (!jpeg_shape(T, C, W, H, s)) return 0;
    Arena ar;
    jpeg_carve(ar, s);
    return ar.off;
}

int gfl_jpeg_sizes(const uint8_t* images, int T, int C, int W, int H, const uint16_t* qtables, int64_t* frame_offsets,
                   void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    JpegShape s;
    if (!jpeg_shape(T, C, W, H, s) || !images || !qtables || !frame_offsets || !workspace) return GFL_ERR_INVALID;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)frame_offsets & 7) || ((uintptr_t)qtables & 1)) return GFL_ERR_INVALID;
    Arena ar;
    ar.base = (char*)workspace;
    const JpegWorkspace w = jpeg_carve(ar, s);
    if (workspace_bytes < ar.off) return GFL_ERR_WORKSPACE;
    const hipStream_t st = (hipStream_t)stream;
    const int n = T * s.ni;
    if (C == 3) jpeg_kernel<3, false><<<n, JPEG_BLOCK, 0, st>>>(images, qtables, s, w.sizes, nullptr, nullptr, 0);
    else jpeg_kernel<1, false><<<n, JPEG_BLOCK, 0, st>>>(images, qtables, s, w.sizes, nullptr, nullptr, 0);
    if (int rc = check_launch()) return rc;
    jpeg_scan_kernel<<<1, JPEG_BLOCK, 0, st>>>(w.sizes, n, s.ni, w.offsets, (long long*)frame_offsets);
    return check_launch();
}

int gfl_jpeg_emit(const uint8_t* images, int T, int C, int W, int H, const uint16_t* qtables, uint8_t* out, int64_t out_bytes,
                  void* workspace, size_t workspace_bytes, gfl_stream_t stream) {
    JpegShape s;
    if (!jpeg_shape(T, C, W, H, s) || !images || !qtables || !out || !workspace || out_bytes < 1) return GFL_ERR_INVALID;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)qtables & 1)) return GFL_ERR_INVALID;
    Arena ar;
    ar.base = (char*)workspace;
    const JpegWorkspace w = jpeg_carve(ar, s);
    if (workspace_bytes < ar.off) return GFL_ERR_WORKSPACE;
    const hipStream_t st = (hipStream_t)stream;
    const int n = T * s.ni;
    if (C == 3) jpeg_kernel<3, true><<<n, JPEG_BLOCK, 0, st>>>(images, qtables, s, nullptr, w.offsets, out, (long long)out_bytes);
    else jpeg_kernel<1, true><<<n, JPEG_BLOCK, 0, st>>>(images, qtables, s, nullptr, w.offsets, out, (long long)out_bytes);
    return check_launch();
}

}  // extern "C"
