// Lossless images on the device (include/gflow_hip.h, "PNG files"): T images of (H, W, C) uint8 -> the zlib stream of T PNG
// files (RFC 1950 / 1951; PNG's filter type 2, Up, on every row).  The host wraps a stream in chunks (gflow_amd.png.png_chunks).
// An image is cut into strips of gfl_png_strip_rows rows whose filtered bytes (a filter-type byte and W C bytes per row) fit
// in 32 KiB of LDS; every strip is a deflate stream of its own that ends on a byte, so ONE workgroup codes one (image, strip):
//   rows -> Up filter against the raw row above -> filtered bytes in LDS, the strip's Adler-32 on the way
//   -> runs of one byte value (a lane walks a chunk of positions; the run that leaves its chunk ends at the next run start, which
//      a suffix scan over the lanes gives): a literal, then matches of 3 .. 258 at distance 1, a tail of 1 or 2 as literals
//   -> histogram of the literal / length symbols -> Huffman code lengths <= 15, Kraft sum exactly 1 (huff_build)
//   -> the code-length sequence with symbols 16 / 17 / 18, its own code of <= 7 bits through the same routine
//   -> every lane counts its tokens' bits -> prefix sum -> the lane ORs its codes into an LDS bit buffer at its offset
//   -> one non-final dynamic block + an empty stored block (000, pad, 00 00 FF FF); or, if that is longer, one stored block.
// Two passes over the same routine (png_strip): gfl_png_sizes keeps every strip's length and Adler-32, scans the lengths into
// offsets and combines the sums per image; gfl_png_emit codes again and writes at the offset.  Integer LDS atomics only: the
// bytes do not depend on the order in which lanes arrive.  No allocation, no host synchronisation.
#include "gfl_common.hpp"

namespace gfl {

constexpr int PNG_BLOCK = 256;
constexpr int PNG_STRIP_BYTES = 32768;             // filtered bytes of a strip, at most
constexpr int PNG_MAX_ROWS = 64;
constexpr long long PNG_MAX_STRIPS = 1ll << 30;
constexpr int PNG_NSYM = 286;                      // literals, EOB (256), lengths 257 .. 285
constexpr int PNG_EOB = 256;
constexpr int PNG_NCL = 19;
constexpr uint32_t ADLER_MOD = 65521u;

__host__ __device__ inline int png_strip_rows(int C, int W) {
    if ((C != 1 && C != 3) || W < 1) return 0;
    const long long rl = 1 + (long long)W * C;
    if (rl > PNG_STRIP_BYTES) return 0;
    const int r = (int)(PNG_STRIP_BYTES / rl);
    return r < 1 ? 1 : (r > PNG_MAX_ROWS ? PNG_MAX_ROWS : r);
}

// ---- Huffman code lengths of a histogram, limited to maxlen, and the canonical codes: the ONE routine of both alphabets
struct HuffScratch {
    uint32_t nodew[2 * PNG_NSYM + 4];              // leaves in ascending order of (count, symbol), then the inner nodes as made
    uint16_t parent[2 * PNG_NSYM + 4];
    uint16_t sorted[PNG_NSYM + 2];                 // the leaves' symbols
    int cnt[16], start[16], next[16];              // codes per length; first leaf of a length; first code of a length
    int m, bad;
};

// freq[nsym] -> len[nsym] (0: unused) and ent[nsym] = the code, bit-reversed for deflate's LSB-first packing, | len << 16.
// At least one count is non-zero.  A lone used symbol gets a partner of length 1 (inflate refuses an incomplete code).
// S.bad is set if the lengths are not a complete code (never seen; the caller then stores the strip).  Whole workgroup.
__device__ void huff_build(const uint32_t* freq, int nsym, int maxlen, uint8_t* len, uint32_t* ent, HuffScratch& S) {
    const int tid = threadIdx.x;
    for (int s = tid; s < nsym; s += PNG_BLOCK) {
        const uint32_t f = freq[s];
        len[s] = 0;
        if (f) {
            int r = 0;
            for (int u = 0; u < nsym; ++u) {
                const uint32_t fu = freq[u];
                r += (fu && (fu < f || (fu == f && u < s))) ? 1 : 0;
            }
            S.sorted[r] = (uint16_t)s;
            S.nodew[r] = f;
        }
    }
    if (tid < 16) S.cnt[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        int m = 0;
        for (int u = 0; u < nsym; ++u) m += freq[u] ? 1 : 0;
        if (m == 1) {
            const uint16_t s0 = S.sorted[0];
            S.sorted[1] = s0; S.nodew[1] = S.nodew[0];
            S.sorted[0] = s0 == 0 ? 1 : 0; S.nodew[0] = 0;
            m = 2;
        }
        // two queues: the leaves and the inner nodes, both in ascending order; a leaf wins a tie (the flatter tree)
        int a = 0, b = m, nn = m;
        for (int k = 0; k < m - 1; ++k) {
            uint32_t w = 0;
            for (int j = 0; j < 2; ++j) {
                int x;
                if (a < m && (b >= nn || S.nodew[a] <= S.nodew[b])) x = a++;
                else x = b++;
                S.parent[x] = (uint16_t)nn;
                w += S.nodew[x];
            }
            S.nodew[nn++] = w;
        }
        S.m = m;
    }
    __syncthreads();
    const int m = S.m, root = 2 * m - 2;
    for (int i = tid; i < m; i += PNG_BLOCK) {
        int d = 0;
        for (int p = i; p != root && d < 2 * PNG_NSYM; p = S.parent[p]) ++d;
        atomicAdd(&S.cnt[min(d, maxlen)], 1);
    }
    __syncthreads();
    if (tid == 0) {
        // depths cut at maxlen over-subscribe the code: take one code off the longest length and split the deepest shorter
        // one into two, a unit of 2^-maxlen at a time, until the Kraft sum is exactly 1 again
        int total = 0;
        for (int l = 1; l <= maxlen; ++l) total += S.cnt[l] << (maxlen - l);
        for (int guard = 0; total > (1 << maxlen) && S.cnt[maxlen] > 0 && guard < 4 * PNG_NSYM; ++guard) {
            --S.cnt[maxlen];
            for (int l = maxlen - 1; l >= 1; --l)
                if (S.cnt[l]) {
                    --S.cnt[l];
                    S.cnt[l + 1] += 2;
                    break;
                }
            --total;
        }
        S.bad = total != (1 << maxlen);
        int pos = 0, code = 0;
        for (int l = maxlen; l >= 1; --l) { S.start[l] = pos; pos += S.cnt[l]; }        // the rarest leaves get the longest codes
        S.cnt[0] = 0;
        for (int l = 1; l <= maxlen; ++l) { code = (code + S.cnt[l - 1]) << 1; S.next[l] = code; }
    }
    __syncthreads();
    for (int i = tid; i < m; i += PNG_BLOCK) {
        int l = maxlen;
        while (l > 1 && !(i >= S.start[l] && i < S.start[l] + S.cnt[l])) --l;
        len[S.sorted[i]] = (uint8_t)l;
    }
    __syncthreads();
    for (int s = tid; s < nsym; s += PNG_BLOCK) {
        const int l = len[s];
        uint32_t e = 0;
        if (l) {
            int c = S.next[l];
            for (int u = 0; u < s; ++u) c += len[u] == l ? 1 : 0;
            e = (__brev((uint32_t)c) >> (32 - l)) | ((uint32_t)l << 16);
        }
        ent[s] = e;
    }
    __syncthreads();
}

// ---- tokens.  A match length 3 .. 258 as (symbol, extra bit count, extra bits): RFC 1951 3.2.5
struct LenCode { int sym, ebits, extra; };
__device__ __forceinline__ LenCode png_len_code(int length) {
    const int l = length - 3;
    if (l < 8) return {257 + l, 0, 0};
    if (length == 258) return {285, 0, 0};
    const int eb = 29 - __clz(l);                  // l in [8 << (eb - 1), 8 << eb)
    return {261 + 4 * eb + ((l >> eb) & 3), eb, l & ((1 << eb) - 1)};
}

// a run of `L` bytes of value v: the literal, matches of 258 while 258 are left, then a match of 3 .. 257 or 1 .. 2 literals
struct RunTokens { int lits, n258, tail; };        // tail: 0, or the last match's length
__device__ __forceinline__ RunTokens png_run_tokens(int L) {
    const int R = L - 1, t = R % 258;
    return {1 + (t < 3 ? t : 0), R / 258, t < 3 ? 0 : t};
}

struct LsbWriter {                                 // ORs into words that hold the stream LSB first, from bit `pos`
    uint32_t* buf;
    int w, n;
    unsigned long long acc = 0;
    __device__ LsbWriter(uint32_t* b, int pos) : buf(b), w(pos >> 5), n(pos & 31) {}
    __device__ __forceinline__ void put(uint32_t v, int len) {       // len <= 32 - 1
        acc |= (unsigned long long)v << n;
        n += len;
        if (n >= 32) {
            atomicOr(&buf[w++], (uint32_t)acc);
            acc >>= 32;
            n -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (n > 0) atomicOr(&buf[w], (uint32_t)acc);
    }
};

// what a lane does with a run it owns: the three sinks of the one walk
struct HistSink {
    uint32_t* hist;
    __device__ __forceinline__ void run(int v, int L) {
        const RunTokens r = png_run_tokens(L);
        atomicAdd(&hist[v], (uint32_t)r.lits);
        if (r.n258) atomicAdd(&hist[285], (uint32_t)r.n258);
        if (r.tail) atomicAdd(&hist[png_len_code(r.tail).sym], 1u);
    }
};
struct CountSink {                                 // a match: its length code, the extra bits, one bit of distance code
    const uint32_t* ent;
    int bits = 0;
    __device__ __forceinline__ void run(int v, int L) {
        const RunTokens r = png_run_tokens(L);
        bits += r.lits * (int)(ent[v] >> 16) + r.n258 * ((int)(ent[285] >> 16) + 1);
        if (r.tail) {
            const LenCode c = png_len_code(r.tail);
            bits += (int)(ent[c.sym] >> 16) + c.ebits + 1;
        }
    }
};
struct WriteSink {
    const uint32_t* ent;
    LsbWriter wr;
    __device__ __forceinline__ void sym(int s, uint32_t extra, int more) {   // the code, then `more` bits of `extra`
        const uint32_t e = ent[s];
        const int l = (int)(e >> 16);
        wr.put((e & 0xffffu) | (extra << l), l + more);
    }
    __device__ __forceinline__ void run(int v, int L) {
        const RunTokens r = png_run_tokens(L);
        sym(v, 0, 0);
        for (int k = 0; k < r.n258; ++k) sym(285, 0, 1);                    // (the distance code of distance 1 is the bit 0)
        if (r.tail) {
            const LenCode c = png_len_code(r.tail);
            sym(c.sym, (uint32_t)c.extra, c.ebits + 1);
        } else {
            for (int k = 1; k < r.lits; ++k) sym(v, 0, 0);
        }
    }
};

// The lane's chunk is the positions [c0, c0 + per) below n.  It owns the runs that START there; `next_start`: the first run
// start behind the chunk (n if none).
template <class Sink>
__device__ __forceinline__ void png_walk(const uint8_t* fb, int n, int c0, int per, int next_start, Sink& sink) {
    int own = -1, val = 0;
    int prev = c0 > 0 && c0 <= n ? fb[c0 - 1] : -1;
    const int c1 = min(c0 + per, n);
    for (int i = c0; i < c1; ++i) {
        const int b = fb[i];
        if (b != prev) {
            if (own >= 0) sink.run(val, i - own);
            own = i;
            val = b;
        }
        prev = b;
    }
    if (own >= 0) sink.run(val, next_start - own);
}

struct PngLds {
    uint32_t fbw[PNG_STRIP_BYTES / 4 + 4];         // the strip's filtered bytes
    uint32_t bits[(PNG_STRIP_BYTES + 8) / 4 + 8];  // a dynamic block is only written when it is no longer than the stored one
    uint32_t hist[PNG_NSYM + 2], ent[PNG_NSYM + 2];
    uint32_t clhist[PNG_NCL + 1], clent[PNG_NCL + 1];
    uint16_t cltok[PNG_NSYM + 8];                  // the code-length sequence: symbol | extra << 8
    uint8_t len[PNG_NSYM + 2], cllen[PNG_NCL + 1];
    HuffScratch hs;
    int tot[PNG_BLOCK / WAVE];
    int firsts[PNG_BLOCK];                         // every lane's first run start, then the suffix minimum behind the lane
    int ncl, hlit, hclen, hdr_bits, bad;
};

struct PngShape { int T, C, W, H, rows, ns; };     // rows per strip; strips per image
struct PngCoded { int n, len, dynamic, nbits; uint32_t adler; };       // filtered bytes; coded bytes; nbits: through EOB and 000

__constant__ uint8_t PNG_CL_ORDER[PNG_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int png_cl_extra_bits(int sym) { return sym == 16 ? 2 : (sym == 17 ? 3 : (sym == 18 ? 7 : 0)); }

// code strip `sp` of image `t`: L.fbw, and -- WRITE, and the dynamic block is the shorter one -- the block's bits in L.bits
template <bool WRITE>
__device__ PngCoded png_strip(PngLds& L, const uint8_t* __restrict__ images, const PngShape& s, int t, int sp) {
    const int tid = threadIdx.x;
    const int wc = s.W * s.C, rl = wc + 1;
    const int y0 = sp * s.rows, nrows = min(s.rows, s.H - y0), n = nrows * rl;
    uint8_t* fb = (uint8_t*)L.fbw;
    const uint8_t* img = images + (size_t)t * s.H * (size_t)wc;
    // Up against the raw row above; the strip's Adler sums: A = 1 + sum b, B = n + sum (n - i) b
    unsigned long long sa = 0, sb = 0;
    for (int r = 0; r < nrows; ++r) {
        const int y = y0 + r;
        const uint8_t* cur = img + (size_t)y * wc;
        const uint8_t* up = y > 0 ? cur - wc : nullptr;
        for (int x = tid; x < wc; x += PNG_BLOCK) {
            const uint32_t b = (uint8_t)(cur[x] - (up ? up[x] : 0));
            const int i = r * rl + 1 + x;
            fb[i] = (uint8_t)b;
            sa += b;
            sb += (unsigned long long)(n - i) * b;
        }
        if (tid == (r & (PNG_BLOCK - 1))) {
            fb[r * rl] = 2;
            sa += 2u;
            sb += (unsigned long long)(n - r * rl) * 2u;
        }
    }
    for (int i = tid; i < PNG_NSYM; i += PNG_BLOCK) L.hist[i] = i == PNG_EOB ? 1u : 0u;
    if (tid < PNG_NCL) L.clhist[tid] = 0u;
    PngCoded out;
    out.n = n;
    out.adler = 0;
    if (!WRITE) {
        int ta, tb;
        block_scan_excl<PNG_BLOCK>((int)(sa % ADLER_MOD), L.tot, ta);
        block_scan_excl<PNG_BLOCK>((int)(sb % ADLER_MOD), L.tot, tb);
        out.adler = (((uint32_t)tb + (uint32_t)n) % ADLER_MOD) << 16 | ((uint32_t)ta + 1u) % ADLER_MOD;
    }
    __syncthreads();
    // a lane's chunk: a multiple of four bytes and an odd number of words, so that the lanes' reads fall into different banks
    int per = ((n + PNG_BLOCK - 1) / PNG_BLOCK + 3) & ~3;
    if (!(per & 4)) per += 4;
    const int c0 = tid * per;
    {
        int first = n;
        for (int i = min(c0 + per, n) - 1; i >= c0; --i)
            if (i == 0 || fb[i] != fb[i - 1]) first = i;
        L.firsts[tid] = first;
    }
    __syncthreads();
    if (tid < WAVE) {                              // suffix minimum over the 256 lanes, exclusive: a wave, four lanes' values each
        int v[4], run = n;
        for (int k = 3; k >= 0; --k) v[k] = L.firsts[tid * 4 + k];
        int mine = min(min(v[0], v[1]), min(v[2], v[3]));
        int suf = mine;                            // inclusive suffix minimum over the wave's lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_down(suf, off);
            if (tid + off < 64) suf = min(suf, o);
        }
        const int behind = __shfl_down(suf, 1);
        run = tid < 63 ? behind : n;
        for (int k = 3; k >= 0; --k) {
            const int own = v[k];
            L.firsts[tid * 4 + k] = run;
            run = min(run, own);
        }
    }
    __syncthreads();
    const int next_start = L.firsts[tid];
    {
        HistSink h{L.hist};
        png_walk(fb, n, c0, per, next_start, h);
    }
    __syncthreads();
    huff_build(L.hist, PNG_NSYM, 15, L.len, L.ent, L.hs);
    if (tid == 0) {
        L.bad = L.hs.bad;
        // the code-length sequence: the literal / length lengths up to the last used one, then the one distance code of length 1
        int hlit = PNG_NSYM;
        while (hlit > 257 && L.len[hlit - 1] == 0) --hlit;
        L.len[hlit] = 1;
        const int N = hlit + 1;
        int nt = 0;
        auto tok = [&](int sym, int extra) {
            L.cltok[nt++] = (uint16_t)(sym | (extra << 8));
            ++L.clhist[sym];
        };
        for (int j = 0; j < N;) {
            const int v = L.len[j];
            int r = 1;
            while (j + r < N && L.len[j + r] == v) ++r;
            j += r;
            if (v == 0) {
                while (r >= 11) { const int c = min(r, 138); tok(18, c - 11); r -= c; }
                if (r >= 3) { tok(17, r - 3); r = 0; }
                while (r-- > 0) tok(0, 0);
            } else {
                tok(v, 0);
                --r;
                while (r >= 3) { const int c = min(r, 6); tok(16, c - 3); r -= c; }
                while (r-- > 0) tok(v, 0);
            }
        }
        L.ncl = nt;
        L.hlit = hlit;
    }
    __syncthreads();
    huff_build(L.clhist, PNG_NCL, 7, L.cllen, L.clent, L.hs);
    if (tid == 0) {
        L.bad |= L.hs.bad;
        int hclen = PNG_NCL;
        while (hclen > 4 && L.cllen[PNG_CL_ORDER[hclen - 1]] == 0) --hclen;
        int bits = 3 + 5 + 5 + 4 + 3 * hclen;
        for (int k = 0; k < L.ncl; ++k) {
            const int sym = L.cltok[k] & 0xff;
            bits += L.cllen[sym] + png_cl_extra_bits(sym);
        }
        L.hclen = hclen;
        L.hdr_bits = bits;
    }
    CountSink cs{L.ent};
    png_walk(fb, n, c0, per, next_start, cs);
    int body_bits;
    const int at = block_scan_excl<PNG_BLOCK>(cs.bits, L.tot, body_bits);            // (its barriers also publish hdr_bits)
    const int hdr_bits = L.hdr_bits;
    const int eob_at = hdr_bits + body_bits;
    out.nbits = eob_at + (int)(L.ent[PNG_EOB] >> 16) + 3;
    const int dyn_len = (out.nbits + 7) / 8 + 4;
    out.dynamic = !L.bad && dyn_len <= n + 5;
    out.len = out.dynamic ? dyn_len : n + 5;
    if (!WRITE || !out.dynamic) return out;
    for (int i = tid; i < out.nbits / 32 + 2; i += PNG_BLOCK) L.bits[i] = 0u;
    __syncthreads();
    if (tid == 0) {
        LsbWriter wr(L.bits, 0);
        wr.put(0u, 1);                             // BFINAL = 0
        wr.put(2u, 2);                             // BTYPE = 10
        wr.put((uint32_t)(L.hlit - 257), 5);
        wr.put(0u, 5);                             // one distance code
        wr.put((uint32_t)(L.hclen - 4), 4);
        for (int k = 0; k < L.hclen; ++k) wr.put(L.cllen[PNG_CL_ORDER[k]], 3);
        for (int k = 0; k < L.ncl; ++k) {
            const int sym = L.cltok[k] & 0xff, extra = L.cltok[k] >> 8;
            const uint32_t e = L.clent[sym];
            const int l = (int)(e >> 16);
            wr.put((e & 0xffffu) | ((uint32_t)extra << l), l + png_cl_extra_bits(sym));
        }
        wr.flush();
    }
    if (tid == PNG_BLOCK - 1) {                    // EOB, then the empty stored block's 000
        LsbWriter wr(L.bits, eob_at);
        const uint32_t e = L.ent[PNG_EOB];
        wr.put(e & 0xffffu, (int)(e >> 16));
        wr.put(0u, 3);
        wr.flush();
    }
    {
        WriteSink ws{L.ent, LsbWriter(L.bits, hdr_bits + at)};
        png_walk(fb, n, c0, per, next_start, ws);
        ws.wr.flush();
    }
    __syncthreads();
    return out;
}

// a strip's bytes in `out`: 78 01 in front of an image's first, 03 00 and the image's Adler-32 behind its last
__device__ __forceinline__ int png_strip_extra(int sp, int ns) { return (sp == 0 ? 2 : 0) + (sp == ns - 1 ? 6 : 0); }

// EMIT = false: sizes[t ns + sp] = the strip's bytes in `out`, adlers[..] its Adler-32.  EMIT = true: the bytes at offsets[..]
template <bool EMIT>
__global__ void __launch_bounds__(PNG_BLOCK)
    png_kernel(const uint8_t* __restrict__ images, PngShape s, int32_t* __restrict__ sizes, uint32_t* __restrict__ adlers,
               const long long* __restrict__ offsets, const uint32_t* __restrict__ image_adler, uint8_t* __restrict__ out,
               long long out_bytes) {
    __shared__ PngLds L;
    const int t = blockIdx.x / s.ns, sp = blockIdx.x - t * s.ns;
    const PngCoded c = png_strip<EMIT>(L, images, s, t, sp);
    const int len = c.len + png_strip_extra(sp, s.ns);
    if (!EMIT) {
        if (threadIdx.x == 0) {
            sizes[blockIdx.x] = len;
            adlers[blockIdx.x] = c.adler;
        }
        return;
    }
    const long long at = offsets[blockIdx.x];
    if (at < 0 || at + len > out_bytes) return;                            // never past `out`, whatever the caller passed
    uint8_t* dst = out + at;
    const int tid = threadIdx.x;
    if (sp == 0) {
        if (tid == 0) { dst[0] = 0x78; dst[1] = 0x01; }
        dst += 2;
    }
    if (c.dynamic) {
        const uint8_t* src = (const uint8_t*)L.bits;                       // (words that hold the stream LSB first: its bytes)
        const int nb = c.len - 4;
        for (int k = tid; k < nb; k += PNG_BLOCK) dst[k] = src[k];
        if (tid < 4) dst[nb + tid] = tid < 2 ? 0x00 : 0xff;
    } else {
        const uint8_t* src = (const uint8_t*)L.fbw;
        if (tid == 0) {
            dst[0] = 0x00;                                                 // BFINAL = 0, BTYPE = 00, on a byte boundary
            dst[1] = (uint8_t)(c.n & 0xff); dst[2] = (uint8_t)(c.n >> 8);
            dst[3] = (uint8_t)(~c.n & 0xff); dst[4] = (uint8_t)((~c.n >> 8) & 0xff);
        }
        for (int k = tid; k < c.n; k += PNG_BLOCK) dst[5 + k] = src[k];
    }
    if (sp == s.ns - 1 && tid == 0) {
        uint8_t* e = dst + c.len;
        const uint32_t a = image_adler[t];
        e[0] = 0x03; e[1] = 0x00;                                          // a final block of the fixed code that holds EOB alone
        e[2] = (uint8_t)(a >> 24); e[3] = (uint8_t)(a >> 16); e[4] = (uint8_t)(a >> 8); e[5] = (uint8_t)a;
    }
}

// one workgroup: offsets[i] = sum of sizes[0 .. i), offsets[n] = the total; frame_offsets[t] = offsets[t ns]; image_adler[t] =
// the strips' sums combined in order: A = A1 + A2 - 1, B = B1 + B2 + n2 (A1 - 1), both mod 65521
__global__ void __launch_bounds__(PNG_BLOCK)
    png_scan_kernel(const int32_t* __restrict__ sizes, const uint32_t* __restrict__ adlers, PngShape s, long long* __restrict__ offsets,
                    long long* __restrict__ frame_offsets, uint32_t* __restrict__ image_adler) {
    __shared__ int tot[PNG_BLOCK / WAVE];
    const int n = s.T * s.ns, ns = s.ns;
    long long carry = 0;
    for (int base = 0; base < n; base += PNG_BLOCK) {
        const int i = base + threadIdx.x;
        int total;
        const int ex = block_scan_excl<PNG_BLOCK>(i < n ? sizes[i] : 0, tot, total);
        if (i < n) {
            offsets[i] = carry + ex;
            if (i % ns == 0) frame_offsets[i / ns] = carry + ex;
        }
        carry += total;
    }
    if (threadIdx.x == 0) {
        offsets[n] = carry;
        frame_offsets[s.T] = carry;
    }
    const unsigned long long rl = 1ull + (unsigned long long)s.W * s.C;
    for (int t = threadIdx.x; t < s.T; t += PNG_BLOCK) {
        unsigned long long A = 1, B = 0;
        for (int sp = 0; sp < ns; ++sp) {
            const uint32_t ad = adlers[(size_t)t * ns + sp];
            const unsigned long long A2 = ad & 0xffffu, B2 = ad >> 16;
            const unsigned long long n2 = (unsigned long long)min(s.rows, s.H - sp * s.rows) * rl;
            B = (B + B2 + (n2 % ADLER_MOD) * ((A + ADLER_MOD - 1) % ADLER_MOD)) % ADLER_MOD;
            A = (A + A2 + ADLER_MOD - 1) % ADLER_MOD;
        }
        image_adler[t] = (uint32_t)(B << 16 | A);
    }
}

// ---- host side
static bool png_shape(int T, int C, int W, int H, PngShape& s) {
    if (T < 1 || H < 1) return false;
    const int rows = png_strip_rows(C, W);
    if (rows == 0) return false;
    s = {T, C, W, H, rows, (int)(((long long)H + rows - 1) / rows)};
    return (long long)T * s.ns <= PNG_MAX_STRIPS;
}
struct PngWorkspace { int32_t* sizes; uint32_t* adlers; long long* offsets; uint32_t* image_adler; };
static PngWorkspace png_carve(Arena& ar, const PngShape& s) {
    PngWorkspace w;
    const size_t n = (size_t)s.T * s.ns;
    w.sizes = ar.take<int32_t>("strip_sizes", n);
    w.adlers = ar.take<uint32_t>("strip_adlers", n);
    w.offsets = ar.take<long long>("strip_offsets", n + 1);
    w.image_adler = ar.take<uint32_t>("image_adlers", (size_t)s.T);
    return w;
}

}  // namespace gfl

using namespace gfl;

extern "C" {

int gfl_png_strip_rows(int C, int W) { return png_strip_rows(C, W); }

size_t gfl_png_workspace_bytes(int T, int C, int W, int H) {
    PngShape s;
    if (!png_shape(T, C, W, H, s)) return 0;
    Arena ar;
    png_carve(ar, s);
    return ar.off;
}

int gfl_png_sizes(const uint8_t* images, int T, int C, int W, int H, int64_t* frame_offsets, void* workspace,
                  size_t workspace_bytes, gfl_stream_t stream) {
    PngShape s;
    if (!png_shape(T, C, W, H, s) || !images || !frame_offsets || !workspace) return GFL_ERR_INVALID;
    if (((uintptr_t)workspace & 7) || ((uintptr_t)frame_offsets & 7)) return GFL_ERR_INVALID;
    Arena ar;
    ar.base = (char*)workspace;
    const PngWorkspace w = png_carve(ar, s);
    if (workspace_bytes < ar.off) return GFL_ERR_WORKSPACE;
    const hipStream_t st = (hipStream_t)stream;
    png_kernel<false><<<T * s.ns, PNG_BLOCK, 0, st>>>(images, s, w.sizes, w.adlers, nullptr, nullptr, nullptr, 0);
    if (int rc = check_launch()) return rc;
    png_scan_kernel<<<1, PNG_BLOCK, 0, st>>>(w.sizes, w.adlers, s, w.offsets, (long long*)frame_offsets, w.image_adler);
    return check_launch();
}

int gfl_png_emit(const uint8_t* images, int T, int C, int W, int H, uint8_t* out, int64_t out_bytes, void* workspace,
                 size_t workspace_bytes, gfl_stream_t stream) {
    PngShape s;
    if (!png_shape(T, C, W, H, s) || !images || !out || !workspace || out_bytes < 1) return GFL_ERR_INVALID;
    if ((uintptr_t)workspace & 7) return GFL_ERR_INVALID;
    Arena ar;
    ar.base = (char*)workspace;
    const PngWorkspace w = png_carve(ar, s);
    if (workspace_bytes < ar.off) return GFL_ERR_WORKSPACE;
    png_kernel<true><<<T * s.ns, PNG_BLOCK, 0, (hipStream_t)stream>>>(images, s, nullptr, nullptr, w.offsets, w.image_adler, out,
                                                                     (long long)out_bytes);
    return check_launch();
}

}  // extern "C"
