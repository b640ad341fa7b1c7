"""Float-free restatement of the PNG coder (include/gflow_hip.h, "PNG files"), for tests: the strips, the Up filter, the run
tokens, the exact (unlimited) Huffman depth of a histogram, a reference stream per image from zlib on the same strips, the
Adler-32 combine -- and ``model_stream``, the library's own rules (code builder, length limiter, table coding) in plain Python."""
import heapq
import zlib

import numpy as np

ADLER_MOD = 65521
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def strip_rows(C, W):
    """gfl_png_strip_rows' formula"""
    if C not in (1, 3) or W < 1:
        return 0
    rl = 1 + W * C
    if rl > 32768:
        return 0
    return max(1, min(64, 32768 // rl))


def as_hwc(image):
    image = np.asarray(image)
    return image[:, :, None] if image.ndim == 2 else image


def filtered_rows(image):
    """(H, 1 + W C) uint8: filter type 2 and every row minus the raw row above (zeros above row 0), mod 256"""
    image = as_hwc(image)
    H, W, C = image.shape
    raw = image.reshape(H, W * C).astype(np.int16)
    up = np.concatenate([np.zeros((1, W * C), np.int16), raw[:-1]])
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = 2
    out[:, 1:] = ((raw - up) & 255).astype(np.uint8)
    return out


def strips(image):
    """the filtered bytes of every strip, in order"""
    image = as_hwc(image)
    H, W, C = image.shape
    rows = strip_rows(C, W)
    assert rows > 0
    f = filtered_rows(image)
    return [f[y:y + rows].tobytes() for y in range(0, H, rows)]


def filtered_bytes(image):
    return filtered_rows(image).tobytes()


def run_tokens(data):
    """the tokens of a strip's filtered bytes: ("lit", value) or ("match", length) at distance 1.  A run of one value is its
    first byte, matches of 258 while 258 are left, then a match of 3 .. 257 or 1 .. 2 literals"""
    out = []
    a = np.frombuffer(data, np.uint8)
    starts = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    ends = np.concatenate([starts[1:], [len(a)]])
    for s, e in zip(starts.tolist(), ends.tolist()):
        v = int(a[s])
        out.append(("lit", v))
        rest = e - s - 1
        out += [("match", 258)] * (rest // 258)
        tail = rest % 258
        out += [("match", tail)] if tail >= 3 else [("lit", v)] * tail
    return out


def expand_tokens(tokens):
    out = bytearray()
    for kind, v in tokens:
        if kind == "lit":
            out.append(v)
        else:
            out += bytes([out[-1]]) * v
    return bytes(out)


def length_code(length):
    """(symbol, extra bit count, extra bits) of a match length: RFC 1951 3.2.5"""
    if length == 258:
        return 285, 0, 0
    l = length - 3
    if l < 8:
        return 257 + l, 0, 0
    eb = l.bit_length() - 3
    return 261 + 4 * eb + ((l >> eb) & 3), eb, l & ((1 << eb) - 1)


def histogram(tokens):
    """counts of the 286 literal / length symbols, EOB (256) once"""
    h = [0] * 286
    h[256] = 1
    for kind, v in tokens:
        h[v if kind == "lit" else length_code(v)[0]] += 1
    return h


def huffman_depths(hist):
    """symbol -> depth in an unlimited Huffman tree of the non-zero counts (ties: the lower symbol / the older node first)"""
    heap = [(c, i, (i,)) for i, c in enumerate(hist) if c]
    depth = {i: 0 for _, i, _ in heap}
    if len(heap) == 1:
        return {heap[0][1]: 1}
    heapq.heapify(heap)
    tick = len(hist)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    return depth


def adler_combine(a1, a2, n2):
    """the Adler-32 of x1 + x2 from adler32(x1), adler32(x2) and len(x2)"""
    A1, B1, A2, B2 = a1 & 0xffff, a1 >> 16, a2 & 0xffff, a2 >> 16
    B = (B1 + B2 + n2 * (A1 - 1)) % ADLER_MOD
    A = (A1 + A2 - 1) % ADLER_MOD
    return B << 16 | A


def reference_stream(image):
    """zlib's own stream on the same strips: run matches only (Z_RLE), its optimal dynamic codes, a sync flush behind every
    strip (the empty stored block that ends it on a byte)"""
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
    out = [b"\x78\x01"]
    ad = 1
    for s in strips(image):
        out.append(co.compress(s) + co.flush(zlib.Z_SYNC_FLUSH))
        ad = adler_combine(ad, zlib.adler32(s), len(s))
    out.append(co.flush(zlib.Z_FINISH))
    out.append(ad.to_bytes(4, "big"))
    return b"".join(out)


# ---------------------------------------------------------------------------------------------- the library's own rules
def limited_lengths(hist, maxlen):
    """The library's code builder: lengths <= maxlen with Kraft sum exactly 1.  Leaves in ascending (count, symbol), the
    two-queue Huffman merge (a leaf wins a tie), depths cut at maxlen, then one code off the longest length and the deepest
    shorter one split in two until the sum is 1 again; the rarest symbols get the longest codes."""
    order = sorted((c, s) for s, c in enumerate(hist) if c)
    if len(order) == 1:
        order = [(0, 1 if order[0][1] == 0 else 0)] + order
    m = len(order)
    w = [c for c, _ in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    a, b, nn = 0, m, m
    for _ in range(m - 1):
        tot = 0
        for _ in range(2):
            if a < m and (b >= nn or w[a] <= w[b]):
                x = a
                a += 1
            else:
                x = b
                b += 1
            parent[x] = nn
            tot += w[x]
        w[nn] = tot
        nn += 1
    cnt = [0] * (maxlen + 2)
    root = 2 * m - 2
    for i in range(m):
        d, p = 0, i
        while p != root:
            p = parent[p]
            d += 1
        cnt[min(d, maxlen)] += 1
    total = sum(cnt[l] << (maxlen - l) for l in range(1, maxlen + 1))
    while total > 1 << maxlen:
        cnt[maxlen] -= 1
        for l in range(maxlen - 1, 0, -1):
            if cnt[l]:
                cnt[l] -= 1
                cnt[l + 1] += 2
                break
        total -= 1
    assert total == 1 << maxlen
    lens = [0] * len(hist)
    i = 0
    for l in range(maxlen, 0, -1):
        for _ in range(cnt[l]):
            lens[order[i][1]] = l
            i += 1
    return lens


def canonical_codes(lens):
    maxlen = max(lens)
    cnt = [0] * (maxlen + 2)
    for l in lens:
        if l:
            cnt[l] += 1
    nxt, code = [0] * (maxlen + 2), 0
    for l in range(1, maxlen + 1):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):                       # n bits of v, least significant first
        self.acc |= v << self.n
        self.n += n

    def huff(self, code, n):                   # a Huffman code: most significant bit first
        self.put(int(format(code, f"0{n}b")[::-1], 2), n)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def table_tokens(seq):
    """the code-length sequence with symbols 16 / 17 / 18: (symbol, extra)"""
    out, j = [], 0
    while j < len(seq):
        v, r = seq[j], 1
        while j + r < len(seq) and seq[j + r] == v:
            r += 1
        j += r
        if v == 0:
            while r >= 11:
                c = min(r, 138)
                out.append((18, c - 11))
                r -= c
            if r >= 3:
                out.append((17, r - 3))
                r = 0
            out += [(0, 0)] * r
        else:
            out.append((v, 0))
            r -= 1
            while r >= 3:
                c = min(r, 6)
                out.append((16, c - 3))
                r -= c
            out += [(v, 0)] * r
    return out


def model_strip(data):
    """the bytes the library codes a strip's filtered bytes into"""
    tokens = run_tokens(data)
    lens = limited_lengths(histogram(tokens), 15)
    codes = canonical_codes(lens)
    hlit = 286
    while hlit > 257 and lens[hlit - 1] == 0:
        hlit -= 1
    tt = table_tokens(lens[:hlit] + [1])
    clh = [0] * 19
    for s, _ in tt:
        clh[s] += 1
    cll = limited_lengths(clh, 7)
    clc = canonical_codes(cll)
    hclen = 19
    while hclen > 4 and cll[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    w = BitWriter()
    w.put(0, 1), w.put(2, 2), w.put(hlit - 257, 5), w.put(0, 5), w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cll[CL_ORDER[k]], 3)
    for s, extra in tt:
        w.huff(clc[s], cll[s])
        w.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))
    for kind, v in tokens:
        if kind == "lit":
            w.huff(codes[v], lens[v])
        else:
            s, eb, extra = length_code(v)
            w.huff(codes[s], lens[s])
            w.put(extra, eb)
            w.put(0, 1)
    w.huff(codes[256], lens[256])
    w.put(0, 3)
    dyn = w.bytes() + b"\x00\x00\xff\xff"
    n = len(data)
    if len(dyn) > n + 5:
        return b"\x00" + n.to_bytes(2, "little") + (n ^ 0xffff).to_bytes(2, "little") + data
    return dyn


def model_stream(image):
    """the library's stream of an image"""
    out = [b"\x78\x01"]
    ad = 1
    for s in strips(image):
        out.append(model_strip(s))
        ad = adler_combine(ad, zlib.adler32(s), len(s))
    return b"".join(out) + b"\x03\x00" + ad.to_bytes(4, "big")


# ------------------------------------------------------------------------------------------------------------- contents
FIBONACCI_COUNTS = [1, 1, 1, 2, 2, 3, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1600]


def fibonacci_row():
    """(1, 4181) uint8: 18 byte values with Fibonacci counts, interleaved so that no value stands beside itself.  Together with
    the row's filter byte and EOB (one each) the histogram is the chain 1, 1 | 1, 1, 1 | 2, 2, 3 | 8, 13, .. 987 | 1600: every count
    from 8 on is more than all the smaller ones together (5 is there as 2 + 3, the last is raised to fill the row), so an
    unlimited Huffman tree is 16 deep whichever way ties fall -- the length limiter has to act."""
    counts = FIBONACCI_COUNTS
    W = sum(counts)
    assert W == 4181 and len(counts) == 18
    values = np.repeat(np.arange(10, 10 + len(counts), dtype=np.uint8), counts)
    h = (W + 1) // 2
    out = np.empty(W, np.uint8)
    out[0::2] = values[:h]
    out[1::2] = values[h:]
    return out[None, :]


def content(name, H, W, C, seed=0):
    """(H, W, C) uint8 test images"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    if name == "smooth":
        base = 127.5 + 80.0 * np.sin(x / 17.0 + 0.3) * np.cos(y / 11.0) + 30.0 * np.sin((x + y) / 5.0)
        img = np.stack([np.roll(base, 3 * c, axis=1) for c in range(C)], -1)
        return np.clip(np.rint(img + rng.normal(0.0, 3.0, img.shape)), 0, 255).astype(np.uint8)
    if name == "noise":
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if name == "flat":
        return np.full((H, W, C), 77, np.uint8)
    if name == "checker":
        return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[:, :, None], C, -1)
    if name == "runs":
        # rows are raw bytes, Up against an equal row above gives zeros: vary the rows so that the FILTERED bytes carry the runs
        n = H * W * C
        lengths, out, v = [2, 3, 258, 259, 260, 261], [], 1
        while sum(len(o) for o in out) < n:
            for l in lengths:
                out.append(np.full(l, v, np.uint8))
                v = v % 250 + 1
        flat = np.concatenate(out)[:n].reshape(H, W * C)
        return np.cumsum(flat, axis=0, dtype=np.uint8).reshape(H, W, C)         # (its Up filter gives `flat` back)
    if name == "disc":
        m = ((x - W / 2) ** 2 + (y - H / 2) ** 2 < (min(H, W) / 3) ** 2).astype(np.uint8) * 255
        return np.repeat(m[:, :, None], C, -1)
    raise ValueError(name)
