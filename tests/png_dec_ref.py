"""A plain Python / numpy PNG decoder, written from RFC 1950 (zlib), RFC 1951 (deflate) and the PNG specification (chunks,
section 9: filtering) -- the reference of gflow_amd.png.decode_png and of the decode core (csrc/gfl_inflate.hpp).  It gives
the pixels, the status of include/gflow_hip.h (GFL_PNG_*: 0, or the FIRST error in stream order) and statistics about what
the stream exercised, so that a test can say what its files cover.

The order of the checks is the contract's: the zlib header; per block the type, then (stored) LEN / NLEN, the input's end,
the output's end -- (dynamic) the counts, the code-length code, the repeats, the end-of-block code, the two codes --; per
symbol the code, the symbol's range, the distance against the output so far, the output's end; after the last block the
output's size, the trailer's presence, the Adler-32; and, once all of that has passed, the filter-type bytes."""
import struct
import zlib

import numpy as np

OK, INPUT_END, BAD_HEADER, BLOCK_TYPE, STORED_LEN, TOO_MANY_CODES, BAD_REPEAT, BAD_CODE, NO_END_OF_BLOCK, BAD_SYMBOL, \
    FAR_DISTANCE, OUTPUT_SIZE, BAD_ADLER, BAD_FILTER = range(14)
NAMES = ["ok", "input ends early", "bad zlib header", "reserved block type", "stored LEN / NLEN disagree",
         "HLIT > 286 or HDIST > 30", "bad repeat code", "over-subscribed or incomplete code", "no end-of-block code",
         "undefined or out-of-range symbol", "distance before the start of the output", "wrong output size",
         "Adler-32 mismatch", "filter type above 4"]

SIGNATURE = b"\x89PNG\r\n\x1a\n"
# RFC 1951, 3.2.5
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class Failed(Exception):
    def __init__(self, status):
        super().__init__(NAMES[status])
        self.status = status


class _Bits:
    """least significant bit first; ``left`` = the bits the stream still has"""

    def __init__(self, data, pos):
        self.data, self.pos, self.acc, self.n = data, pos, 0, 0

    def fill(self):
        take = min((64 - self.n) // 8, len(self.data) - self.pos)
        if take > 0:
            self.acc |= int.from_bytes(self.data[self.pos:self.pos + take], "little") << self.n
            self.pos += take
            self.n += 8 * take

    def take(self, k):
        """k bits, INPUT_END where the stream has fewer"""
        if self.n < k:
            self.fill()
            if self.n < k:
                raise Failed(INPUT_END)
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        return v

    def to_byte_boundary(self):
        self.take(self.n & 7)

    def unread(self):
        self.pos -= self.n >> 3
        self.acc = self.n = 0


def _code(lengths, strict):
    """(table, bits): table[the next `bits` bits] = symbol << 4 | length, 0 where no code starts so (RFC 1951, 3.2.2)"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    left, longest = 1, 0
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise Failed(BAD_CODE)
        if count[l]:
            longest = l
    if left > 0 and (strict or longest > 1):
        raise Failed(BAD_CODE)
    bits = max(longest, 1)
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = [0] * (1 << bits)
    for sym, l in enumerate(lengths):
        if l:
            c = nxt[l]
            nxt[l] += 1
            rev = int(format(c, "0%db" % l)[::-1], 2)
            table[rev::1 << l] = [sym << 4 | l] * (1 << (bits - l))
    return table, bits


def _symbol(b, code):
    table, bits = code
    if b.n < 15:
        b.fill()
    e = table[b.acc & ((1 << bits) - 1)]
    if e == 0 or (e & 15) > b.n:
        raise Failed(INPUT_END if b.n < 15 else BAD_SYMBOL)
    b.acc >>= e & 15
    b.n -= e & 15
    return e >> 4


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), _code([5] * 32, False))
    return _FIXED


def _dynamic(b):
    nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if nlen > 286 or ndist > 30:
        raise Failed(TOO_MANY_CODES)
    cl = [0] * 19
    for i in range(ncode):
        cl[CL_ORDER[i]] = b.take(3)
    code = _code(cl, True)
    lengths = []
    while len(lengths) < nlen + ndist:
        sym = _symbol(b, code)
        if sym < 16:
            lengths.append(sym)
            continue
        if sym == 16:
            if not lengths:
                raise Failed(BAD_REPEAT)
            prev, rep = lengths[-1], 3 + b.take(2)
        elif sym == 17:
            prev, rep = 0, 3 + b.take(3)
        else:
            prev, rep = 0, 11 + b.take(7)
        if len(lengths) + rep > nlen + ndist:
            raise Failed(BAD_REPEAT)
        lengths += [prev] * rep
    if lengths[256] == 0:
        raise Failed(NO_END_OF_BLOCK)
    return _code(lengths[:nlen], False), _code(lengths[nlen:], False)


def new_stats():
    return dict(blocks=set(), filters=set(), max_distance=0, max_length=0, overlap=False, stored_blocks=0, idat=0)


def inflate(stream, expect, stats=None):
    """the ``expect`` bytes of a zlib stream, or Failed(status)"""
    stats = new_stats() if stats is None else stats
    stream = bytes(stream)
    if len(stream) < 2:
        raise Failed(INPUT_END)
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf << 8 | flg) % 31 or flg & 32:
        raise Failed(BAD_HEADER)
    b = _Bits(stream, 2)
    out = bytearray()
    while True:
        last, kind = b.take(1), b.take(2)
        if kind == 3:
            raise Failed(BLOCK_TYPE)
        stats["blocks"].add(kind)
        if kind == 0:
            b.to_byte_boundary()
            b.unread()
            if b.pos + 4 > len(stream):
                raise Failed(INPUT_END)
            n, inv = struct.unpack_from("<HH", stream, b.pos)
            if n ^ 0xffff != inv:
                raise Failed(STORED_LEN)
            b.pos += 4
            if n > len(stream) - b.pos:
                raise Failed(INPUT_END)
            if n > expect - len(out):
                raise Failed(OUTPUT_SIZE)
            out += stream[b.pos:b.pos + n]
            b.pos += n
            stats["stored_blocks"] += 1
        else:
            lit, dist = _fixed() if kind == 1 else _dynamic(b)
            while True:
                sym = _symbol(b, lit)
                if sym < 256:
                    if len(out) >= expect:
                        raise Failed(OUTPUT_SIZE)
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                if sym > 285:
                    raise Failed(BAD_SYMBOL)
                n = LENGTH_BASE[sym - 257] + b.take(LENGTH_EXTRA[sym - 257])
                dsym = _symbol(b, dist)
                if dsym > 29:
                    raise Failed(BAD_SYMBOL)
                d = DIST_BASE[dsym] + b.take(DIST_EXTRA[dsym])
                if d > len(out):
                    raise Failed(FAR_DISTANCE)
                if n > expect - len(out):
                    raise Failed(OUTPUT_SIZE)
                stats["max_distance"] = max(stats["max_distance"], d)
                stats["max_length"] = max(stats["max_length"], n)
                if d >= n:
                    at = len(out) - d
                    out += out[at:at + n]
                else:
                    stats["overlap"] = True
                    piece = bytes(out[-d:])
                    out += (piece * (n // d + 1))[:n]
        if last:
            break
    if len(out) != expect:
        raise Failed(OUTPUT_SIZE)
    b.to_byte_boundary()
    want = 0
    for _ in range(4):
        want = want << 8 | b.take(8)
    s1, s2 = 1, 0
    for i in range(0, len(out), 4096):              # (RFC 1950, 8.2, by pieces short enough for exact int64 sums)
        piece = np.frombuffer(out, np.uint8, min(4096, len(out) - i), i).astype(np.int64)
        s2 = (s2 + len(piece) * s1 + int((piece * np.arange(len(piece), 0, -1)).sum())) % 65521
        s1 = (s1 + int(piece.sum())) % 65521
    if (s2 << 16 | s1) != want:
        raise Failed(BAD_ADLER)
    return bytes(out)


def unfilter(rows, H, W, bpp, stats=None):
    """(H, W, bpp) uint8 from the H * (1 + W * bpp) filtered bytes (PNG specification, 9.2), or Failed(BAD_FILTER)"""
    stats = new_stats() if stats is None else stats
    rowb = W * bpp
    data = np.frombuffer(rows, np.uint8).reshape(H, 1 + rowb)
    if (data[:, 0] > 4).any():
        raise Failed(BAD_FILTER)
    out = np.zeros((H, rowb), np.uint8)
    above = np.zeros(rowb, np.int64)
    for r in range(H):
        ft, x = int(data[r, 0]), data[r, 1:].astype(np.int64)
        stats["filters"].add(ft)
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + above) & 255
        elif ft == 1:
            cur = x.copy()
            for c in range(bpp):                    # a running sum per channel
                cur[c::bpp] = np.cumsum(x[c::bpp]) & 255
        else:
            cur = np.zeros(rowb, np.int64)
            xs, ab = x.tolist(), above.tolist()
            res = [0] * rowb
            for i in range(rowb):
                a = res[i - bpp] if i >= bpp else 0
                b = ab[i]
                if ft == 3:
                    p = (a + b) >> 1
                else:
                    c = ab[i - bpp] if i >= bpp else 0
                    est = a + b - c
                    pa, pb, pc = abs(est - a), abs(est - b), abs(est - c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                res[i] = (xs[i] + p) & 255
            cur[:] = res
        out[r] = cur
        above = cur
    return out.reshape(H, W, bpp)


# ---------------------------------------------------------------------------------------------------------- the container
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def parse(data):
    """dict(W, H, bpp, colour, palette, stream, idat) of a non-interlaced 8-bit PNG file; ValueError for anything else"""
    if data[:8] != SIGNATURE:
        raise ValueError("signature")
    pos, head, palette, idat, ended = 8, None, None, [], False
    while pos < len(data) and not ended:
        if pos + 8 > len(data):
            raise ValueError("chunk header cut")
        n, kind = struct.unpack_from(">I4s", data, pos)
        if pos + 12 + n > len(data):
            raise ValueError("chunk cut")
        body = data[pos + 8:pos + 8 + n]
        crc_ok = struct.unpack_from(">I", data, pos + 8 + n)[0] == zlib.crc32(kind + body) & 0xffffffff
        pos += 12 + n
        critical = not kind[0] & 32
        if critical and not crc_ok:
            raise ValueError("crc")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        elif critical:
            raise ValueError("unknown critical chunk")
    if head is None or not idat or not ended:
        raise ValueError("IHDR, IDAT or IEND missing")
    W, H, depth, colour, _, _, interlace = head
    if depth != 8 or interlace or colour not in BPP:
        raise ValueError("out of scope")
    return dict(W=W, H=H, bpp=BPP[colour], colour=colour, palette=palette, stream=b"".join(idat), idat=len(idat))


def decode_stream(stream, H, W, bpp, stats=None):
    """((H, W, bpp) uint8 -- zeros with a non-zero status --, status) of one zlib stream"""
    try:
        return unfilter(inflate(stream, H * (1 + W * bpp), stats), H, W, bpp, stats), OK
    except Failed as e:
        return np.zeros((H, W, bpp), np.uint8), e.status


def decode(data, stats=None):
    """((H, W, bpp) uint8, status, stats) of a PNG file"""
    stats = new_stats() if stats is None else stats
    p = parse(data)
    stats["idat"] = max(stats["idat"], p["idat"])
    pixels, status = decode_stream(p["stream"], p["H"], p["W"], p["bpp"], stats)
    return pixels, status, stats


def zlib_accepts(stream, H, W, bpp):
    """zlib's own verdict on a stream, with the PNG layer's: does it inflate to the end, to the right size, with filter
    types 0 .. 4?"""
    d = zlib.decompressobj()
    try:
        rows = d.decompress(bytes(stream))
    except zlib.error:
        return False
    if not d.eof or len(rows) != H * (1 + W * bpp):
        return False
    return not (np.frombuffer(rows, np.uint8).reshape(H, -1)[:, 0] > 4).any()
