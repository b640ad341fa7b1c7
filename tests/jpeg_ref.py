"""A restatement of the baseline JPEG the library codes (include/gflow_hip.h, "video files"), written from ITU-T T.81: the
transform in float64, the entropy coder in Python integers, and a scan DECODER back to quantised coefficients.  It shares
the tables with gflow_amd.video (which a CPU test pins to the segments PIL writes) and nothing else.  Slow and plain: for tests.

Coefficients are (n_mcu, C, 64) integers, MCUs in scan order, 64 in zigzag order."""
import numpy as np

from gflow_amd.video import HUFFMAN, ZIGZAG, quant_tables

# T.81 A.3.3: D[u][x] = C(u) / 2 cos((2 x + 1) u pi / 16)
_D = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2.0 * np.cos((2 * x + 1) * u * np.pi / 16.0) for x in range(8)]
               for u in range(8)])
_ZZ = np.array(ZIGZAG)


def huffman_codes(cls, tid):
    """symbol -> (code, length) of table (class, id): T.81 annex C"""
    bits, vals = HUFFMAN[(cls, tid)]
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


_CODES = {key: huffman_codes(*key) for key in HUFFMAN}
_DECODE = {key: {(l, c): s for s, (c, l) in tab.items()} for key, tab in _CODES.items()}


def _planes(img):
    """(C, H, W) float64, level shifted: JFIF's YCbCr of (H, W, 3), or the grey plane of (H, W)"""
    a = np.asarray(img).astype(np.float64)
    if a.ndim == 2:
        return (a - 128.0)[None]
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    return np.stack([0.299 * r + 0.587 * g + 0.114 * b - 128.0,
                     -0.168736 * r - 0.331264 * g + 0.5 * b,
                     0.5 * r - 0.418688 * g - 0.081312 * b])


def ratios(img, quality):
    """F / q before rounding: (n_mcu, C, 64) float64, zigzag.  Blocks over the edge repeat the last column / row."""
    p = _planes(img)
    C, H, W = p.shape
    my, mx = (H + 7) // 8, (W + 7) // 8
    p = np.pad(p, ((0, 0), (0, my * 8 - H), (0, mx * 8 - W)), mode="edge")
    blocks = p.reshape(C, my, 8, mx, 8).transpose(1, 3, 0, 2, 4).reshape(my * mx, C, 8, 8)
    F = _D @ blocks @ _D.T
    qt = quant_tables(quality).astype(np.float64).reshape(2, 8, 8)
    q = np.stack([qt[0 if c == 0 else 1] for c in range(C)])
    return (F / q).reshape(my * mx, C, 64)[..., _ZZ]


def quantise(r):
    """round half away from zero"""
    return (np.sign(r) * np.floor(np.abs(r) + 0.5)).astype(np.int64)


def coefficients(img, quality):
    return quantise(ratios(img, quality))


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length

    def bytes(self):
        """padded with 1-bits to a byte, FF stuffed"""
        pad = -self.n % 8
        acc = (self.acc << pad) | ((1 << pad) - 1)
        raw = acc.to_bytes((self.n + pad) // 8, "big")
        return raw.replace(b"\xff", b"\xff\x00")


def _category(v):
    return int(abs(int(v))).bit_length()


def _put_value(bits, code, v, cat):
    c, l = code
    bits.put(c, l)
    if cat:
        bits.put((int(v) if v >= 0 else int(v) - 1) & ((1 << cat) - 1), cat)


def entropy_encode(coef, ri):
    """The scan of (n_mcu, C, 64) coefficients: restart intervals of ``ri`` MCUs, RSTm between them (T.81 F.1.2, E.1.4)"""
    coef = np.asarray(coef)
    n, C = coef.shape[:2]
    out = []
    for i, start in enumerate(range(0, n, ri)):
        bits = _Bits()
        pred = [0] * C
        for m in range(start, min(start + ri, n)):
            for c in range(C):
                tid = 0 if c == 0 else 1
                zz = coef[m, c]
                diff = int(zz[0]) - pred[c]
                pred[c] = int(zz[0])
                cat = _category(diff)
                _put_value(bits, _CODES[(0, tid)][cat], diff, cat)
                ac, run = _CODES[(1, tid)], 0
                for k in range(1, 64):
                    v = int(zz[k])
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        bits.put(*ac[0xF0])
                        run -= 16
                    cat = _category(v)
                    _put_value(bits, ac[run << 4 | cat], v, cat)
                    run = 0
                if run:
                    bits.put(*ac[0x00])
        out.append(bits.bytes())
        if start + ri < n:
            out.append(bytes([0xFF, 0xD0 + i % 8]))
    return b"".join(out)


def encode_scan(img, quality, ri):
    return entropy_encode(coefficients(img, quality), ri)


def split_intervals(scan):
    """The scan's intervals with the stuffing removed; checks that the RSTm count 0 .. 7 in order"""
    parts, cur, i, n = [], bytearray(), 0, len(scan)
    while i < n:
        b = scan[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        if i + 1 >= n:
            raise ValueError("scan ends inside a marker")
        nxt = scan[i + 1]
        if nxt == 0x00:
            cur.append(0xFF)
        elif nxt == 0xD0 + len(parts) % 8:
            parts.append(bytes(cur))
            cur = bytearray()
        else:
            raise ValueError(f"unexpected marker FF {nxt:02X} at byte {i} (interval {len(parts)})")
        i += 2
    parts.append(bytes(cur))
    return parts


class _Reader:
    def __init__(self, data):
        self.v, self.left = int.from_bytes(data, "big"), 8 * len(data)

    def take(self, n):
        if n > self.left:
            raise ValueError("interval ends inside a symbol")
        self.left -= n
        return (self.v >> self.left) & ((1 << n) - 1)

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = code << 1 | self.take(1)
            s = table.get((length, code))
            if s is not None:
                return s
        raise ValueError("no such Huffman code")

    def value(self, cat):
        if cat == 0:
            return 0
        v = self.take(cat)
        return v if v >> (cat - 1) else v - (1 << cat) + 1


def decode_scan(scan, n_mcu, C, ri):
    """Quantised coefficients (n_mcu, C, 64) of a scan; checks the interval count, and that what is left of every interval
    is fewer than 8 bits, all ones"""
    parts = split_intervals(scan)
    if len(parts) != (n_mcu + ri - 1) // ri:
        raise ValueError(f"{len(parts)} intervals for {n_mcu} MCUs of {ri}")
    coef = np.zeros((n_mcu, C, 64), dtype=np.int64)
    for i, data in enumerate(parts):
        rd = _Reader(data)
        pred = [0] * C
        for m in range(i * ri, min((i + 1) * ri, n_mcu)):
            for c in range(C):
                tid = 0 if c == 0 else 1
                pred[c] += rd.value(rd.symbol(_DECODE[(0, tid)]))
                coef[m, c, 0] = pred[c]
                k = 1
                while k < 64:
                    s = rd.symbol(_DECODE[(1, tid)])
                    run, cat = s >> 4, s & 15
                    if cat == 0:
                        if run == 15:
                            k += 16
                            continue
                        if run == 0:
                            break
                        raise ValueError(f"symbol {s:02X}")
                    k += run
                    if k > 63:
                        raise ValueError("run past the block")
                    coef[m, c, k] = rd.value(cat)
                    k += 1
        left = rd.left
        if left >= 8 or rd.take(left) != (1 << left) - 1:
            raise ValueError(f"interval {i}: padding")
    return coef


def n_mcus(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


def scan_of(jpeg_bytes):
    """the entropy-coded bytes of a complete file: between the SOS segment and the trailing EOI"""
    at = 2 + sum(4 + len(p) for _, p in segments(jpeg_bytes))
    if jpeg_bytes[-2:] != b"\xff\xd9":
        raise ValueError("no EOI")
    return jpeg_bytes[at:-2]


def segments(jpeg_bytes):
    """[(marker, payload)] of the segments in front of the scan"""
    out, at = [], 2
    while True:
        assert jpeg_bytes[at] == 0xFF
        marker = jpeg_bytes[at + 1]
        size = int.from_bytes(jpeg_bytes[at + 2:at + 4], "big")
        out.append((marker, jpeg_bytes[at + 4:at + 2 + size]))
        at += 2 + size
        if marker == 0xDA:
            return out


def tables(jpeg_bytes, marker):
    """{table id byte: table bytes} of all DQT (0xDB) or DHT (0xC4) segments, a segment with several tables split up"""
    out = {}
    for m, p in segments(jpeg_bytes):
        if m != marker:
            continue
        at = 0
        while at < len(p):
            if marker == 0xDB:
                size = 1 + (128 if p[at] >> 4 else 64)
            else:
                size = 17 + sum(p[at + 1:at + 17])
            out[p[at]] = bytes(p[at:at + size])
            at += size
    return out
