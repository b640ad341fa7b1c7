"""A numpy restatement of the baseline JPEG decoder (include/gflow_hip.h, "video files": Decoding), written from ITU-T T.81 and
from the arithmetic libjpeg's default path is known by: a parser, an entropy decoder on Python integers (T.81 F.2.2: DECODE,
RECEIVE, EXTEND, one bit at a time), the slow-integer inverse DCT, triangle ("fancy") upsampling and the 16-bit fixed-point
colour transform, vectorised.  It shares nothing with the product but ``gflow_amd.video.ZIGZAG``.

``decode(data)`` is what ``np.asarray(PIL.Image.open(...))`` gives, bit for bit (tests/test_jpeg_dec_host.py holds it to
that).  On damaged data it follows the contract the header states for a unit (a restart interval): the reader supplies
1-bits behind the unit's bytes, a unit stops at its first error with a status code, a block counts only once it is decoded
whole, the blocks behind stay zero -- so the host harness and the device can be held to it on malformed files too."""
import struct

import numpy as np

from gflow_amd.video import ZIGZAG

OK, BAD_RECORD, NO_CODE, INDEX, SHORT, LEFT_OVER, SYMBOL = 0, 1, 2, 3, 4, 5, 6


# --------------------------------------------------------------------------------------------------------------- parser
def parse(data):
    """dict(W, H, comps [(id, h, v, tq)], quant {id: 64 ints, natural order}, huff {(class, id): (bits, vals)}, dri, sel
    [(td, ta)], scan (start, end), units [(first MCU, MCU count, offset, bytes)]) of a baseline file with one scan"""
    assert data[:2] == b"\xff\xd8"
    pos, out = 2, dict(quant={}, huff={}, dri=0)
    while True:
        assert data[pos] == 0xFF, pos
        m = data[pos + 1]
        n = struct.unpack_from(">H", data, pos + 2)[0]
        seg = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m == 0xC0:
            out["H"], out["W"] = struct.unpack_from(">HH", seg, 1)
            out["comps"] = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xDB:
            for at in range(0, len(seg), 65):
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = seg[at + 1 + k]
                out["quant"][seg[at] & 15] = nat
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                bits = list(seg[at + 1:at + 17])
                out["huff"][(seg[at] >> 4, seg[at] & 15)] = (bits, list(seg[at + 17:at + 17 + sum(bits)]))
                at += 17 + sum(bits)
        elif m == 0xDD:
            out["dri"] = struct.unpack(">H", seg)[0]
        elif m == 0xDA:
            out["sel"] = [(seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15) for c in range(seg[0])]
            break
    hs, vs = out["comps"][0][1], out["comps"][0][2]
    out["mx"], out["my"] = -(-out["W"] // (8 * hs)), -(-out["H"] // (8 * vs))
    n_mcu = out["mx"] * out["my"]
    # the scan, byte by byte: it ends at the first marker that is not RSTm; the units lie between the RSTm
    i, start, cuts = pos, pos, []
    while i < len(data):
        if data[i] == 0xFF and i + 1 < len(data) and data[i + 1] != 0:
            if 0xD0 <= data[i + 1] <= 0xD7:
                cuts.append(i)
                i += 2
                continue
            break
        i += 1
    end = i
    out["scan"] = (start, end)
    ri = out["dri"] or n_mcu
    bounds = [start] + [c + 2 for c in cuts]
    ends = cuts + [end]
    out["units"] = []
    for k in range(-(-n_mcu // ri)):
        a, b = (bounds[k], ends[k]) if k < len(bounds) else (end, end)
        out["units"].append((k * ri, min(ri, n_mcu - k * ri), a, b - a))
    return out


# ------------------------------------------------------------------------------------------------------ entropy decoding
class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def huff_table(bits, vals):
    """T.81 figures C.1, C.2, F.15: (maxcode, valptr, mincode) [1 .. 16] and the 256 values"""
    maxcode, valptr, mincode = [-1] * 17, [0] * 17, [0] * 17
    code = k = 0
    for l in range(1, 17):
        n = bits[l - 1]
        valptr[l], mincode[l] = k, code
        maxcode[l] = code + n - 1 if n else -1
        code = (code + n) << 1
        k += n
    return maxcode, valptr, mincode, list(vals) + [0] * (256 - len(vals))


class _Bits:
    """the unit's bits: stuffing removed, ended by a marker (whose FF still counts); behind them, 1-bits"""

    def __init__(self, data):
        raw, i = bytearray(), 0
        while i < len(data):
            raw.append(data[i])
            i += 1
            if raw[-1] == 0xFF:
                if i < len(data) and data[i] == 0:
                    i += 1
                else:
                    break
        self.s = "".join(f"{b:08b}" for b in raw)
        self.pos = 0

    def bit(self):
        b = int(self.s[self.pos]) if self.pos < len(self.s) else 1
        self.pos += 1
        return b

    def receive(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def decode(self, table):
        maxcode, valptr, mincode, vals = table
        code, l = self.bit(), 1
        while code > maxcode[l]:
            l += 1
            if l > 16:
                raise _Stop(NO_CODE)
            code = (code << 1) | self.bit()
        j = valptr[l] + code - mincode[l]
        if not 0 <= j <= 255:
            raise _Stop(SYMBOL)
        return vals[j]


def _extend(v, t):
    return 0 if t == 0 else (v - (1 << t) + 1 if v < (1 << (t - 1)) else v)


def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _block(br, dc, ac, pred):
    blk = [0] * 64
    t = br.decode(dc)
    if t > 15:
        raise _Stop(SYMBOL)
    pred = _wrap(pred + _extend(br.receive(t), t), 32)
    blk[0] = _wrap(pred, 16)
    k = 1
    while k < 64:
        rs = br.decode(ac)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 15
            if k > 63:
                raise _Stop(INDEX)
            k += 1
            continue
        k += r
        if k > 63:
            raise _Stop(INDEX)
        blk[ZIGZAG[k]] = _wrap(_extend(br.receive(s), s), 16)
        k += 1
    if br.pos > len(br.s):
        raise _Stop(SHORT)
    return blk, pred


def decode_units(data, units, comps, sel, huff, mx, my):
    """(coefficient planes per component [(bh, bw, 64) int16], status per unit).  ``units``: (first MCU, count, offset, bytes)
    into ``data``; ``huff``: {(class, id): (bits, vals)}."""
    hmax, vmax = comps[0][1], comps[0][2]
    planes = [np.zeros((my * v, mx * h, 64), dtype=np.int16) for _, h, v, _ in comps]
    tabs = {k: huff_table(*v) for k, v in huff.items()}
    status = []
    for first, count, off, nb in units:
        if first < 0 or count < 1 or first + count > mx * my or nb < 0 or off < 0 or off + nb > len(data):
            status.append(BAD_RECORD)
            continue
        br = _Bits(data[off:off + nb])
        pred = [0] * len(comps)
        try:
            for m in range(first, first + count):
                row, col = divmod(m, mx)
                for c, (_, h, v, _) in enumerate(comps):
                    for j in range(v):
                        for i in range(h):
                            blk, pred[c] = _block(br, tabs[(0, sel[c][0])], tabs[(1, sel[c][1])], pred[c])
                            planes[c][row * v + j, col * h + i] = blk
            rest = br.s[br.pos:]
            status.append(OK if len(rest) < 8 and set(rest) <= {"1"} else LEFT_OVER)
        except _Stop as e:
            status.append(e.status)
    return planes, status


# ------------------------------------------------------------------------------------------------------- block arithmetic
def _i32(x):
    return np.asarray(x).astype(np.int64).astype(np.int32)


def _pass(v, shift):
    """one pass of the butterfly along axis 0 of v (8, ...), int32 with its wrap-around"""
    with np.errstate(over="ignore"):
        v = [_i32(x) for x in v]
        c = lambda k: np.int32(k)
        z1 = (v[2] + v[6]) * c(4433)
        t2 = z1 - v[6] * c(15137)
        t3 = z1 + v[2] * c(6270)
        t0 = (v[0] + v[4]) << c(13)
        t1 = (v[0] - v[4]) << c(13)
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a, b, cc, d = v[7], v[5], v[3], v[1]
        z5 = (a + cc + b + d) * c(9633)
        z1 = -(a + d) * c(7373)
        z2 = -(b + cc) * c(20995)
        z3 = -(a + cc) * c(16069) + z5
        z4 = -(b + d) * c(3196) + z5
        a = a * c(2446) + z1 + z3
        b = b * c(16819) + z2 + z4
        cc = cc * c(25172) + z2 + z3
        d = d * c(12299) + z1 + z4
        outs = [t10 + d, t11 + cc, t12 + b, t13 + a, t13 - a, t12 - b, t11 - cc, t10 - d]
        return [(o + c(1 << (shift - 1))) >> c(shift) for o in outs]


def idct_plane(coef, q):
    """(bh, bw, 64) int16 coefficients, 64 quantisers (natural order) -> (bh * 8, bw * 8) uint8"""
    bh, bw, _ = coef.shape
    x = (coef.astype(np.int32) * np.asarray(q, dtype=np.int32)).reshape(bh, bw, 8, 8)
    cols = np.stack(_pass([x[:, :, k, :] for k in range(8)], 11), axis=2)                # along each column
    rows = np.stack(_pass([cols[:, :, :, k] for k in range(8)], 18), axis=3)             # along each row
    with np.errstate(over="ignore"):
        px = np.clip(rows + np.int32(128), 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample(p, hs, vs, H, W):
    """a chroma plane cropped to its real size -> (H, W) int32 by the triangle filter"""
    ch, cw = -(-H // vs), -(-W // hs)
    p = p[:ch, :cw].astype(np.int32)
    if hs == 1:
        return p
    if vs == 1:
        left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
        right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
        even, odd = (3 * p + left + 1) >> 2, (3 * p + right + 2) >> 2
        even[:, 0], odd[:, -1] = p[:, 0], p[:, -1]
        return np.stack([even, odd], axis=2).reshape(ch, 2 * cw)[:, :W]
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    rows = []
    for other in (up, down):
        s = 3 * p + other
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        rows.append(np.stack([even, odd], axis=2).reshape(ch, 2 * cw))
    return np.stack(rows, axis=1).reshape(2 * ch, 2 * cw)[:H, :W]


def ycc_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(planes, comps, quant, H, W):
    """coefficient planes -> (H, W, 3) or (H, W) uint8"""
    hs, vs = comps[0][1], comps[0][2]
    px = [idct_plane(planes[c], quant[tq]) for c, (_, _, _, tq) in enumerate(comps)]
    if len(comps) == 1:
        return px[0][:H, :W]
    return ycc_rgb(px[0][:H, :W], upsample(px[1], hs, vs, H, W), upsample(px[2], hs, vs, H, W))


def decode_parsed(data, p, units=None, huff=None):
    planes, status = decode_units(data, p["units"] if units is None else units, p["comps"], p["sel"],
                                  p["huff"] if huff is None else huff, p["mx"], p["my"])
    return pixels(planes, p["comps"], p["quant"], p["H"], p["W"]), status, planes


def decode(data):
    """the image of a whole, well-formed file"""
    image, status, _ = decode_parsed(data, parse(data))
    assert not any(status), status
    return image
