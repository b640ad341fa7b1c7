"""Video files: baseline JPEG coded on the device, and a Motion-JPEG AVI around it ("Video files").

The reference's deliverables are videos (fit_video.py:357-392 writes its renders and the trajectory visualiser's overlays as
.mp4 through imageio / ffmpeg).  Neither is needed for a file a player opens: a Motion-JPEG AVI is a RIFF container around
whole JPEG images.  The images this project makes -- renders, track overlays, masks, the viewer's paths -- are (T, H, W, 3)
uint8 stacks ON THE DEVICE, and the two library calls gfl_jpeg_sizes / gfl_jpeg_emit (csrc/gfl_jpeg.hip; the format is written
out in include/gflow_hip.h, "video files") turn a whole stack into the entropy-coded scans there.  The host adds the header
(``jpeg_header``: pure Python) and writes bytes:

    frames = encode_jpeg(images, quality=90)          # list of complete .jpg files, as bytes
    write_avi("clip.avi", images, fps=5)              # the same, streamed into an AVI in stacks of `chunk` frames
    read_avi("clip.avi")                              # dict(width, height, fps, frames=[bytes]) -- for users without a player

    python -m gflow_amd.video --frames DIR --out FILE.avi [--fps 5] [--quality 90] [--gpu 0]

The way back ("Decoding video files") is gfl_jpeg_decode (csrc/gfl_jpeg_dec.hip over csrc/gfl_jpeg_dec.hpp): the
host parses the headers and finds the restart intervals (``parse_jpeg``: pure Python and numpy), the device decodes a whole
stack, with the bits ``PIL.Image.open`` gives for the same files:

    parse_jpeg(data)                                  # dict: size, sampling, tables, DRI, the scan's bytes, the units
    images = decode_jpeg(files)                       # list of .jpg files as bytes -> (T, H, W, C) uint8 on the device
    images = read_avi_frames("clip.avi")              # read_avi + decode_jpeg, in stacks of `chunk` frames

    python -m gflow_amd.video --unpack FILE.avi --out DIR [--gpu 0]        # the frames as PNG files

The AVI writer and reader, ``jpeg_header`` and ``parse_jpeg`` need no device; ``encode_jpeg`` and ``decode_jpeg`` have no CPU
path.
"""
import argparse
import ctypes
import os
import struct

import numpy as np
import torch

from . import _lib as L

# ---- ITU-T T.81 Annex K: the quantisation tables (K.1, K.2; natural order) and the Huffman tables (K.3 - K.6) as BITS / HUFFVAL
_Q_LUM = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
          80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
          95, 98, 112, 100, 103, 99)
_Q_CHR = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
          99, 99) + (99,) * 32
HUFFMAN = {                                                                # (class, id) -> (BITS[16], HUFFVAL)
    (0, 0): ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0, 1): ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (1, 0): ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), tuple(bytes.fromhex(
        "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
        "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
        "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))),
    (1, 1): ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(bytes.fromhex(
        "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
        "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
        "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))),
}
# ZIGZAG[k] = natural index (row * 8 + column) of the k-th coefficient in zigzag order (T.81 figure A.6)
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
EOI = b"\xff\xd9"


def restart_interval():
    """MCUs per restart interval of the library's scans (gfl_jpeg_restart_interval; needs no device)"""
    return int(L.load().gfl_jpeg_restart_interval())


def quant_tables(quality):
    """(luminance, chrominance): Annex K's tables scaled by the IJG rule for ``quality`` in 1 .. 100 (50 = the tables
    themselves), entries clipped to 1 .. 255 -- what libjpeg's jpeg_set_quality(force_baseline) gives.  (2, 64) uint16,
    natural order."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"gflow_amd.video: quality {quality!r}: an integer in 1 .. 100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([[min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (_Q_LUM, _Q_CHR)], dtype=np.uint16)


def _segment(marker, payload):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_header(W, H, C, quality, ri=None):
    """Everything of a baseline JPEG file in front of the scan: SOI, JFIF APP0, DQT, SOF0, the standard DHTs, DRI, SOS.
    ``C`` = 3: YCbCr 4:4:4, components 1, 2, 3; ``C`` = 1: one grey component.  One table per DQT / DHT segment, in libjpeg's
    order.  ``ri``: the restart interval in MCUs, the library's by default."""
    W, H, C = int(W), int(H), int(C)
    if C not in (1, 3) or not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f"gflow_amd.video: a JPEG of {W}x{H} with {C} components")
    ri = restart_interval() if ri is None else int(ri)
    qt = quant_tables(quality)
    ids = (0, 1) if C == 3 else (0,)
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0]) + struct.pack(">HH", 1, 1) + bytes([0, 0]))]
    for i in ids:
        out.append(_segment(0xDB, bytes([i]) + bytes(int(qt[i][n]) for n in ZIGZAG)))
    comps = [(1, 0)] if C == 1 else [(1, 0), (2, 1), (3, 1)]                           # (component id, table id)
    out.append(_segment(0xC0, bytes([8]) + struct.pack(">HH", H, W) + bytes([C]) + b"".join(bytes([c, 0x11, t]) for c, t in comps)))
    for i in ids:
        for cls in (0, 1):
            bits, vals = HUFFMAN[(cls, i)]
            out.append(_segment(0xC4, bytes([cls << 4 | i]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack(">H", ri)))
    out.append(_segment(0xDA, bytes([C]) + b"".join(bytes([c, t << 4 | t]) for c, t in comps) + bytes([0, 63, 0])))
    return b"".join(out)


def _tensor(images):
    if isinstance(images, np.ndarray) and not images.flags.writeable:
        images = images.copy()                     # (torch refuses to wrap a read-only array quietly)
    return torch.as_tensor(images)


def _as_images(images):
    """(T, H, W, C) uint8 on a HIP device, C = 1 or 3, from (T, H, W, 3) or (T, H, W)"""
    t = _tensor(images)
    if t.dtype != torch.uint8 or not (t.dim() == 3 or (t.dim() == 4 and t.shape[-1] == 3)):
        raise ValueError(f"gflow_amd.video: images must be (T, H, W, 3) or (T, H, W) uint8, got {tuple(t.shape)} {t.dtype}")
    if not t.is_cuda and torch.cuda.is_available():
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    L.need_device(t)
    return (t if t.dim() == 4 else t.unsqueeze(-1)).contiguous()


def encode_scans(images, quality=90):
    """The library's two calls on one stack: (scan bytes of all frames as one host uint8 array, the T + 1 frame offsets).
    ``images``: (T, H, W, C) uint8 on the device.  One read of the offsets between the passes, one copy of the bytes."""
    T, H, W, C = (int(v) for v in images.shape)
    lib = L.load()
    dev = images.device
    need = lib.gfl_jpeg_workspace_bytes(T, C, W, H)
    if need == 0:
        raise ValueError(f"gflow_amd.video: unsupported stack T={T} H={H} W={W} C={C} (sides up to 65535, at least one frame)")
    with torch.cuda.device(dev):
        qt = torch.from_numpy(quant_tables(quality).astype(np.int16)).to(dev)        # (the bits of the uint16 table)
        ws = L.scratch(need, dev)
        offsets = torch.empty(T + 1, dtype=torch.int64, device=dev)
        L.check(lib.gfl_jpeg_sizes(L.ptr(images), T, C, W, H, L.ptr(qt), L.ptr(offsets), L.ptr(ws), ws.numel(), L.stream()),
                "jpeg sizes")
        off = offsets.cpu().numpy()
        out = torch.empty(int(off[T]), dtype=torch.uint8, device=dev)
        L.check(lib.gfl_jpeg_emit(L.ptr(images), T, C, W, H, L.ptr(qt), L.ptr(out), out.numel(), L.ptr(ws), ws.numel(),
                                  L.stream()), "jpeg emit")
        return out.cpu().numpy(), off


def encode_jpeg(images, quality=90):
    """``images`` -- (T, H, W, 3) or (T, H, W) uint8; a device tensor, a host tensor or an array (host input is moved to the
    current HIP device; without one this raises: there is no CPU path) -- as T complete baseline JPEG files: a list of bytes,
    each header + scan + EOI.  RGB becomes YCbCr 4:4:4, a (T, H, W) stack one grey component."""
    images = _as_images(images)
    T, H, W, C = (int(v) for v in images.shape)
    if T == 0:
        return []
    head = jpeg_header(W, H, C, quality)
    data, off = encode_scans(images, quality)
    return [head + data[off[t]:off[t + 1]].tobytes() + EOI for t in range(T)]


# ------------------------------------------------------------------------------------------------------------- decoding
# the mirrors of gfl_jpeg_unit and gfl_jpeg_frame_tables (include/gflow_hip.h states the layout; _check_mirrors the sizes)
UNIT_DTYPE = np.dtype([("frame", "<i4"), ("first_mcu", "<i4"), ("n_mcu", "<i4"), ("n_bytes", "<i4"), ("offset", "<i8")])
TABLES_DTYPE = np.dtype([("q", "u1", (4, 64)), ("qsel", "u1", 4), ("dcsel", "u1", 4), ("acsel", "u1", 4), ("first_unit", "<i4"),
                         ("n_units", "<i4"), ("huff", [("bits", "u1", 16), ("vals", "u1", 256)], 4)])
UNIT_STATUS = {1: "the unit record is out of range", 2: "a code that matches no Huffman code", 3: "a coefficient index past 63",
               4: "the data ended early", 5: "data left behind the last MCU", 6: "a symbol out of range", -1: "never run"}
_SOF_NAMES = {0xC1: "extended sequential coding", 0xC2: "progressive coding", 0xC3: "lossless coding"}
_mirrors_checked = False


def _check_mirrors(lib):
    global _mirrors_checked
    if not _mirrors_checked:
        a, b = ctypes.c_int(), ctypes.c_int()
        L.check(lib.gfl_jpeg_decode_struct_bytes(ctypes.byref(a), ctypes.byref(b)), "jpeg decode struct sizes")
        if (a.value, b.value) != (UNIT_DTYPE.itemsize, TABLES_DTYPE.itemsize):
            raise RuntimeError(f"gflow_amd.video: the library's gfl_jpeg_unit / gfl_jpeg_frame_tables are {a.value} / {b.value} "
                               f"bytes, the binding's {UNIT_DTYPE.itemsize} / {TABLES_DTYPE.itemsize}: rebuild the library")
        _mirrors_checked = True


def parse_jpeg(data, name="JPEG data"):
    """The headers of one baseline JPEG file (``data``: bytes) and where its entropy-coded data lies; no device, nothing is
    decoded.  Returns dict(width, height, components, hs, vs -- the luminance sampling; sampling, component_ids, qsel, dcsel,
    acsel -- per component; quant -- {id: (64,) uint8, natural order}; huffman -- {(class, id): (BITS[16], HUFFVAL)}; dri;
    jfif, adobe_transform; scan -- (start, end) of the entropy-coded bytes in ``data``; mcus -- (per row, per column);
    units -- (n, 4) int64 rows (first MCU, MCU count, byte offset in ``data``, byte count), one per restart interval).
    Raises ValueError, naming ``name``, for everything gfl_jpeg_decode does not take: anything but SOF0 with 8-bit samples and
    8-bit quantisers, one interleaved scan of 1 component or of 3 that libjpeg reads as YCbCr with chroma 1x1 and luminance
    1x1, 2x1 or 2x2 -- and for restart markers that do not count 0 .. 7 in order."""
    def refuse(why):
        raise ValueError(f"gflow_amd.video: {name}: {why}")

    data = bytes(data)
    n = len(data)
    if n < 4 or data[:2] != b"\xff\xd8":
        refuse("not a JPEG file (no SOI)")
    pos, quant, huff, dri, sof, jfif, adobe, sos = 2, {}, {}, 0, None, False, None, None
    while sos is None:
        if pos + 2 > n:
            refuse("no scan (the file ends inside its headers)")
        if data[pos] != 0xFF:
            refuse(f"byte {pos} is not a marker")
        while pos < n and data[pos] == 0xFF:                   # (fill bytes may precede a marker)
            pos += 1
        if pos >= n:
            refuse("no scan (the file ends inside its headers)")
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            refuse("no scan (EOI after the headers)")
        if pos + 2 > n:
            refuse("no scan (the file ends inside its headers)")
        length = struct.unpack_from(">H", data, pos)[0]
        if length < 2 or pos + length > n:
            refuse(f"the segment of marker FF{m:02X} runs past the end of the file")
        seg = data[pos + 2:pos + length]
        pos += length
        if m == 0xC0:
            if sof is not None:
                refuse("two frame headers")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                refuse("a frame header of the wrong length")
            P, H, W, nf = seg[0], *struct.unpack_from(">HH", seg, 1), seg[5]
            if P != 8:
                refuse(f"{P}-bit samples (8-bit only)")
            if nf not in (1, 3):
                refuse(f"{nf} components (1 or 3 only)")
            if W < 1 or H < 1:
                refuse(f"a frame of {W}x{H} (the height in a DNL segment is not supported)")
            sof = dict(W=W, H=H, comps=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nf)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            refuse("arithmetic coding" if m >= 0xC9 else _SOF_NAMES.get(m, f"differential coding (SOF{m - 0xC0})") + " (baseline SOF0 only)")
        elif m == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    refuse("a 16-bit quantisation table (8-bit only)")
                if tq > 3 or at + 65 > len(seg):
                    refuse("a malformed DQT segment")
                nat = np.zeros(64, dtype=np.uint8)
                nat[list(ZIGZAG)] = np.frombuffer(seg, dtype=np.uint8, count=64, offset=at + 1)
                quant[tq] = nat
                at += 65
        elif m == 0xC4:
            at = 0
            while at < len(seg):
                tc, th = seg[at] >> 4, seg[at] & 15
                if tc > 1 or th > 1 or at + 17 > len(seg):
                    refuse("a Huffman table with class or id above 1, or a malformed DHT segment (baseline: ids 0 and 1)")
                bits = tuple(seg[at + 1:at + 17])
                if sum(bits) > 256 or at + 17 + sum(bits) > len(seg):
                    refuse("a malformed DHT segment")
                huff[(tc, th)] = (bits, bytes(seg[at + 17:at + 17 + sum(bits)]))
                at += 17 + sum(bits)
        elif m == 0xDD:
            if len(seg) != 2:
                refuse("a malformed DRI segment")
            dri = struct.unpack(">H", seg)[0]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            if sof is None:
                refuse("a scan before the frame header")
            sos = seg
    comps = sof["comps"]
    C, W, H = len(comps), sof["W"], sof["H"]
    if len(sos) < 1 or len(sos) != 4 + 2 * sos[0]:
        refuse("a scan header of the wrong length")
    if sos[0] != C:
        refuse(f"a scan of {sos[0]} of the {C} components (several scans; one interleaved scan only)")
    if [sos[1 + 2 * c] for c in range(C)] != [cid for cid, _, _, _ in comps]:
        refuse("the scan lists the components in another order than the frame")
    if tuple(sos[1 + 2 * C:]) != (0, 63, 0):
        refuse("a scan that is not the whole spectrum at full precision (progressive parameters)")
    dcsel, acsel = [sos[2 + 2 * c] >> 4 for c in range(C)], [sos[2 + 2 * c] & 15 for c in range(C)]
    sampling = [(h, v) for _, h, v, _ in comps]
    if C == 1 and sampling[0] != (1, 1):
        refuse(f"a single component sampled {sampling[0][0]}x{sampling[0][1]} (1x1 only)")
    if C == 3 and (sampling[1] != (1, 1) or sampling[2] != (1, 1) or sampling[0] not in ((1, 1), (2, 1), (2, 2))):
        refuse("sampling factors " + ", ".join(f"{h}x{v}" for h, v in sampling) + " (chroma 1x1 with luminance 1x1, 2x1 or 2x2 only)")
    if C == 3:
        if adobe is not None and adobe != 1:
            refuse(f"an Adobe APP14 marker with transform {adobe}: not YCbCr")
        if adobe is None and not jfif and bytes(cid for cid, _, _, _ in comps) == b"RGB":
            refuse("components R, G, B without JFIF: libjpeg reads them as RGB, not YCbCr")
    for c, (_, _, _, tq) in enumerate(comps):
        if tq not in quant or dcsel[c] > 1 or acsel[c] > 1 or (0, dcsel[c]) not in huff or (1, acsel[c]) not in huff:
            refuse(f"component {c} uses a table the file does not define")
    hs, vs = sampling[0]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    # the scan: up to the first marker that is neither a stuffed FF nor RSTm -- EOI in a whole file
    a = np.frombuffer(data, dtype=np.uint8)[pos:]
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, dtype=np.int64)
    nxt = a[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    other = ff[(nxt != 0) & ~is_rst]
    end = int(other[0]) if other.size else int(a.size)
    if other.size and a[end + 1] != 0xD9:
        refuse("fill bytes inside the scan" if a[end + 1] == 0xFF else
               f"marker FF{a[end + 1]:02X} after the scan (several scans or tables between them)")
    rst = ff[is_rst]
    rst = rst[rst < end]
    n_mcu = mx * my
    if dri == 0:
        if rst.size:
            refuse("restart markers in a file without DRI")
        units = np.array([[0, n_mcu, pos, end]], dtype=np.int64)
    else:
        n_int = -(-n_mcu // dri)
        if rst.size > n_int - 1:
            refuse(f"{rst.size} restart markers for {n_int} restart intervals")
        if not np.array_equal(a[rst + 1].astype(np.int64) - 0xD0, np.arange(rst.size) & 7):
            refuse("restart markers that do not count 0 .. 7 in order")
        starts = np.full(n_int, end, dtype=np.int64)           # (a scan that ends early: the intervals behind are empty)
        ends = np.full(n_int, end, dtype=np.int64)
        starts[0] = 0
        starts[1:rst.size + 1] = rst + 2
        ends[:rst.size] = rst
        first = np.arange(n_int, dtype=np.int64) * dri
        units = np.stack([first, np.minimum(dri, n_mcu - first), pos + starts, ends - starts], axis=1)
    return dict(width=W, height=H, components=C, hs=hs, vs=vs, sampling=sampling, component_ids=[c[0] for c in comps],
                qsel=[c[3] for c in comps], dcsel=dcsel, acsel=acsel, quant=quant, huffman=huff, dri=dri, jfif=jfif,
                adobe_transform=adobe, scan=(pos, pos + end), mcus=(mx, my), units=units)


def decode_arrays(files, parsed):
    """What gfl_jpeg_decode takes, on the host, from ``files`` (bytes each) and their ``parse_jpeg`` results (one shape):
    (units -- UNIT_DTYPE, tables -- TABLES_DTYPE [T], bytes -- every frame's scan, concatenated, uint8)."""
    T = len(files)
    tables = np.zeros(T, dtype=TABLES_DTYPE)
    units, scans, at = [], [], 0
    for t, (data, p) in enumerate(zip(files, parsed)):
        ft = tables[t]
        for i, q in p["quant"].items():
            ft["q"][i] = q
        C = p["components"]
        ft["qsel"][:C], ft["dcsel"][:C], ft["acsel"][:C] = p["qsel"], p["dcsel"], p["acsel"]
        for (cls, i), (bits, vals) in p["huffman"].items():
            ft["huff"][2 * cls + i]["bits"] = bits
            ft["huff"][2 * cls + i]["vals"][:len(vals)] = np.frombuffer(vals, dtype=np.uint8)
        u = np.zeros(len(p["units"]), dtype=UNIT_DTYPE)
        u["frame"], u["first_mcu"], u["n_mcu"], u["n_bytes"] = t, p["units"][:, 0], p["units"][:, 1], p["units"][:, 3]
        u["offset"] = p["units"][:, 2] - p["scan"][0] + at
        ft["first_unit"], ft["n_units"] = sum(len(x) for x in units), len(u)
        units.append(u)
        scans.append(np.frombuffer(data, dtype=np.uint8)[p["scan"][0]:p["scan"][1]])
        at += p["scan"][1] - p["scan"][0]
    return np.concatenate(units), tables, np.concatenate(scans) if scans else np.zeros(0, dtype=np.uint8)


def decode_jpeg(files, device=None, names=None):
    """``files`` -- a list of complete baseline JPEG files as bytes, all of one size, component count and sampling (their
    tables and restart intervals may differ) -- as a (T, H, W, C) uint8 stack on ``device`` (default: the current HIP device;
    without one this raises: there is no CPU path).  C = 3: RGB; C = 1: grey.  The bits are those of
    ``np.asarray(PIL.Image.open(file))``.  One upload, one library call, one read-back of the units' status: a unit that
    went wrong raises ValueError naming its frame (``names[t]`` if given) and unit.  Raises ValueError too for a file
    ``parse_jpeg`` refuses."""
    files = [bytes(f) for f in files]
    T = len(files)
    if device is None and torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device("cpu" if device is None else device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.video: decode_jpeg needs a HIP (cuda) device; there is no CPU fallback")
    if T == 0:
        return torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device)
    label = lambda t: f"frame {t}" + (f" ({names[t]})" if names is not None else "")
    parsed = [parse_jpeg(f, label(t)) for t, f in enumerate(files)]
    key = lambda p: (p["width"], p["height"], p["components"], p["hs"], p["vs"])
    for t, p in enumerate(parsed):
        if key(p) != key(parsed[0]):
            raise ValueError(f"gflow_amd.video: {label(t)} is {key(p)} (width, height, components, sampling), {label(0)} is "
                             f"{key(parsed[0])}: one call decodes one shape")
    W, H, C, hs, vs = key(parsed[0])
    units, tables, data = decode_arrays(files, parsed)
    images, st = decode_stack(units, tables, data, W, H, C, hs, vs, device)
    bad = np.flatnonzero(st)
    if bad.size:
        u = int(bad[0])
        t = int(units["frame"][u])
        raise ValueError(f"gflow_amd.video: {label(t)}, unit {u - int(tables['first_unit'][t])} of {int(tables['n_units'][t])}: "
                         f"{UNIT_STATUS.get(int(st[u]), f'status {int(st[u])}')} ({bad.size} of {len(units)} units of the call "
                         "went wrong)")
    return images


def decode_stack(units, tables, data, W, H, C, hs, vs, device):
    """gfl_jpeg_decode on host arrays (``decode_arrays``): ((T, H, W, C) uint8 on ``device``, the units' status as a host
    int32 array).  One upload, one call, one read-back; nothing is raised for a unit that went wrong."""
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError("gflow_amd.video: decode_stack needs a HIP (cuda) device; there is no CPU fallback")
    T = len(tables)
    units, tables = np.ascontiguousarray(units, dtype=UNIT_DTYPE), np.ascontiguousarray(tables, dtype=TABLES_DTYPE)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    lib = L.load()
    _check_mirrors(lib)
    need = lib.gfl_jpeg_decode_workspace_bytes(T, C, W, H, hs, vs, len(units))
    if need == 0:
        raise ValueError(f"gflow_amd.video: unsupported stack T={T} H={H} W={W} C={C} sampling {hs}x{vs}")
    # ONE upload: the units, the tables and the bytes behind each other, each on a 16-byte boundary
    parts = [units.view(np.uint8).reshape(-1), tables.view(np.uint8).reshape(-1), data]
    offs = np.cumsum([0] + [(len(x) + 15) // 16 * 16 for x in parts])
    host = np.zeros(int(offs[-1]) + 16, dtype=np.uint8)
    for o, x in zip(offs, parts):
        host[o:o + len(x)] = x
    with torch.cuda.device(device):
        blob = torch.from_numpy(host).to(device)
        images = torch.empty((T, H, W, C), dtype=torch.uint8, device=device)
        status = torch.empty(len(units), dtype=torch.int32, device=device)
        ws = L.scratch(need, device)
        at = lambda i: ctypes.c_void_p(blob.data_ptr() + int(offs[i]))
        L.check(lib.gfl_jpeg_decode(at(2), len(data), at(0), len(units), at(1), T, C, W, H, hs, vs, L.ptr(images), L.ptr(status),
                                    L.ptr(ws), ws.numel(), L.stream()), "jpeg decode")
        st = status.cpu().numpy()
    return images, st


# ---------------------------------------------------------------------------------------------------------- the container
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
MAX_FILE = (1 << 31) - 1               # a plain AVI: one RIFF chunk, 32-bit sizes that every reader takes as signed; no OpenDML
_MOVI_LIST = 212                       # where "LIST <size> movi" starts: the headers in front have a fixed size


def _rate_scale(fps):
    fps = float(fps)
    if not fps > 0 or fps != fps or fps == float("inf"):
        raise ValueError(f"gflow_amd.video: fps {fps!r}")
    return (int(fps), 1) if fps == int(fps) else (int(round(fps * 1000)), 1000)


class AviWriter:
    """A Motion-JPEG AVI, streamed to disk: ``add`` appends one complete JPEG image as a ``00dc`` chunk (padded to even
    length), ``close`` writes ``idx1`` (every frame a key frame, offsets relative to the ``movi`` fourcc) and patches the
    sizes and counts in the headers.  Host only.  ``dwRate / dwScale`` is the frame rate: scale 1 for an integer fps, 1000
    otherwise.  A file that would pass 2 GiB - 1 raises ValueError on ``add`` (the file so far stays valid to close)."""

    def __init__(self, path, W, H, fps):
        self.W, self.H = int(W), int(H)
        if self.W < 1 or self.H < 1:
            raise ValueError(f"gflow_amd.video: an AVI of {W}x{H}")
        self.rate, self.scale = _rate_scale(fps)
        self.path = path
        self._index = []               # (offset from the movi fourcc, size) per frame
        self._largest = 0
        self._f = open(path, "wb")
        self._f.write(self._headers(0))
        self._pos = self._f.tell()     # bytes written so far: what the 2 GiB guard counts
        assert self._pos == _MOVI_LIST + 12

    def _headers(self, movi_bytes):
        n = len(self._index)
        usec = int(round(1e6 * self.scale / self.rate))
        per_sec = int(self._largest * self.rate / self.scale)
        avih = struct.pack("<14I", usec, min(per_sec, 0xFFFFFFFF), 0, AVIF_HASINDEX, n, 0, 1, self._largest, self.W, self.H,
                           0, 0, 0, 0)
        strh = (b"vidsMJPG" + struct.pack("<IHHIIIIIIII", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, 0xFFFFFFFF, 0)
                + struct.pack("<4h", 0, 0, self.W, self.H))
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        idx_bytes = 8 + 16 * n
        riff = 4 + 8 + len(hdrl) + 8 + 4 + movi_bytes + idx_bytes
        return (b"RIFF" + struct.pack("<I", riff) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi")

    def add(self, jpeg_bytes):
        if self._f is None:
            raise ValueError("gflow_amd.video: the AVI is closed")
        data = bytes(jpeg_bytes)
        padded = len(data) + (len(data) & 1)
        if self._pos + 8 + padded + 8 + 16 * (len(self._index) + 1) > MAX_FILE:
            raise ValueError(f"gflow_amd.video: {self.path} would pass 2 GiB with frame {len(self._index)} (no OpenDML: "
                             "start another file)")
        self._index.append((self._pos - (_MOVI_LIST + 8), len(data)))
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (padded - len(data)))
        self._pos += 8 + padded
        self._largest = max(self._largest, len(data))

    @property
    def frames(self):
        return len(self._index)

    def close(self):
        """idx1 and the patched headers; returns the file's size"""
        if self._f is None:
            return self._pos
        f, self._f = self._f, None
        movi_bytes = self._pos - (_MOVI_LIST + 12)
        f.write(b"idx1" + struct.pack("<I", 16 * len(self._index))
                + b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, o, s) for o, s in self._index))
        self._pos += 8 + 16 * len(self._index)
        f.seek(0)
        f.write(self._headers(movi_bytes))
        f.close()
        return self._pos

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def write_avi(path, images, fps=5, quality=90, chunk=64):
    """``images`` ((T, H, W, 3) or (T, H, W) uint8, device or host) as a Motion-JPEG AVI: coded on the device in stacks of
    ``chunk`` frames, each stack appended before the next is coded.  Returns dict(frames, bytes)."""
    t = _tensor(images)
    if t.dtype != torch.uint8 or t.dim() not in (3, 4):
        raise ValueError(f"gflow_amd.video: images must be (T, H, W, 3) or (T, H, W) uint8, got {tuple(t.shape)} {t.dtype}")
    chunk = max(int(chunk), 1)
    with AviWriter(path, t.shape[2], t.shape[1], fps) as avi:
        for a in range(0, int(t.shape[0]), chunk):
            for frame in encode_jpeg(t[a:a + chunk], quality):
                avi.add(frame)
    return dict(frames=avi.frames, bytes=avi.close())


def _chunks(buf, start, end):
    """(fourcc, payload start, payload size) of the chunks in buf[start:end]"""
    pos = start
    while pos + 8 <= end:
        size = struct.unpack_from("<I", buf, pos + 4)[0]
        yield buf[pos:pos + 4], pos + 8, size
        pos += 8 + size + (size & 1)


def read_avi(path):
    """Walk the RIFF tree of an AVI and its ``idx1``: dict(width, height, fps, frames) with every frame's bytes (a complete
    JPEG image each, for a Motion-JPEG file) in index order.  Raises ValueError on a file that is not such an AVI."""
    buf = open(path, "rb").read()
    if len(buf) < 12 or buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    end = min(len(buf), 8 + struct.unpack_from("<I", buf, 4)[0])
    avih = strh = strf = movi = idx1 = None
    for cc, at, size in _chunks(buf, 12, end):
        if cc == b"LIST" and buf[at:at + 4] == b"hdrl":
            for cc2, at2, size2 in _chunks(buf, at + 4, at + size):
                if cc2 == b"avih":
                    avih = struct.unpack_from("<14I", buf, at2)
                elif cc2 == b"LIST" and buf[at2:at2 + 4] == b"strl" and strh is None:
                    for cc3, at3, size3 in _chunks(buf, at2 + 4, at2 + size2):
                        if cc3 == b"strh":
                            strh = (buf[at3:at3 + 4], buf[at3 + 4:at3 + 8]) + struct.unpack_from("<IHHIIIIIIII", buf, at3 + 8)
                        elif cc3 == b"strf":
                            strf = struct.unpack_from("<IiiHH4sIiiII", buf, at3)
        elif cc == b"LIST" and buf[at:at + 4] == b"movi":
            movi = at                                        # (the fourcc: what idx1's offsets count from)
        elif cc == b"idx1":
            idx1 = [(buf[p:p + 4],) + struct.unpack_from("<III", buf, p + 4) for p in range(at, at + size, 16)]
    if None in (avih, strh, strf, movi, idx1):
        raise ValueError(f"{path}: an AVI without avih, strh, strf, movi or idx1")
    frames = []
    for cc, _, off, size in idx1:
        at = movi + off
        if buf[at:at + 4] != cc or struct.unpack_from("<I", buf, at + 4)[0] != size:
            raise ValueError(f"{path}: idx1 entry {len(frames)} does not point at its chunk")
        frames.append(buf[at + 8:at + 8 + size])
    return dict(width=strf[1], height=abs(strf[2]), fps=strh[7] / strh[6], frames=frames, handler=strh[1], total_frames=avih[4],
                stream_length=strh[9])


def read_avi_frames(path, device=None, chunk=64, select=None):
    """The frames of a Motion-JPEG AVI as a (T, H, W, C) uint8 stack on the device: ``read_avi``, then ``decode_jpeg`` in
    stacks of ``chunk`` frames.  ``select``: the indices of the frames to decode (default: all, in order)."""
    frames = read_avi(path)["frames"]
    idx = list(range(len(frames))) if select is None else [int(i) for i in select]
    chunk = max(int(chunk), 1)
    stacks = [decode_jpeg([frames[i] for i in idx[a:a + chunk]], device, names=[f"{path}, frame {i}" for i in idx[a:a + chunk]])
              for a in range(0, len(idx), chunk)]
    return torch.cat(stacks) if stacks else decode_jpeg([], device)


def _unpack(path, out, chunk=64):
    from PIL import Image
    os.makedirs(out, exist_ok=True)
    frames = read_avi(path)["frames"]
    for a in range(0, len(frames), chunk):
        stack = decode_jpeg(frames[a:a + chunk], names=[f"{path}, frame {i}" for i in range(a, min(a + chunk, len(frames)))])
        for i, img in enumerate(stack.cpu().numpy()):
            Image.fromarray(img[..., 0] if img.shape[-1] == 1 else img).save(os.path.join(out, f"frame_{a + i:05d}.png"))
    print(f"{len(frames)} frames of {path} -> {out}")
    return 0


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(description="a folder of images as a Motion-JPEG AVI, coded on the device (--frames), or "
                                 "the frames of such a file, decoded on the device, as PNG files (--unpack)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--frames", help="directory of image files (taken in sorted order, one shape)")
    src.add_argument("--unpack", metavar="FILE.avi", help="a Motion-JPEG AVI whose frames go to --out as frame_00000.png, ...")
    ap.add_argument("--out", required=True, help="the .avi file (--frames) or the directory of PNG files (--unpack)")
    ap.add_argument("--fps", type=float, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
    if args.unpack:
        torch.cuda.set_device(args.gpu)
        return _unpack(args.unpack, args.out)
    names = sorted(n for n in os.listdir(args.frames) if n.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")))
    if not names:
        raise ValueError(f"{args.frames}: no image files")
    torch.cuda.set_device(args.gpu)
    chunk, n, size = 64, 0, None
    first = Image.open(os.path.join(args.frames, names[0]))
    with AviWriter(args.out, first.width, first.height, args.fps) as avi:
        for a in range(0, len(names), chunk):
            stack = np.stack([np.asarray(Image.open(os.path.join(args.frames, f)).convert("RGB")) for f in names[a:a + chunk]])
            for frame in encode_jpeg(stack, args.quality):
                avi.add(frame)
        n = avi.frames
        size = avi.close()
    print(f"{n} frames of {first.width}x{first.height} at {args.fps:g} fps -> {args.out} ({size} bytes)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
