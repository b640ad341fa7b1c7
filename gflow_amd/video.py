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

The AVI writer and reader and ``jpeg_header`` need no device; ``encode_jpeg`` has no CPU path.
"""
import argparse
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


def main(argv=None):
    from PIL import Image
    ap = argparse.ArgumentParser(description="a folder of images as a Motion-JPEG AVI, coded on the device")
    ap.add_argument("--frames", required=True, help="directory of image files (taken in sorted order, one shape)")
    ap.add_argument("--out", required=True, help="the .avi file")
    ap.add_argument("--fps", type=float, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
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
