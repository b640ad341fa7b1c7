"""CPU: video files -- the ABI entries, the tables of gflow_amd.video against the segments PIL writes, the float64 / integer
restatement (tests/jpeg_ref.py) against PIL and against its own decoder, and the AVI writer and reader.  Also holds the
inputs the GPU tests (tests/test_gpu_video.py) share."""
import ctypes
import functools
import io
import os
import re
import struct

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def content(kind, H, W, C=3, seed=0):
    """(H, W, C) uint8 (C = 1: (H, W)), computed once and left unchanged.  "flat": one grey; "smooth": a sinusoid per channel;
    "noise": uniform bytes; "checker": 0 / 255 per pixel; "cosine": every block the single highest-frequency basis image,
    (7, 7), which a block codes as zero runs of 62."""
    rng = np.random.default_rng([seed, H, W, C, len(kind), ord(kind[0])])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "flat":
        a = np.full((H, W, C), 100.0)
    elif kind == "smooth":
        a = np.stack([127.5 + 110.0 * np.sin(0.11 * (c + 1) * x + 0.07 * y + c) * np.cos(0.05 * y - 0.03 * c * x)
                      for c in range(C)], axis=-1)
    elif kind == "noise":
        a = rng.integers(0, 256, size=(H, W, C)).astype(np.float64)
    elif kind == "checker":
        a = np.repeat((((x + y) % 2) * 255.0)[..., None], C, axis=-1)
    elif kind == "cosine":
        a = 128.0 + 100.0 * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
        a = np.repeat(a[..., None], C, axis=-1)
    else:
        raise KeyError(kind)
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    a = a[..., 0] if C == 1 else a
    a.setflags(write=False)
    return a


def psnr(a, b):
    mse = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)


def pil_jpeg(img, quality):
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(buf, format="JPEG", quality=quality, subsampling=0, optimize=False)
    return buf.getvalue()


def pil_decode(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


# WINDOW: a device coefficient may differ from the float64 one only where F / q lies this close (times 1 / q) to a half
# integer.  The float32 error of F: a coefficient is a 64-term sum of products |sample| <= 128 times two DCT weights,
# |F| <= 1024; summed in float32 in any order the error is at most 64 eps |terms| <= 64 * 2^-24 * 1024 = 2^-8, and the colour
# transform adds at most 3 eps * 255 per sample, 2^-14, carried through weights that sum to at most 8: 2^-11.  2^-6 is twice
# that bound and more.
WINDOW = 2.0 ** -6


def near_half(ratio, quality, C):
    """mask over (n_mcu, C, 64): |F - q (n + 1/2)| <= WINDOW, i.e. F / q within WINDOW / q of a half integer"""
    from gflow_amd.video import ZIGZAG, quant_tables
    qt = quant_tables(quality).astype(np.float64)[:, list(ZIGZAG)]
    q = np.stack([qt[0 if c == 0 else 1] for c in range(C)])[None]
    frac = np.abs(ratio) - np.floor(np.abs(ratio))
    return np.abs(frac - 0.5) <= WINDOW / q


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_entries_within_312():
    from gflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    assert re.search(r"^#define GFL_VERSION 312$", hdr, flags=re.M) and _lib.MIN_VERSION == 312
    assert _lib.load().gfl_version() == 312
    assert "video files (additive within 312" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n in (("gfl_jpeg_restart_interval", 0), ("gfl_jpeg_workspace_bytes", 4), ("gfl_jpeg_sizes", 10),
                    ("gfl_jpeg_emit", 11)):
        args = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1)
        got = 0 if args.strip() == "void" else len(args.split(","))
        assert got == n == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["gfl_jpeg_workspace_bytes"][0] is ctypes.c_size_t
    assert "gfl_jpeg.hip" in open(os.path.join(ROOT, "gflow_amd", "csrc", "Makefile")).read()


def test_refused_arguments_without_a_device():
    from gflow_amd import _lib
    lib = _lib.load()
    ri = lib.gfl_jpeg_restart_interval()
    assert 1 <= ri <= 65535
    ws = lib.gfl_jpeg_workspace_bytes
    assert 0 < ws(1, 3, 854, 480) < ws(2, 3, 854, 480) < ws(64, 3, 854, 480)    # (regions are rounded up to 256 bytes)
    assert 0 < ws(1, 3, 64, 48) <= ws(2, 3, 64, 48) < ws(64, 3, 64, 48)
    assert ws(1, 1, 8, 8) > 0 and ws(1, 3, 65535, 65535) > 0
    # host memory stands in for every buffer: a call that got past the checks would hand it to the device runtime
    buf = (ctypes.c_uint64 * 64)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    good = dict(T=2, C=3, W=17, H=9)
    need = ws(*good.values())

    def sizes(images=p, qt=p, off=p, w=p, size=need, **shape):
        s = dict(good, **shape)
        return lib.gfl_jpeg_sizes(images, s["T"], s["C"], s["W"], s["H"], qt, off, w, size, null)

    def emit(images=p, qt=p, out=p, out_bytes=512, w=p, size=need, **shape):
        s = dict(good, **shape)
        return lib.gfl_jpeg_emit(images, s["T"], s["C"], s["W"], s["H"], qt, out, out_bytes, w, size, null)

    for bad in (dict(T=0), dict(T=-1), dict(C=0), dict(C=2), dict(C=4), dict(W=0), dict(H=0), dict(W=-8), dict(W=65536),
                dict(H=65536), dict(T=1 << 30, W=4096, H=4096)):
        assert ws(*dict(good, **bad).values()) == 0, bad
        assert sizes(**bad, size=1 << 40) == -1 and emit(**bad, size=1 << 40) == -1, bad
    for kw in (dict(images=null), dict(qt=null), dict(w=null)):
        assert sizes(**kw) == -1 and emit(**kw) == -1, kw
    assert sizes(off=null) == -1 and emit(out=null) == -1 and emit(out_bytes=0) == -1
    assert sizes(size=need - 1) == -2 and emit(size=need - 1) == -2 and sizes(size=0) == -2
    assert not any(buf)


def test_no_cpu_path(monkeypatch):
    from gflow_amd import video
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video.encode_jpeg(np.zeros((1, 8, 8, 3), dtype=np.uint8))


# ---------------------------------------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("q", [1, 50, 75, 90, 100])
def test_tables_are_the_segments_pil_writes(q):
    from gflow_amd import video
    img = content("smooth", 16, 16)
    for C, src in ((3, img), (1, img[..., 0])):
        ours, pil = video.jpeg_header(16, 16, C, q), pil_jpeg(src, q)
        for marker in (0xDB, 0xC4):
            a, b = R.tables(ours, marker), R.tables(pil, marker)
            assert sorted(a) == sorted(b) and len(a) == ((2 if C == 3 else 1) * (1 if marker == 0xDB else 2)), (C, marker)
            for k in a:
                assert a[k] == b[k], (q, C, hex(marker), k)
    with pytest.raises(ValueError):
        video.quant_tables(0)
    with pytest.raises(ValueError):
        video.quant_tables(101)


def test_header_layout():
    from gflow_amd import video
    h = video.jpeg_header(300, 200, 3, 90, ri=32)
    assert h[:2] == b"\xff\xd8"
    seg = R.segments(h)
    assert [m for m, _ in seg] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert seg[0][1][:5] == b"JFIF\0"
    assert seg[3][1] == bytes([8]) + struct.pack(">HH", 200, 300) + bytes([3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert seg[8][1] == struct.pack(">H", 32)
    assert seg[9][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert video.jpeg_header(300, 200, 3, 90) == video.jpeg_header(300, 200, 3, 90, ri=video.restart_interval())
    g = R.segments(video.jpeg_header(8, 8, 1, 50, ri=4))
    assert [m for m, _ in g] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDD, 0xDA]
    for bad in (dict(W=0), dict(H=65536), dict(C=2)):
        with pytest.raises(ValueError):
            video.jpeg_header(**dict(dict(W=8, H=8, C=3, quality=90, ri=4), **bad))


# ------------------------------------------------------------------------------------ the reference encoder and PIL
CASES = [("smooth", 40, 56, 3, 90), ("noise", 17, 9, 3, 90), ("smooth", 17, 9, 1, 50), ("noise", 24, 40, 1, 100),
         ("checker", 16, 24, 3, 100), ("cosine", 16, 16, 3, 90), ("flat", 8, 8, 3, 75), ("smooth", 33, 70, 3, 50)]


@pytest.mark.parametrize("kind,H,W,C,q", CASES)
def test_reference_file_opens_in_pil_and_is_as_good_as_pils(kind, H, W, C, q):
    """header + reference scan + EOI is a file PIL opens at the right size and mode, and it decodes no worse than PIL's own
    encode with the same tables (only the rounding of the transform differs: libjpeg's is in integers).
    Measured, PSNR of ours minus PSNR of PIL's, dB, over CASES in order: +0.096, +0.172, 0.000, +0.414, then checker, cosine
    and flat, which both decode exactly (infinite PSNR), and +0.035: never below PIL's."""
    from gflow_amd import video
    img = content(kind, H, W, C)
    ri = 5                                         # (not the library's: a file states its own interval)
    data = video.jpeg_header(W, H, C, q, ri=ri) + R.encode_scan(img, q, ri) + video.EOI
    im = pil_decode(data)
    assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "L")
    ours, pils = psnr(np.asarray(im), img), psnr(np.asarray(pil_decode(pil_jpeg(img, q))), img)
    print(f"{kind} {H}x{W} C={C} q={q}: ours {ours:.3f} dB, PIL {pils:.3f} dB, difference {ours - pils:+.3f}")
    assert ours >= pils - 0.2 or ours == float("inf")


@pytest.mark.parametrize("kind,H,W,C,q", CASES)
def test_decoder_inverts_the_entropy_coder(kind, H, W, C, q):
    img = content(kind, H, W, C)
    coef = R.coefficients(img, q)
    for ri in (1, 3, 32):
        scan = R.entropy_encode(coef, ri)
        back = R.decode_scan(scan, R.n_mcus(W, H), C, ri)
        assert np.array_equal(back, coef)
        assert R.entropy_encode(back, ri) == scan
    if kind == "cosine":
        assert np.all(coef[:, 0, 1:63] == 0) and np.all(coef[:, 0, 63] != 0)         # runs of 62: three ZRL per block
    if kind == "flat":
        assert np.all(coef[:, :, 1:] == 0) and np.all(coef[1:, :, 0] == coef[:1, :, 0])
    if kind == "checker":
        assert np.abs(coef[:, 0, 1:]).max() >= 512                                   # the largest AC category


def test_decoder_refuses_damage():
    img = content("noise", 24, 40, 1)
    scan = R.encode_scan(img, 100, 4)
    assert b"\xff\x00" in scan and b"\xff\xd0" in scan and b"\xff\xd1" in scan
    with pytest.raises(ValueError):
        R.decode_scan(scan.replace(b"\xff\xd1", b"\xff\xd2", 1), R.n_mcus(40, 24), 1, 4)
    with pytest.raises(ValueError):
        R.decode_scan(scan, R.n_mcus(40, 24), 1, 5)


def test_window_does_not_swallow_the_check():
    """on the reference alone: at most 5 % of an input's coefficients may lie where a +-1 is allowed"""
    for kind, H, W, C, q in CASES:
        share = near_half(R.ratios(content(kind, H, W, C), q), q, C).mean()
        print(f"{kind} {H}x{W} C={C} q={q}: {100 * share:.2f} % inside the window")
        assert share <= 0.05, (kind, q, share)


# ------------------------------------------------------------------------------------------------------------ the AVI
def _riff(buf):
    """flat list of (path, fourcc, payload offset, size) of every chunk, LISTs entered"""
    from gflow_amd.video import _chunks
    out = []

    def walk(start, end, path):
        for cc, at, size in _chunks(buf, start, end):
            if cc in (b"RIFF", b"LIST"):
                kind = bytes(buf[at:at + 4])
                out.append((path, cc + b":" + kind, at, size))
                walk(at + 4, at + size, path + (kind,))
            else:
                out.append((path, bytes(cc), at, size))
    walk(0, len(buf), ())
    return out


@pytest.mark.parametrize("fps,rate,scale", [(5, 5, 1), (30.0, 30, 1), (29.97, 29970, 1000), (12.5, 12500, 1000)])
def test_avi_round_trip_and_structure(tmp_path, fps, rate, scale):
    from gflow_amd import video
    rng = np.random.default_rng(3)
    frames = [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (11, 12, 1, 255, 4096, 7)]      # odd and even
    path = str(tmp_path / "a.avi")
    w = video.AviWriter(path, 34, 18, fps)
    for f in frames:
        w.add(f)
    assert w.frames == len(frames)
    size = w.close()
    assert w.close() == size == os.path.getsize(path)
    with pytest.raises(ValueError):
        w.add(b"x")
    got = video.read_avi(path)
    assert got["frames"] == frames and (got["width"], got["height"]) == (34, 18)
    assert got["fps"] == pytest.approx(float(fps), abs=1e-9) and got["handler"] == b"MJPG"
    assert got["total_frames"] == got["stream_length"] == len(frames)
    buf = open(path, "rb").read()
    chunks = _riff(buf)
    assert [c[1] for c in chunks if c[0] == ()] == [b"RIFF:AVI "]
    riff = chunks[0]
    assert riff[3] == len(buf) - 8
    top = [c for c in chunks if c[0] == (b"AVI ",)]
    assert [c[1] for c in top] == [b"LIST:hdrl", b"LIST:movi", b"idx1"]
    assert top[2][2] + top[2][3] == len(buf)                                   # idx1 ends the file
    movi = top[1]
    dc = [c for c in chunks if c[0] == (b"AVI ", b"movi")]
    assert [c[1] for c in dc] == [b"00dc"] * len(frames) and [c[3] for c in dc] == [len(f) for f in frames]
    assert movi[3] == 4 + sum(8 + len(f) + len(f) % 2 for f in frames)         # odd chunks are padded
    assert all(c[2] % 2 == 0 for c in dc)
    for c, f in zip(dc, frames):
        if len(f) % 2:
            assert buf[c[2] + len(f)] == 0
    idx = [struct.unpack_from("<4sIII", buf, top[2][2] + 16 * k) for k in range(len(frames))]
    assert top[2][3] == 16 * len(frames)
    for (cc, flags, off, n), c in zip(idx, dc):
        assert cc == b"00dc" and flags == video.AVIIF_KEYFRAME and n == c[3]
        assert movi[2] + off == c[2] - 8                                       # from the movi fourcc to the chunk's header
    by = {c[1]: c for c in chunks}
    avih = struct.unpack_from("<14I", buf, by[b"avih"][2])
    assert by[b"avih"][3] == 56 and avih[3] & video.AVIF_HASINDEX and avih[4] == len(frames) and avih[6] == 1
    assert avih[8:10] == (34, 18) and avih[0] == round(1e6 * scale / rate)
    at = by[b"strh"][2]
    assert by[b"strh"][3] == 56 and buf[at:at + 8] == b"vidsMJPG"
    strh = struct.unpack_from("<IHHIIIIIIII", buf, at + 8)
    assert (strh[4], strh[5]) == (scale, rate) and strh[7] == len(frames)
    strf = struct.unpack_from("<IiiHH4sI", buf, by[b"strf"][2])
    assert by[b"strf"][3] == 40 and strf[:6] == (40, 34, 18, 1, 24, b"MJPG")


def test_avi_empty_and_guard(tmp_path):
    from gflow_amd import video
    path = str(tmp_path / "e.avi")
    with video.AviWriter(path, 8, 8, 5):
        pass
    got = video.read_avi(path)
    assert got["frames"] == [] and got["total_frames"] == 0
    # the 2 GiB guard looks at the writer's byte counter: moved, not written
    w = video.AviWriter(str(tmp_path / "g.avi"), 8, 8, 5)
    w.add(b"abc")
    w._pos = video.MAX_FILE - 8 - 100 - 8 - 32 + 1
    with pytest.raises(ValueError, match="2 GiB"):
        w.add(b"\0" * 100)
    w._pos -= 1
    w.add(b"\0" * 100)                             # ends exactly at the limit
    assert w._pos + 8 + 16 * 2 == video.MAX_FILE
    w._f.close()
    for bad in (0, -1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            video.AviWriter(str(tmp_path / "b.avi"), 8, 8, bad)
    with pytest.raises(ValueError):
        video.read_avi(__file__)


def test_users_meet_it():
    """the viewer and fit_video take --video; --out is optional with it, --format is as it was"""
    from gflow_amd import fit_video, track_vis, viewer
    assert callable(track_vis.write_video)
    with pytest.raises(SystemExit) as e:
        viewer.main(["--folder", "x"])                                         # neither --out nor --video
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        viewer.main(["--folder", "x", "--video", "f.avi", "--format", "gif"])
    assert e.value.code == 2
    ap = fit_video._parser()
    assert ap.parse_args(["--video", "--track-vis", "d", "--traj-num", "4"]).video is True and ap.parse_args([]).video is False
    with pytest.raises(SystemExit):
        fit_video._check_args(ap, ap.parse_args(["--video"]))                  # --video needs --track-vis
