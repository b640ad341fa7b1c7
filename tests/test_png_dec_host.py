"""CPU: decoding PNG files -- the Python reference (tests/png_dec_ref.py) against PIL, bit for bit, and against zlib's accept /
reject; ``png.parse_png`` against the reference's parser and its refusals; the decode core (csrc/gfl_inflate.hpp) on the CPU
under the address and undefined-behaviour sanitizers (tools/png_dec_host.cpp, a stand-alone program run as a subprocess) on
good and on malformed streams; the loader's option.  Also holds the inputs the GPU tests (tests/test_gpu_png_dec.py) share."""
import ctypes
import functools
import io
import os
import re
import shutil
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_dec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4, "P": 1}
COLOUR = {"L": 0, "LA": 4, "RGB": 2, "RGBA": 6, "P": 3}
SETTINGS = (dict(compress_level=0), dict(compress_level=1), dict(compress_level=9), dict(optimize=True), dict())
SIZES = ((1, 1), (1, 300), (65, 3), (50, 70), (200, 300))
KINDS = ("smooth", "noise", "photo", "checker", "constant")


# ------------------------------------------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def content(kind, H, W, C, seed=0):
    """(H, W, C) uint8, computed once and left unchanged.  "photo": smooth plus noise of +-6"""
    rng = np.random.default_rng([seed, H, W, C, len(kind), ord(kind[0])])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    smooth = np.stack([127.5 + 110.0 * np.sin(0.11 * (c + 1) * x + 0.07 * y + c) * np.cos(0.05 * y - 0.03 * c * x)
                       for c in range(C)], axis=-1)
    if kind == "smooth":
        a = smooth
    elif kind == "noise":
        a = rng.integers(0, 256, size=(H, W, C)).astype(np.float64)
    elif kind == "photo":
        a = smooth + rng.integers(-6, 7, size=(H, W, C))
    elif kind == "checker":
        a = np.repeat((((x + y) % 2) * 255.0)[..., None], C, axis=-1)
    elif kind == "constant":
        a = np.full((H, W, C), 100.0)
    else:
        raise KeyError(kind)
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pil_file(kind, H, W, mode, setting, seed=0):
    """a PNG file as PIL writes it: ``mode`` of MODES, ``setting`` an index into SETTINGS"""
    a = content(kind, H, W, MODES[mode], seed)
    img = Image.frombytes(mode, (W, H), a.tobytes())
    if mode == "P":
        img.putpalette(bytes(range(256)) * 3)
    buf = io.BytesIO()
    img.save(buf, format="PNG", **SETTINGS[setting])
    return buf.getvalue()


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def as_hwc(a):
    return a[..., None] if a.ndim == 2 else a


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def make_png(W, H, colour, pieces, extra=()):
    """a file around the IDAT payloads ``pieces``; ``extra``: chunks between IHDR and the first IDAT"""
    out = [R.SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, colour, 0, 0, 0))]
    if colour == 3:
        out.append(_chunk(b"PLTE", bytes(range(256)) * 3))
    out += [_chunk(k, b) for k, b in extra]
    out += [_chunk(b"IDAT", bytes(p)) for p in pieces]
    return b"".join(out + [_chunk(b"IEND", b"")])


def filtered_rows(img, types):
    """the filtered bytes of (H, W, bpp) uint8 with filter type types[r] for row r (PNG specification, 9.2), computed here"""
    H, W, bpp = img.shape
    raw = img.reshape(H, W * bpp).astype(np.int64)
    out = bytearray()
    for r in range(H):
        cur, up = raw[r], (raw[r - 1] if r else np.zeros(W * bpp, np.int64))
        a = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
        c = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])
        p = a + up - c
        pa, pb, pc = abs(p - a), abs(p - up), abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        pred = [0 * cur, a, up, (a + up) >> 1, paeth][types[r]]
        out += bytes([types[r]]) + ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


class BitWriter:
    """deflate's bit order: values least significant bit first, prefix codes most significant bit first"""

    def __init__(self):
        self.bits = []

    def value(self, v, n):
        self.bits += [(v >> i) & 1 for i in range(n)]
        return self

    def code(self, c, n):
        self.bits += [(c >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(bit << i for i, bit in enumerate(b[k:k + 8])) for k in range(0, len(b), 8))


def dynamic_header(lit, dist, w=None, nlen=None, ndist=None, cl=None):
    """a final dynamic block's header for the code lengths ``lit`` and ``dist``, every length sent as its own symbol under a
    code-length code of 16 codes of 4 bits (``cl``: other lengths of that code, in symbol order)"""
    w = BitWriter() if w is None else w
    w.value(1, 1).value(2, 2).value((len(lit) if nlen is None else nlen) - 257, 5)
    w.value((len(dist) if ndist is None else ndist) - 1, 5).value(15, 4)
    cl = [4] * 16 + [0] * 3 if cl is None else cl
    for sym in R.CL_ORDER:
        w.value(cl[sym], 3)
    for l in list(lit) + list(dist):
        w.code(l, 4)
    return w


def _lit_lengths(**lengths):
    out = [0] * (max(int(k[1:]) for k in lengths) + 1)
    for k, l in lengths.items():
        out[int(k[1:])] = l
    return out


def zstream(body, rows=None):
    """78 9C, the blocks, and the Adler-32 of ``rows`` where given"""
    return b"\x78\x9c" + body + (struct.pack(">I", zlib.adler32(rows)) if rows is not None else b"")


# canonical codes: length 3 (symbol 257) is 0, literal 1 is 10, end of block 11; ONE distance code of length 1 (distance 1):
# the incomplete code zlib allows
_TINY_LIT = _lit_lengths(s1=2, s256=2, s257=1)
TINY_SHAPE = dict(W=3, H=1, bpp=1)             # 4 filtered bytes: 01 01 01 01 -- Sub over 1 1 1 -> pixels 1 2 3


def tiny_stream():
    w = dynamic_header(_TINY_LIT, [1])
    w.code(2, 2).code(0, 1).code(0, 1).code(3, 2)               # literal 1, length 3, distance 1, end of block
    return zstream(w.bytes(), b"\x01" * 4)


@functools.lru_cache(maxsize=None)
def handmade_files():
    """[(name, file bytes, expected (H, W, bpp) pixels or None: ask PIL)]"""
    out = []
    for bpp, colour in ((1, 0), (2, 4), (3, 2), (4, 6)):
        img = content("photo", 6, 9, bpp, seed=bpp)
        for ft in range(5):                                     # row 0 carries Up, Average and Paeth too
            out.append((f"filter {ft} bpp {bpp}", make_png(9, 6, colour, [zlib.compress(filtered_rows(img, [ft] * 6))]), img))
        out.append((f"filters mixed bpp {bpp}", make_png(9, 6, colour, [zlib.compress(filtered_rows(img, [4, 3, 2, 1, 0, 4]))]), img))
    img = content("smooth", 20, 40, 3)
    co = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
    rows = filtered_rows(img, [1] * 20)
    out.append(("fixed blocks", make_png(40, 20, 2, [co.compress(rows) + co.flush()]), img))
    rng = np.random.default_rng(11)
    base = rng.integers(0, 256, size=(15, 700, 3)).astype(np.uint8)
    img = base[np.arange(40) % 15]                              # rows repeat 15 rows = 31515 filtered bytes back
    stream = zlib.compress(filtered_rows(img, [0] * 40), 9)
    out.append(("rows repeating 31515 back", make_png(700, 40, 2, [stream]), img))
    whole = pil_file("photo", 50, 70, "RGB", 4)
    s = R.parse(whole)["stream"]
    pieces, at, n = [], 0, 1
    while at < len(s):                                          # IDAT chunks of 1, 2, 3, ... bytes
        pieces.append(s[at:at + n])
        at += n
        n += 1
    out.append(("idat cut into 1, 2, 3, ... bytes", make_png(70, 50, 2, pieces, extra=[(b"tEXt", b"k\0v"), (b"gAMA", b"\0\1\x86\xa0")]),
                content("photo", 50, 70, 3)))
    from gflow_amd import png
    img = content("photo", 12, 17, 3)
    out.append(("png_chunks", png.png_chunks(zlib.compress(filtered_rows(img, [2] * 12)), 17, 12, 3), img))
    out.append(("one distance code of length 1", make_png(3, 1, 0, [tiny_stream()]), np.array([[[1], [2], [3]]], np.uint8)))
    return out


def _grid():
    """(kind, H, W, mode, setting): what the Python reference is held to PIL on.  Up to 50 x 70 the whole cross of content,
    mode and PIL setting (the default among them); at 200 x 300, where the Python reference takes its time, the cases that
    size is there for: several stored blocks (level 0 of 180200 bytes), several IDAT chunks as PIL cuts them (noise), long
    streams of every mode.  The implementations -- the sanitized harness and the device -- are held to PIL on the whole
    cross at 200 x 300 as well: GRID_LARGE."""
    out = [(k, H, W, m, s) for H, W in SIZES[:4] for k in KINDS for m in MODES for s in range(len(SETTINGS))]
    out += [("noise", 200, 300, "RGB", 4), ("photo", 200, 300, "RGB", 0), ("photo", 200, 300, "RGBA", 3),
            ("smooth", 200, 300, "L", 2), ("checker", 200, 300, "LA", 1), ("constant", 200, 300, "P", 2),
            ("photo", 200, 300, "P", 4), ("smooth", 200, 300, "RGB", 1)]
    return out


GRID = _grid()
GRID_LARGE = [(k, 200, 300, m, s) for k in KINDS for m in MODES for s in range(len(SETTINGS))]


@functools.lru_cache(maxsize=None)
def reference_decode(data):
    pixels, status, stats = R.decode(data)
    pixels.setflags(write=False)
    return pixels, status, stats


# ------------------------------------------------------------------------------------- 1. the reference is PIL, bit for bit
def _merge(total, s):
    for k in ("blocks", "filters"):
        total[k] |= s[k]
    for k in ("max_distance", "max_length", "stored_blocks", "idat"):
        total[k] = max(total[k], s[k])
    total["overlap"] |= s["overlap"]


@pytest.mark.parametrize("mode", list(MODES))
def test_reference_is_pil_bit_for_bit(mode):
    """The acceptance criterion rests on this: the restated inflate and unfilter equal PIL's decode exactly.  Not to be
    loosened -- a PIL build that breaks it is named here by its first differing case."""
    n = 0
    for case in GRID:
        if case[3] != mode:
            continue
        data = pil_file(*case)
        want = as_hwc(pil_pixels(data))
        got, status, _ = reference_decode(data)
        assert status == 0 and got.shape == want.shape and np.array_equal(got, want), case
        assert np.array_equal(want, content(case[0], case[1], case[2], MODES[mode])), case
        n += 1
    assert n >= 100


def test_handmade_files_and_what_the_grid_covers():
    pil_stats, all_stats = R.new_stats(), R.new_stats()
    for case in GRID:
        if case[1:3] in ((50, 70), (200, 300), (1, 300)):
            _merge(pil_stats, reference_decode(pil_file(*case))[2])
    _merge(all_stats, pil_stats)
    per_file = {}
    for name, data, want in handmade_files():
        got, status, stats = reference_decode(data)
        assert status == 0 and np.array_equal(got, want), name
        assert np.array_equal(as_hwc(pil_pixels(data)), want), name
        _merge(all_stats, stats)
        per_file[name] = stats
    assert all_stats["blocks"] == {0, 1, 2} and per_file["fixed blocks"]["blocks"] == {1}
    assert pil_stats["filters"] == {0, 1, 2, 3, 4}                          # from PIL's own files
    assert {f for c in GRID if c[:3] == ("noise", 50, 70) and c[4] != 3
            for f in reference_decode(pil_file(*c))[2]["filters"]} >= {0, 1, 2, 4}
    assert per_file["rows repeating 31515 back"]["max_distance"] >= 30000 and all_stats["max_length"] == 258
    assert all_stats["overlap"] and per_file["one distance code of length 1"]["overlap"]
    big = reference_decode(pil_file("photo", 200, 300, "RGB", 0))[2]
    assert big["blocks"] == {0} and big["stored_blocks"] >= 3               # 180200 bytes: several stored blocks
    assert R.parse(pil_file("noise", 200, 300, "RGB", 4))["idat"] >= 3      # as PIL wrote it
    assert R.parse(handmade_files()[-3][1])["idat"] > 100
    for ft in range(5):
        assert per_file[f"filter {ft} bpp 3"]["filters"] == {ft}


# ----------------------------------------------------------------------------------------- 2. accept and reject are zlib's
BASE_A = ("photo", 50, 70, "RGB", 4)            # dynamic blocks
BASE_B = ("photo", 50, 70, "RGB", 0)            # stored blocks
BASE_SHAPE = dict(W=70, H=50, bpp=3)
N_FLIPS = 10                                    # per base file: 20 seeded positions in all


@functools.lru_cache(maxsize=None)
def mutation_sets():
    """[dict(name, streams -- the zlib streams of one call, the last of them a good one --, W, H, bpp)]: the malformed inputs,
    made once.  ``files()`` of a set wraps every stream into a file with correct chunk CRCs."""
    a, b = (R.parse(pil_file(*base))["stream"] for base in (BASE_A, BASE_B))
    sets = []

    def add(name, streams, shape=BASE_SHAPE, good=a):
        sets.append(dict(name=name, streams=[bytes(s) for s in streams] + [good], **shape))

    for tag, s in (("A", a), ("B", b)):
        add(f"truncated {tag}", [s[:0], s[:1], s[:len(s) // 2]])
        rng = np.random.default_rng([7, ord(tag)])
        add(f"flipped {tag}", [s[:at] + bytes([s[at] ^ 0xFF]) + s[at + 1:]
                               for at in sorted(int(v) for v in rng.choice(len(s), size=N_FLIPS, replace=False))])
    add("wrong adler", [a[:-1] + bytes([a[-1] ^ 1]), b[:-4] + bytes([b[-4] ^ 0x80]) + b[-3:]])
    add("stored nlen broken", [b[:5] + bytes([b[5] ^ 1]) + b[6:]])
    bad5 = bytearray(filtered_rows(content("photo", 50, 70, 3), [1] * 50))
    bad5[7 * 211] = 5
    add("filter byte of 5", [zlib.compress(bytes(bad5))])
    add("ihdr height one lower", [a, b], dict(BASE_SHAPE, H=49), good=zlib.compress(bytes(49 * 211)))
    add("ihdr height one higher", [a, b], dict(BASE_SHAPE, H=51), good=zlib.compress(bytes(51 * 211)))
    over = dynamic_header([], [], cl=[1] * 4 + [0] * 15, nlen=257, ndist=1)
    incomplete = dynamic_header(_lit_lengths(s1=2, s256=2), [1])
    no_eob = dynamic_header(_lit_lengths(s0=1, s1=1, s256=0), [1])
    hdist = BitWriter().value(1, 1).value(2, 2).value(0, 5).value(30, 5).value(15, 4).value(0, 64)
    far = dynamic_header(_TINY_LIT, [1, 1])
    far.code(2, 2).code(0, 1).code(1, 1).code(3, 2)                 # literal 1, length 3, distance 2: one before the start
    reserved = BitWriter().value(1, 1).value(3, 2).value(0, 29)                              # BTYPE = 3
    repeat = dynamic_header([], [], cl=[4] * 15 + [0, 4, 0, 0], nlen=257, ndist=1)          # symbols 0 .. 14 and 16: 16 is 1111
    repeat.code(15, 4).value(0, 2).value(0, 32)                                             # "repeat the previous length" first
    sym286 = BitWriter().value(1, 1).value(1, 2).code(0xC6, 8).value(0, 32)                 # fixed code: 11000110 is symbol 286
    cm7 = b"\x77\x09" + tiny_stream()[2:]                                                   # CM = 7, FCHECK right
    headers = [zstream(w.bytes(), b"\x01" * 4) for w in (over, incomplete, no_eob, hdist, far, reserved, repeat, sym286)]
    add("hand-made headers", headers + [cm7], TINY_SHAPE, good=tiny_stream())
    return sets


def set_files(s):
    colour = {1: 0, 3: 2}[s["bpp"]]
    return [make_png(s["W"], s["H"], colour, [st]) for st in s["streams"]]


def reference_of_set(s):
    """((T, H, W, bpp), status [T]) of a set by the reference"""
    res = [R.decode_stream(st, s["H"], s["W"], s["bpp"]) for st in s["streams"]]
    return np.stack([p for p, _ in res]), np.array([st for _, st in res], np.int32)


N_SETS = 10


@pytest.mark.parametrize("i", range(N_SETS))
def test_accept_and_reject_are_zlibs(i):
    sets = mutation_sets()
    assert len(sets) == N_SETS
    s = sets[i]
    images, status = reference_of_set(s)
    print(s["name"], status.tolist())
    for t, st in enumerate(s["streams"]):
        accepted = R.zlib_accepts(st, s["H"], s["W"], s["bpp"])
        assert (status[t] == 0) == accepted, (s["name"], t, int(status[t]))
        if accepted:                                                # a flip may leave a well-formed stream: then zlib's bytes
            rows = zlib.decompress(st)
            assert np.array_equal(images[t], R.unfilter(rows, s["H"], s["W"], s["bpp"])), (s["name"], t)
    assert status[-1] == 0
    if not s["name"].startswith("flipped"):
        assert status[:-1].all(), s["name"]
    expect = {"wrong adler": [R.BAD_ADLER] * 2, "stored nlen broken": [R.STORED_LEN], "filter byte of 5": [R.BAD_FILTER],
              "ihdr height one lower": [R.OUTPUT_SIZE] * 2, "ihdr height one higher": [R.OUTPUT_SIZE] * 2,
              "truncated A": [R.INPUT_END] * 3, "truncated B": [R.INPUT_END] * 3,
              "hand-made headers": [R.BAD_CODE, R.BAD_CODE, R.NO_END_OF_BLOCK, R.TOO_MANY_CODES, R.FAR_DISTANCE, R.BLOCK_TYPE,
                                    R.BAD_REPEAT, R.BAD_SYMBOL, R.BAD_HEADER]}
    if s["name"] in expect:
        assert status[:-1].tolist() == expect[s["name"]], s["name"]


def test_flips_find_errors():
    sets = [s for s in mutation_sets() if s["name"].startswith("flipped")]
    assert sum(len(s["streams"]) - 1 for s in sets) == 2 * N_FLIPS
    assert all(reference_of_set(s)[1][:-1].any() for s in sets)


# ------------------------------------------------------------------------------------------------------- 3. parse_png
@pytest.mark.parametrize("case", [("photo", 50, 70, "RGB", 4), ("noise", 200, 300, "RGB", 4), ("smooth", 1, 1, "L", 0),
                                  ("checker", 65, 3, "LA", 3), ("photo", 1, 300, "RGBA", 2), ("noise", 50, 70, "P", 1)])
def test_parse_png_against_the_references_parser(case):
    from gflow_amd import png
    data = pil_file(*case)
    p, r = png.parse_png(data), R.parse(data)
    assert (p["width"], p["height"], p["bpp"], p["colour_type"]) == (r["W"], r["H"], r["bpp"], r["colour"]) \
        == (case[2], case[1], MODES[case[3]], COLOUR[case[3]])
    assert p["stream"] == r["stream"] and p["idat_chunks"] == r["idat"]
    assert (p["palette"] is None) == (case[3] != "P")
    if case[3] == "P":
        assert p["palette"].dtype == np.uint8 and np.array_equal(p["palette"], r["palette"])
    for name, data, _ in handmade_files():
        assert png.parse_png(data)["stream"] == R.parse(data)["stream"], name


def _saved(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="PNG", **kw)
    return buf.getvalue()


def test_parse_png_refuses_what_is_out_of_scope():
    from gflow_amd import png
    good = pil_file("photo", 50, 70, "RGB", 4)
    grey = Image.fromarray(content("smooth", 8, 8, 1)[..., 0])
    stream = R.parse(good)["stream"]
    ihdr = lambda *v: _chunk(b"IHDR", struct.pack(">IIBBBBB", *v))
    idat, iend = _chunk(b"IDAT", stream), _chunk(b"IEND", b"")
    at = good.index(b"IDAT") + 10
    cases = {
        "not a png": (b"\x89PNX" + good[4:], "signature"),
        "wrong crc": (good[:at] + bytes([good[at] ^ 1]) + good[at + 1:], "CRC"),
        "one bit": (_saved(grey.convert("1")), "bit depth 1"),
        "sixteen bits": (_saved(Image.fromarray(np.arange(64, dtype=np.uint16).reshape(8, 8) * 900)), "bit depth 16"),
        "interlaced": (R.SIGNATURE + ihdr(70, 50, 8, 2, 0, 0, 1) + idat + iend, "interlaced"),
        "colour type 5": (R.SIGNATURE + ihdr(70, 50, 8, 5, 0, 0, 0) + idat + iend, "colour type 5"),
        "no ihdr": (R.SIGNATURE + idat + iend, "no IHDR"),
        "no idat": (R.SIGNATURE + ihdr(70, 50, 8, 2, 0, 0, 0) + iend, "no IDAT"),
        "no iend": (good[:-12], "no IEND"),
        "unknown critical": (R.SIGNATURE + ihdr(70, 50, 8, 2, 0, 0, 0) + _chunk(b"ABCD", b"x") + idat + iend, "unknown critical"),
        "cut": (good[:len(good) // 2], "cut short"),
    }
    for name, (data, why) in cases.items():
        with pytest.raises(ValueError, match=why) as e:
            png.parse_png(data, "the file " + name)
        assert "the file " + name in str(e.value), name
        if name not in ("one bit", "sixteen bits"):
            with pytest.raises(ValueError):
                R.parse(data)
    # ancillary chunks are skipped, whatever their CRC says
    anc = make_png(70, 50, 2, [stream], extra=[(b"tRNS", bytes(6)), (b"pHYs", bytes(9))])
    k = anc.index(b"pHYs") + 13
    assert png.parse_png(anc[:k] + bytes([anc[k] ^ 1]) + anc[k + 1:])["stream"] == stream


# -------------------------------------------------------------------------------------------------------------- 4. the ABI
def test_abi_entries():
    from gflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n in (("gfl_png_decode_workspace_bytes", 4), ("gfl_png_decode", 12)):
        args = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(args.split(",")) == n == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["gfl_png_decode_workspace_bytes"][0] is ctypes.c_size_t
    assert "gfl_png_dec.hip" in open(os.path.join(ROOT, "gflow_amd", "csrc", "Makefile")).read()
    assert "#define GFL_VERSION 312" in hdr
    core = open(os.path.join(ROOT, "gflow_amd", "csrc", "gfl_inflate.hpp")).read()
    assert "hip/" not in core and "__host__ __device__" in core             # one source for hipcc and a host compiler
    for k, name in enumerate(("OK", "INPUT_END", "BAD_HEADER", "BLOCK_TYPE", "STORED_LEN", "TOO_MANY_CODES", "BAD_REPEAT",
                              "BAD_CODE", "NO_END_OF_BLOCK", "BAD_SYMBOL", "FAR_DISTANCE", "OUTPUT_SIZE", "BAD_ADLER",
                              "BAD_FILTER")):
        assert re.search(r"#define GFL_PNG_%s %d\b" % (name, k), hdr) and re.search(r"\b%s = %d\b" % (name, k), core), name
        assert getattr(R, name) == k


def test_refused_arguments_without_a_device():
    from gflow_amd import _lib
    lib = _lib.load()
    ws = lib.gfl_png_decode_workspace_bytes
    assert ws(1, 3, 854, 480) >= 480 * (1 + 3 * 854) and ws(2, 3, 854, 480) >= 2 * ws(1, 3, 854, 480) - 256
    assert ws(1, 1, 1, 1) > 0 and ws(3, 4, 9, 6) >= 3 * 6 * 37
    need = ws(2, 3, 17, 9)
    buf = (ctypes.c_uint64 * 512)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)

    def call(data=p, n_bytes=64, offsets=p, T=2, bpp=3, W=17, H=9, images=p, status=p, w=p, size=need):
        return lib.gfl_png_decode(data, n_bytes, offsets, T, bpp, W, H, images, status, w, size, null)

    for bad in (dict(T=0), dict(bpp=0), dict(bpp=5), dict(W=0), dict(H=0), dict(T=-1), dict(W=1 << 30, H=4)):
        shape = dict(dict(T=2, bpp=3, W=17, H=9), **bad)
        assert ws(shape["T"], shape["bpp"], shape["W"], shape["H"]) == 0, bad
        assert call(**bad, size=1 << 40) == -1, bad
    for kw in (dict(data=null), dict(offsets=null), dict(images=null), dict(status=null), dict(w=null), dict(n_bytes=-1)):
        assert call(**kw) == -1, kw
    assert call(size=need - 1) == -2 and call(size=0) == -2
    assert not any(buf)


def test_no_cpu_path(monkeypatch):
    from gflow_amd import png
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for kw in (dict(), dict(device="cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            png.decode_png([pil_file("smooth", 1, 1, "L", 0)], **kw)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            png.decode_png([], **kw)


# ------------------------------------------------------------------------------------------------------- 5. the harness
@functools.lru_cache(maxsize=None)
def harness():
    """the sanitized host build of the decode core, made once per session; None without g++"""
    gxx = shutil.which("g++")
    if gxx is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="gfl_png_dec_"), "png_dec_host")
    res = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                          os.path.join(ROOT, "tools", "png_dec_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def run_harness(streams, W, H, bpp):
    """((T, H, W, bpp) uint8, status [T]) from the stand-alone program: exit 0 and a silent sanitizer, or the test fails"""
    exe = harness()
    if exe is None:
        pytest.skip("no g++")
    T = len(streams)
    off = np.cumsum([0] + [len(s) for s in streams], dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "in"), "wb") as f:
            f.write(b"GPD1" + struct.pack("<4iq", T, bpp, W, H, int(off[-1])) + off.tobytes() + b"".join(streams))
        res = subprocess.run([exe, os.path.join(tmp, "in"), os.path.join(tmp, "out")], capture_output=True, text=True)
        assert res.returncode == 0 and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
        out = open(os.path.join(tmp, "out"), "rb").read()
    n = T * H * W * bpp
    assert len(out) == n + 4 * T
    return np.frombuffer(out, np.uint8, n).reshape(T, H, W, bpp), np.frombuffer(out[n:], np.int32)


# stacks of T = 3 whose codes differ: stored, dynamic and PIL's optimised filters
def good_stack(H, W, mode):
    return [pil_file("photo", H, W, mode, 0), pil_file("noise", H, W, mode, 2), pil_file("smooth", H, W, mode, 3)]


@pytest.mark.parametrize("H,W,mode", [(1, 1, "L"), (1, 300, "RGBA"), (65, 3, "LA"), (50, 70, "RGB"), (50, 70, "P"),
                                       (200, 300, "RGB")])
def test_harness_decodes_good_files_exactly(H, W, mode):
    files = good_stack(H, W, mode) if H < 200 else [pil_file("noise", 200, 300, "RGB", 4), pil_file("photo", 200, 300, "RGB", 0),
                                                     pil_file("smooth", 200, 300, "RGB", 1)]
    images, status = run_harness([R.parse(f)["stream"] for f in files], W, H, MODES[mode])
    assert not status.any()
    for t, f in enumerate(files):
        assert np.array_equal(images[t], as_hwc(pil_pixels(f))), t


@pytest.mark.parametrize("mode", list(MODES))
def test_harness_decodes_the_large_grid_exactly(mode):
    """the whole cross of content and PIL setting at 200 x 300, one call per mode, against PIL"""
    files = [pil_file(*c) for c in GRID_LARGE if c[3] == mode]
    assert len(files) == 25
    images, status = run_harness([R.parse(f)["stream"] for f in files], 300, 200, MODES[mode])
    assert not status.any()
    for t, f in enumerate(files):
        assert np.array_equal(images[t], as_hwc(pil_pixels(f))), t


def test_harness_decodes_handmade_files_exactly():
    for name, data, want in handmade_files():
        p = R.parse(data)
        images, status = run_harness([p["stream"]], p["W"], p["H"], p["bpp"])
        assert status.tolist() == [0] and np.array_equal(images[0], want), name


@functools.lru_cache(maxsize=None)
def checked_mutation(i):
    """Set i of mutation_sets through the host harness, held to the reference: (images, status) as every implementation of
    the contract must give them -- the program exits 0 with a silent sanitizer, its status array EQUALS the reference's,
    entry for entry, and its images the reference's, pixel for pixel: zeros where the status is not 0.  A set is run on the
    GPU only after it has passed here."""
    s = mutation_sets()[i]
    images, status = run_harness(s["streams"], s["W"], s["H"], s["bpp"])
    want_images, want_status = reference_of_set(s)
    assert np.array_equal(status, want_status), (s["name"], status.tolist(), want_status.tolist())
    assert np.array_equal(images, want_images), s["name"]
    assert not images[status != 0].any()
    return images, status


@pytest.mark.parametrize("i", range(N_SETS))
def test_harness_on_malformed_streams(i):
    images, status = checked_mutation(i)
    assert status[-1] == 0 and images[-1].any() == (mutation_sets()[i]["name"][:4] != "ihdr")


# --------------------------------------------------------------------------------------------------------- 6. the loader
def test_loader_options(tmp_path):
    from gflow_amd import io as gio
    from gflow_amd import fit_video
    assert gio._OPTIONS["decode"] == ("host", "device", "device-all")
    with pytest.raises(ValueError, match="needs device"):
        gio.load_sequence(str(tmp_path / "seq"), decode="device-all")
    with pytest.raises(ValueError, match="needs device"):
        gio.load_sequence(str(tmp_path / "seq"), decode="device")
    with pytest.raises(ValueError, match="decode must be"):
        gio.load_sequence(str(tmp_path / "seq"), decode="gpu")
    ap = fit_video._parser()
    assert ap.parse_args([]).decode == "host" and ap.parse_args(["--decode", "device-all"]).decode == "device-all"
    with pytest.raises(SystemExit):
        ap.parse_args(["--decode", "all"])
