"""CPU: decoding video files -- the numpy reference (tests/jpeg_dec_ref.py) against PIL, bit for bit; ``video.parse_jpeg``
against the reference's parser and its refusals; the decode core (csrc/gfl_jpeg_dec.hpp) on the CPU under the address and
undefined-behaviour sanitizers (tools/jpeg_dec_host.cpp, a stand-alone program run as a subprocess) on good and on malformed
files; the loader's path logic.  Also holds the inputs the GPU tests (tests/test_gpu_jpeg_dec.py) share."""
import ctypes
import functools
import io
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_dec_ref as R
from tests.test_video_host import content

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"grey": None, "444": 0, "422": 1, "420": 2}


# ------------------------------------------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def pil_file(kind, H, W, mode, q, optimize=False, rmb=0, seed=0):
    """a JPEG file as PIL writes it: ``mode`` of MODES, ``rmb``: restart_marker_blocks (0: no DRI)"""
    img = content(kind, H, W, 1 if mode == "grey" else 3, seed)
    kw = dict(quality=q, optimize=optimize)
    if mode != "grey":
        kw["subsampling"] = MODES[mode]
    if rmb:
        kw["restart_marker_blocks"] = rmb
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def as_hwc(a):
    return a[..., None] if a.ndim == 2 else a


def stack_arrays(files):
    """(units, tables, bytes, shape dict) of a stack as video.decode_jpeg passes it to the library"""
    from gflow_amd import video
    parsed = [video.parse_jpeg(f, f"frame {t}") for t, f in enumerate(files)]
    p = parsed[0]
    units, tables, data = video.decode_arrays(files, parsed)
    return units, tables, data, dict(T=len(files), C=p["components"], W=p["width"], H=p["height"], hs=p["hs"], vs=p["vs"])


def reference_from_arrays(units, tables, data, shape):
    """the reference on the arrays of a call: ((T, H, W, C) uint8, status per unit), unit records checked as the header says"""
    T, C, W, H, hs, vs = (shape[k] for k in "T C W H hs vs".split())
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    blob = bytes(np.asarray(data, dtype=np.uint8))
    images = np.zeros((T, H, W, C), dtype=np.uint8)
    status = np.full(len(units), -1, dtype=np.int32)
    for t in range(T):
        ft = tables[t]
        comps = [(c, hs if c == 0 else 1, vs if c == 0 else 1, int(ft["qsel"][c])) for c in range(C)]
        sel = [(int(ft["dcsel"][c]), int(ft["acsel"][c])) for c in range(C)]
        huff = {(k >> 1, k & 1): (ft["huff"][k]["bits"].tolist(), ft["huff"][k]["vals"].tolist()) for k in range(4)}
        quant = {i: ft["q"][i].tolist() for i in range(4)}
        first, n = int(ft["first_unit"]), int(ft["n_units"])
        mine = [(int(u["first_mcu"]), int(u["n_mcu"]), int(u["offset"]), int(u["n_bytes"])) if int(u["frame"]) == t else
                (-1, 0, 0, 0) for u in units[first:first + n]]
        planes, st = R.decode_units(blob, mine, comps, sel, huff, mx, my)
        status[first:first + n] = st
        images[t] = as_hwc(R.pixels(planes, comps, quant, H, W))
    return images, status


# the thinned grid of the reference-against-PIL check: (kind, H, W, mode, quality, optimize, restart_marker_blocks)
def _grid():
    out = []
    for H, W in ((1, 1), (17, 23), (16, 17), (50, 70)):
        for mode in MODES:
            out.append(("smooth", H, W, mode, 30, False, 0))
            out.append(("noise", H, W, mode, 100, True, 0))
            out.append(("checker", H, W, mode, 90, False, 3))
    out.append(("noise", 50, 70, "444", 100, False, 3))
    out.append(("checker", 17, 23, "420", 100, True, 1))
    return out


GRID = _grid()


@pytest.mark.parametrize("mode", list(MODES))
def test_reference_is_pil_bit_for_bit(mode):
    """The acceptance criterion rests on this: the restated arithmetic equals libjpeg's default decode path exactly.  Not to
    be loosened -- a PIL build that breaks it is named here by its first differing case."""
    n = 0
    for case in GRID:
        if case[3] != mode:
            continue
        data = pil_file(*case)
        want, got = pil_pixels(data), R.decode(data)
        assert got.shape == want.shape and np.array_equal(got, want), (case, int(np.abs(got.astype(int) - want).max()))
        n += 1
    assert n >= 12
    if mode == "444":
        p = R.parse(pil_file("noise", 50, 70, "444", 100, False, 3))
        assert len(p["units"]) == 21 and p["dri"] == 3                     # the RST counter wraps past 7


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_entries_and_struct_mirrors():
    from gflow_amd import _lib, video
    hdr = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, n in (("gfl_jpeg_decode_workspace_bytes", 7), ("gfl_jpeg_decode", 16), ("gfl_jpeg_decode_struct_bytes", 2)):
        args = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(args.split(",")) == n == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["gfl_jpeg_decode_workspace_bytes"][0] is ctypes.c_size_t
    assert "gfl_jpeg_dec.hip" in open(os.path.join(ROOT, "gflow_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    a, b = ctypes.c_int(), ctypes.c_int()
    assert lib.gfl_jpeg_decode_struct_bytes(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (video.UNIT_DTYPE.itemsize, video.TABLES_DTYPE.itemsize) == (24, 1364)
    core = open(os.path.join(ROOT, "gflow_amd", "csrc", "gfl_jpeg_dec.hpp")).read()
    assert "hip/" not in core and "__host__ __device__" in core             # one source for hipcc and a host compiler


def test_refused_arguments_without_a_device():
    from gflow_amd import _lib
    lib = _lib.load()
    ws = lib.gfl_jpeg_decode_workspace_bytes
    good = dict(T=2, C=3, W=17, H=9, hs=2, vs=2)
    assert 0 < ws(1, 3, 854, 480, 2, 2, 60) < ws(2, 3, 854, 480, 2, 2, 60)
    assert ws(1, 1, 1, 1, 1, 1, 1) > 0 and ws(1, 3, 65535, 65535, 1, 1, 1) > 0
    need = ws(*good.values(), 4)
    buf = (ctypes.c_uint64 * 512)()
    p, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)

    def call(data=p, n_bytes=64, units=p, n_units=4, tables=p, images=p, status=p, w=p, size=need, **shape):
        s = dict(good, **shape)
        return lib.gfl_jpeg_decode(data, n_bytes, units, n_units, tables, s["T"], s["C"], s["W"], s["H"], s["hs"], s["vs"], images,
                                   status, w, size, null)

    for bad in (dict(T=0), dict(C=2), dict(C=4), dict(W=0), dict(H=65536), dict(hs=1, vs=2), dict(hs=2, vs=4), dict(hs=4, vs=1),
                dict(C=1), dict(hs=0), dict(T=1 << 20, W=8192, H=8192)):
        assert ws(*dict(good, **bad).values(), 4) == 0, bad
        assert call(**bad, size=1 << 40) == -1, bad
    assert ws(*good.values(), 0) == 0
    for kw in (dict(data=null), dict(units=null), dict(tables=null), dict(images=null), dict(status=null), dict(w=null),
               dict(n_units=0), dict(n_bytes=-1)):
        assert call(**kw) == -1, kw
    assert call(size=need - 1) == -2 and call(size=0) == -2
    assert not any(buf)


def test_no_cpu_path(monkeypatch):
    from gflow_amd import video
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video.decode_jpeg([pil_file("smooth", 8, 8, "444", 90)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        video.decode_jpeg([pil_file("smooth", 8, 8, "444", 90)], device="cpu")


# --------------------------------------------------------------------------------------------------------- parse_jpeg
@pytest.mark.parametrize("case", [("smooth", 17, 23, "420", 30, False, 0), ("noise", 16, 17, "422", 100, True, 0),
                                  ("noise", 50, 70, "444", 100, False, 3), ("checker", 1, 1, "grey", 90, False, 3),
                                  ("smooth", 33, 31, "grey", 75, True, 2)])
def test_parse_jpeg_against_the_references_parser(case):
    from gflow_amd import video
    data = pil_file(*case)
    p, r = video.parse_jpeg(data), R.parse(data)
    assert (p["width"], p["height"], p["components"]) == (r["W"], r["H"], len(r["comps"]))
    assert p["sampling"] == [(h, v) for _, h, v, _ in r["comps"]] and (p["hs"], p["vs"]) == p["sampling"][0]
    assert p["component_ids"] == [c[0] for c in r["comps"]] and p["qsel"] == [c[3] for c in r["comps"]]
    assert list(zip(p["dcsel"], p["acsel"])) == r["sel"] and p["dri"] == r["dri"] == case[6]
    assert sorted(p["quant"]) == sorted(r["quant"]) and all(p["quant"][k].tolist() == r["quant"][k] for k in r["quant"])
    assert sorted(p["huffman"]) == sorted(r["huff"])
    for k, (bits, vals) in r["huff"].items():
        assert list(p["huffman"][k][0]) == bits and list(p["huffman"][k][1]) == vals
    assert p["scan"] == r["scan"] and data[p["scan"][1]:p["scan"][1] + 2] == b"\xff\xd9"
    assert p["mcus"] == (r["mx"], r["my"]) and [tuple(u) for u in p["units"].tolist()] == r["units"]
    assert sum(u[1] for u in r["units"]) == r["mx"] * r["my"]
    assert p["jfif"] is True and p["adobe_transform"] is None


def _segments(data):
    """[(marker, start of the FF, end)] of the header segments up to and including SOS"""
    pos, out = 2, []
    while True:
        m, n = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        out.append((m, pos, pos + 2 + n))
        pos += 2 + n
        if m == 0xDA:
            return out


def _patched(data, marker, offset, value, nth=0):
    """``data`` with payload byte ``offset`` of the nth segment of ``marker`` set to ``value``"""
    at = [s for s in _segments(data) if s[0] == marker][nth][1] + 4 + offset
    return data[:at] + bytes([value]) + data[at + 1:]


def _without(data, marker):
    for m, a, b in _segments(data):
        if m == marker:
            return data[:a] + data[b:]
    raise KeyError(marker)


def _saved(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="JPEG", **kw)
    return buf.getvalue()


def test_parse_jpeg_refuses_what_is_out_of_scope():
    from gflow_amd import video
    rgb = Image.fromarray(np.asarray(content("smooth", 24, 24)))
    good = pil_file("smooth", 24, 24, "422", 90)
    rst = pil_file("noise", 50, 70, "444", 100, False, 3)
    sof = [s for s in _segments(good) if s[0] == 0xC0][0][1]
    sos = [s for s in _segments(good) if s[0] == 0xDA][0]
    one_scan = good[:sos[1]] + b"\xff\xda" + struct.pack(">H", 8) + bytes([1, 1, 0x00, 0, 63, 0]) + good[sos[2]:]
    adobe = lambda t: good[:2] + b"\xff\xee" + struct.pack(">H", 14) + b"Adobe\0\x64\0\0\0\0" + bytes([t]) + good[2:]
    as_rgb = _without(good, 0xE0)
    for c, ch in enumerate(b"RGB"):
        as_rgb = _patched(_patched(as_rgb, 0xC0, 6 + 3 * c, ch), 0xDA, 1 + 2 * c, ch)
    cases = {
        "progressive": (_saved(rgb, progressive=True), "progressive"),
        "cmyk": (_saved(rgb.convert("CMYK")), "4 components"),
        "arithmetic": (good[:sof + 1] + b"\xc9" + good[sof + 2:], "arithmetic"),
        "12 bit": (_patched(good, 0xC0, 0, 12), "12-bit"),
        "16-bit dqt": (_patched(good, 0xDB, 0, 0x10), "16-bit quantisation"),
        "1x2": (_patched(good, 0xC0, 7, 0x12), "sampling"),
        "4x1": (_patched(good, 0xC0, 7, 0x41), "sampling"),
        "chroma 2x1": (_patched(good, 0xC0, 10, 0x21), "sampling"),
        "several scans": (one_scan, "several scans"),
        "adobe transform 0": (adobe(0), "Adobe"),
        "adobe transform 2": (adobe(2), "Adobe"),
        "rgb ids": (as_rgb, "R, G, B"),
        "rst order": (rst.replace(b"\xff\xd1", b"\xff\xd3", 1), "restart markers"),
        "rst without dri": (_without(rst, 0xDD), "without DRI"),
        "huffman id 2": (_patched(good, 0xC4, 0, 0x02), "Huffman table"),
        "not a jpeg": (b"RIFF" + good[4:], "SOI"),
        "headers only": (good[:sos[1]], "no scan"),
    }
    for name, (data, why) in cases.items():
        with pytest.raises(ValueError, match=why) as e:
            video.parse_jpeg(data, "the file " + name)
        assert "the file " + name in str(e.value), name
    assert rst.count(b"\xff\xd1") >= 1 and video.parse_jpeg(adobe(1))["adobe_transform"] == 1
    # a scan cut short is NOT refused here: its intervals are listed, the missing ones empty, and the decoder reports them
    scan = video.parse_jpeg(rst)["scan"]
    cut = video.parse_jpeg(rst[:scan[0] + 40] + b"\xff\xd9")
    assert len(cut["units"]) == 21 and cut["units"][-1][3] == 0 and cut["units"][:, 3].sum() <= 40


# -------------------------------------------------------------------------------------------------------- the harness
@functools.lru_cache(maxsize=None)
def harness():
    """the sanitized host build of the decode core, made once per session; None without g++"""
    gxx = shutil.which("g++")
    if gxx is None:
        return None
    exe = os.path.join(tempfile.mkdtemp(prefix="gfl_jpeg_dec_"), "jpeg_dec_host")
    res = subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                          os.path.join(ROOT, "tools", "jpeg_dec_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def run_harness(units, tables, data, shape):
    """((T, H, W, C) uint8, status) from the stand-alone program: exit 0 and a silent sanitizer, or the test fails"""
    exe = harness()
    if exe is None:
        pytest.skip("no g++")
    T, C, W, H, hs, vs = (shape[k] for k in "T C W H hs vs".split())
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "in"), "wb") as f:
            f.write(b"GJD1" + struct.pack("<6i2q", T, C, W, H, hs, vs, len(units), len(data)))
            f.write(np.ascontiguousarray(units).tobytes() + np.ascontiguousarray(tables).tobytes() + np.asarray(data, np.uint8).tobytes())
        res = subprocess.run([exe, os.path.join(tmp, "in"), os.path.join(tmp, "out")], capture_output=True, text=True)
        assert res.returncode == 0 and "Sanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-2000:]
        out = open(os.path.join(tmp, "out"), "rb").read()
    n = T * H * W * C
    assert len(out) == n + 4 * len(units)
    return np.frombuffer(out, np.uint8, n).reshape(T, H, W, C), np.frombuffer(out, np.int32, len(units), n)


# stacks of T = 3 whose tables differ: content and optimize=True change the DHTs, the qualities the DQTs
def good_stack(H, W, mode, rmb):
    return [pil_file("smooth", H, W, mode, 90, False, rmb), pil_file("noise", H, W, mode, 100, True, rmb),
            pil_file("checker", H, W, mode, 30, False, rmb)]


@pytest.mark.parametrize("H,W,mode,rmb", [(1, 1, "grey", 0), (17, 23, "420", 0), (16, 17, "422", 1), (33, 31, "444", 3),
                                           (50, 70, "420", 2), (8, 8, "444", 0), (33, 31, "grey", 3)])
def test_harness_decodes_good_files_exactly(H, W, mode, rmb):
    files = good_stack(H, W, mode, rmb)
    units, tables, data, shape = stack_arrays(files)
    images, status = run_harness(units, tables, data, shape)
    assert not status.any()
    for t, f in enumerate(files):
        assert np.array_equal(images[t], as_hwc(R.decode(f))), t


# ---- malformed input, shared with the device test
BASE_A = ("smooth", 50, 70, "444", 90, False, 3)        # 63 MCUs of one block per component, 21 units
BASE_B = ("noise", 33, 31, "420", 75, False, 0)         # one unit
N_FLIPS = 10                                            # per base file: 20 seeded positions in all


def _with_scan(data, scan):
    from gflow_amd import video
    a, _ = video.parse_jpeg(data)["scan"]
    return data[:a] + scan + b"\xff\xd9"


def _truncated(data, n):
    from gflow_amd import video
    a, b = video.parse_jpeg(data)["scan"]
    while n > 0 and data[a + n - 1] == 0xFF:            # (a cut behind an FF would leave a marker of its own making)
        n -= 1
    return _with_scan(data, data[a:a + n])


def _code_removed(data):
    """the file with the FIRST (shortest, most used) code of AC table 0 taken out of its DHT segment: every later code moves"""
    for m, a, b in _segments(data):
        if m == 0xC4 and data[a + 4] == 0x10:
            bits, vals = bytearray(data[a + 5:a + 21]), data[a + 21:b]
            first = next(i for i, n in enumerate(bits) if n)
            bits[first] -= 1
            seg = bytes([0x10]) + bytes(bits) + vals[1:]
            return data[:a] + b"\xff\xc4" + struct.pack(">H", len(seg) + 2) + seg + data[b:]
    raise KeyError("no DHT segment of AC table 0 on its own")


@functools.lru_cache(maxsize=None)
def mutation_sets():
    """[dict(name, files -- the mutated files of the call, or None where only the arrays can say it; arrays -- (units, tables,
    bytes, shape); refused -- [(name, bytes)] the host refuses; all_fail -- must every frame report a unit?; flipped -- the
    absolute byte per frame, or None)]: the malformed inputs of the issue, made once."""
    from gflow_amd import video
    sets = []
    for tag, base in (("A", BASE_A), ("B", BASE_B)):
        good = pil_file(*base)
        a, b = video.parse_jpeg(good)["scan"]
        files = [_truncated(good, 0), _truncated(good, 1), _truncated(good, (b - a) // 2)]
        sets.append(dict(name=f"truncated {tag}", files=files, arrays=stack_arrays(files), refused=[], all_fail=True, flipped=None))
        rng = np.random.default_rng([7, ord(tag)])
        files, refused, where = [], [], []
        for at in sorted(int(v) for v in rng.choice(np.arange(a, b), size=N_FLIPS, replace=False)):
            f = good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:]
            try:
                video.parse_jpeg(f)
                files.append(f)
                where.append(at)
            except ValueError:
                refused.append((f"{tag} byte {at}", f))
        sets.append(dict(name=f"flipped {tag}", files=files, arrays=stack_arrays(files), refused=refused, all_fail=False,
                         flipped=where))
        files = [good, _code_removed(good)]
        sets.append(dict(name=f"huffman code removed {tag}", files=files, arrays=stack_arrays(files), refused=[], all_fail=False,
                         flipped=None))
    units, tables, data, shape = stack_arrays([pil_file(*BASE_A)])
    units = units.copy()
    units["n_mcu"][5] += 1                          # runs into unit 6's first MCU
    units["n_mcu"][20] += 1                         # runs out of the frame
    sets.append(dict(name="mcu count raised", files=None, arrays=(units, tables, data, shape), refused=[], all_fail=True,
                     flipped=None))
    return sets


@functools.lru_cache(maxsize=None)
def checked_mutation(i):
    """Set i of mutation_sets through the host harness, held to the reference: (images, status) as every implementation of
    the contract must give them.  What is asserted, and why it is not "every mutated file has a non-zero status": a byte
    flipped inside the extra bits of a coefficient leaves a well-formed stream that merely says other values -- no decoder
    can tell.  So: the program exits 0 with a silent sanitizer; its status array EQUALS the reference's, entry for entry,
    and its image the reference's, pixel for pixel (units are independent, so every unit whose bytes were not touched is
    decoded exactly); truncations, the table with a code removed and the raised MCU counts must show non-zero entries; and
    of the 20 flips at least one must, the rest either do or decode, without error, to what the reference decodes."""
    s = mutation_sets()[i]
    units, tables, data, shape = s["arrays"]
    images, status = run_harness(units, tables, data, shape)
    want_images, want_status = reference_from_arrays(units, tables, data, shape)
    assert np.array_equal(status, want_status), (s["name"], status.tolist(), want_status.tolist())
    assert np.array_equal(images, want_images), s["name"]
    return images, status


@pytest.mark.parametrize("i", range(7))
def test_harness_on_malformed_files(i):
    from gflow_amd import video
    s = mutation_sets()[i]
    units, tables, data, shape = s["arrays"]
    images, status = checked_mutation(i)
    frame_fails = [bool(status[int(ft["first_unit"]):int(ft["first_unit"]) + int(ft["n_units"])].any()) for ft in tables]
    print(s["name"], "status", status.tolist(), "refused on the host:", [n for n, _ in s["refused"]])
    if s["all_fail"]:
        assert all(frame_fails)
    if s["name"].startswith("huffman"):
        assert frame_fails == [False, True]
        assert np.array_equal(images[0], as_hwc(R.decode(s["files"][0])))            # the good frame beside it is exact
    if s["name"].startswith("flipped"):
        assert len(s["files"]) + len(s["refused"]) == N_FLIPS
        assert any(frame_fails) or s["refused"]
    if s["name"] == "flipped A":
        # 4:4:4: an MCU is one 8x8 block of pixels.  Every unit that reports no error and does not hold the flipped byte
        # shows exactly the good file's pixels.
        good = as_hwc(R.decode(pil_file(*BASE_A)))
        mx = -(-shape["W"] // 8)
        for t, at in enumerate(s["flipped"]):
            a = video.parse_jpeg(s["files"][t])["scan"][0]
            first = int(tables[t]["first_unit"])
            for k in range(int(tables[t]["n_units"])):
                u = units[first + k]
                lo = a + int(u["offset"]) - int(units[first]["offset"])
                if status[first + k] == 0 and not lo <= at < lo + int(u["n_bytes"]) + 2:
                    for m in range(int(u["first_mcu"]), int(u["first_mcu"]) + int(u["n_mcu"])):
                        y, x = 8 * (m // mx), 8 * (m % mx)
                        assert np.array_equal(images[t, y:y + 8, x:x + 8], good[y:y + 8, x:x + 8]), (t, k, m)
    if s["name"] == "mcu count raised":
        assert status[5] != 0 and status[20] == R.BAD_RECORD and not status[:5].any() and not status[6:20].any()
        good = as_hwc(R.decode(pil_file(*BASE_A)))
        # unit 5's own MCUs and unit 6 stand; only unit 20's (MCUs 60 .. 62: the last three blocks of the last row) are gone
        assert np.array_equal(images[0, :48], good[:48]) and np.array_equal(images[0, 48:, :48], good[48:, :48])
        assert not np.array_equal(images[0, 48:, 48:], good[48:, 48:])


# --------------------------------------------------------------------------------------------------------- the loader
def test_loader_options_and_avi_paths(tmp_path):
    from gflow_amd import io as gio
    from gflow_amd import fit_video, video
    with pytest.raises(ValueError, match="needs device"):
        gio.load_sequence(str(tmp_path / "seq"), decode="device")
    with pytest.raises(ValueError, match="decode must be"):
        gio.load_sequence(str(tmp_path / "seq"), decode="gpu")
    clip = str(tmp_path / "clip.avi")
    with video.AviWriter(clip, 8, 8, 5) as avi:
        for k in range(5):
            avi.add(pil_file("smooth", 8, 8, "444", 90, seed=k))
    for d in ("_flow_unimatch", "_epipolar", "_depth_mast3r_s2", "_camera_mast3r_s2"):
        os.makedirs(str(tmp_path / "clip") + d)
    for k in range(4):
        open(str(tmp_path / "clip_flow_unimatch" / f"{k:05d}_pred.flo"), "wb").close()
        open(str(tmp_path / "clip_epipolar" / f"{k:05d}_open.png"), "wb").close()
    assert gio.is_video(clip) and not gio.is_video(str(tmp_path / "clip")) and not gio.is_video(str(tmp_path / "none.avi"))
    os.makedirs(str(tmp_path / "folder.avi"))
    assert not gio.is_video(str(tmp_path / "folder.avi"))
    p = gio.sequence_paths(clip)
    assert [f.name for f in p["img"]] == [f"frame_{k:05d}" for k in range(4)]           # frame_range -1: all but the last
    assert all(f.path == clip for f in p["img"]) and [f.index for f in p["img"]] == [0, 1, 2, 3]
    assert [os.path.basename(str(f)) for f in p["flow"]] == [f"{k:05d}_pred.flo" for k in range(4)]
    assert str(p["flow"][0].parent) == str(tmp_path / "clip_flow_unimatch") and len(p["move"]) == 4 and p["depth"] == []
    cut = gio.sequence_paths(clip, frame_start=1, frame_range=4, skip_interval=2)
    assert [f.name for f in cut["img"]] == ["frame_00001", "frame_00003"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gio.load_sequence(clip)
    ap = fit_video._parser()
    assert ap.parse_args([]).decode == "host" and ap.parse_args(["--decode", "device"]).decode == "device"
    with pytest.raises(SystemExit):
        video.main(["--out", "x"])                                                       # neither --frames nor --unpack
