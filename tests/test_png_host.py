"""CPU: the PNG container, the strip rule and the restatement the device's stream is held against (tests/png_ref.py)."""
import io
import os
import re
import zlib

import numpy as np
import pytest
from PIL import Image

from gflow_amd import _lib
from gflow_amd import png as P
from tests import png_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gfl_png_strip_rows", "gfl_png_workspace_bytes", "gfl_png_sizes", "gfl_png_emit"]
SHAPES = [(1, 1), (3, 5), (37, 61)]
PALETTE = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], -1).astype(np.uint8)


def pil_pixels(data):
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", ["grey", "rgb", "palette"])
def test_chunks_around_the_reference_stream_round_trip_through_pil(kind, H, W):
    C = 3 if kind == "rgb" else 1
    img = R.content("smooth", H, W, C, seed=H)
    data = P.png_chunks(R.reference_stream(img), W, H, C, PALETTE if kind == "palette" else None)
    im = pil_pixels(data)
    assert im.size == (W, H)
    assert im.mode == {"grey": "L", "rgb": "RGB", "palette": "P"}[kind]
    got = np.asarray(im)
    assert np.array_equal(got.reshape(H, W, C), img)
    if kind == "palette":
        assert np.array_equal(np.asarray(im.convert("RGB")), PALETTE[img[:, :, 0]])


def test_chunks_refuse_what_a_png_cannot_hold():
    with pytest.raises(ValueError):
        P.png_chunks(b"", 4, 4, 2)
    with pytest.raises(ValueError):
        P.png_chunks(b"", 0, 4, 1)
    with pytest.raises(ValueError):
        P.png_chunks(b"", 4, 4, 3, PALETTE)
    with pytest.raises(ValueError):
        P.png_chunks(b"", 4, 4, 1, PALETTE.astype(np.int32))
    with pytest.raises(ValueError):
        P.encode_png(np.zeros((2, 4, 4, 3), np.float32))
    with pytest.raises(ValueError):
        P.encode_png(np.zeros((2, 4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        P.encode_png(np.zeros((2, 2, 4, 4, 3), np.uint8))


def test_adler_combine_equals_the_adler_of_the_whole():
    rng = np.random.default_rng(0)
    for n1, n2 in [(1, 1), (5, 70000), (32768, 32768), (65521, 3), (100000, 1)]:
        a, b = rng.integers(0, 256, n1, dtype=np.uint8).tobytes(), rng.integers(200, 256, n2, dtype=np.uint8).tobytes()
        assert R.adler_combine(zlib.adler32(a), zlib.adler32(b), n2) == zlib.adler32(a + b)
    img = R.content("noise", 480, 854, 3)
    assert R.reference_stream(img)[-4:] == zlib.adler32(R.filtered_bytes(img)).to_bytes(4, "big")


def test_strip_rows_is_the_formula_and_needs_no_device():
    lib = _lib.load()
    assert lib.gfl_png_strip_rows(3, 854) == 12
    assert lib.gfl_png_strip_rows(1, 854) == 38
    assert lib.gfl_png_strip_rows(3, 11000) == 0
    for C in (0, 1, 2, 3, 4):
        for W in (-1, 0, 1, 2, 5, 61, 170, 255, 256, 511, 512, 854, 4181, 10922, 10923, 32767, 32768, 1 << 30):
            assert lib.gfl_png_strip_rows(C, W) == R.strip_rows(C, W), (C, W)
            assert P.strip_rows(C, W) == R.strip_rows(C, W)
    # a strip's filtered bytes fit in 32 KiB
    for C in (1, 3):
        for W in (1, 2, 170, 854, 4181, 10922):
            assert 0 < R.strip_rows(C, W) * (1 + W * C) <= 32768


def test_workspace_query_refuses_bad_arguments():
    lib = _lib.load()
    assert lib.gfl_png_workspace_bytes(2, 3, 854, 480) > 0
    assert lib.gfl_png_workspace_bytes(2, 2, 854, 480) == 0          # C = 2
    assert lib.gfl_png_workspace_bytes(2, 3, 0, 480) == 0            # W = 0
    assert lib.gfl_png_workspace_bytes(0, 3, 854, 480) == 0          # T = 0
    assert lib.gfl_png_workspace_bytes(2, 3, 854, 0) == 0
    assert lib.gfl_png_workspace_bytes(2, 3, 11000, 480) == 0        # one filtered row does not fit
    # and the two calls say so before any launch
    assert lib.gfl_png_sizes(None, 1, 3, 8, 8, None, None, 0, None) == -1
    assert lib.gfl_png_emit(None, 1, 3, 8, 8, None, 0, None, 0, None) == -1


def test_header_and_binding_list_the_entries():
    text = open(os.path.join(ROOT, "include", "gflow_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in _lib.SIGNATURES
        assert name in text.split("#define GFL_VERSION")[0], f"{name} is not in the version comment"
    assert re.search(r"^#define GFL_VERSION 312$", text, flags=re.M) and _lib.MIN_VERSION == 312
    assert "gfl_png.hip" in open(os.path.join(ROOT, "gflow_amd", "csrc", "Makefile")).read()


def test_run_tokens_restate_the_bytes():
    # run lengths 1 .. 3, around 258 and around 2 x 258 + 1, back to back
    lengths = [1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 516, 517, 518, 519, 520, 1]
    data = b"".join(bytes([k + 1]) * l for k, l in enumerate(lengths))
    tokens = R.run_tokens(data)
    assert R.expand_tokens(tokens) == data
    assert all(3 <= v <= 258 for kind, v in tokens if kind == "match")
    by_run = {2: ["lit", "lit"], 3: ["lit", "lit", "lit"], 4: ["lit", "match"], 259: ["lit", "match"], 260: ["lit", "match", "lit"],
              261: ["lit", "match", "lit", "lit"], 262: ["lit", "match", "match"]}
    for l, kinds in by_run.items():
        assert [k for k, _ in R.run_tokens(b"\x07" * l)] == kinds, l
    for length in range(3, 259):
        sym, eb, extra = R.length_code(length)
        assert 257 <= sym <= 285 and 0 <= extra < (1 << eb) if eb else extra == 0


def test_fibonacci_content_is_deeper_than_fifteen():
    row = R.fibonacci_row()
    assert row.shape == (1, 4181) and len(np.unique(row)) == 18
    assert (row[0, 1:] != row[0, :-1]).all()                        # no value repeats, let alone three times
    assert R.strip_rows(1, 4181) >= 1
    hist = R.histogram(R.run_tokens(R.strips(row)[0]))
    assert max(R.huffman_depths(hist).values()) > 15
    lens = R.limited_lengths(hist, 15)
    assert max(lens) == 15 and sum(2.0 ** -l for l in lens if l) == 1.0


@pytest.mark.parametrize("name", ["smooth", "noise", "flat", "runs", "checker", "disc"])
def test_the_rules_of_the_library_make_a_stream_zlib_accepts(name):
    """tests/png_ref.model_stream restates the device's rules; zlib's inflate is the judge of the code builder's Kraft sums"""
    for H, W, C in [(1, 1, 1), (3, 5, 3), (37, 61, 1), (65, 300, 3)]:
        img = R.content(name, H, W, C)
        d = zlib.decompressobj()
        assert d.decompress(R.model_stream(img)) == R.filtered_bytes(img) and d.eof and d.unused_data == b""
        for s in R.strips(img):
            assert len(R.model_strip(s)) <= len(s) + 5
