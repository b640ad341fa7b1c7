"""GPU: the device's PNG coder (gfl_png_sizes / gfl_png_emit, gflow_amd.png) against PIL, zlib and tests/png_ref.py."""
import functools
import io
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from gflow_amd import _lib as L
from gflow_amd import png as P
from tests import png_ref as R

pytestmark = pytest.mark.gpu

STRIP_W = 1365                                     # 8 rows per strip with three channels, 23 with one
SHAPES = ["tiny", "odd", "strip-", "strip", "strip+", "wide"]
CONTENTS = ["smooth", "noise", "flat", "runs", "checker"]
PALETTE = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], -1).astype(np.uint8)


def shape_of(name, C):
    """(H, W): the smallest shapes that reach each branch, from the library's own strip rule"""
    rows = P.strip_rows(C, STRIP_W)
    return {"tiny": (1, 1), "odd": (37, 61), "strip-": (rows - 1, STRIP_W), "strip": (rows, STRIP_W),
            "strip+": (rows + 1, STRIP_W), "wide": (1, 4181)}[name]


@functools.lru_cache(maxsize=None)
def image(content, shape, C):
    if content == "fibonacci":
        assert (shape, C) == ("wide", 1)
        return R.fibonacci_row()[:, :, None]
    H, W = shape_of(shape, C)
    img = R.content(content, H, W, C, seed=3)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def encoded(content, shape, C):
    """(the PNG file, its zlib stream) of one image, coded alone"""
    img = image(content, shape, C)
    data, off = P.encode_streams(torch.from_numpy(img.copy())[None].cuda())
    assert off[0] == 0 and off[1] == len(data)
    stream = data.tobytes()
    return P.png_chunks(stream, img.shape[1], img.shape[0], C), stream


CASES = [(c, s, C) for c in CONTENTS for s in SHAPES for C in (1, 3)] + [("fibonacci", "wide", 1)]


def test_shapes_reach_the_branches():
    for C in (1, 3):
        rows = P.strip_rows(C, STRIP_W)
        assert rows == R.strip_rows(C, STRIP_W) and 2 <= rows < 64
        assert [len(R.strips(image("flat", s, C))) for s in ("strip-", "strip", "strip+")] == [1, 1, 2]
        assert (61 * C) % 4 != 0                                       # rows that are no multiple of four bytes
    assert len(R.strips(image("flat", "strip+", 3))[1]) == 1 + STRIP_W * 3       # a last strip of one row
    # the contents: runs longer than 258; run lengths 2, 3, 258 .. 261 back to back; a histogram deeper than 15
    flat = R.run_tokens(R.strips(image("flat", "strip", 1))[0])
    assert sum(1 for k, v in flat if k == "match" and v == 258) > 4
    runs = R.strips(image("runs", "strip", 1))[0]
    a = np.frombuffer(runs, np.uint8)[1:STRIP_W]
    lengths = np.diff(np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1], [True]])))
    assert lengths[:6].tolist() == [2, 3, 258, 259, 260, 261]
    fib = R.histogram(R.run_tokens(R.strips(image("fibonacci", "wide", 1))[0]))
    assert max(R.huffman_depths(fib).values()) > 15


@pytest.mark.parametrize("content,shape,C", CASES)
def test_pil_and_zlib_read_the_file(content, shape, C):
    img = image(content, shape, C)
    H, W = img.shape[:2]
    data, stream = encoded(content, shape, C)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.size == (W, H) and im.mode == ("RGB" if C == 3 else "L")
    assert np.array_equal(np.asarray(im).reshape(H, W, C), img)
    d = zlib.decompressobj()
    assert d.decompress(stream) == R.filtered_bytes(img)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    # the hard cap: a strip never takes more than a stored block
    strips = R.strips(img)
    cap = sum(len(s) + 5 for s in strips) + 8
    assert len(stream) <= cap
    if content == "noise":
        assert len(stream) == cap, "a strip of uniform bytes was not stored"
    if content in ("flat", "checker", "runs") and shape != "tiny":
        assert len(stream) < cap / 2


@pytest.mark.parametrize("content,shape,C", CASES)
def test_the_bytes_are_the_restated_rules(content, shape, C):
    """tests/png_ref.model_stream: the code builder, the length limiter and the table coding in plain Python"""
    assert encoded(content, shape, C)[1] == R.model_stream(image(content, shape, C))


def test_palette():
    idx = image("smooth", "odd", 1)
    data = P.encode_png(idx[:, :, 0], palette=PALETTE)
    assert len(data) == 1
    im = Image.open(io.BytesIO(data[0]))
    im.load()
    assert im.mode == "P" and np.array_equal(np.asarray(im), idx[:, :, 0])
    assert np.array_equal(np.asarray(im.convert("RGB")), PALETTE[idx[:, :, 0]])
    with pytest.raises(ValueError):
        P.encode_png(image("smooth", "odd", 3), palette=PALETTE)


def _raw_calls(stack, guard=64):
    """the two calls on a (T, H, W, C) device stack: (frame offsets, the out buffer with `guard` bytes of 0xA5 behind it)"""
    lib = L.load()
    T, H, W, C = (int(v) for v in stack.shape)
    ws = L.scratch(lib.gfl_png_workspace_bytes(T, C, W, H), stack.device)
    off = torch.full((T + 1,), -1, dtype=torch.int64, device=stack.device)
    L.check(lib.gfl_png_sizes(L.ptr(stack), T, C, W, H, L.ptr(off), L.ptr(ws), ws.numel(), L.stream()), "sizes")
    off = off.cpu().numpy()
    out = torch.full((int(off[T]) + guard,), 0xA5, dtype=torch.uint8, device=stack.device)
    L.check(lib.gfl_png_emit(L.ptr(stack), T, C, W, H, L.ptr(out), int(off[T]), L.ptr(ws), ws.numel(), L.stream()), "emit")
    return off, out.cpu().numpy()


@pytest.mark.parametrize("C", [1, 3])
def test_stack_offsets_guard_bytes_and_two_calls(C):
    names = ["smooth", "flat", "noise"]
    stack = torch.from_numpy(np.stack([image(n, "strip+", C) for n in names])).cuda()
    off, out = _raw_calls(stack)
    assert off[0] == 0 and (np.diff(off) > 0).all()
    total = int(off[-1])
    assert (out[total:] == 0xA5).all(), "bytes behind `out` were written"
    # the size pass and the emit pass agree: every image's stream ends exactly where the next one starts
    for t, n in enumerate(names):
        stream = out[off[t]:off[t + 1]].tobytes()
        d = zlib.decompressobj()
        assert d.decompress(stream) == R.filtered_bytes(image(n, "strip+", C)) and d.eof and d.unused_data == b""
        assert stream == encoded(n, "strip+", C)[1], "an image of a stack differs from its own encode"
    off2, out2 = _raw_calls(stack)
    assert np.array_equal(off, off2) and np.array_equal(out, out2), "two calls gave different bytes"
    # an `out` that is too short by one byte: the last strip is not written, nothing behind out_bytes is touched
    lib = L.load()
    T, H, W, _ = (int(v) for v in stack.shape)
    ws = L.scratch(lib.gfl_png_workspace_bytes(T, C, W, H), stack.device)
    o = torch.empty(T + 1, dtype=torch.int64, device=stack.device)
    L.check(lib.gfl_png_sizes(L.ptr(stack), T, C, W, H, L.ptr(o), L.ptr(ws), ws.numel(), L.stream()), "sizes")
    short = torch.full((total,), 0xA5, dtype=torch.uint8, device=stack.device)
    L.check(lib.gfl_png_emit(L.ptr(stack), T, C, W, H, L.ptr(short), total - 1, L.ptr(ws), ws.numel(), L.stream()), "emit")
    short = short.cpu().numpy()
    assert short[total - 1] == 0xA5 and np.array_equal(short[:off[2]], out[:off[2]])


def test_encode_png_shapes_and_files(tmp_path):
    rgb = np.stack([image("smooth", "odd", 3), image("checker", "odd", 3)])
    files = P.encode_png(rgb)
    assert len(files) == 2 and files[0] == encoded("smooth", "odd", 3)[0]
    assert P.encode_png(torch.from_numpy(rgb[1].copy()).cuda()) == [files[1]]             # a single (H, W, 3) image
    grey = rgb[..., 0]
    assert P.encode_png(grey) == P.encode_png(grey[..., None])                             # (T, H, W)
    assert P.encode_png(grey[0]) == P.encode_png(grey[:1])                                 # (H, W)
    strided = torch.from_numpy(np.concatenate([rgb, rgb], 2)).cuda()[:, :, :61]            # not contiguous
    assert P.encode_png(strided) == files
    paths = P.write_pngs(rgb, [tmp_path / "a.png", tmp_path / "b.png"])
    assert [np.array_equal(np.asarray(Image.open(p)), x) for p, x in zip(paths, rgb)] == [True, True]
    with pytest.raises(ValueError):
        P.write_pngs(rgb, [tmp_path / "a.png"])
    with pytest.raises(ValueError):
        P.encode_png(np.zeros((1, 2, 11000, 3), np.uint8))                                 # one filtered row does not fit


# device / reference (zlib's optimal codes on the same strips), measured on an MI355X (the bytes are deterministic), and the
# bound: the measured value plus 5 % of slack for a change of the contents
RATIOS = {"smooth": (1.0000, (480, 854, 3)), "flat": (1.0000, (480, 854, 3)), "disc": (0.9974, (480, 854, 1))}


@pytest.mark.parametrize("content", sorted(RATIOS))
def test_size_against_zlibs_optimal_codes(content):
    measured, (H, W, C) = RATIOS[content]
    img = R.content(content, H, W, C)
    data, off = P.encode_streams(torch.from_numpy(img)[None].cuda())
    stream = data.tobytes()
    assert zlib.decompress(stream) == R.filtered_bytes(img)
    ref = R.reference_stream(img)
    ratio = len(stream) / len(ref)
    print(f"png size {content} {H}x{W}x{C}: device {len(stream)} reference {len(ref)} ratio {ratio:.4f}")
    assert ratio <= measured * 1.05
