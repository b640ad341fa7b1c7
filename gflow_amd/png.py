"""PNG files coded on the device (include/gflow_hip.h, "PNG files"; INTEGRATION.md, "PNG files").

The library's two calls give the zlib stream of every image of a stack -- Up filter, runs as distance-1 matches, a dynamic
Huffman code per strip of rows, built on the device --; the host puts the PNG chunks around each stream.  ``encode_png`` is
the whole, ``write_pngs`` writes the files, ``png_chunks`` is the host container alone (no device needed)."""
import struct
import zlib

import numpy as np
import torch

from . import _lib as L

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def strip_rows(C, W):
    """rows of a strip (gfl_png_strip_rows): clamp(32768 // (1 + W C), 1, 64); 0 where one filtered row does not fit"""
    return int(L.load().gfl_png_strip_rows(int(C), int(W)))


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xffffffff)


def _palette_bytes(palette):
    p = np.asarray(palette)
    if p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= 256:
        raise ValueError(f"gflow_amd.png: a palette is (1 .. 256, 3) uint8, got {p.shape} {p.dtype}")
    return p.tobytes()


def png_chunks(stream, W, H, C, palette=None):
    """One PNG file around the zlib stream of an image's filtered rows: signature, IHDR (8 bits; colour type 0 for C = 1,
    2 for C = 3, 3 for C = 1 with a ``palette`` of (K, 3) uint8), PLTE with a palette, one IDAT, IEND."""
    W, H, C = int(W), int(H), int(C)
    if C not in (1, 3) or W < 1 or H < 1:
        raise ValueError(f"gflow_amd.png: an image is W, H >= 1 with 1 or 3 channels, got W={W} H={H} C={C}")
    if palette is not None and C != 1:
        raise ValueError("gflow_amd.png: a palette goes with one channel of indices")
    colour = 2 if C == 3 else (3 if palette is not None else 0)
    out = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, colour, 0, 0, 0))]
    if palette is not None:
        out.append(_chunk(b"PLTE", _palette_bytes(palette)))
    out.append(_chunk(b"IDAT", bytes(stream)))
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)


def _as_images(images):
    """(T, H, W, C) uint8 on a HIP device, C = 1 or 3, from (T, H, W, C), (T, H, W), (H, W, 3) or (H, W); and whether the
    input was a single image"""
    if isinstance(images, np.ndarray) and not images.flags.writeable:
        images = images.copy()                     # (torch refuses to wrap a read-only array quietly)
    t = torch.as_tensor(images)
    if t.dtype != torch.uint8:
        raise ValueError(f"gflow_amd.png: images must be uint8, got {t.dtype}")
    single = False
    if t.dim() == 2:
        t, single = t[None, :, :, None], True
    elif t.dim() == 3 and t.shape[-1] == 3:        # (a (T, H, 3) stack of grey images is not told apart: pass (T, H, 3, 1))
        t, single = t[None], True
    elif t.dim() == 3:
        t = t[..., None]
    if t.dim() != 4 or t.shape[-1] not in (1, 3):
        raise ValueError(f"gflow_amd.png: images must be (T, H, W, C) with C = 1 or 3, (T, H, W), (H, W, 3) or (H, W), got "
                         f"{tuple(torch.as_tensor(images).shape)}")
    if not t.is_cuda and torch.cuda.is_available():
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    L.need_device(t)
    return t.contiguous(), single


def encode_streams(images):
    """The library's two calls on one stack: (the zlib streams of all images as one host uint8 array, the T + 1 offsets).
    ``images``: (T, H, W, C) uint8 on the device.  One read of the offsets between the passes, one copy of the bytes."""
    T, H, W, C = (int(v) for v in images.shape)
    lib = L.load()
    dev = images.device
    need = lib.gfl_png_workspace_bytes(T, C, W, H)
    if need == 0:
        raise ValueError(f"gflow_amd.png: unsupported stack T={T} H={H} W={W} C={C} (at least one image, a filtered row of "
                         "1 + W C <= 32768 bytes)")
    with torch.cuda.device(dev):
        ws = L.scratch(need, dev)
        offsets = torch.empty(T + 1, dtype=torch.int64, device=dev)
        L.check(lib.gfl_png_sizes(L.ptr(images), T, C, W, H, L.ptr(offsets), L.ptr(ws), ws.numel(), L.stream()), "png sizes")
        off = offsets.cpu().numpy()
        out = torch.empty(int(off[T]), dtype=torch.uint8, device=dev)
        L.check(lib.gfl_png_emit(L.ptr(images), T, C, W, H, L.ptr(out), out.numel(), L.ptr(ws), ws.numel(), L.stream()),
                "png emit")
        return out.cpu().numpy(), off


def encode_png(images, palette=None):
    """``images`` -- (T, H, W, C) with C = 1 or 3, (T, H, W), or a single (H, W, 3) / (H, W) image, uint8; a device tensor, a
    host tensor or an array (host input is moved to the current HIP device; without one this raises: there is no CPU path) --
    as T complete PNG files: a list of bytes.  ``palette``: (K, 3) uint8, the colours of a one-channel stack's indices."""
    if palette is not None:
        _palette_bytes(palette)
    images, _ = _as_images(images)
    T, H, W, C = (int(v) for v in images.shape)
    if palette is not None and C != 1:
        raise ValueError("gflow_amd.png: a palette goes with one channel of indices")
    if T == 0:
        return []
    data, off = encode_streams(images)
    return [png_chunks(data[off[t]:off[t + 1]].tobytes(), W, H, C, palette) for t in range(T)]


def write_pngs(images, paths, palette=None):
    """encode_png, one file per image: ``paths`` has one entry per image"""
    files = encode_png(images, palette)
    paths = list(paths)
    if len(paths) != len(files):
        raise ValueError(f"gflow_amd.png: {len(files)} images and {len(paths)} paths")
    for path, data in zip(paths, files):
        with open(path, "wb") as f:
            f.write(data)
    return paths
