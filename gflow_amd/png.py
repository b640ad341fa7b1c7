"""PNG files coded on the device (include/gflow_hip.h, "PNG files"; INTEGRATION.md, "PNG files").

The library's two calls give the zlib stream of every image of a stack -- Up filter, runs as distance-1 matches, a dynamic
Huffman code per strip of rows, built on the device --; the host puts the PNG chunks around each stream.  ``encode_png`` is
the whole, ``write_pngs`` writes the files, ``png_chunks`` is the host container alone (no device needed).

Decoding ("Decoding PNG files") is the other direction: ``parse_png`` takes the container apart on the host,
``decode_png`` inflates and unfilters a stack of one shape on the device with the bits of ``np.asarray(PIL.Image.open(f))``,
``python -m gflow_amd.png --check DIR`` holds a folder of files against PIL."""
import struct
import sys
import time
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


# ------------------------------------------------------------------------------------------------------------ decoding
BYTES_PER_PIXEL = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}          # colour type -> bytes per pixel at 8 bits
# status of an image (include/gflow_hip.h, GFL_PNG_*)
STATUS = {1: "the input ends early", 2: "bad zlib header", 3: "reserved block type", 4: "a stored block's LEN / NLEN disagree",
          5: "HLIT > 286 or HDIST > 30", 6: "a repeat code with nothing to repeat or past the end",
          7: "an over-subscribed or incomplete code", 8: "no end-of-block code", 9: "an undefined or out-of-range symbol",
          10: "a distance reaching before the start of the output", 11: "more or fewer bytes than the image holds",
          12: "Adler-32 mismatch", 13: "a filter type above 4"}


def parse_png(data, name="PNG data"):
    """The container of one PNG file, on the host; nothing is decoded.  dict(width, height, bpp -- bytes per pixel --,
    colour_type, palette -- (K, 3) uint8 or None --, stream -- all IDAT payloads put together: ONE zlib stream, cut into
    chunks at any byte --, idat_chunks -- how many there were).  ValueError naming ``name`` for everything ``decode_png`` does
    not take: no PNG signature, a cut chunk, a critical chunk with a wrong CRC, a bit depth other than 8, an interlaced file,
    a colour type other than 0, 2, 3, 4 or 6, no IHDR, IDAT or IEND, an unknown critical chunk.  Ancillary chunks (tRNS, gAMA,
    pHYs, text ...) are skipped: PIL leaves the pixel array alone for them."""
    data = bytes(data)

    def refuse(why):
        return ValueError(f"gflow_amd.png: {name}: {why}")

    if data[:8] != SIGNATURE:
        raise refuse("no PNG signature")
    pos, head, palette, idat, ended = 8, None, None, [], False
    while not ended and pos < len(data):
        if pos + 12 > len(data):
            raise refuse(f"a chunk header cut short at byte {pos}")
        n, kind = struct.unpack_from(">I4s", data, pos)
        if pos + 12 + n > len(data):
            raise refuse(f"chunk {kind!r} at byte {pos} cut short")
        body = data[pos + 8:pos + 8 + n]
        critical = not kind[0] & 0x20
        if critical and struct.unpack_from(">I", data, pos + 8 + n)[0] != zlib.crc32(kind + body) & 0xffffffff:
            raise refuse(f"chunk {kind!r} at byte {pos} has a wrong CRC")
        pos += 12 + n
        if kind == b"IHDR":
            if n != 13:
                raise refuse("an IHDR chunk of the wrong size")
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            if n == 0 or n % 3 or n > 768:
                raise refuse("a PLTE chunk of the wrong size")
            palette = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3).copy()
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        elif critical:
            raise refuse(f"unknown critical chunk {kind!r}")
    if head is None:
        raise refuse("no IHDR chunk")
    if not idat:
        raise refuse("no IDAT chunk")
    if not ended:
        raise refuse("no IEND chunk")
    W, H, depth, colour, compression, filtering, interlace = head
    if colour not in BYTES_PER_PIXEL:
        raise refuse(f"colour type {colour} (0, 2, 3, 4 and 6 are decoded)")
    if depth != 8:
        raise refuse(f"bit depth {depth} (8 bits are decoded)")
    if interlace:
        raise refuse("an interlaced (Adam7) file")
    if compression or filtering or W < 1 or H < 1:
        raise refuse(f"an IHDR of compression {compression}, filter method {filtering}, {W} x {H}")
    return dict(width=W, height=H, bpp=BYTES_PER_PIXEL[colour], colour_type=colour, palette=palette, stream=b"".join(idat),
                idat_chunks=len(idat))


def _decode_device(device, what):
    if device is None and torch.cuda.is_available():
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device("cpu" if device is None else device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"gflow_amd.png: {what} needs a HIP (cuda) device; there is no CPU fallback")
    return device


def decode_streams(streams, W, H, bpp, device):
    """gfl_png_decode on the zlib streams of T images of one shape: ((T, H, W, bpp) uint8 on ``device``, the images' status as
    a host int32 array).  One upload, one call, one read-back; nothing is raised for an image that went wrong (it is zero)."""
    device = _decode_device(device, "decode_streams")
    T, W, H, bpp = len(streams), int(W), int(H), int(bpp)
    lib = L.load()
    need = lib.gfl_png_decode_workspace_bytes(T, bpp, W, H)
    if need == 0:
        raise ValueError(f"gflow_amd.png: unsupported stack T={T} H={H} W={W} bytes per pixel {bpp}")
    # ONE upload: the T + 1 offsets, then the streams behind each other from a 16-byte boundary
    first = ((T + 1) * 8 + 15) // 16 * 16
    off = first + np.cumsum([0] + [len(s) for s in streams], dtype=np.int64)
    host = np.zeros(int(off[-1]) + 16, dtype=np.uint8)
    host[:(T + 1) * 8] = off.view(np.uint8)
    host[first:int(off[-1])] = np.frombuffer(b"".join(streams), dtype=np.uint8)
    with torch.cuda.device(device):
        blob = torch.from_numpy(host).to(device)
        images = torch.empty((T, H, W, bpp), dtype=torch.uint8, device=device)
        status = torch.empty(T, dtype=torch.int32, device=device)
        ws = L.scratch(need, device)
        L.check(lib.gfl_png_decode(L.ptr(blob), blob.numel(), L.ptr(blob), T, bpp, W, H, L.ptr(images), L.ptr(status), L.ptr(ws),
                                   ws.numel(), L.stream()), "png decode")
        return images, status.cpu().numpy()


def decode_png(files, device=None, names=None):
    """``files`` -- a list of complete PNG files as bytes, all of one width, height and bytes per pixel (8 bits, not
    interlaced; their compression, filters and chunking may differ) -- as a (T, H, W, C) uint8 stack on ``device`` (default:
    the current HIP device; without one this raises: there is no CPU path).  C = the file's bytes per pixel: 1 grey or the
    INDICES of a palette file (the palette is not applied, nor is tRNS), 2 grey + alpha, 3 RGB, 4 RGBA -- the bits of
    ``np.asarray(PIL.Image.open(file))``.  One upload, one library call, one read-back of the status: an image that went
    wrong raises ValueError naming its file (``names[t]`` if given) and the code.  Raises ValueError too for a file
    ``parse_png`` refuses.  An entry of ``files`` may also be the dict ``parse_png`` gave for a file: it is not parsed again."""
    device = _decode_device(device, "decode_png")
    if not files:
        return torch.empty((0, 0, 0, 1), dtype=torch.uint8, device=device)
    label = lambda t: f"image {t}" + (f" ({names[t]})" if names is not None else "")
    parsed = [f if isinstance(f, dict) else parse_png(f, label(t)) for t, f in enumerate(files)]
    key = lambda p: (p["width"], p["height"], p["bpp"])
    for t, p in enumerate(parsed):
        if key(p) != key(parsed[0]):
            raise ValueError(f"gflow_amd.png: {label(t)} is {key(p)} (width, height, bytes per pixel), {label(0)} is "
                             f"{key(parsed[0])}: one call decodes one shape")
    W, H, bpp = key(parsed[0])
    images, st = decode_streams([p["stream"] for p in parsed], W, H, bpp, device)
    bad = np.flatnonzero(st)
    if bad.size:
        t = int(bad[0])
        raise ValueError(f"gflow_amd.png: {label(t)}: {STATUS.get(int(st[t]), 'unknown')} (status {int(st[t])}; {bad.size} of "
                         f"{len(parsed)} images of the call went wrong)")
    return images


def check_folder(folder, device=None, out=sys.stdout):
    """Every .png of ``folder`` decoded on the device, in stacks by shape, and compared with PIL: (matched, differing,
    refused)."""
    import os
    from PIL import Image
    device = _decode_device(device, "--check")
    paths = sorted(os.path.join(folder, f) for f in os.listdir(folder) if f.lower().endswith(".png"))
    stacks, refused = {}, []
    for path in paths:
        with open(path, "rb") as f:
            data = f.read()
        try:
            p = parse_png(data, os.path.basename(path))
            stacks.setdefault((p["height"], p["width"], p["bpp"]), []).append((path, data))
        except ValueError as e:
            refused.append(str(e))
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    decoded = {}
    for key, members in stacks.items():
        stack = decode_png([d for _, d in members], device, names=[os.path.basename(q) for q, _ in members])
        decoded[key] = stack.cpu().numpy()
    t_device = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = {key: [np.asarray(Image.open(q)) for q, _ in members] for key, members in stacks.items()}
    t_host = time.perf_counter() - t0
    matched, differing = 0, []
    for key, members in stacks.items():
        for t, (path, _) in enumerate(members):
            w = want[key][t]
            if np.array_equal(decoded[key][t], w[..., None] if w.ndim == 2 else w):
                matched += 1
            else:
                differing.append(path)
    print(f"{len(paths)} PNG files in {len(stacks)} stacks: {matched} match PIL bit for bit, {len(differing)} differ, "
          f"{len(refused)} refused by parse_png", file=out)
    for why in refused:
        print("  refused:", why, file=out)
    for path in differing:
        print("  DIFFERS:", path, file=out)
    print(f"device {t_device * 1e3:.1f} ms (decode and read-back), PIL {t_host * 1e3:.1f} ms", file=out)
    return matched, differing, refused


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gflow_amd.png", description="hold a folder of PNG files against PIL")
    ap.add_argument("--check", metavar="DIR", required=True, help="decode every .png of DIR on the device and compare with PIL")
    ap.add_argument("--gpu", type=int, default=0)
    args = ap.parse_args(argv)
    _, differing, _ = check_folder(args.check, torch.device("cuda", args.gpu))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
