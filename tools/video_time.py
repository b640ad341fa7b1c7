"""What coding a stack of frames as JPEG costs ("Video files"): T = 60 frames of 480 x 854 x 3, a smooth
moving pattern with 2 % noise over it (a render, not a test chart), quality 90, on the device and with PIL on the same machine.

    python tools/video_time.py device     # HIP events around the two library calls and around encode_jpeg (needs the GPU)
    python tools/video_time.py pil        # PIL's host encode of the same frames (quality 90, 4:4:4, standard tables)
    python tools/video_time.py both

Each prints one JSON line.  Nothing in the test suite gates on these numbers."""
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, W, T, Q = 480, 854, 60, 90


def frames():
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        for c in range(3):
            a = 127.5 + 100.0 * np.sin(0.02 * (c + 1) * x + 0.3 * t) * np.cos(0.015 * y - 0.1 * c * t)
            out[t, ..., c] = np.clip(a + rng.normal(0.0, 5.0, (H, W)), 0, 255).astype(np.uint8)
    return out


def device():
    import torch
    from gflow_amd import _lib as L
    from gflow_amd import video
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    imgs = torch.from_numpy(frames()).to(dev)
    lib = L.load()
    qt = torch.from_numpy(video.quant_tables(Q).astype(np.int16)).to(dev)
    ws = L.scratch(lib.gfl_jpeg_workspace_bytes(T, 3, W, H), dev)
    off = torch.empty(T + 1, dtype=torch.int64, device=dev)
    args = (L.ptr(imgs), T, 3, W, H, L.ptr(qt))
    L.check(lib.gfl_jpeg_sizes(*args, L.ptr(off), L.ptr(ws), ws.numel(), L.stream()), "sizes")
    total = int(off[T].item())
    out = torch.empty(total, dtype=torch.uint8, device=dev)

    def sizes():
        L.check(lib.gfl_jpeg_sizes(*args, L.ptr(off), L.ptr(ws), ws.numel(), L.stream()), "sizes")

    def emit():
        L.check(lib.gfl_jpeg_emit(*args, L.ptr(out), total, L.ptr(ws), ws.numel(), L.stream()), "emit")

    def timed(fn, n):
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return sorted(ms)

    for _ in range(3):
        sizes()
        emit()
        video.encode_jpeg(imgs, Q)
    torch.cuda.synchronize()
    res = dict(H=H, W=W, T=T, quality=Q, bytes=total, sizes_ms=timed(sizes, 10), emit_ms=timed(emit, 10),
               encode_jpeg_ms=timed(lambda: video.encode_jpeg(imgs, Q), 10))
    both = res["sizes_ms"][5] + res["emit_ms"][5]
    res["frames_per_s_two_passes"] = T / (both * 1e-3)
    res["frames_per_s_encode_jpeg"] = T / (res["encode_jpeg_ms"][5] * 1e-3)
    print(json.dumps(res))


def pil():
    from PIL import Image
    imgs = frames()
    best, size = None, 0
    for _ in range(3):
        t0 = time.perf_counter()
        size = 0
        for f in imgs:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, format="JPEG", quality=Q, subsampling=0, optimize=False)
            size += buf.tell()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    print(json.dumps(dict(H=H, W=W, T=T, quality=Q, bytes=size, pil_encode_s=best, frames_per_s=T / best)))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "both"
    if mode in ("device", "both"):
        device()
    if mode in ("pil", "both"):
        pil()
