"""Time gflow_amd.png.decode_png against a PIL loop over the same files ("Decoding PNG files"): 60 frames of
480 x 854 RGB as PIL writes them by default and as gflow_amd.png.encode_png writes them, 60 one-channel masks, one image.
Every case is warmed up, timed RUNS times between device synchronisations, and held to PIL bit for bit; the median and the
range are printed, one JSON line per case.  Needs a HIP device.

    python tools/png_dec_time.py [--frames 60] [--runs 7] [--only NAME]     (kernel times: run it under a kernel trace)"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import png  # noqa: E402

H, W = 480, 854


def frames(n, seed=0):
    """(n, H, W, 3) uint8: a smooth scene that drifts, with sensor noise of +-3 -- what a camera frame costs a PNG coder"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W, 3), np.uint8)
    for t in range(n):
        a = np.stack([127.5 + 90.0 * np.sin(0.013 * (c + 1) * (x + 3 * t) + 0.009 * y + c) * np.cos(0.007 * y - 0.004 * c * x)
                      for c in range(3)], axis=-1)
        edges = 40.0 * (((x + 2 * t) // 61 + y // 47) % 2)[..., None]
        out[t] = np.clip(np.rint(a + edges + rng.integers(-3, 4, size=a.shape)), 0, 255).astype(np.uint8)
    return out


def masks(n):
    """(n, H, W) uint8, 0 / 255: blobs that move, as a move mask's"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    return np.stack([(((x - 300 - 4 * t) ** 2 / 9e3 + (y - 240) ** 2 / 4e3 < 1) | ((x - 600 + 2 * t) ** 2 + (y - 120) ** 2 < 2500))
                     .astype(np.uint8) * 255 for t in range(n)])


def pil_files(stack):
    out = []
    for a in stack:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="PNG")
        out.append(buf.getvalue())
    return out


def timed(fn, runs):
    fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ts)), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rgb, msk = frames(args.frames), masks(args.frames)
    cases = {"rgb, PIL default": pil_files(rgb), "rgb, encode_png": png.encode_png(rgb), "masks, PIL default": pil_files(msk),
             "one rgb image, PIL default": pil_files(rgb[:1])}
    for name, files in cases.items():
        if args.only and args.only != name:
            continue
        want = np.stack([np.asarray(Image.open(io.BytesIO(f))) for f in files])
        got = png.decode_png(files, dev).cpu().numpy()
        assert np.array_equal(got.reshape(want.shape), want), name
        device = timed(lambda: png.decode_png(files, dev), args.runs)
        host = timed(lambda: [np.asarray(Image.open(io.BytesIO(f))) for f in files], args.runs)
        up = timed(lambda: torch.from_numpy(want).to(dev), args.runs)
        print(json.dumps(dict(case=name, images=len(files), file_bytes=sum(len(f) for f in files), decode_png=device, pil_loop=host,
                              upload_of_pil_arrays=up)), flush=True)


if __name__ == "__main__":
    main()
