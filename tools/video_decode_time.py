"""What decoding a stack of JPEG frames costs ("Decoding video files"): tools/video_time.py's T = 60 frames of
480 x 854 x 3, written by PIL at quality 90, 4:2:0, once with the encoder's restart interval (many units per frame) and once
without DRI (one unit, so one lane, per frame: what a DAVIS file is) -- on the device, and with PIL on the same machine.

    python tools/video_decode_time.py     # needs the GPU; prints one JSON line per case

Per case: ``parse_ms`` (the host's parse_jpeg of the 60 files), ``library_ms`` (HIP events around gfl_jpeg_decode alone, sorted,
10 calls after 3 warm-ups), ``decode_jpeg_ms`` (wall clock of the whole call: parse, one upload, the library call, the
read-back of the status), ``pil_ms`` (np.asarray(Image.open(...)) of the same files, best of 3).  Nothing in the test suite
gates on these numbers."""
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.video_time import H, Q, T, W, frames  # noqa: E402


def main():
    import torch
    from PIL import Image
    from gflow_amd import _lib as L
    from gflow_amd import video
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    imgs = frames()
    lib = L.load()
    for name, rmb in (("restart interval %d" % video.restart_interval(), video.restart_interval()), ("no DRI", 0)):
        files = []
        for f in imgs:
            buf = io.BytesIO()
            Image.fromarray(f).save(buf, format="JPEG", quality=Q, subsampling=2, **({"restart_marker_blocks": rmb} if rmb else {}))
            files.append(buf.getvalue())
        t0 = time.perf_counter()
        parsed = [video.parse_jpeg(f) for f in files]
        parse_ms = 1e3 * (time.perf_counter() - t0)
        units, tables, data = video.decode_arrays(files, parsed)
        p = parsed[0]
        shape = (T, 3, W, H, p["hs"], p["vs"])
        u, tb, d = (torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev) for a in (units, tables, data))
        out = torch.empty((T, H, W, 3), dtype=torch.uint8, device=dev)
        status = torch.empty(len(units), dtype=torch.int32, device=dev)
        ws = L.scratch(lib.gfl_jpeg_decode_workspace_bytes(*shape, len(units)), dev)

        def call():
            L.check(lib.gfl_jpeg_decode(L.ptr(d), len(data), L.ptr(u), len(units), L.ptr(tb), *shape, L.ptr(out), L.ptr(status),
                                        L.ptr(ws), ws.numel(), L.stream()), "decode")

        for _ in range(3):
            call()
        torch.cuda.synchronize()
        library_ms = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            library_ms.append(a.elapsed_time(b))
        assert not status.any().item()
        whole = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = video.decode_jpeg(files, dev)
            torch.cuda.synchronize()
            whole.append(1e3 * (time.perf_counter() - t0))
        pil = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = [np.asarray(Image.open(io.BytesIO(f))) for f in files]
            pil.append(1e3 * (time.perf_counter() - t0))
        assert np.array_equal(got.cpu().numpy(), np.stack(want)) and torch.equal(got, out)
        print(json.dumps(dict(case=name, H=H, W=W, T=T, quality=Q, sampling="4:2:0", bytes=int(len(data)), units=int(len(units)),
                              parse_ms=parse_ms, library_ms=sorted(library_ms), decode_jpeg_ms=sorted(whole), pil_ms=min(pil))),
              flush=True)


if __name__ == "__main__":
    main()
