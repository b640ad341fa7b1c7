"""What loading a prepared sequence costs on the host and on the device (INTEGRATION.md "Frame preparation"):
   python tools/load_time.py [--frames 8] [--height 1080] [--width 1920] [--resize 480] [--blur] [--repeats 3] [--dir DIR]
writes a synthetic clip of that size with io.write_sequence into a temporary folder (or into DIR, where a clip that is already
there is used as it is), then times, median of ``repeats`` runs
after one warm-up each:
   decode_s        every file of the clip decoded to a raw array (PIL, np.load, .flo), nothing else: common to both paths
   host_load_s     io.load_sequence(...)              -> host_prep_s   = host_load_s - decode_s
   host_upload_s   fit_video.upload_clip of those frames (what the host path still owes before a fit)
   device_load_s   io.load_sequence(..., device=...)  -> device_prep_s = device_load_s - decode_s (stacking, one upload per
                   kind, the library calls, the read-back of occ_count; synchronised)
   device_kernels_s  the gfl_prep_frames calls of that load alone, on stacks that are already resident (HIP events)
and prints one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import io as gio  # noqa: E402
from gflow_amd import prep as P  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402
from gflow_amd.fit_video import upload_clip  # noqa: E402


def median_time(fn, repeats, sync=False):
    times = []
    for r in range(repeats + 1):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        if r:
            times.append(time.perf_counter() - t0)
        del out
    return float(np.median(times))


def decode(sp):
    """every array the loaders decode, and nothing else"""
    p = gio.sequence_paths(sp)
    n = len(p["img"])
    return dict(image=[gio._decode_image(f)[0] for f in p["img"]],
                depth=[np.asarray(np.load(f), dtype=np.float32)[..., None] for f in p["depth"][:n]],
                flow=[gio._read_flo(f) for f in p["flow"][:n]],
                move=[gio._decode_mask(f) for f in p["move"][:n]],
                occ=[gio._decode_image(f)[0] for f in p["occ"][:n - 1]])


def kernels_time(raw, resize, blur, dev, repeats):
    """the library calls of one device load on resident stacks: HIP events around them"""
    stacks = {k: torch.from_numpy(np.stack(v)).to(dev) for k, v in raw.items() if v}
    calls = [("image", dict(div=255.0, blur=blur)), ("depth", {}), ("flow", dict(blur=blur)), ("move", dict(as_mask=True)),
             ("occ", dict(div=255.0, blur=blur))]
    times = []
    for r in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for k, kw in calls:
            if k in stacks:
                P.prep_frames(stacks[k], resize, **kw)
        b.record()
        torch.cuda.synchronize()
        if r:
            times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description="load time of a synthetic sequence: host path against device path")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--resize", type=int, default=480)
    ap.add_argument("--blur", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dir", default=None, help="keep the clip in DIR/seq and reuse the one that is there")
    ap.add_argument("--host-only", action="store_true", help="no device: the decode and the host path alone")
    args = ap.parse_args(argv)
    dev = None if args.host_only else torch.device("cuda", 0)
    with tempfile.TemporaryDirectory() as tmp:
        sp = os.path.join(args.dir or tmp, "seq")
        if not os.path.isdir(sp):
            # (the reference's file lists drop the last image: one frame more is written than is loaded)
            gio.write_sequence(S.make_clip(args.frames + 1, args.height, args.width, seed=0), sp)
        kw = dict(resize=args.resize, blur=args.blur)
        out = dict(frames=args.frames, height=args.height, width=args.width, resize=args.resize, blur=args.blur,
                   torch_threads=torch.get_num_threads())
        out["decode_s"] = median_time(lambda: decode(sp), args.repeats)
        out["host_load_s"] = median_time(lambda: gio.load_sequence(sp, **kw), args.repeats)
        out["host_prep_s"] = out["host_load_s"] - out["decode_s"]
        if dev is not None:
            host = gio.load_sequence(sp, **kw)
            out["host_upload_s"] = median_time(lambda: upload_clip(host, dev), args.repeats, sync=True)
            out["device_load_s"] = median_time(lambda: gio.load_sequence(sp, device=dev, **kw), args.repeats, sync=True)
            out["device_prep_s"] = out["device_load_s"] - out["decode_s"]
            out["device_kernels_s"] = kernels_time(decode(sp), args.resize, args.blur, dev, args.repeats)
            frames = gio.load_sequence(sp, device=dev, **kw)
            out["loaded"] = [len(frames)] + list(frames[0]["image"].shape)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
