"""What saving a clip fit costs ("Saving a fit" and "PNG files"):
   python tools/png_time.py [FRAMES [REPEATS]]
Two measurements, host clocks around work that ends in a device synchronise, each after one warm-up:
   1. encode_png of a (FRAMES, 480, 854, 3) stack of renders of the bench scene (default 60 frames; the viewer's images of a
      synthetic log folder, every frame from a camera a little further along) against PIL saving the same images on this host
      at its default level and at compress_level=1; the files' sizes.
   2. a FRAMES-frame clip fit (BASELINE.json configs[2]: 60 000 splats, 500 / 300 / 150 iterations, 480 x 854) without
      ``save``, with ``save`` (a temporary folder), and what the same files cost through PIL: the seven images per frame of the
      saved folder written again with Image.save.  Frames per second of each; then the saving fit once more by parts: its
      frame loop, and inside result() the hull masks, the checkpoints, the PNG files and the AVI files.
One JSON line at the end."""
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import png as P  # noqa: E402
from gflow_amd import render as R  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402
from gflow_amd.fit_video import fit_clip, upload_clip  # noqa: E402

dev = torch.device("cuda", 0)
H, W, N = 480, 854, 60000


def renders(T):
    """(T, H, W, 3) uint8 on the device: the bench scene from T cameras"""
    frame = S.make_frame(H, W, seed=0)
    raw = S.init_splats(frame, N, seed=0, grown=True)
    act = [raw["xyz"], raw["scale"].abs(), torch.nn.functional.normalize(raw["rotate"]), torch.sigmoid(10 * raw["opacity"]),
           torch.sigmoid(raw["rgb"])]
    act = [a.detach().float().to(dev) for a in act]
    out = []
    with torch.no_grad():
        for t in range(T):
            extr = raw["extr"].float().clone()
            extr[0, 3] += 0.002 * t
            img = R.render_multiple([*act, raw["intr"].float().to(dev), extr.to(dev), 0.0, W, H], ["rgb"])["rgb"]
            out.append(R.render2img_device(img))
    return torch.stack(out).contiguous()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def pil_save(images, **kw):
    n = 0
    for im in images:
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, format="PNG", **kw)
        n += buf.tell()
    return n


def time_encode(T, repeats):
    stack = renders(T)
    host = stack.cpu().numpy()
    P.encode_png(stack[:2])                                           # warm-up: code objects, the allocator
    ours = [clock(lambda: P.encode_png(stack)) for _ in range(repeats)]
    files = ours[0][1]
    assert all(np.array_equal(np.asarray(Image.open(io.BytesIO(f))), im) for f, im in zip(files[:3], host[:3]))
    pil6 = [clock(lambda: pil_save(host)) for _ in range(max(1, repeats // 2))]
    pil1 = [clock(lambda: pil_save(host, compress_level=1)) for _ in range(max(1, repeats // 2))]
    return dict(frames=T, device_s=min(t for t, _ in ours), device_bytes=sum(len(f) for f in files),
                pil_default_s=min(t for t, _ in pil6), pil_default_bytes=pil6[0][1],
                pil_level1_s=min(t for t, _ in pil1), pil_level1_bytes=pil1[0][1])


def time_fit(T):
    from gflow_amd import log_folder as LF
    from gflow_amd.clip_fit import ClipFit
    from gflow_amd.trainer import run_to_end
    clip = upload_clip(S.make_clip(T, H, W, seed=0, device=dev), dev)
    warm = dict(iterations_first=20, iterations_after=10, iterations_camera=5)
    fit_clip(clip[:2], dev, warm, seed=0)
    plain_s, plain = clock(lambda: fit_clip(clip, dev, None, seed=0))
    with tempfile.TemporaryDirectory() as folder:
        fit_clip(clip[:2], dev, warm, seed=0, save=os.path.join(folder, "warm"))
        saved_s, saved = clock(lambda: fit_clip(clip, dev, None, seed=0, save=os.path.join(folder, "clip")))
        # once more, by parts: the frame loop with the recorder, then the writers one by one
        spent = {}

        def timed(name, fn):
            def run(*a, **kw):
                t, out = clock(lambda: fn(*a, **kw))
                spent[name] = spent.get(name, 0.0) + t
                return out
            return run
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            cf = ClipFit(clip, dev, None, seed=0, save=os.path.join(folder, "parts"))
            loop_s, _ = clock(lambda: run_to_end(cf.steps()))
            rec = cf.tr.seg_recorder
            rec.masks = timed("hull_masks", rec.masks)
            keep = (LF.torch.save, LF.PN.write_pngs, LF.VD.write_avi)
            LF.torch.save, LF.PN.write_pngs, LF.VD.write_avi = (timed("checkpoints", keep[0]), timed("png_files", keep[1]),
                                                                 timed("avi_files", keep[2]))
            try:
                result_s, _ = clock(cf.result)
            finally:
                LF.torch.save, LF.PN.write_pngs, LF.VD.write_avi = keep
        images = [np.asarray(Image.open(os.path.join(folder, "clip", "images", f)))
                  for f in sorted(os.listdir(os.path.join(folder, "clip", "images")))]
        size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(folder, "clip")) for f in fs)
    t0 = time.perf_counter()
    pil_save(images)
    pil_s = time.perf_counter() - t0
    return dict(frames=T, plain_s=plain_s, plain_frames_per_s=T / plain_s, saved_s=saved_s, saved_frames_per_s=T / saved_s,
                pil_same_images_s=pil_s, plain_plus_pil_frames_per_s=T / (plain_s + pil_s), folder_bytes=size,
                rasterisations=(plain["rasterisations"], saved["rasterisations"]),
                by_parts=dict(frame_loop_s=loop_s, result_s=result_s, **{k + "_s": v for k, v in spent.items()}))


def main(T=60, repeats=3):
    out = dict(encode=time_encode(T, repeats), fit=time_fit(T))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main(*(int(v) for v in sys.argv[1:3]))
