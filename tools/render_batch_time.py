"""What an inference image costs, batched and one at a time (the row of rb_blend_kernel):
   python tools/render_batch_time.py [J ...]
on the bench scene (480 x 854, 60 000 grown splats of synthetic.init_splats, seed 0), J = 1, 8, 60 cameras stepping sideways:
   (a) render_jobs(sets, cameras, uint8=True): gfl_render_batch, the bytes written by the blend;
   (b) the same images as a loop of render() under torch.no_grad() followed by render2img_device;
   and, beside (a), render_views(gaussians, cameras, uint8=True): the same library call without render_jobs' concatenation of
   J copies of the rows ("views").
Device events around ``calls`` repetitions back to back on an idle stream, per image; median [min, max] of ``groups`` such
windows after ``warm`` warm-up windows, (a) and (b) alternating.  Also the host time to ENQUEUE one repetition (a host clock
around the calls, no synchronise inside).  The images of (a) and (b) are compared once per J."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import render as R  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402

dev = torch.device("cuda", 0)
H, W, N = 480, 854, 60000
NAMES = ("xyz", "scale", "rotate", "opacity", "rgb")


def scene():
    frame = S.make_frame(H, W, seed=0)
    raw = S.init_splats(frame, N, seed=0, grown=True)
    gs = dict(xyz=raw["xyz"], scale=raw["scale"].abs(), rotate=torch.nn.functional.normalize(raw["rotate"]),
              opacity=torch.sigmoid(10 * raw["opacity"]), rgb=torch.sigmoid(raw["rgb"]))
    return {k: v.float().to(dev) for k, v in gs.items()}, raw["intr"].float().to(dev), raw["extr"].float().to(dev)


def measure(J, gs, intr, extr, groups=9, warm=2):
    cams = []
    for j in range(J):
        e = extr.clone()
        e[0, 3] += 0.002 * j                     # a stereo-like sweep: every image is a different one
        cams.append(dict(intr=intr, extr=e, W=W, H=H))
    stacked = dict(intr=intr, extr=torch.stack([c["extr"] for c in cams]), W=W, H=H)
    sets = [gs] * J
    calls = max(1, 40 // J)

    def batched():
        return R.render_jobs(sets, stacked, bg=1.0, uint8=True)["img"]

    def looped():
        with torch.no_grad():
            return torch.stack([R.render2img_device(R.render(gs, c, 1.0)["rgb"]) for c in cams])

    def views():
        return R.render_views(gs, stacked, bg=1.0, uint8=True)["img"]

    a, b = batched(), looped()
    torch.cuda.synchronize()
    differ = float((a != b).float().mean())
    assert torch.equal(views(), a)
    res = {"batched": ([], []), "views": ([], []), "looped": ([], [])}
    for g in range(warm + groups):
        for name, fn in (("batched", batched), ("views", views), ("looped", looped)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            host = time.perf_counter() - t0
            torch.cuda.synchronize()
            if g >= warm:
                res[name][0].append(e0.elapsed_time(e1) / (calls * J) * 1e3)
                res[name][1].append(host / (calls * J) * 1e6)
    R.check_overflow()
    out = {}
    for name, (d, h) in res.items():
        d, h = np.array(d), np.array(h)
        out[name] = float(np.median(d))
        print(f"J = {J:3d}  {name:8s} {np.median(d):8.1f} us per image on the device [{d.min():.1f}, {d.max():.1f}], "
              f"{np.median(h):7.1f} us per image to enqueue [{h.min():.1f}, {h.max():.1f}]  ({calls} repetitions x {groups} windows)")
    print(f"J = {J:3d}  looped / batched = {out['looped'] / out['batched']:.2f}; bytes that differ between the two: {differ:.2e}")


if __name__ == "__main__":
    gs, intr, extr = scene()
    for J in ([int(v) for v in sys.argv[1:]] or [1, 8, 60]):
        measure(J, gs, intr, extr)
