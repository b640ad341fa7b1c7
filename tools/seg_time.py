"""What moving-region segmentation costs:
   python tools/seg_time.py kernel            gfl_seg_score at T = 60, 480x854, radius 8: HIP events around 20 replays
   python tools/seg_time.py fit [runs] [T]    a T-frame 480p clip fit without / with segment=True, alternating in one
                                              process (medians), the end-of-clip hull pass on its own, and the J, F, J&F
                                              the fit reaches on its synthetic disc"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import fit_video as FV  # noqa: E402
from gflow_amd import _lib as L  # noqa: E402
from gflow_amd import segmentation as SG  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402

dev = torch.device("cuda", 0)


def kernel(T=60, H=480, W=854, radius=8, reps=20):
    # a disc that moves, against the same disc a few pixels off, 1 % of the pixels flipped: boundaries of a real mask pair
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    t = torch.arange(T, device=dev).view(T, 1, 1)
    disc = lambda dx: ((xx - (200 + 6 * t + dx)) ** 2 + (yy - 240) ** 2 <= 110 ** 2)
    noise = lambda: torch.rand(T, H, W, device=dev, generator=g) < 0.01
    pred = ((disc(0) ^ noise()).to(torch.uint8) * 255).contiguous()
    gt = (disc(5) ^ noise()).to(torch.uint8).contiguous()
    counts = torch.empty(T, 6, dtype=torch.int32, device=dev)
    lib = L.load()
    run = lambda: L.check(lib.gfl_seg_score(L.ptr(pred), L.ptr(gt), None, T, H, W, radius, L.ptr(counts), L.stream()), "seg")
    for _ in range(5):
        run()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / reps
    print(f"gfl_seg_score T={T} {H}x{W} radius {radius}: {ms * 1e3:.1f} us per call ({2 * T * H * W / ms / 1e6:.1f} GB/s of mask "
          f"bytes), boundary pixels per frame {counts[:, 2].float().mean().item():.0f} / {counts[:, 3].float().mean().item():.0f}")


def fit(runs=3, T=60):
    frames = FV.upload_clip(S.make_clip(T, 480, 854, seed=0), dev)
    cfg = dict(num_points=60000, traj_num=100, traj_offset=2)
    FV.fit_clip(frames[:2], dev, cfg, seed=0, snapshot_interval=10, segment=True)
    walls = {False: [], True: []}
    for r in range(runs):
        for seg in (False, True):
            keep = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = FV.fit_clip(frames, dev, cfg, seed=0, snapshot_interval=10, segment=seg, keep=keep)
            torch.cuda.synchronize()
            walls[seg].append(time.perf_counter() - t0)
    for seg, w in walls.items():
        w = np.array(w)
        print(f"segment={seg}: median {np.median(w):.4f} s ({T / np.median(w):.2f} frames/s)  min {w.min():.4f} s  all {np.round(w, 4)}")
    rec = keep["trainer"].seg_recorder
    t0 = time.perf_counter()
    host = rec.fetch()
    t1 = time.perf_counter()
    masks, valid = rec.masks(host)
    t2 = time.perf_counter()
    counts = rec.score(masks, valid, [fr["move_mask"] for fr in frames])
    t3 = time.perf_counter()
    print(f"end of clip: copy {1e3 * (t1 - t0):.1f} ms, hull masks {1e3 * (t2 - t1):.1f} ms ({1e3 * (t2 - t1) / T:.2f} per frame, "
          f"{int(np.mean([x[1].sum() for x in host if x is not None]))} points), upload + score + copy {1e3 * (t3 - t2):.1f} ms")
    print("quality on the synthetic disc:", SG.evaluate(m["segmentation"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "fit":
        fit(*(int(v) for v in sys.argv[2:4]))
    else:
        kernel()
