"""What the reconstruction and camera scores cost, and what the camera score says:
   python tools/recon_time.py kernel          gfl_recon_frame at 480x854: device events around 200 calls, and the same score
                                              written with torch float64 ops (F.conv2d), timed the same way.  Under
                                              `rocprofv3 --kernel-trace --stats -- python tools/recon_time.py kernel` the
                                              kernels' own times (recon_tile_kernel, recon_fold_kernel)
   python tools/recon_time.py fit [runs] [T]  a T-frame 480p / 60 k clip fit without / with recon=True, camera=True,
                                              alternating in one process (medians)
   python tools/recon_time.py camera [T]      ATE / RPE_t / RPE_r (and PSNR / SSIM) of a T-frame synthetic clip fit"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import fit_video as FV  # noqa: E402
from gflow_amd import quality as QL  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402

dev = torch.device("cuda", 0)
CONV2D = True


def torch_score(render, gt, win2):
    """the same two sums with torch float64 ops"""
    x = (torch.clamp(render[:3], 0.0, 1.0) * 255.0).to(torch.uint8).float().div(255.0).double()
    y = torch.clamp(gt.permute(2, 0, 1), 0.0, 1.0).double()
    sse = ((x - y) ** 2).sum()
    maps = torch.stack([x, y, x * x, y * y, x * y], dim=1).reshape(15, 1, *x.shape[1:])
    if CONV2D:
        f = F.conv2d(maps, win2)
    else:                                                # (no float64 convolution in this build: the window as two matmuls)
        w1 = win2[0, 0].sum(dim=0)
        f = (maps.unfold(3, 11, 1) @ w1).unfold(2, 11, 1) @ w1
    f = f.reshape(3, 5, x.shape[1] - 10, x.shape[2] - 10)
    mx, my = f[:, 0], f[:, 1]
    sxx, syy, sxy = f[:, 2] - mx * mx, f[:, 3] - my * my, f[:, 4] - mx * my
    ss = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    return torch.stack([sse, ss.sum()])


def timed(run, reps):
    for _ in range(10):
        run()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def kernel(H=480, W=854, reps=200):
    g = torch.Generator(device=dev).manual_seed(0)
    render = torch.rand(4, H, W, device=dev, generator=g) * 1.2 - 0.1
    gt = (render[:3].permute(1, 2, 0) + 0.05 * torch.randn(H, W, 3, device=dev, generator=g)).contiguous()
    rec = QL.ReconRecorder(1, H, W, dev)
    i = torch.arange(11, dtype=torch.float64, device=dev) - 5
    w1 = torch.exp(-i ** 2 / 4.5)
    w1 = w1 / w1.sum()
    win2 = torch.outer(w1, w1).reshape(1, 1, 11, 11)
    global CONV2D
    try:
        torch_score(render, gt, win2)
    except RuntimeError as e:
        print("F.conv2d in float64 failed here, timing unfold + matmul instead:", str(e).splitlines()[0])
        CONV2D = False
    us_hip = timed(lambda: rec.frame(0, render, gt), reps)
    us_torch = timed(lambda: torch_score(render, gt, win2), reps)
    a, b = rec.result(), torch_score(render, gt, win2).cpu().numpy()
    how = "F.conv2d" if CONV2D else "unfold + matmul"
    print(f"gfl_recon_frame {H}x{W}: {us_hip:.1f} us per call (two launches, device events); torch float64 ops ({how}): "
          f"{us_torch:.1f} us per call; sse {a['sse'][0]!r} / {b[0]!r}, ssim_sum {a['ssim_sum'][0]!r} / {b[1]!r}")


def fit(runs=3, T=8):
    frames = FV.upload_clip(S.make_clip(T, 480, 854, seed=0), dev)
    cfg = dict(num_points=60000)
    FV.fit_clip(frames[:2], dev, cfg, seed=0, snapshot_interval=10, recon=True, camera=True)
    walls = {False: [], True: []}
    for r in range(runs):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            FV.fit_clip(frames, dev, cfg, seed=0, snapshot_interval=10, recon=on, camera=on)
            torch.cuda.synchronize()
            walls[on].append(time.perf_counter() - t0)
    med = {on: float(np.median(w)) for on, w in walls.items()}
    for on, w in walls.items():
        print(f"recon+camera={on}: median {med[on]:.4f} s ({T / med[on]:.2f} frames/s)  min {min(w):.4f} s  all {np.round(w, 4)}")
    print(f"cost: {100.0 * (med[True] / med[False] - 1.0):+.2f} % of the fit's wall time")


def camera(T=60):
    frames = FV.upload_clip(S.make_clip(T, 480, 854, seed=0), dev)
    m = FV.fit_clip(frames, dev, dict(num_points=60000), seed=0, snapshot_interval=10, recon=True, camera=True)
    print(f"{T}-frame synthetic clip:", {k: m["camera"][k] for k in ("ATE", "RPE_t", "RPE_r")}, QL.evaluate(m["recon"]),
          f"psnr_mean_db {m['psnr_sum'] / T:.3f}")
    gt = np.stack([fr["extr_gt"].cpu().numpy() for fr in frames])
    print("camera travel (ground truth):", float(np.linalg.norm(gt[-1, :, 3] - gt[0, :, 3])), "estimated:",
          float(np.linalg.norm(m["camera"]["extr"][-1, :, 3] - m["camera"]["extr"][0, :, 3])))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if mode == "fit":
        fit(*(int(v) for v in sys.argv[2:4]))
    elif mode == "camera":
        camera(*(int(v) for v in sys.argv[2:3]))
    else:
        kernel()
