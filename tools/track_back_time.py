"""What backward point tracking costs ("Point tracking"):
   python tools/track_back_time.py     gfl_track_history on one frame (480x854, 60 000 fit records of stride 12) and
                                       gfl_track_backward at the end of a clip (256 queries spread over 60 frames whose rows
                                       grow from 60 000 to 100 000) into buffers allocated once: HIP events around 20 calls
                                       back to back on an idle stream, per call; median [min, max] of 9 such groups after 2
                                       warm-ups"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import _lib as L  # noqa: E402

dev = torch.device("cuda", 0)


def timed(run, calls=20, groups=9, warm=2):
    us = []
    for g in range(warm + groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(calls):
            run()
        b.record()
        torch.cuda.synchronize()
        if g >= warm:
            us.append(a.elapsed_time(b) / calls * 1e3)
    us = np.array(us)
    return f"{np.median(us):.1f} us [{us.min():.1f}, {us.max():.1f}] per call"


def history(N=60000, H=480, W=854):
    lib = L.load()
    g = torch.Generator(device=dev).manual_seed(0)
    rec = torch.rand(N, 12, device=dev, generator=g) * torch.tensor([float(W), float(H)] + [1.0] * 10, device=dev)
    dm = torch.rand(H, W, device=dev, generator=g)
    h_uv = torch.empty(N, 2, device=dev)
    h_occ = torch.empty(N, dtype=torch.uint8, device=dev)
    run = lambda: L.check(lib.gfl_track_history(L.ptr(rec), 12, L.ptr(rec[:, 9]), 12, N, L.ptr(dm), W, H, 0.05, L.ptr(h_uv),
                                                L.ptr(h_occ), L.stream()), "track history")
    print(f"gfl_track_history {N} rows {H}x{W}: {timed(run)}, occluded {float((h_occ != 0).float().mean()):.4f}")


def backward(Q=256, T=60, N0=60000, N1=100000, H=480, W=854):
    lib = L.load()
    g = torch.Generator(device=dev).manual_seed(0)
    counts = np.linspace(N0, N1, T).astype(np.int64)
    total = int(counts.sum())
    hist_uv = torch.rand(total, 2, device=dev, generator=g) * torch.tensor([float(W), float(H)], device=dev)
    hist_occ = (torch.rand(total, device=dev, generator=g) < 0.3).to(torch.uint8)
    row_start = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])).to(dev)
    xy = torch.rand(Q, 2, device=dev, generator=g, dtype=torch.float64) * torch.tensor([float(W), float(H)], device=dev)
    qf = torch.sort(torch.randint(0, T, (Q,), device=dev, generator=g).int()).values
    tracks = torch.zeros(Q, T, 2, device=dev)
    occ = torch.zeros(Q, T, dtype=torch.uint8, device=dev)
    back = torch.zeros(Q, T, dtype=torch.int32, device=dev)
    ws = L.scratch(lib.gfl_track_backward_workspace_bytes(Q, T), dev)
    run = lambda: L.check(lib.gfl_track_backward(L.ptr(hist_uv), L.ptr(hist_occ), L.ptr(row_start), T, L.ptr(xy), L.ptr(qf), Q,
                                                 L.ptr(tracks), L.ptr(occ), L.ptr(back), L.ptr(ws), ws.numel(), L.stream()),
                          "track backward")
    print(f"gfl_track_backward {Q} queries, {T} frames of {N0}..{N1} rows ({total * 9 / 1e6:.0f} MB of history, "
          f"{ws.numel() / 1e6:.0f} MB of workspace): {timed(run)}")


if __name__ == "__main__":
    history()
    backward()
