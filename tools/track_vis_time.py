"""What one track-overlay call costs ("Track overlays"): 480 x 854, T = 60, N = 300 random walks of at
most 6 px a step, 30 % of the points occluded.

    python tools/track_vis_time.py device     # HIP events around gfl_track_vis and around draw_tracks (needs the GPU)
    python tools/track_vis_time.py pil        # the PIL painter of tests/track_vis_ref.py on the same input, and the pairs

Each prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
H, W, T, N, STILL = 480, 854, 60, 300, 120


def scene():
    rng = np.random.default_rng(11)
    start = rng.uniform([8, 8], [W - 8, H - 8], (N, 2))
    steps = rng.uniform(-6, 6, (T, N, 2))
    steps[0] = 0
    tracks = (start[None] + np.cumsum(steps, axis=0)).astype(np.float32)
    occluded = rng.random((T, N)) < 0.3
    video = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    return video, tracks, occluded


def device():
    import torch
    from gflow_amd import _lib as L
    from gflow_amd import color
    from gflow_amd import track_vis as TV
    video, tracks, occluded = scene()
    dev = torch.device("cuda", 0)
    v, t = torch.from_numpy(video).to(dev), torch.from_numpy(tracks).to(dev)
    o = torch.from_numpy(occluded).to(dev).to(torch.uint8)
    k_cap = TV.default_k_cap(T, N, W, H)
    lib = L.load()
    ws = L.scratch(lib.gfl_track_vis_workspace_bytes(T, N, W, H, k_cap), dev)
    out, ovf, lut = torch.empty_like(v), torch.zeros(1, dtype=torch.int32, device=dev), color.lut("gist_rainbow", dev)

    def call():
        L.check(lib.gfl_track_vis(L.ptr(v), L.ptr(t), L.ptr(o), T, N, W, H, STILL, L.ptr(lut), k_cap, L.ptr(out), L.ptr(ovf),
                                  L.ptr(ws), ws.numel(), L.stream()), "track vis")

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
        call()
        TV.draw_tracks(v, t, o, still_length=STILL)
    torch.cuda.synchronize()
    print(json.dumps(dict(H=H, W=W, T=T, N=N, k_cap=k_cap, lib_call_ms=timed(call, 10),
                          draw_tracks_ms=timed(lambda: TV.draw_tracks(v, t, o, still_length=STILL), 10), overflow=int(ovf.item()))))


def pil():
    from tests import track_vis_ref as TR
    video, tracks, occluded = scene()
    pairs = TR.pairs_per_tile(tracks, W, H)
    t0 = time.perf_counter()
    TR.pil_paint(video, tracks, occluded, STILL)
    print(json.dumps(dict(H=H, W=W, T=T, N=N, pil_paint_s=time.perf_counter() - t0, pairs_needed=int(pairs.sum()),
                          pairs_in_the_fullest_tile=int(pairs.max()))))


if __name__ == "__main__":
    {"device": device, "pil": pil}[sys.argv[1] if len(sys.argv) > 1 else "device"]()
