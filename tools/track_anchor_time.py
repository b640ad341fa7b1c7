"""gfl_track_anchor at Q_new = 4096 against N = 400 000 fit-record rows (stride 12), timed with events; run it under
``rocprofv3 --kernel-trace --stats -- python tools/track_anchor_time.py`` for the per-kernel split."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import _lib as L  # noqa: E402


def main(N=400000, Q=4096, reps=20):
    dev = "cuda"
    lib = L.load()
    g = torch.Generator(device=dev).manual_seed(0)
    rec = torch.rand(N, 12, device=dev, generator=g) * 500
    xy = torch.rand(Q, 2, device=dev, generator=g, dtype=torch.float64) * 500
    anchor = torch.empty(Q, dtype=torch.int32, device=dev)
    shift = torch.empty(Q, 2, dtype=torch.float64, device=dev)
    ws = L.scratch(lib.gfl_track_anchor_workspace_bytes(Q, N), dev)
    run = lambda: L.check(lib.gfl_track_anchor(L.ptr(rec), 12, N, L.ptr(xy), Q, L.ptr(anchor), L.ptr(shift), L.ptr(ws),
                                               ws.numel(), L.stream()), "track anchor")
    for _ in range(3):
        run()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    print(f"gfl_track_anchor Q={Q} N={N}: {a.elapsed_time(b) / reps:.3f} ms per call")


if __name__ == "__main__":
    main()
