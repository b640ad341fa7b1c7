"""What an in-between image costs ("Layers, edits and in-between frames"):
   python tools/compose_time.py [T [K]]
A log folder of T (default 6) checkpoints of the bench scene (480 x 854, 60 000 grown splats of synthetic.init_splats, seed 0;
every frame the moving third of the rows a little further along, the last frame 2 000 rows longer) is written to a temporary
directory and opened as a ViewerSession.  Three numbers, each the median [min, max] of ``groups`` windows of four back-to-back calls after
``warm`` warm-up windows, the variants alternating (and the host time to enqueue one call, no synchronise inside):
   images/s of play_at(slowmo(T, K)) (default K = 4): the composer in front of the batched rasteriser;
   images/s of play(follow): the batched rasteriser on the checkpoints' own rows;
   the composer's share of the play_at call: device events around gfl_compose_rows alone, on the same job tables."""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import _lib as L  # noqa: E402
from gflow_amd import render as R  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402
from gflow_amd import viewer as V  # noqa: E402

dev = torch.device("cuda", 0)
H, W, N = 480, 854, 60000


def write_clip(folder, T):
    frame = S.make_frame(H, W, seed=0)
    raw = S.init_splats(frame, N + 2000, seed=0, grown=True)
    still = (torch.arange(N + 2000) % 3) != 1
    os.makedirs(os.path.join(folder, "ckpt"))
    for t in range(T):
        n = N + 2000 if t == T - 1 else N
        attrs = {k: raw[k][:n].detach().float().cpu().clone() for k in ("xyz", "scale", "rotate", "opacity", "rgb")}
        attrs["xyz"] += 0.004 * t * (~still[:n]).float().unsqueeze(1) * torch.tensor([[1.0, 0.0, 0.0]])
        extr = raw["extr"].float().cpu().clone()
        extr[0, 3] += 0.002 * t
        torch.save({"attributes": attrs, "intr": raw["intr"].float().cpu(), "extr": extr, "still_mask": still[:N].clone(),
                    "move_seg": None, "last_uv": None, "width": W, "height": H}, os.path.join(folder, "ckpt", f"frame_{t:04d}.tar"))


def window(fn, calls=4):
    """(device ms per call between events around ``calls`` back-to-back repetitions, host ms per call to enqueue one)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls, 1e3 * host / calls


def main(T=6, K=4, groups=9, warm=2):
    with tempfile.TemporaryDirectory() as folder:
        write_clip(folder, T)
        session = V.ViewerSession(folder, dev)
    taus = V.slowmo(T, K)
    follow = V.follow(session.extrs)
    # the composer alone, on play_at's own job tables
    lib = L.load()
    src = torch.tensor([session.ranges[a] + session.ranges[b] for a, b, _ in (V.split_time(t, T) for t in taus)], dtype=torch.int32).to(dev)
    s = torch.tensor([V.split_time(t, T)[2] for t in taus], dtype=torch.float32).to(dev)
    J, rows_max = len(taus), session.rows_max
    out_rows = torch.empty(J * rows_max, 16, device=dev)
    job_rows = torch.empty(J, 2, dtype=torch.int32, device=dev)
    flags = torch.empty(J, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.gfl_compose_rows_workspace_bytes(J, rows_max), dtype=torch.uint8, device=dev)

    def composer():
        L.check(lib.gfl_compose_rows(L.ptr(session.block), L.ptr(session.labels), session.block.shape[0], L.ptr(src), L.ptr(s), None, 1,
                                     J, rows_max, L.ptr(out_rows), L.ptr(job_rows), L.ptr(flags), L.ptr(ws), ws.numel(), L.stream()),
                "compose_rows")
    variants = {"play_at": (lambda: session.play_at(taus), J), "play": (lambda: session.play(follow), T), "composer": (composer, J)}
    ms, host = {k: [] for k in variants}, {k: [] for k in variants}
    for g in range(warm + groups):
        for name, (fn, _) in variants.items():
            d, h = window(fn)
            if g >= warm:
                ms[name].append(d)
                host[name].append(h)
    R.check_overflow()
    assert int(flags.max()) == 0
    for name, (_, n) in variants.items():
        d = np.array(ms[name])
        print(f"{name:9s} {n:3d} images  {np.median(d):8.3f} ms per call [{d.min():.3f}, {d.max():.3f}]  "
              f"{1e3 * n / np.median(d):8.0f} images/s [{1e3 * n / d.max():.0f}, {1e3 * n / d.min():.0f}]  "
              f"host enqueue {np.median(host[name]):.3f} ms per call")
    rows = int(job_rows[:, 1].sum())
    med = float(np.median(ms["composer"]))
    print(f"composer: {100 * med / np.median(ms['play_at']):.1f} % of the play_at call; {rows} rows kept of {J} jobs, "
          f"{rows * 64 * 3 / med / 1e6:.0f} GB/s of the 64 B read twice and written once per row")


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:3]])
