"""What depth and camera from the flows cost ("Depth and camera kernels"):
   python tools/sfm_time.py [frames [H W [repeats]]]   the stages of gflow_amd.sfm on the synthetic clip's flows (default 60 frames at
                                                      480x854: 118 pair problems; the backward flows are the negated forward ones,
                                                      which is enough for a clock): HIP events around each stage, after a warm-up
                                                      call, 5 repeats; min and median.  Gated nowhere.  GFLOW_HIP_LIB picks another
                                                      build."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import sfm  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402

dev = torch.device("cuda", 0)


def timed(name, fn, repeats):
    ms = []
    for r in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 1:
            ms.append(e0.elapsed_time(e1))
    print(f"{name}: min {min(ms):.1f} ms, median {np.median(ms):.1f} ms", flush=True)
    return out


def main(frames=60, H=480, W=854, repeats=5):
    clip = S.make_clip(frames, H, W, seed=0, device=dev)
    fwd = torch.stack([fr["flow"].float() for fr in clip[:-1]])
    focal, pp = float(clip[0]["focal"]), clip[0]["pp"]
    del clip
    bwd = -fwd
    flows = torch.cat([fwd, bwd])
    n = frames - 1
    intr = (focal, focal, float(pp[0]), float(pp[1]))
    print(f"{flows.shape[0]} pair problems {H}x{W}")
    F0 = timed("initial F (gfl_epi_fundamental per pair, 256 hypotheses)", lambda: sfm.initial_F(flows), repeats)
    tv = timed("refit + pose + triangulation", lambda: sfm.two_view(flows, intr, F_init=F0), repeats)
    rf, wf, rb, wb = sfm._frame_stacks(tv, n)
    timed("baseline ratios", lambda: sfm.masked_median(rf, rb, wf, wb, 1e-7), repeats)
    one = torch.ones(frames, dtype=torch.float64, device=dev)
    timed("fusion, fill and 20 sweeps", lambda: sfm.fuse_fill(rf, wf, rb, wb, one, one), repeats)
    res = timed("clip_depth_camera, all of it with the read-back", lambda: sfm.clip_depth_camera(fwd, bwd, focal=focal, pp=pp), repeats)
    print("degenerate pairs", int(res["degenerate"].sum()), "unreliable frames", int(res["unreliable"].sum()))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:]])
