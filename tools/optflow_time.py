"""What the optical-flow estimate of a clip costs ("Optical flow"):
   python tools/optflow_time.py [frames [H W [repeats [plain]]]]   estimate_flow of the 2 (frames - 1) problems of the synthetic clip (default 60
                                                  frames at 480x854: 118 problems), defaults, with the sweeps fused and with
                                                  GFL_OPTFLOW_FUSED=0 (one launch per sweep): HIP events around one call, after
                                                  a warm-up call, 5 repeats; min and median.  GFLOW_HIP_LIB picks another build."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import optflow as OF  # noqa: E402
from gflow_amd import synthetic as S  # noqa: E402

dev = torch.device("cuda", 0)


def main(frames=60, H=480, W=854, repeats=5, plain=1):
    clip = S.make_clip(frames, H, W, seed=0, device=dev)
    images = torch.stack([(fr["image"].float().clamp(0, 1) * 255.0 + 0.5).to(torch.uint8) for fr in clip])
    truth = torch.stack([fr["flow"].float() for fr in clip[:-1]])
    del clip
    a, b = torch.cat([images[:-1], images[1:]]), torch.cat([images[1:], images[:-1]])
    results = {}
    for mode in ("fused", "one sweep per launch")[:1 + bool(plain)]:
        if mode == "fused":
            os.environ.pop("GFL_OPTFLOW_FUSED", None)
        else:
            os.environ["GFL_OPTFLOW_FUSED"] = "0"
        ms = []
        for r in range(repeats + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            flow = OF.estimate_flow(a, b)
            e1.record()
            torch.cuda.synchronize()
            if r >= 1:
                ms.append(e0.elapsed_time(e1))
        results[mode] = flow
        err = (flow[:frames - 1] - truth).norm(dim=-1).mean().item()
        print(f"estimate_flow {a.shape[0]} problems {H}x{W} {mode}: min {min(ms):.1f} ms, median {np.median(ms):.1f} ms "
              f"(forward EPE {err:.3f} px)", flush=True)
    os.environ.pop("GFL_OPTFLOW_FUSED", None)
    if plain:
        print("same bits:", torch.equal(results["fused"], results["one sweep per launch"]))


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:]])
