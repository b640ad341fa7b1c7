"""Cost of the deterministic mode (GFL_FIT_DETERMINISTIC): microseconds per fused iteration of each kind -- first frame
(10 sums per pair), camera-only stage (6), joint stage (7) -- in the default and the deterministic mode, on bench.py's
480x854 / 60 000-splat scene, replayed from captured graphs.  Prints one JSON line.

    python tools/det_cost.py [--iters 200]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/det_cost.py --iters 50    (per-kernel times of both modes)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = (("first_frame", dict(freeze_rgb=0, freeze_all_splats=0, lr_camera=0.0)),
         ("camera", dict(freeze_rgb=1, freeze_all_splats=1, lr_camera=1e-3)),
         ("joint", dict(freeze_rgb=1, freeze_all_splats=0, lr_camera=0.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--per-graph", type=int, default=4)
    args = ap.parse_args()
    from gflow_amd import synthetic as S
    from gflow_amd.fused import FitEngine
    H, W, N = 480, 854, 60000
    frame = S.make_frame(H, W, seed=0)
    raw = S.init_splats(frame, N, seed=0, grown=True)
    out = {}
    for det in (False, True):
        eng = FitEngine(W, H, 2 * N, "cuda", deterministic=det)
        eng.set_splats({k: raw[k].cuda() for k in ("xyz", "scale", "rotate", "opacity", "rgb")})
        eng.intr.copy_(raw["intr"].cuda())
        eng.set_targets(frame["image"], frame["depth"])
        eng.hp.lambda_depth, eng.hp.lambda_var, eng.hp.lr, eng.hp.total_iters = 0.1, 10.0, 1e-3, 0
        eng.reset_optimizer()
        for kind, hp in KINDS:
            for k, v in hp.items():
                setattr(eng.hp, k, v)
            saved = eng.save_state()
            for _ in range(3):
                eng.iteration(use_graph=True, count=args.per_graph)       # (captures, warms the schedule's feedback)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = max(1, args.iters // args.per_graph)
            t0.record()
            for _ in range(reps):
                eng.iteration(use_graph=True, count=args.per_graph)
            t1.record()
            torch.cuda.synchronize()
            out[f"{kind}_{'det' if det else 'default'}_us"] = round(1e3 * t0.elapsed_time(t1) / (reps * args.per_graph), 2)
            eng.restore_state(saved)
        eng.check_overflow()
    for kind, _ in KINDS:
        out[f"{kind}_ratio"] = round(out[f"{kind}_det_us"] / out[f"{kind}_default_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
