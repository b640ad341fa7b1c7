"""What the occlusion check costs ("Occlusion kernel"):
   python tools/occ_time.py [pairs ...]     gfl_flow_occlusion at 480x854 on the tests' scene into outputs allocated once, all
                                            four outputs and the masks alone: HIP events around 20 calls back to back on an
                                            idle stream, per call; median [min, max] of 9 such groups after 2 warm-ups"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gflow_amd import _lib as L  # noqa: E402
from tests.test_occlusion_host import make_scene  # noqa: E402

dev = torch.device("cuda", 0)


def kernel(pairs=1, H=480, W=854, calls=20, groups=9, warm=2):
    scenes = [make_scene(H, W, seed) for seed in range(min(pairs, 4))]
    fwd = torch.stack([torch.tensor(scenes[p % len(scenes)][0]) for p in range(pairs)]).to(dev)
    bwd = torch.stack([torch.tensor(scenes[p % len(scenes)][1]) for p in range(pairs)]).to(dev)
    diff = [torch.empty(pairs, H, W, dtype=torch.float32, device=dev) for _ in range(2)]
    occ = [torch.empty(pairs, H, W, dtype=torch.uint8, device=dev) for _ in range(2)]
    lib = L.load()
    for maps in (True, False):
        d = diff if maps else [None, None]
        run = lambda: L.check(lib.gfl_flow_occlusion(L.ptr(fwd), L.ptr(bwd), pairs, W, H, 0.01, 0.5, L.ptr(d[0]), L.ptr(d[1]),
                                                     L.ptr(occ[0]), L.ptr(occ[1]), L.stream()), "flow occlusion")
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
        moved = pairs * H * W * (2 * 8 + (2 * 4 if maps else 0) + 2)                # flows read once, outputs written
        print(f"gfl_flow_occlusion {pairs} pair(s) {H}x{W} {'maps + masks' if maps else 'masks'}: {np.median(us):.1f} us "
              f"[{us.min():.1f}, {us.max():.1f}] per call ({moved / 1e6:.1f} MB: {moved / np.median(us) / 1e3:.0f} GB/s), "
              f"occluded {float((occ[1] != 0).float().mean()):.4f}")


if __name__ == "__main__":
    for p in ([int(v) for v in sys.argv[1:]] or [1, 59]):
        kernel(p)
