"""What asking for the intrinsics gradient costs: render() forward + backward at 480 x 854 / 60 000 splats with and without
``intr.requires_grad``, timed the way tools/op_time.py times the drop-in levels ("Differentiable intrinsics").
Alternates the two a few times so that a drift of the device's clocks shows up as spread and not as a difference."""
import os, sys, time, torch
sys.path.insert(0, os.getcwd())
import gflow_amd.render as R
from gflow_amd import synthetic as S
DEV = torch.device("cuda", 0)
H, W, N = 480, 854, 60000
frame = S.make_frame(H, W, seed=0)
raw = S.init_splats(frame, N, seed=0, grown=True)
act = dict(xyz=raw["xyz"], scale=raw["scale"].abs(), rotate=torch.nn.functional.normalize(raw["rotate"]),
           opacity=torch.sigmoid(10 * raw["opacity"]), rgb=torch.sigmoid(raw["rgb"]))
leaves = {k: v.to(DEV).requires_grad_(True) for k, v in act.items()}
extr = raw["extr"].to(DEV).requires_grad_(True)
intr_plain = raw["intr"].to(DEV)
intr_asked = raw["intr"].to(DEV).requires_grad_(True)
grad = ((torch.rand(3, H, W, device=DEV) - 0.5) / (H * W)).contiguous()
def both(intr):
    out = R.render(leaves, dict(intr=intr, extr=extr, W=W, H=H), 0.0)
    out["rgb"].backward(grad)
def timed(fn, n=200):
    for _ in range(20): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n
rows = []
for _ in range(5):
    rows.append((timed(lambda: both(intr_plain)) * 1e3, timed(lambda: both(intr_asked)) * 1e3))
for a, b in rows:
    print("fwd+bwd without d_intr %.4f ms   with d_intr %.4f ms" % (a, b))
med = lambda v: sorted(v)[len(v) // 2]
print("median: without %.4f ms, with %.4f ms" % (med([a for a, _ in rows]), med([b for _, b in rows])))
assert intr_asked.grad is not None and intr_asked.grad.shape == (4,) and intr_plain.grad is None
