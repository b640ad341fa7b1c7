"""The forward-backward occlusion check of include/gflow_hip.h ("occlusion masks from the flows") restated in float64
numpy, with an explicit floor and gather -- what tests/test_occlusion_host.py ties to torch's grid_sample and
tests/test_gpu_occlusion.py compares gfl_flow_occlusion with."""
import numpy as np

FLOW_MAX = 2.0 ** 20


def sample(img, flow):
    """S(img, x + flow.x, y + flow.y) for every pixel: img, flow (H, W, 2) float64.  Bilinear with the weights of the
    flow's own fraction; a corner outside the image contributes zero, a corner inside always enters the sum (0 * NaN is
    NaN); a flow component that is not of magnitude < 2^20 puts every corner outside."""
    H, W = flow.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        near = (np.abs(flow[..., 0]) < FLOW_MAX) & (np.abs(flow[..., 1]) < FLOW_MAX)
        f = np.where(near[..., None], flow, 0.0)
        fl = np.floor(f)
        t = f - fl
        x0, y0 = xx + fl[..., 0].astype(np.int64), yy + fl[..., 1].astype(np.int64)
        out = np.zeros((H, W, 2))
        for dy in (0, 1):
            for dx in (0, 1):
                xc, yc = x0 + dx, y0 + dy
                inside = near & (xc >= 0) & (xc < W) & (yc >= 0) & (yc < H)
                w = (t[..., 0] if dx else 1.0 - t[..., 0]) * (t[..., 1] if dy else 1.0 - t[..., 1])
                v = img[np.clip(yc, 0, H - 1), np.clip(xc, 0, W - 1)]
                out += np.where(inside[..., None], w[..., None] * v, 0.0)
    return out


def _norm(v):
    """(|v| in float64, whether the float32 evaluation sqrt(x x + y y) stays finite)"""
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])
        x, y = v[..., 0].astype(np.float32), v[..., 1].astype(np.float32)
        ok = np.isfinite(x * x + y * y)
    return n, ok


def flow_occlusion(fwd, bwd, alpha=0.01, beta=0.5):
    """fwd, bwd (H, W, 2) -> dict(diff, diff_bwd, thr (H, W) float64; known, known_bwd (H, W) bool; occ, occ_bwd (H, W)
    uint8 0 / 255).  The arithmetic is float64; a pixel is UNKNOWN (difference 0, mask 0) where the difference or the
    threshold is not finite in the header's float32 evaluation (a norm overflows from a component of about 1.8e19 on)."""
    fwd, bwd = np.asarray(fwd, dtype=np.float64), np.asarray(bwd, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        na, ok_a = _norm(fwd)
        nb, ok_b = _norm(bwd)
        thr = alpha * (na + nb) + beta
        thr_ok = ok_a & ok_b & np.isfinite(thr.astype(np.float32))
        out = dict(thr=thr)
        for key, own, other in (("", fwd, bwd), ("_bwd", bwd, fwd)):
            d, ok = _norm(own + sample(other, own))
            known = thr_ok & ok & np.isfinite(d)
            out["known" + key] = known
            out["diff" + key] = np.where(known, d, 0.0)
            out["occ" + key] = np.where(known & (d > thr), 255, 0).astype(np.uint8)
    return out


def flow_occlusion_grid_sample(fwd, bwd, alpha=0.01, beta=0.5):
    """The same check the way the original states it: torch.nn.functional.grid_sample(mode="bilinear",
    padding_mode="zeros", align_corners=True) of the other flow at the normalised x + flow, in float64.  (diff, diff_bwd,
    thr); finite flows only."""
    import torch
    import torch.nn.functional as F
    fwd, bwd = (torch.tensor(np.asarray(f), dtype=torch.float64) for f in (fwd, bwd))
    H, W = fwd.shape[:2]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")

    def warp(img, flow):
        gx = 2.0 * (xx + flow[..., 0]) / (W - 1) - 1.0
        gy = 2.0 * (yy + flow[..., 1]) / (H - 1) - 1.0
        grid = torch.stack([gx, gy], dim=-1).unsqueeze(0)
        s = F.grid_sample(img.permute(2, 0, 1).unsqueeze(0), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        return s[0].permute(1, 2, 0)

    thr = alpha * (torch.linalg.norm(fwd, dim=-1) + torch.linalg.norm(bwd, dim=-1)) + beta
    d_f = torch.linalg.norm(fwd + warp(bwd, fwd), dim=-1)
    d_b = torch.linalg.norm(bwd + warp(fwd, bwd), dim=-1)
    return d_f.numpy(), d_b.numpy(), thr.numpy()
